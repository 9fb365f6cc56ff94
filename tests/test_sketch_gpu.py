"""GPU parity of kmc_sketch_from_counts and kmc_sketch_distances against the numpy
oracle of tests/sketch_util.py.  Every case runs in libkmc.so and in
libkmc_diag.so, whose small walk ranges (256 entries per workgroup, chunks of
64) and distance tiles (4 x 4 rows, 512 values of LDS) put a few hundred entries
through many workgroups, chunks and flushes and a few records through many tiles.

Sketch rows and sizes are compared bit for bit, tail fill included; shared and
denom exactly; distances within one float32 ulp (the device evaluates the formula
in double: two correct double logs differ by less than a double ulp, which moves
the rounded float by at most one ulp), the special values NaN, 1.0 and +0.0 bit
for bit.
"""

import numpy as np
import pytest

import golden_util as G
import sketch_util as S
from sketch_util import assert_sketch, dev, which

pytestmark = pytest.mark.gpu

LIBS = ["ship", "diag"]
cached = S.cache()
U64 = np.uint64


def dev_lists(keys, counts, off, cuda):
    """uint64 / uint32 host lists as the int64 / int32 tensors the binding takes."""
    return (dev(np.asarray(keys, dtype=np.uint64).view(np.int64), cuda),
            None if counts is None else dev(np.asarray(counts, dtype=np.uint32).view(np.int32), cuda),
            dev(np.asarray(off, dtype=np.uint64).view(np.int64), cuda))


def gpu_sketch(kmc, cuda, keys, counts, off, s, **kw):
    import torch
    dk, dc, do = dev_lists(keys, counts, off, cuda)
    sk, sz = kmc.sketch_from_counts(dk, dc, do, s, **kw)
    torch.cuda.synchronize()
    return sk.cpu().numpy().view(np.uint64), sz.cpu().numpy().view(np.uint32)


def lists_of(rng, sizes):
    """Random distinct 62-bit keys, sizes[r] of them in record r, shuffled."""
    total = int(np.sum(sizes))
    keys = np.unique(rng.integers(0, 1 << 62, size=total + total // 8 + 16, dtype=np.uint64))
    keys = rng.permutation(keys)[:total]
    assert keys.size == total
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return keys, off


# 1. record shapes -----------------------------------------------------------------
def shapes_case(s):
    def make():
        rng = np.random.default_rng(100 + s)
        sizes = [0, 1, max(s - 1, 0), s, s + 1, 5 * s + 3, 40000, 0, 7]
        keys, off = lists_of(rng, sizes)
        return keys, off, S.sketch_expected(keys, None, off, len(sizes), s)
    return cached(("shapes", s), make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("s", [1, 2, 1000, 16384])
def test_sketch_record_shapes(kmc, cuda, lib, s):
    keys, off, exp = shapes_case(s)
    with which(kmc, lib):
        assert_sketch(gpu_sketch(kmc, cuda, keys, None, off, s), exp, "s=%d" % s)


# 2. many tiny records ---------------------------------------------------------------
def tiny_case():
    def make():
        rng = np.random.default_rng(2)
        sizes = list(rng.integers(0, 41, size=150)) + [40000] + list(rng.integers(0, 41, size=150))
        keys, off = lists_of(rng, sizes)
        counts = rng.integers(1, 4, size=keys.size).astype(np.uint32)
        return keys, counts, off, len(sizes)
    return cached("tiny", make)


@pytest.mark.parametrize("lib", LIBS)
def test_sketch_many_tiny_records(kmc, cuda, lib):
    keys, counts, off, n = tiny_case()
    exp = cached("tiny16", lambda: S.sketch_expected(keys, None, off, n, 16))
    with which(kmc, lib):
        assert_sketch(gpu_sketch(kmc, cuda, keys, counts, off, 16), exp)


# 3. every digit level decides -------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("b", range(8))
def test_sketch_every_byte_position_decides(kmc, cuda, lib, b):
    """Record 0: 40 hashes that agree above byte b and differ in byte b (s = 8, so
    the select has to descend to that byte); record 1: unrelated keys; record 2:
    hashes that include 0 and UINT64_MAX."""
    rng = np.random.default_rng(30 + b)
    seed, s = 42, 8
    base = int(rng.integers(0, 1 << 62)) | (1 << 63)
    hi_mask = ((1 << 64) - 1) ^ ((1 << (8 * (b + 1))) - 1)
    digits = rng.permutation(256)[:40]
    low = rng.integers(0, 1 << 62, size=40, dtype=np.uint64) & U64((1 << (8 * b)) - 1)
    h0 = (U64(base & hi_mask) | (digits.astype(np.uint64) << U64(8 * b)) | low).astype(np.uint64)
    assert np.unique(h0 >> U64(8 * b)).size == 40
    h2 = np.array([0, (1 << 64) - 1, 5, 1 << 63], dtype=np.uint64)
    other = rng.integers(0, 1 << 62, size=300, dtype=np.uint64)
    for extra in (np.zeros(0, np.uint64), rng.integers(0, 1 << 64, size=20, dtype=np.uint64)):
        r2 = np.unique(np.concatenate([h2, extra]))
        keys = np.concatenate([rng.permutation(S.unhash(h0, seed)), np.unique(other),
                               rng.permutation(S.unhash(r2, seed))])
        off = np.cumsum([0, 40, np.unique(other).size, r2.size]).astype(np.uint64)
        exp = S.sketch_expected(keys, None, off, 3, s, seed)
        np.testing.assert_array_equal(exp[0][0], np.sort(h0)[:s])
        assert exp[0][2][0] == 0 and (r2.size > s or exp[0][2][r2.size - 1] == S.FILL)
        with which(kmc, lib):
            assert_sketch(gpu_sketch(kmc, cuda, keys, None, off, s, seed=seed), exp, "byte %d" % b)


# 4. min_count -----------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("min_count", [0, 1, 2, 4])
def test_sketch_min_count(kmc, cuda, lib, min_count):
    keys, counts, off, n = tiny_case()
    exp = S.sketch_expected(keys, counts, off, n, 16, min_count=min_count)
    if min_count == 4:
        assert not exp[1].any() and (exp[0] == S.FILL).all()
    if min_count == 2:
        assert 0 < exp[1].sum() < S.sketch_expected(keys, counts, off, n, 16)[1].sum()
    with which(kmc, lib):
        assert_sketch(gpu_sketch(kmc, cuda, keys, counts, off, 16, min_count=min_count), exp)
        if min_count <= 1:  # counts may be NULL
            assert_sketch(gpu_sketch(kmc, cuda, keys, None, off, 16, min_count=min_count), exp)


# 5. seeds ---------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_sketch_seeds(kmc, cuda, lib):
    keys, counts, off, n = tiny_case()
    got = {}
    with which(kmc, lib):
        for seed in (42, 0xDEADBEEFCAFEF00D):
            got[seed] = gpu_sketch(kmc, cuda, keys, None, off, 16, seed=seed)
            assert_sketch(got[seed], S.sketch_expected(keys, None, off, n, 16, seed), "seed %x" % seed)
    a, b = got.values()
    assert (a[0] != b[0]).any()


# 6. clamping ------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_sketch_offsets_beyond_num_entries_are_clamped(kmc, cuda, lib):
    """rec_offsets[n] and the inner offset before it lie above num_entries; keys and
    counts are exactly num_entries long.  The result is the oracle's on the clamped
    offsets: the record before last runs to num_entries, the last one is empty."""
    rng = np.random.default_rng(6)
    sizes = [30, 0, 500, 3, 9000, 70, 11]
    keys, off = lists_of(rng, sizes)
    counts = rng.integers(1, 4, size=keys.size).astype(np.uint32)
    n = len(sizes)
    cut = int(off[n - 2]) + 20  # inside the record before last
    off = off.copy()
    off[n - 1] = keys.size + 1000
    off[n] = keys.size + (1 << 40)
    keys, counts = keys[:cut].copy(), counts[:cut].copy()
    exp = S.sketch_expected(keys, counts, off, n, 16, min_count=2)
    assert exp[1][n - 1] == 0 and exp[1][n - 2] > 0
    with which(kmc, lib):
        assert_sketch(gpu_sketch(kmc, cuda, keys, counts, off, 16, min_count=2), exp)


# 7. caller workspace ----------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_sketch_caller_workspace(kmc, cuda, lib):
    import torch
    keys, counts, off, n = tiny_case()
    dk, dc, do = dev_lists(keys, counts, off, cuda)
    with which(kmc, lib):
        need = kmc.sketch_workspace_size(n, keys.size, 16, cuda.index or 0)
        assert need > 0
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
        own = kmc.sketch_from_counts(dk, dc, do, 16)
        for _ in range(2):  # the second call finds the first one's state in the workspace
            got = kmc.sketch_from_counts(dk, dc, do, 16, workspace=ws)
            torch.cuda.synchronize()
            assert torch.equal(got[0], own[0]) and torch.equal(got[1], own[1])
        with pytest.raises(kmc.KmcError) as ei:
            kmc.sketch_from_counts(dk, dc, do, 16, workspace=ws[: need - 1])
        assert ei.value.code == 1004
    exp = cached("tiny16", lambda: S.sketch_expected(keys, None, off, n, 16))
    assert_sketch((own[0].cpu().numpy().view(np.uint64), own[1].cpu().numpy().view(np.uint32)), exp)


# 8. distance counts and floats ------------------------------------------------------
def dist_rows(n, s):
    """Rows with controlled overlap from one pool of sorted random values: a full
    row, a row sharing exactly one of the s smallest of their union with it
    (shared/denom = 1/s: past the cap at k = 3, s = 1000), an identical copy
    (d = +0), two empty rows (NaN), a short row disjoint from all others (d = 1),
    then random subsets of random size 0..s."""
    def make():
        rng = np.random.default_rng(8000 + 31 * n + s)
        pool = np.unique(rng.integers(1, (1 << 64) - 1, size=5 * s + 64, dtype=np.uint64))
        pool = pool[:5 * s + 8]
        full = pool[:s]
        one = np.concatenate([pool[:1], pool[s:2 * s - 1]])
        special = [full, one, full.copy(), pool[:0], pool[:0], pool[4 * s:4 * s + max(s // 2, 1)]]
        rows = np.full((n, s), S.FILL, dtype=np.uint64)
        sizes = np.zeros(n, dtype=np.uint32)
        for r in range(n):
            if r < len(special):
                v = special[r]
            else:
                m = int(rng.integers(0, s + 1)) if r % 3 else s
                v = np.sort(rng.choice(pool[:3 * s], size=m, replace=False))
            rows[r, :v.size] = v
            sizes[r] = v.size
        return rows, sizes
    return cached(("rows", n, s), make)


def assert_distances(got, exp, msg=""):
    (out, sh, dn), (eout, esh, edn) = got, exp
    if sh is not None:
        np.testing.assert_array_equal(sh, esh, err_msg="%s shared" % msg)
        np.testing.assert_array_equal(dn, edn, err_msg="%s denom" % msg)
    assert out.shape == eout.shape, msg
    special = np.isnan(eout) | (eout == 1.0) | (eout == 0.0)
    gb, eb = out.view(np.uint32).astype(np.int64), eout.view(np.uint32).astype(np.int64)
    assert (gb[special] == eb[special]).all(), "%s: special values differ" % msg
    ulp = np.abs(gb[~special] - eb[~special])  # positive finite floats: bit patterns are ordered
    print("%s: %d pairs, %d special, max ulp %d" % (msg, out.size, int(special.sum()), int(ulp.max(initial=0))))
    assert (ulp <= 1).all(), "%s: max %d ulp" % (msg, int(ulp.max()))


def gpu_distances(kmc, cuda, rows, sizes, k, with_counts):
    import torch
    r = kmc.sketch_distances(dev(rows.view(np.int64), cuda), dev(sizes.view(np.int32), cuda), k,
                             with_counts=with_counts)
    torch.cuda.synchronize()
    if with_counts:
        return r[0].cpu().numpy(), r[1].cpu().numpy().view(np.uint32), r[2].cpu().numpy().view(np.uint32)
    return r.cpu().numpy(), None, None


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("n,s,k", [(2, 16, 21), (3, 16, 21), (65, 16, 21), (130, 16, 21),
                                   (5, 1, 3), (5, 1000, 3), (5, 16384, 3),
                                   # diag tile edge 4: one full tile, one row past it, three ragged tile rows
                                   (4, 64, 21), (5, 64, 21), (9, 64, 21)])
def test_sketch_distance_counts_and_floats(kmc, cuda, lib, n, s, k):
    rows, sizes = dist_rows(n, s)
    exp = cached(("dist", n, s, k), lambda: S.distances_expected(rows, sizes, s, k))
    eout, esh, edn = exp
    if s > 1:
        assert esh[0] == 1 and edn[0] == s  # (full, one)
    if (s, k) == (1000, 3):
        assert -np.log(2 * .001 / 1.001) / 3 > 2.0 and eout[0] == 1.0 and esh[0] == 1  # capped
    if n >= 6:
        i, j = np.triu_indices(n, 1)
        assert eout[(i == 0) & (j == 2)][0] == 0.0 and np.isnan(eout[(i == 3) & (j == 4)][0])
        assert (eout[(i == 0) & (j == 5)] == 1.0).all() and esh[(i == 0) & (j == 5)][0] == 0
    with which(kmc, lib):
        assert_distances(gpu_distances(kmc, cuda, rows, sizes, k, True), exp, "n=%d s=%d" % (n, s))
        assert_distances(gpu_distances(kmc, cuda, rows, sizes, k, False), exp, "n=%d s=%d, no counts" % (n, s))


# 9. exact Jaccard when nothing is dropped -------------------------------------------
def overlapping_lists(rng, n, universe_size, p):
    universe = np.unique(rng.integers(0, 1 << 62, size=universe_size, dtype=np.uint64))
    keys, off, sets = [], [0], []
    for _ in range(n):
        mine = universe[rng.random(universe.size) < p]
        sets.append(mine)
        keys.append(rng.permutation(mine))
        off.append(off[-1] + mine.size)
    return np.concatenate(keys), np.asarray(off, dtype=np.uint64), sets


@pytest.mark.parametrize("lib", LIBS)
def test_sketch_exact_jaccard_when_nothing_is_dropped(kmc, cuda, lib):
    """s = 900 holds every record and every union of two (the universe has at most
    900 keys): shared and denom are |A n B| and |A u B| of the key sets themselves.
    s = 700 still holds every record but not every union: the merge rule then
    drops shared values past the s-th of the union, so the counts are the oracle's
    over the rows, no longer the key sets'."""
    import torch
    rng = np.random.default_rng(9)
    n, k = 9, 21
    keys, off, sets = overlapping_lists(rng, n, 900, 0.6)
    i, j = np.triu_indices(n, 1)
    inter = np.array([np.intersect1d(sets[a], sets[b]).size for a, b in zip(i, j)])
    union = np.array([np.union1d(sets[a], sets[b]).size for a, b in zip(i, j)])
    assert max(x.size for x in sets) <= 700 < union.max() <= 900
    dk, _, do = dev_lists(keys, None, off, cuda)
    for s in (900, 700):
        with which(kmc, lib):
            sk, sz = kmc.sketch_from_counts(dk, None, do, s)
            out, sh, dn = kmc.sketch_distances(sk, sz, k, with_counts=True)
            torch.cuda.synchronize()
        np.testing.assert_array_equal(sz.cpu().numpy(), [x.size for x in sets])
        got = (out.cpu().numpy(), sh.cpu().numpy().view(np.uint32), dn.cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(got[2], np.minimum(s, union))
        if s == 900:
            np.testing.assert_array_equal(got[1], inter)
        else:
            assert (got[1] <= inter).all() and (got[1] < inter).any()
        assert_distances(got, S.distances_expected(sk.cpu().numpy().view(np.uint64), sz.cpu().numpy(), s, k),
                         "jaccard s=%d" % s)


# 10. batches concatenate -------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_sketch_batches_concatenate(kmc, cuda, lib):
    import torch
    rng = np.random.default_rng(10)
    n, s, k = 8, 64, 21
    keys, off, _ = overlapping_lists(rng, n, 3000, 0.5)
    off = off.astype(np.int64)
    with which(kmc, lib):
        dk, _, do = dev_lists(keys, None, off, cuda)
        sk, sz = kmc.sketch_from_counts(dk, None, do, s)
        whole = kmc.sketch_distances(sk, sz, k, with_counts=True)
        parts = []
        for a, b in ((0, 4), (4, 8)):
            lo, hi = int(off[a]), int(off[b])
            pk, _, po = dev_lists(keys[lo:hi], None, off[a:b + 1] - lo, cuda)
            parts.append(kmc.sketch_from_counts(pk, None, po, s))
        sk2, sz2 = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        assert torch.equal(sk2, sk) and torch.equal(sz2, sz)
        stacked = kmc.sketch_distances(sk2, sz2, k, with_counts=True)
        torch.cuda.synchronize()
    for x, y in zip(whole, stacked):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))


# 11. end to end on the committed fixtures ----------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("name,dialect", G.cases())
def test_sketch_after_the_canonical_counter(kmc, oracle, cuda, lib, name, dialect):
    """GPU canonical count -> sketch (s = 64) equals the oracle sketch of the host
    canonical oracle's lists, whose key order within a record differs."""
    import torch
    g = G.load(name, dialect)
    idx = G.full_indices(g)
    n = idx.size - 1
    data = g["data"]
    d = dev(data if data.size else np.zeros(16, np.uint8), cuda)
    di = dev(idx, cuda)
    with which(kmc, lib):
        for k in (5, 21):
            ek, ec, eo = oracle.count_canonical(data, idx, k)
            exp = S.sketch_expected(ek, ec, eo, n, 64)
            keys, counts, off = kmc.count_canonical(d, di, k, capacity=max(data.size, 1))
            sk, sz = kmc.sketch_from_counts(keys, counts, off, 64)
            torch.cuda.synchronize()
            assert_sketch((sk.cpu().numpy().view(np.uint64), sz.cpu().numpy().view(np.uint32)), exp,
                          "%s/%s k=%d" % (name, dialect, k))
