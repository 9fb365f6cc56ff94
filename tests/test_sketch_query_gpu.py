"""GPU parity of kmc_sketch_distances_rect and kmc_sketch_nearest against the numpy
oracle of tests/sketch_query_util.py.  Every case runs in libkmc.so and in
libkmc_diag.so, whose constants (512 staged values, tiles of at most 4 rows, slabs
of 8 references, candidate buffers of pow2(top + 4) keys, a merge buffer of 2
pow2(top) keys) put a few dozen references through many chunks, compactions,
slabs and merge passes.

Rows are built directly: sorted random uint64 with planted overlaps.  shared,
denom, hit_refs, hit_counts, the fill values and the special floats NaN, 1.0 and
+0.0 are compared bit for bit; the other floats within one float32 ulp of
sketch_util.mash_formula (the rule and the reason of test_sketch_gpu.py: the device
evaluates the formula in double, and two correct double logs differ by less than
a double ulp, which moves the rounded float by at most one ulp).  hit_dist equals
kmc_sketch_distances_rect's float of the pair bit for bit.
"""
import os
import subprocess

import numpy as np
import pytest

import golden_util as G
import sketch_query_util as Q
import sketch_util as S
from sketch_util import dev, which

pytestmark = pytest.mark.gpu

LIBS = ["ship", "diag"]
cached = S.cache()
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")
RANDOM_FA = os.path.join(G.GOLDEN, "random.fa")


def dev_rows(rows, sizes, cuda):
    return dev(rows.view(np.int64), cuda), dev(sizes.view(np.int32), cuda)


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def random_rows(rng, n, s, pool, forced=()):
    """n ascending subsets of `pool`; the first sizes are `forced`, the rest random in 0..s."""
    lists = []
    for r in range(n):
        size = forced[r] if r < len(forced) else (int(rng.integers(0, s + 1)) if r % 3 else s)
        lists.append(rng.choice(pool, size=min(size, s), replace=False))
    return Q.pack(lists, s)


def gpu_rect(kmc, cuda, q, r, k, with_counts=True):
    import torch
    got = kmc.sketch_distances_rect(*dev_rows(*q, cuda), *dev_rows(*r, cuda), k, with_counts=with_counts)
    torch.cuda.synchronize()
    if with_counts:
        return host(got[0]), host(got[1], np.uint32), host(got[2], np.uint32)
    return host(got), None, None


def gpu_nearest(kmc, cuda, q, r, k, top, min_shared, **kw):
    import torch
    got = kmc.sketch_nearest(*dev_rows(*q, cuda), *dev_rows(*r, cuda), k, top, min_shared=min_shared, **kw)
    torch.cuda.synchronize()
    refs, sh, dn, dist, counts = got
    return host(refs, np.uint32), host(sh, np.uint32), host(dn, np.uint32), host(dist), host(counts, np.uint32)


def assert_floats(out, eout, msg):
    """The special values bit for bit, the others within one float32 ulp."""
    assert out.shape == eout.shape, msg
    special = np.isnan(eout) | (eout == 1.0) | (eout == 0.0)
    gb, eb = out.view(np.uint32).astype(np.int64), eout.view(np.uint32).astype(np.int64)
    assert (gb[special] == eb[special]).all(), "%s: special values differ" % msg
    ulp = np.abs(gb[~special] - eb[~special])  # positive finite floats: bit patterns are ordered
    print("%s: %d floats, %d special, max ulp %d" % (msg, out.size, int(special.sum()), int(ulp.max(initial=0))))
    assert (ulp <= 1).all(), "%s: max %d ulp" % (msg, int(ulp.max()))


def assert_rect(got, exp, msg):
    (out, sh, dn), (eout, esh, edn) = got, exp
    if sh is not None:
        np.testing.assert_array_equal(sh, esh, err_msg="%s shared" % msg)
        np.testing.assert_array_equal(dn, edn, err_msg="%s denom" % msg)
    assert_floats(out, eout, msg)


def assert_nearest(got, exp, msg):
    for name, g, e in zip(("hit_refs", "hit_shared", "hit_denom"), got[:3], exp[:3]):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (msg, name))
    np.testing.assert_array_equal(got[4], exp[4], err_msg="%s hit_counts" % msg)
    assert_floats(got[3], exp[3], msg)


def assert_dist_is_rects(got, rect_out, msg):
    """hit_dist[q, i] is the rectangle's float of (q, hit_refs[q, i]) bit for bit; NaN in the unused slots."""
    refs, dist, counts = got[0], got[3], got[4]
    for q in range(refs.shape[0]):
        c = int(counts[q])
        a, b = dist[q, :c].view(np.uint32), rect_out[q, refs[q, :c].astype(np.int64)].view(np.uint32)
        assert np.array_equal(a, b), "%s: query %d" % (msg, q)
        assert (dist[q, c:].view(np.uint32) == 0x7FC00000).all(), "%s: query %d fill" % (msg, q)


# 1. the rectangle: shapes ------------------------------------------------------------
def rect_case(m, n, s):
    def make():
        rng = np.random.default_rng(1000 * m + 10 * n + s)
        pool = np.unique(rng.integers(1, (1 << 64) - 1, size=3 * s + 64, dtype=np.uint64))[:3 * s + 8]
        edge = [0, 1, max(s - 1, 0), s, 0]
        q = random_rows(rng, m, s, pool, edge[:m])
        r = random_rows(rng, n, s, pool, ([s, 0, 1, 0, max(s - 1, 0)])[:n])
        k = 3 if s >= 1000 else 21
        return q, r, k, Q.rect_expected(*q, *r, s, k)
    return cached(("rect", m, n, s), make)


RECT_SHAPES = [(m, n, s) for (m, n) in ((1, 1), (5, 7), (9, 37), (3, 300)) for s in (1, 2, 64, 1000)] + [(3, 5, 16384)]


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("m,n,s", RECT_SHAPES)
def test_rect_shapes(kmc, cuda, lib, m, n, s):
    """(m, n) no tile multiples; s = 1000 runs from global memory under diag, s = 16384
    when shipped; row sizes 0, 1, s - 1 and s, pairs with one and with both sides empty."""
    q, r, k, exp = rect_case(m, n, s)
    if m >= 5 and n >= 7:
        assert np.isnan(exp[0][0, 1]) and exp[2][0, 1] == 0  # both empty
        assert exp[2][0, 0] == s and exp[1][0, 0] == 0 and exp[0][0, 0] == 1.0  # an empty side
    with which(kmc, lib):
        assert_rect(gpu_rect(kmc, cuda, q, r, k), exp, "m=%d n=%d s=%d" % (m, n, s))
        assert_rect(gpu_rect(kmc, cuda, q, r, k, False), exp, "m=%d n=%d s=%d, no counts" % (m, n, s))


# 2. the rectangle against the triangle -----------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("s", [64, 1000])
def test_rect_of_one_row_set_is_the_triangle(kmc, cuda, lib, s):
    import torch
    rng = np.random.default_rng(2 + s)
    n, k = 11, 21
    pool = np.unique(rng.integers(1, (1 << 64) - 1, size=3 * s, dtype=np.uint64))[:2 * s]
    rows, sizes = random_rows(rng, n, s, pool, [s, 0, 1, s - 1, 0])
    d_rows, d_sizes = dev_rows(rows, sizes, cuda)
    with which(kmc, lib):
        tri = kmc.sketch_distances(d_rows, d_sizes, k, with_counts=True)
        rect = kmc.sketch_distances_rect(d_rows, d_sizes, d_rows, d_sizes, k, with_counts=True)
        torch.cuda.synchronize()
    i, j = np.triu_indices(n, 1)
    for t, r in zip(tri, rect):
        t, r = host(t, np.uint32), host(r, np.uint32)
        assert np.array_equal(r[i, j], t), "upper triangle"
        assert np.array_equal(r[j, i], t), "lower triangle"
    diag = host(rect[0], np.uint32)[np.arange(n), np.arange(n)]
    assert np.array_equal(diag, np.where(sizes > 0, 0, 0x7FC00000).astype(np.uint32))
    np.testing.assert_array_equal(host(rect[1], np.uint32)[np.arange(n), np.arange(n)], sizes)
    np.testing.assert_array_equal(host(rect[2], np.uint32)[np.arange(n), np.arange(n)], sizes)


# 3. nearest, general -----------------------------------------------------------------
def general_case():
    def make():
        rng = np.random.default_rng(3)
        m, n, s, k = 9, 300, 64, 21
        pool = np.unique(rng.integers(1, (1 << 64) - 1, size=4 * s, dtype=np.uint64))[:3 * s]
        q = random_rows(rng, m, s, pool, [s, 0, 1, s - 1])
        r = random_rows(rng, n, s, pool, [s, 0, 1, s - 1, 0])
        # some references share nothing with anyone: distance 1.0
        far = np.unique(rng.integers(1, (1 << 64) - 1, size=64 * s, dtype=np.uint64))
        far = np.setdiff1d(far, pool)
        for j in range(10, n, 17):
            v = np.sort(rng.choice(far, size=int(rng.integers(1, s + 1)), replace=False))
            r[0][j] = S.FILL
            r[0][j, :v.size] = v
            r[1][j] = v.size
        return q, r, s, k, Q.rect_expected(*q, *r, s, k)
    return cached("general", make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("min_shared", [0, 1, 5])
@pytest.mark.parametrize("top", [1, 3, 10, 1024])
def test_nearest_general(kmc, cuda, lib, top, min_shared):
    q, r, s, k, rect = general_case()
    exp = cached(("general", top, min_shared), lambda: Q.nearest_expected(rect, top, min_shared))
    if top == 1024:
        assert (exp[4] < top).all() and exp[4].max() > 20
        assert exp[4][1] == (0 if min_shared else (r[1] > 0).sum())  # query 1 is empty: shared 0 of denom > 0
    if min_shared == 0:
        assert (rect[0] == 1.0).any() and (top < 1024 or exp[4].max() > 200)
    with which(kmc, lib):
        got = gpu_nearest(kmc, cuda, q, r, k, top, min_shared)
        assert_nearest(got, exp, "top=%d min_shared=%d" % (top, min_shared))
        assert_dist_is_rects(got, gpu_rect(kmc, cuda, q, r, k)[0], "top=%d" % top)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("m,n,s", [(3, 20, 1000), (3, 5, 16384), (70, 9, 16)])
def test_nearest_other_sketch_sizes(kmc, cuda, lib, m, n, s):
    """s = 1000: rows read from global memory under diag; s = 16384: when shipped;
    (70, 9, 16): more query tiles than one, fewer references than a tile."""
    rng = np.random.default_rng(31 + s)
    k = 21
    pool = np.unique(rng.integers(1, (1 << 64) - 1, size=3 * s + 64, dtype=np.uint64))[:2 * s + 8]
    q = random_rows(rng, m, s, pool, [s, 0])
    r = random_rows(rng, n, s, pool, [s, 0, 1])
    rect = Q.rect_expected(*q, *r, s, k)
    with which(kmc, lib):
        for top, min_shared in ((4, 1), (16, 0)):
            got = gpu_nearest(kmc, cuda, q, r, k, top, min_shared)
            assert_nearest(got, Q.nearest_expected(rect, top, min_shared), "s=%d top=%d" % (s, top))


# 4. ties -----------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_nearest_identical_references_come_in_index_order(kmc, cuda, lib):
    rng = np.random.default_rng(4)
    n, s, k = 100, 64, 21
    pool = np.unique(rng.integers(1, (1 << 64) - 1, size=4 * s, dtype=np.uint64))[:3 * s]
    q = Q.pack([pool[:s]], s)
    r = random_rows(rng, n, s, pool[s // 2:], [])
    twin = np.sort(np.concatenate([pool[:40], pool[2 * s:2 * s + 24]]))  # 40 of the query's 64 values
    twins = np.sort(rng.choice(n, size=40, replace=False))
    r[0][twins] = twin
    r[1][twins] = s
    rect = Q.rect_expected(*q, *r, s, k)
    assert np.unique(rect[1][0, twins]).size == 1 and (rect[1][0, twins] > rect[1][0].max() - 1).all()
    with which(kmc, lib):
        for top in (5, 40, 64):
            got = gpu_nearest(kmc, cuda, q, r, k, top, 1)
            assert_nearest(got, Q.nearest_expected(rect, top, 1), "top=%d" % top)
            np.testing.assert_array_equal(got[0][0, :min(top, 40)], twins[:top])


@pytest.mark.parametrize("lib", LIBS)
def test_nearest_equal_and_close_fractions(kmc, cuda, lib):
    """Query 0 = {10, 20}: reference 1 = {10} gives 1/2 and reference 0 = {10, 20, 30, 40}
    gives 2/4, equal fractions with different denominators, so index order decides.
    Query 1 = {10, 20, 30, 40}: reference 2 gives 3/7 and reference 3 gives 4/9, whose
    codes are close (0.4286 and 0.4444) and order 3 before 2.  With min_shared = 0 the
    unrelated references 4, 5, 6, 7 (distance 1.0; 5 is empty: shared 0 of denom = the
    query's size) follow every related one, in index order."""
    s, k = 16, 21
    q = Q.pack([[10, 20], [10, 20, 30, 40]], s)
    r = Q.pack([[10, 20, 30, 40], [10], [10, 20, 30, 50, 60, 70], [10, 20, 30, 40, 51, 52, 53, 54, 55],
                [100, 101], [], [7], [900, 901, 902]], s)
    rect = Q.rect_expected(*q, *r, s, k)
    assert (rect[1][0, 1], rect[2][0, 1], rect[1][0, 0], rect[2][0, 0]) == (1, 2, 2, 4)
    assert (rect[1][1, 2], rect[2][1, 2], rect[1][1, 3], rect[2][1, 3]) == (3, 7, 4, 9)
    with which(kmc, lib):
        for min_shared in (0, 1):
            got = gpu_nearest(kmc, cuda, q, r, k, 8, min_shared)
            assert_nearest(got, Q.nearest_expected(rect, 8, min_shared), "min_shared=%d" % min_shared)
            # query 0: 2/4 (ref 0) and 1/2 (ref 1) tie, then 2/6 (ref 2), 2/9 (ref 3)
            assert got[0][0, :4].tolist() == [0, 1, 2, 3]
            # query 1: 4/4, then 4/9, 3/7, 1/4
            assert got[0][1, :4].tolist() == [0, 3, 2, 1]
            if min_shared == 0:
                assert got[0][:, 4:].tolist() == [[4, 5, 6, 7]] * 2 and got[4].tolist() == [8, 8]
                assert (got[3][:, 4:] == 1.0).all()
            else:
                assert got[4].tolist() == [4, 4]


# 5. empties --------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_nearest_empty_rows_and_reference_sets(kmc, cuda, lib):
    import torch
    rng = np.random.default_rng(5)
    s, k, top = 64, 21, 4
    pool = np.unique(rng.integers(1, (1 << 64) - 1, size=3 * s, dtype=np.uint64))[:2 * s]
    q = Q.pack([[], pool[:s], []], s)
    r = random_rows(rng, 20, s, pool, [0, s, 0, 0])
    rect = Q.rect_expected(*q, *r, s, k)
    empty_refs = np.nonzero(r[1] == 0)[0]
    with which(kmc, lib):
        for min_shared in (0, 1):
            got = gpu_nearest(kmc, cuda, q, r, k, 20, min_shared)
            assert_nearest(got, Q.nearest_expected(rect, 20, min_shared), "min_shared=%d" % min_shared)
            if min_shared == 1:  # an all-empty query: nothing takes part; an empty reference never does
                assert got[4][0] == 0 and (got[0][0] == 0xFFFFFFFF).all() and not got[1][0].any()
                assert not got[2][0].any() and (got[3][0].view(np.uint32) == 0x7FC00000).all()
                assert not np.isin(got[0], empty_refs).any()
            else:  # shared 0 of denom > 0 takes part: for the empty query every reference but the empty ones
                # (both rows empty: NaN, never returned); for the full query all of them, the empty ones at 1.0
                assert got[4][0] == 20 - empty_refs.size and not np.isin(got[0][0], empty_refs).any()
                assert got[4][1] == 20 and np.isin(empty_refs, got[0][1]).all()
        # one reference
        one = (r[0][1:2], r[1][1:2])
        got = gpu_nearest(kmc, cuda, q, one, k, top, 1)
        assert_nearest(got, Q.nearest_expected(Q.rect_expected(*q, *one, s, k), top, 1), "one reference")
        assert got[4].tolist() == [0, 1, 0] and got[0][1].tolist() == [0] + [0xFFFFFFFF] * 3
        # no reference: every row filled, whatever the outputs held
        dq, dqs = dev_rows(*q, cuda)
        none = torch.empty((0, s), dtype=torch.int64, device=cuda)
        refs, sh, dn, dist, counts = kmc.sketch_nearest(dq, dqs, none, torch.empty(0, dtype=torch.int32, device=cuda),
                                                        k, top)
        torch.cuda.synchronize()
        assert not host(counts).any() and (host(refs) == -1).all() and not host(sh).any() and not host(dn).any()
        assert (host(dist, np.uint32) == 0x7FC00000).all()
        assert kmc.sketch_nearest_workspace_size(3, 0, s, top) == 0


# 6. slab and compaction pressure -----------------------------------------------------
def pressure_case():
    def make():
        rng = np.random.default_rng(6)
        n, s, k = 300, 64, 21
        pool = np.unique(rng.integers(1, (1 << 64) - 1, size=8 * s, dtype=np.uint64))[:6 * s]
        query = pool[:s]
        # every reference shares 8..20 of the query's values, most shares occurring many times
        base = [np.concatenate([rng.choice(query, size=int(rng.integers(8, 21)), replace=False),
                                rng.choice(pool[s:], size=s - 20, replace=False)]) for _ in range(n)]
        best = [np.concatenate([query[:c], pool[5 * s:6 * s - c]]) for c in (60, 55, 50)]
        return Q.pack([query, pool[s // 2:s // 2 + s]], s), base, best, s, k
    return cached("pressure", make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("where", [(297, 298, 299), (0, 1, 2), (7, 8, 159), (31, 32, 160), (299, 150, 0)])
def test_nearest_keeps_late_and_early_winners(kmc, cuda, lib, where):
    """The three best references of query 0 planted last, first and on both sides of
    slab boundaries (slabs of 8 under diag, of a multiple of 32 shipped): neither the
    threshold nor the merge may lose them."""
    q, base, best, s, k = pressure_case()
    lists = list(base)
    for at, v in zip(where, best):
        lists[at] = v
    r = Q.pack(lists, s)
    rect = Q.rect_expected(*q, *r, s, k)
    exp = Q.nearest_expected(rect, 3, 1)
    assert exp[0][0].tolist() == list(where)
    with which(kmc, lib):
        got = gpu_nearest(kmc, cuda, q, r, k, 3, 1)
        assert_nearest(got, exp, "best at %s" % (where,))
        assert_dist_is_rects(got, gpu_rect(kmc, cuda, q, r, k)[0], "best at %s" % (where,))


# 7. caller workspace -----------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_nearest_caller_workspace(kmc, cuda, lib):
    import torch
    q, r, s, k, rect = general_case()
    top = 10
    dq, dr = dev_rows(*q, cuda), dev_rows(*r, cuda)
    with which(kmc, lib):
        need = kmc.sketch_nearest_workspace_size(q[0].shape[0], r[0].shape[0], s, top, cuda.index or 0)
        assert need >= 256
        own = kmc.sketch_nearest(*dq, *dr, k, top)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
        for _ in range(2):  # the second call finds the first one's state in the workspace
            got = kmc.sketch_nearest(*dq, *dr, k, top, workspace=ws)
            torch.cuda.synchronize()
            for a, b in zip(got, own):
                assert np.array_equal(host(a).view(np.uint32), host(b).view(np.uint32))
        with pytest.raises(kmc.KmcError) as ei:
            kmc.sketch_nearest(*dq, *dr, k, top, workspace=ws[: need - 256])
        assert ei.value.code == 1004
    exp = cached(("general", top, 1), lambda: Q.nearest_expected(rect, top, 1))
    assert_nearest(tuple(host(x).view(np.uint32) if x.dtype != torch.float32 else host(x) for x in own), exp, "own")


# 8. the driver -----------------------------------------------------------------------
def split_fasta(tmp_path, kmc):
    """tests/golden/random.fa (three records) as a reference file of the first two records
    and a query file of the last two, so that query 0 is reference 1 and query 1 is unrelated
    to both; returns the paths and the record buffers (data, indices) as the loader reads them."""
    recs, cur = [], None
    for line in open(RANDOM_FA):
        if line.startswith(">"):
            cur = []
            recs.append(cur)
        if cur is not None:
            cur.append(line)
    assert len(recs) == 3
    files, bufs = [], []
    for name, part in (("refs.fa", recs[:2]), ("query.fa", recs[1:])):
        p = tmp_path / name
        p.write_text("".join("".join(r) for r in part))
        files.append(p)
        data, idx, _ = kmc.load_fasta(str(p), kmc.DIALECT_NONL, 0)
        assert idx.size - 1 == len(part)
        bufs.append((data, idx))
    return files, bufs


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def fmt_matches(line, e):
    return np.isnan(float(line)) if np.isnan(e) else line == "%f" % e


def test_cli_query(kmc, cuda, tmp_path):
    import torch
    k, s, top = 21, 64, 3
    (ref_fa, query_fa), bufs = split_fasta(tmp_path, kmc)
    rows = []
    for data, idx in bufs:
        rows.append(kmc.sketch_from_sequences(dev(data, cuda), dev(idx, cuda), k, s))
    (rr, rs), (qr, qs) = rows
    refs, sh, dn, dist, counts = kmc.sketch_nearest(qr, qs, rr, rs, k, top)
    rect = kmc.sketch_distances_rect(qr, qs, rr, rs, k)
    torch.cuda.synchronize()
    refs, sh, dn, dist, counts = host(refs), host(sh), host(dn), host(dist), host(counts)
    assert counts.tolist() == [1, 0] and refs[0, 0] == 1 and dist[0, 0] == 0.0
    base = ["-k", k, "--canonical", "--sketch", s, "--sketch-direct", "--dialect", "nonl", "--max-seqs", 0]
    out = tmp_path / "out"
    out.mkdir()
    r = run(base + ["--out", out, "--query", query_fa, "--top", top, ref_fa])
    assert r.returncode == 0, r.stderr
    assert not (out / "sketch_results.csv").exists()
    lines = open(out / "query_results.tsv").read().splitlines()
    exp = [(q, i + 1, refs[q, i], sh[q, i], dn[q, i], dist[q, i]) for q in range(refs.shape[0])
           for i in range(counts[q])]
    assert len(lines) == len(exp)
    for line, e in zip(lines, exp):
        f = line.split("\t")
        assert len(f) == 6 and [int(x) for x in f[:5]] == [int(x) for x in e[:5]], line
        assert fmt_matches(f[5], e[5]), line
    out0 = tmp_path / "out0"
    out0.mkdir()
    r = run(base + ["--out", out0, "--query", query_fa, "--top", 0, ref_fa])
    assert r.returncode == 0, r.stderr
    assert not (out0 / "sketch_results.csv").exists() and not (out0 / "query_results.tsv").exists()
    lines = open(out0 / "query_distances.csv").read().splitlines()
    flat = host(rect).reshape(-1)
    assert len(lines) == flat.size
    for i, (line, e) in enumerate(zip(lines, flat)):
        assert fmt_matches(line, e), "line %d: %s vs %f" % (i, line, e)


def test_cli_query_per_file(kmc, cuda, tmp_path):
    """--per-file: every reference file and the query file are one genome each."""
    import torch
    k, s = 21, 64
    (ref_fa, query_fa), bufs = split_fasta(tmp_path, kmc)
    rows = []
    for data, idx in bufs:
        go = torch.tensor([0, idx.size - 1], dtype=torch.int64, device=cuda)
        rows.append(kmc.sketch_from_sequences_grouped(dev(data, cuda), dev(idx, cuda), go, k, s))
    # references: the reference file, then the query file itself
    rr, rs = torch.cat([rows[0][0], rows[1][0]]), torch.cat([rows[0][1], rows[1][1]])
    refs, sh, dn, dist, counts = kmc.sketch_nearest(*rows[1], rr, rs, k, 10)
    torch.cuda.synchronize()
    c = int(counts[0])
    assert c >= 1 and int(refs[0, 0]) == 1 and float(dist[0, 0]) == 0.0
    out = tmp_path / "out"
    out.mkdir()
    r = run(["-k", k, "--canonical", "--sketch", s, "--sketch-direct", "--per-file", "--dialect", "nonl", "--out", out,
             "--query", query_fa, ref_fa, query_fa])
    assert r.returncode == 0, r.stderr
    lines = open(out / "query_results.tsv").read().splitlines()
    assert len(lines) == c
    for i, line in enumerate(lines):
        f = line.split("\t")
        assert [int(x) for x in f[:5]] == [0, i + 1, int(refs[0, i]), int(sh[0, i]), int(dn[0, i])]
        assert fmt_matches(f[5], float(dist[0, i]))
