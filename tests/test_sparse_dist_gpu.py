"""GPU parity of kmc_pair_distances_sparse (pairwise distance from per-record
(key, count) lists): against the reference's own CSV values (golden kX_dist),
the oracle's dense distance, exact numpy sums, the host canonical oracle and the
dense GPU path.  Every case runs in libkmc.so and in libkmc_diag.so, whose small
bucket target and LDS capacity (64 / 256 entries) put a few hundred entries
through the multi-pass and the tiled paths.

Floats are compared bit for bit (NaN == NaN, +0 == -0); the sums are exact.
"""

import numpy as np
import pytest

import golden_util as G
import sparse_dist_util as U
from sketch_util import dev, which

pytestmark = pytest.mark.gpu

LIBS = ["ship", "diag"]


def same_floats(got, exp, msg=""):
    got = np.asarray(got, dtype=np.float32)
    exp = np.asarray(exp, dtype=np.float32)
    assert got.shape == exp.shape, msg
    both_nan = np.isnan(got) & np.isnan(exp)
    bad = ~both_nan & (got.view(np.uint32) != exp.view(np.uint32)) & ~((got == 0) & (exp == 0))
    assert not bad.any(), "%s: %d mismatches, first at %d: %r vs %r" % (
        msg, int(bad.sum()), int(np.argmax(bad)), got[bad][:3], exp[bad][:3])


def dev_lists(keys, counts, off, cuda):
    """uint64 / uint32 host lists as the int64 / int32 tensors the binding takes."""
    return (dev(np.asarray(keys, dtype=np.uint64).view(np.int64), cuda),
            dev(np.asarray(counts, dtype=np.uint32).view(np.int32), cuda),
            dev(np.asarray(off, dtype=np.uint64).view(np.int64), cuda))


def gpu_sparse(kmc, cuda, keys, counts, off, idx, k, **kw):
    import torch
    dk, dc, do = dev_lists(keys, counts, off, cuda)
    out = kmc.pair_distances_sparse(dk, dc, do, dev(np.asarray(idx, dtype=np.int64), cuda), k, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def lens_to_idx(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64) + 1)]).astype(np.int64)


# 1. the reference's own distances ------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("name,dialect", G.cases())
def test_sparse_matches_reference_distances(kmc, cuda, lib, name, dialect):
    """Entries = the non-zero bins of the fixture's dense histogram (key = bin code,
    count = bin value, shuffled within each record) -> the reference's
    sequentialKmerCount2 output, including records shorter than k (NaN) and empty
    records.  For k <= 8 the bins are read off G.dense_expected; above that the
    4^k x n matrix is not materialised and the fixture's (code, record, count)
    triplets, which are exactly what dense_expected scatters, are taken directly."""
    g = G.load(name, dialect)
    idx = G.full_indices(g)
    n = int(g["n_seqs"])
    rng = np.random.default_rng(11)
    with which(kmc, lib):
        for k in g["ks"]:
            k = int(k)
            if k <= 8:
                keys, counts, off = U.lists_from_dense(rng, G.dense_expected(g, k)[0])
            else:
                keys, counts, off = U.lists_from_triplets(rng, g["k%d_code" % k], g["k%d_rec" % k],
                                                          g["k%d_count" % k], n)
            got = gpu_sparse(kmc, cuda, keys, counts, off, idx, k)
            same_floats(got, g["k%d_dist" % k], "%s/%s k=%d" % (name, dialect, k))


# 2. random entries against the oracle's dense distance ---------------------------
_random_cache = {}


def random_case(oracle, n):
    """U = 2000 random 62-bit keys, every record a random subset with counts < 2^20;
    expected from the same counts scattered into a dense matrix (2000 rows, padded
    with zero rows to the 4^6 bins oracle.pair_distances walks at k = 6)."""
    if n not in _random_cache:
        k, nkeys = 6, 2000
        rng = np.random.default_rng(7000 + n)
        universe = np.unique(rng.integers(0, 1 << 62, size=nkeys, dtype=np.uint64))
        dense = np.zeros((1 << (2 * k), n), dtype=np.int32)
        present = rng.random((universe.size, n)) < 0.5
        dense[:universe.size][present] = rng.integers(1, 1 << 20, size=int(present.sum()))
        lens = dense.astype(np.int64).sum(axis=0) + k - 1 + rng.integers(0, 50, size=n)
        rows, counts, off = U.lists_from_dense(rng, dense)
        keys = universe[rows.astype(np.int64)]
        exp = oracle.pair_distances(dense, lens, k)
        _random_cache[n] = (keys, counts, off, lens_to_idx(lens), k, exp)
    return _random_cache[n]


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("n", [2, 5, 17, 65, 300])
def test_sparse_random_vs_oracle(kmc, oracle, cuda, lib, n):
    keys, counts, off, idx, k, exp = random_case(oracle, n)
    with which(kmc, lib):
        got = gpu_sparse(kmc, cuda, keys, counts, off, idx, k)
    same_floats(got, exp, "n=%d" % n)


# 3. sums beyond 2^32 ---------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_sparse_exact_64_bit_sums(kmc, cuda, lib):
    rng = np.random.default_rng(3)
    n, k, nkeys = 12, 21, 300
    universe = np.unique(rng.integers(0, 1 << 62, size=nkeys, dtype=np.uint64))
    keys, counts, off = [], [], [0]
    for s in range(n):
        mine = universe[rng.random(universe.size) < 0.7]
        keys.append(rng.permutation(mine))
        c = rng.integers(1 << 31, 1 << 32, size=mine.size, dtype=np.uint64).astype(np.uint32)
        c[: min(3, c.size)] = 0xFFFFFFFF
        counts.append(c)
        off.append(off[-1] + mine.size)
    keys, counts = np.concatenate(keys), np.concatenate(counts)
    off = np.asarray(off, dtype=np.uint64)
    S = U.pair_sums(keys, counts, off, n)
    assert S.max() > 1 << 32
    lens = rng.integers(1 << 33, 1 << 41, size=n)
    with which(kmc, lib):
        got = gpu_sparse(kmc, cuda, keys, counts, off, lens_to_idx(lens), k)
    same_floats(got, U.distances_from_sums(S, lens, k))


# 4. key groups larger than a bucket's capacity -----------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_sparse_one_key_in_every_record(kmc, cuda, lib):
    """n = 700: the shared key's group exceeds the diagnostic LDS capacity (256),
    and no hash bit can split it."""
    rng = np.random.default_rng(4)
    n, k = 700, 31
    shared = np.uint64(0x2545F4914F6CDD1D)
    private = np.arange(1, 3 * n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    cs = (1 + np.arange(n) % 7).astype(np.uint32)
    keys = np.empty(4 * n, dtype=np.uint64)
    counts = np.empty(4 * n, dtype=np.uint32)
    for s in range(n):
        o = rng.permutation(4)
        kk = np.concatenate([[shared], private[3 * s:3 * s + 3]])
        cc = np.concatenate([[cs[s]], rng.integers(1, 100, size=3).astype(np.uint32)])
        keys[4 * s:4 * s + 4], counts[4 * s:4 * s + 4] = kk[o], cc[o]
    off = (4 * np.arange(n + 1)).astype(np.uint64)
    lens = rng.integers(100, 1000, size=n)
    i, j = np.triu_indices(n, 1)
    S = np.minimum(cs[i], cs[j]).astype(np.uint64)
    with which(kmc, lib):
        got = gpu_sparse(kmc, cuda, keys, counts, off, lens_to_idx(lens), k)
    same_floats(got, U.distances_from_sums(S, lens, k))


@pytest.mark.parametrize("lib", LIBS)
def test_sparse_three_distinct_keys(kmc, cuda, lib):
    """3 distinct keys over 500 records: everything lands in at most 3 buckets."""
    rng = np.random.default_rng(5)
    n, k = 500, 17
    universe = np.array([7, 1 << 40, (1 << 62) - 5], dtype=np.uint64)
    dense = rng.integers(1, 1000, size=(3, n)).astype(np.int64)
    dense[rng.random((3, n)) < 0.3] = 0
    rows, counts, off = U.lists_from_dense(rng, dense)
    lens = rng.integers(100, 1000, size=n)
    i, j = np.triu_indices(n, 1)
    S = np.minimum(dense[:, i], dense[:, j]).sum(axis=0).astype(np.uint64)
    with which(kmc, lib):
        got = gpu_sparse(kmc, cuda, universe[rows.astype(np.int64)], counts, off, lens_to_idx(lens), k)
    same_floats(got, U.distances_from_sums(S, lens, k))


# 5. edges ------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_sparse_edges(kmc, cuda, lib):
    rng = np.random.default_rng(6)
    with which(kmc, lib):
        # no entries at all: the formula with S = 0 (a record of exactly k - 1 bases gives 0/0)
        lens = np.array([40, 5, 4, 0, 9])
        got = gpu_sparse(kmc, cuda, np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(6, np.uint64),
                         lens_to_idx(lens), 5)
        same_floats(got, U.distances_from_sums(np.zeros(10, np.uint64), lens, 5), "no entries")
        # empty ranges at both ends and in the middle
        dense = rng.integers(0, 9, size=(64, 7)).astype(np.int64)
        dense[:, [0, 3, 4, 6]] = 0
        keys, counts, off = U.lists_from_dense(rng, dense)
        lens = dense.sum(axis=0) + 2 + rng.integers(0, 9, size=7)
        i, j = np.triu_indices(7, 1)
        S = np.minimum(dense[:, i], dense[:, j]).sum(axis=0).astype(np.uint64)
        got = gpu_sparse(kmc, cuda, keys, counts, off, lens_to_idx(lens), 3)
        same_floats(got, U.distances_from_sums(S, lens, 3), "empty ranges")
        # two records
        keys = np.array([5, 9, 1, 9, 5, 77], dtype=np.uint64)
        counts = np.array([3, 8, 2, 6, 4, 1], dtype=np.uint32)
        got = gpu_sparse(kmc, cuda, keys, counts, np.array([0, 3, 6], np.uint64), lens_to_idx([30, 20]), 4)
        same_floats(got, U.distances_from_sums(np.array([3 + 6], np.uint64), [30, 20], 4), "n = 2")


# 6. after the real counter -------------------------------------------------------
_dna_cache = {}


def dna_records():
    """20 records of 200..5000 bases, 2 % N, records 10..19 mutated copies of
    0..9 (substitutions, so that intersections are non-trivial); `soft` has
    lowercase runs on top."""
    if not _dna_cache:
        rng = np.random.default_rng(60)
        alpha = np.frombuffer(b"ACGTN", dtype=np.uint8)
        recs = [rng.choice(alpha, size=int(L), p=[.245, .245, .245, .245, .02])
                for L in rng.integers(200, 5001, size=10)]
        for s in range(10):
            r = recs[s].copy()
            hit = rng.random(r.size) < 0.03
            r[hit] = rng.choice(alpha[:4], size=int(hit.sum()))
            recs.append(r[: int(rng.integers(r.size // 2, r.size + 1))])
        soft = []
        for r in recs:
            r = r.copy()
            for _ in range(3):
                a = int(rng.integers(0, r.size))
                r[a:a + int(rng.integers(1, 200))] |= 0x20
            soft.append(r)
        for name, rr in (("upper", recs), ("soft", soft)):
            data = np.concatenate([np.append(r, np.uint8(0)) for r in rr])
            idx = np.concatenate([[0], np.cumsum([r.size + 1 for r in rr])]).astype(np.int64)
            _dna_cache[name] = (data, idx)
    return _dna_cache


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("k,canonical,soft", [(11, False, False), (11, True, False), (31, True, False),
                                              (31, True, True)])
def test_sparse_after_the_canonical_counter(kmc, oracle, cuda, lib, k, canonical, soft):
    import torch
    data, idx = dna_records()["soft" if soft else "upper"]
    flags = (0 if canonical else kmc.CANON_FORWARD) | (kmc.CANON_SOFTMASK if soft else 0)
    exp = U.canonical_expected(oracle, data, idx, k, soft=soft, forward=not canonical)
    d, di = dev(data, cuda), dev(idx, cuda)
    with which(kmc, lib):
        keys, counts, off = kmc.count_canonical(d, di, k, flags)
        got = kmc.pair_distances_sparse(keys, counts, off, di, k)
        torch.cuda.synchronize()
        same_floats(got.cpu().numpy(), exp, "k=%d flags=%d" % (k, flags))
        if not canonical:
            dense, _ = kmc.count_dense(d, di, k)
            ref = kmc.pair_distances(dense, di, k)
            torch.cuda.synchronize()
            same_floats(got.cpu().numpy(), ref.cpu().numpy(), "dense path")


# 7. workspace --------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_sparse_caller_workspace(kmc, oracle, cuda, lib):
    import torch
    keys, counts, off, idx, k, exp = random_case(oracle, 65)
    n = idx.size - 1
    dk, dc, do = dev_lists(keys, counts, off, cuda)
    di = dev(idx, cuda)
    with which(kmc, lib):
        need = kmc.pair_distances_sparse_workspace_size(n, keys.size, cuda.index or 0)
        assert need > 0
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
        for _ in range(2):  # the second call finds the first one's sums in the workspace
            got = kmc.pair_distances_sparse(dk, dc, do, di, k, workspace=ws)
            torch.cuda.synchronize()
            same_floats(got.cpu().numpy(), exp)
        own = kmc.pair_distances_sparse(dk, dc, do, di, k)
        torch.cuda.synchronize()
        same_floats(own.cpu().numpy(), exp)
        with pytest.raises(kmc.KmcError) as ei:
            kmc.pair_distances_sparse(dk, dc, do, di, k, workspace=ws[: need - 1])
        assert ei.value.code == 1004


@pytest.mark.parametrize("lib", LIBS)
def test_sparse_offsets_beyond_num_entries_are_clamped(kmc, oracle, cuda, lib):
    """rec_offsets describes more entries than num_entries (and than keys / counts
    hold): the call returns, and the pairs of records lying wholly below
    num_entries are right.  The walk indexes entries by e < num_entries only and
    merely compares against the (clamped) offsets."""
    keys, counts, off, idx, k, exp = random_case(oracle, 17)
    n = idx.size - 1
    cut = int(off[n - 1]) + int(off[n] - off[n - 1]) // 2  # inside the last record
    with which(kmc, lib):
        got = gpu_sparse(kmc, cuda, keys[:cut], counts[:cut], off, idx, k, num_entries=cut)
    i, j = np.triu_indices(n, 1)
    whole = j < n - 1
    same_floats(got[whole], exp[whole])
