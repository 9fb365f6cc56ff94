"""GPU parity of kmc_sketch_from_sequences_grouped and kmc_sketch_merge_groups against
the CPU (sketch_group_util: the canonical oracle's distinct keys per record,
np.unique per group, hashed, sorted and cut).  Rows and sizes are compared bit for
bit, tail fill included.  Every case runs in libkmc.so and in libkmc_diag.so, whose
64-thread walking workgroups, 256-byte ranges and 64-value staging buffer put a few
thousand bases through many ranges, merges and partial sets: there a group's span
crosses many range cuts, and a stretch of short records is longer than a range.
"""
import ctypes

import numpy as np
import pytest

import sketch_group_util as GU
import sketch_util as S
from sketch_util import assert_sketch, bases, pack, which

pytestmark = pytest.mark.gpu

LIBS = ["ship", "diag"]
cached = S.cache()
SOFT, FWD = GU.SOFT, GU.FWD


def revcomp(seq):
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    return comp[seq][::-1]


def to_device(cuda, data, idx, shift=0):
    """A device copy of `data` that starts `shift` bytes after a 16-byte boundary, and the offsets."""
    import torch
    buf = torch.zeros(shift + data.size + 16, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 16 == 0
    d = buf[shift:shift + data.size]
    d.copy_(torch.from_numpy(np.ascontiguousarray(data)))
    return d, torch.from_numpy(np.ascontiguousarray(idx)).to(cuda)


def host(pair):
    import torch
    torch.cuda.synchronize()
    return pair[0].cpu().numpy().view(np.uint64), pair[1].cpu().numpy().view(np.uint32)


def gpu_grouped(kmc, cuda, data, idx, go, k, s, flags=0, shift=0, **kw):
    import torch
    d, di = to_device(cuda, data, idx, shift)
    dg = torch.from_numpy(np.asarray(go, dtype=np.int64)).to(cuda)
    return host(kmc.sketch_from_sequences_grouped(d, di, dg, k, s, flags=flags, **kw))


def gpu_merged(kmc, cuda, data, idx, go, k, s, flags=0, **kw):
    """kmc_sketch_merge_groups of the rows kmc_sketch_from_sequences writes per record."""
    import torch
    d, di = to_device(cuda, data, idx)
    dg = torch.from_numpy(np.asarray(go, dtype=np.int64)).to(cuda)
    rows, sizes = kmc.sketch_from_sequences(d, di, k, s, flags=flags, **kw)
    return host(kmc.sketch_merge_groups(rows, sizes, dg))


# 1. identity grouping -----------------------------------------------------------------
def shapes_case(oracle, s, k=21):
    """The record-shapes input of test_sketch_seq_gpu.py."""
    def make():
        rng = np.random.default_rng(500 + s)
        windows = [1, max(s - 1, 1), s, s + 1, 5 * s + 3]
        recs = [bases(rng, k - 1), bases(rng, 0)] + [bases(rng, w + k - 1) for w in windows] + [bases(rng, 40000)]
        data, idx = pack(recs)
        go = np.arange(idx.size, dtype=np.int64)
        exp = GU.grouped_expected(oracle, data, idx, go, k, s)
        np.testing.assert_array_equal(exp[1], [0, 0] + [min(w, s) for w in windows] + [min(40000 - k + 1, s)])
        return data, idx, go, exp
    return cached(("shapes", s), make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("s", [1, 2, 1000, 16384])
def test_group_identity_equals_the_ungrouped_call(kmc, oracle, cuda, lib, s):
    data, idx, go, exp = shapes_case(oracle, s)
    with which(kmc, lib):
        got = gpu_grouped(kmc, cuda, data, idx, go, 21, s)
        d, di = to_device(cuda, data, idx)
        one = host(kmc.sketch_from_sequences(d, di, 21, s))
    assert_sketch(got, one, "s=%d against the ungrouped call" % s)
    assert_sketch(got, exp, "s=%d" % s)


# 2. one group over records that repeat each other ----------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_group_of_repeated_records(kmc, oracle, cuda, lib):
    """The same 3 kbase record three times and its reverse complement, one group: the
    keys of one record, whatever s."""
    k = 21
    def make():
        rng = np.random.default_rng(21)
        rec = bases(rng, 3000)
        data, idx = pack([rec, rec, rec, revcomp(rec)])
        go = np.array([0, 4], dtype=np.int64)
        one = GU.grouped_expected(oracle, data, idx, [0, 1], k, 4000)
        exp = {s: GU.grouped_expected(oracle, data, idx, go, k, s) for s in (4000, 500)}
        assert one[1][0] == 3000 - k + 1 and exp[4000][1][0] == one[1][0] and exp[500][1][0] == 500
        np.testing.assert_array_equal(exp[4000][0], one[0])
        return data, idx, go, exp
    data, idx, go, exp = cached("repeat", make)
    with which(kmc, lib):
        for s in (4000, 500):
            assert_sketch(gpu_grouped(kmc, cuda, data, idx, go, k, s), exp[s], "s=%d" % s)
            assert_sketch(gpu_merged(kmc, cuda, data, idx, go, k, s), exp[s], "merged s=%d" % s)


# 3. group sizes around s ---------------------------------------------------------------
def around_case(oracle):
    k, s = 21, 100
    def make():
        rng = np.random.default_rng(22)
        win = lambda w: bases(rng, w + k - 1)
        recs = [win(50), win(49), win(50), win(50), win(50), win(51)] + [win(40) for _ in range(4)] \
            + [win(1), win(1)]
        go = np.array([0, 2, 4, 6, 10, 12], dtype=np.int64)
        data, idx = pack(recs)
        exp = GU.grouped_expected(oracle, data, idx, go, k, s)
        # random 21-mers: every window is distinct.  s - 1, s, s + 1; records below s with a
        # union above it; two records of exactly k bases (three values if windows spanned records)
        np.testing.assert_array_equal(exp[1], [s - 1, s, s, s, 2])
        return data, idx, go, exp
    return cached("around", make)


@pytest.mark.parametrize("lib", LIBS)
def test_group_sizes_around_s(kmc, oracle, cuda, lib):
    data, idx, go, exp = around_case(oracle)
    with which(kmc, lib):
        assert_sketch(gpu_grouped(kmc, cuda, data, idx, go, 21, 100), exp)
        assert_sketch(gpu_merged(kmc, cuda, data, idx, go, 21, 100), exp, "merged")


# 4. empty and windowless groups ----------------------------------------------------------
def empty_case(oracle):
    k, s = 21, 32
    def make():
        rng = np.random.default_rng(23)
        recs = [bases(rng, 500), bases(rng, 300), bases(rng, 10), bases(rng, 0), bases(rng, k - 1), bases(rng, 400)]
        recs += [bases(rng, k + int(x)) for x in rng.integers(0, 4, size=200)]
        # empty first; two adjacent empty ones in the middle; a group of records shorter than k
        # and of length 0; 50 groups of four records of k..k+3 bases; empty last
        go = [0, 0, 2, 2, 2, 5, 6] + [6 + 4 * (i + 1) for i in range(50)] + [206]
        go = np.array(go, dtype=np.int64)
        data, idx = pack(recs)
        assert idx.size - 1 == 206
        exp = GU.grouped_expected(oracle, data, idx, go, k, s)
        assert list(exp[1][:6]) == [0, s, 0, 0, 0, s] and exp[1][-1] == 0
        assert (exp[1][6:-1] >= 4).all() and (exp[1][6:-1] <= 16).all()
        return data, idx, go, exp
    return cached("empty", make)


@pytest.mark.parametrize("lib", LIBS)
def test_group_empty_and_windowless_groups(kmc, oracle, cuda, lib):
    data, idx, go, exp = empty_case(oracle)
    with which(kmc, lib):
        got = gpu_grouped(kmc, cuda, data, idx, go, 21, 32)
        assert_sketch(got, exp)
        assert (got[0][[0, 2, 3, 4, -1]] == S.FILL).all()
        assert_sketch(gpu_merged(kmc, cuda, data, idx, go, 21, 32), exp, "merged")


# 5. a range that holds no window of the group that crosses it ----------------------------
def stretch_case(oracle, where):
    """One group of two 2 kbase records and 60 records of 10 bases (660 bytes: more than
    two of the diag build's 256-byte ranges hold no window at k = 21), the stretch in
    the middle, first or last in the group; a neighbouring group on each side."""
    k, s = 21, 64
    def make():
        rng = np.random.default_rng(24 + len(where))
        long_a, long_b = bases(rng, 2000), bases(rng, 2000)
        shorts = [bases(rng, 10) for _ in range(60)]
        mid = {"middle": [long_a] + shorts + [long_b], "first": shorts + [long_a, long_b],
               "last": [long_a, long_b] + shorts}[where]
        recs = [bases(rng, 300)] + mid + [bases(rng, 300)]
        go = np.array([0, 1, 63, 64], dtype=np.int64)
        data, idx = pack(recs)
        exp = GU.grouped_expected(oracle, data, idx, go, k, s)
        assert list(exp[1]) == [s, s, s]
        return data, idx, go, exp
    return cached(("stretch", where), make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("shift", [0, 5, 15])
def test_group_range_without_a_window(kmc, oracle, cuda, lib, shift):
    for where in ("middle", "first", "last"):
        data, idx, go, exp = stretch_case(oracle, where)
        with which(kmc, lib):
            assert_sketch(gpu_grouped(kmc, cuda, data, idx, go, 21, 64, shift=shift), exp,
                          "%s shift=%d" % (where, shift))
            if shift == 0:
                assert_sketch(gpu_merged(kmc, cuda, data, idx, go, 21, 64), exp, "merged %s" % where)


# 6. k, flags, seed ---------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("k", [1, 15, 16, 31])
def test_group_key_widths(kmc, oracle, cuda, lib, k):
    def make():
        rng = np.random.default_rng(600 + k)
        data, idx = pack([bases(rng, 3000), bases(rng, k), bases(rng, 5000), bases(rng, k - 1), bases(rng, 700)])
        go = np.array([0, 2, 2, 5], dtype=np.int64)
        return data, idx, go, {f: GU.grouped_expected(oracle, data, idx, go, k, 100, f) for f in (0, FWD)}
    data, idx, go, exp = cached(("widths", k), make)
    with which(kmc, lib):
        for f in (0, FWD):
            assert_sketch(gpu_grouped(kmc, cuda, data, idx, go, k, 100, flags=f), exp[f], "k=%d flags=%d" % (k, f))


def dirty_case():
    """The dirty-bytes input of test_sketch_seq_gpu.py: lowercase runs, N runs, stray bytes."""
    def make():
        rng = np.random.default_rng(7)
        recs = []
        for L in (900, 2500, 40, 1300):
            r = bases(rng, L)
            for _ in range(L // 150):
                a = int(rng.integers(0, L - 1))
                b = a + int(rng.integers(1, 30))
                kind = int(rng.integers(0, 3))
                if kind == 0:
                    r[a:b] |= 0x20
                elif kind == 1:
                    r[a:b] = ord("N")
                else:
                    r[a] = rng.choice(np.frombuffer(b"\r\0|n", dtype=np.uint8))
            recs.append(r)
        return pack(recs)
    return cached("dirty", make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("flags,seed", [(0, S.DEFAULT_SEED), (FWD, S.DEFAULT_SEED), (SOFT, S.DEFAULT_SEED),
                                        (0, 0x123456789ABCDEF)])
def test_group_flags_seed_and_invalid_bytes(kmc, oracle, cuda, lib, flags, seed):
    data, idx = dirty_case()
    k, s, go = 11, 64, np.array([0, 1, 3, 4], dtype=np.int64)
    exp = cached(("dirty", flags, seed), lambda: GU.grouped_expected(oracle, data, idx, go, k, s, flags, seed))
    base = cached(("dirty", 0, S.DEFAULT_SEED), lambda: GU.grouped_expected(oracle, data, idx, go, k, s))
    if (flags, seed) != (0, S.DEFAULT_SEED):
        assert (base[0] != exp[0]).any()
    with which(kmc, lib):
        assert_sketch(gpu_grouped(kmc, cuda, data, idx, go, k, s, flags=flags, seed=seed, shift=3), exp,
                      "flags=%d seed=%x" % (flags, seed))


# 7. offsets ----------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_group_offsets_are_clamped_and_outer_records_left_out(kmc, oracle, cuda, lib):
    data, idx = dirty_case()
    k, s, n = 11, 64, 4
    for go in ([0, 2, n + 5, n + 9], [1, 2, 3], [-3, 1, 4]):
        exp = cached(("dirty-go", tuple(go)), lambda: GU.grouped_expected(oracle, data, idx, go, k, s))
        with which(kmc, lib):
            assert_sketch(gpu_grouped(kmc, cuda, data, idx, go, k, s), exp, "group_offsets=%s" % go)
    assert cached(("dirty-go", (0, 2, n + 5, n + 9)), None)[1][2] == 0  # [n, n): empty


@pytest.mark.parametrize("lib", LIBS)
def test_group_descending_pair_is_an_empty_group(kmc, cuda, lib):
    """[3, 2) is empty and the call succeeds; the groups that overlap are unspecified."""
    data, idx = dirty_case()
    with which(kmc, lib):
        rows, sizes = gpu_grouped(kmc, cuda, data, idx, [0, 3, 2, 4], 11, 64)
    assert sizes[1] == 0 and (rows[1] == S.FILL).all()


# 8. workspace --------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_group_caller_workspace(kmc, oracle, cuda, lib):
    import torch
    data, idx, go, exp = empty_case(oracle)
    go2 = np.array([0, 1, 100, 206], dtype=np.int64)
    exp2 = cached("empty-go2", lambda: GU.grouped_expected(oracle, data, idx, go2, 21, 32))
    dv = cuda.index or 0
    n = idx.size - 1
    with which(kmc, lib):
        need = kmc.sketch_from_sequences_grouped_workspace_size(n, go.size - 1, data.size, 32, dv)
        assert need > kmc.sketch_from_sequences_workspace_size(n, data.size, 32, dv) > 0
        assert kmc.sketch_from_sequences_grouped_workspace_size(n, go2.size - 1, data.size, 32, dv) <= need
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
        assert_sketch(gpu_grouped(kmc, cuda, data, idx, go, 21, 32, workspace=ws), exp, "prefilled workspace")
        # another grouping of the same data on the workspace the first call left behind, and back
        assert_sketch(gpu_grouped(kmc, cuda, data, idx, go2, 21, 32, workspace=ws), exp2, "second grouping")
        assert_sketch(gpu_grouped(kmc, cuda, data, idx, go, 21, 32, workspace=ws), exp, "first grouping again")
        with pytest.raises(kmc.KmcError) as ei:
            gpu_grouped(kmc, cuda, data, idx, go, 21, 32, workspace=ws[: need - 1])
        assert ei.value.code == 1004
        big = torch.zeros(need + 8, dtype=torch.uint8, device=cuda)
        with pytest.raises(kmc.KmcError) as ei:
            gpu_grouped(kmc, cuda, data, idx, go, 21, 32, workspace=big[4:])
        assert ei.value.code == 1003


# 9. kmc_sketch_merge_groups on rows of its own ---------------------------------------------
def rows_case(s, nrows):
    """Ascending rows drawn from one pool of 3 s values (so rows share values), with sizes
    0, 1, s - 1 and s among them; group 1 holds `nrows` rows."""
    def make():
        rng = np.random.default_rng(900 + s)
        pool = np.unique(rng.integers(0, 1 << 63, size=3 * s, dtype=np.uint64) * np.uint64(2))
        total = nrows + 6
        sizes = rng.integers(s // 2, s + 1, size=total).astype(np.uint32)
        sizes[[0, 3, total - 1]] = [0, 1, s - 1]
        sizes[5] = s
        rows = np.full((total, s), S.FILL, dtype=np.uint64)
        for r in range(total):
            rows[r, :sizes[r]] = np.sort(rng.choice(pool, size=int(sizes[r]), replace=False))
        go = np.array([0, 3, 3 + nrows, 3 + nrows, total, total + 7], dtype=np.int64)
        return rows, sizes, go, GU.merged_expected(rows, sizes, go, s)
    return cached(("rows", s, nrows), make)


@pytest.mark.parametrize("lib", LIBS)
def test_merge_groups_of_300_rows(kmc, cuda, lib):
    """s = 16384 in both builds (the diag build folds 64 values per merge and stays below a second)."""
    import torch
    s = 16384
    rows, sizes, go, exp = rows_case(s, 300)
    dr = torch.from_numpy(rows.view(np.int64)).to(cuda)
    dz = torch.from_numpy(sizes.view(np.int32)).to(cuda)
    dg = torch.from_numpy(go).to(cuda)
    with which(kmc, lib):
        assert_sketch(host(kmc.sketch_merge_groups(dr, dz, dg)), exp)
        # the output over the input is refused
        rc = kmc.lib().kmc_sketch_merge_groups(ctypes.c_void_p(dr.data_ptr()), ctypes.c_void_p(dz.data_ptr()),
                                               dr.shape[0], ctypes.c_void_p(dg.data_ptr()), 2, s,
                                               ctypes.c_void_p(dr.data_ptr() + 8 * s), ctypes.c_void_p(dz.data_ptr()),
                                               None)
        assert rc == 1001
    assert exp[1][2] == 0 and exp[1][4] == 0 and exp[1][1] == s


# 10. distances on grouped rows -----------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_group_rows_feed_the_distances(kmc, oracle, cuda, lib):
    import torch
    data, idx, go, exp = around_case(oracle)
    d, di = to_device(cuda, data, idx)
    dg = torch.from_numpy(go).to(cuda)
    with which(kmc, lib):
        rows, sizes = kmc.sketch_from_sequences_grouped(d, di, dg, 21, 100)
        out, sh, dn = kmc.sketch_distances(rows, sizes, 21, with_counts=True)
        torch.cuda.synchronize()
    eo, es, ed = cached("around-dist", lambda: S.distances_expected(exp[0], exp[1], 100, 21))
    np.testing.assert_array_equal(sh.cpu().numpy().view(np.uint32), es)
    np.testing.assert_array_equal(dn.cpu().numpy().view(np.uint32), ed)
    np.testing.assert_array_equal(out.cpu().numpy(), eo)
