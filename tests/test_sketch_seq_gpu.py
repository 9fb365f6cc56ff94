"""GPU parity of kmc_sketch_from_sequences against the CPU: the canonical oracle's
distinct keys per record (oracle.count_canonical), hashed, sorted and cut by
sketch_util.sketch_expected.  Rows and sizes are compared bit for bit, tail fill
included.  Every case runs in libkmc.so and in libkmc_diag.so, whose 64-thread
walking workgroups, 256-byte ranges (16 chunks of 16 bytes, while the input has at
most 2 x CUs of them) and 64-value staging buffer put a few thousand bases through
many ranges, merges and partial sets.

Offsets above 2^31 are not tested here: the walk's 64-bit path (chunk_raw's
rebased buffer resource, kmc_canon_walk.h) is shared unchanged with the canonical
counter, whose large-offset tests cover it.
"""
import os

import numpy as np
import pytest

import sketch_group_util as GU
import sketch_util as S
from sketch_util import assert_sketch, bases, pack, which

pytestmark = pytest.mark.gpu

LIBS = ["ship", "diag"]
cached = S.cache()
SOFT, FWD = 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def expected(oracle, data, idx, k, s, flags=0, seed=S.DEFAULT_SEED):
    ek, _, eo = oracle.count_canonical(data, idx, k, soft=bool(flags & SOFT), forward=bool(flags & FWD))
    return S.sketch_expected(ek, None, eo, idx.size - 1, s, seed)


def gpu_seq(kmc, cuda, data, idx, k, s, flags=0, shift=0, **kw):
    """The call on a device copy of `data` that starts `shift` bytes after a 16-byte boundary."""
    import torch
    buf = torch.zeros(shift + data.size + 16, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 16 == 0
    d = buf[shift:shift + data.size]
    d.copy_(torch.from_numpy(np.ascontiguousarray(data)))
    di = torch.from_numpy(np.ascontiguousarray(idx)).to(cuda)
    sk, sz = kmc.sketch_from_sequences(d, di, k, s, flags=flags, **kw)
    torch.cuda.synchronize()
    return sk.cpu().numpy().view(np.uint64), sz.cpu().numpy().view(np.uint32)


# 1. record shapes -----------------------------------------------------------------
def shapes_case(oracle, s, k=21):
    def make():
        rng = np.random.default_rng(500 + s)
        windows = [1, max(s - 1, 1), s, s + 1, 5 * s + 3]
        recs = [bases(rng, k - 1), bases(rng, 0)] + [bases(rng, w + k - 1) for w in windows] + [bases(rng, 40000)]
        data, idx = pack(recs)
        exp = expected(oracle, data, idx, k, s)
        # random 21-mers: every window of a record is distinct
        np.testing.assert_array_equal(exp[1], [0, 0] + [min(w, s) for w in windows] + [min(40000 - k + 1, s)])
        return data, idx, exp
    return cached(("shapes", s), make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("s", [1, 2, 1000, 16384])
def test_seq_record_shapes(kmc, oracle, cuda, lib, s):
    data, idx, exp = shapes_case(oracle, s)
    with which(kmc, lib):
        assert_sketch(gpu_seq(kmc, cuda, data, idx, 21, s), exp, "s=%d" % s)


# 2. key width edges -----------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("k", [1, 2, 15, 16, 31])
def test_seq_key_widths(kmc, oracle, cuda, lib, k):
    """k = 15 | 16: the one-dword / two-dword key instances.  At k <= 3 the key space
    (at most 4^k / 2 + a few canonical keys) is below s = 100: a long record keeps its
    set unfilled to the end."""
    def make():
        rng = np.random.default_rng(600 + k)
        data, idx = pack([bases(rng, 3000), bases(rng, k), bases(rng, 5000), bases(rng, k - 1), bases(rng, 700)])
        return data, idx, {f: expected(oracle, data, idx, k, 100, f) for f in (0, FWD)}
    data, idx, exp = cached(("widths", k), make)
    if k <= 2:
        assert exp[0][1].max() < 100 and exp[FWD][1][0] == 4 ** k
    with which(kmc, lib):
        for f in (0, FWD):
            assert_sketch(gpu_seq(kmc, cuda, data, idx, k, 100, flags=f), exp[f], "k=%d flags=%d" % (k, f))


# 3. flags and invalid bytes ---------------------------------------------------------
def dirty_case():
    def make():
        rng = np.random.default_rng(7)
        recs = []
        for L in (900, 2500, 40, 1300):
            r = bases(rng, L)
            for _ in range(L // 150):  # lowercase runs, N runs, stray bytes
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
@pytest.mark.parametrize("flags", [0, SOFT, FWD, SOFT | FWD])
def test_seq_flags_and_invalid_bytes(kmc, oracle, cuda, lib, flags):
    data, idx = dirty_case()
    k, s = 11, 64
    exp = cached(("dirty", flags), lambda: expected(oracle, data, idx, k, s, flags))
    if flags == SOFT:  # lowercase windows count only with the flag
        assert (cached(("dirty", 0), lambda: expected(oracle, data, idx, k, s, 0))[0] != exp[0]).any()
    with which(kmc, lib):
        assert_sketch(gpu_seq(kmc, cuda, data, idx, k, s, flags=flags), exp, "flags=%d" % flags)


@pytest.mark.parametrize("lib", LIBS)
def test_seq_window_touching_an_invalid_byte_is_not_sketched(kmc, oracle, cuda, lib):
    """One N in the middle of 2k - 1 bases: no window is valid; beside k clean bases."""
    k = 9
    rng = np.random.default_rng(8)
    bad = bases(rng, 2 * k - 1)
    bad[k - 1] = ord("N")
    data, idx = pack([bad, bases(rng, k)])
    with which(kmc, lib):
        got = gpu_seq(kmc, cuda, data, idx, k, 4)
    np.testing.assert_array_equal(got[1], [0, 1])
    assert (got[0][0] == S.FILL).all()
    assert_sketch(got, expected(oracle, data, idx, k, 4))


# 4. duplicates ----------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_seq_all_a_record(kmc, oracle, cuda, lib):
    rng = np.random.default_rng(9)
    data, idx = pack([np.full(20000, ord("A"), np.uint8), bases(rng, 300)])
    exp = cached("all_a", lambda: expected(oracle, data, idx, 21, 16))
    assert exp[1][0] == 1
    with which(kmc, lib):
        assert_sketch(gpu_seq(kmc, cuda, data, idx, 21, 16), exp)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("dp", [-1, 0, 1])
def test_seq_repeated_unit(kmc, oracle, cuda, lib, dp):
    """A unit of p bases repeated 12 times has p distinct forward windows (a random
    unit, k = 21), p = s - 1, s, s + 1; the canonical fold keeps them distinct."""
    s, k = 150, 21
    p = s + dp
    def make():
        rng = np.random.default_rng(40 + p)
        unit = bases(rng, p)
        data, idx = pack([np.tile(unit, 12), bases(rng, 50)])
        exp = {f: expected(oracle, data, idx, k, s, f) for f in (0, FWD)}
        assert exp[FWD][1][0] == min(p, s) and exp[0][1][0] == min(p, s)
        return data, idx, exp
    data, idx, exp = cached(("unit", p), make)
    with which(kmc, lib):
        for f in (0, FWD):
            assert_sketch(gpu_seq(kmc, cuda, data, idx, k, s, flags=f), exp[f], "p=%d flags=%d" % (p, f))


@pytest.mark.parametrize("lib", LIBS)
def test_seq_identical_halves_and_reverse_complement(kmc, oracle, cuda, lib):
    """Record 0: a 1000-base half twice, so the diag build's 256-byte ranges hold the
    same hashes in several partial sets and the merge kernel drops them.  Record 1: a
    sequence followed by its reverse complement (the same canonical keys twice)."""
    k, s = 21, 2000
    def make():
        rng = np.random.default_rng(11)
        half = bases(rng, 1000)
        seq = bases(rng, 1500)
        comp = np.zeros(256, np.uint8)
        comp[list(b"ACGT")] = list(b"TGCA")
        data, idx = pack([np.concatenate([half, half]), np.concatenate([seq, comp[seq][::-1]])])
        exp = expected(oracle, data, idx, k, s)
        # half the windows repeat (but for those across the seam)
        assert exp[1][0] < 1000 + k and 1500 - k < exp[1][1] <= 1500 + k
        return data, idx, exp
    data, idx, exp = cached("halves", make)
    with which(kmc, lib):
        assert_sketch(gpu_seq(kmc, cuda, data, idx, k, s), exp)
        assert_sketch(gpu_seq(kmc, cuda, data, idx, k, 100), cached("halves100", lambda: expected(oracle, data, idx, k, 100)))


# 5. ranges and pieces ---------------------------------------------------------------
def tiny_case():
    def make():
        rng = np.random.default_rng(12)
        lens = list(rng.integers(0, 41, size=150)) + [40000] + list(rng.integers(0, 41, size=150))
        return pack([bases(rng, L) for L in lens])
    return cached("tiny", make)


@pytest.mark.parametrize("lib", LIBS)
def test_seq_many_tiny_records_around_a_long_one(kmc, oracle, cuda, lib):
    """301 records; in the diag build the long one runs over about 150 ranges."""
    data, idx = tiny_case()
    exp = cached("tiny16", lambda: expected(oracle, data, idx, 15, 16))
    with which(kmc, lib):
        assert_sketch(gpu_seq(kmc, cuda, data, idx, 15, 16), exp)


@pytest.mark.parametrize("lib", LIBS)
def test_seq_record_boundaries_on_range_cuts(kmc, oracle, cuda, lib):
    """4096 bytes of records: the diag build walks them in 256-byte ranges (256 chunks
    over 17 workgroups, 16 chunks each).  Record starts on a range cut, one byte before
    and after it, and on 16-byte boundaries +- 1."""
    k, s = 5, 8
    def make():
        rng = np.random.default_rng(13)
        cuts = [255, 256, 257, 271, 272, 273, 511, 512, 513, 768, 1023, 1025, 1279, 1280, 1296, 2047, 2049, 2560,
                3071, 3072, 3073, 3583, 3584, 3600, 4096]
        recs, at = [], 0
        for c in cuts:
            recs.append(bases(rng, c - at - 1))
            at = c
        data, idx = pack(recs)
        assert data.size == 4096 and list(idx[1:]) == cuts
        return data, idx, expected(oracle, data, idx, k, s)
    data, idx, exp = cached("cuts", make)
    with which(kmc, lib):
        assert_sketch(gpu_seq(kmc, cuda, data, idx, k, s), exp)


def diag_range_bytes(nbytes):
    """Bytes per range of the diag build's walk over `nbytes` of 16-byte aligned records
    (kmc_sketch_seq.hip: 16 chunks per range at least; far fewer ranges than 2 x CUs)."""
    chunks = (nbytes + 15) // 16
    groups = -(-(nbytes // 16 + 3) // 16)
    return 16 * max(-(-chunks // groups), 1)


def records_at(rng, starts, total):
    """Records that start at the bytes `starts` (0 first), the last one's terminator at total - 1."""
    ends = list(starts[1:]) + [total]
    return pack([bases(rng, e - a - 1) for a, e in zip(starts, ends)])


@pytest.mark.parametrize("lib", LIBS)
def test_seq_window_span_against_byte_span(kmc, oracle, cuda, lib):
    """Where a record's set goes follows from its window starts, not from its bytes (diag
    build, cuts every 256 bytes).  Record 1 starts at 300 and has 212 windows: the last
    one starts at 511 and the last k - 1 bases and the terminator lie beyond cut 512, so
    it is range 1's whole record.  Record 3 starts on cut 768 and crosses two cuts.
    Record 4 starts in range 5, crosses cut 1536 and its windows end on cut 2048.
    s = 16: the sets fill and merges run at 64 staged values."""
    k, s = 21, 16
    def make():
        rng = np.random.default_rng(16)
        starts = [0, 300, 533, 768, 1469, 2069]
        data, idx = records_at(rng, starts, 4096)
        assert data.size == 4096 and diag_range_bytes(data.size) == 256
        nw = np.diff(idx) - k
        assert idx[1] + nw[1] == 512 and idx[2] > 512 and idx[3] == 768 and idx[4] + nw[4] == 2048 < idx[5]
        return data, idx, expected(oracle, data, idx, k, s)
    data, idx, exp = cached("spans", make)
    assert list(exp[1]) == [s] * 6
    with which(kmc, lib):
        assert_sketch(gpu_seq(kmc, cuda, data, idx, k, s), exp)


@pytest.mark.parametrize("lib", LIBS)
def test_seq_windowless_stretch_between_long_records(kmc, oracle, cuda, lib):
    """60 records of 10 bases (660 bytes, k = 21: no window; in the diag build at least two
    whole 256-byte ranges hold nothing else) between two records of 1 kbase that each cross
    cuts: the short ones get size 0 and rows of UINT64_MAX, whatever the walk's workgroups
    zeroed or left in their slots."""
    k, s = 21, 16
    def make():
        rng = np.random.default_rng(17)
        data, idx = pack([bases(rng, 1000)] + [bases(rng, 10) for _ in range(60)] + [bases(rng, 1000)])
        rb = diag_range_bytes(data.size)
        assert rb == 256 and idx[61] // rb - (idx[1] + rb - 1) // rb >= 2
        return data, idx, expected(oracle, data, idx, k, s)
    data, idx, exp = cached("stretch", make)
    assert list(exp[1]) == [s] + [0] * 60 + [s]
    with which(kmc, lib):
        got = gpu_seq(kmc, cuda, data, idx, k, s)
    assert (got[1][1:61] == 0).all() and (got[0][1:61] == S.FILL).all()
    assert_sketch(got, exp)


def test_seq_long_record_over_three_ship_ranges(kmc, oracle, cuda):
    """The shipped walk gives a workgroup at most 1024 chunks = 16 384 bytes while the
    input has fewer than CUs x 16 KB, so a record of 3 x 16 384 + 100 bases spans at
    least three ranges (four here: 51 KB are cut into 4 ranges of 12.5 KB)."""
    rng = np.random.default_rng(14)
    range_bytes = 1024 * 16
    data, idx = pack([bases(rng, 1000), bases(rng, 3 * range_bytes + 100), bases(rng, 500)])
    for s in (1000, 5000):
        assert_sketch(gpu_seq(kmc, cuda, data, idx, 21, s), expected(oracle, data, idx, 21, s), "s=%d" % s)


# 6. addressing ----------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("shift", [1, 7, 15])
def test_seq_unaligned_data(kmc, oracle, cuda, lib, shift):
    data, idx = dirty_case()
    exp = cached(("dirty", 0), lambda: expected(oracle, data, idx, 11, 64, 0))
    with which(kmc, lib):
        assert_sketch(gpu_seq(kmc, cuda, data, idx, 11, 64, shift=shift), exp, "shift=%d" % shift)


@pytest.mark.parametrize("lib", LIBS)
def test_seq_first_offset_above_zero(kmc, oracle, cuda, lib):
    """indices[0] = 333: the bytes before it are never sketched."""
    rng = np.random.default_rng(15)
    data, idx = pack([bases(rng, 332), bases(rng, 1200), bases(rng, 30), bases(rng, 900)])
    sub = idx[1:]
    assert sub[0] == 333
    ek, _, eo = oracle.count_canonical(data, idx, 9)
    exp = S.sketch_expected(ek[int(eo[1]):], None, (eo[1:] - eo[1]).astype(np.uint64), sub.size - 1, 32)
    with which(kmc, lib):
        assert_sketch(gpu_seq(kmc, cuda, data, sub, 9, 32, shift=3), exp)


# 7. workspace -----------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_seq_caller_workspace(kmc, oracle, cuda, lib):
    import torch
    a = tiny_case()
    b = dirty_case()
    ea = cached("tiny16", lambda: expected(oracle, a[0], a[1], 15, 16))
    eb = cached("dirty15", lambda: expected(oracle, b[0], b[1], 15, 16))
    dv = cuda.index or 0
    with which(kmc, lib):
        need = max(kmc.sketch_from_sequences_workspace_size(x[1].size - 1, x[0].size, 16, dv) for x in (a, b))
        assert need > 0
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
        assert_sketch(gpu_seq(kmc, cuda, a[0], a[1], 15, 16, workspace=ws), ea, "prefilled workspace")
        # another input on the workspace the first call left behind, and back
        assert_sketch(gpu_seq(kmc, cuda, b[0], b[1], 15, 16, workspace=ws), eb, "second input")
        assert_sketch(gpu_seq(kmc, cuda, a[0], a[1], 15, 16, workspace=ws), ea, "first input again")
        assert_sketch(gpu_seq(kmc, cuda, a[0], a[1], 15, 16), ea, "library workspace")
        exact = kmc.sketch_from_sequences_workspace_size(a[1].size - 1, a[0].size, 16, dv)
        with pytest.raises(kmc.KmcError) as ei:
            gpu_seq(kmc, cuda, a[0], a[1], 15, 16, workspace=ws[: exact - 1])
        assert ei.value.code == 1004


def stale_case(oracle):
    """4096 bytes twice: one record over every range, then 41 records that cross other cuts
    (and a windowless one), alone and as 6 groups (one empty, one windowless)."""
    k, s = 21, 16
    def make():
        rng = np.random.default_rng(18)
        one = records_at(rng, [0], 4096)
        starts = [0] + sorted(int(x) for x in rng.choice(np.arange(30, 4000), size=39, replace=False)) + [4086]
        many = records_at(rng, starts, 4096)
        assert one[0].size == many[0].size == 4096 and diag_range_bytes(4096) == 256
        go = np.array([0, 0, 7, 8, 30, 40, 41], dtype=np.int64)
        return (one, expected(oracle, *one, k, s), many, expected(oracle, *many, k, s), go,
                GU.grouped_expected(oracle, *many, go, k, s))
    return cached("stale", make)


@pytest.mark.parametrize("lib", LIBS)
def test_seq_stale_workspace_of_another_layout(kmc, oracle, cuda, lib):
    """The first call leaves its partial sets and their sizes in every range's slots; the
    second call, on the same workspace and the same number of bytes, reads none of them."""
    import torch
    k, s = 21, 16
    one, exp_one, many, exp_many, go, exp_groups = stale_case(oracle)
    assert exp_one[1][0] == s and exp_many[1][-1] == 0 and list(exp_groups[1]) == [0, s, s, s, s, 0]
    dv = cuda.index or 0
    n = many[1].size - 1
    with which(kmc, lib):
        need = max(kmc.sketch_from_sequences_workspace_size(x, 4096, s, dv) for x in (1, n))
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
        assert_sketch(gpu_seq(kmc, cuda, *one, k, s, workspace=ws), exp_one, "one record")
        assert_sketch(gpu_seq(kmc, cuda, *many, k, s, workspace=ws), exp_many, "many records after one")
        # the same pair with the grouped call second
        need = max(need, kmc.sketch_from_sequences_grouped_workspace_size(n, go.size - 1, 4096, s, dv))
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
        assert_sketch(gpu_seq(kmc, cuda, *one, k, s, workspace=ws), exp_one, "one record again")
        d = torch.from_numpy(many[0]).to(cuda)
        di = torch.from_numpy(many[1]).to(cuda)
        got = kmc.sketch_from_sequences_grouped(d, di, torch.from_numpy(go).to(cuda), k, s, workspace=ws)
        torch.cuda.synchronize()
        assert_sketch((got[0].cpu().numpy().view(np.uint64), got[1].cpu().numpy().view(np.uint32)), exp_groups,
                      "groups after one record")


@pytest.mark.parametrize("lib", LIBS)
def test_seq_workspace_size_saturates(kmc, cuda, lib):
    dv = cuda.index or 0
    with which(kmc, lib):
        sizes = [kmc.sketch_from_sequences_workspace_size(100, b, 1000, dv)
                 for b in (0, 1, 1000, 10 ** 5, 10 ** 7, 10 ** 9, 1 << 36, 1 << 40)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] == sizes[-2] and sizes[0] < sizes[-1]


# 8. equivalence on the device -------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_seq_equals_the_two_step_path_on_random_fa(kmc, cuda, lib):
    import torch
    data, idx, _ = kmc.load_fasta(os.path.join(GOLDEN, "random.fa"))
    d = torch.from_numpy(np.ascontiguousarray(data)).to(cuda)
    di = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(cuda)
    with which(kmc, lib):
        for k, s in ((21, 64), (5, 1000)):
            two = kmc.sketch_from_counts(*kmc.count_canonical(d, di, k), s)
            one = kmc.sketch_from_sequences(d, di, k, s)
            torch.cuda.synchronize()
            assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]), (k, s)
            da = kmc.sketch_distances(*one, k, with_counts=True)
            db = kmc.sketch_distances(*two, k, with_counts=True)
            torch.cuda.synchronize()
            assert torch.equal(da[1], db[1]) and torch.equal(da[2], db[2])
