"""GPU parity of the screen (kmc_sketch_screen_build, _count, _results) against the CPU:
sketch_screen_util sums the canonical oracle's counts of every record of the mixture
per key and hashes the keys; shared and the median multiplicity of every reference row
are compared bit for bit, the identity as test_sketch_query_gpu compares distances.
Every case runs in libkmc.so and in libkmc_diag.so, whose 64-thread walking
workgroups, 256-byte ranges and table of two slots per value put a few thousand bases
through many ranges and long probe chains."""
import numpy as np
import pytest

import sketch_query_util as Q
import sketch_screen_util as U
import sketch_util as S
import stream_util as T
from sketch_screen_util import FWD, SOFT
from sketch_util import bases, dev, pack, which
from test_sketch_seq_gpu import diag_range_bytes

pytestmark = pytest.mark.gpu

LIBS = ["ship", "diag"]
cached = S.cache()
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def revcomp(x):
    return COMP[x][::-1]


def sketch_rows(kmc, cuda, data, idx, k, s, flags=0, seed=S.DEFAULT_SEED):
    """The rows of the records on the device (kmc_sketch_from_sequences) and on the host."""
    import torch
    d, di = U.device_records(cuda, data, idx)
    sk, sz = kmc.sketch_from_sequences(d, di, k, s, flags=flags, seed=seed)
    torch.cuda.synchronize()
    return sk, sz, sk.cpu().numpy().view(np.uint64), sz.cpu().numpy().view(np.uint32)


def device_rows(cuda, rows, sizes):
    return dev(np.asarray(rows, dtype=np.uint64).view(np.int64), cuda), dev(np.asarray(sizes, dtype=np.uint32).view(np.int32), cuda)


def screen(kmc, cuda, sk, sz, batches, k, flags=0, seed=S.DEFAULT_SEED, index=None, shift=0):
    """build, one count per batch (data, idx), results: (index, host results)."""
    import torch
    index = kmc.sketch_screen_build(sk, sz, index=index)
    for data, idx in batches:
        d, di = U.device_records(cuda, data, idx, shift)
        kmc.sketch_screen_count(index, d, di, k, flags=flags, seed=seed)
    res = kmc.sketch_screen_results(index, sk, sz, k)
    torch.cuda.synchronize()
    return index, U.host_results(res)


# 1. the general case -----------------------------------------------------------------
def general_case():
    """12 references; a mixture of four of them whole, two as halves, one as its reverse
    complement, one three times and 20 kbase of unrelated bases, cut into records at
    arbitrary places, with N and lowercase sprinkled in."""
    def make():
        rng = np.random.default_rng(900)
        lens = [300, 500, 800, 1200, 1500, 2000, 2500, 3000, 4000, 6000]
        refs = [bases(rng, L) for L in lens]
        refs.append(np.tile(bases(rng, 40), 10))  # 40 distinct forward 21-mers: fewer than s = 64
        refs.append(bases(rng, 15))               # no window: size 0
        masked = refs[2].copy()
        masked[100:160] |= 0x20                   # the mixture's copy has a soft-masked stretch
        parts = [refs[0], refs[1], masked, refs[3], refs[4][:750], refs[5][1000:], revcomp(refs[6]),
                 refs[7], refs[7], refs[7], refs[10], bases(rng, 20000)]
        order = rng.permutation(len(parts))
        mix = np.concatenate([np.concatenate([parts[i], np.full(1, ord("N"), np.uint8)]) for i in order])
        for _ in range(60):  # N and lowercase runs
            a = int(rng.integers(0, mix.size - 40))
            if rng.random() < 0.3:
                mix[a] = ord("N")
            else:
                mix[a:a + int(rng.integers(1, 40))] |= 0x20
        mix[mix == (ord("N") | 0x20)] = ord("N")
        cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(1, mix.size), size=25, replace=False)) + [mix.size]
        recs = [mix[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        recs.insert(5, bases(rng, 7))  # a record shorter than k
        recs.insert(9, bases(rng, 0))  # an empty record
        return pack(refs), pack(recs)
    return cached("general", make)


def general_mix(oracle, k, flags):
    _, (data, idx) = general_case()
    return cached(("general-mix", k, flags), lambda: U.mixture_hashes(oracle, data, idx, k, flags))


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("flags", [0, SOFT, FWD])
@pytest.mark.parametrize("s", [1, 64, 1000])
def test_screen_general(kmc, oracle, cuda, lib, s, flags):
    k = 21
    (rdata, ridx), (data, idx) = general_case()
    mix = general_mix(oracle, k, flags)
    with which(kmc, lib):
        sk, sz, rows, sizes = sketch_rows(kmc, cuda, rdata, ridx, k, s, flags)
        _, got = screen(kmc, cuda, sk, sz, [(data, idx)], k, flags)
    exp = U.screen_expected(mix, rows, sizes, s, k)
    assert sizes[11] == 0 and np.isnan(exp[2][11]) and exp[0][11] == 0
    if s == 64:
        assert sizes[10] < s
    if s == 1000:
        # (the cuts, N and lowercase cost the whole references a few windows each)
        assert (exp[0][[0, 1, 3, 7]] > 0.8 * sizes[[0, 1, 3, 7]]).all() and exp[1][7] == 3 and exp[1][0] == 1
        assert 0 < exp[0][4] < 0.7 * sizes[4] and 0 < exp[0][5] < 0.7 * sizes[5] and exp[0][8] == exp[0][9] == 0
        assert (exp[0][6] == 0) == (flags == FWD)  # the reverse complement shares nothing without the fold
        plain = U.screen_expected(general_mix(oracle, k, 0), rows, sizes, s, k)
        if flags == SOFT:  # the lowercase stretch counts only with the flag
            assert exp[0][2] >= plain[0][2] + 60
    U.assert_screen(got, exp, "s=%d flags=%d" % (s, flags))


# 2. key width edges ------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("k", [1, 15, 16, 31])
def test_screen_key_widths(kmc, oracle, cuda, lib, k):
    """k = 15 | 16: the one-dword / two-dword key instances; k = 1: two canonical keys,
    each with thousands of windows."""
    s = 100

    def make():
        rng = np.random.default_rng(910 + k)
        refs = [bases(rng, L) for L in (400, 900, 3000, 1500)]
        refs[3][:] = ord("C")  # at k = 1: a reference the mixture may lack nothing of
        mixrecs = [refs[0], bases(rng, 2500), refs[2][500:2500], bases(rng, k), bases(rng, max(k - 1, 0)),
                   bases(rng, 2500)]
        return pack(refs), pack(mixrecs)
    (rdata, ridx), (data, idx) = cached(("widths", k), make)
    with which(kmc, lib):
        for f in (0, FWD):
            mix = cached(("widths-mix", k, f), lambda: U.mixture_hashes(oracle, data, idx, k, f))
            sk, sz, rows, sizes = sketch_rows(kmc, cuda, rdata, ridx, k, s, f)
            _, got = screen(kmc, cuda, sk, sz, [(data, idx)], k, f)
            exp = U.screen_expected(mix, rows, sizes, s, k)
            assert exp[0][0] == sizes[0] > 0
            if k == 1:
                assert list(sizes) == ([2, 2, 2, 1] if f == 0 else [4, 4, 4, 1]) and exp[1][0] > 1000
            U.assert_screen(got, exp, "k=%d flags=%d" % (k, f))


# 3. accumulation ---------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_screen_accumulates_over_batches(kmc, oracle, cuda, lib):
    """Records [0, n/2), then [n/2, n) of the same buffer through two offset arrays equal
    one count of all of them; results between and after leave the index as it is;
    building again zeroes the multiplicities."""
    import torch
    k, s = 21, 64
    (rdata, ridx), (data, idx) = general_case()
    n = idx.size - 1
    h = n // 2
    mix = general_mix(oracle, k, 0)
    first = cached("accumulate-first", lambda: U.mixture_hashes(oracle, data, idx[:h + 1], k, 0))
    with which(kmc, lib):
        sk, sz, rows, sizes = sketch_rows(kmc, cuda, rdata, ridx, k, s)
        d, _ = U.device_records(cuda, data, idx)
        index = kmc.sketch_screen_build(sk, sz)
        kmc.sketch_screen_count(index, d, dev(idx[:h + 1], cuda), k)
        before = index.clone()
        half = U.host_results(kmc.sketch_screen_results(index, sk, sz, k))
        torch.cuda.synchronize()
        assert torch.equal(index, before), "results changed the index"
        kmc.sketch_screen_count(index, d, dev(idx[h:], cuda), k)
        two = U.host_results(kmc.sketch_screen_results(index, sk, sz, k))
        twice = index.clone()
        again = U.host_results(kmc.sketch_screen_results(index, sk, sz, k))
        torch.cuda.synchronize()
        assert torch.equal(index, twice)
        values = np.unique(np.concatenate([rows[r, :sizes[r]] for r in range(rows.shape[0])]))
        mults = U.index_multiplicities(kmc, index, values, cuda)
        _, one = screen(kmc, cuda, sk, sz, [(data, idx)], k)
        kmc.sketch_screen_build(sk, sz, index=index)
        zero = U.host_results(kmc.sketch_screen_results(index, sk, sz, k))
        torch.cuda.synchronize()
    exp = U.screen_expected(mix, rows, sizes, s, k)
    exp_half = U.screen_expected(first, rows, sizes, s, k)
    assert (exp_half[0] != exp[0]).any()
    U.assert_screen(half, exp_half, "first half")
    U.assert_screen(two, exp, "two batches")
    U.assert_screen(again, exp, "results twice")
    U.assert_screen(one, exp, "one batch")
    np.testing.assert_array_equal(mults, U.multiplicities(mix, values))
    assert (zero[0] == 0).all() and (zero[1] == 0).all()
    assert (zero[2][sizes > 0] == 0.0).all() and np.isnan(zero[2][sizes == 0]).all()


# 4. values that several references hold -----------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_screen_shared_values(kmc, oracle, cuda, lib):
    """Two identical references and two overlapping ones, every k-mer kept (s above the
    windows): a common value is indexed once, so it has one multiplicity for all."""
    k, s = 21, 4096

    def make():
        rng = np.random.default_rng(920)
        seq = bases(rng, 3000)
        refs = [seq[:2000], seq[:2000], seq[1000:], bases(rng, 800)]
        mixrecs = [seq, bases(rng, 3000), seq[500:1500], seq[1200:1300]]
        return pack(refs), pack(mixrecs)
    (rdata, ridx), (data, idx) = cached("shared", make)
    mix = cached("shared-mix", lambda: U.mixture_hashes(oracle, data, idx, k, 0))
    with which(kmc, lib):
        sk, sz, rows, sizes = sketch_rows(kmc, cuda, rdata, ridx, k, s)
        index, got = screen(kmc, cuda, sk, sz, [(data, idx)], k)
        per_row = [U.index_multiplicities(kmc, index, rows[r, :sizes[r]], cuda) for r in range(4)]
    exp = U.screen_expected(mix, rows, sizes, s, k)
    assert list(exp[0]) == [sizes[0], sizes[1], sizes[2], 0] and sizes[0] == 1980
    U.assert_screen(got, exp)
    np.testing.assert_array_equal(per_row[0], per_row[1])
    common, i0, i2 = np.intersect1d(rows[0, :sizes[0]], rows[2, :sizes[2]], return_indices=True)
    assert common.size == 980
    np.testing.assert_array_equal(per_row[0][i0], per_row[2][i2])
    assert set(per_row[0]) == {1, 2, 3}
    for r in range(4):
        np.testing.assert_array_equal(per_row[r], U.multiplicities(mix, rows[r, :sizes[r]]))


# 5. rows the index was not built from ---------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_screen_foreign_rows(kmc, oracle, cuda, lib):
    """results with another row set, of another sketch size: values not in the index are
    absent, whether the mixture holds them or not."""
    import torch
    k, s, s2 = 21, 64, 50
    (rdata, ridx), (data, idx) = general_case()
    mix = general_mix(oracle, k, 0)
    with which(kmc, lib):
        sk, sz, rows, sizes = sketch_rows(kmc, cuda, rdata, ridx, k, s)
        index, _ = screen(kmc, cuda, sk, sz, [(data, idx)], k)
        rng = np.random.default_rng(930)
        indexed = np.unique(np.concatenate([rows[r, :sizes[r]] for r in range(rows.shape[0])]))
        in_mix_only = np.setdiff1d(mix[0], indexed)[:500]  # hashes the mixture holds, the index does not
        lists = [np.concatenate([rng.choice(indexed, 20, replace=False), rng.choice(in_mix_only, 25, replace=False)]),
                 rng.choice(in_mix_only, s2, replace=False),
                 np.unique(rng.integers(1, 1 << 63, size=30, dtype=np.uint64)),
                 rows[0, :s2], []]
        frows, fsizes = Q.pack(lists, s2)
        fsk, fsz = device_rows(cuda, frows, fsizes)
        got = U.host_results(kmc.sketch_screen_results(index, fsk, fsz, k))
        torch.cuda.synchronize()
    only_indexed = (indexed, U.multiplicities(mix, indexed))
    exp = U.screen_expected(only_indexed, frows, fsizes, s2, k)
    assert exp[0][1] == 0 and exp[0][2] == 0 and 0 < exp[0][3] <= s2 and 0 < exp[0][0] <= 20 and np.isnan(exp[2][4])
    U.assert_screen(got, exp)


# 6. UINT64_MAX as a real hash ------------------------------------------------------------
def kmer_of(key, k):
    """The bases of a forward key (first base most significant)."""
    return np.frombuffer(b"ACGT", dtype=np.uint8)[[(int(key) >> (2 * (k - 1 - p))) & 3 for p in range(k)]]


@pytest.mark.parametrize("lib", LIBS)
def test_screen_uint64_max_is_a_value(kmc, oracle, cuda, lib):
    """k = 31, KMC_CANON_FORWARD, seed 42: unhash(UINT64_MAX) is below 2^62, the key of a
    31-mer.  A row that holds UINT64_MAX within its size finds it in a mixture with that
    31-mer (twice) and not in one without; a row that ends before it does not."""
    k, seed, s = 31, 42, 8
    key = int(S.unhash(np.array([S.FILL]), seed)[0])
    assert key == 0x31628af67b213181 and key < 1 << 62

    def make():
        rng = np.random.default_rng(940)
        mer = kmer_of(key, k)
        others = [bases(rng, 31) for _ in range(3)]
        with_it = pack([np.concatenate([others[0], others[1]]), mer, bases(rng, 300), np.concatenate([others[2], mer])])
        without = pack([np.concatenate([others[0], others[1]]), bases(rng, 300), others[2], mer[:30], mer[1:]])
        keys = [int("".join(str(b"ACGT".index(c)) for c in bytes(o)), 4) for o in others]
        return with_it, without, S.hash_keys(np.array(keys, dtype=np.uint64), seed)
    with_it, without, oh = cached("ffff", make)
    rows = np.full((3, s), S.FILL, dtype=np.uint64)
    rows[0, :3] = np.sort(oh)
    rows[1, :3] = np.sort(oh)
    rows[2, :1] = np.sort(oh)[:1]
    sizes = np.array([4, 3, 2], dtype=np.uint32)  # rows 0 and 2 hold UINT64_MAX within their size, row 1 ends before it
    with which(kmc, lib):
        sk, sz = device_rows(cuda, rows, sizes)
        for name, (data, idx), found in (("with", with_it, 1), ("without", without, 0)):
            mix = U.mixture_hashes(oracle, data, idx, k, FWD, seed)
            assert (mix[0][-1] == S.FILL) == bool(found) and (not found or mix[1][-1] == 2)
            _, got = screen(kmc, cuda, sk, sz, [(data, idx)], k, FWD, seed)
            exp = U.screen_expected(mix, rows, sizes, s, k)
            assert list(exp[0]) == [3 + found, 3, 1 + found], name
            U.assert_screen(got, exp, name)
        # an index without it: the mixture's UINT64_MAX windows count nowhere
        index, got = screen(kmc, cuda, sk[1:2], sz[1:2], [with_it], k, FWD, seed)
        assert list(got[0]) == [3]
        assert list(U.index_multiplicities(kmc, index, [S.FILL], cuda)) == [0]


# 7. long and wrapping probe chains ---------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_screen_colliding_values(kmc, oracle, cuda, lib):
    """200 values that agree in their low 32 bits and 200 that agree in their high 32 bits:
    whatever bits the slot function takes, one set collides throughout (with the low
    bits, 0xFFFFFFF4: a chain of 200 that starts 12 slots before the table's end and
    wraps).  All are hashes (seed 42) of keys below 2^62, so at k = 31 FORWARD the
    mixture holds exactly every other one, each as a record of its own."""
    k, seed, s = 31, 42, 200

    def make():
        rng = np.random.default_rng(950)
        low = (np.arange(1, 2000, dtype=np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFF4)
        high = (np.uint64(0x0000ABCD) << np.uint64(32)) | (np.arange(1, 2000, dtype=np.uint64) * np.uint64(3))
        sets = []
        for cand in (low, high):
            keys = S.unhash(cand, seed)
            ok = keys < np.uint64(1 << 62)
            assert ok.sum() >= s
            sets.append((cand[ok][:s], keys[ok][:s]))
        recs = [kmer_of(key, k) for _, keys in sets for key in keys[::2]]
        recs += [bases(rng, 31) for _ in range(50)]
        order = rng.permutation(len(recs))
        return sets, pack([recs[i] for i in order])
    sets, (data, idx) = cached("collide", make)
    rows, sizes = Q.pack([sets[0][0], sets[1][0]], s)
    mix = cached("collide-mix", lambda: U.mixture_hashes(oracle, data, idx, k, FWD, seed))
    exp = U.screen_expected(mix, rows, sizes, s, k)
    assert list(exp[0]) == [100, 100] and list(exp[1]) == [1, 1]
    with which(kmc, lib):
        sk, sz = device_rows(cuda, rows, sizes)
        index, got = screen(kmc, cuda, sk, sz, [(data, idx)], k, FWD, seed)
        U.assert_screen(got, exp)
        for r in range(2):  # exactly the chosen half, no false hit
            np.testing.assert_array_equal(U.index_multiplicities(kmc, index, rows[r], cuda), np.tile([1, 0], 100))


# 8. contention ------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_screen_one_value_many_windows(kmc, oracle, cuda, lib):
    """One record of 20 000 A at k = 21: 19 980 windows add to one multiplicity."""
    k, s = 21, 4
    data, idx = pack([np.full(20000, ord("A"), np.uint8)])
    rows, sizes = Q.pack([S.hash_keys(np.array([0], dtype=np.uint64)), [3, 5, 1 << 40]], s)
    mix = cached("all-a-mix", lambda: U.mixture_hashes(oracle, data, idx, k, 0))
    exp = U.screen_expected(mix, rows, sizes, s, k)
    assert list(exp[0]) == [1, 0] and list(exp[1]) == [19980, 0] and list(exp[2]) == [1.0, 0.0]
    with which(kmc, lib):
        _, got = screen(kmc, cuda, *device_rows(cuda, rows, sizes), [(data, idx)], k)
    U.assert_screen(got, exp)


# 9. range cuts -------------------------------------------------------------------------------
def cuts_case():
    """24 ranges of 256 bytes (the diag walk's).  Range R = 1..22 holds a record of exactly
    21 bases that starts at its byte 234 + R (235..256: the last one on the next range's
    first byte), so the 21-mer ends at the record's terminator, beyond the cut; every
    other record is shorter than k."""
    def make():
        rng = np.random.default_rng(960)
        k = 21
        recs, at, mers = [], 0, []
        for R in range(1, 23):
            start = 256 * R + 234 + R
            while at < start:  # records of at most 14 bases up to the start
                n = min(start - at, 15)
                recs.append(bases(rng, n - 1))
                at += n
            mers.append(bases(rng, k))
            recs.append(mers[-1])
            at += k + 1
        while at < 24 * 256:
            n = min(24 * 256 - at, 15)
            recs.append(bases(rng, n - 1))
            at += n
        data, idx = pack(recs)
        assert data.size == 24 * 256 and diag_range_bytes(data.size) == 256
        starts = idx[:-1][np.diff(idx) == k + 1]
        assert list(starts % 256)[:21] == list(range(235, 256)) and starts[21] % 256 == 0 and starts.size == 22
        return data, idx, mers
    return cached("cuts", make)


@pytest.mark.parametrize("lib", LIBS)
def test_screen_windows_on_range_cuts(kmc, oracle, cuda, lib):
    k, s = 21, 32
    data, idx, mers = cuts_case()
    mix = cached("cuts-mix", lambda: U.mixture_hashes(oracle, data, idx, k, 0))
    assert mix[0].size == 22 and (mix[1] == 1).all()
    rng = np.random.default_rng(961)
    rows, sizes = Q.pack([mix[0], mix[0][::3], np.unique(rng.integers(1, 1 << 63, size=s, dtype=np.uint64))], s)
    exp = U.screen_expected(mix, rows, sizes, s, k)
    assert list(exp[0]) == [22, 8, 0] and list(exp[1]) == [1, 1, 0]
    with which(kmc, lib):
        index, got = screen(kmc, cuda, *device_rows(cuda, rows, sizes), [(data, idx)], k)
        U.assert_screen(got, exp)
        assert (U.index_multiplicities(kmc, index, mix[0], cuda) == 1).all(), "each is found exactly once"


# 10. addressing ------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("shift", [1, 7, 15])
def test_screen_unaligned_data(kmc, oracle, cuda, lib, shift):
    k, s = 21, 64
    (rdata, ridx), (data, idx) = general_case()
    mix = general_mix(oracle, k, 0)
    with which(kmc, lib):
        sk, sz, rows, sizes = sketch_rows(kmc, cuda, rdata, ridx, k, s)
        _, got = screen(kmc, cuda, sk, sz, [(data, idx)], k, shift=shift)
    U.assert_screen(got, U.screen_expected(mix, rows, sizes, s, k), "shift=%d" % shift)


@pytest.mark.parametrize("lib", LIBS)
def test_screen_first_offset_above_zero(kmc, oracle, cuda, lib):
    """indices[0] > 0: the bytes before it are never counted."""
    k, s = 21, 64
    (rdata, ridx), (data, idx) = general_case()
    sub = idx[3:]
    assert sub[0] > 0
    rest = cached("offset-mix", lambda: U.mixture_hashes(oracle, data, idx, k, 0, first=3))
    with which(kmc, lib):
        sk, sz, rows, sizes = sketch_rows(kmc, cuda, rdata, ridx, k, s)
        _, got = screen(kmc, cuda, sk, sz, [(data, sub)], k, shift=3)
    exp = U.screen_expected(rest, rows, sizes, s, k)
    assert (exp[0] != U.screen_expected(general_mix(oracle, k, 0), rows, sizes, s, k)[0]).any()
    U.assert_screen(got, exp)


# 11. what a former use left in the blob --------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_screen_stale_index(kmc, oracle, cuda, lib):
    """build reads nothing of the blob: 0xFF bytes, and the counted index of another
    shape (more and other values, another slot count) give the results of a fresh one."""
    import torch
    k, s = 21, 64
    (rdata, ridx), (data, idx) = general_case()
    mix = general_mix(oracle, k, 0)
    with which(kmc, lib):
        sk, sz, rows, sizes = sketch_rows(kmc, cuda, rdata, ridx, k, s)
        big_sk, big_sz, _, _ = sketch_rows(kmc, cuda, data, idx, k, 1000)  # the mixture's own records, s = 1000
        need = max(kmc.sketch_screen_index_size(rows.shape[0], s), kmc.sketch_screen_index_size(idx.size - 1, 1000))
        assert need > kmc.sketch_screen_index_size(rows.shape[0], s)
        blob = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
        exp = U.screen_expected(mix, rows, sizes, s, k)
        _, got = screen(kmc, cuda, sk, sz, [(data, idx)], k, index=blob)
        U.assert_screen(got, exp, "0xFF")
        screen(kmc, cuda, big_sk, big_sz, [(data, idx)], k, index=blob)
        _, got = screen(kmc, cuda, sk, sz, [(data, idx)], k, index=blob)
        U.assert_screen(got, exp, "after an index of another shape")
        blob.zero_()
        _, got = screen(kmc, cuda, sk, sz, [(data, idx)], k, index=blob)
        U.assert_screen(got, exp, "zeros")
        with pytest.raises(kmc.KmcError) as ei:
            kmc.sketch_screen_build(sk, sz, index=blob[:kmc.sketch_screen_index_size(rows.shape[0], s) - 256])
        assert ei.value.code == 1004


# 12. the stream -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delay(kmc, cuda):
    kmc.lib()
    cycles, ms = T.sleep_cycles(T.DELAY_MS)
    assert ms >= 0.9 * T.DELAY_MS, "the delay spins %.1f ms, not %.1f" % (ms, T.DELAY_MS)
    return cycles


@pytest.fixture(scope="module")
def streams(kmc, cuda, delay):
    return T.side_streams(kmc, cuda, delay)


def check_screen(got, exp, msg):
    U.assert_screen((got[0].view(np.uint32), got[1].view(np.uint32), got[2]), exp, msg)


def flat(exp):
    return tuple(exp)


def outputs(cuda, n):
    import torch
    return [torch.empty(n, dtype=torch.int32, device=cuda), torch.empty(n, dtype=torch.int32, device=cuda),
            torch.empty(n, dtype=torch.float32, device=cuda)]


def case_count(kmc, oracle, cuda):
    """The records arrive late; the index is built, counted into and read on the stream."""
    import torch
    k, s = 21, 64
    real, decoy = T.records(71, T.LENS_REAL), T.records(72, T.LENS_DECOY)
    assert real[0].size == decoy[0].size
    rk, _, ro = oracle.count_canonical(real[0], real[1], k)
    rows, sizes = S.sketch_expected(rk, None, ro, real[1].size - 1, s)
    sk, sz = device_rows(cuda, rows, sizes)
    exp = {w: U.screen_expected(U.mixture_hashes(oracle, x[0], x[1], k), rows, sizes, s, k)
           for w, x in (("real", real), ("decoy", decoy))}
    d_live = torch.zeros(real[0].size + 16, dtype=torch.uint8, device=cuda)[:real[0].size]
    i_live = torch.zeros(real[1].size, dtype=torch.int64, device=cuda)
    ins = [(d_live, dev(decoy[0], cuda), dev(real[0], cuda)), (i_live, dev(decoy[1], cuda), dev(real[1], cuda))]
    outs = outputs(cuda, rows.shape[0])
    index = torch.zeros(kmc.sketch_screen_index_size(rows.shape[0], s), dtype=torch.uint8, device=cuda)

    def run(which_, stream):
        kmc.sketch_screen_build(sk, sz, index=index, stream=stream)
        kmc.sketch_screen_count(index, d_live, i_live, k, stream=stream)
        kmc.sketch_screen_results(index, sk, sz, k, out=tuple(outs), stream=stream)
    return T.Call("sketch_screen_count", ins, outs, run, exp, check_screen, flat, ws=index)


def case_results(kmc, oracle, cuda):
    """The rows arrive late; the index is built and counted into beforehand."""
    import torch
    k, s = 21, 64
    data, idx = T.records(73, T.LENS_REAL)
    keys, _, off = oracle.count_canonical(data, idx, k)
    rows, sizes = S.sketch_expected(keys, None, off, idx.size - 1, s)
    decoy_rows, decoy_sizes = rows[::-1].copy(), sizes[::-1].copy()
    decoy_rows[0, :8] = np.arange(1, 9)  # (values the mixture lacks: the two results differ)
    decoy_sizes[0] = 8
    sk, sz = device_rows(cuda, rows, sizes)
    index, _ = screen(kmc, cuda, sk, sz, [(data, idx)], k)
    mix = U.mixture_hashes(oracle, data, idx, k)
    exp = {"real": U.screen_expected(mix, rows, sizes, s, k),
           "decoy": U.screen_expected(mix, decoy_rows, decoy_sizes, s, k)}
    r_live, s_live = torch.zeros_like(sk), torch.zeros_like(sz)
    ins = [(r_live, device_rows(cuda, decoy_rows, decoy_sizes)[0], sk),
           (s_live, device_rows(cuda, decoy_rows, decoy_sizes)[1], sz)]
    outs = outputs(cuda, rows.shape[0])

    def run(which_, stream):
        kmc.sketch_screen_results(index, r_live, s_live, k, out=tuple(outs), stream=stream)
    return T.Call("sketch_screen_results", ins, outs, run, exp, check_screen, flat)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("make", [case_count, case_results], ids=["count", "results"])
def test_screen_late_input_on_a_side_stream(kmc, oracle, cuda, delay, streams, lib, make):
    with which(kmc, lib):
        T.late_call(make(kmc, oracle, cuda), streams[0], delay)
