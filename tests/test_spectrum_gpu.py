"""GPU parity of kmc_spectrum_from_accum (kmc.SketchAccum.spectrum) against the CPU.
The expected hist and stats of every case are spectrum_util.model's: the bincount of
the oracle's exact multiplicities (sketch_screen_util.mixture_hashes) of the hashes
below the limit the device reports, which check_limit holds against the level's bound
as test_sketch_accum_gpu.check does.  hist and stats are compared exactly.  Every case
runs in libkmc.so and in libkmc_diag.so."""
import numpy as np
import pytest

import sketch_screen_util as U
import sketch_util as S
import spectrum_util as P
import stream_util as T
from sketch_screen_util import FWD, SOFT
from sketch_util import bases, dev, pack, which
from test_sketch_accum_gpu import (FILL, LIBS, NSEP, PURGE_LG, add, bound, finish, level, mixture, planted_case,
                                   purge_case, purge_levels, purge_seed, records_case, roomy)

pytestmark = pytest.mark.gpu

INVALID = 1001
cached = S.cache()


def spectrum(acc, B, **kw):
    """(hist uint64 [B], stats [4] Python ints or None) of acc.spectrum(B)."""
    import torch
    hist, stats = acc.spectrum(B, **kw)
    torch.cuda.synchronize()
    return P.host(hist, stats)


def check(got, mix, B, j, msg, lossless=None):
    """hist and stats equal the model's at the device's limit; returns the stats."""
    hist, stats = got
    limit, everything = P.check_limit(stats, j, lossless)
    ehist, estats = P.model(mix, limit, everything, B)
    print("%s: B=%d j=%d stats=%s, %d bins in use" % (msg, B, j, stats, int((hist > 0).sum())))
    assert hist.shape == (B,), msg
    np.testing.assert_array_equal(hist, ehist, err_msg="%s hist" % msg)
    assert stats == estats, "%s: stats %s, expected %s" % (msg, stats, estats)
    assert int(hist.sum()) == stats[2], msg
    return stats


# 1. the exact spectrum ------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("flags", [0, SOFT, FWD])
@pytest.mark.parametrize("k", [1, 5, 16, 31])
def test_exact_spectrum(kmc, oracle, cuda, lib, k, flags):
    data, idx = records_case()
    mix = mixture(oracle, ("records-mix", k, flags), [(data, idx)], k, flags)
    h, c = mix
    with which(kmc, lib):
        with kmc.SketchAccum(64, k, flags=flags, log2_slots=roomy(data.size)) as acc:
            add(kmc, cuda, acc, (data, idx), shift=1)
            got = {B: spectrum(acc, B) for B in (2, 16, 300, 8192)}
    for B, g in got.items():
        stats = check(g, mix, B, 0, "k=%d flags=%d B=%d" % (k, flags, B), lossless=True)
        assert stats == [1, FILL, h.size, int(c.sum())]  # every distinct key, every valid window
        np.testing.assert_array_equal(g[0], np.bincount(np.minimum(c, B - 1), minlength=B).astype(np.uint64))
    if k == 1:
        assert int(c.max()) >= 300 and got[300][0][299] > 0  # counts beyond the bins: the last one took them


# 2. the saturation edge -----------------------------------------------------------------
def short_case():
    return cached("short", lambda: pack([bases(np.random.default_rng(41), 26)]))


def poly_case(windows, k):
    return pack([np.full(windows + k - 1, ord("A"), np.uint8)])


@pytest.mark.parametrize("lib", LIBS)
def test_saturation_edge(kmc, oracle, cuda, lib):
    k = 21
    batch = short_case()
    one = mixture(oracle, "short-mix", [batch], k)
    assert one[0].size == 6 and (one[1] == 1).all()  # six distinct keys, once each
    with which(kmc, lib):
        with kmc.SketchAccum(16, k, log2_slots=roomy(8 * batch[0].size)) as acc:
            for n in range(1, 9):
                add(kmc, cuda, acc, batch)
                if n >= 6:
                    mix = (one[0], one[1] * n)
                    stats = check(spectrum(acc, 8), mix, 8, 0, "n=%d B=8" % n, lossless=True)
                    hist = spectrum(acc, 8)[0]
                    assert hist[min(n, 7)] == 6 and int(hist.sum()) == 6 and stats[3] == 6 * n
                    two = spectrum(acc, 2)
                    check(two, mix, 2, 0, "n=%d B=2" % n, lossless=True)
                    assert list(two[0]) == [0, 6] and two[1][3] == 6 * n
        for windows in (8000, 8191, 9000):  # one key: at its count, in the last bin, beyond it
            batch = poly_case(windows, k)
            mix = mixture(oracle, ("poly-mix", windows), [batch], k)
            assert mix[0].size == 1 and int(mix[1][0]) == windows
            with kmc.SketchAccum(16, k, log2_slots=roomy(batch[0].size)) as acc:
                add(kmc, cuda, acc, batch)
                hist, stats = spectrum(acc, 8192)
                check((hist, stats), mix, 8192, 0, "poly %d" % windows, lossless=True)
                assert hist[min(windows, 8191)] == 1 and stats[2:] == [1, windows]  # the sum is not truncated


# 3. tiny and large tables ---------------------------------------------------------------
def table_case(n):
    def make():
        rng = np.random.default_rng(42 + n)
        return pack([bases(rng, x) for x in (n // 3, 0, n - n // 3)])
    return cached(("table", n), make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("lg,n", [(4, 4), (4, 14), (8, 60), (8, 700), (21, 5000)])
def test_tiny_and_large_tables(kmc, oracle, cuda, lib, lg, n):
    """16 slots: less than a workgroup's threads; 2^21: above 4096 workgroups of 256, so
    the grid-stride loop runs twice."""
    k = 3 if lg == 4 else 21
    batch = table_case(n)
    mix = mixture(oracle, ("table-mix", n, k), [batch], k)
    j = level(batch[0].size, lg)
    assert (j == 0) == ((lg, n) in ((8, 60), (21, 5000)))
    with which(kmc, lib):
        with kmc.SketchAccum(4, k, log2_slots=lg) as acc:
            add(kmc, cuda, acc, batch)
            got = [spectrum(acc, B) for B in (4, 256)]
            _, _, fstats = finish(acc, 1)
    for B, g in zip((4, 256), got):
        stats = check(g, mix, B, j, "lg=%d n=%d B=%d" % (lg, n, B), lossless=True if j == 0 else None)
        assert stats[1:3] == fstats[1:3]
    if lg == 21:
        assert got[1][1][2] == mix[0].size > 4000


# 4. sampled: the spectrum after every add of a table that purges -------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_sampled_spectrum_through_purges(kmc, oracle, cuda, lib):
    k, s, B = 21, 16, 8
    batches, js = purge_case(), purge_levels()
    assert js == [7, 8, 9, 10]  # three purges
    seed = purge_seed(oracle, k, s)
    seen = []
    with which(kmc, lib):
        with kmc.SketchAccum(s, k, seed=seed, log2_slots=PURGE_LG) as acc:
            for i, b in enumerate(batches):
                add(kmc, cuda, acc, b)
                mix = mixture(oracle, ("purge-mix", seed, i), batches[:i + 1], k, 0, seed)
                stats = check(spectrum(acc, B), mix, B, js[i], "call %d" % i, lossless=True)
                _, _, fstats = finish(acc, 1)
                assert stats[0] == 0 and stats[1] == bound(js[i]) and stats[2] == fstats[2] > 0
                again = spectrum(acc, B)
                assert again[1] == stats
                seen.append(again[0])
    assert seen[-1][2] > seen[-1][1]  # almost every key ends with multiplicity 2 (purge_case)


# 5. lossy: more distinct keys below the bound than half the table ------------------------
def lossy_case(lg):
    """FORWARD 8-mers chosen by their hash (below 2^56, so below the bound of the level
    these few hundred bytes reach), 1 to 3 times each, separated by N: more of them than
    C / 2, so inserts are refused and `lost` bounds the limit."""
    def make():
        k, C = 8, 1 << lg
        keys = np.arange(1 << 16, dtype=np.uint64)
        h = S.hash_keys(keys)
        pick = np.nonzero(h < np.uint64(1 << 56))[0][:C // 2 + C // 4]
        assert pick.size == C // 2 + C // 4
        parts = []
        for i, x in enumerate(pick):
            km = np.frombuffer(b"ACGT", np.uint8)[[(int(x) >> (2 * (k - 1 - p))) & 3 for p in range(k)]]
            parts += [km, NSEP] * (i % 3 + 1)
        third = len(parts) // 3 // 2 * 2
        return pack([np.concatenate(parts[:third]), np.concatenate(parts[third:])]), np.sort(h[pick])
    return cached(("lossy", lg), make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("lg", [4, 5, 6])
def test_lossy_spectrum(kmc, oracle, cuda, lib, lg):
    k, B = 8, 4
    batch, chosen = lossy_case(lg)
    mix = mixture(oracle, ("lossy-mix", lg), [batch], k, FWD)
    np.testing.assert_array_equal(mix[0], chosen)
    assert sorted(set(int(x) for x in mix[1])) == [1, 2, 3]
    j = level(batch[0].size, lg)
    assert 0 < j <= 8 and (chosen < np.uint64(bound(j))).all() and chosen.size > (1 << lg) // 2
    with which(kmc, lib):
        with kmc.SketchAccum(2, k, flags=FWD, log2_slots=lg) as acc:
            add(kmc, cuda, acc, batch)
            got = spectrum(acc, B)
            _, _, fstats = finish(acc, 1)
    stats = check(got, mix, B, j, "lg=%d" % lg, lossless=False)
    assert (stats[1] & (stats[1] - 1)) != 0  # a lost hash, not a level's bound
    assert stats[1:3] == fstats[1:3] and stats[2] <= (1 << lg) // 2


# 6. no side effects ---------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_spectrum_leaves_the_accumulator_alone(kmc, oracle, cuda, lib):
    k, s, B = 21, 64, 8
    batch = planted_case()
    mix = mixture(oracle, "planted-mix", [batch], k)
    lg = roomy(2 * batch[0].size)  # (the batch is added twice below)
    with which(kmc, lib):
        with kmc.SketchAccum(s, k, log2_slots=lg) as plain:
            add(kmc, cuda, plain, batch)
            rows = [finish(plain, m) for m in (1, 2)]
        with kmc.SketchAccum(s, k, log2_slots=lg) as acc:
            empty = spectrum(acc, B)  # before any add
            add(kmc, cuda, acc, batch)
            before = spectrum(acc, B)
            got = []
            for m in (1, 2):
                got.append(finish(acc, m))
                after = spectrum(acc, B)
                np.testing.assert_array_equal(after[0], before[0])
                assert after[1] == before[1]
            acc.reset()
            cleared = spectrum(acc, B)
            add(kmc, cuda, acc, batch)  # add, spectrum, add, spectrum, finish, spectrum
            once = spectrum(acc, B)
            add(kmc, cuda, acc, batch)
            twice = spectrum(acc, B)
            finish(acc, 2)
            last = spectrum(acc, B)
    check(before, mix, B, 0, "before", lossless=True)
    assert set(range(1, 6)) <= set(np.nonzero(before[0])[0].tolist())  # multiplicities 1 .. 5 are planted
    for g, e in zip(got, rows):  # finish's row after a spectrum is the row without one
        np.testing.assert_array_equal(g[0], e[0])
        assert g[1] == e[1] and g[2] == e[2]
    for g in (empty, cleared):
        assert not g[0].any() and g[1] == [1, FILL, 0, 0]
    check(once, mix, B, 0, "once", lossless=True)
    check(twice, (mix[0], mix[1] * 2), B, 0, "twice", lossless=True)
    np.testing.assert_array_equal(last[0], twice[0])
    assert last[1] == twice[1]


# 7. arguments on a live handle ----------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_spectrum_arguments(kmc, oracle, cuda, lib):
    import ctypes
    import torch
    k = 21
    batch = short_case()
    mix = mixture(oracle, "short-mix", [batch], k)
    buf = (ctypes.c_char * 64)()
    host = ctypes.c_void_p(ctypes.addressof(buf))  # never dereferenced: the arguments are judged first
    with which(kmc, lib) as D:
        L = D if lib == "diag" else kmc.lib()
        with kmc.SketchAccum(16, k, log2_slots=roomy(batch[0].size)) as acc:
            add(kmc, cuda, acc, batch)
            f = L.kmc_spectrum_from_accum
            assert f(acc._h, 256, None, host, None) == INVALID
            for B in (0, 1, 8193):
                assert f(acc._h, B, host, host, None) == INVALID, B
                with pytest.raises(kmc.KmcError):
                    acc.spectrum(B)
            without = spectrum(acc, 8, stats=False)  # null stats: accepted
            assert without[1] is None
            own = (torch.full((8,), -1, dtype=torch.int64, device=cuda), torch.zeros(4, dtype=torch.int64, device=cuda))
            hist, stats = acc.spectrum(8, stats=own[1], out=own[0])
            assert hist is own[0] and stats is own[1]
            torch.cuda.synchronize()
            got = P.host(hist, stats)
        with pytest.raises(ValueError):
            acc.spectrum(8)  # closed
    check(got, mix, 8, 0, "own tensors", lossless=True)
    np.testing.assert_array_equal(without[0], got[0])


# 8. a side stream -----------------------------------------------------------------------
STREAM_LENS = [0, 5, 900, 3000, 1, 40]


def test_spectrum_on_a_side_stream(kmc, oracle, cuda):
    """stream_util's late input: the accumulator is emptied, takes the records and gives
    its spectrum, all on a side stream behind a delay, while the record buffers still
    hold a decoy.  Work the library put on another stream would read the decoy or the
    empty table, or miss the snapshot."""
    import torch
    k, B = 16, 32
    kmc.lib()
    cycles, _ = T.sleep_cycles(T.DELAY_MS)
    s, _ = T.side_streams(kmc, cuda, cycles)
    pair = (T.records(5, STREAM_LENS[::-1]), T.records(6, STREAM_LENS))
    ins = [(dev(d, cuda), dev(d, cuda), dev(r, cuda)) for d, r in zip(*pair)]  # (live, decoy, real) of data and offsets
    hist = torch.empty(B, dtype=torch.int64, device=cuda)
    stats = torch.empty(4, dtype=torch.int64, device=cuda)

    def expected(w):
        return P.model(mixture(oracle, ("stream-mix", w), [pair[w]], k), FILL, True, B)
    exp = {"decoy": expected(0), "real": expected(1)}

    def compare(got, e, msg):
        np.testing.assert_array_equal(got[0].view(np.uint64), e[0], err_msg=msg)
        assert [int(x) for x in got[1].view(np.uint64)] == e[1], msg

    with kmc.SketchAccum(16, k, log2_slots=roomy(pair[0][0].size)) as acc:
        def run(w, st):
            acc.reset(stream=st)
            acc.add(ins[0][0], ins[1][0], stream=st)
            acc.spectrum(B, stats=stats, out=hist, stream=st)
        call = T.Call("spectrum", ins, [hist, stats], run, exp, compare, lambda e: (e[0], np.array(e[1], dtype=np.uint64)))
        T.late_call(call, s, cycles)
