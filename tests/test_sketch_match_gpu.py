"""GPU parity of kmc_match_from_accum (kmc.SketchAccum.match) against the CPU.  The
expected windows, sampled, hits and stats of every case are sketch_match_util.model's:
the oracle's per-record keys and counts, looked up in the oracle's multiset of what was
added, at the limit the device reports, which spectrum_util.check_limit holds against
the level's bound.  Everything is compared exactly.  The outputs are filled with 0xFF
before every call, so a record the kernel skipped shows.  Every case runs in libkmc.so
and in libkmc_diag.so, where a wave's range is 256 bytes."""
import numpy as np
import pytest

import sketch_match_util as M
import sketch_screen_util as U
import sketch_util as S
import spectrum_util as P
import stream_util as T
from sketch_screen_util import FWD, SOFT
from sketch_util import bases, dev, pack, which
from test_sketch_accum_gpu import (EMPTY, FILL, LIBS, LOST_LG, NSEP, PURGE_LG, add, bound, finish, level, lost_case,
                                   mixture, planted_case, purge_case, purge_levels, purge_seed, records_case, roomy)

pytestmark = pytest.mark.gpu

INVALID, OK = 1001, 0
cached = S.cache()


def match(cuda, acc, batch, shift=0, m=1, **kw):
    """The host copies of acc.match over `batch`, the outputs filled with 0xFF first."""
    import torch
    data, idx = batch
    d, di = U.device_records(cuda, data, idx, shift)
    n = idx.size - 1
    own = [torch.full((n,), -1, dtype=torch.int32, device=cuda) for _ in range(3)]
    st = torch.full((4,), -1, dtype=torch.int64, device=cuda)
    res = acc.match(d, di, m, windows=own[0], sampled=own[1], stats=st, out=own[2], **kw)
    assert res[0] is own[0] and res[1] is own[1] and res[2] is own[2] and res[3] is st
    torch.cuda.synchronize()
    return M.host(res)


def check(oracle, got, batch, k, mix, j, msg, m=1, flags=0, seed=S.DEFAULT_SEED, lossless=None):
    """The outputs equal the model's at the device's limit; returns the model's."""
    limit, everything = P.check_limit(got[3], j, lossless)
    exp = M.model(oracle, batch[0], batch[1], k, mix, limit, everything, m, flags, seed)
    print("%s: j=%d stats=%s, %d records, %d with hits" % (msg, j, got[3], got[2].size, int((got[2] > 0).sum())))
    M.assert_match(got, exp, msg)
    return exp


# 1. self-match --------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("flags", [0, SOFT, FWD])
@pytest.mark.parametrize("k", [1, 5, 16, 31])
def test_self_match(kmc, oracle, cuda, lib, k, flags):
    batch = records_case()
    mix = mixture(oracle, ("records-mix", k, flags), [batch], k, flags)
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, flags=flags, log2_slots=roomy(batch[0].size)) as acc:
            add(kmc, cuda, acc, batch, shift=1)
            got = match(cuda, acc, batch, shift=1)
    exp = check(oracle, got, batch, k, mix, 0, "k=%d flags=%d" % (k, flags), flags=flags, lossless=True)
    np.testing.assert_array_equal(got[2], got[1])
    np.testing.assert_array_equal(got[1], got[0])
    total = int(exp[0].astype(np.int64).sum())
    assert got[3] == [1, FILL, total, total] and total == int(mix[1].sum())
    assert total > 0 or (k == 31 and flags != SOFT)  # (N and lowercase: only SOFT leaves a run of 31 bases)


# 2. foreign reads -----------------------------------------------------------------------
def foreign_case():
    """A set of 6 records and 40 reads of 20 .. 200 bases: copies of pieces of the set,
    fresh ones, and copies with one to three point mutations (each kills up to k windows)."""
    def make():
        rng = np.random.default_rng(51)
        refs = [bases(rng, n) for n in (700, 1200, 333, 64, 2000, 150)]
        reads = []
        for i in range(40):
            n = int(rng.integers(20, 201))
            src = refs[int(rng.integers(0, len(refs)))]
            if i % 3 == 1 or src.size < n:
                reads.append(bases(rng, n))
                continue
            a = int(rng.integers(0, src.size - n + 1))
            rd = src[a:a + n].copy()
            if i % 3 == 2:
                for p in rng.integers(0, n, size=int(rng.integers(1, 4))):
                    rd[p] = ord("ACGT"[("ACGT".index(chr(rd[p])) + 1) % 4])
            reads.append(rd)
        return pack(refs), pack(reads)
    return cached("foreign", make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("k,flags", [(21, 0), (16, FWD), (5, 0)])
def test_foreign_reads(kmc, oracle, cuda, lib, k, flags):
    refs, reads = foreign_case()
    mix = mixture(oracle, ("foreign-mix", k, flags), [refs], k, flags)
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, flags=flags, log2_slots=roomy(refs[0].size)) as acc:
            add(kmc, cuda, acc, refs)
            got = [match(cuda, acc, reads, shift=sh) for sh in (0, 7)]
    for g in got:
        check(oracle, g, reads, k, mix, 0, "k=%d flags=%d" % (k, flags), flags=flags, lossless=True)
    if k == 21:
        win, _, hit, _ = got[0]
        assert (hit == win).any() and (hit[win > 0] == 0).any() and ((hit > 0) & (hit < win)).any()


# 3. record edges ------------------------------------------------------------------------
def edges_case(k):
    def make():
        rng = np.random.default_rng(52 + k)
        every7 = bases(rng, 300)
        every7[6::7] = ord("N")
        long = bases(rng, 1000)
        recs = [bases(rng, 0), bases(rng, k - 1), bases(rng, k), bases(rng, k + 1), np.full(90, ord("N"), np.uint8),
                every7]
        recs += [bases(rng, i % 4) for i in range(60)]  # several records inside one 16-byte chunk
        recs += [long, bases(rng, 37), long[100:400].copy(), bases(rng, k + 5)]
        added = pack([long[:700], every7[:150], recs[2], bases(rng, 200)])
        return added, pack(recs)
    return cached(("edges", k), make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("k", [3, 21])
def test_record_edges(kmc, oracle, cuda, lib, k):
    added, batch = edges_case(k)
    assert batch[1][-1] == batch[0].size  # the last record ends at data_bytes
    mix = mixture(oracle, ("edges-mix", k), [added], k)
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, log2_slots=roomy(added[0].size)) as acc:
            add(kmc, cuda, acc, added)
            got = {sh: match(cuda, acc, batch, shift=sh) for sh in (0, 1, 15)}
    for sh, g in got.items():
        exp = check(oracle, g, batch, k, mix, 0, "k=%d shift=%d" % (k, sh), lossless=True)
    win = exp[0]
    assert list(win[:5]) == [0, 0, 1, 2, 0] and win[66] == 1000 - k + 1
    if k == 21:
        assert win[5] == 0 and not win[6:66].any() and 0 < got[0][2][66] < win[66]


# 4. threshold ---------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_threshold(kmc, oracle, cuda, lib):
    k = 21
    batches, js = purge_case(), purge_levels()
    seed = purge_seed(oracle, k, 16)
    mix = mixture(oracle, ("purge-mix", seed, 3), batches, k, 0, seed)
    rng = np.random.default_rng(53)
    def rec(b, r):
        d, i = batches[b]
        return d[i[r]:i[r + 1] - 1]
    reads = pack([rec(2, 3)[100:], bases(rng, 700), np.concatenate([rec(0, r) for r in range(6)]), bases(rng, 30)])
    with which(kmc, lib):
        with kmc.SketchAccum(16, k, seed=seed, log2_slots=PURGE_LG) as acc:
            for b in batches:
                add(kmc, cuda, acc, b)
            got = [match(cuda, acc, rd, m=m) for rd in (batches[3], reads) for m in (1, 2)]
    for i, g in enumerate(got):
        rd = (batches[3], reads)[i // 2]
        check(oracle, g, rd, k, mix, js[-1], "case %d" % i, m=1 + i % 2, seed=seed, lossless=True)
        assert g[3][0] == 0 and g[3][1] == bound(js[-1])
        assert (g[1] < g[0]).any() and g[3][2] > 0
    assert got[0][3][3] >= got[1][3][3] > 0  # almost every key of the set has multiplicity 2


# 5. lost inserts ------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_lost_inserts(kmc, oracle, cuda, lib):
    k = 21
    batch, seed, _ = lost_case(oracle, k)
    mix = mixture(oracle, "lost-mix", [batch], k, 0, seed)
    j = level(batch[0].size, LOST_LG)
    with which(kmc, lib):
        with kmc.SketchAccum(2, k, seed=seed, log2_slots=LOST_LG) as acc:
            add(kmc, cuda, acc, batch)
            got = match(cuda, acc, batch)
            _, _, fstats = finish(acc, 1)
    check(oracle, got, batch, k, mix, j, "lost", seed=seed, lossless=False)
    assert got[3][1] == fstats[1] < bound(j)  # limit == lost
    np.testing.assert_array_equal(got[2], got[1])  # every key below `lost` was tracked


# 6. min_count ---------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_min_count(kmc, oracle, cuda, lib):
    k = 21
    batch = planted_case()
    mix = mixture(oracle, "planted-mix", [batch], k)
    ms = (1, 2, 3, (1 << 32) - 1, 0)
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, log2_slots=roomy(batch[0].size)) as acc:
            add(kmc, cuda, acc, batch)
            got = [match(cuda, acc, batch, m=m) for m in ms]
    for m, g in zip(ms, got):
        check(oracle, g, batch, k, mix, 0, "m=%d" % m, m=m, lossless=True)
    sums = [g[3][3] for g in got]
    assert sums[0] > sums[1] > sums[2] > sums[3] == 0 and sums[4] == sums[0]  # 0 and 1 both mean every key


# 7. homopolymer -------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_homopolymer(kmc, oracle, cuda, lib):
    k = 21
    poly = pack([np.full(9000, ord("A"), np.uint8)])
    rng = np.random.default_rng(54)
    sets = {"with": pack([bases(rng, 100), np.full(30, ord("T"), np.uint8)]), "without": pack([bases(rng, 130)])}
    got = {}
    with which(kmc, lib):
        for name, added in sets.items():
            with kmc.SketchAccum(1, k, log2_slots=roomy(added[0].size)) as acc:
                add(kmc, cuda, acc, added)
                got[name] = match(cuda, acc, poly, shift=3)
    for name, g in got.items():
        check(oracle, g, poly, k, mixture(oracle, ("poly-set", name), [sets[name]], k), 0, name, lossless=True)
        assert list(g[0]) == [8980] and list(g[1]) == [8980]
    assert list(got["with"][2]) == [8980] and list(got["without"][2]) == [0]


# 8. read-only ---------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_match_leaves_the_accumulator_alone(kmc, oracle, cuda, lib):
    k, s, B = 21, 64, 8
    first, reads = foreign_case()
    lg = roomy(first[0].size + reads[0].size)
    with which(kmc, lib):
        with kmc.SketchAccum(s, k, log2_slots=lg) as plain:
            add(kmc, cuda, plain, first)
            row = finish(plain, 2)
            spec = P.host(*plain.spectrum(B))
        with kmc.SketchAccum(s, k, log2_slots=lg) as acc:
            empty = match(cuda, acc, reads)  # before any add
            add(kmc, cuda, acc, first)
            one, two = match(cuda, acc, reads), match(cuda, acc, reads)
            after = finish(acc, 2)
            aspec = P.host(*acc.spectrum(B))
            add(kmc, cuda, acc, reads)  # add, match, add, match, finish, spectrum
            later = match(cuda, acc, reads)
            finish(acc, 1)
            acc.spectrum(B)
            last = match(cuda, acc, reads)
    np.testing.assert_array_equal(after[0], row[0])
    assert after[1:] == row[1:]
    np.testing.assert_array_equal(aspec[0], spec[0])
    assert aspec[1] == spec[1]
    assert not empty[2].any() and empty[3][2] > 0 and empty[3][3] == 0
    check(oracle, one, reads, k, mixture(oracle, ("foreign-mix", k, 0), [first], k), 0, "one", lossless=True)
    for a, b in ((one, two), (later, last)):
        for x, y in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(x, y)
        assert a[3] == b[3]
    check(oracle, later, reads, k, mixture(oracle, "foreign-both", [first, reads], k), 0, "later", lossless=True)
    np.testing.assert_array_equal(later[2], later[0])  # the reads themselves are in the set now
    assert (one[2] < later[2]).any()


# 9. optional outputs, no record, arguments on a live handle --------------------------------
def live_handle_errors(L, h, host):
    f = L.kmc_match_from_accum
    assert f(h, host, host, 1, 8, 1, host, host, None, host, None) == INVALID  # null hits
    assert f(h, host, None, 1, 8, 1, None, None, host, None, None) == INVALID  # null indices
    assert f(h, None, host, 1, 8, 1, None, None, host, None, None) == INVALID  # null data, bytes above 0
    assert f(h, host, host, (1 << 40) + 1, 8, 1, None, None, host, None, None) == INVALID
    assert f(h, host, host, 1, 1 << 62, 1, None, None, host, None, None) == INVALID


@pytest.mark.parametrize("lib", LIBS)
def test_optional_outputs(kmc, oracle, cuda, lib):
    import ctypes
    import torch
    k = 21
    refs, reads = foreign_case()
    mix = mixture(oracle, ("foreign-mix", k, 0), [refs], k)
    d, di = U.device_records(cuda, *reads)
    buf = (ctypes.c_char * 64)()
    host = ctypes.c_void_p(ctypes.addressof(buf))  # never dereferenced: the arguments are judged first
    with which(kmc, lib) as D:
        L = D if lib == "diag" else kmc.lib()
        with kmc.SketchAccum(1, k, log2_slots=roomy(refs[0].size)) as acc:
            add(kmc, cuda, acc, refs)
            live_handle_errors(L, acc._h, host)
            full = match(cuda, acc, reads)
            some = {}
            for name, kw in (("no windows", dict(windows=None)), ("no sampled", dict(sampled=None)),
                             ("hits only", dict(windows=None, sampled=False)), ("no stats", dict(stats=None)),
                             ("hits alone", dict(windows=False, sampled=False, stats=False))):
                res = acc.match(d, di, **kw)
                torch.cuda.synchronize()
                some[name] = M.host(res)
            # no record: only stats is written
            e_d, e_i = U.device_records(cuda, *EMPTY)
            own = torch.full((3,), -1, dtype=torch.int32, device=cuda)
            st = torch.full((4,), -1, dtype=torch.int64, device=cuda)
            none = acc.match(e_d, e_i, out=own[:0], windows=own[:0], sampled=own[:0], stats=st)
            assert acc.match(e_d, e_i, stats=False)[3] is None
            torch.cuda.synchronize()
        with pytest.raises(ValueError):
            acc.match(d, di)  # closed
    exp = check(oracle, full, reads, k, mix, 0, "full", lossless=True)
    assert some["no windows"][0] is None and some["no sampled"][1] is None and some["no stats"][3] is None
    assert some["hits only"][:2] == (None, None) and some["hits alone"][:2] == (None, None)
    assert some["hits alone"][3] is None
    for name, g in some.items():
        M.assert_match(g, exp, name)
    assert none[2].numel() == 0 and (own.cpu().numpy() == -1).all()
    assert [int(x) for x in st.cpu().numpy().view(np.uint64)] == [1, FILL, 0, 0]


# 10. a side stream ----------------------------------------------------------------------
STREAM_LENS = [0, 5, 900, 3000, 1, 40]


def test_match_on_a_side_stream(kmc, oracle, cuda):
    """stream_util's late input: the accumulator is emptied, takes the set and matches
    the records, all on a side stream behind a delay, while the record buffers still hold
    a decoy.  Work the library put on another stream would read the decoy or the empty
    table, or miss the snapshot."""
    import torch
    k = 16
    kmc.lib()
    cycles, _ = T.sleep_cycles(T.DELAY_MS)
    s, _ = T.side_streams(kmc, cuda, cycles)
    pair = (T.records(5, STREAM_LENS[::-1]), T.records(6, STREAM_LENS))
    added = T.records(6, STREAM_LENS, related=0.5)  # shares k-mers with the real records, and some with the decoy
    a_d, a_i = U.device_records(cuda, *added)
    ins = [(dev(d, cuda), dev(d, cuda), dev(r, cuda)) for d, r in zip(*pair)]  # (live, decoy, real) of data and offsets
    n = len(STREAM_LENS)
    outs = [torch.empty(n, dtype=torch.int32, device=cuda) for _ in range(3)]
    stats = torch.empty(4, dtype=torch.int64, device=cuda)
    mix = mixture(oracle, "stream-set", [added], k)

    def expected(w):
        return M.model(oracle, pair[w][0], pair[w][1], k, mix, FILL, True)
    exp = {"decoy": expected(0), "real": expected(1)}

    def compare(got, e, msg):
        for g, x in zip(got[:3], e[:3]):
            np.testing.assert_array_equal(g.view(np.uint32), x, err_msg=msg)
        assert [int(x) for x in got[3].view(np.uint64)] == e[3], msg

    with kmc.SketchAccum(1, k, log2_slots=roomy(added[0].size)) as acc:
        def run(w, st):
            acc.reset(stream=st)
            acc.add(a_d, a_i, stream=st)
            acc.match(ins[0][0], ins[1][0], windows=outs[0], sampled=outs[1], out=outs[2], stats=stats, stream=st)
        call = T.Call("match", ins, outs + [stats], run, exp, compare,
                      lambda e: tuple(e[:3]) + (np.array(e[3], dtype=np.uint64),))
        T.late_call(call, s, cycles)
    assert exp["real"][3][3] > 0
