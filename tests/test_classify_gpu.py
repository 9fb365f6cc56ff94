"""GPU parity of kmc_label_accum, kmc_classify_from_accum (kmc.SketchAccum.label,
.classify) and kmc_classify_select against the CPU.  The expected outputs of every case
are classify_util.model's: the oracle's per-record keys and counts, the set's
multiplicities, a dict hash -> source mask built from the sources' records below the
limit the device reports (spectrum_util.check_limit holds it against the level's bound),
then integer counting.  Everything is compared exactly.  The outputs are filled with 0xFF
before every call, so a record the kernels skipped shows.  Every case runs in libkmc.so
and in libkmc_diag.so, where a wave's range is 256 bytes and almost every record is cut."""
import numpy as np
import pytest

import classify_util as C
import sketch_match_util as M
import sketch_screen_util as U
import sketch_util as S
import spectrum_util as P
import stream_util as T
from sketch_screen_util import FWD, SOFT
from sketch_util import bases, dev, pack, which
from test_sketch_accum_gpu import (EMPTY, FILL, LIBS, LOST_LG, PURGE_LG, add, bound, finish, level, lost_case, mixture,
                                   planted_case, purge_case, purge_levels, purge_seed, roomy)
from test_sketch_match_gpu import match

pytestmark = pytest.mark.gpu

INVALID, OK, WORKSPACE, ALIGNMENT = 1001, 0, 1004, 1003
NONE = C.NONE
cached = S.cache()
COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b


def revcomp(x):
    return COMP[x[::-1]]


def records_of(batch):
    d, i = batch
    return [d[i[r]:i[r + 1] - 1] for r in range(i.size - 1)]


def label(cuda, acc, batch, g, shift=0):
    d, di = U.device_records(cuda, batch[0], batch[1], shift)
    acc.label(d, di, g)


def classify(cuda, acc, batch, ns, shift=0, m=1, scores=True, ws=None, fill=None):
    """The host copies of acc.classify over `batch`, the outputs filled with 0xFF first."""
    import torch
    data, idx = batch
    d, di = U.device_records(cuda, data, idx, shift)
    n = idx.size - 1
    own = [torch.full((n,), -1, dtype=torch.int32, device=cuda) for _ in range(6)]
    sc = torch.full((n, ns), -1, dtype=torch.int32, device=cuda) if scores else False
    st = torch.full((4,), -1, dtype=torch.int64, device=cuda)
    if ws is None:
        ws = torch.empty(max(kmc_ws_size(n, data.size, ns), 1), dtype=torch.uint8, device=cuda)
        ws.fill_(0xFF if fill is None else fill)
    res = acc.classify(d, di, ns, m, windows=own[0], sampled=own[1], scores=sc, stats=st, workspace=ws, out=own[2:])
    torch.cuda.synchronize()
    return C.host(res)


def kmc_ws_size(n, nbytes, ns):
    import torch

    import kmc
    size = kmc.classify_workspace_size(n, nbytes, ns, torch.cuda.current_device())
    assert size > 0
    return size


def check(oracle, got, batch, k, mix, sources, ns, j, msg, m=1, flags=0, seed=S.DEFAULT_SEED, lossless=None):
    """The outputs equal the model's at the device's limit; returns the model's."""
    limit, everything = P.check_limit(got[7], j, lossless)
    lab = C.labels(oracle, sources, k, limit, everything, flags, seed)
    exp = C.model(oracle, batch[0], batch[1], k, mix, lab, ns, limit, everything, m, flags, seed)
    print("%s: j=%d stats=%s, %d records, %d with a source, %d ties" % (
        msg, j, got[7], got[2].size, int((got[3] != NONE).sum()), int(((got[4] == got[5]) & (got[4] > 0)).sum())))
    C.assert_classify(got, exp, msg)
    return exp


# the two related references ---------------------------------------------------------------
def related_case():
    """Two references that share their first half; the second half of B is A's with a
    substitution every 9 .. 14 bases.  60 reads of 25 .. 220 bases from either strand of
    either reference, and some fresh ones; N and lowercase in a few."""
    def make():
        rng = np.random.default_rng(610)
        a = bases(rng, 1600)
        b = a.copy()
        p = 800
        while p < b.size:
            b[p] = ord("ACGT"[("ACGT".index(chr(b[p])) + 1 + int(rng.integers(0, 3))) % 4])
            p += int(rng.integers(9, 15))
        reads = []
        for i in range(60):
            n = int(rng.integers(25, 221))
            if i % 6 == 5:
                reads.append(bases(rng, n))
                continue
            src = (a, b)[i % 2]
            at = int(rng.integers(0, src.size - n + 1))
            rd = src[at:at + n].copy()
            if i % 4 >= 2:
                rd = revcomp(rd)
            if i % 7 == 3:
                rd[n // 2] = ord("N")
            if i % 7 == 4:
                rd[n // 3:n // 3 + 5] += 32  # lowercase
            reads.append(rd)
        return pack([a]), pack([b]), pack(reads)
    return cached("related", make)


# 1. walk variants -----------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("flags", [0, SOFT, FWD])
@pytest.mark.parametrize("k", [1, 5, 16, 31])
def test_walk_variants(kmc, oracle, cuda, lib, k, flags):
    a, b, reads = related_case()
    mix = mixture(oracle, ("related-mix", k, flags), [a, b], k, flags)
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, flags=flags, log2_slots=roomy(a[0].size + b[0].size)) as acc:
            add(kmc, cuda, acc, a)
            add(kmc, cuda, acc, b, shift=3)
            label(cuda, acc, a, 0, shift=5)
            label(cuda, acc, b, 1)
            got = classify(cuda, acc, reads, 2, shift=1)
    exp = check(oracle, got, reads, k, mix, [(0, a), (1, b)], 2, 0, "k=%d flags=%d" % (k, flags), flags=flags,
                lossless=True)
    if k >= 16:
        assert (exp[3] == 0).any() and (exp[3] == 1).any() and (exp[3] == NONE).any()
        assert ((exp[4] == exp[5]) & (exp[4] > 0)).any() and (exp[4] > exp[5]).any()


# 2. sources at the word's edges ---------------------------------------------------------
def edges_case():
    """32 sources: all hold `common`; source g holds a piece of its own; reads of the
    common piece, of single sources (0, 5, 31 among them) and of two joined."""
    def make():
        rng = np.random.default_rng(611)
        common = bases(rng, 90)
        own = [bases(rng, 60 + g) for g in range(32)]
        sources = [pack([common, own[g]]) for g in range(32)]
        reads = [common, own[0], own[31], own[5], np.concatenate([own[0][:40], own[31]]),
                 np.concatenate([own[1], common[:50], own[30][:30]]), bases(rng, 80), own[31][5:50]]
        return sources, pack(reads)
    return cached("edges", make)


@pytest.mark.parametrize("lib", LIBS)
def test_sources_at_the_word_edges(kmc, oracle, cuda, lib):
    k = 21
    sources, reads = edges_case()
    mix = mixture(oracle, "edges-mix", sources, k)
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, log2_slots=roomy(sum(s[0].size for s in sources))) as acc:
            for s in sources:
                add(kmc, cuda, acc, s)
            for g, s in enumerate(sources):
                label(cuda, acc, s, g)
            label(cuda, acc, sources[5], 5)  # a source labelled twice
            got = {ns: classify(cuda, acc, reads, ns) for ns in (1, 2, 32)}
    srcs = list(enumerate(sources))
    for ns, g in got.items():
        exp = check(oracle, g, reads, k, mix, srcs, ns, 0, "ns=%d" % ns, lossless=True)  # bits >= ns ignored
    e = exp  # ns = 32
    assert list(e[6][0]) == [90 - k + 1] * 32 and e[3][0] == 0 and e[4][0] == e[5][0]  # held by all 32
    assert e[3][2] == 31 and e[5][2] == 0 and e[3][1] == 0
    assert got[1][5].max() == 0 and got[2][3][2] == NONE and got[2][2][2] > 0  # a hit whose bit is not below ns
    assert e[6][3][5] == 65 - k + 1  # labelled twice: counted once


# 3. ties and empty results --------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_ties_and_empty_results(kmc, oracle, cuda, lib):
    k = 16
    rng = np.random.default_rng(612)
    x, y, z, w = (bases(rng, n) for n in (120, 100, 140, 90))
    s1, s2, unl = pack([x, y]), pack([x, z]), pack([w])  # sources 1 and 2, and an input never labelled
    reads = pack([x, bases(rng, 0), bases(rng, k - 1), bases(rng, 200), w, np.concatenate([w, y[:30]]),
                  np.full(50, ord("N"), np.uint8), z[10:90], np.concatenate([y[:40], z[:40]])])
    mix = mixture(oracle, "ties-mix", [s1, s2, unl], k)
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, log2_slots=roomy(700)) as acc:
            for s in (s1, s2, unl):
                add(kmc, cuda, acc, s)
            label(cuda, acc, s1, 1)
            label(cuda, acc, s2, 2)
            got = classify(cuda, acc, reads, 3)
    e = check(oracle, got, reads, k, mix, [(1, s1), (2, s2)], 3, 0, "ties", lossless=True)
    n = 120 - k + 1
    assert (e[3][0], e[4][0], e[5][0]) == (1, n, n) and list(e[6][0]) == [0, n, n]  # a tie: the smallest index
    for r in (1, 2, 6):  # no window
        assert e[0][r] == 0 and e[3][r] == NONE
    assert e[0][3] > 0 and e[2][3] == 0 and (e[3][3], e[4][3], e[5][3]) == (NONE, 0, 0)  # windows, no hit
    assert e[2][4] == 90 - k + 1 and e[3][4] == NONE and not e[6][4].any()  # hits whose label is 0
    assert e[3][5] == 1 and e[2][5] > e[4][5] > 0
    assert e[4][8] > 0 and e[5][8] > 0  # both sources hold a part


# 4. cuts --------------------------------------------------------------------------------
def cuts_case():
    """Records against the launch's cuts: 20 records of 256 bytes and one whose last window
    ends on a multiple of 256 (the diag library's ranges, when the data starts a chunk);
    100 records of 0 .. 40 bases; one record of 66 000 bases that spans every wave of
    either library's launch, made of pieces of both references and fresh bases; 30 reads."""
    def make():
        k = 21
        rng = np.random.default_rng(613)
        a, b, _ = related_case()
        a, b = a[0][:-1], b[0][:-1]
        def piece(n):
            src = (a, b)[int(rng.integers(0, 2))]
            at = int(rng.integers(0, src.size - n + 1))
            return src[at:at + n].copy()
        recs = [piece(255) for _ in range(20)] + [piece(256 + k - 1)]
        assert sum(r.size + 1 for r in recs[:20]) == 5120
        recs += [piece(int(n)) for n in rng.integers(0, 41, size=100)]
        parts, total = [], 0
        while total < 66_000:
            p = piece(int(rng.integers(30, 400))) if len(parts) % 3 else bases(rng, int(rng.integers(30, 400)))
            parts.append(p)
            total += p.size
        recs.append(np.concatenate(parts))
        recs += [piece(150) for _ in range(30)]
        return pack(recs)
    return cached("cuts", make)


def cuts_run(kmc, cuda, lib, shifts):
    k = 21
    a, b, _ = related_case()
    batch = cuts_case()
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, log2_slots=roomy(a[0].size + b[0].size)) as acc:
            add(kmc, cuda, acc, a)
            add(kmc, cuda, acc, b)
            label(cuda, acc, a, 0)
            label(cuda, acc, b, 1)
            return {sh: classify(cuda, acc, batch, 2, shift=sh) for sh in shifts}


def cuts_expected(oracle, stats):
    k = 21
    a, b, _ = related_case()
    batch = cuts_case()
    def make():
        mix = mixture(oracle, ("related-mix", k, 0), [a, b], k)
        lab = C.labels(oracle, [(0, a), (1, b)], k, FILL, True)
        return C.model(oracle, batch[0], batch[1], k, mix, lab, 2, FILL, True)
    assert stats[:2] == [1, FILL]
    return cached("cuts-model", make)


@pytest.mark.parametrize("lib", LIBS)
def test_cut_records(kmc, oracle, cuda, lib):
    got = cuts_run(kmc, cuda, lib, range(16))
    exp = cuts_expected(oracle, got[0][7])
    for sh, g in got.items():
        C.assert_classify(g, exp, "%s shift %d" % (lib, sh))
    long = 121
    assert exp[0][long] >= 66_000 - 20 and exp[4][long] > exp[5][long] > 0 and exp[0][20] == 256


def test_both_libraries_agree(kmc, oracle, cuda):
    ship, diag = (cuts_run(kmc, cuda, lib, (0, 9))for lib in LIBS)
    for sh in (0, 9):
        C.assert_same(ship[sh], diag[sh], "shift %d" % sh)
        assert ship[sh][7] == diag[sh][7]


# 5. sampling ----------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_sampled_table(kmc, oracle, cuda, lib):
    """Labelled after the purges: source b is batch b; the votes are the model's below limit."""
    k = 21
    batches, js = purge_case(), purge_levels()
    seed = purge_seed(oracle, k, 16)
    mix = mixture(oracle, ("purge-mix", seed, 3), batches, k, 0, seed)
    assert js[-1] > 0
    with which(kmc, lib):
        with kmc.SketchAccum(16, k, seed=seed, log2_slots=PURGE_LG) as acc:
            for b in batches:
                add(kmc, cuda, acc, b)
            for g, b in enumerate(batches):
                label(cuda, acc, b, g)
            got = [classify(cuda, acc, rd, len(batches), m=m) for rd in (batches[3], batches[0]) for m in (1, 2)]
    srcs = list(enumerate(batches))
    for i, g in enumerate(got):
        rd = (batches[3], batches[0])[i // 2]
        e = check(oracle, g, rd, k, mix, srcs, len(batches), js[-1], "case %d" % i, m=1 + i % 2, seed=seed,
                  lossless=True)
        assert g[7][0] == 0 and g[7][1] == bound(js[-1]) and (g[1] < g[0]).any()
    assert got[0][4].max() > 0


@pytest.mark.parametrize("lib", LIBS)
def test_lost_inserts(kmc, oracle, cuda, lib):
    k = 21
    batch, seed, _ = lost_case(oracle, k)
    mix = mixture(oracle, "lost-mix", [batch], k, 0, seed)
    j = level(batch[0].size, LOST_LG)
    recs = records_of(batch)
    half = [pack(recs[:len(recs) // 2]), pack(recs[len(recs) // 2:])] if len(recs) > 1 else [batch, batch]
    with which(kmc, lib):
        with kmc.SketchAccum(2, k, seed=seed, log2_slots=LOST_LG) as acc:
            add(kmc, cuda, acc, batch)
            label(cuda, acc, half[0], 0)
            label(cuda, acc, half[1], 31)
            got = classify(cuda, acc, batch, 32)
    check(oracle, got, batch, k, mix, [(0, half[0]), (31, half[1])], 32, j, "lost", seed=seed, lossless=False)


@pytest.mark.parametrize("lib", LIBS)
def test_min_count(kmc, oracle, cuda, lib):
    k = 21
    batch = planted_case()
    mix = mixture(oracle, "planted-mix", [batch], k)
    recs = records_of(batch)
    srcs = [(0, pack(recs[0::2])), (1, pack(recs[1::2]))]
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, log2_slots=roomy(batch[0].size)) as acc:
            add(kmc, cuda, acc, batch)
            for g, s in srcs:
                label(cuda, acc, s, g)
            got = {m: classify(cuda, acc, batch, 2, m=m) for m in (1, 2)}
    for m, g in got.items():
        check(oracle, g, batch, k, mix, srcs, 2, 0, "m=%d" % m, m=m, lossless=True)
    assert got[1][7][3] > got[2][7][3] > 0


# 6. agreement with the match, optional outputs, the workspace ------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_agreement_with_match(kmc, oracle, cuda, lib):
    import torch
    k = 21
    a, b, _ = related_case()
    batch = cuts_case()
    n = batch[1].size - 1
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, log2_slots=roomy(a[0].size + b[0].size)) as acc:
            add(kmc, cuda, acc, a)
            add(kmc, cuda, acc, b)
            label(cuda, acc, a, 0)
            label(cuda, acc, b, 1)
            plain = match(cuda, acc, batch, shift=2)
            ws = torch.empty(kmc_ws_size(n, batch[0].size, 2), dtype=torch.uint8, device=cuda)
            ws.fill_(0xFF)
            full = classify(cuda, acc, batch, 2, shift=2, ws=ws)
            again = classify(cuda, acc, batch, 2, shift=2, ws=ws)  # the former call's bytes in the workspace
            other = classify(cuda, acc, pack(records_of(batch)[::-1]), 2, ws=ws)
            third = classify(cuda, acc, batch, 2, shift=2, ws=ws, scores=False)
            zero = classify(cuda, acc, batch, 2, shift=2, fill=0)
            d, di = U.device_records(cuda, *batch)
            bare = C.host(acc.classify(d, di, 2, windows=False, sampled=None, stats=False))  # the library's workspace
            torch.cuda.synchronize()
    M.assert_match(full[:3] + (full[7],), plain, "classify against match")
    assert third[6] is None and bare[0] is None and bare[1] is None and bare[6] is None and bare[7] is None
    for name, g in (("again", again), ("no scores", third), ("zero workspace", zero), ("bare", bare)):
        C.assert_same(full, g, name)
    np.testing.assert_array_equal(other[3], full[3][::-1])
    np.testing.assert_array_equal(other[6], full[6][::-1])


@pytest.mark.parametrize("lib", LIBS)
def test_arguments_on_a_live_handle(kmc, oracle, cuda, lib):
    import ctypes

    import torch
    k = 21
    a, b, reads = related_case()
    d, di = U.device_records(cuda, *reads)
    n = reads[1].size - 1
    buf = (ctypes.c_char * 64)()
    host = ctypes.c_void_p(ctypes.addressof(buf))  # never dereferenced: the arguments are judged first
    with which(kmc, lib) as D:
        L = D if lib == "diag" else kmc.lib()
        f = L.kmc_classify_from_accum
        with kmc.SketchAccum(1, k, log2_slots=roomy(a[0].size)) as acc:
            h = acc._h
            add(kmc, cuda, acc, a)
            label(cuda, acc, a, 0)
            assert f(h, host, host, 1, 8, 1, 1, None, None, None, host, host, host, None, None, None, 0, None) == INVALID
            assert f(h, host, host, 1, 8, 1, 1, None, None, host, None, host, host, None, None, None, 0, None) == INVALID
            assert f(h, host, host, 1, 8, 1, 1, None, None, host, host, None, host, None, None, None, 0, None) == INVALID
            assert f(h, host, host, 1, 8, 1, 1, None, None, host, host, host, None, None, None, None, 0, None) == INVALID
            assert f(h, host, None, 1, 8, 1, 1, None, None, host, host, host, host, None, None, None, 0, None) == INVALID
            assert f(h, None, host, 1, 8, 1, 1, None, None, host, host, host, host, None, None, None, 0, None) == INVALID
            for ns in (0, 33):
                assert f(h, host, host, 1, 8, ns, 1, None, None, host, host, host, host, None, None, None, 0,
                         None) == INVALID
            assert f(h, host, host, (1 << 40) + 1, 8, 1, 1, None, None, host, host, host, host, None, None, None, 0,
                     None) == INVALID
            assert f(h, host, host, 1, 1 << 62, 1, 1, None, None, host, host, host, host, None, None, None, 0,
                     None) == INVALID
            assert L.kmc_label_accum(h, host, host, 1, 8, 32, None) == INVALID
            assert L.kmc_label_accum(h, host, None, 1, 8, 0, None) == INVALID
            assert L.kmc_label_accum(h, None, host, 1, 8, 0, None) == INVALID
            assert L.kmc_label_accum(h, host, host, (1 << 40) + 1, 8, 0, None) == INVALID
            assert L.kmc_label_accum(h, host, host, 1, 1 << 62, 0, None) == INVALID
            size = kmc_ws_size(n, reads[0].size, 1)
            ws = torch.empty(size + 8, dtype=torch.uint8, device=cuda)
            with pytest.raises(kmc.KmcError) as small:
                acc.classify(d, di, 1, workspace=ws[:size - 1])
            with pytest.raises(kmc.KmcError) as odd:
                acc.classify(d, di, 1, workspace=ws[1:size + 1])
            with pytest.raises(kmc.KmcError) as both:
                acc.classify(d, di, 1, workspace=ws[1:size - 1])
            # no record: only stats is written
            e_d, e_i = U.device_records(cuda, *EMPTY)
            own = torch.full((3,), -1, dtype=torch.int32, device=cuda)
            st = torch.full((4,), -1, dtype=torch.int64, device=cuda)
            acc.classify(e_d, e_i, 1, windows=own[:0], sampled=own[:0], out=[own[:0]] * 4, stats=st)
            torch.cuda.synchronize()
    assert (small.value.code, odd.value.code, both.value.code) == (WORKSPACE, ALIGNMENT, WORKSPACE)
    assert (own.cpu().numpy() == -1).all()
    assert [int(x) for x in st.cpu().numpy().view(np.uint64)] == [1, FILL, 0, 0]
    assert kmc_ws_size(1 << 20, 1 << 20, 2) == kmc_ws_size(1, 1 << 20, 32)  # not with num_seqs * num_sources


# 7. the label is read-only --------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_label_leaves_the_accumulator_alone(kmc, oracle, cuda, lib):
    k, s, B = 21, 64, 8
    a, b, reads = related_case()
    def state(acc):
        row = finish(acc, 1)
        spec = P.host(*acc.spectrum(B))
        return row, spec, match(cuda, acc, reads)
    with which(kmc, lib):
        with kmc.SketchAccum(s, k, log2_slots=roomy(a[0].size + b[0].size)) as acc:
            add(kmc, cuda, acc, a)
            add(kmc, cuda, acc, b)
            before = state(acc)
            label(cuda, acc, a, 0)
            middle = state(acc)
            label(cuda, acc, b, 1)
            label(cuda, acc, a, 0)
            once = classify(cuda, acc, reads, 2)
            after = state(acc)
            twice = classify(cuda, acc, reads, 2)
    for other in (middle, after):
        np.testing.assert_array_equal(other[0][0], before[0][0])
        assert other[0][1:] == before[0][1:]
        np.testing.assert_array_equal(other[1][0], before[1][0])
        assert other[1][1] == before[1][1]
        M.assert_match(other[2], before[2], "match")
    C.assert_same(once, twice, "finish, spectrum and match leave the labels alone")


# 8. life cycle --------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_life_cycle(kmc, oracle, cuda, lib):
    k = 21
    a, b, reads = related_case()
    d, di = U.device_records(cuda, *reads)
    mix = mixture(oracle, ("related-a", k), [a], k)
    def refused(acc):
        with pytest.raises(kmc.KmcError) as e:
            acc.classify(d, di, 4)
        assert e.value.code == INVALID
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, log2_slots=roomy(a[0].size + b[0].size)) as acc:
            refused(acc)  # before any label
            add(kmc, cuda, acc, a)
            refused(acc)
            label(cuda, acc, a, 3)
            first = classify(cuda, acc, reads, 4)
            add(kmc, cuda, acc, EMPTY)  # an add of no record leaves the labels
            classify(cuda, acc, reads, 4)
            add(kmc, cuda, acc, b)  # label, add, classify
            refused(acc)
            acc.reset()
            refused(acc)
            add(kmc, cuda, acc, a)
            refused(acc)
            label(cuda, acc, EMPTY, 0)  # no record: the labels are established all the same
            blank = classify(cuda, acc, reads, 4)
            label(cuda, acc, a, 1)
            second = classify(cuda, acc, reads, 4)
    check(oracle, first, reads, k, mix, [(3, a)], 4, 0, "before the reset", lossless=True)
    check(oracle, blank, reads, k, mix, [], 4, 0, "established, nothing labelled", lossless=True)
    e = check(oracle, second, reads, k, mix, [(1, a)], 4, 0, "after the reset", lossless=True)
    assert e[6][:, 1].any() and not second[6][:, 3].any()  # only bit 1: nothing stale
    assert (blank[3] == NONE).all() and blank[2].any()


# 9. homopolymer and low complexity ------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_homopolymer(kmc, oracle, cuda, lib):
    k = 21
    rng = np.random.default_rng(614)
    s0 = pack([bases(rng, 100), np.full(30, ord("T"), np.uint8)])
    s1 = pack([np.tile(np.frombuffer(b"AC", np.uint8), 40), np.full(25, ord("A"), np.uint8)])
    s2 = pack([np.tile(np.frombuffer(b"ACG", np.uint8), 30)])
    reads = pack([np.full(9000, ord("A"), np.uint8), np.tile(np.frombuffer(b"GT", np.uint8), 700),
                  np.tile(np.frombuffer(b"CGT", np.uint8), 333), np.concatenate([np.full(40, ord("T"), np.uint8),
                                                                                 np.tile(np.frombuffer(b"CA", np.uint8), 30)])])
    srcs = [(0, s0), (1, s1), (2, s2)]
    mix = mixture(oracle, "poly-mix", [s0, s1, s2], k)
    with which(kmc, lib):
        with kmc.SketchAccum(1, k, log2_slots=roomy(400)) as acc:
            for _, s in srcs:
                add(kmc, cuda, acc, s)
            for g, s in srcs:
                label(cuda, acc, s, g)
            got = classify(cuda, acc, reads, 3, shift=3)
    e = check(oracle, got, reads, k, mix, srcs, 3, 0, "poly", lossless=True)
    assert list(e[6][0]) == [8980, 8980, 0] and (e[3][0], e[5][0]) == (0, 8980)
    assert e[3][1] == 1 and e[3][2] == 2 and e[4][1] == 1400 - k + 1


# 10. streams ----------------------------------------------------------------------------
STREAM_LENS = [0, 5, 900, 3000, 1, 40]


def test_classify_on_a_side_stream(kmc, oracle, cuda):
    """stream_util's late input: the accumulator is emptied, takes the set and its labels
    and classifies the records, all on a side stream behind a delay, while the record
    buffers still hold a decoy."""
    import torch
    k = 16
    kmc.lib()
    cycles, _ = T.sleep_cycles(T.DELAY_MS)
    s, _ = T.side_streams(kmc, cuda, cycles)
    pair = (T.records(5, STREAM_LENS[::-1]), T.records(6, STREAM_LENS))
    added = T.records(6, STREAM_LENS, related=0.5)
    halves = [pack(records_of(added)[:3]), pack(records_of(added)[3:])]
    a_d, a_i = U.device_records(cuda, *added)
    h_in = [U.device_records(cuda, *h) for h in halves]
    ins = [(dev(d, cuda), dev(d, cuda), dev(r, cuda)) for d, r in zip(*pair)]
    n = len(STREAM_LENS)
    outs = [torch.empty(n, dtype=torch.int32, device=cuda) for _ in range(6)]
    sc = torch.empty((n, 2), dtype=torch.int32, device=cuda)
    stats = torch.empty(4, dtype=torch.int64, device=cuda)
    ws = torch.empty(kmc_ws_size(n, pair[0][0].size, 2), dtype=torch.uint8, device=cuda)
    mix = mixture(oracle, "stream-set", [added], k)
    lab = C.labels(oracle, list(enumerate(halves)), k, FILL, True)

    def expected(w):
        return C.model(oracle, pair[w][0], pair[w][1], k, mix, lab, 2, FILL, True)
    exp = {"decoy": expected(0), "real": expected(1)}

    def compare(got, e, msg):
        for g, x in zip(got[:7], e[:7]):
            np.testing.assert_array_equal(g.view(np.uint32), x, err_msg=msg)
        assert [int(x) for x in got[7].view(np.uint64)] == e[7], msg

    with kmc.SketchAccum(1, k, log2_slots=roomy(added[0].size)) as acc:
        def run(w, st):
            acc.reset(stream=st)
            acc.add(a_d, a_i, stream=st)
            for g, (hd, hi) in enumerate(h_in):
                acc.label(hd, hi, g, stream=st)
            acc.classify(ins[0][0], ins[1][0], 2, windows=outs[0], sampled=outs[1], out=outs[2:], scores=sc, stats=stats,
                         workspace=ws, stream=st)
        call = T.Call("classify", ins, outs + [sc, stats], run, exp, compare,
                      lambda e: tuple(e[:7]) + (np.array(e[7], dtype=np.uint64),), ws=ws)
        T.late_call(call, s, cycles)
    assert (exp["real"][3] != NONE).any()


def test_two_handles_overlap(kmc, oracle, cuda):
    """Two accumulators, each with its own outputs and workspace, classify alternately on
    two side streams, eight rounds, without a host synchronisation in between."""
    import torch
    k = 21
    a, b, reads = related_case()
    batch = cuts_case()
    jobs = []
    accs = [kmc.SketchAccum(1, k, log2_slots=roomy(a[0].size + b[0].size)) for _ in range(2)]
    try:
        for w, acc in enumerate(accs):
            for s in (a, b):
                add(kmc, cuda, acc, s)
            label(cuda, acc, a, w)
            label(cuda, acc, b, 1 - w)
            rd = (batch, reads)[w]
            d, di = U.device_records(cuda, *rd)
            ws = torch.empty(kmc_ws_size(rd[1].size - 1, rd[0].size, 2), dtype=torch.uint8, device=cuda)
            jobs.append((acc, d, di, ws, classify(cuda, acc, rd, 2)))
        s1, s2 = torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)
        torch.cuda.synchronize()
        res = []
        for _ in range(8):
            for (acc, d, di, ws, _), st in zip(jobs, (s1, s2)):
                with torch.cuda.stream(st):
                    ws.fill_(0xFF)
                res.append(acc.classify(d, di, 2, scores=True, workspace=ws, stream=st))
        s1.synchronize()
        s2.synchronize()
        for i, r in enumerate(res):
            C.assert_same(C.host(r), jobs[i % 2][4], "round %d handle %d" % (i // 2, i % 2))
    finally:
        for acc in accs:
            acc.close()
    exp = cuts_expected(oracle, jobs[0][4][7])
    C.assert_classify(jobs[0][4], exp, "handle 0")


# 11. kmc_classify_select ----------------------------------------------------------------
def test_classify_select(kmc, cuda):
    import torch
    rng = np.random.default_rng(615)
    n = 1000
    best = rng.integers(0, 4, size=n).astype(np.uint32)
    best[rng.random(n) < 0.2] = NONE
    nh = rng.integers(0, 50, size=n).astype(np.uint32)
    bh = nh + rng.integers(0, 4, size=n).astype(np.uint32)  # margins 0 .. 3
    bh[best == NONE] = 0
    nh[best == NONE] = 0
    listed = (rng.random(n) < 0.7).astype(np.uint32) * rng.integers(1, 9, size=n).astype(np.uint32)
    t = [dev(x.view(np.int32), cuda) for x in (listed, best, bh, nh)]
    for src, margin in ((0, 1), (3, 0), (2, 2), (1, 3), (31, 1), (0, 4)):
        for lst in (t[0], None):
            keep, kept = kmc.classify_select(lst, t[1], t[2], t[3], src, margin)
            torch.cuda.synchronize()
            exp = C.select(listed if lst is not None else None, best, bh, nh, src, margin)
            np.testing.assert_array_equal(keep.cpu().numpy().view(np.uint32), exp)
            assert int(kept.item()) == int(exp.sum())
    margins = (bh - nh)[(best == 2) & (listed != 0)]
    assert (margins == 0).any() and (margins == 2).any() and (margins == 1).any()
    alias = t[0].clone()
    keep, kept = kmc.classify_select(alias, t[1], t[2], t[3], 2, 2, count=False, out=alias)  # keep is listed
    torch.cuda.synchronize()
    assert keep is alias and kept is None
    np.testing.assert_array_equal(alias.cpu().numpy().view(np.uint32), C.select(listed, best, bh, nh, 2, 2))
    e = torch.empty(0, dtype=torch.int32, device=cuda)
    keep, kept = kmc.classify_select(None, e, e, e, 0)
    torch.cuda.synchronize()
    assert keep.numel() == 0 and int(kept.item()) == 0
