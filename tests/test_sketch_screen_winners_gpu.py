"""GPU parity of the winner-takes-all screen (kmc_sketch_screen_winners) against the numpy
restatement of its rule (sketch_screen_winners_util): won, the median multiplicity of the
won values and all[] are compared bit for bit, the identity as test_sketch_screen_gpu
compares it.  Every case runs in libkmc.so and in libkmc_diag.so (64-thread workgroups, a
table of two slots per value: long probe chains).  Rows are opaque values, so most cases
compose them by hand from the hashes of a small mixture (present values) and random values
checked absent, which gives exact control of all[] and size[]."""
import numpy as np
import pytest

import sketch_query_util as Q
import sketch_screen_util as U
import sketch_screen_winners_util as W
import sketch_util as S
import stream_util as T
from sketch_screen_util import FWD
from sketch_util import bases, pack, which
from test_sketch_screen_gpu import LIBS, device_rows, general_case, general_mix, kmer_of, sketch_rows

pytestmark = pytest.mark.gpu

cached = S.cache()
K = 21


def composed(oracle):
    """A mixture of 20 kbase with a part of it twice more and a part of that once more
    (multiplicities 1, 2 and 3), its hashes in random order (present) and 40 000 values it
    lacks (absent)."""
    def make():
        rng = np.random.default_rng(1200)
        b = bases(rng, 20000)
        mixture = pack([b, b[:6000], b[:2500]])
        mix = U.mixture_hashes(oracle, mixture[0], mixture[1], K)
        assert mix[0].size > 19000 and set(np.unique(mix[1])) >= {1, 2, 3}
        cand = np.unique(rng.integers(1, 1 << 63, size=41000, dtype=np.uint64))
        absent = rng.permutation(cand[~np.isin(cand, mix[0])])[:40000]
        assert absent.size == 40000
        return mixture, mix, rng.permutation(mix[0]), absent
    return cached("composed", make)


def winners(kmc, cuda, rows, sizes, mixture, k=K, flags=0, seed=S.DEFAULT_SEED, index_rows=None, **kw):
    """build (from index_rows, or the rows themselves), one count, winners: (index, host results)."""
    import torch
    sk, sz = device_rows(cuda, rows, sizes)
    bsk, bsz = (sk, sz) if index_rows is None else device_rows(cuda, *index_rows)
    index = kmc.sketch_screen_build(bsk, bsz)
    d, di = U.device_records(cuda, *mixture)
    kmc.sketch_screen_count(index, d, di, k, flags=flags, seed=seed)
    res = kmc.sketch_screen_winners(index, sk, sz, k, **kw)
    torch.cuda.synchronize()
    return index, W.host_winners(res)


def check(kmc, cuda, lib, lists, s, mixture, mix, want_won=None, want_all=None, k=K, msg=""):
    """The rows `lists` screened in `lib` against the oracle; want_*: what the case states by hand."""
    rows, sizes = Q.pack(lists, s)
    exp = W.winners_expected(mix, rows, sizes, s, k)
    if want_all is not None:
        assert list(exp[3]) == want_all, "%s: the case's own all[] %s" % (msg, list(exp[3]))
    if want_won is not None:
        assert list(exp[0]) == want_won, "%s: the oracle's won %s" % (msg, list(exp[0]))
    with which(kmc, lib):
        _, got = winners(kmc, cuda, rows, sizes, mixture, k=k)
    W.assert_winners(got, exp, msg)
    return got, exp


# 1. the general case -----------------------------------------------------------------
def general_rows(kmc, oracle, cuda, lib, s, flags):
    """test_sketch_screen_gpu's 12 references sketched on the device, and three more rows: a
    copy of row 7, row 3 with every other value replaced by an absent one, and the bottom-s
    of the union of rows 0 and 1."""
    (rdata, ridx), mixture = general_case()
    mix = general_mix(oracle, K, flags)
    with which(kmc, lib):
        _, _, rows, sizes = sketch_rows(kmc, cuda, rdata, ridx, K, s, flags)
    rng = np.random.default_rng(1210 + s)
    cand = np.unique(rng.integers(1, 1 << 63, size=2 * s + 64, dtype=np.uint64))
    absent = cand[~np.isin(cand, mix[0]) & ~np.isin(cand, rows)]
    lists = [rows[r, :sizes[r]] for r in range(12)]
    half = lists[3].copy()
    half[::2] = absent[:half[::2].size]
    lists += [lists[7], half, np.union1d(lists[0], lists[1])[:s]]
    return Q.pack(lists, s) + (mixture, mix)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("flags", [0, FWD])
@pytest.mark.parametrize("s", [64, 1000])
def test_winners_general(kmc, oracle, cuda, lib, s, flags):
    rows, sizes, mixture, mix = general_rows(kmc, oracle, cuda, lib, s, flags)
    exp = W.winners_expected(mix, rows, sizes, s, K)
    plain = U.screen_expected(mix, rows, sizes, s, K)
    np.testing.assert_array_equal(exp[3], plain[0])
    assert W.contested(mix, rows, sizes, s).size > 0, "no value is contested"
    assert (exp[0] != exp[3]).any(), "the case would pass on the plain results"
    assert exp[0][12] == 0 and exp[3][12] == exp[3][7] > 0, "the copy of row 7 loses everything to it"
    with which(kmc, lib):
        _, got = winners(kmc, cuda, rows, sizes, mixture, flags=flags)
    W.assert_winners(got, exp, "s=%d flags=%d" % (s, flags))


# 9. invariants (on case 1), optional outputs --------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_winners_invariants_and_optional_outputs(kmc, oracle, cuda, lib):
    import torch
    s = 64
    rows, sizes, mixture, mix = general_rows(kmc, oracle, cuda, lib, s, 0)
    exp = W.winners_expected(mix, rows, sizes, s, K)
    with which(kmc, lib):
        index, got = winners(kmc, cuda, rows, sizes, mixture)
        held = np.unique(np.concatenate([rows[r, :sizes[r]] for r in range(rows.shape[0])]))
        found = int((U.multiplicities(mix, held) > 0).sum())
        assert int(got[0].sum()) == found == int(exp[0].sum()), "every found value is credited exactly once"
        assert (got[0] <= got[3]).all()
        W.assert_winners(got, exp, "all four")
        sk, sz = device_rows(cuda, rows, sizes)
        for kw in (dict(median=False), dict(identity=False), dict(shared_all=False),
                   dict(median=False, identity=False, shared_all=False)):
            res = kmc.sketch_screen_winners(index, sk, sz, K, **kw)
            torch.cuda.synchronize()
            part = W.host_winners(res)
            assert [x is None for x in part[1:]] == [not kw.get(n, True) for n in ("median", "identity", "shared_all")]
            for a, b in zip(part, got):
                if a is not None:
                    assert a.tobytes() == b.tobytes(), kw


# 2. identical rows ---------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_winners_identical_rows(kmc, oracle, cuda, lib):
    """Two rows of the same ten found values: the lower index takes everything, the other
    gets won 0, median 0 and identity +0.0f; a third row on other values keeps its own, and
    whichever of the equal rows stands first wins."""
    mixture, mix, P, _ = composed(oracle)
    a, other = P[:10], P[10:15]
    for lists, want in (([a, a, other], [10, 0, 5]), ([other, a, a], [5, 10, 0]), ([a, other, a], [10, 5, 0])):
        got, _ = check(kmc, cuda, lib, lists, 16, mixture, mix, want_won=want, want_all=[len(x) for x in lists])
        loser = want.index(0)
        assert got[1][loser] == 0 and got[2].view(np.uint32)[loser] == 0, "median 0 and +0.0f bit for bit"
        assert got[2][want.index(10)] == 1.0


# 3. exact ties ---------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_winners_exact_ties(kmc, oracle, cuda, lib):
    """A: 2 found of size 4; B: 3 found of size 6; they share one found value: 2 * 6 == 3 * 4,
    so it goes to the smaller index in both orders."""
    mixture, mix, P, A = composed(oracle)
    ra = [P[0], P[1], A[0], A[1]]
    rb = [P[0], P[2], P[3], A[2], A[3], A[4]]
    check(kmc, cuda, lib, [ra, rb], 8, mixture, mix, want_won=[2, 2], want_all=[2, 3], msg="A first")
    check(kmc, cuda, lib, [rb, ra], 8, mixture, mix, want_won=[3, 1], want_all=[3, 2], msg="B first")


# 4. exact where float32 ties ---------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_winners_exact_where_float32_ties(kmc, oracle, cuda, lib):
    """s = 16384.  A: size 16384 with 16383 found; B: size 16383 with 16382 found, all of them
    A's.  16383/16384 > 16382/16383 and the two are one float32: A wins whichever index it
    has.  At the other end 1/16384 < 1/16383 on one shared value: B wins."""
    s = 16384
    mixture, mix, P, A = composed(oracle)
    assert np.float32(16383 / 16384) == np.float32(16382 / 16383) and 16383 * 16383 > 16382 * 16384
    ra = np.concatenate([P[:16383], A[:1]])
    rb = np.concatenate([P[1:16383], A[1:2]])
    check(kmc, cuda, lib, [ra, rb], s, mixture, mix, want_won=[16383, 0], want_all=[16383, 16382], msg="A first")
    check(kmc, cuda, lib, [rb, ra], s, mixture, mix, want_won=[0, 16383], want_all=[16382, 16383], msg="B first")
    ra = np.concatenate([P[:1], A[:16383]])
    rb = np.concatenate([P[:1], A[16383:16383 + 16382]])
    assert np.float32(1 / 16384) != np.float32(1 / 16383)
    check(kmc, cuda, lib, [ra, rb], s, mixture, mix, want_won=[0, 1], want_all=[1, 1], msg="1/16384, 1/16383")
    check(kmc, cuda, lib, [rb, ra], s, mixture, mix, want_won=[1, 0], want_all=[1, 1], msg="1/16383, 1/16384")


# 5. one round ------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_winners_chain_is_one_round(kmc, oracle, cuda, lib):
    """A holds x (1/1), B holds x and y (2/3), C holds y and z (2/4): x goes to A, y to B, z
    to C.  B's loss of x (it keeps 1/3, below C's 2/4) does not demote it for y."""
    mixture, mix, P, A = composed(oracle)
    x, y, z = P[20], P[21], P[22]
    ra, rb, rc = [x], [x, y, A[0]], [y, z, A[1], A[2]]
    check(kmc, cuda, lib, [ra, rb, rc], 4, mixture, mix, want_won=[1, 1, 1], want_all=[1, 2, 2])
    check(kmc, cuda, lib, [rc, rb, ra], 4, mixture, mix, want_won=[1, 1, 1], want_all=[2, 2, 1], msg="reversed")


# 6. UINT64_MAX contested ---------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_winners_uint64_max_is_contested(kmc, oracle, cuda, lib):
    """test_screen_uint64_max_is_a_value's construction (k = 31, KMC_CANON_FORWARD, seed 42: the
    mixture holds the 31-mer whose hash is UINT64_MAX, twice).  Row A holds it with one more
    found value and an absent one (2/3), row B with one more found value (2/2): B wins it in
    both orders.  With an index that lacks it, nobody does."""
    k, seed, s = 31, 42, 8
    key = int(S.unhash(np.array([S.FILL]), seed)[0])
    assert key < 1 << 62

    def make():
        rng = np.random.default_rng(1260)
        mer = kmer_of(key, k)
        others = [bases(rng, 31) for _ in range(2)]
        mixture = pack([others[0], mer, bases(rng, 300), np.concatenate([others[1], mer])])
        keys = [int("".join(str(b"ACGT".index(c)) for c in bytes(o)), 4) for o in others]
        mix = U.mixture_hashes(oracle, mixture[0], mixture[1], k, FWD, seed)
        return mixture, mix, S.hash_keys(np.array(keys, dtype=np.uint64), seed)
    mixture, mix, oh = cached("ffff", make)
    assert mix[0][-1] == S.FILL and mix[1][-1] == 2
    absent = np.uint64(12345)
    assert U.multiplicities(mix, [absent])[0] == 0 and (U.multiplicities(mix, oh) == 1).all()
    ra, rb = [oh[0], absent, S.FILL], [oh[1], S.FILL]
    for order, want_won, want_all in (((ra, rb), [1, 2], [2, 2]), ((rb, ra), [2, 1], [2, 2])):
        rows = np.full((2, s), S.FILL, dtype=np.uint64)
        for r, v in enumerate(order):
            rows[r, :len(v)] = v
        sizes = np.array([len(v) for v in order], dtype=np.uint32)
        exp = W.winners_expected(mix, rows, sizes, s, k)
        assert list(exp[0]) == want_won and list(exp[3]) == want_all
        assert exp[1][want_won.index(2)] == 1, "the lower median of multiplicities 1 and 2"
        with which(kmc, lib):
            _, got = winners(kmc, cuda, rows, sizes, mixture, k=k, flags=FWD, seed=seed)
            W.assert_winners(got, exp, "UINT64_MAX indexed")
            # an index without it: the rows still hold it, it is absent
            lacking = Q.pack([[oh[0], oh[1], absent]], s)
            _, got = winners(kmc, cuda, rows, sizes, mixture, k=k, flags=FWD, seed=seed, index_rows=lacking)
        exp = W.winners_expected((mix[0][:-1], mix[1][:-1]), rows, sizes, s, k)
        assert list(exp[0]) == [1, 1] and list(exp[3]) == [1, 1]
        W.assert_winners(got, exp, "UINT64_MAX not indexed")


# 7. no sharing ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_winners_without_sharing_equal_results(kmc, oracle, cuda, lib):
    """Disjoint rows: won, median and identity are kmc_sketch_screen_results' bit for bit."""
    import torch
    s = 300
    mixture, mix, P, A = composed(oracle)
    lists = [np.concatenate([P[100:350], A[:50]]), P[400:401], A[100:130], [], np.concatenate([P[500:600], A[200:377]]),
             P[1000:1300]]
    rows, sizes = Q.pack(lists, s)
    assert W.contested(mix, rows, sizes, s).size == 0
    with which(kmc, lib):
        index, got = winners(kmc, cuda, rows, sizes, mixture)
        res = U.host_results(kmc.sketch_screen_results(index, *device_rows(cuda, rows, sizes), K))
        torch.cuda.synchronize()
    assert list(got[0]) == [250, 1, 0, 0, 100, 300] and np.isnan(got[2][3]) and got[2][5] == 1.0 and 0 < got[2][4] < 1
    for a, b in zip(got, res + (res[0],)):
        assert a.tobytes() == b.tobytes()
    W.assert_winners(got, W.winners_expected(mix, rows, sizes, s, K))


# 8. foreign rows and stale state ------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_winners_foreign_rows_and_stale_state(kmc, oracle, cuda, lib):
    import torch
    s, s2 = 64, 50
    mixture, mix, P, A = composed(oracle)
    rng = np.random.default_rng(1280)
    built = Q.pack([P[:64], P[32:96], np.concatenate([P[90:120], A[:20]]), P[200:210]], s)
    indexed = np.unique(np.concatenate([built[0][r, :built[1][r]] for r in range(4)]))
    only_indexed = (indexed, U.multiplicities(mix, indexed))
    # rows of another sketch size: indexed values, values the mixture holds and the index lacks, absent ones
    f_lists = [np.concatenate([P[:20], P[300:325]]), np.concatenate([P[:30], A[100:105]]), P[300:350],
               A[200:230], np.concatenate([P[40:60], P[95:100]]), []]
    g_lists = [P[:50], P[10:40], P[200:205], A[300:310], np.concatenate([P[60:96], A[:10]]), P[25:26]]
    frows, fsizes = Q.pack(f_lists, s2)
    grows, gsizes = Q.pack(g_lists, s2)
    exp_f = W.winners_expected(only_indexed, frows, fsizes, s2, K)
    exp_g = W.winners_expected(only_indexed, grows, gsizes, s2, K)
    assert list(exp_f[3]) == [20, 30, 0, 0, 25, 0] and list(exp_f[0]) == [0, 30, 0, 0, 25, 0] and np.isnan(exp_f[2][5])
    assert (exp_g[0] != exp_f[0]).any()
    with which(kmc, lib):
        index, got = winners(kmc, cuda, frows, fsizes, mixture, index_rows=built)
        W.assert_winners(got, exp_f, "foreign rows, the library's workspace")
        fsk, fsz = device_rows(cuda, frows, fsizes)
        gsk, gsz = device_rows(cuda, grows, gsizes)
        need = kmc.sketch_screen_winners_workspace_size(index, 6)
        assert need > 0
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)

        def call(sk, sz, workspace=None):
            res = kmc.sketch_screen_winners(index, sk, sz, K, workspace=workspace)
            torch.cuda.synchronize()
            return W.host_winners(res)
        first = call(fsk, fsz, ws)  # over 0xFF bytes
        W.assert_winners(first, exp_f, "a caller's workspace")
        W.assert_winners(call(gsk, gsz, ws), exp_g, "other rows, the same workspace")
        again = call(fsk, fsz, ws)
        for a, b, c in zip(again, first, got):
            assert a.tobytes() == b.tobytes() == c.tobytes(), "nothing a former call left is read; NULL equals the caller's"
        with pytest.raises(kmc.KmcError) as ei:
            kmc.sketch_screen_winners(index, fsk, fsz, K, workspace=ws[:need - 256])
        assert ei.value.code == 1004
        with pytest.raises(kmc.KmcError) as ei:
            kmc.sketch_screen_winners(index, fsk, fsz, K, workspace=torch.empty(need + 8, dtype=torch.uint8, device=cuda)[4:])
        assert ei.value.code == 1003
        # the index is only read: results before and after are equal, and so are its bytes
        before = index.clone()
        r0 = U.host_results(kmc.sketch_screen_results(index, fsk, fsz, K))
        call(fsk, fsz)
        r1 = U.host_results(kmc.sketch_screen_results(index, fsk, fsz, K))
        torch.cuda.synchronize()
        assert torch.equal(index, before), "winners changed the index"
        for a, b in zip(r0, r1):
            assert a.tobytes() == b.tobytes()
        # count, winners, count, winners: the multiplicities accumulate
        d, di = U.device_records(cuda, *mixture)
        kmc.sketch_screen_count(index, d, di, K)
        twice = call(fsk, fsz, ws)
    exp2 = W.winners_expected((indexed, 2 * only_indexed[1]), frows, fsizes, s2, K)
    assert (exp2[1] == 2 * exp_f[1]).all() and (exp2[1] != exp_f[1]).any()
    W.assert_winners(twice, exp2, "after a second count")


# 10. the stream ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delay(kmc, cuda):
    kmc.lib()
    cycles, ms = T.sleep_cycles(T.DELAY_MS)
    assert ms >= 0.9 * T.DELAY_MS, "the delay spins %.1f ms, not %.1f" % (ms, T.DELAY_MS)
    return cycles


@pytest.fixture(scope="module")
def streams(kmc, cuda, delay):
    return T.side_streams(kmc, cuda, delay)


def check_winners(got, exp, msg):
    W.assert_winners((got[0].view(np.uint32), got[1].view(np.uint32), got[2], got[3].view(np.uint32)), exp, msg)


def case_winners(kmc, oracle, cuda):
    """The rows arrive late; the index is built and counted into beforehand.  The caller's
    workspace holds zeros, then 0xFF, when the call comes."""
    import torch
    s = 64
    mixture, mix, P, A = composed(oracle)
    real = Q.pack([P[:64], P[32:96], np.concatenate([P[90:120], A[:20]]), P[200:210], P[:10], []], s)
    decoy = Q.pack([P[200:210], P[:64], P[:10], np.concatenate([P[5:30], A[:8]]), A[50:60], P[300:301]], s)
    both = Q.pack([np.union1d(real[0][r, :real[1][r]], decoy[0][r, :decoy[1][r]]) for r in range(6)], 2 * s)
    sk, sz = device_rows(cuda, *real)
    dk, dz = device_rows(cuda, *decoy)
    index, _ = winners(kmc, cuda, both[0], both[1], mixture)
    exp = {"real": W.winners_expected(mix, real[0], real[1], s, K), "decoy": W.winners_expected(mix, decoy[0], decoy[1], s, K)}
    assert W.contested(mix, real[0], real[1], s).size > 0 and (exp["real"][0] != exp["real"][3]).any()
    r_live, s_live = torch.zeros_like(sk), torch.zeros_like(sz)
    ins = [(r_live, dk, sk), (s_live, dz, sz)]
    outs = [torch.empty(6, dtype=torch.int32, device=cuda), torch.empty(6, dtype=torch.int32, device=cuda),
            torch.empty(6, dtype=torch.float32, device=cuda), torch.empty(6, dtype=torch.int32, device=cuda)]
    ws = torch.zeros(kmc.sketch_screen_winners_workspace_size(index, 6), dtype=torch.uint8, device=cuda)

    def run(which_, stream):
        kmc.sketch_screen_winners(index, r_live, s_live, K, workspace=ws, out=tuple(outs), stream=stream)
    return T.Call("sketch_screen_winners", ins, outs, run, exp, check_winners, tuple, ws=ws)


@pytest.mark.parametrize("lib", LIBS)
def test_winners_late_input_on_a_side_stream(kmc, oracle, cuda, delay, streams, lib):
    with which(kmc, lib):
        T.late_call(case_winners(kmc, oracle, cuda), streams[0], delay)
