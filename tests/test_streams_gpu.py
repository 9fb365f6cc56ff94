"""The stream contract of include/kmc.h: every device entry point works on the stream
it is given (late-input harness, stream_util.py), does not wait for the device where
the header says "asynchronous" / "no host read-back", and calls with their own
workspaces and status words may overlap on different streams.

Expected values are the oracle's and the numpy helpers' of the entry points' own test
files, compared the way those files compare.  Only the two control cases observe a
reordering, and they read valid memory."""
import threading

import numpy as np
import pytest

import fasta_util as F
import sketch_group_util as GU
import sketch_query_util as Q
import sketch_util as S
import sparse_dist_util as U
import stream_util as T
from sketch_util import assert_sketch, dev, which
from test_dist_gpu import random_counts, same_floats
from test_hash_gpu import assert_same
from test_sketch_query_gpu import assert_nearest, assert_rect
from test_sketch_gpu import assert_distances

pytestmark = pytest.mark.gpu

cached = S.cache()
SOFT = 1

# Entry points include/kmc.h documents as synchronous on their stream: the harness does
# not assert that they return while the delay is spinning.
SYNCHRONOUS = {
    "count_canonical": "kmc_count_canonical_hash[_ex]: the distinct total is returned to the host",
    "parse_fasta_device": "kmc_fasta_parse_device: *num_seqs and *data_bytes are returned to the host",
    "load_fasta_device": "kmc_fasta_load_device: parses with kmc_fasta_parse_device, returns sizes (not run here: "
                         "it takes a path, no device input)",
    "count_multi": "kmc_count_multi: host buffers in and out, its own streams (not run here: no stream argument)",
}


@pytest.fixture(scope="module")
def delay(kmc, cuda):
    """Cycles of the device-side delay (stream_util.DELAY_MS), measured not guessed."""
    kmc.lib()
    cycles, ms = T.sleep_cycles(T.DELAY_MS)
    print("delay: %d cycles, %.1f ms (target %.1f ms)" % (cycles, ms, T.DELAY_MS))
    assert ms >= 0.9 * T.DELAY_MS, "the delay spins %.1f ms, not %.1f" % (ms, T.DELAY_MS)
    return cycles


@pytest.fixture(scope="module")
def streams(kmc, cuda, delay):
    """(s, t): non-blocking side streams (hipStreamGetFlags) that share no hardware queue
    with the null stream nor with each other (stream_util.side_streams): on a shared
    queue a misplaced launch would run in enqueue order and go unseen."""
    return T.side_streams(kmc, cuda, delay)


def empty(cuda, shape, dtype):
    import torch
    return torch.empty(shape, dtype=dtype, device=cuda)


def both(make):
    """{"decoy": make(0), "real": make(1)}"""
    return {"decoy": make(0), "real": make(1)}


def void(f):
    """run(which, stream) of a wrapper call whose result is the case's own out= tensors."""
    def run(w, st):
        f(w, st)
    return run


def recs():
    return cached("recs", lambda: (T.records(2, T.LENS_DECOY), T.records(1, T.LENS_REAL)))


def live_of(pair, cuda):
    """(live, decoy, real) device tensors of a (decoy, real) pair of host arrays."""
    d, r = dev(pair[0], cuda), dev(pair[1], cuda)
    assert d.shape == r.shape
    return (d.clone(), d, r)


def u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


# dense --------------------------------------------------------------------------------
def dense_check(got, exp, msg):
    for g, e, what in zip(got, exp, ("sum", "invalid", "status")):
        np.testing.assert_array_equal(g.reshape(np.asarray(e).shape), e, err_msg="%s %s" % (msg, what))


def case_dropin(kmc, oracle, cuda):
    import torch
    R = recs()
    n = 6
    data = live_of([r[0] for r in R], cuda)
    idx = live_of([r[1].astype(np.int32) for r in R], cuda)
    out = empty(cuda, 64 * n, torch.int32)
    exp = both(lambda w: (oracle.count_dense(R[w][0], R[w][1], 3)[0],))
    return T.Call("dropin_count", [data, idx], [out],
                  void(lambda w, st: kmc.dropin_count(data[0], idx[0], n, out=out, stream=st)),
                  exp, dense_check, lambda e: e)


def case_dense(kmc, oracle, cuda, k, ex=False):
    """count_dense (invalid, caller workspace of the _ex size) or count_dense_ex with its own status word."""
    import torch
    R = recs()
    n = 6
    data, idx = live_of([r[0] for r in R], cuda), live_of([r[1] for r in R], cuda)
    out = empty(cuda, (1 << (2 * k), n), torch.int32)
    inv = empty(cuda, n, torch.int32)
    need = kmc.dense_ex_workspace_size(kmc.dense_args(data[0], idx[0], k, out), torch.cuda.current_device())
    assert need > 0
    ws = empty(cuda, need, torch.uint8)
    exp = both(lambda w: oracle.count_dense(R[w][0], R[w][1], k) + ((np.zeros(1, np.int32),) if ex else ()))
    if ex:
        st_word = torch.zeros(1, dtype=torch.int32, device=cuda)

        def run(w, st):
            kmc.count_dense_ex(kmc.dense_args(data[0], idx[0], k, out, invalid=inv, workspace=ws, status=st_word),
                               stream=st)
        return T.Call("count_dense_ex k=%d" % k, [data, idx], [out, inv], run, exp, dense_check, lambda e: e, ws=ws,
                      zeroed=[st_word])

    def run(w, st):
        kmc.count_dense(data[0], idx[0], k, data_bytes=data[0].numel(), invalid=inv, workspace=ws, out=out, stream=st)
    return T.Call("count_dense k=%d" % k, [data, idx], [out, inv], run, exp, dense_check, lambda e: e, ws=ws)


# dense distances ----------------------------------------------------------------------
def case_pair_distances(kmc, oracle, cuda, n, k, split):
    """split None: whatever plan the device gives (a workspace when it asks for one)."""
    import torch
    C = [random_counts(np.random.default_rng(900 + 10 * n + k + w), n, k, 40) for w in (0, 1)]
    counts, idx = live_of([c[0] for c in C], cuda), live_of([c[1] for c in C], cuda)
    out = empty(cuda, n * (n - 1) // 2, torch.float32)
    need = kmc.pair_distances_workspace_size(n, k, torch.cuda.current_device())
    if split is not None:
        assert (need > 0) == split, "n=%d k=%d: workspace of %d bytes" % (n, k, need)
    ws = empty(cuda, need, torch.uint8) if need else None
    exp = both(lambda w: (oracle.pair_distances(C[w][0], np.diff(C[w][1]) - 1, k),))
    return T.Call("pair_distances n=%d k=%d" % (n, k), [counts, idx], [out],
                  void(lambda w, st: kmc.pair_distances(counts[0], idx[0], k, out=out, workspace=ws, stream=st)),
                  exp, lambda g, e, m: same_floats(g[0], e[0], m), lambda e: e, ws=ws)


def split_k(kmc):
    """The smallest k >= 9 at which three records take the split plan (a workspace)."""
    import torch
    for k in range(9, 14):
        if kmc.pair_distances_workspace_size(3, k, torch.cuda.current_device()) > 0:
            return k
    raise AssertionError("no split plan for three records at k = 9..13")


def case_min_kmeres2(kmc, oracle, cuda):
    import torch
    n = 12
    C = []
    for w in (0, 1):
        counts, idx = random_counts(np.random.default_rng(1200 + w), n, 3, 40)
        C.append((counts, idx.astype(np.int32)))
    sums, idx = live_of([c[0].reshape(-1) for c in C], cuda), live_of([c[1] for c in C], cuda)
    mins = empty(cuda, n * (n - 1) // 2, torch.float32)

    def expect(w):
        e = np.zeros(n * (n - 1) // 2, dtype=np.float32)
        for cur in range(n):
            oracle.min_kmeres2_row(C[w][0], C[w][1], cur, 3, e)
        return (e,)

    def run(w, st):
        for cur in range(n):
            kmc.min_kmeres2(sums[0], mins, n, cur, idx[0], stream=st)
    return T.Call("min_kmeres2 n=12", [sums, idx], [mins], run, both(expect),
                  lambda g, e, m: same_floats(g[0], e[0], m), lambda e: e)


# canonical ----------------------------------------------------------------------------
def canon_lists(oracle, k):
    """The oracle's SOFTMASK lists of the decoy and the real records, shuffled within records."""
    def make():
        out = []
        for w, (data, idx) in enumerate(recs()):
            keys, counts, off = oracle.count_canonical(data, idx, k, soft=True)
            keys, counts = U.shuffle_within_records(np.random.default_rng(50 + w), keys, counts, off)
            out.append((keys, counts, off))
        return out
    return cached(("lists", k), make)


def case_canonical(kmc, oracle, cuda, k, with_out=True):
    import torch
    R = recs()
    data, idx = live_of([r[0] for r in R], cuda), live_of([r[1] for r in R], cuda)
    cap = int(data[0].numel())
    outs = [empty(cuda, cap, torch.int64), empty(cuda, cap, torch.int32), empty(cuda, 7, torch.int64)]
    need = max(kmc.canonical_workspace_size(r[1], k, torch.cuda.current_device()) for r in R)
    ws = empty(cuda, need, torch.uint8)
    exp = both(lambda w: oracle.count_canonical(R[w][0], R[w][1], k, soft=True))

    def run(w, st):
        kw = {"out": outs} if with_out else {}
        return list(kmc.count_canonical(data[0], idx[0], k, flags=kmc.CANON_SOFTMASK, capacity=cap, workspace=ws,
                                        stream=st, **kw))

    def check(got, e, msg):
        keys, counts, off = got[-3:]
        assert keys.size == e[0].size, "%s: %d distinct, expected %d" % (msg, keys.size, e[0].size)
        np.testing.assert_array_equal(u64(off), e[2], err_msg="%s rec_offsets" % msg)
        assert_same((u64(keys), u32(counts), off), e, msg)
    return T.Call("count_canonical k=%d" % k, [data, idx], outs if with_out else [], run, exp, check,
                  lambda e: e, ws=ws)


def case_sparse(kmc, oracle, cuda):
    import torch
    k = 21
    R, L = recs(), canon_lists(oracle, k)
    E = [int(x[0].size) for x in L]
    keys = live_of([T.padded(x[0], max(E)).view(np.int64) for x in L], cuda)
    counts = live_of([T.padded(x[1], max(E)).view(np.int32) for x in L], cuda)
    off = live_of([x[2].view(np.int64) for x in L], cuda)
    idx = live_of([r[1] for r in R], cuda)
    out = empty(cuda, 15, torch.float32)
    ws = empty(cuda, kmc.pair_distances_sparse_workspace_size(6, max(E), torch.cuda.current_device()), torch.uint8)
    exp = both(lambda w: (U.canonical_expected(oracle, R[w][0], R[w][1], k, soft=True),))
    assert (np.nan_to_num(exp["real"][0], nan=1.0) < 1).any()
    return T.Call("pair_distances_sparse", [keys, counts, off, idx], [out],
                  void(lambda w, st: kmc.pair_distances_sparse(keys[0], counts[0], off[0], idx[0], k, num_entries=E[w == "real"],
                                                          out=out, workspace=ws, stream=st)),
                  exp, lambda g, e, m: same_floats(g[0], e[0], m), lambda e: e, ws=ws)


# sketches -----------------------------------------------------------------------------
def sketch_check(got, exp, msg):
    assert_sketch((u64(got[0]), u32(got[1])), exp, msg)


def case_sketch_from_counts(kmc, oracle, cuda, s):
    import torch
    L = canon_lists(oracle, 21)
    E = [int(x[0].size) for x in L]
    keys = live_of([T.padded(x[0], max(E)).view(np.int64) for x in L], cuda)
    off = live_of([x[2].view(np.int64) for x in L], cuda)
    outs = [empty(cuda, (6, s), torch.int64), empty(cuda, 6, torch.int32)]
    need = kmc.sketch_workspace_size(6, max(E), s, torch.cuda.current_device())
    assert need > 0
    ws = empty(cuda, need, torch.uint8)
    exp = both(lambda w: S.sketch_expected(L[w][0], None, L[w][2], 6, s))
    return T.Call("sketch_from_counts s=%d" % s, [keys, off], outs,
                  void(lambda w, st: kmc.sketch_from_counts(keys[0], None, off[0], s, workspace=ws, num_entries=E[w == "real"],
                                                       out=outs, stream=st)),
                  exp, sketch_check, lambda e: e, ws=ws)


GROUPS = ([0, 1, 1, 4, 6], [0, 0, 2, 3, 6])   # decoy, real


def seq_expected(oracle, s, grouped):
    def make():
        R = recs()
        return both(lambda w: GU.grouped_expected(oracle, R[w][0], R[w][1], GROUPS[w] if grouped else np.arange(7), 21, s,
                                                  flags=SOFT))
    return cached(("seq", s, grouped), make)


def case_sketch_from_sequences(kmc, oracle, cuda, s, grouped, with_ws):
    import torch
    R = recs()
    data, idx = live_of([r[0] for r in R], cuda), live_of([r[1] for r in R], cuda)
    ins = [data, idx]
    rows = 4 if grouped else 6
    outs = [empty(cuda, (rows, s), torch.int64), empty(cuda, rows, torch.int32)]
    dv = torch.cuda.current_device()
    ws = None
    if grouped:
        grp = live_of([np.asarray(g, dtype=np.int64) for g in GROUPS], cuda)
        ins.append(grp)
        if with_ws:
            ws = empty(cuda, kmc.sketch_from_sequences_grouped_workspace_size(6, 4, data[0].numel(), s, dv), torch.uint8)

        def run(w, st):
            kmc.sketch_from_sequences_grouped(data[0], idx[0], grp[0], 21, s, flags=SOFT, workspace=ws, out=outs, stream=st)
    else:
        if with_ws:
            ws = empty(cuda, kmc.sketch_from_sequences_workspace_size(6, data[0].numel(), s, dv), torch.uint8)

        def run(w, st):
            kmc.sketch_from_sequences(data[0], idx[0], 21, s, flags=SOFT, workspace=ws, out=outs, stream=st)
    name = "sketch_from_sequences%s s=%d" % ("_grouped" if grouped else "", s)
    return T.Call(name, ins, outs, run, seq_expected(oracle, s, grouped), sketch_check, lambda e: e, ws=ws)


def case_merge_groups(kmc, oracle, cuda, s=16, strided=False):
    """The per-record rows of sketch_from_sequences merged by GROUPS; strided: the rows
    are the left half of a wider tensor, so the wrapper's .contiguous() copies."""
    import torch
    per = seq_expected(oracle, s, False)
    P = (per["decoy"], per["real"])
    rows = live_of([p[0].view(np.int64) for p in P], cuda)
    if strided:
        wide = torch.zeros((6, 2 * s), dtype=torch.int64, device=cuda)
        rows = (wide[:, :s], rows[1], rows[2])
        assert not rows[0].is_contiguous()
    sizes = live_of([p[1].view(np.int32) for p in P], cuda)
    grp = live_of([np.asarray(g, dtype=np.int64) for g in GROUPS], cuda)
    outs = [] if strided else [empty(cuda, (4, s), torch.int64), empty(cuda, 4, torch.int32)]
    exp = both(lambda w: GU.merged_expected(P[w][0], P[w][1], GROUPS[w], s))

    def run(w, st):
        if strided:   # (the wrapper's own outputs: the call as kmc.py took it before out= existed)
            return list(kmc.sketch_merge_groups(rows[0], sizes[0], grp[0], stream=st))
        kmc.sketch_merge_groups(rows[0], sizes[0], grp[0], out=outs, stream=st)
    return T.Call("sketch_merge_groups", [rows, sizes, grp], outs, run, exp, sketch_check, lambda e: e)


def row_sets(cuda, n, s=64):
    P = [T.overlap_rows(3000 + w, n, s) for w in (0, 1)]
    return P, live_of([p[0].view(np.int64) for p in P], cuda), live_of([p[1].view(np.int32) for p in P], cuda)


def case_sketch_distances(kmc, oracle, cuda):
    import torch
    n, s, k = 6, 64, 21
    P, rows, sizes = row_sets(cuda, n)
    npairs = n * (n - 1) // 2
    outs = [empty(cuda, npairs, torch.float32), empty(cuda, npairs, torch.int32), empty(cuda, npairs, torch.int32)]
    exp = both(lambda w: S.distances_expected(P[w][0], P[w][1], s, k))
    return T.Call("sketch_distances", [rows, sizes], outs,
                  void(lambda w, st: kmc.sketch_distances(rows[0], sizes[0], k, with_counts=True, out=outs, stream=st)),
                  exp, lambda g, e, m: assert_distances((g[0], u32(g[1]), u32(g[2])), e, m), lambda e: e)


def query_sets(cuda, seed, m=2, n=6, s=64):
    """Queries (rows 2, 3 of one overlap_rows pool) and references (the other rows: a full
    and an empty one among them), decoy and real: (P, q, qs, r, rs) with P[w] = host (q, qs, r, rs)."""
    P = []
    for w in (0, 1):
        rows, sizes = T.overlap_rows(seed + w, m + n, s)
        P.append((rows[2:2 + m], sizes[2:2 + m], np.delete(rows, (2, 3), 0), np.delete(sizes, (2, 3))))
    live = [live_of([np.ascontiguousarray(p[i]).view(np.int32 if i % 2 else np.int64) for p in P], cuda)
            for i in range(4)]
    return [P] + live


def case_rect(kmc, oracle, cuda):
    import torch
    m, n, s, k = 2, 6, 64, 21
    P, q, qs, r, rs = query_sets(cuda, 3200)
    outs = [empty(cuda, (m, n), torch.float32), empty(cuda, (m, n), torch.int32), empty(cuda, (m, n), torch.int32)]
    exp = both(lambda w: Q.rect_expected(*P[w], s, k))
    return T.Call("sketch_distances_rect", [q, qs, r, rs], outs,
                  void(lambda w, st: kmc.sketch_distances_rect(q[0], qs[0], r[0], rs[0], k, with_counts=True, out=outs,
                                                               stream=st)),
                  exp, lambda g, e, m_: assert_rect((g[0], u32(g[1]), u32(g[2])), e, m_), lambda e: e)


def case_nearest(kmc, oracle, cuda):
    import torch
    m, n, s, k, top = 2, 6, 64, 21, 3
    P, q, qs, r, rs = query_sets(cuda, 3100)
    outs = [empty(cuda, (m, top), torch.int32), empty(cuda, (m, top), torch.int32), empty(cuda, (m, top), torch.int32),
            empty(cuda, (m, top), torch.float32), empty(cuda, m, torch.int32)]
    need = kmc.sketch_nearest_workspace_size(m, n, s, top, torch.cuda.current_device())
    assert need > 0
    ws = empty(cuda, need, torch.uint8)
    exp = both(lambda w: Q.nearest_expected(Q.rect_expected(*P[w], s, k), top, 0))
    return T.Call("sketch_nearest", [q, qs, r, rs], outs,
                  void(lambda w, st: kmc.sketch_nearest(q[0], qs[0], r[0], rs[0], k, top, min_shared=0, workspace=ws, out=outs,
                                                   stream=st)),
                  exp, lambda g, e, m_: assert_nearest((u32(g[0]), u32(g[1]), u32(g[2]), g[3], u32(g[4])), e, m_),
                  lambda e: e, ws=ws)


# synthetic and parse ------------------------------------------------------------------
SYNTH = (3, 10_000)
SEEDS = {"decoy": 0x5EED0001, "real": 0x5EED0008}


def case_synth(kmc, oracle, cuda, ranged):
    import torch
    nrec, L = SYNTH
    lo, hi = (4093, 2 * (L + 1) + 77) if ranged else (0, nrec * (L + 1))
    buf = empty(cuda, hi - lo + 64, torch.uint8)
    if ranged:
        exp = both(lambda w: (kmc.synth_host_range(lo, hi, L, SEEDS[("decoy", "real")[w]]),))
    else:
        exp = both(lambda w: (kmc.synth_host(nrec, L, SEEDS[("decoy", "real")[w]], 17),))

    def run(w, st):
        if ranged:
            kmc.synth_fill_range(buf, lo, hi, L, SEEDS[w], stream=st)
        else:
            kmc.synth_fill(buf, nrec, L, SEEDS[w], 17, stream=st)

    def check(got, e, msg):
        np.testing.assert_array_equal(got[0][:hi - lo], e[0], err_msg=msg)
        assert (got[0][hi - lo:] == T.POISON).all(), "%s: bytes written past the end" % msg
    return T.Call("synth_fill_range" if ranged else "synth_fill", [], [buf], run, exp, check, lambda e: e)


def case_parse(kmc, oracle, cuda, tmp_path, dialect):
    raws = (F.one_motif_input("nl_nl", F.FP_TILE, 0), F.one_motif_input("nl_cr_text", 2 * F.FP_TILE, 2))
    assert len(raws[0]) == len(raws[1]) and len(raws[1]) % 16
    raw = live_of([np.frombuffer(x, dtype=np.uint8) for x in raws], cuda)

    def expect(w):
        path = str(tmp_path / ("h%d.fa" % w))
        with open(path, "wb") as f:
            f.write(raws[w])
        return kmc.load_fasta(path, dialect, 0)[:2]

    def check(got, e, msg):
        np.testing.assert_array_equal(got[1], e[1], err_msg="%s indices" % msg)
        np.testing.assert_array_equal(got[0], e[0], err_msg="%s data" % msg)
    return T.Call("parse_fasta_device dialect %d" % dialect, [raw], [],
                  lambda w, st: list(kmc.parse_fasta_device(raw[0], dialect, stream=st)), both(expect), check, lambda e: e)


# 1. + 2. the late-input harness over every entry point ----------------------------------
CASES = {
    "dropin_count": ("ship", lambda *a: case_dropin(*a)),
    "count_dense-k5": ("ship", lambda *a: case_dense(*a, 5)),
    "count_dense-k8": ("ship", lambda *a: case_dense(*a, 8)),
    "count_dense-k11": ("ship", lambda *a: case_dense(*a, 11)),
    "count_dense-k11-sampled": ("diag-sampled", lambda *a: case_dense(*a, 11)),
    "count_dense_ex-k8-status": ("ship", lambda *a: case_dense(*a, 8, ex=True)),
    # (on 256 CUs n = 20, k = 4 is a plan of two splits with a workspace; k = 3 is the unsplit one)
    "pair_distances-n20-k4": ("ship", lambda *a: case_pair_distances(*a, 20, 4, None)),
    "pair_distances-n20-k3-unsplit": ("ship", lambda *a: case_pair_distances(*a, 20, 3, False)),
    "pair_distances-n3-split": ("ship", lambda kmc, *a: case_pair_distances(kmc, *a, 3, split_k(kmc), True)),
    "min_kmeres2": ("ship", lambda *a: case_min_kmeres2(*a)),
    "count_canonical-k21": ("ship", lambda *a: case_canonical(*a, 21)),
    "count_canonical-k31": ("ship", lambda *a: case_canonical(*a, 31)),
    "pair_distances_sparse": ("ship", lambda *a: case_sparse(*a)),
    "synth_fill": ("ship", lambda *a: case_synth(*a, False)),
    "synth_fill_range": ("ship", lambda *a: case_synth(*a, True)),
}
for _lib in ("ship", "diag"):
    CASES.update({
        "sketch_from_counts-s64-" + _lib: (_lib, lambda *a: case_sketch_from_counts(*a, 64)),
        "sketch_from_counts-s1000-" + _lib: (_lib, lambda *a: case_sketch_from_counts(*a, 1000)),
        "sketch_from_sequences-s16-" + _lib: (_lib, lambda *a: case_sketch_from_sequences(*a, 16, False, False)),
        "sketch_from_sequences-s1000-ws-" + _lib: (_lib, lambda *a: case_sketch_from_sequences(*a, 1000, False, True)),
        "sketch_from_sequences_grouped-s16-" + _lib: (_lib, lambda *a: case_sketch_from_sequences(*a, 16, True, False)),
        "sketch_from_sequences_grouped-s1000-ws-" + _lib: (_lib, lambda *a: case_sketch_from_sequences(*a, 1000, True, True)),
        "sketch_merge_groups-" + _lib: (_lib, lambda *a: case_merge_groups(*a)),
        "sketch_distances-" + _lib: (_lib, lambda *a: case_sketch_distances(*a)),
        "sketch_distances_rect-" + _lib: (_lib, lambda *a: case_rect(*a)),
        "sketch_nearest-" + _lib: (_lib, lambda *a: case_nearest(*a)),
    })


def library(kmc, lib):
    """The context of a case's library; "diag-sampled": the diagnostic one with the
    sampled radix pipeline forced (kmc_diag_radix_mode(2, 1.0))."""
    if lib != "diag-sampled":
        return which(kmc, lib)

    class sampled:
        def __enter__(self):
            self.ctx = kmc.diag()
            assert self.ctx.__enter__().kmc_diag_radix_mode(2, 1.0) == 0

        def __exit__(self, *exc):
            return self.ctx.__exit__(*exc)
    return sampled()


@pytest.mark.parametrize("name", list(CASES))
def test_late_input(kmc, oracle, cuda, delay, streams, name):
    lib, make = CASES[name]
    s = streams[0]
    with library(kmc, lib):
        call = make(kmc, oracle, cuda)
        T.late_call(call, s, delay, asynchronous=call.name.split()[0] not in SYNCHRONOUS)
    print("%s: warm-up %.3f ms" % (call.name, T.WARM_MS[call.name]))


@pytest.mark.parametrize("dialect", [0, 1])
def test_late_input_parse_fasta(kmc, oracle, cuda, delay, streams, tmp_path, dialect):
    assert "parse_fasta_device" in SYNCHRONOUS
    T.late_call(case_parse(kmc, oracle, cuda, tmp_path, dialect), streams[0], delay, asynchronous=False)


@pytest.mark.parametrize("name", ["pair_distances-n20-k4", "sketch_from_sequences-s1000-ws-ship"])
def test_control_second_stream_reads_the_decoy(kmc, oracle, cuda, delay, streams, name):
    """The harness cannot pass vacuously: with the library on a second side stream the
    reordering is observed (the decoy's result), so the delay is long enough and the
    streams do not order against each other on this machine."""
    T.control_call(CASES[name][1](kmc, oracle, cuda), streams[0], streams[1], delay)


# 4. the wrapper's stream= argument ------------------------------------------------------
@pytest.mark.parametrize("name", ["count_canonical", "sketch_merge_groups"])
def test_explicit_stream_argument(kmc, oracle, cuda, delay, streams, name):
    """stream=s with the default stream left current: the wrapper's own tensor work
    (count_canonical's allocations and zeroing, sketch_merge_groups' .contiguous() copy
    of a strided row view) runs on s too.  Before kmc.py did that, the merge case read
    the decoy; the canonical case passed (its wrapper's work finished before the
    library's began, whichever stream it was on)."""
    import torch
    s = streams[0]
    call = case_canonical(kmc, oracle, cuda, 21, with_out=False) if name == "count_canonical" else \
        case_merge_groups(kmc, oracle, cuda, strided=True)
    T.warm_up(call)
    call.stage("decoy", 0)
    torch.cuda.synchronize()
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(delay)
        call.stage("real", 0xFF)
    extra = call.run("real", s) or []          # the default stream is current here
    with torch.cuda.stream(s):
        snaps = [x.clone() if isinstance(x, torch.Tensor) else x for x in call.results() + list(extra)]
    s.synchronize()
    call.check([x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in snaps], call.exp["real"],
               "%s stream=s, default stream current" % call.name)


# 3. overlapping calls -------------------------------------------------------------------
BIG_LENS = ([700_001, 600_000, 700_000], [650_003, 700_000, 649_999])
ROUNDS = 8


def big():
    return cached("big", lambda: [T.records(70 + w, BIG_LENS[w], b"ACGTN", (.2475, .2475, .2475, .2475, .01))
                                  for w in (0, 1)])


def overlap_dense(kmc, oracle, cuda, k):
    """Per input: enqueue(stream) -> fresh outputs, verify(outputs)."""
    import torch
    jobs = []
    for data, idx in big():
        d, di = dev(data, cuda), dev(idx, cuda)
        exp = [dev(x, cuda) for x in oracle.count_dense(data, idx, k)]
        probe = empty(cuda, (1 << (2 * k), 3), torch.int32)
        ws = empty(cuda, kmc.dense_ex_workspace_size(kmc.dense_args(d, di, k, probe), torch.cuda.current_device()),
                   torch.uint8)
        word = torch.zeros(1, dtype=torch.int32, device=cuda)

        def enqueue(st, d=d, di=di, ws=ws, word=word):
            with torch.cuda.stream(st):
                out, inv = torch.empty_like(probe), empty(cuda, 3, torch.int32)
            kmc.count_dense_ex(kmc.dense_args(d, di, k, out, invalid=inv, workspace=ws, status=word), stream=st)
            return out, inv

        def verify(res, msg, exp=exp, word=word):
            assert int(word.item()) == 0, "%s: status word %d" % (msg, int(word.item()))
            assert torch.equal(res[0], exp[0]) and torch.equal(res[1], exp[1]), "%s: counts differ from the oracle" % msg
        jobs.append((enqueue, verify))
    return jobs


def overlap_sparse(kmc, oracle, cuda):
    import torch
    k = 21
    jobs = []
    for w, (data, idx) in enumerate(big()):
        keys, counts, off = oracle.count_canonical(data, idx, k)
        exp = U.distances_from_sums(U.pair_sums(keys, counts, off, 3), np.diff(idx) - 1, k)
        assert ((exp > 0) & (exp < 1)).all()
        dk, dc, do = dev(keys.view(np.int64), cuda), dev(counts.view(np.int32), cuda), dev(off.view(np.int64), cuda)
        di = dev(idx, cuda)
        ws = empty(cuda, kmc.pair_distances_sparse_workspace_size(3, keys.size, torch.cuda.current_device()), torch.uint8)

        def enqueue(st, a=(dk, dc, do, di), ws=ws):
            with torch.cuda.stream(st):
                out = empty(cuda, 3, torch.float32)
            return (kmc.pair_distances_sparse(*a, k, out=out, workspace=ws, stream=st),)

        def verify(res, msg, exp=exp):
            same_floats(res[0].cpu().numpy(), exp, msg)
        jobs.append((enqueue, verify))
    return jobs


def overlap_sketch_seq(kmc, oracle, cuda):
    import torch
    k, s = 21, 1000
    jobs = []
    for data, idx in big():
        exp = GU.grouped_expected(oracle, data, idx, np.arange(4), k, s)
        d, di = dev(data, cuda), dev(idx, cuda)
        ws = empty(cuda, kmc.sketch_from_sequences_workspace_size(3, data.size, s, torch.cuda.current_device()), torch.uint8)

        def enqueue(st, d=d, di=di, ws=ws):
            with torch.cuda.stream(st):
                outs = (empty(cuda, (3, s), torch.int64), empty(cuda, 3, torch.int32))
            return kmc.sketch_from_sequences(d, di, k, s, workspace=ws, out=outs, stream=st)

        def verify(res, msg, exp=exp):
            sketch_check([x.cpu().numpy() for x in res], exp, msg)
        jobs.append((enqueue, verify))
    return jobs


def overlap_nearest(kmc, oracle, cuda):
    import torch
    m, n, s, k, top = 8, 1500, 64, 21, 3
    jobs = []
    for w in (0, 1):
        rows, sizes = T.overlap_rows(4000 + w, m + n, s)
        exp = Q.nearest_expected(Q.rect_expected(rows[2:2 + m], sizes[2:2 + m], rows, sizes, s, k), top, 0)
        a = (dev(rows[2:2 + m].view(np.int64), cuda), dev(sizes[2:2 + m].view(np.int32), cuda),
             dev(rows.view(np.int64), cuda), dev(sizes.view(np.int32), cuda))
        ws = empty(cuda, kmc.sketch_nearest_workspace_size(m, m + n, s, top, torch.cuda.current_device()), torch.uint8)

        def enqueue(st, a=a, ws=ws):
            with torch.cuda.stream(st):
                outs = [empty(cuda, (m, top), torch.int32) for _ in range(3)] + \
                       [empty(cuda, (m, top), torch.float32), empty(cuda, m, torch.int32)]
            return kmc.sketch_nearest(*a, k, top, min_shared=0, workspace=ws, out=outs, stream=st)

        def verify(res, msg, exp=exp):
            g = [x.cpu().numpy() for x in res]
            assert_nearest((u32(g[0]), u32(g[1]), u32(g[2]), g[3], u32(g[4])), exp, msg)
        jobs.append((enqueue, verify))
    return jobs


OVERLAP = {
    "count_dense_ex-k8": lambda *a: overlap_dense(*a, 8),
    "count_dense_ex-k11": lambda *a: overlap_dense(*a, 11),
    "pair_distances_sparse": overlap_sparse,
    "sketch_from_sequences-s1000": overlap_sketch_seq,
    "sketch_nearest": overlap_nearest,
}


@pytest.mark.parametrize("name", list(OVERLAP))
def test_async_calls_overlap(kmc, oracle, cuda, name):
    """Inputs A and B, each with its own outputs, workspace and status word, enqueued
    alternately on two side streams from one host thread, eight rounds, without a host
    synchronisation in between: all sixteen results are the oracle's."""
    import torch
    (enq_a, ver_a), (enq_b, ver_b) = OVERLAP[name](kmc, oracle, cuda)
    s1, s2 = torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    res = []
    for _ in range(ROUNDS):
        res.append((enq_a(s1), enq_b(s2)))
    s1.synchronize()
    s2.synchronize()
    for i, (ra, rb) in enumerate(res):
        ver_a(ra, "%s round %d input A" % (name, i))
        ver_b(rb, "%s round %d input B" % (name, i))
    if name.startswith("count_dense"):
        assert kmc.lib().kmc_dense_status(torch.cuda.current_device()) == 0


def test_canonical_calls_overlap_from_two_threads(kmc, oracle, cuda):
    """kmc_count_canonical_hash_ex is synchronous: two host threads (ctypes drops the
    GIL in the call), each with its own stream and workspace, four calls of A or of B."""
    import torch
    k = 31
    dv = torch.cuda.current_device()
    work = []
    for data, idx in big():
        ws = empty(cuda, kmc.canonical_workspace_size(idx, k, dv), torch.uint8)
        work.append(dict(d=dev(data, cuda), di=dev(idx, cuda), ws=ws, st=torch.cuda.Stream(device=cuda), got=[], err=[],
                         exp=oracle.count_canonical(data, idx, k)))
    torch.cuda.synchronize()

    def worker(w):
        try:
            torch.cuda.set_device(dv)
            for _ in range(4):
                w["got"].append(kmc.count_canonical(w["d"], w["di"], k, workspace=w["ws"], stream=w["st"]))
        except BaseException as e:   # reported by the main thread
            w["err"].append(e)

    threads = [threading.Thread(target=worker, args=(w,)) for w in work]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    for name, w in zip("AB", work):
        assert not w["err"], "thread %s: %r" % (name, w["err"])
        assert len(w["got"]) == 4
        for i, (keys, counts, off) in enumerate(w["got"]):
            assert_same((u64(keys.cpu().numpy()), u32(counts.cpu().numpy()), off.cpu().numpy()), w["exp"],
                        "input %s call %d" % (name, i))


# kmc_dense.hip / kmc_stream.h: tiles of kTile = 1024 bytes, dealt to G = one 1024-thread
# workgroup per CU (tiles rounded up per workgroup).  A workgroup whose piece of a poly-A
# record holds W windows wraps its 16-bit AAAAAAAA counter W / 65 536 times and emits at
# least one spill entry per wrap, so more entries than the forced capacity of 1 need two
# wraps in a piece: 2 * 65 536 windows per workgroup, plus 8 tiles each for the rounding
# (34 MB on 256 CUs; test_dense_spill_overflow_raises_status uses 64 MB).
K_TILE = 1024


def test_dense_status_words_stay_apart(kmc, oracle, cuda):
    """A (poly-A, overflows its spill lists under kmc_diag_dense_spill_cap(1)) and B
    (random records) interleaved on two streams, each with its own status word: A's
    reads KMC_ERR_CAPACITY, B's 0, B's counts are the oracle's, the device flag is 0."""
    import torch
    dv = torch.cuda.current_device()
    G = torch.cuda.get_device_properties(dv).multi_processor_count
    size = 2 * 65_536 * G + 8 * K_TILE * G    # two wraps in every workgroup's piece, and tile rounding
    a_data = np.append(np.full(size, ord("A"), np.uint8), np.uint8(0))
    a_idx = np.array([0, a_data.size], dtype=np.int64)
    b_data, b_idx = big()[1]
    exp_b = [dev(x, cuda) for x in oracle.count_dense(b_data, b_idx, 8)]
    s1, s2 = torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)
    with kmc.diag() as D:
        jobs = []
        for data, idx in ((a_data, a_idx), (b_data, b_idx)):
            d, di = dev(data, cuda), dev(idx, cuda)
            out = empty(cuda, (1 << 16, idx.size - 1), torch.int32)
            inv = empty(cuda, idx.size - 1, torch.int32)
            word = torch.zeros(1, dtype=torch.int32, device=cuda)
            jobs.append([d, di, out, inv, word, None])
        try:
            assert D.kmc_diag_dense_spill_cap(1) == 0
            for j in jobs:   # (the workspace size depends on the cap)
                j[5] = empty(cuda, kmc.dense_ex_workspace_size(kmc.dense_args(j[0], j[1], 8, j[2]), dv), torch.uint8)
            torch.cuda.synchronize()
            for _ in range(2):
                for (d, di, out, inv, word, ws), st in zip(jobs, (s1, s2)):
                    kmc.count_dense_ex(kmc.dense_args(d, di, 8, out, invalid=inv, workspace=ws, status=word), stream=st)
            s1.synchronize()
            s2.synchronize()
            assert int(jobs[0][4].item()) == kmc.KMC_ERR_CAPACITY
            assert int(jobs[1][4].item()) == 0
            assert torch.equal(jobs[1][2], exp_b[0]) and torch.equal(jobs[1][3], exp_b[1])
            assert D.kmc_dense_status(dv) == 0
        finally:
            D.kmc_diag_dense_spill_cap(0)
