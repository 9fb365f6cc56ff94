"""The canonical counter's front half at its edges: K1
(canon_count_kernel), K3a (canon_coarse_kernel, staged_round), the list starts, K3b
(canon_fine_kernel, the Ring8 LDS rings) and the walk they share
(kmc_canon_walk.h: for_each_piece, chunk_raw, chunk_keys).

Every case is compared with the self-oracle (oracle.count_canonical): per-record
sorted (key, count) sets bit for bit, and rec_off.  The small and the constructed
inputs are also compared with np_count below, a numpy restatement over the k-mers
the test laid down.  No case assumes the path it is named after: each asserts it
from plan(), a Python mirror of canon_plan, from k3a_groups / k3b_fill_bounds
(which entries a K3b round can hold) or from the oracle's per-list counts.

Part A (walk edges) needs no hook.  Parts B and C set the windows-per-list target
with kmc_diag_canon_list_target (diagnostic library), so that records of up to
1 MiB have every K3b geometry lf = 1 .. 8 (lf = log2 lists per coarse bucket; ring
entries per list R = 2^(14 - lf)).

Controlled occupancy (part C): a record made of 31-mers separated by one N each has
one valid window per 32 bytes; under KMC_CANON_FORWARD its key is the 31-mer.  The
partition value is m = key * C mod 2^64 (coarse bucket: top 7 bits; list: top lg
bits), and C is odd, so a key of a wanted list is m * C^-1 for an m with those top
bits, kept when it is below 4^31 (one draw in four).  K3a writes a coarse bucket's
entries in input order up to the order inside one of its rounds of one workgroup
(k3a_groups); 16 400 bytes of N between two sections keep them in separate groups.
"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MUL_C = 0x9E3779B97F4A7C15
MUL_CINV = pow(MUL_C, -1, 1 << 64)
KC = 31                       # k of the constructed records
SEG = 16                      # entries per K3b segment (kSeg)
K3B_ROUND = 8192              # entries per K3b round
K3A_ROUND_CHUNKS = 1024       # chunks per K3a round
GROUP_PAD = 16 * K3A_ROUND_CHUNKS + 16  # bytes of N no K3a round of one workgroup spans
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N_BYTE = np.uint8(ord("N"))


# ---------------------------------------------------------------------------
# the mirrors
# ---------------------------------------------------------------------------
def cu_count(cuda):
    import torch
    return torch.cuda.get_device_properties(cuda).multi_processor_count


def plan(idx, k, cus, target=4096):
    """canon_plan: G workgroups of cpw chunks from chunk c_lo; per record lg, w0, nwg;
    M counters; K3b workgroups (128 per record with lg > 7 and a window)."""
    idx = [int(x) for x in idx]
    n = len(idx) - 1
    lo, hi = idx[0], idx[n]
    c_lo = lo >> 4
    chunks = ((hi + 15) >> 4) - c_lo if hi > lo else 0
    G = max(1, min(cus, chunks))
    cpw = max(1, (chunks + G - 1) // G)
    lg, w0, nwg = [], [], []
    M = Mc = L = windows = k3b = 0
    for r in range(n):
        a, nw = idx[r], max(0, idx[r + 1] - idx[r] - k)
        windows += nw
        g = 0
        while g < 15 and (target << g) < nw:
            g += 1
        gc = min(g, 7)
        f = n_ = 0
        if nw > 0:
            f = ((a >> 4) - c_lo) // cpw
            n_ = (((a + nw - 1) >> 4) - c_lo) // cpw - f + 1
        lg.append(g)
        w0.append(f)
        nwg.append(n_)
        M += (1 << g) * n_
        Mc += (1 << gc) * n_
        L += 1 << g
        if g > gc and nw > 0:
            k3b += 1 << gc
    return types.SimpleNamespace(c_lo=c_lo, G=G, cpw=cpw, lg=lg, w0=w0, nwg=nwg, M=M, Mc=Mc, L=L,
                                 windows=windows, k3b=k3b)


def pieces(idx, k, P):
    """for_each_piece: (workgroup, record, ps, pe) of every record piece."""
    idx = [int(x) for x in idx]
    n = len(idx) - 1
    out = []
    for w in range(P.G):
        cb = P.c_lo + w * P.cpw
        wlo, whi = max(cb << 4, idx[0]), min((cb + P.cpw) << 4, idx[n])
        if wlo >= whi:
            continue
        for r in range(n):
            a, e = idx[r], idx[r + 1]
            ps, pe = max(a, wlo), min(a + max(e - a - k, 0), whi)
            if ps < pe:
                out.append((w, r, ps, pe))
    return out


def piece_chunks(ps, pe):
    return ((pe - 1) >> 4) + 1 - (ps >> 4)


def part(keys):
    with np.errstate(over="ignore"):
        return np.asarray(keys, dtype=np.uint64) * np.uint64(MUL_C)


def bucket_of(keys):
    return (part(keys) >> np.uint64(57)).astype(np.int64)


def list_of(keys, lg):
    return (part(keys) >> np.uint64(64 - lg)).astype(np.int64)


def k3a_groups(pos, a, P):
    """The (workgroup, K3a round) of window starts `pos` of the record starting at a,
    as one increasing id: K3a writes a bucket's entries group by group, in any order
    inside a group."""
    pos = np.asarray(pos, dtype=np.int64)
    w = ((pos >> 4) - P.c_lo) // P.cpw
    ps = np.maximum(a, (P.c_lo + w * P.cpw) << 4)
    return w * (1 << 20) + ((pos >> 4) - (ps >> 4)) // K3A_ROUND_CHUNKS


def k3b_fill_bounds(lists, groups, first, F):
    """Least and most entries each of the F lists from `first` on can take in each
    K3b round of a bucket whose entries, in input order, go to `lists` and lie in
    K3a `groups`: of a group that straddles a round boundary the round holds a
    known number of entries, but any of them.  Returns (lo, hi), each [rounds, F]."""
    lists = np.asarray(lists) - first
    groups = np.asarray(groups)
    n = lists.size
    rounds = max(1, -(-n // K3B_ROUND))
    lo = np.zeros((rounds, F), dtype=np.int64)
    hi = np.zeros((rounds, F), dtype=np.int64)
    for t in range(rounds):
        b0, b1 = t * K3B_ROUND, min(n, (t + 1) * K3B_ROUND)
        sure = np.zeros(n, dtype=bool)
        sure[b0:b1] = True
        for g in {int(groups[b0]), int(groups[b1 - 1])}:
            at = np.flatnonzero(groups == g)
            if at[0] >= b0 and at[-1] < b1:
                continue  # the whole group lies in this round
            sure[at] = False
            n_in = int(((at >= b0) & (at < b1)).sum())
            of = np.bincount(lists[at], minlength=F)
            lo[t] += np.maximum(0, n_in - (at.size - of))
            hi[t] += np.minimum(n_in, of)
        both = np.bincount(lists[sure], minlength=F)
        lo[t] += both
        hi[t] += both
    return lo, hi


def np_count(data, idx, k, forward=False, soft=False):
    """Per record the sorted (keys, counts) of the valid windows, by numpy: MSB-first
    2-bit keys, the smaller of a window and its reverse complement unless forward."""
    d = np.asarray(data, dtype=np.uint8).copy()
    if soft:
        low = (d >= ord("a")) & (d <= ord("z"))
        d[low] -= 32
    code = np.full(d.size, 4, dtype=np.uint64)
    for c, b in enumerate(b"ACGT"):
        code[d == b] = c
    badc = np.concatenate([[0], np.cumsum(code == 4)])
    out = []
    for r in range(len(idx) - 1):
        a, e = int(idx[r]), int(idx[r + 1])
        nw = e - a - k
        if nw <= 0:
            out.append((np.zeros(0, np.uint64), np.zeros(0, np.int64)))
            continue
        s = np.arange(a, a + nw)
        ok = badc[s + k] == badc[s]
        f = np.zeros(nw, dtype=np.uint64)
        rc = np.zeros(nw, dtype=np.uint64)
        for i in range(k):
            c = code[a + i:a + i + nw] & np.uint64(3)
            f |= c << np.uint64(2 * (k - 1 - i))
            rc |= (np.uint64(3) - c) << np.uint64(2 * i)
        key = f if forward else np.minimum(f, rc)
        out.append(np.unique(key[ok], return_counts=True))
    return out


# ---------------------------------------------------------------------------
# running and comparing
# ---------------------------------------------------------------------------
def run(kmc, cuda, data, idx, k, flags=0, workspace=None):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(data)).to(cuda)
    assert d.data_ptr() % 16 == 0  # the mirrors take the offsets as they are
    di = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(cuda)
    keys, counts, off = kmc.count_canonical(d, di, k, flags=flags, capacity=max(int(data.size), 1),
                                            workspace=workspace)
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32), off.cpu().numpy()


def per_record(keys, counts, off):
    out = []
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        o = np.argsort(keys[a:b], kind="stable")
        out.append((keys[a:b][o], counts[a:b][o]))
    return out


def assert_equal(got, exp, msg, laid=None):
    """got == the oracle's exp: rec_off and every record's sorted set; and == laid
    (np_count's records) where given."""
    np.testing.assert_array_equal(got[2].astype(np.int64), exp[2].astype(np.int64), err_msg=msg + ": rec_off")
    g, e = per_record(*got), per_record(*exp)
    for r, ((gk, gc), (ek, ec)) in enumerate(zip(g, e)):
        np.testing.assert_array_equal(gk, ek, err_msg="%s: record %d keys" % (msg, r))
        np.testing.assert_array_equal(gc, ec, err_msg="%s: record %d counts" % (msg, r))
    if laid is not None:
        assert len(laid) == len(g)
        for r, ((gk, gc), (lk, lc)) in enumerate(zip(g, laid)):
            np.testing.assert_array_equal(gk, lk, err_msg="%s: record %d keys (laid down)" % (msg, r))
            np.testing.assert_array_equal(gc.astype(np.int64), lc, err_msg="%s: record %d counts (laid down)" % (msg, r))


def check(kmc, oracle, cuda, data, idx, k, flags=0, laid=True, msg=""):
    soft, fwd = bool(flags & kmc.CANON_SOFTMASK), bool(flags & kmc.CANON_FORWARD)
    exp = oracle.count_canonical(data, idx, k, soft=soft, forward=fwd)
    got = run(kmc, cuda, data, idx, k, flags)
    assert_equal(got, exp, "%s k=%d flags=%d" % (msg, k, flags),
                 np_count(data, idx, k, forward=fwd, soft=soft) if laid else None)
    return got, exp


@pytest.fixture
def list_target(kmc):
    """kmc_diag_canon_list_target(t): the windows per list canon_plan aims at (16 ..
    4096; 0 restores 4096).  The hook exists only in the diagnostic library, which
    every binding uses inside kmc.diag(); restored afterwards."""
    with kmc.diag() as D:
        yield D.kmc_diag_canon_list_target
        assert D.kmc_diag_canon_list_target(0) == 0


# ---------------------------------------------------------------------------
# building inputs
# ---------------------------------------------------------------------------
def bases(rng, n, p_n=0.0, p_low=0.0):
    s = ACGT[rng.integers(0, 4, size=int(n))]
    if p_low:
        low = rng.random(s.size) < p_low
        s[low] += 32
    if p_n:
        s[rng.random(s.size) < p_n] = N_BYTE
    return s


class Records:
    """Records appended one after another; pos is the next record's start."""

    def __init__(self, rng):
        self.rng, self.parts, self.idx, self.pos = rng, [], [0], 0

    def add(self, seq):
        """One record of these bases (its terminator appended); returns its number."""
        self.parts += [np.asarray(seq, dtype=np.uint8), np.zeros(1, np.uint8)]
        self.pos += len(seq) + 1
        self.idx.append(self.pos)
        return len(self.idx) - 2

    def empty(self):
        """A record of no bytes at all (two equal offsets)."""
        self.idx.append(self.pos)

    def fill_to(self, target, p_n=0.0):
        """A filler record that ends right before byte `target`."""
        assert target > self.pos, (target, self.pos)
        self.add(bases(self.rng, target - self.pos - 1, p_n))

    def done(self):
        return np.concatenate(self.parts), np.array(self.idx, dtype=np.int64)


def keys_for_lists(rng, lists, lg):
    """One 31-mer key per entry of `lists`, all distinct, whose list (top lg bits of
    part) is that entry."""
    lists = np.asarray(lists, dtype=np.uint64)
    out = np.zeros(lists.size, dtype=np.uint64)
    todo = np.arange(lists.size)
    while todo.size:
        low = rng.integers(0, 1 << (64 - lg), size=todo.size, dtype=np.uint64)
        with np.errstate(over="ignore"):
            key = ((lists[todo] << np.uint64(64 - lg)) | low) * np.uint64(MUL_CINV)
        ok = key < np.uint64(1 << (2 * KC))
        out[todo[ok]] = key[ok]
        todo = todo[~ok]
    assert np.unique(out).size == out.size and (list_of(out, lg) == lists.astype(np.int64)).all()
    return out


def kmer_bytes(keys):
    """Each key as its 31 bases and one N: 32 bytes per key, flat."""
    keys = np.asarray(keys, dtype=np.uint64)
    sh = (np.uint64(2) * np.arange(KC - 1, -1, -1, dtype=np.uint64))[None, :]
    out = np.full((keys.size, KC + 1), N_BYTE, dtype=np.uint8)
    out[:, :KC] = ACGT[((keys[:, None] >> sh) & np.uint64(3)).astype(np.int64)]
    return out.reshape(-1)


def lay(sections, lg_windows, lf, tail=0):
    """One record from `sections` (key arrays, or ints: that many bytes of N), padded
    with N to more than 2^lg_windows windows (`tail` more bytes after that), and the
    target that gives it 2^(7 + lf) lists.  Returns data, idx, the keys in input
    order, their window starts, the target."""
    chunks, keys, pos, at = [], [], [], 0
    for s in sections:
        if isinstance(s, (int, np.integer)):
            chunks.append(np.full(int(s), N_BYTE, dtype=np.uint8))
            at += int(s)
        else:
            chunks.append(kmer_bytes(s))
            keys.append(np.asarray(s, dtype=np.uint64))
            pos.append(at + (KC + 1) * np.arange(len(s), dtype=np.int64))
            at += (KC + 1) * len(s)
    need = (1 << lg_windows) + 1 + KC - 1  # bases of a record of 2^lg_windows + 1 windows
    chunks.append(np.full(max(0, need - at) + tail, N_BYTE, dtype=np.uint8))
    data = np.concatenate(chunks + [np.zeros(1, np.uint8)])
    idx = np.array([0, data.size], dtype=np.int64)
    windows = data.size - KC
    assert (1 << lg_windows) < windows <= (2 << lg_windows), windows
    target = 1 << (lg_windows - 6 - lf)
    assert 16 <= target <= 4096
    return data, idx, np.concatenate(keys), np.concatenate(pos), target


def sparse_buckets(rng, lg, skip, per=2):
    """`per` keys for each of the 128 coarse buckets not in `skip`, each in a list of
    its bucket other than the bucket's first (so that fillers in first lists, see
    fillers_for, are the only entries there)."""
    F = 1 << (lg - 7)
    ls = [c * F + int(rng.integers(1, F)) for c in range(128) if c not in skip for _ in range(per)]
    return keys_for_lists(rng, ls, lg)


def fillers_for(rng, lg, others, hot, start):
    """Keys for list 0 that bring the entries of the lists below `hot` (those of
    `others`, plus these) to `start` modulo 16."""
    below = int((list_of(others, lg) < hot).sum())
    return keys_for_lists(rng, [0] * ((start - below) % SEG), lg)


def oracle_list_counts(exp, lg):
    """Entries per list of record 0, from the oracle's forward keys and counts."""
    a, b = int(exp[2][0]), int(exp[2][1])
    return np.bincount(list_of(exp[0][a:b], lg), weights=exp[1][a:b], minlength=1 << lg).astype(np.int64)


def run_laid(kmc, oracle, cuda, list_target, data, idx, keys, target, lg, msg, workspace=None):
    """The constructed record under the hook, forward keys; returns the plan, the
    oracle's per-list counts and the GPU result."""
    P = plan(idx, KC, cu_count(cuda), target)
    assert P.lg[0] == lg and P.k3b == 128, (P.lg, P.k3b)
    assert list_target(target) == 0
    exp = oracle.count_canonical(data, idx, KC, forward=True)
    got = run(kmc, cuda, data, idx, KC, kmc.CANON_FORWARD, workspace=workspace)
    lk, lc = np.unique(keys, return_counts=True)
    assert_equal(got, exp, msg, [(lk, lc)])
    return P, oracle_list_counts(exp, lg), got


# ---------------------------------------------------------------------------
# A. walk edges (K1, K3a, chunk_keys): no hook
# ---------------------------------------------------------------------------
WALK_KS = (1, 2, 15, 16, 17, 31)


def walk_flags(kmc):
    return (0, kmc.CANON_FORWARD, kmc.CANON_SOFTMASK)


@pytest.mark.parametrize("k", WALK_KS)
def test_record_start_and_last_window_at_chunk_offsets_0_1_15(kmc, oracle, cuda, k):
    """lo_m / hi_m of chunk_keys: nine records whose first window starts at chunk
    offset 0, 1 or 15 and whose last window starts at chunk offset 0, 1 or 15 (the
    last window valid: a lowercase run lies in the record's first bases only)."""
    rng = np.random.default_rng(1100 + k)
    R = Records(rng)
    want = []
    for s in (0, 1, 15):
        for e in (0, 1, 15):
            R.fill_to(R.pos + ((s - R.pos - 1) % 16) + 1)
            L = k + 40
            L += (e - (R.pos + L - k)) % 16
            seq = bases(rng, L)
            seq[5:12] += 32  # acgt
            want.append((R.add(seq), s, e))
    data, idx = R.done()
    for r, s, e in want:
        assert idx[r] % 16 == s and (idx[r + 1] - 1 - k) % 16 == e and idx[r + 1] - idx[r] - k > 16
    for flags in walk_flags(kmc):
        check(kmc, oracle, cuda, data, idx, k, flags, msg="chunk offsets")


@pytest.mark.parametrize("k", (1, 2, 3))
def test_four_records_with_all_windows_in_one_chunk(kmc, oracle, cuda, k):
    """Four records of three bases inside one 16-byte chunk (3, 2 or 1 windows each)."""
    rng = np.random.default_rng(1200 + k)
    R = Records(rng)
    R.fill_to(32)
    four = [R.add(bases(rng, 3)) for _ in range(4)]
    R.fill_to(R.pos + 40)
    data, idx = R.done()
    for r in four:
        assert idx[r] >> 4 == 2 and (idx[r + 1] - 1 - k) >> 4 == 2 and idx[r + 1] - idx[r] - k == 4 - k
    for flags in walk_flags(kmc):
        check(kmc, oracle, cuda, data, idx, k, flags, msg="four records in a chunk")


@pytest.mark.parametrize("k", (1, 2, 16, 31))
def test_records_of_k_minus_1_k_and_k_plus_1_bases(kmc, oracle, cuda, k):
    """No window, one window, two windows; at two alignments."""
    rng = np.random.default_rng(1300 + k)
    R = Records(rng)
    short = []
    for lead in (16, 23):
        R.fill_to(R.pos + lead)
        short += [(R.add(bases(rng, L)), L - k + 1) for L in (k - 1, k, k + 1)]
    data, idx = R.done()
    for flags in walk_flags(kmc):
        got, _ = check(kmc, oracle, cuda, data, idx, k, flags, msg="k-1, k, k+1 bases")
        for r, windows in short:
            assert int(got[1][int(got[2][r]):int(got[2][r + 1])].sum()) == windows


@pytest.mark.parametrize("k", (1, 2, 3, 16, 17, 31))
def test_n_as_first_base_last_base_and_one_past_a_window(kmc, oracle, cuda, k):
    """The bad-base smear of chunk_keys (OR of bits j .. j + k - 1 by doubling; k - 1
    a power of two ends it on a step of its own): one N at every chunk offset, 2k + 17
    bases apart, so that for each N the window it ends (invalid), the one before
    that (valid: the N is one past its last base), the one it starts (invalid) and
    the next (valid) are all there; random bases make a lost or an extra window a
    wrong count."""
    rng = np.random.default_rng(1400 + k)
    seq = bases(rng, 40 + 16 * (2 * k + 17) + 40)
    at = 40 + (2 * k + 17) * np.arange(16)
    seq[at] = N_BYTE
    R = Records(rng)
    r = R.add(seq)
    R.add(bases(rng, 50))
    data, idx = R.done()
    assert sorted((idx[r] + at) % 16) == list(range(16))
    valid = seq.size - k + 1 - 16 * k  # each N takes the k windows that hold it
    for flags in (0, kmc.CANON_FORWARD):
        got, _ = check(kmc, oracle, cuda, data, idx, k, flags, msg="N positions")
        assert int(got[1][int(got[2][r]):int(got[2][r + 1])].sum()) == valid


def cuts_input(rng, k, cus):
    """40 KiB whose workgroup cuts (multiples of 16 cpw bytes) fall on: a record's
    first window; its last window; one past its last window; its terminator; its
    k - 1 tail; a run of five empty records; a record without a window; and a record
    with a window at chunk offset 15 right before the cut."""
    T = 40960
    step = 16 * plan([0, T], k, cus).cpw
    stride = -(-400 // step) + 1
    names = ("first", "last", "past_last", "terminator", "tail", "empties", "no_window", "halo")
    R = Records(rng)
    feat = {}
    for j, name in enumerate(names):
        C = (j + 1) * stride * step
        if name == "first":
            R.fill_to(C)
            feat[name] = (R.add(bases(rng, k + 50)), C)
        elif name in ("last", "past_last", "terminator", "tail"):
            R.fill_to(C - 60)
            L = {"last": 60 + k, "past_last": 59 + k, "terminator": 60, "tail": 60 + max(1, (k - 1) // 2)}[name]
            feat[name] = (R.add(bases(rng, L)), C)
        elif name == "empties":
            R.fill_to(C)
            feat[name] = (len(R.idx) - 1, C)
            for _ in range(5):
                R.empty()
            R.add(bases(rng, k + 50))
        elif name == "no_window":
            nb = min(k - 1, 6)
            R.fill_to(C - nb // 2)
            feat[name] = (R.add(bases(rng, nb)), C)
        else:
            R.fill_to(C - 100)
            feat[name] = (R.add(bases(rng, 200 + k)), C)
    R.fill_to(T, p_n=0.01)
    data, idx = R.done()
    return data, idx, feat, step


@pytest.mark.parametrize("k", WALK_KS)
def test_workgroup_cuts_on_record_edges(kmc, oracle, cuda, k):
    """for_each_piece: its binary search (equal offsets included), ps / pe at the
    cuts, pieces of one window, records that lie on a cut without a window."""
    rng = np.random.default_rng(1500 + k)
    data, idx, feat, step = cuts_input(rng, k, cu_count(cuda))
    P = plan(idx, k, cu_count(cuda))
    assert 16 * P.cpw == step and P.c_lo == 0 and idx[-1] == 40960
    cut = lambda name: feat[name][1]
    a = lambda name: int(idx[feat[name][0]])
    e = lambda name: int(idx[feat[name][0] + 1])
    for name in feat:
        assert cut(name) % step == 0 and 0 < cut(name) // step < P.G, name
    assert a("first") == cut("first")
    assert e("last") - 1 - k == cut("last")                   # the last window starts on the cut
    assert e("past_last") - 1 - k == cut("past_last") - 1     # ... right before it
    assert e("terminator") - 1 == cut("terminator")
    if k > 1:  # (k = 1 has no tail: the case equals `terminator` one base on)
        assert e("tail") - k <= cut("tail") < e("tail") - 1
    r0 = feat["empties"][0]
    assert (idx[r0:r0 + 6] == cut("empties")).all() and idx[r0 + 6] > cut("empties")
    assert a("no_window") <= cut("no_window") < e("no_window") and e("no_window") - a("no_window") - k <= 0
    assert a("halo") <= cut("halo") - 1 and cut("halo") - 1 + k < e("halo")  # a window at chunk offset 15
    for flags in (0, kmc.CANON_FORWARD):
        check(kmc, oracle, cuda, data, idx, k, flags, msg="workgroup cuts")


def key_of(seq):
    f = r = 0
    for i, b in enumerate(seq):
        c = b"ACGT".index(b)
        f = (f << 2) | c
        r |= (3 - c) << (2 * i)
    return f, r


def test_extreme_keys_poly_t_poly_a_and_a_palindrome(kmc, oracle, cuda):
    """poly-T at k = 31: forward key 2^62 - 1, canonical key 0; poly-A: 0 both ways;
    ACGT repeated at k = 16: the windows at phases 0 and 2 are their own reverse
    complement (forward key == reverse key), those at 1 and 3 each other's."""
    R = Records(np.random.default_rng(1600))
    n_t, n_a, n_p = 1000, 777, 403
    R.add(np.frombuffer(b"T" * n_t, dtype=np.uint8))
    R.add(np.frombuffer(b"A" * n_a, dtype=np.uint8))
    R.add(np.frombuffer((b"ACGT" * n_p)[:n_p], dtype=np.uint8))
    data, idx = R.done()
    top = (1 << 62) - 1
    got, _ = check(kmc, oracle, cuda, data, idx, 31, kmc.CANON_FORWARD, msg="extreme keys")
    assert list(got[2][:3]) == [0, 1, 2] and list(got[0][:2]) == [top, 0] and list(got[1][:2]) == [n_t - 30, n_a - 30]
    got, _ = check(kmc, oracle, cuda, data, idx, 31, 0, msg="extreme keys")
    assert list(got[0][:2]) == [0, 0] and list(got[1][:2]) == [n_t - 30, n_a - 30]
    phases = [key_of(b"ACGTACGTACGTACGTACGT"[p:p + 16]) for p in range(4)]
    assert phases[0][0] == phases[0][1] and phases[2][0] == phases[2][1] and phases[1][1] == phases[3][0]
    for flags in (0, kmc.CANON_FORWARD):
        got, _ = check(kmc, oracle, cuda, data, idx, 16, flags, msg="palindrome")
        pk, pc = per_record(*got)[2]
        want = set(f for f, _ in phases) if flags else set(min(f, r) for f, r in phases)
        assert list(pk) == sorted(want) and len(want) == (4 if flags else 3) and int(pc.sum()) == n_p - 15


def test_k3a_pieces_of_1024_and_1025_chunks(kmc, oracle, cuda):
    """K3a takes 1024 chunks per round and flips between its two count buffers: with
    1026 chunks per workgroup (16 416 bytes for every CU) the call holds pieces of
    exactly 1024 chunks (one round; one aligned, one starting mid-chunk), of 1025 (a
    second round of one window) and of 1026."""
    k = 21
    cus = cu_count(cuda)
    assert cus >= 8
    cpw = 1026
    wlo = lambda w: 16 * cpw * w
    rng = np.random.default_rng(1700)
    R = Records(rng)
    R.fill_to(wlo(1) - 100, p_n=0.01)
    r1 = R.add(bases(rng, wlo(1) + 16 * 1024 + k - 1 - R.pos))       # windows up to wlo + 16 383
    R.fill_to(wlo(3) - 100, p_n=0.01)
    r2 = R.add(bases(rng, wlo(3) + 16 * 1024 + 1 + k - 1 - R.pos))   # ... up to wlo + 16 384
    R.fill_to(wlo(5) + 24, p_n=0.01)
    r3 = R.add(bases(rng, 16 * 1024 - 8 + k - 1))                    # windows wlo + 24 .. wlo + 16 399
    R.fill_to(wlo(cus), p_n=0.01)
    data, idx = R.done()
    P = plan(idx, k, cus)
    assert P.cpw == cpw and P.G == cus
    by = {(w, r): piece_chunks(ps, pe) for w, r, ps, pe in pieces(idx, k, P)}
    assert by[(1, r1)] == 1024 and by[(3, r2)] == 1025 and by[(5, r3)] == 1024 and idx[r3] % 16 == 8
    assert max(by.values()) == 1026
    check(kmc, oracle, cuda, data, idx, k, 0, laid=False, msg="K3a rounds")


# ---------------------------------------------------------------------------
# B. K3b geometry and the scan
# ---------------------------------------------------------------------------
GEOMETRY_K = {1: 31, 2: 15, 3: 21, 4: 16, 5: 31, 6: 13, 7: 25, 8: 31}


def random_big_record(rng, windows, k):
    """A 300-base record, one of `windows` windows (2 % N, 4 % lowercase), a 300-base one."""
    R = Records(rng)
    R.add(bases(rng, 300, 0.02, 0.04))
    r = R.add(bases(rng, windows + k - 1, 0.02, 0.04))
    R.add(bases(rng, 300, 0.02, 0.04))
    data, idx = R.done()
    assert idx[r + 1] - idx[r] - k == windows
    return data, idx, r


@pytest.mark.parametrize("lf", range(1, 9))
def test_every_ring_geometry_vs_oracle(kmc, oracle, cuda, list_target, lf):
    """lf = 1 .. 8 lists bits per coarse bucket (1024 >> lf owner threads and
    2^(14 - lf) ring entries per list): at 64 windows per list, a random record of the
    fewest windows that has that lf, plus one.  lf = 8 (2^15 lists) also takes both
    scans past one block of tile sums (M > 4096 x 1024: the carry loop of
    scan_blocks_kernel)."""
    k = GEOMETRY_K[lf]
    data, idx, r = random_big_record(np.random.default_rng(2000 + lf), 64 * (1 << (6 + lf)) + 1 + 1, k)
    P = plan(idx, k, cu_count(cuda), 64)
    assert P.lg[r] == 7 + lf and P.k3b == 128 and P.lg[0] == P.lg[2] == 3
    assert plan([0, 64 * (1 << (6 + lf)) + k], k, 1, 64).lg[0] == 6 + lf  # one window fewer than the fewest
    if lf == 8:
        assert P.M > 4096 * 1024, P.M
    assert list_target(64) == 0
    for flags in (0, kmc.CANON_SOFTMASK):
        check(kmc, oracle, cuda, data, idx, k, flags, laid=False, msg="lf=%d" % lf)


def test_shipped_target_smallest_record_with_k3b(kmc, oracle, cuda):
    """The shipped library and its 4096 windows per list: 524 289 windows is the
    smallest record that K3b takes (lg = 8, lf = 1); one window fewer has lg = 7."""
    k = 31
    data, idx, r = random_big_record(np.random.default_rng(2100), 524_289, k)
    P = plan(idx, k, cu_count(cuda))
    assert P.lg[r] == 8 and P.k3b == 128
    assert plan([0, 524_288 + k], k, cu_count(cuda)).k3b == 0
    check(kmc, oracle, cuda, data, idx, k, kmc.CANON_SOFTMASK, laid=False, msg="shipped target")


def test_empty_and_skewed_coarse_buckets(kmc, oracle, cuda, list_target):
    """ACG repeated: three keys, each 100 000 times; at most three of the record's 128
    K3b workgroups have any entry (a0 == a1 in the others), and theirs all go to one
    list of 64 (every round overflows its ring)."""
    k = 31
    R = Records(np.random.default_rng(2200))
    r = R.add(np.frombuffer(b"ACG" * 100_010, dtype=np.uint8)[:300_000 + k - 1])
    data, idx = R.done()
    P = plan(idx, k, cu_count(cuda), 64)
    assert P.lg[r] == 13 and P.k3b == 128
    assert list_target(64) == 0
    got, exp = check(kmc, oracle, cuda, data, idx, k, 0, laid=False, msg="ACG repeat")
    assert exp[0].size == 3 and (exp[1] == 100_000).all()
    assert np.unique(bucket_of(exp[0])).size <= 3


# ---------------------------------------------------------------------------
# C. K3b rounds and ring overflow: controlled occupancy
# ---------------------------------------------------------------------------
HOT_BUCKET, EMPTY_BUCKET = 77, 100


@pytest.mark.parametrize("lf", (3, 8))
@pytest.mark.parametrize("total", (8191, 8192, 8193, 16384, 16385))
def test_bucket_of_exactly_n_entries_round_edges(kmc, oracle, cuda, list_target, total, lf):
    """K3b's round loop (two register sets that swap, left at i0 + 8192 >= a1): one
    coarse bucket of exactly 8191 .. 16 385 entries, dealt to its lists in turn so
    that no ring overflows; the other buckets hold two entries each, one none."""
    lg, F, R = 7 + lf, 1 << lf, 1 << (14 - lf)
    rng = np.random.default_rng(3000 + total + lf)
    first = HOT_BUCKET * F
    body = keys_for_lists(rng, first + np.arange(total) % F, lg)
    others = sparse_buckets(rng, lg, (HOT_BUCKET, EMPTY_BUCKET))
    data, idx, keys, pos, target = lay([others[:100], body, others[100:]], 19, lf)
    P, per_list, _ = run_laid(kmc, oracle, cuda, list_target, data, idx, keys, target, lg,
                              "bucket of %d, lf=%d" % (total, lf))
    per_bucket = per_list.reshape(128, F).sum(axis=1)
    assert per_bucket[HOT_BUCKET] == total and per_bucket[EMPTY_BUCKET] == 0
    assert (np.delete(per_bucket, (HOT_BUCKET, EMPTY_BUCKET)) == 2).all()
    mine = bucket_of(keys) == HOT_BUCKET
    _, hi = k3b_fill_bounds(list_of(keys[mine], lg), k3a_groups(pos[mine], 0, P), first, F)
    assert hi.shape[0] == -(-total // K3B_ROUND) and hi.max() + SEG - 1 <= R  # no overflow in any round


def overflow_input(rng, lf, hot_n, start, lg_windows, second_n=0, one_key=False, tail=0):
    """Bucket HOT_BUCKET: hot_n entries of the hot list, GROUP_PAD bytes of N, (second_n
    entries of the list before the hot one,) then four distinct keys for each
    other list of the bucket in turn.  The other buckets hold two entries each, one
    none, and list 0 what brings the hot list's start (the second list's, if any)
    to `start` modulo 16."""
    lg, F = 7 + lf, 1 << lf
    first = HOT_BUCKET * F
    hot = first + F // 2
    quiet = [hot, hot - 1] if second_n else [hot]
    hot_keys = keys_for_lists(rng, [hot] * (1 if one_key else hot_n), lg)
    if one_key:
        hot_keys = np.repeat(hot_keys, hot_n)
    second = keys_for_lists(rng, [hot - 1] * second_n, lg)
    rest = [l for l in range(first, first + F) if l not in quiet]
    spread = keys_for_lists(rng, np.tile(rest, 4), lg)
    others = sparse_buckets(rng, lg, (HOT_BUCKET, EMPTY_BUCKET))
    fill = fillers_for(rng, lg, np.concatenate([others, spread]), quiet[-1], start)
    data, idx, keys, pos, target = lay([others, fill, hot_keys, GROUP_PAD, second, spread], lg_windows, lf, tail)
    return data, idx, keys, pos, target, hot


def check_overflow_case(P, per_list, keys, pos, lf, hot, hot_n, start, second_n=0):
    """From the oracle's per-list counts and the mirrors: the hot list's length and
    start modulo 16, and exactly which of its entries each K3b round takes."""
    lg, F = 7 + lf, 1 << lf
    first = HOT_BUCKET * F
    starts = np.concatenate([[0], np.cumsum(per_list)])
    assert per_list[hot] == hot_n and starts[hot] % SEG == (start + second_n) % SEG
    if second_n:
        assert per_list[hot - 1] == second_n and starts[hot - 1] % SEG == start
    assert per_list.reshape(128, F).sum(axis=1)[EMPTY_BUCKET] == 0
    mine = bucket_of(keys) == HOT_BUCKET
    lo, hi = k3b_fill_bounds(list_of(keys[mine], lg), k3a_groups(pos[mine], 0, P), first, F)
    np.testing.assert_array_equal(lo[:, hot - first], hi[:, hot - first])  # the hot list's share of every round
    return lo[:, hot - first]


@pytest.mark.parametrize("start", (0, 1, 15))
@pytest.mark.parametrize("delta", (-16, -15, -1, 0, 1, "round"))
@pytest.mark.parametrize("lf", (2, 6))
def test_ring_fill_at_the_overflow_threshold(kmc, oracle, cuda, list_target, lf, delta, start):
    """Ring8::add's cold path (lo >= R), flush's V = F1 and finish's max(H, V): the
    first R - 16, R - 15, R - 1, R, R + 1 or 8192 entries of a bucket all go to one list
    (distinct keys: a stale ring entry written in place of one is a wrong key), which
    starts at offset 0, 1 or 15 of a 16-entry segment: its ring overflows when offset +
    entries > R.  R = 4096 (lf = 2) and 256 (lf = 6)."""
    R = 1 << (14 - lf)
    hot_n = K3B_ROUND if delta == "round" else R + delta
    rng = np.random.default_rng(4000 + 100 * lf + 10 * start + (99 if delta == "round" else delta))
    data, idx, keys, pos, target, hot = overflow_input(rng, lf, hot_n, start, 18)
    P, per_list, _ = run_laid(kmc, oracle, cuda, list_target, data, idx, keys, target, 7 + lf,
                              "lf=%d entries=%d start=%d" % (lf, hot_n, start))
    share = check_overflow_case(P, per_list, keys, pos, lf, hot, hot_n, start)
    assert share[0] == hot_n and share[1:].sum() == 0
    print("lf=%d R=%d entries=%d start=%d: overflow %s" % (lf, R, hot_n, start, start + hot_n > R))


@pytest.mark.parametrize("start", (0, 1))
def test_full_round_into_one_list_overflows_by_f0_alone(kmc, oracle, cuda, list_target, start):
    """lf = 1, R = 8192 = one round: a round that goes entirely to one list fits its ring
    when the list starts a segment, and overflows by one entry when it starts at
    offset 1."""
    lf = 1
    rng = np.random.default_rng(4500 + start)
    data, idx, keys, pos, target, hot = overflow_input(rng, lf, K3B_ROUND, start, 18)
    P, per_list, _ = run_laid(kmc, oracle, cuda, list_target, data, idx, keys, target, 7 + lf, "f0 alone, start=%d" % start)
    share = check_overflow_case(P, per_list, keys, pos, lf, hot, K3B_ROUND, start)
    assert share[0] == K3B_ROUND == 1 << (14 - lf)


@pytest.mark.parametrize("one_key", (True, False))
def test_two_rounds_into_one_list_after_an_overflow(kmc, oracle, cuda, list_target, one_key):
    """20 000 entries into one list of a bucket (one key 20 000 times; and 20 000
    distinct keys, so that an entry written from a stale ring shows), then 17 into the
    list before it (a whole segment and one: it starts a segment, so the hot list
    starts at offset 1): two rounds of 8192 that overflow (R = 4096), each leaving F
    at offset 1 of a segment that lies partly below V, then 3616 more that fit, then
    a last segment of one entry."""
    lf, hot_n = 2, 20_000
    rng = np.random.default_rng(4600 + one_key)
    data, idx, keys, pos, target, hot = overflow_input(rng, lf, hot_n, 0, 19, second_n=17, one_key=one_key)
    P, per_list, _ = run_laid(kmc, oracle, cuda, list_target, data, idx, keys, target, 7 + lf, "two rounds, one_key=%s" % one_key)
    share = check_overflow_case(P, per_list, keys, pos, lf, hot, hot_n, 0, second_n=17)
    assert list(share[:3]) == [K3B_ROUND, K3B_ROUND, hot_n - 2 * K3B_ROUND] and share[3:].sum() == 0
    assert share[2] + SEG - 1 <= 1 << (14 - lf)
    assert (1 + K3B_ROUND) % SEG == 1 and (1 + hot_n) % SEG == 1  # F after each overflow, and at the end


def test_exact_size_caller_workspace_under_the_hook(kmc, oracle, cuda, list_target):
    """The size query follows the hook: a caller workspace of exactly that many bytes,
    filled with 0xFF, gives the library workspace's result (an overflow case, lf = 6),
    and one byte fewer is refused (KMC_ERR_WORKSPACE).  The query covers every
    alignment of the data pointer; the record's N tail is chosen so that the aligned
    call's plan is the largest of the sixteen."""
    import torch
    lf, hot_n, start = 6, (1 << 8) + 1, 15
    cus = cu_count(cuda)
    sizes = lambda Q: (Q.M, Q.Mc, Q.L, Q.windows, Q.k3b)
    for tail in range(64):
        data, idx, keys, pos, target, hot = overflow_input(np.random.default_rng(4700), lf, hot_n, start, 18, tail=tail)
        mine = sizes(plan(idx, KC, cus, target))
        if all(all(a >= b for a, b in zip(mine, sizes(plan(idx + mis, KC, cus, target)))) for mis in range(1, 16)):
            break
    else:
        pytest.fail("no tail for which the aligned plan is the largest")
    P, per_list, got = run_laid(kmc, oracle, cuda, list_target, data, idx, keys, target, 7 + lf, "library workspace")
    check_overflow_case(P, per_list, keys, pos, lf, hot, hot_n, start)
    wsb = kmc.canonical_workspace_size(idx, KC, torch.cuda.current_device())
    assert list_target(0) == 0
    shipped = kmc.canonical_workspace_size(idx, KC, torch.cuda.current_device())
    assert list_target(target) == 0
    assert wsb > shipped > 0  # 2^13 lists against 2^7
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=cuda)
    _, _, again = run_laid(kmc, oracle, cuda, list_target, data, idx, keys, target, 7 + lf, "caller workspace", workspace=ws)
    for g, a in zip(per_record(*got), per_record(*again)):
        np.testing.assert_array_equal(g[0], a[0])
        np.testing.assert_array_equal(g[1], a[1])
    with pytest.raises(kmc.KmcError) as ei:
        run(kmc, cuda, data, idx, KC, kmc.CANON_FORWARD, workspace=ws[:wsb - 1])
    assert ei.value.code == 1004


def test_list_target_hook_arguments(list_target):
    """16 .. 4096 and 0 are taken, everything else is KMC_ERR_INVALID_ARG."""
    for t in (16, 64, 1000, 4096, 0):
        assert list_target(t) == 0
    for t in (1, 15, 4097, 1 << 20):
        assert list_target(t) == 1001
