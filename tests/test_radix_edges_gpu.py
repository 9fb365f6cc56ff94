"""The radix path (csrc/kmc_radix.hip, k = 9..13) with a bucket placed on each of its
limits: R3's ring fit (fill = RING - 1 .. 2 RING + 1 at carries 0, 1 and 31, overflow
followed by quiet rounds, at a piece's end, either side of a record boundary, beside
its neighbour rings, and past a sampled region's end), R4's 16-bit bins around 65 536
and 131 072, and R5 either side of its 16-record switch.

Every GPU case is kmc.count_dense_ex against oracle.count_dense, bit for bit, counts
and `invalid`, both pre-filled with -1.  No case assumes the path it is named after:
the fills come from the mirrors in radix_util.py, evaluated on the final input for the
device's own workgroup count, and the occurrence counts from the oracle's output.
Part A checks the mirrors and the builder against a brute-force recount without a GPU.
"""
import numpy as np
import pytest

import radix_util as R

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------
# A. mirrors and builder (CPU)
# ---------------------------------------------------------------------------
def test_geometry_table():
    table = {9: (12, 64, 1024), 10: (14, 64, 1024), 11: (15, 128, 512), 12: (16, 256, 256), 13: (16, 1024, 64)}
    for k in R.KS:
        assert (R.low_bits(k), R.nbk(k), R.ring(k)) == table[k]
        assert R.nbk(k) * R.ring(k) == 65536 and R.nbk(k) << R.low_bits(k) == 4 ** k


@pytest.mark.parametrize("cus", [1, 3, 7, 300])
def test_plan_pieces_partition_the_windows(cus):
    """Every window of every record lies in exactly one piece, inside its workgroup's
    tile range; the wave runs of a piece partition its tiles, at most `per` each."""
    k = 11
    lens = [0, 5, 3000, 1, 1024, 1023, 0, 40_000, k, k + 1, 7000]
    idx = np.concatenate([[0], np.cumsum(np.array(lens) + 1)]).astype(np.int64)
    for win in (None, (1500, 41_111)):
        pl = R.plan(idx, k, cus, win=win)
        wl, wh = win or (0, int(idx[-1]))
        assert pl.G == min(cus, ((wh + 1023) >> 10) - (wl >> 10))
        seen = np.zeros(int(idx[-1]), np.int32)
        for pc in pl.pieces:
            seen[pc.ps:pc.pe] += 1
            tb = pl.T0 + pc.w * pl.tpw
            # the workgroup of a window, written out: tiles of the range over G, rounded up
            ntile = ((wh + 1023) >> 10) - (wl >> 10)
            per_wg = -(-ntile // min(cus, ntile))
            for pos in (pc.ps, pc.pe - 1):
                assert pc.w == ((pos >> 10) - (wl >> 10)) // per_wg
            assert tb * 1024 <= pc.ps and pc.pe <= min(tb + pl.tpw, pl.T1) * 1024
            assert idx[pc.s] <= pc.ps and pc.pe <= idx[pc.s + 1] - k
            tiles = [t for v in range(R.NWAVES)
                     for t in range(pc.tp0 + v * pc.per, min(pc.tp0 + (v + 1) * pc.per, pc.tp1))]
            assert tiles == list(range(pc.tp0, pc.tp1))
        exp = np.zeros_like(seen)
        for s, L in enumerate(lens):
            a = int(idx[s])
            lo, hi = max(a, wl), min(a + max(L + 1 - k, 0), wh)
            if hi > lo:
                exp[lo:hi] = 1
        np.testing.assert_array_equal(seen, exp)
        order = [(pc.w, pc.s) for pc in pl.pieces]
        assert order == sorted(order)


def _small_case(k, cus=8):
    """The fill-edge layout on a small device: two records, planted rounds, fixers."""
    ring = R.ring(k)
    b = R.Builder(k, cus, seed=40 + k, cut=(5 * 36 + 17) * 1024 + 500)
    want = []
    # (a T fixer lies between the target before and its own; the lower-bucket one of
    # the second record's first piece anywhere in that record)
    for w, s, cy in ((1, 0, 1), (3, 0, 31), (7, 1, 0)):
        p = b.piece_index(w, s)
        b.reserve_fixer(p, b.piece_index(w - 1, s))
        b.plant_T(p, 0, cy)
        b.plant_T(p, 1, ring + 1 - cy)
        b.plant_T(p, 2, 5)
        want.append((p, 1, ring + 1, cy))
    p = b.piece_index(5, 1)  # the second record's first piece
    b.reserve_fixer(p, b.piece_index(6, 1), bucket=0)
    b.plant_T(p, 0, ring)
    b.plant_bucket(p, 0, 37, b.tb ^ 1)
    b.plant_bucket(p, 1, 70, b.tb - 2)
    want.append((p, 0, ring, 0))
    b.align()
    return b, want


@pytest.mark.parametrize("k", R.KS)
def test_mirrors_and_builder_vs_brute_force(oracle, k):
    b, want = _small_case(k)
    pl = b.plan
    assert len({(pc.w, pc.s) for pc in pl.pieces}) == len(pl.pieces) == 9
    rf = R.round_fill(b.data, b.idx, k, pl)
    cnt, F, nohalo = R.brute_round_fill(b.data, b.idx, k, pl)
    np.testing.assert_array_equal(rf.cnt, cnt)
    np.testing.assert_array_equal(rf.F, F)
    np.testing.assert_array_equal(R.sample_counts(b.data, k, pl), cnt.sum(axis=1) - nohalo)
    # the builder: every planted (piece, round, bucket) holds exactly what was planted,
    # the wanted fills and carries are there in exact and in sampled mode
    for (p, r, bk), c in b.planted.items():
        assert rf.cnt[p, r, bk] == c, (p, r, bk)
    assert rf.cnt[:, :, b.tb].sum() == sum(c for (_, _, bk), c in b.planted.items() if bk == b.tb)
    for view in (rf, R.as_sampled(rf)):
        for p, r, fill, cy in want:
            assert R.fill(view)[p, r, b.tb] == fill and R.carry(view)[p, r, b.tb] == cy
    # the buckets against the oracle's bins: summed over pieces and rounds
    exp, _ = oracle.count_dense(b.data, b.idx, k)
    per_bucket = exp.reshape(R.nbk(k), 1 << R.low_bits(k), 2).sum(axis=1)
    for s in (0, 1):
        mine = sum(rf.tot[i] for i, pc in enumerate(pl.pieces) if pc.s == s)
        np.testing.assert_array_equal(mine, per_bucket[:, s])
    assert exp[R.code_of(b"T" * k), 0] == b.total_T(0) and exp[R.code_of(b"T" * k), 1] == b.total_T(1)


def test_caps_mirror_formula():
    """radix_cap_kernel in float32: 1.05 c + 6 sqrt(16 c) + 64, scaled, up to 32."""
    k = 13
    b = R.Builder(k, 2, seed=1)
    p = b.piece_index(1)
    b.plant_T(p, 1, 4016)
    cap, x = R.caps(b.data, k, b.plan, 1.0)
    assert abs(float(x[p, b.tb]) - (1.05 * 4016 + 24 * 4016 ** 0.5 + 64)) < 0.01
    assert cap[p, b.tb] == (int(x[p, b.tb]) + 31) // 32 * 32
    assert cap[p, 0] % 32 == 0 and cap[p, 0] >= R.round_fill(b.data, b.idx, k, b.plan).tot[p, 0]
    capz, _ = R.caps(b.data, k, b.plan, 100.0)  # never beyond the piece's windows
    pc = b.plan.pieces[p]
    assert capz[p, b.tb] == (pc.pe - pc.ps + 31) // 32 * 32


# ---------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------
@pytest.fixture
def radix_mode(kmc):
    """kmc_diag_radix_mode(mode, cap_scale) of the diagnostic library (see
    test_dense_gpu.py); restored to auto afterwards."""
    with kmc.diag() as D:
        yield D.kmc_diag_radix_mode
        assert D.kmc_diag_radix_mode(0, 1.0) == 0


EXACT, SAMPLED = (1, 1.0), (2, 1.0)


def _cus(cuda):
    import torch
    return torch.cuda.get_device_properties(cuda).multi_processor_count


def dev(x, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


_CASES = {}  # name -> the finished case, made once, never written; the last few only (k = 13: 268 MB each)


def _cached(name, make):
    if name not in _CASES:
        while len(_CASES) >= 2:
            _CASES.pop(next(iter(_CASES)))
        _CASES[name] = make()
    return _CASES[name]


def _expect(oracle, data, idx, k):
    exp, exp_inv = oracle.count_dense(data, idx, k)
    return dict(data=data, idx=idx, k=k, exp=exp, exp_inv=exp_inv)


def _check(kmc, cuda, radix_mode, case, modes, ld=0, off=0):
    """count_dense_ex in every (mode, scale) of `modes` into a matrix pre-filled with
    -1 (columns [off, off + n) of `ld` when ld > 0), compared on the device."""
    import torch
    k, exp, n = case["k"], case["exp"], case["idx"].size - 1
    d, di = dev(case["data"], cuda), dev(case["idx"], cuda)
    exp_d = dev(exp, cuda)
    for mode, scale in modes:
        assert radix_mode(mode, scale) == 0
        big = torch.full((1 << (2 * k), ld or n), -1, dtype=torch.int32, device=cuda)
        inv = torch.full((n,), -1, dtype=torch.int32, device=cuda)
        kmc.count_dense_ex(kmc.dense_args(d, di, k, big.view(-1)[off:], ld=ld, invalid=inv))
        torch.cuda.synchronize()
        got = big[:, off:off + n]
        if not torch.equal(got, exp_d):
            np.testing.assert_array_equal(got.cpu().numpy(), exp, err_msg="mode %d scale %g" % (mode, scale))
        np.testing.assert_array_equal(inv.cpu().numpy(), case["exp_inv"], err_msg="invalid, mode %d" % mode)
        if ld:
            assert bool((big[:, :off] == -1).all()) and bool((big[:, off + n:] == -1).all())
        del big, got


def _finish(b, oracle):
    """Align, then the case with its mirrors (exact and sampled) and the oracle's
    counts; the planted bin of every record is what the builder planted."""
    b.align()
    case = _expect(oracle, b.data, b.idx, b.k)
    rf = R.round_fill(b.data, b.idx, b.k, b.plan)
    case.update(b=b, rf=rf, rs=R.as_sampled(rf))
    for (p, r, bk), c in b.planted.items():
        assert rf.cnt[p, r, bk] == c, "piece %d round %d bucket %d" % (p, r, bk)
    tcode = R.code_of(b.base * b.k)
    for s in range(b.idx.size - 1):
        assert case["exp"][tcode, s] == b.total_T(s) == sum(
            rf.tot[i, b.tb] for i, pc in enumerate(b.plan.pieces) if pc.s == s)
    return case


def _assert_rounds(case, p, counts, views=("rf", "rs")):
    """Piece p's planted bucket receives `counts` in its rounds, starting 32-aligned, in
    exact and in sampled mode; returns the fill of every round."""
    b = case["b"]
    fills = []
    for view in (case[v] for v in views):
        f = 0
        fills = []
        for r, c in enumerate(counts):
            assert view.cnt[p, r, b.tb] == c and view.fstart[p, r, b.tb] == f, (p, r)
            fills.append((f & 31) + c)
            assert R.fill(view)[p, r, b.tb] == fills[-1]
            f += c
    return fills


# ---------------------------------------------------------------------------
# B. R3 ring fit
# ---------------------------------------------------------------------------
FILLS = {"RING-1": (1, -1), "RING": (1, 0), "RING+1": (1, 1), "RING+31": (1, 31), "RING+32": (1, 32),
         "RING+33": (1, 33), "2RING+1": (2, 1)}


def _fill_case(oracle, k, cus, name):
    def make():
        mul, add = FILLS[name]
        fill = mul * R.ring(k) + add
        b = R.Builder(k, cus, seed=100 * k + len(name))
        # the round before brings the carry; at k = 13 also 32 more: the other ring half
        pre = (0, 1, 31) + ((32, 33, 63) if k == 13 else ())
        targets = []
        for i, cy in enumerate(pre):
            p = b.piece_index(2 + 2 * i)
            b.reserve_fixer(p, b.piece_index(1 + 2 * i))
            targets.append((p, cy))
        for p, cy in targets:
            b.plant_T(p, 0, cy)
            b.plant_T(p, 1, fill - (cy & 31))
            b.plant_T(p, 2, 5)
        case = _finish(b, oracle)
        case.update(fill=fill, targets=targets)
        return case
    return _cached(("fill", k, name), make)


@gpu
@pytest.mark.parametrize("name", list(FILLS))
@pytest.mark.parametrize("k", R.KS)
def test_ring_fill_edges(kmc, oracle, cuda, radix_mode, k, name):
    """One bucket's fill in one round = RING - 1 .. RING + 33 and 2 RING + 1, each
    reached with carry 0, 1 and 31 (three workgroups of one input; at k = 13 three more
    with the round's first segment in the other ring half), exact and sampled.  The
    RING + 1 input also at scale 0.25: the gated exact rerun."""
    case = _fill_case(oracle, k, _cus(cuda), name)
    b, fill = case["b"], case["fill"]
    assert fill == {"RING-1": R.ring(k) - 1, "RING": R.ring(k), "RING+1": R.ring(k) + 1, "RING+31": R.ring(k) + 31,
                    "RING+32": R.ring(k) + 32, "RING+33": R.ring(k) + 33, "2RING+1": 2 * R.ring(k) + 1}[name]
    halves = set()
    for p, cy in case["targets"]:
        assert b.plan.pieces[p].per == 3
        fills = _assert_rounds(case, p, [cy, fill - (cy & 31), 5])
        assert fills[1] == fill
        for view in (case["rf"], case["rs"]):
            assert R.carry(view)[p, 1, b.tb] == cy & 31 and view.fstart[p, 1, b.tb] & 32 == cy & 32
        halves.add(cy & 32)
    assert halves == ({0, 32} if k == 13 else {0})
    _check(kmc, cuda, radix_mode, case, [EXACT, SAMPLED] + ([(2, 0.25)] if name == "RING+1" else []))


@gpu
@pytest.mark.parametrize("k", R.KS)
def test_ring_round_sequences(kmc, oracle, cuda, radix_mode, k):
    """Rounds in a row, one workgroup each: an overflow by exactly 1 followed by a round
    of 0, 1 and 33 entries (segment 0 partly before v), two overflowing rounds in a
    row, an overflowing round that is the piece's last, and pieces that end with a
    partial segment of 1 and of 31 entries."""
    ring = R.ring(k)
    seqs = [(ring + 1, 0, 9), (ring + 1, 1, 9), (ring + 1, 33, 9),
            (ring + 1, ring + 7, 3), (40, ring + 1, 2 * ring + 1),
            (5, 9, ring + 1), (0, 0, ring + 33),
            (0, 32, 33), (0, 64, 31), (ring, 1, 0)]

    def make():
        b = R.Builder(k, _cus(cuda), seed=200 + k)
        ps = []
        for i in range(len(seqs)):
            ps.append(b.piece_index(2 + 2 * i))
            b.reserve_fixer(ps[-1], b.piece_index(1 + 2 * i))
        for p, seq in zip(ps, seqs):
            for r, c in enumerate(seq):
                b.plant_T(p, r, c)
        case = _finish(b, oracle)
        case["ps"] = ps
        return case
    case = _cached(("seq", k), make)
    for p, seq in zip(case["ps"], seqs):
        fills = _assert_rounds(case, p, list(seq))
        over = [f > ring for f in fills]
        if seq[0] == ring + 1:
            assert fills[0] == ring + 1 and over[0]
        if seq in ((ring + 1, ring + 7, 3), (40, ring + 1, 2 * ring + 1)):
            assert (over[0] and over[1]) or (over[1] and over[2])
        if seq in ((5, 9, ring + 1), (0, 0, ring + 33)):
            assert over[2] and not over[0] and not over[1]
    assert sum(seqs[7]) % 32 == 1 and sum(seqs[8]) % 32 == 31 and sum(seqs[9]) % 32 == 1
    _check(kmc, cuda, radix_mode, case, [EXACT, SAMPLED])


@gpu
@pytest.mark.parametrize("k", R.KS)
def test_ring_record_boundary_in_a_range(kmc, oracle, cuda, radix_mode, k):
    """A record ends and the next begins in the middle of a tile in the middle of a
    workgroup's range: the bucket filled to exactly RING in the last round before the
    boundary and in the first round after it (finish, then begin, in one workgroup)."""
    ring = R.ring(k)

    def make():
        wc = 4
        b = R.Builder(k, _cus(cuda), seed=300 + k, cut=(wc * 36 + 17) * 1024 + 500)
        pa, pb = b.piece_index(wc, 0), b.piece_index(wc, 1)
        b.reserve_fixer(pa, b.piece_index(wc - 1, 0))
        b.reserve_fixer(pb, b.piece_index(wc + 1, 1), bucket=0)
        la = b.plan.pieces[pa].per - 1
        b.plant_T(pa, la, ring)
        b.plant_T(pb, 0, ring)
        b.plant_T(pb, 1, 3)
        case = _finish(b, oracle)
        case.update(pa=pa, pb=pb, la=la)
        return case
    case = _cached(("cut", k), make)
    b, pa, pb, la = case["b"], case["pa"], case["pb"], case["la"]
    A, B = b.plan.pieces[pa], b.plan.pieces[pb]
    assert A.w == B.w and A.s + 1 == B.s and A.pe < B.ps and A.pe % 1024 and B.ps % 1024
    assert A.tp1 - 1 == B.tp0 and la >= 1 and B.per >= 2
    for view in (case["rf"], case["rs"]):
        assert R.fill(view)[pa, la, b.tb] == ring and R.carry(view)[pa, la, b.tb] == 0
        assert R.fill(view)[pb, 0, b.tb] == ring and R.carry(view)[pb, 0, b.tb] == 0
    _check(kmc, cuda, radix_mode, case, [EXACT, SAMPLED])


@gpu
@pytest.mark.parametrize("k", R.KS)
def test_ring_neighbours(kmc, oracle, cuda, radix_mode, k):
    """A bucket b in the middle of the rings (all-G, background {A, C}) at RING and at
    RING + 1 while b ^ 1 (the same swizzle; b + 1, at k = 11 b - 1), the ring on its
    other side, b + 2 and b - 2 (the ring pairs next to it in LDS, above and below)
    each receive their own pattern in the same rounds: a write into a neighbour's
    ring, in either direction, changes a count."""
    ring = R.ring(k)
    pats = {"^1": (37, 70, 5), "other 1": (3, 40, 0), "+2": (64, 1, 33), "-2": (20, 65, 2)}

    def buckets(tb):
        return {"^1": tb ^ 1, "other 1": 2 * tb - (tb ^ 1), "+2": tb + 2, "-2": tb - 2}

    def make():
        b = R.Builder(k, _cus(cuda), seed=400 + k, base=b"G")
        ps = []
        for i, fill in enumerate((ring, ring + 1)):
            p = b.piece_index(2 + 2 * i)
            b.reserve_fixer(p, b.piece_index(1 + 2 * i))
            ps.append((p, fill))
        for p, fill in ps:
            b.plant_T(p, 1, fill)
            b.plant_T(p, 2, 40)
            for name, bk in buckets(b.tb).items():
                for r, c in enumerate(pats[name]):
                    b.plant_bucket(p, r, c, bk)
        case = _finish(b, oracle)
        case["ps"] = ps
        return case
    case = _cached(("nb", k), make)
    b = case["b"]
    nbs = buckets(b.tb)
    assert sorted(nbs.values()) == [b.tb - 2, b.tb - 1, b.tb + 1, b.tb + 2] and 2 <= b.tb < R.nbk(k) - 2
    assert R.ring_swz(b.tb) == R.ring_swz(nbs["^1"])
    for p, fill in case["ps"]:
        fills = _assert_rounds(case, p, [0, fill, 40])
        assert fills[1] == fill
        for name, bk in nbs.items():
            assert tuple(case["rf"].cnt[p, :, bk]) == pats[name], name
    _check(kmc, cuda, radix_mode, case, [EXACT, SAMPLED])


@gpu
@pytest.mark.parametrize("k", R.KS)
def test_ring_sampled_region_end(kmc, oracle, cuda, radix_mode, k):
    """Sampled mode at a scale below 1, chosen from the capacity mirror so that the
    planted bucket's region (3584 entries; regions start and end on segment edges by
    construction) ends one segment into the last round's flush: that flush stores a
    complete segment inside the region and passes the complete ones after it to the
    overflow list (ovf_seg), and the piece's partial last segment follows entry by
    entry (ovf_put).  Where the round exceeds the ring (k >= 12) the entries beyond it
    take ovf_put from the direct path.  The overflow lists stay far from full, so the
    result comes from the sampled pass, not from the exact rerun."""
    cap_want, total = 3584, 4016
    seq = ((cap_want - 32) // 2, (cap_want - 32) // 2, total - (cap_want - 32))

    def make():
        b = R.Builder(k, _cus(cuda), seed=500 + k)
        p = b.piece_index(2)
        for r, c in enumerate(seq):
            b.plant_T(p, r, c)
        case = _finish(b, oracle)
        _, x1 = R.caps(b.data, k, b.plan, 1.0)
        case.update(p=p, scale=float(np.float32((cap_want - 16) / float(x1[p, b.tb]))))
        return case
    case = _cached(("cap", k), make)
    b, p, scale = case["b"], case["p"], case["scale"]
    assert 0.5 < scale < 0.7
    cap, x = R.caps(b.data, k, b.plan, scale)
    assert cap[p, b.tb] == cap_want and 8 < float(x[p, b.tb]) % 32 < 24  # an ulp moves nothing
    rs = case["rs"]
    _assert_rounds(case, p, list(seq), views=("rs",))
    f2 = int(rs.fstart[p, 2, b.tb])
    assert f2 == cap_want - 32 and f2 % 32 == 0 and seq[2] >= 64 + 16 and (f2 + seq[2]) % 32 == 16
    # the overflow lists: at most half full in every workgroup, by the mirror
    over = np.maximum(rs.tot - cap, 0).sum(axis=1)
    per_wg = np.bincount([pc.w for pc in b.plan.pieces], weights=over, minlength=b.plan.G)
    assert per_wg[b.plan.pieces[p].w] >= total - cap_want
    assert per_wg.max() <= R.ovf_cap(b.plan) // 2
    assert cap.sum() + 32 * cap.size <= R.ent_cap(b.plan, k, 1)  # the regions fit the entry array (an ulp each to spare)
    _check(kmc, cuda, radix_mode, case, [(2, scale)])


# ---------------------------------------------------------------------------
# C. R4 bin wrap (k = 12, 13: two 16-bit bins per LDS word; k = 11: 32-bit bins)
# ---------------------------------------------------------------------------
def _background(rng, n, without):
    pool = np.array([c for c in b"ACGT" if c not in without], np.uint8)
    return pool[rng.integers(0, pool.size, n)]


def _run_of(base, c, k):
    return np.concatenate([[R.N], np.full(c + k - 1, base, np.uint8), [R.N]]).astype(np.uint8)


def _record(parts):
    data = np.concatenate(list(parts) + [np.zeros(1, np.uint8)]).astype(np.uint8)
    return data, np.array([0, data.size], np.int64)


def _bin_half(k, code):
    """hist_add: entry e = the low LOW bits of the code; word e >> 1, high half iff e & 1."""
    e = code & ((1 << R.low_bits(k)) - 1)
    return e >> 1, e & 1


@gpu
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("c", [65_535, 65_536, 65_537, 131_071, 131_072])
@pytest.mark.parametrize("k", [11, 12, 13])
def test_hist_bin_wrap(kmc, oracle, cuda, radix_mode, k, c, half):
    """One k-mer exactly c times in one list, c around the 16-bit wrap and the second
    one, in the low half of its LDS word (poly-A) and in the high half (poly-T); exact
    (hist_recount) and sampled (hist_recount_regions)."""
    base = b"AT"[half]
    rng = np.random.default_rng(k * 1000 + c % 1000 + half)
    data, idx = _record([_background(rng, 20_011, [base]), _run_of(base, c, k), _background(rng, 9_000, [base])])
    code = R.code_of(bytes([base]) * k)
    assert _bin_half(k, code)[1] == half
    case = _expect(oracle, data, idx, k)
    assert case["exp"][code, 0] == c
    _check(kmc, cuda, radix_mode, case, [EXACT, SAMPLED])


@gpu
@pytest.mark.parametrize("k", [11, 12, 13])
def test_hist_both_bins_of_a_word_wrap(kmc, oracle, cuda, radix_mode, k):
    """Two k-mers of one word, 65 536 and 65 537 times, in one list: A..A (a run) and
    CA..A (isolated windows)."""
    rng = np.random.default_rng(77 + k)
    ca = np.frombuffer(b"C" + b"A" * (k - 1) + b"N", np.uint8)
    data, idx = _record([_background(rng, 5_003, b"A"), _run_of(ord("A"), 65_536, k), np.tile(ca, 65_537),
                         _background(rng, 3_000, b"A")])
    c0, c1 = R.code_of(b"A" * k), R.code_of(b"C" + b"A" * (k - 1))
    assert c0 >> R.low_bits(k) == c1 >> R.low_bits(k)  # one list
    assert _bin_half(k, c0) == (0, 0) and _bin_half(k, c1) == (0, 1)
    case = _expect(oracle, data, idx, k)
    assert case["exp"][c0, 0] == 65_536 and case["exp"][c1, 0] == 65_537
    _check(kmc, cuda, radix_mode, case, [EXACT, SAMPLED])


@gpu
@pytest.mark.parametrize("k", [11, 12, 13])
def test_hist_packed_list_beside_recounted_list(kmc, oracle, cuda, radix_mode, k):
    """Two lists of one record: 65 535 (the largest count that keeps the packed result)
    and 65 536 (recounted); both exact."""
    rng = np.random.default_rng(99 + k)
    data, idx = _record([_background(rng, 7_001, b"AT"), _run_of(ord("A"), 65_535, k),
                         _background(rng, 2_000, b"AT"), _run_of(ord("T"), 65_536, k), _background(rng, 1_500, b"AT")])
    ca, ct = R.code_of(b"A" * k), R.code_of(b"T" * k)
    assert ca >> R.low_bits(k) != ct >> R.low_bits(k)
    case = _expect(oracle, data, idx, k)
    assert case["exp"][ca, 0] == 65_535 and case["exp"][ct, 0] == 65_536
    _check(kmc, cuda, radix_mode, case, [EXACT, SAMPLED])


# ---------------------------------------------------------------------------
# D. R5 place: 16-record tiles (ld > n or n <= 16) | contiguous (ld == n > 16)
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("k,n", [(9, n) for n in (1, 15, 16, 17, 32, 33)] + [(12, n) for n in (1, 15, 16, 17)])
def test_place_record_counts(kmc, oracle, cuda, radix_mode, k, n, wide):
    """Record counts either side of R5's switch at 16 | 17 and of a second tile row at
    32 | 33, lengths 0..3000, into a matrix of its own (ld == n) and into columns
    [3, 3 + n) of one with ld = n + 5 whose other columns stay -1.  (k = 12 stops at
    17 records: 32 and 33 are 2.1 and 2.2 GB of output, 10 s in the host oracle alone.)"""
    def make():
        rng = np.random.default_rng(600 + 40 * k + n)
        lens = rng.integers(0, 3001, size=n)
        if n > 1:
            lens[n // 2] = 0
        recs = [np.append(R.BASES[rng.integers(0, 4, int(L))], np.uint8(0)) for L in lens]
        data = np.concatenate(recs)
        data[rng.random(data.size) < 0.002] = R.N
        for i in np.cumsum([r.size for r in recs]) - 1:
            data[i] = 0
        idx = np.concatenate([[0], np.cumsum([r.size for r in recs])]).astype(np.int64)
        return _expect(oracle, data, idx, k)
    case = _cached(("place", k, n), make)
    if wide:
        _check(kmc, cuda, radix_mode, case, [EXACT], ld=n + 5, off=3)
    else:
        _check(kmc, cuda, radix_mode, case, [EXACT])
