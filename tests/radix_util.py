"""Host mirrors of the radix path (csrc/kmc_radix.hip, k = 9..13) and an input builder
that puts chosen numbers of windows of chosen buckets into chosen R3 rounds.

Mirrors (numpy only, checked against a brute-force recount in test_radix_edges_gpu.py):
  low_bits / nbk / ring   RingGeom per k
  plan                    tile_geom + wg_range + for_each_tile_piece + wave_run
                          (csrc/kmc_stream.h) and G from radix_plan
  round_fill              per (piece, round, bucket): windows ranked in the round and the
                          list position (relative to the piece's 32-aligned base) at
                          which the round starts -> carry = f & 31, ring half = f & 32
  sample_counts / caps    sample_tiles (runs of at most 16 tiles: every tile, without
                          the windows that need lane 63's halo) and radix_cap_kernel
Codes are little-endian: base i of a window at bits 2i, A C G T = 0 1 2 3; the bucket
is code >> LOW, i.e. the window's last bases (and at k = 11 the high bit of base 7).
"""
from collections import namedtuple

import numpy as np

TILE = 1024
TILE_SHIFT = 10
NWAVES = 16          # waves per workgroup of R1/R3: a round is one tile per wave
SEG = 32             # entries per 64-byte list segment
SAMPLE_ALL = 16      # sample_tiles: runs of up to this many tiles are read whole
KS = (9, 10, 11, 12, 13)

_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
BASES = np.frombuffer(b"ACGT", np.uint8)
N = ord("N")


def low_bits(k):
    lim = 16 if k >= 12 else 15
    return min(2 * k - 6, lim)


def nbk(k):
    return 1 << (2 * k - low_bits(k))


def ring(k):
    return 65536 // nbk(k)


Piece = namedtuple("Piece", "w s ps pe tp0 tp1 per")
Plan = namedtuple("Plan", "G T0 T1 tpw wl wh pieces")


def plan(idx, k, cus, nbytes=None, win=None):
    """The pieces of a call over records `idx` on a device of `cus` compute units, in
    the order the kernels visit them (workgroup, then record).  `win`: the counted
    range (default the whole buffer of `nbytes`, default idx[-1])."""
    idx = np.asarray(idx, np.int64)
    n = idx.size - 1
    wl, wh = win if win is not None else (0, int(idx[-1] if nbytes is None else nbytes))
    tiles = ((wh + TILE - 1) >> TILE_SHIFT) - (wl >> TILE_SHIFT) if wh > wl else 0
    G = cus
    if tiles < G:
        G = tiles if tiles > 0 else 1
    T0 = T1 = 0
    tpw = 1
    if wh > wl:
        T0, T1 = wl >> TILE_SHIFT, (wh + TILE - 1) >> TILE_SHIFT
        tpw = (T1 - T0 + G - 1) // G
    pieces = []
    for w in range(G):
        tb = T0 + w * tpw
        te = min(tb + tpw, T1)
        if tb >= te:
            continue
        R0, R1 = max(tb << TILE_SHIFT, wl), min(te << TILE_SHIFT, wh)
        s0 = int(np.clip(np.searchsorted(idx[:n], R0, "right") - 1, 0, max(n - 1, 0)))
        for s in range(s0, n):
            a, e = int(idx[s]), int(idx[s + 1])
            if a >= R1:
                break
            nw = max(e - a - k, 0)
            ps, pe = max(a, wl, R0), min(a + nw, wh, R1)
            if ps >= pe:
                continue
            tp0, tp1 = ps >> TILE_SHIFT, ((pe - 1) >> TILE_SHIFT) + 1
            pieces.append(Piece(w, s, ps, pe, tp0, tp1, (tp1 - tp0 + NWAVES - 1) // NWAVES))
    return Plan(G, T0, T1, tpw, wl, wh, pieces)


def round_of(pc, pos):
    """Round of piece `pc` in which the window at byte `pos` is ranked: wave v streams
    tiles tp0 + v*per .. of the piece, one per round."""
    return ((np.asarray(pos) >> TILE_SHIFT) - pc.tp0) % pc.per


def window_buckets(data, k):
    """(valid, bucket) per window start 0 .. size-k: all k bytes upper-case ACGT; the
    bucket = code >> LOW from the bases that reach into it."""
    data = np.asarray(data, np.uint8)
    c = _CODE[data]
    nwin = max(data.size - k + 1, 0)
    bad = np.concatenate([[0], np.cumsum(c == 255, dtype=np.int64)])
    valid = (bad[k:k + nwin] - bad[:nwin]) == 0
    low = low_bits(k)
    acc = np.zeros(nwin, np.uint32)
    c32 = (c & 3).astype(np.uint32)
    for j in range(low // 2, k):
        acc |= c32[j:j + nwin] << np.uint32(2 * j - 2 * (low // 2))
    return valid, (acc >> np.uint32(low - 2 * (low // 2))).astype(np.int64)


def code_of(kmer):
    """Dense bin of a k-mer given as bytes."""
    return sum(int(_CODE[b]) << (2 * i) for i, b in enumerate(kmer))


def kmer_of(code, k):
    return bytes(BASES[(code >> (2 * i)) & 3] for i in range(k))


RoundFill = namedtuple("RoundFill", "cnt fstart tot F")


def _piece_counts(data, k, pl, tile_filter=None):
    """cnt[piece, round, bucket] of valid windows; tile_filter(pos) -> bool mask."""
    nb = nbk(k)
    valid, bucket = window_buckets(data, k)
    R = max([pc.per for pc in pl.pieces] + [1])
    cnt = np.zeros((len(pl.pieces), R, nb), np.int64)
    for i, pc in enumerate(pl.pieces):
        pos = np.arange(pc.ps, pc.pe)
        m = valid[pc.ps:pc.pe].copy()
        if tile_filter is not None:
            m &= tile_filter(pos)
        pos = pos[m]
        key = round_of(pc, pos) * nb + bucket[pos]
        cnt[i, :pc.per] = np.bincount(key, minlength=pc.per * nb).reshape(pc.per, nb)
    return cnt


def list_offsets(tot, pl, nb):
    """Exact-mode start of every (piece, bucket) segment in the entry array: the
    exclusive prefix sum of the counts in (record, bucket, workgroup) order."""
    F = np.zeros_like(tot)
    order = sorted(range(len(pl.pieces)), key=lambda i: (pl.pieces[i].s, pl.pieces[i].w))
    base = 0
    i = 0
    while i < len(order):
        j = i
        while j < len(order) and pl.pieces[order[j]].s == pl.pieces[order[i]].s:
            j += 1
        grp = order[i:j]
        flat = tot[grp].T.reshape(-1)  # (bucket, workgroup)
        ex = base + np.concatenate([[0], np.cumsum(flat)[:-1]])
        F[grp] = ex.reshape(nb, len(grp)).T
        base += int(flat.sum())
        i = j
    return F


def round_fill(data, idx, k, pl, sampled=False):
    """cnt[p, r, b]: valid windows of bucket b ranked in round r of piece p;
    fstart[p, r, b]: the list index, relative to the piece's 32-aligned base P0, of the
    round's first entry (so carry = fstart & 31, ring half = fstart & 32, and the fill
    the flush sees = carry + cnt).  Exact mode: the piece starts at the exact offset
    of all earlier lists and earlier workgroups of its list; sampled mode: regions are
    32-aligned, so every piece starts at 0."""
    nb = nbk(k)
    cnt = _piece_counts(data, k, pl)
    tot = cnt.sum(axis=1)
    F = np.zeros_like(tot) if sampled else list_offsets(tot, pl, nb)
    fstart = (F & 31)[:, None, :] + np.cumsum(cnt, axis=1) - cnt
    return RoundFill(cnt, fstart, tot, F)


def as_sampled(rf):
    """The same counts with every piece starting 32-aligned (sampled regions)."""
    return RoundFill(rf.cnt, np.cumsum(rf.cnt, axis=1) - rf.cnt, rf.tot, np.zeros_like(rf.F))


def carry(rf):
    return rf.fstart & 31


def fill(rf):
    return (rf.fstart & 31) + rf.cnt


def sample_counts(data, k, pl):
    """radix_count_kernel<SAMPLE> for pieces whose wave runs are at most SAMPLE_ALL
    tiles: every tile with weight 1, but lane 63 has no halo, so windows that start
    in the last k - 1 bytes of a tile are skipped."""
    assert all(pc.per <= SAMPLE_ALL for pc in pl.pieces), "strided sampling is not mirrored"
    return _piece_counts(data, k, pl, lambda pos: (pos & (TILE - 1)) < TILE + 1 - k).sum(axis=1)


def caps(data, k, pl, scale):
    """radix_cap_kernel: (capacity, x) per (piece, bucket), x the float32 value before
    it is rounded up to 32 entries (and clamped to the piece's windows)."""
    c = sample_counts(data, k, pl).astype(np.float32)
    f32 = np.float32
    x = (f32(1.05) * c + f32(6.0) * np.sqrt(f32(16.0) * c) + f32(64.0)) * f32(scale)
    pmax = np.array([(pc.pe - pc.ps + 31) & ~31 for pc in pl.pieces], np.int64)[:, None]
    cap = np.where(x >= pmax.astype(np.float32), pmax, (x.astype(np.int64) + 31) & ~31)
    return cap, x


def ring_swz(b):
    """Slot swizzle of bucket b: shared by b and b ^ 1."""
    return ((b >> 1) & 7) * 8


def ent_cap(pl, k, n):
    """radix_plan: entries the entry array holds in sampled mode (n records)."""
    win = float(pl.wh - pl.wl)
    regions = (pl.G + float(n)) * nbk(k)
    return int(1.05 * win + 95.0 * regions + 6.0 * (16.0 * win * regions) ** 0.5 + 64.0)


def ovf_cap(pl):
    return int(min(max(4096.0, (pl.wh - pl.wl) / 32.0 / pl.G), 1 << 30))


def brute_round_fill(data, idx, k, pl):
    """The same as round_fill(...).cnt and .F, and the windows per (piece, bucket)
    that reach past their tile, window by window in plain Python (small inputs only)."""
    nb, low = nbk(k), low_bits(k)
    raw = bytes(np.asarray(data, np.uint8))
    R = max([pc.per for pc in pl.pieces] + [1])
    cnt = np.zeros((len(pl.pieces), R, nb), np.int64)
    nohalo = np.zeros((len(pl.pieces), nb), np.int64)  # windows the sampled walk skips
    for i, pc in enumerate(pl.pieces):
        for v in range(NWAVES):
            a0 = pc.tp0 + v * pc.per
            for r, t in enumerate(range(a0, min(a0 + pc.per, pc.tp1))):
                for pos in range(max(t * TILE, pc.ps), min((t + 1) * TILE, pc.pe)):
                    w = raw[pos:pos + k]
                    if len(w) == k and all(ch in b"ACGT" for ch in w):
                        cnt[i, r, code_of(w) >> low] += 1
                        if pos % TILE + k > TILE:
                            nohalo[i, code_of(w) >> low] += 1
    # offsets: lists in (record, bucket) order, workgroups in order inside a list
    F = np.zeros((len(pl.pieces), nb), np.int64)
    base = 0
    for s in sorted({pc.s for pc in pl.pieces}):
        for b in range(nb):
            for i, pc in enumerate(pl.pieces):  # (pieces are in workgroup order)
                if pc.s == s:
                    F[i, b] = base
                    base += int(cnt[i, :, b].sum())
    return cnt, F, nohalo


class Builder:
    """One or two records over cus * tpw tiles of background without the planted base
    (`base`, default T: background {A, C, G}; G: background {A, C}), so no stray window
    falls into the planted homopolymer bucket `tb` -- the last bucket for T, one in the
    middle of the rings for G.  A planted tile is first filled with N, so what a
    plant costs in background windows does not depend on how many it plants.
    tpw = 36: the workgroups of R1/R3 are min(CUs, tiles) and a piece's rounds are
    ceil(tiles / 16), so a piece needs 33+ tiles for three rounds (carry, the round
    under test, the round after); 36 gives 12 tiles a round, 9.4 MB on 256 CUs.
      plant_T(piece, round, c)      c windows of bucket tb: runs of the base between N's
      plant_bucket(piece, round, c, b)  c isolated windows N<k bases>N of bucket b
      align(targets)                T windows in reserved fixer pieces so that, in
                                    exact mode, every target piece's segment of the
                                    planted list starts 32-aligned (as it always does in
                                    sampled mode)
    """

    def __init__(self, k, cus, tpw=36, seed=0, cut=None, base=b"T"):
        self.k, self.cus, self.base = k, cus, base
        size = cus * tpw * TILE
        self.rng = np.random.default_rng(seed)
        pool = np.frombuffer(b"ACG" if base == b"T" else b"AC", np.uint8)
        assert base in (b"T", b"G")
        self.data = pool[self.rng.integers(0, pool.size, size)].copy()
        self.data[-1] = 0
        bounds = [0, size]
        if cut is not None:
            self.data[cut - 1] = 0
            bounds = [0, cut, size]
        self.idx = np.array(bounds, np.int64)
        self.plan = plan(self.idx, k, cus, nbytes=size)
        self.used = set()
        self.tb = code_of(base * k) >> low_bits(k)  # the planted homopolymer's bucket
        self.planted = {}     # (piece, round, bucket) -> windows planted
        self.fixers = {}      # target piece -> (fixer piece, tile)

    def piece_index(self, w, s=0):
        return next(i for i, pc in enumerate(self.plan.pieces) if pc.w == w and pc.s == s)

    def free_tiles(self, piece, r):
        pc = self.plan.pieces[piece]
        return [t for t in range(pc.tp0, pc.tp1)
                if (t - pc.tp0) % pc.per == r and t * TILE >= pc.ps and (t + 1) * TILE <= pc.pe
                and t not in self.used]

    def _take(self, piece, r, c, per_tile):
        free = self.free_tiles(piece, r)
        need = -(-c // per_tile)
        nt = min(len(free), max(need, 2 if c >= 2 else 1))
        assert need <= nt, "round %d of piece %d cannot take %d windows" % (r, piece, c)
        out = []
        for q in range(nt):
            t = free[q]
            self.used.add(t)
            self.data[t * TILE:(t + 1) * TILE] = N
            out.append((t, c // nt + (1 if q < c % nt else 0)))
        return out

    def _run(self, t, c):
        o = t * TILE
        if c:
            self.data[o + 1:o + c + self.k] = self.base[0]

    def _singles(self, t, m, b):
        k, low = self.k, low_bits(self.k)
        assert m * (k + 1) <= TILE - 1
        for q in range(m):
            code = (b << low) | int(self.rng.integers(0, 1 << low))
            o = t * TILE + 1 + q * (k + 1)
            self.data[o:o + k] = np.frombuffer(kmer_of(code, k), np.uint8)

    def plant_T(self, piece, r, c):
        if c == 0:
            return
        for t, m in self._take(piece, r, c, TILE - 1 - self.k):
            self._run(t, m)
        key = (piece, r, self.tb)
        self.planted[key] = self.planted.get(key, 0) + c

    def plant_bucket(self, piece, r, c, b):
        if c == 0:
            return
        for t, m in self._take(piece, r, c, (TILE - 1) // (self.k + 1)):
            self._singles(t, m, b)
        key = (piece, r, b)
        self.planted[key] = self.planted.get(key, 0) + c

    def reserve_fixer(self, target, fixer_piece, bucket=None, r=0):
        """A tile of `fixer_piece` that align() fills for `target`: with T windows (the
        fixer must lie before the target in its planted list, or in an earlier record),
        or with isolated windows of a lower `bucket` (a piece of the target's record
        that no other target follows)."""
        t = self.free_tiles(fixer_piece, r)[-1]
        self.used.add(t)
        self.data[t * TILE:(t + 1) * TILE] = N
        self.fixers[target] = (fixer_piece, t, bucket)

    def align(self):
        """Fill the fixers (each with 0..31 windows).  One mirror pass: a fixer adds its
        windows to the start of every later segment of the planted lists, nothing else
        moves (the callers assert the result from a fresh mirror)."""
        rf = round_fill(self.data, self.idx, self.k, self.plan)
        order = sorted(self.fixers, key=lambda i: (self.plan.pieces[i].s, self.plan.pieces[i].w))
        shift = 0
        for tgt in order:
            fp, t, bucket = self.fixers[tgt]
            a = self.plan.pieces[fp]
            y = int(-(rf.F[tgt, self.tb] + shift)) % 32
            if bucket is None:
                self._run(t, y)
                key = (fp, int(round_of(a, t * TILE)), self.tb)
                self.planted[key] = self.planted.get(key, 0) + y
            else:  # (a background bucket: not in `planted`, whose counts are exact)
                self._singles(t, y, bucket)
            shift += y

    def total_T(self, s=0):
        return sum(c for (p, _, b), c in self.planted.items() if b == self.tb and self.plan.pieces[p].s == s)
