"""kmc_pair_distances and minKmeres2_hip at the limits of their contracts
(include/kmc.h): counts with bit 31 set, records whose bins sum to 2^32 - 1
inside one LDS chunk, denominators that round in float, every k from 1 to 13,
both tile instances on both sides of every plan edge, a column block of a wider
matrix, degenerate record lengths, and more than one block of the drop-in.

The expected values never come from the library: S_ij is summed in numpy from
the counts viewed as uint32 and widened to uint64 (`pair_sums`), the distance is
sparse_dist_util.distances_from_sums (float32, the conversions of distance_of);
oracle.pair_distances (C, signed int32 counts) is used where the counts stay far
below 2^31 and the pair count is in the millions.  Floats are compared bit for
bit (NaN == NaN, +0 == -0).

Every dense call here writes into an `out` followed by 64 guard floats and, when
the plan splits the bin axis, uses a caller workspace of exactly the queried size
cut out of a larger tensor: neither may be written outside its own range.  Every
call also checks the size query against the documented plan (`plan`), so the log
shows which (n, k) ran which instance with how many splits.
"""
import numpy as np
import pytest

import sparse_dist_util as U
from test_dist_gpu import dev, same_floats

pytestmark = pytest.mark.gpu

FULL = 2 ** 32 - 1
CHUNK = 32                # codes per LDS chunk of pair_min_kernel
GUARD = 64                # guard floats after `out`, guard bytes around the workspace
GUARD_BITS = 0x7FC5A5A5   # a NaN no arithmetic produces
UNWRITTEN = -777.25       # what `out` holds before the call


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
def pair_sums(ct, signed=False):
    """S_ij in packed-triangle order from ct (n, bins) uint32, one record per row:
    row i against the rows i + 1 ..., the minima widened to 64 bits in the sum.
    `signed`: what a kernel comparing the counts as int32 would add up (int64)."""
    ct = np.ascontiguousarray(ct, dtype=np.uint32)
    n = ct.shape[0]
    if signed:
        ct, wide = ct.view(np.int32), np.int64
    else:
        wide = np.uint64
    out = np.empty(n * (n - 1) // 2, dtype=wide)
    q = 0
    for i in range(n - 1):
        out[q:q + n - 1 - i] = np.minimum(ct[i], ct[i + 1:]).sum(axis=1, dtype=wide)
        q += n - 1 - i
    return out


def lens_to_idx(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64) + 1)]).astype(np.int64)


def tri(i, j, n):
    return n * i - i * (i - 1) // 2 + (j - i) - (i + 1)


def plan(n, k, cus):
    """The plan of kmc_pair_distances as kmc_dist.hip documents it: (tile side,
    splits, split_len).  n <= 16: 16 x 16 tiles, else 64 x 64; enough splits of the
    bin axis for 4 workgroups per CU, at most one per 128 codes; split_len rounded
    up to whole chunks, so the last split may be short."""
    tt = 16 if n <= 16 else 64
    tiles = -(-n // tt)
    tile_pairs = tiles * (tiles + 1) // 2
    nbins = 4 ** k
    want = 4 * cus
    splits = 1 if tile_pairs >= want else -(-want // tile_pairs)
    splits = max(1, min(splits, -(-nbins // (4 * CHUNK))))
    split_len = -(-(-(-nbins // splits)) // CHUNK) * CHUNK
    return tt, -(-nbins // split_len), split_len


def cu_count(cuda):
    import torch
    return torch.cuda.get_device_properties(cuda).multi_processor_count


# ---------------------------------------------------------------------------
# the calls under test
# ---------------------------------------------------------------------------
def device_counts(ct, cuda, ld=0, col0=0, fill=0):
    """(bins, n) int32 device matrix of ct (n, bins) uint32; with `ld`, columns
    col0 .. col0 + n of a (bins, ld) matrix whose other columns hold `fill`."""
    import torch
    ct = np.ascontiguousarray(ct, dtype=np.uint32)
    n, nb = ct.shape
    rows = dev(ct.view(np.int32), cuda)
    if not ld:
        return rows.t().contiguous(), None
    wide = torch.full((nb, ld), int(np.uint32(fill).astype(np.int32)), dtype=torch.int32, device=cuda)
    wide[:, col0:col0 + n] = rows.t()
    return wide[:, col0:], wide


def run_dense(kmc, cuda, ct, idx, k, split=None, ld=0, col0=0, fill=0):
    """kmc_pair_distances on ct (n, bins) with guards behind `out` and around a
    caller workspace of exactly the queried size.  Asserts that the size query
    agrees with `plan` (and with `split` when the case states what it expects)."""
    import torch
    n = ct.shape[0]
    npairs = n * (n - 1) // 2
    need = kmc.pair_distances_workspace_size(n, k, torch.cuda.current_device())
    tt, splits, split_len = plan(n, k, cu_count(cuda))
    print("pair_distances n=%d k=%d: %dx%d tiles, %d split(s) of %d codes, workspace %d B"
          % (n, k, tt, tt, splits, split_len, need))
    assert need == (8 * npairs if splits > 1 else 0), "the size query disagrees with the documented plan"
    if split is not None:
        assert (need > 0) == split, "n=%d k=%d: expected split=%r" % (n, k, split)
    counts, keep = device_counts(ct, cuda, ld, col0, fill)
    di = dev(np.asarray(idx, dtype=np.int64), cuda)
    out = torch.full((npairs + GUARD,), UNWRITTEN, dtype=torch.float32, device=cuda)
    out[npairs:].view(torch.int32).fill_(GUARD_BITS)
    big = ws = None
    if need:
        big = torch.full((need + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=cuda)
        ws = big[GUARD:GUARD + need]
    kmc.pair_distances(counts, di, k, num_seqs=n, ld=ld, out=out, workspace=ws)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[npairs:].view(np.uint32) == GUARD_BITS).all(), "written behind the packed triangle"
    if big is not None:
        edge = torch.cat([big[:GUARD], big[GUARD + need:]]).cpu().numpy()
        assert (edge == 0xFF).all(), "written outside the caller workspace"
    if keep is not None:
        others = torch.cat([keep[:, :col0], keep[:, col0 + n:]], dim=1).cpu().numpy()
        assert (others.view(np.uint32) == np.uint32(fill)).all(), "the neighbouring columns changed"
    del counts, keep, out, big, ws
    return host[:npairs]


def run_sparse(kmc, cuda, ct, idx, k, diag):
    """kmc_pair_distances_sparse on the non-zero bins of ct (key = bin index)."""
    import contextlib
    import torch
    keys, counts, off = U.lists_from_dense(np.random.default_rng(17), np.ascontiguousarray(ct, np.uint32).T)
    with (kmc.diag() if diag else contextlib.nullcontext()):
        out = kmc.pair_distances_sparse(dev(keys.view(np.int64), cuda), dev(counts.view(np.int32), cuda),
                                        dev(off.view(np.int64), cuda), dev(np.asarray(idx, np.int64), cuda), k)
        torch.cuda.synchronize()
    return out.cpu().numpy()


def random_ct(rng, n, k):
    """Random counts whose every record sums to less than 2^32 (the contract):
    values below min(2^20, 2^32 / bins), a third of the bins empty, and in every
    third record the rest quartered to make room for one bin with bit 31 set."""
    nb = 4 ** k
    scale = min(1 << 20, FULL // nb)
    ct = rng.integers(0, scale, size=(n, nb), dtype=np.int64)
    ct[rng.random((n, nb)) < 0.33] = 0
    ct[::3] >>= 2
    hot = rng.integers(0, nb, size=n)
    ct[np.arange(n)[::3], hot[::3]] = 0x80000000 + rng.integers(0, 1 << 10, size=len(hot[::3]))
    assert ct.sum(axis=1).max() <= FULL
    lens = ct.sum(axis=1) + k - 1 + rng.integers(0, 50, size=n)
    return ct.astype(np.uint32), lens


def check_random(kmc, cuda, n, k, split=None, seed=0, **kw):
    rng = np.random.default_rng(100_000 * seed + 100 * n + k)
    ct, lens = random_ct(rng, n, k)
    exp = U.distances_from_sums(pair_sums(ct), lens, k)
    got = run_dense(kmc, cuda, ct, lens_to_idx(lens), k, split=split, **kw)
    same_floats(got, exp, "n=%d k=%d" % (n, k))


# ---------------------------------------------------------------------------
# 1. unsigned counts at the contract limit
# ---------------------------------------------------------------------------
# denominators (min(len) - k + 1) that float32 rounds, or that lie beyond 32 bits
ROUNDING_DENOMS = [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 28 + 9, 2 ** 31 + 129, 2 ** 32 - 1, 2 ** 32 + 50,
                   2 ** 36 + 12345, 2 ** 40]


def limit_case(n, k, pattern):
    """ct (n, bins) uint32 and the record lengths.  Roles (n = 5: one record each;
    n = 70: one in tile row 0 and one in the ragged tile row 1):
      full     one bin of 2^32 - 1 at code y and nothing else
      high     0x80000005 at code y, a few small bins
      seven    7 at code y: the unsigned minimum against `high` and `full` is 7,
               the signed one is the partner's negative value
      twins    identical records whose bins sum to 2^32 - 1 inside one aligned chunk:
               "chunk" = all 32 codes (what one thread of the 64 x 64 instance adds),
               "lane" = the 8 codes r = 3 (mod 4) (one code lane of the 16 x 16 one)
    The other records of n = 70 are random, a third with bit 31 set at code y."""
    nb = 4 ** k
    rng = np.random.default_rng(1000 * n + 10 * k + len(pattern))
    y, c0 = (5, 32) if k == 3 else (1234, 32 * 77)
    codes = c0 + (np.arange(32) if pattern == "chunk" else 3 + 4 * np.arange(8))
    pat = np.full(codes.size, 2 ** 32 // codes.size, dtype=np.int64)
    pat[-1] -= 1
    ct = np.zeros((n, nb), dtype=np.int64)
    den = np.zeros(n, dtype=np.int64)  # the independent denominators; 0: the record's own windows
    if n == 5:
        full, high, seven, twins = [0], [1], [2], [3, 4]
        den[1], den[2] = 2 ** 32 + 50, 2 ** 24 + 1
    else:
        full, high, seven, twins = [0, 64], [1, 66], [2, 67], [3, 4, 68, 69]
        pool = np.unique(np.concatenate([c0 + np.arange(32), [y], rng.integers(0, nb, size=20)]))
        for s in range(n):
            mine = rng.choice(pool, size=12, replace=False)
            ct[s, mine] = rng.integers(1, 1 << 27, size=12)
            if s % 3 == 0:
                ct[s, y] = 0x80000000 + int(rng.integers(0, 1 << 20))
            den[s] = ROUNDING_DENOMS[s % len(ROUNDING_DENOMS)] if s % 4 else 0
    for s in full:
        ct[s] = 0
        ct[s, y] = FULL
        den[s] = 0
    for s in high:
        ct[s] = 0
        ct[s, y] = 0x80000005
        ct[s, c0 + 1], ct[s, c0 + 3] = 1000, 2000
        den[s] = den[s] or 2 ** 32 + 50
    for s in seven:
        ct[s] = 0
        ct[s, y] = 7
        ct[s, c0 + 3], ct[s, c0 + 4] = 1 << 20, 3
        den[s] = den[s] or 2 ** 24 + 1
    for s in twins:
        ct[s] = 0
        ct[s, codes] = pat
        den[s] = 0
    windows = ct.sum(axis=1)
    lens = np.where(den > 0, den, windows) + k - 1
    return ct.astype(np.uint32), lens, windows, twins


@pytest.mark.parametrize("pattern", ["chunk", "lane"])
@pytest.mark.parametrize("k", [3, 6])
@pytest.mark.parametrize("n", [5, 70])
def test_unsigned_counts_at_the_contract_limit(kmc, cuda, n, k, pattern):
    """The contract of kmc_pair_distances: counts are unsigned, and every record's
    bins sum to its windows, at most 2^32 - 1.  Here records reach that sum in one
    bin, in the 32 codes of one chunk and in the 8 codes of one code lane, bins have
    bit 31 set, and denominators lie where float32 rounds (2^24 .. 2^40).  The dense
    result, the sparse result on the non-zero bins (both library builds) and the
    numpy reference are equal bit for bit."""
    ct, lens, windows, twins = limit_case(n, k, pattern)
    assert windows.max() == FULL and (windows <= FULL).all()  # the contract holds, and is reached
    S = pair_sums(ct)
    assert int(S.max()) == FULL
    assert (pair_sums(ct, signed=True) != S.astype(np.int64)).any()  # a signed min would be caught
    exp = U.distances_from_sums(S, lens, k)
    a, b = twins[0], twins[1]
    assert S[tri(a, b, n)] == FULL and lens[a] == lens[b] and exp[tri(a, b, n)] == 0
    idx = lens_to_idx(lens)
    got = run_dense(kmc, cuda, ct, idx, k, split=(k == 6))
    same_floats(got, exp, "dense")
    for diag in (False, True):
        sp = run_sparse(kmc, cuda, ct, idx, k, diag)
        same_floats(sp, exp, "sparse diag=%r" % diag)
        same_floats(sp, got, "sparse against dense, diag=%r" % diag)


@pytest.mark.parametrize("n", [5, 70])
def test_sums_beyond_32_bits_across_chunks(kmc, cuda, n):
    """Beyond the header's promise (records of fewer than 2^32 windows), but what
    the kernel's uint64 totals, the CPU path's `long sum` and the sparse twin all
    deliver, and what test_distances_large_counts_exact already relies on: each
    of the two chunks of k = 3 adds up to 2^32 - 1 in 32 bits, their total
    2^33 - 2 needs 64.  Three records hold it in the codes r = 3 (mod 4), so that
    in both instances it is one thread that meets 2^32 - 1 twice."""
    k, nb = 3, 64
    rng = np.random.default_rng(n)
    ct = rng.integers(0, 1 << 27, size=(n, nb), dtype=np.int64)
    for s in (1, 3, n - 1):
        ct[s] = 0
        ct[s, 3::4] = 1 << 29
        ct[s, [31, 63]] -= 1
    assert ct[:, :32].sum(axis=1).max() == FULL and ct[:, 32:].sum(axis=1).max() == FULL
    ct = ct.astype(np.uint32)
    lens = rng.integers(1 << 33, 1 << 35, size=n)
    S = pair_sums(ct)
    assert int(S.max()) == 2 ** 33 - 2
    exp = U.distances_from_sums(S, lens, k)
    idx = lens_to_idx(lens)
    got = run_dense(kmc, cuda, ct, idx, k, split=False)
    same_floats(got, exp, "dense")
    same_floats(run_sparse(kmc, cuda, ct, idx, k, False), got, "sparse against dense")


# ---------------------------------------------------------------------------
# 2. every k
# ---------------------------------------------------------------------------
def sparse_ct(rng, n, k, split_len):
    """For k >= 9: a few ten thousand hot codes per record, among them the first
    and the last code and the codes on both sides of a split boundary."""
    nb = 4 ** k
    hot = np.concatenate([rng.integers(0, nb, size=50_000), [0, nb - 1, split_len - 1, split_len % nb]])
    ct = np.zeros((n, nb), dtype=np.uint32)
    for s in range(n):
        np.add.at(ct[s], rng.choice(hot, size=80_000), rng.integers(1, 5000, size=80_000).astype(np.uint32))
        ct[s, hot[-4:]] += np.uint32(s + 1)
    lens = ct.sum(axis=1, dtype=np.int64) + k - 1 + rng.integers(0, 50, size=n)
    return ct, lens


@pytest.mark.parametrize("n,k", [(n, k) for k in range(1, 14) for n in (3, 17) if n == 3 or k <= 10])
def test_every_k(kmc, cuda, n, k):
    """k = 1 (4 codes, less than one chunk: only the code guard keeps the rest of
    the chunk zero) to k = 13 (67 M codes), in the 16 x 16 and the 64 x 64 instance."""
    import torch
    rng = np.random.default_rng(50 * k + n)
    tt, splits, split_len = plan(n, k, cu_count(cuda))
    if k <= 8:
        ct, lens = random_ct(rng, n, k)
    else:
        ct, lens = sparse_ct(rng, n, k, split_len)
    S = pair_sums(ct)
    assert k <= 8 or S.min() > 0  # the hot codes overlap
    exp = U.distances_from_sums(S, lens, k)
    got = run_dense(kmc, cuda, ct, lens_to_idx(lens), k, split=k >= 4)
    same_floats(got, exp, "n=%d k=%d" % (n, k))
    del ct
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# 3. plan edges
# ---------------------------------------------------------------------------
def last_split_tiles(kmc, k):
    """The largest T for which n = 64 T still splits at this k, asked of the size query."""
    import torch
    dv = torch.cuda.current_device()
    T = 1
    assert kmc.pair_distances_workspace_size(64, k, dv) > 0
    while kmc.pair_distances_workspace_size(64 * (T + 1), k, dv) > 0:
        T += 1
        assert T < 4096
    return T


@pytest.mark.parametrize("past", [0, 1])
def test_where_the_split_switches_off(kmc, oracle, cuda, past):
    """n = 64 T, the most tile pairs that still split the bin axis (most workgroups
    add into the workspace with atomics, and pair_finish_kernel inverts the largest
    triangle the dense path ever gives it), and n = 64 T + 1, the first unsplit
    launch, whose last tile row holds one record.  Counts below 40, so the C
    oracle's signed counts decide."""
    import torch
    k = 4
    T = last_split_tiles(kmc, k)
    n = 64 * T + past
    need = kmc.pair_distances_workspace_size(n, k, torch.cuda.current_device())
    assert need == (0 if past else 8 * (n * (n - 1) // 2))
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 40, size=(4 ** k, n), dtype=np.int64).astype(np.int32)
    lens = counts.astype(np.int64).sum(axis=0) + k - 1 + rng.integers(0, 50, size=n)
    exp = oracle.pair_distances(counts, lens, k)
    got = run_dense(kmc, cuda, counts.T.view(np.uint32), lens_to_idx(lens), k, split=not past)
    same_floats(got, exp, "n=%d" % n)


GRID_N = [2, 15, 16, 17, 63, 64, 65, 128, 129]
GRID_K = [1, 2, 4, 5, 7]


@pytest.mark.parametrize("k", GRID_K)
@pytest.mark.parametrize("n", GRID_N)
def test_tile_and_split_edges(kmc, cuda, n, k):
    """Both instances on both sides of n = 16, full and ragged 64 x 64 tiles, and
    the bin axis unsplit (k = 1, 2: fewer than 128 codes) and split."""
    check_random(kmc, cuda, n, k, split=k >= 4)  # (the 6 tile pairs of n = 129 fill no chip)


def short_split_cases(cus):
    """(cost, n, k) of plans whose last split is shorter than the others, n = one
    record into the last tile row."""
    found = []
    for k in GRID_K:
        for T in range(2, 65):
            n = 64 * (T - 1) + 1
            tt, splits, split_len = plan(n, k, cus)
            if splits > 1 and (4 ** k) % split_len:
                found.append((4 ** k * n * n, n, k))
    return sorted(found)


def test_short_last_split(kmc, cuda):
    """split_len is rounded up to whole chunks, so the splits need not divide the
    bins: the last one is short and `code < c1` ends it.  On 256 CUs no (n, k) of
    test_tile_and_split_edges has such a plan (their splits are capped at one per
    128 codes, which divides 4^k), so the cheapest one is looked up from the plan."""
    cus = cu_count(cuda)
    cases = short_split_cases(cus)
    assert cases, "no plan with a short last split on %d CUs" % cus
    _, n, k = cases[0]
    tt, splits, split_len = plan(n, k, cus)
    assert splits > 1 and (4 ** k) % split_len != 0 and splits * split_len > 4 ** k
    check_random(kmc, cuda, n, k, split=True, seed=1)


# ---------------------------------------------------------------------------
# 4. a column block of a wider matrix, over several tiles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,split", [(6, True), (2, False)])
def test_sum_ld_over_several_tiles(kmc, cuda, k, split):
    """70 records (two tile rows, the last ragged) at column 11 of a 97-column
    matrix whose other columns hold 0xFFFFFFF9."""
    check_random(kmc, cuda, 70, k, split=split, seed=2, ld=97, col0=11, fill=0xFFFFFFF9)


# ---------------------------------------------------------------------------
# 6. degenerate denominators
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bins", ["zero", "nonzero"])
@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("n", [6, 18])
def test_degenerate_denominators(kmc, cuda, n, k, bins):
    """Records of 0, k - 2, k - 1 and k bases and an empty one (len = -1): the
    denominator m - k + 1 is negative, 0, 0, 1 and negative.  The expression is
    total and the reference decides: NaN for 0 / 0, -inf for S / 0, more than 1
    for a negative denominator.  k = 2 is unsplit (the tile kernel divides), k = 5
    split (pair_finish_kernel does)."""
    rng = np.random.default_rng(10 * n + k)
    ct, lens = random_ct(rng, n, k)
    lens[:5] = [0, k - 2, k - 1, k, -1]
    if bins == "zero":
        ct[:5] = 0
    idx = lens_to_idx(lens)
    assert idx[5] == idx[4] and (np.diff(idx) - 1 == lens).all()
    exp = U.distances_from_sums(pair_sums(ct), lens, k)
    if bins == "zero":
        assert np.isnan(exp).any() and (exp[~np.isnan(exp)] == 1).any()
    else:
        assert np.isneginf(exp).any() and (exp > 1).any()
    got = run_dense(kmc, cuda, ct, idx, k, split=(k == 5))
    same_floats(got, exp)
    same_floats(run_sparse(kmc, cuda, ct, idx, k, False), got, "sparse against dense")


# ---------------------------------------------------------------------------
# 7. minKmeres2_hip beyond one block
# ---------------------------------------------------------------------------
_dropin = {}


def dropin_case():
    """600 records of the 64 codes of k = 3: counts of a few thousand behind one bin
    of about 2^24, which lifts the float running sum to where odd counts round."""
    if not _dropin:
        rng = np.random.default_rng(600)
        n = 600
        counts = rng.integers(1000, 6000, size=(64, n), dtype=np.int64)
        counts[0] = (1 << 24) + rng.integers(0, 1000, size=n)
        lens = rng.integers(1000, 3_000_000, size=n)
        idx32 = lens_to_idx(lens)
        assert idx32[-1] < 2 ** 31
        for cur in (0, 342, 343):  # the float running sum rounds for some pair of these rows
            m = np.minimum(counts[:, cur:cur + 1], counts[:, cur + 1:])
            run = np.zeros(n - 1 - cur, dtype=np.float32)
            for t in range(64):
                run += m[t].astype(np.float32)
            assert (run.astype(np.float64) != m.sum(axis=0)).any()
        _dropin.update(n=n, counts=counts.astype(np.int32), idx32=idx32.astype(np.int32))
    return _dropin


@pytest.mark.parametrize("cur", [0, 342, 343, 598, 599])
def test_min_kmeres2_beyond_one_block(kmc, oracle, cuda, cur):
    """599, 257, 256, 1 and 0 later records: three blocks, a second block with one
    record, exactly one full block, one record, and no launch.  Row `cur`
    is the oracle's (float accumulation in code order); nothing else is written."""
    import torch
    c = dropin_case()
    n, counts, idx32 = c["n"], c["counts"], c["idx32"]
    npairs = n * (n - 1) // 2
    exp = np.full(npairs + GUARD, UNWRITTEN, dtype=np.float32)
    oracle.min_kmeres2_row(counts, idx32, cur, 3, exp)
    row = slice(tri(cur, cur + 1, n), tri(cur, cur + 1, n) + n - 1 - cur)
    assert (exp[row] != UNWRITTEN).all() and (np.delete(exp, row) == UNWRITTEN).all()
    sums, ix = dev(counts.reshape(-1), cuda), dev(idx32, cuda)
    launches = [lambda mins: kmc.min_kmeres2(sums, mins, n, cur, ix)]
    if oracle.have_ref_kernel():
        L = oracle.ref_kernel()
        launches.append(lambda mins: L.ref_min_kmeres2_launch(sums.data_ptr(), mins.data_ptr(), n, cur, ix.data_ptr()))
    for launch in launches:
        mins = torch.full((npairs + GUARD,), UNWRITTEN, dtype=torch.float32, device=cuda)
        assert not launch(mins)
        torch.cuda.synchronize()
        got = mins.cpu().numpy()
        same_floats(got[row], exp[row], "row %d" % cur)
        assert (np.delete(got, row) == UNWRITTEN).all(), "written outside row %d" % cur
