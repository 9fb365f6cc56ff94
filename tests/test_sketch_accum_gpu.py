"""GPU parity of the abundance accumulator (kmc_sketch_accum_*, kmc.SketchAccum) against
the CPU.  The expected row of every case comes from the oracle: the hashes of all added
records with their multiplicities (sketch_screen_util.mixture_hashes), those with
count >= m, ascending; the row must be their first `size`, bit for bit, and the four
stats words must say what the header says they do (check()).  j is computed here from
the byte counts and the slot count by the header's formula.  Every case runs in
libkmc.so and in libkmc_diag.so, whose 64-thread walking workgroups and 256-byte
ranges put a few thousand bases through many ranges."""
import numpy as np
import pytest

import sketch_group_util as GU
import sketch_screen_util as U
import sketch_util as S
import stream_util as T
from sketch_screen_util import FWD, SOFT
from sketch_util import bases, dev, pack, which
from test_sketch_accum_args import live_handle_errors

pytestmark = pytest.mark.gpu

LIBS = ["ship", "diag"]
cached = S.cache()
FILL = int(S.FILL)
NSEP = np.full(1, ord("N"), np.uint8)


def level(nbytes, lg):
    """The smallest j >= 0 with ceil(N / 2^j) <= C / 4."""
    j = 0
    while -(-nbytes // (1 << j)) > (1 << lg) // 4:
        j += 1
    return j


def bound(j):
    """The exclusive bound of level j as stats[1] holds it when nothing was lost."""
    return FILL if j == 0 else 1 << (64 - j)


def roomy(nbytes):
    """The smallest log2_slots at which nbytes bytes keep j = 0."""
    lg = 4
    while level(nbytes, lg) > 0:
        lg += 1
    return lg


def add(kmc, cuda, acc, batch, shift=0):
    data, idx = batch
    d, di = U.device_records(cuda, data, idx, shift)
    acc.add(d, di)
    return data.size


def finish(acc, m):
    """(row uint64 [s], size, stats [4] as Python ints) of finish(m)."""
    import torch
    row, size, stats = acc.finish(m)
    torch.cuda.synchronize()
    return (row.cpu().numpy().view(np.uint64), int(size.cpu().numpy().view(np.uint32)[0]),
            [int(x) for x in stats.cpu().numpy().view(np.uint64)])


def check(got, mix, m, s, j, msg, lossless=None):
    """The generic property.  lossless: True / False when the case knows whether an
    insert was refused; None when it does not."""
    row, size, stats = got
    h, c = mix
    q = h[c >= max(m, 1)]
    print("%s: m=%d size=%d stats=%s oracle: %d hashes, %d qualifying, j=%d" % (msg, m, size, stats, h.size, q.size, j))
    complete, limit, tracked, qualifying = stats
    assert complete in (0, 1), msg
    assert limit <= bound(j), "%s: limit above 2^(64 - j)" % msg
    if lossless is True:
        assert limit == bound(j), "%s: something was lost" % msg
    if lossless is False:
        assert limit < bound(j), "%s: nothing was lost" % msg
    everything = j == 0 and limit == FILL
    below = np.ones(h.size, bool) if everything else h < np.uint64(limit)
    assert tracked == int(below.sum()), "%s: tracked" % msg
    assert qualifying == int((below & (c >= max(m, 1))).sum()), "%s: qualifying" % msg
    if complete:
        assert size == min(s, q.size), "%s: a complete row of %d" % (msg, size)
        assert everything or size == s, msg
    else:
        assert size < s and size == qualifying, "%s: an incomplete row of %d" % (msg, size)
    np.testing.assert_array_equal(row[:size], q[:size], err_msg="%s row" % msg)
    assert (row[size:] == S.FILL).all(), "%s: fill" % msg


def mixture(oracle, key, batches, k, flags=0, seed=S.DEFAULT_SEED):
    """mixture_hashes over the concatenation of the batches' records, once per key."""
    def make():
        recs = [d[i[r]:i[r + 1] - 1] for d, i in batches for r in range(i.size - 1)]
        data, idx = pack(recs) if recs else (np.zeros(0, np.uint8), np.zeros(1, np.int64))
        return U.mixture_hashes(oracle, data, idx, k, flags, seed)
    return cached(key, make)


EMPTY = (np.zeros(0, np.uint8), np.zeros(1, np.int64))


# 1. m = 1 equals the grouped sketcher ------------------------------------------------
def records_case():
    """Empty records, records shorter than k, N and lowercase (stream_util.records)."""
    return cached("records", lambda: T.records(77, [0, 5, 900, 3000, 1, 40, 2500, 0, 30, 1200]))


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("flags", [0, SOFT, FWD])
@pytest.mark.parametrize("k", [1, 5, 15, 16, 21, 31])
def test_accum_equals_grouped_sketch(kmc, oracle, cuda, lib, k, flags):
    import torch
    s = 600  # above the 512 canonical 5-mers (and the 4 1-mers): rows shorter than s
    data, idx = records_case()
    lg = roomy(data.size)
    mix = mixture(oracle, ("records-mix", k, flags), [(data, idx)], k, flags)
    exp = GU.grouped_expected(oracle, data, idx, [0, idx.size - 1], k, s, flags)
    with which(kmc, lib):
        for shift in (0, 1, 15):
            d, di = U.device_records(cuda, data, idx, shift)
            grp = dev(np.array([0, idx.size - 1], np.int64), cuda)
            sk, sz = kmc.sketch_from_sequences_grouped(d, di, grp, k, s, flags=flags)
            with kmc.SketchAccum(s, k, flags=flags, log2_slots=lg) as acc:
                acc.add(d, di)
                got = finish(acc, 1)
            torch.cuda.synchronize()
            msg = "k=%d flags=%d shift=%d" % (k, flags, shift)
            grow, gsize = sk.cpu().numpy().view(np.uint64)[0], int(sz.cpu().numpy().view(np.uint32)[0])
            np.testing.assert_array_equal(got[0], grow, err_msg=msg)
            assert got[1] == gsize == int(exp[1][0]), msg
            np.testing.assert_array_equal(got[0], exp[0][0], err_msg=msg)
            assert got[2][0] == 1 and got[2][1] == FILL, msg
            check(got, mix, 1, s, 0, msg, lossless=True)
    if k == 1 or (k == 5 and flags != FWD):
        assert got[1] < s


# 2. min_count ------------------------------------------------------------------------
def planted_case():
    """Segments of 60 bases planted 1 .. 5 times among unrelated bases: keys of every
    multiplicity 1 .. 5, so for m = 2 and m = 3 keys with exactly m - 1, m and m + 1."""
    def make():
        rng = np.random.default_rng(31)
        segs = [(bases(rng, 60), r) for r in (1, 2, 3, 4, 5) for _ in range(6)]
        parts = []
        for seg, r in segs:
            parts += [seg] * r
        parts += [bases(rng, 50) for _ in range(40)]
        order = rng.permutation(len(parts))
        recs, cur = [], []
        for i in order:  # a few parts per record, separated by N
            cur += [parts[i], NSEP]
            if len(cur) >= 10:
                recs.append(np.concatenate(cur))
                cur = []
        recs.append(np.concatenate(cur) if cur else bases(rng, 0))
        return pack(recs)
    return cached("planted", make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("s", [32, 1000])
def test_accum_min_count(kmc, oracle, cuda, lib, s):
    k = 21
    batch = planted_case()
    mix = mixture(oracle, "planted-mix", [batch], k)
    present = set(int(x) for x in np.unique(mix[1]))
    assert {1, 2, 3, 4, 5} <= present
    with which(kmc, lib):
        with kmc.SketchAccum(s, k, log2_slots=roomy(batch[0].size)) as acc:
            add(kmc, cuda, acc, batch)
            got = [finish(acc, m) for m in (1, 2, 3, 4, 0, 6)]
    for m, g in zip((1, 2, 3, 4, 0, 6), got):
        check(g, mix, m, s, 0, "s=%d m=%d" % (s, m), lossless=True)
    assert got[4][1] == got[0][1] and (got[4][0] == got[0][0]).all()  # 0 and 1 both mean every key
    if s == 1000:
        sizes = [g[1] for g in got[:4]]
        assert sizes == sorted(sizes, reverse=True) and len(set(sizes)) == 4 and got[5][1] == 0


# 3. batches add up -------------------------------------------------------------------
def batches_case():
    """22 records; one 40-base segment occurs in record 3 and in record 17 and nowhere else."""
    def make():
        rng = np.random.default_rng(32)
        recs = [bases(rng, int(n)) for n in rng.integers(0, 400, size=22)]
        twice = bases(rng, 40)
        recs[3] = np.concatenate([bases(rng, 100), twice, bases(rng, 30)])
        recs[17] = np.concatenate([twice, NSEP, bases(rng, 80)])
        recs[8] = recs[5].copy()  # and a whole record twice
        return recs, twice
    return cached("batches", make)


@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("cuts", [[], [10], [4, 9, 9, 15]], ids=["1call", "2calls", "5calls"])
def test_accum_batches_add_up(kmc, oracle, cuda, lib, cuts):
    k, s = 21, 4096
    recs, twice = batches_case()
    ends = [0] + cuts + [len(recs)]
    batches = [pack(recs[a:b]) if b > a else EMPTY for a, b in zip(ends[:-1], ends[1:])]
    assert len(batches) == len(cuts) + 1 and (len(cuts) < 4 or batches[2] is EMPTY)  # the third of five calls is empty
    mix = mixture(oracle, "batches-mix", [pack(recs)], k)
    planted = U.mixture_hashes(oracle, *pack([twice]), k)[0]
    assert (U.multiplicities(mix, planted) == 2).all() and planted.size == 20
    total = sum(b[0].size for b in batches)
    with which(kmc, lib):
        with kmc.SketchAccum(s, k, log2_slots=roomy(total)) as acc:
            for b in batches:
                add(kmc, cuda, acc, b)
            one, two = finish(acc, 1), finish(acc, 2)
    check(one, mix, 1, s, 0, "m=1", lossless=True)
    check(two, mix, 2, s, 0, "m=2", lossless=True)
    assert two[1] < s and np.isin(planted, two[0][:two[1]]).all()  # once in each of two calls: it qualifies


# 4. the same key from every thread ---------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_accum_same_key_from_every_thread(kmc, oracle, cuda, lib):
    k, s = 21, 1000

    def make():
        rng = np.random.default_rng(33)
        one = bases(rng, 300)
        poly = [np.full(400, ord("A"), np.uint8), np.full(150, ord("T"), np.uint8), np.full(21, ord("A"), np.uint8)]
        return pack([one] * 64 + poly)
    batch = cached("same-key", make)
    mix = mixture(oracle, "same-key-mix", [batch], k)
    h, c = mix
    top = int(c.max())
    assert top == 380 + 130 + 1 and int((c == 64).sum()) == h.size - 1 == 280
    with which(kmc, lib):
        with kmc.SketchAccum(s, k, log2_slots=roomy(batch[0].size)) as acc:
            add(kmc, cuda, acc, batch)
            got = {m: finish(acc, m) for m in (1, 64, 65, top, top + 1)}
    for m, g in got.items():
        check(g, mix, m, s, 0, "m=%d" % m, lossless=True)
        assert g[2][2] == h.size  # tracked: the distinct keys
    assert got[64][1] == h.size and got[65][1] == 1 and got[top][1] == 1 and got[top + 1][1] == 0
    assert got[top][0][0] == h[c == top][0]


# 5. threshold and purge --------------------------------------------------------------
PURGE_LG = 8


def purge_case():
    """Four calls over a 27.5 kbase genome in records of 500 bases: its first 8 kbase,
    the same again, the next 16 kbase, then those again and the rest twice, so that
    almost every key ends with multiplicity 2.  N passes 2^13, 2^14 and 2^15 at the
    second, third and fourth call: with 256 slots j = 7, 8, 9, 10.  (Four equal calls
    cannot do that: a rise needs N to double.)"""
    def make():
        rng = np.random.default_rng(34)
        g = bases(rng, 27500)

        def cut(a, b):
            return [g[x:min(x + 500, b)] for x in range(a, b, 500)]
        calls = [cut(0, 8000), cut(0, 8000), cut(8000, 24000), cut(8000, 24000) + cut(24000, 27500) * 2]
        return [pack(c) for c in calls]
    return cached("purge", make)


def purge_levels():
    sizes = np.cumsum([b[0].size for b in purge_case()])
    return [level(int(n), PURGE_LG) for n in sizes]


def purge_seed(oracle, k, s):
    """The first hash seed, found with the oracle alone, at which at most C / 2 distinct
    hashes lie below the bound of every call and at least s hashes of multiplicity >= 2
    below the last one."""
    def make():
        batches, js = purge_case(), purge_levels()
        for seed in range(1, 13):
            ok = True
            for i, j in enumerate(js):
                h, c = mixture(oracle, ("purge-mix", seed, i), batches[:i + 1], k, 0, seed)
                ok = ok and int((h < np.uint64(bound(j))).sum()) <= (1 << PURGE_LG) // 2
            ok = ok and int(((h < np.uint64(bound(js[-1]))) & (c >= 2)).sum()) >= s
            if ok:
                return seed
        raise AssertionError("no seed among 12 fits the table: change the case")
    return cached("purge-seed", make)


@pytest.mark.parametrize("lib", LIBS)
def test_accum_threshold_and_purge(kmc, oracle, cuda, lib):
    k, s = 21, 16
    batches, js = purge_case(), purge_levels()
    assert js == [7, 8, 9, 10]
    seed = purge_seed(oracle, k, s)
    with which(kmc, lib):
        with kmc.SketchAccum(s, k, seed=seed, log2_slots=PURGE_LG) as acc:
            for i, b in enumerate(batches):
                add(kmc, cuda, acc, b)
                mix = mixture(oracle, ("purge-mix", seed, i), batches[:i + 1], k, 0, seed)
                for m in (1, 2):  # (finish leaves the accumulator as it is)
                    check(finish(acc, m), mix, m, s, js[i], "call %d m=%d" % (i, m), lossless=True)
            last = [finish(acc, m) for m in (1, 2, 3)]
    h, c = mix
    for m, g in zip((1, 2, 3), last):
        check(g, mix, m, s, js[-1], "final m=%d" % m, lossless=True)
    for m, g in zip((1, 2), last):  # the true bottom-16; m = 2: the counts survived the moves
        assert g[2][0] == 1 and g[1] == s
        np.testing.assert_array_equal(g[0], h[c >= m][:s])
    assert (last[0][0] != last[1][0]).any() or (c[:s] >= 2).all()


# 5b. the same through a roomy table: no threshold, no purge, the same bottom-16
@pytest.mark.parametrize("lib", LIBS)
def test_accum_purged_row_equals_unbounded_row(kmc, oracle, cuda, lib):
    k, s = 21, 16
    batches = purge_case()
    seed = purge_seed(oracle, k, s)
    with which(kmc, lib):
        rows = []
        for lg in (PURGE_LG, roomy(sum(b[0].size for b in batches))):
            with kmc.SketchAccum(s, k, seed=seed, log2_slots=lg) as acc:
                for b in batches:
                    add(kmc, cuda, acc, b)
                rows.append(finish(acc, 2))
    assert rows[0][1] == rows[1][1] == s and (rows[0][0] == rows[1][0]).all()
    assert rows[1][2][1] == FILL and rows[0][2][1] == bound(10)


# 6. lost inserts ---------------------------------------------------------------------
LOST_LG = 4


def lost_case(oracle, k):
    """4096 bytes of records (j = 10 with 16 slots: about 4 hashes below the bound are
    expected) and the first hash seed at which more than C / 2 = 8 distinct hashes lie
    below it; then the first small input (64 bytes: j = 4) of which, at that seed, 2 to
    8 distinct hashes lie below its bound.  All found on the CPU."""
    def make():
        rng = np.random.default_rng(35)
        batch = pack([bases(rng, 511) for _ in range(8)])
        assert batch[0].size == 4096 and level(4096, LOST_LG) == 10
        keys = S.unhash(U.mixture_hashes(oracle, *batch, k)[0])
        seed = next(sd for sd in range(1, 5000)
                    if int((S.hash_keys(keys, sd) < np.uint64(bound(10))).sum()) > (1 << LOST_LG) // 2)
        for ds in range(100):
            small = pack([bases(np.random.default_rng(3500 + ds), 63)])
            n = int((U.mixture_hashes(oracle, *small, k, 0, seed)[0] < np.uint64(bound(4))).sum())
            if 2 <= n <= 8:
                return batch, seed, small
        raise AssertionError("no small input fits: change the case")
    return cached(("lost", k), make)


@pytest.mark.parametrize("lib", LIBS)
def test_accum_lost_inserts(kmc, oracle, cuda, lib):
    k, s = 21, 2
    batch, seed, small = lost_case(oracle, k)
    assert small[0].size == 64 and level(64, LOST_LG) == 4
    mix = mixture(oracle, "lost-mix", [batch], k, 0, seed)
    mix_small = mixture(oracle, "lost-small-mix", [small], k, 0, seed)
    with which(kmc, lib):
        with kmc.SketchAccum(s, k, seed=seed, log2_slots=LOST_LG) as acc:
            add(kmc, cuda, acc, batch)  # (returns KMC_OK: the binding raises otherwise)
            lost = [finish(acc, m) for m in (1, 2)]
            acc.reset()
            add(kmc, cuda, acc, small)
            again = finish(acc, 1)
    for m, g in zip((1, 2), lost):
        check(g, mix, m, s, 10, "lost m=%d" % m, lossless=False)
    check(again, mix_small, 1, s, 4, "after reset", lossless=True)
    assert again[2][0] == 1 and again[1] == s


# 7. chains at the table's end --------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("s", [4, 16])
def test_accum_chains_wrap_round_the_table(kmc, oracle, cuda, lib, s):
    """FORWARD 8-mers whose slots are the last two of a 64-slot table: their chains run
    over the table's end into its first slots."""
    k, lg = 8, 6
    C = 1 << lg

    def make():
        keys = np.arange(1 << 16, dtype=np.uint64)
        h = S.hash_keys(keys)
        pick = np.nonzero(((h & np.uint64(C - 1)) >= np.uint64(C - 2)) & (h < np.uint64(1 << 58)))[0][:10]
        assert pick.size == 10
        kmers = [np.frombuffer(b"ACGT", np.uint8)[[(int(x) >> (2 * (k - 1 - p))) & 3 for p in range(k)]] for x in pick]
        parts = []
        for i, km in enumerate(kmers):
            parts += [km, NSEP] * (i % 3 + 1)
        return pack([np.concatenate(parts[:20]), np.concatenate(parts[20:])]), np.sort(h[pick])
    batch, chosen = cached("wrap", make)
    mix = mixture(oracle, "wrap-mix", [batch], k, FWD)
    np.testing.assert_array_equal(mix[0], chosen)
    assert sorted(set(int(x) for x in mix[1])) == [1, 2, 3]
    j = level(batch[0].size, lg)
    assert 0 < j <= 6 and (chosen < np.uint64(bound(j))).all()
    with which(kmc, lib):
        with kmc.SketchAccum(s, k, flags=FWD, log2_slots=lg) as acc:
            add(kmc, cuda, acc, batch)
            got = [finish(acc, m) for m in (1, 2, 3, 4)]
    for m, g in zip((1, 2, 3, 4), got):
        check(g, mix, m, s, j, "s=%d m=%d" % (s, m), lossless=True)
        assert g[2][2] == 10
    assert got[0][1] == min(s, 10)


# 8. life cycle -----------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_accum_life_cycle(kmc, oracle, cuda, lib):
    k, s = 21, 64
    first, second = planted_case(), pack(batches_case()[0])
    lg = roomy(first[0].size + second[0].size)
    none = (np.zeros(0, np.uint64), np.zeros(0, np.int64))
    with which(kmc, lib) as D:
        L = D if lib == "diag" else kmc.lib()
        with kmc.SketchAccum(s, k, log2_slots=lg) as acc:
            live_handle_errors(L, acc._h)
            empty = finish(acc, 1)  # before any add
            add(kmc, cuda, acc, first)
            one = finish(acc, 2)
            add(kmc, cuda, acc, EMPTY)  # num_seqs == 0 leaves everything as it is
            same = finish(acc, 2)
            add(kmc, cuda, acc, second)  # add after finish
            both = finish(acc, 2)
            acc.reset()
            cleared = finish(acc, 1)
            add(kmc, cuda, acc, second)
            after_reset = finish(acc, 1)
        with kmc.SketchAccum(s, k, log2_slots=lg) as fresh:
            add(kmc, cuda, fresh, second)
            of_fresh = finish(fresh, 1)
        with pytest.raises(ValueError):
            fresh.add(None, None)  # closed
    for g in (empty, cleared):
        check(g, none, 1, s, 0, "nothing added", lossless=True)
        assert g[1] == 0 and g[2] == [1, FILL, 0, 0]
    check(one, mixture(oracle, "planted-mix", [first], k), 2, s, 0, "first", lossless=True)
    assert same[1] == one[1] and (same[0] == one[0]).all() and same[2] == one[2]
    check(both, mixture(oracle, "life-both", [first, second], k), 2, s, 0, "both", lossless=True)
    check(after_reset, mixture(oracle, "batches-mix", [second], k), 1, s, 0, "after reset", lossless=True)
    assert after_reset[1] == of_fresh[1] and (after_reset[0] == of_fresh[0]).all() and after_reset[2] == of_fresh[2]
