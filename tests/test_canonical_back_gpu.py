"""The canonical counter's back half at its edges: the two K4s
counting-sort instances (sort_list), the probed table kernel (canon_table_kernel),
the direct-output reservation chain (reserve_pairs, chain_from, run_direct's launch
groups) and the two readers of pk (canon_fallback_kernel, canon_place_kernel).

Every GPU case is compared with the self-oracle (oracle.count_canonical): per-record
sorted (key, count) sets bit for bit, and rec_off; the constructed inputs also with
np_count over the k-mers the test laid down.  No case assumes the path it is named
after: each asserts it from a Python mirror below (slot_words / list_mirror: K4s's
slot words, nsk, na, nres, nhot; pass_of / table_split: the table kernel's passes;
launch_groups: run_direct's groups) and, for a direct-output call, from the
diagnostic read-backs kmc_diag_canon_fallback[_detail] (fallback entries and pairs,
pairs per record, lists queued to the big instance and to the table kernel's two
launches).  Those read-backs exist for direct-output calls only: a call with direct
output off (kmc_diag_canon_direct(0): pk and canon_place_kernel) must leave them
unchanged, and its route is the mirror's.  Every case runs both; parts E and G run
direct output only (the chain exists only there).

Inputs follow the front-half suite (test_canonical_front_gpu.py): KMC_CANON_FORWARD
31-mers, one N after each (32 bytes and one valid window per key).  A list holds
h = feistel(key); K4s's slot is its low 12 bits (13 in the big instance) and the sub
the next 4, so a key of a wanted slot and sub is feistel((random << 17) | low bits)
(the round is its own inverse and keeps the high 45 bits).  A record of more than
4096 windows has 2^lg lists, and every constructed key then lies in list 0 (top lg
bits of key * C zero).  Where only a list's length matters, a random record of n + 30
bases is one list of exactly n keys (n <= 4096).

The CPU-only tests (no gpu mark) check the mirrors against a word-by-word restatement
and prove each input's claims -- exactly n keys in list 0, nres, nhot, the pass bits,
the launch groups -- from the oracle's output alone.
"""
import ctypes
import types

import numpy as np
import pytest

from test_canonical_front_gpu import (KC, N_BYTE, Records, assert_equal, bases, cu_count, keys_for_lists, kmer_bytes,
                                      lay, list_of, np_count, oracle_list_counts, plan, run)
from test_hash_gpu import _list_value

gpu = pytest.mark.gpu

# kmc_hash.hip's constants
SORT_MAX_M = 16        # kSortMaxM: keys per slot the pairwise dedup takes
HOT_MAX = 128          # kHotMax: crowded slots per list K4s takes
PASS_DISTINCT = 2048   # kPassDistinct
RES_KEYS = 8192        # kResKeys: a list the table kernel keeps in registers
CLAIM_W = 320          # kClaimW
MAX_INIT_PASSES = 16
PASS_BITS = 17
MAX_PASSES = 1 << PASS_BITS
GROUP_LISTS = 8192     # kGroupLists
PASS_C = 0xD6E8FEB86659FD93
PASS_CINV = pow(PASS_C, -1, 1 << 64)
ERR_INVALID_ARG = 1001
# SortSmall / SortBig: slot bits, kCap, kSk, kRc
COMMON = types.SimpleNamespace(name="common", slots_lg=12, cap=6080, sk=7456, rc=1024)
BIG = types.SimpleNamespace(name="big", slots_lg=13, cap=12288, sk=15232, rc=2048)
INSTANCES = {"common": COMMON, "big": BIG}


# ---------------------------------------------------------------------------
# the mirrors
# ---------------------------------------------------------------------------
def feistel(x):
    return _list_value(np.asarray(x, dtype=np.uint64))


def popcount16(x):
    return np.unpackbits(np.asarray(x).astype(">u2").view(np.uint8)).reshape(-1, 16).sum(axis=1)


def slot_words(h, inst, counts=None):
    """K4s's slot words after the rank step, of the list values h (each `counts`
    times): per slot the key count (the word's low half) and the verdict -- the
    high half sums 2^sub per key, truncated to 16 bits, and the slot's keys are
    proved distinct when it has as many bits set as the slot has keys."""
    h = np.asarray(h, dtype=np.uint64)
    w = np.ones(h.size, np.int64) if counts is None else np.asarray(counts).astype(np.int64)
    S = 1 << inst.slots_lg
    slot = (h & np.uint64(S - 1)).astype(np.int64)
    sub = ((h >> np.uint64(inst.slots_lg)) & np.uint64(15)).astype(np.int64)
    cnt = np.zeros(S, np.int64)
    hi = np.zeros(S, np.int64)
    np.add.at(cnt, slot, w)
    np.add.at(hi, slot, w << sub)
    assert cnt.max(initial=0) < 1 << 16
    return cnt, popcount16(hi & 0xFFFF) == cnt


def list_mirror(h, inst, counts=None):
    """Of one list in a K4s instance: n keys, nsk of them in failing slots, na in
    distinct ones, nres results (distinct keys in failing slots), nhot crowded slots
    (failing, more than kSortMaxM keys), rcap results staged in LDS, and how many
    results have a count below 4 (a tag, not the escape to pc)."""
    h = np.asarray(h, dtype=np.uint64)
    w = np.ones(h.size, np.int64) if counts is None else np.asarray(counts).astype(np.int64)
    cnt, dist = slot_words(h, inst, w)
    fail = ~dist
    uh, inv = np.unique(h, return_inverse=True)
    uc = np.bincount(inv, weights=w, minlength=uh.size).astype(np.int64)
    in_fail = fail[(uh & np.uint64((1 << inst.slots_lg) - 1)).astype(np.int64)]
    n, nsk = int(cnt.sum()), int(cnt[fail].sum())
    return types.SimpleNamespace(n=n, nsk=nsk, na=n - nsk, nres=int(in_fail.sum()),
                                 nhot=int((fail & (cnt > SORT_MAX_M)).sum()), rcap=min(inst.sk - n, inst.rc),
                                 small_results=int((in_fail & (uc < 4)).sum()), cnt=cnt, fail=fail)


def k4_route(h, counts=None, c=COMMON.cap, b=BIG.cap):
    """Which kernel counts a list of these list values under sort caps c and b:
    (route, mirror), route one of common, big, table1 (too long for the big
    instance), table2 (handed back by K4s: more than kHotMax crowded slots), and the
    queue counts (big, table1, table2) a direct-output call of that one list reads back."""
    n = h.size if counts is None else int(np.asarray(counts).astype(np.int64).sum())
    if n > c and n > b:
        return "table1", None, (0, 1, 0)
    inst = COMMON if n <= c else BIG
    m = list_mirror(h, inst, counts)
    q_big = 1 if inst is BIG else 0
    if m.nhot > HOT_MAX:
        return "table2", m, (q_big, 0, 1)
    return inst.name, m, (q_big, 0, 0)


def fallback_of(route, m, distinct):
    """(entries, pairs) the fallback copies of a list of record 0 (its start is known
    from the setup): a table list is one copy of all its pairs, a K4s list one copy
    of the results past the stage, if any."""
    if route.startswith("table"):
        return 1, distinct
    over = max(0, m.nres - m.rcap)
    return (1 if over else 0), over


def pass_bits(h):
    with np.errstate(over="ignore"):
        x = np.asarray(h, dtype=np.uint64) * np.uint64(PASS_C)
    return ((x >> np.uint64(32)) & np.uint64(MAX_PASSES - 1)).astype(np.int64)


def pass_of(h, P):
    """The table kernel's pass of h among P: the P-quantile of 17 bits of h * odd."""
    return (pass_bits(h) * P) >> PASS_BITS


def initial_passes(n):
    return 1 if n <= PASS_DISTINCT else min(MAX_INIT_PASSES, -(-n // PASS_DISTINCT))


def table_split(bits_by_wave, n, cap):
    """The pass loop of canon_table_kernel for distinct keys whose pass bits are
    known per wave: a pass in which a wave claims more than cap is split in two; the
    final P, or None where a pass still overflows at kMaxPasses (kErrPasses)."""
    P, q = initial_passes(n), 0
    while q < P:
        if any(int((((b * P) >> PASS_BITS) == q).sum()) > cap for b in bits_by_wave):
            if P >= MAX_PASSES:
                return None
            P, q = 2 * P, 2 * q
            continue
        q += 1
    return P


def launch_groups(lists):
    """run_direct's launches of the common instance: [r0, r1) per group, from the
    lists per record."""
    lb = np.concatenate([[0], np.cumsum(lists)])
    n, out, r0 = len(lists), [], 0
    while r0 < n:
        r1 = r0 + 1
        if lb[r1] - lb[r0] < GROUP_LISTS:
            while r1 < n and lb[r1 + 1] - lb[r0] <= GROUP_LISTS and lb[r1 + 1] - lb[r1] < GROUP_LISTS:
                r1 += 1
        out.append((r0, r1))
        r0 = r1
    return out


# ---------------------------------------------------------------------------
# building inputs
# ---------------------------------------------------------------------------
def lg_for(nkeys):
    """log2 lists of a record of nkeys 32-byte keys at the shipped target."""
    return plan([0, 32 * nkeys + 1], KC, 1).lg[0]


def in_list0(keys, lg):
    return np.ones(len(keys), dtype=bool) if lg == 0 else list_of(keys, lg) == 0


def random_keys(rng, n, lg):
    """n distinct 31-mer keys of list 0 of 2^lg."""
    if lg:
        return keys_for_lists(rng, np.zeros(n, np.int64), lg)
    out = np.unique(rng.integers(0, 1 << (2 * KC), size=2 * n + 8, dtype=np.uint64))
    assert out.size >= n
    return rng.permutation(out)[:n]


def keys_with_low17(rng, low, lg):
    """One key per entry of `low` whose list value has those low 17 bits (slot and
    sub of both K4s instances), all distinct, in list 0 of 2^lg."""
    low = np.asarray(low, dtype=np.uint64)
    out = np.zeros(low.size, dtype=np.uint64)
    todo = np.arange(low.size)
    while todo.size:
        hi = rng.integers(0, 1 << 45, size=todo.size, dtype=np.uint64)
        key = feistel((hi << np.uint64(17)) | low[todo])
        ok = in_list0(key, lg)
        out[todo[ok]] = key[ok]
        todo = todo[~ok]
    assert np.unique(out).size == out.size and (out < np.uint64(1 << (2 * KC))).all()
    assert ((feistel(out) & np.uint64(0x1FFFF)) == low).all()
    return out


def keys_with_pass_bits(rng, bits):
    """One key per entry of `bits` whose list value has those 17 pass bits, all distinct."""
    bits = np.asarray(bits, dtype=np.uint64)
    out = np.zeros(bits.size, dtype=np.uint64)
    todo = np.arange(bits.size)
    hole = ~np.uint64((MAX_PASSES - 1) << 32)
    while todo.size:
        x = np.frombuffer(rng.bytes(8 * todo.size), dtype=np.uint64)
        with np.errstate(over="ignore"):
            h = ((x & hole) | (bits[todo] << np.uint64(32))) * np.uint64(PASS_CINV)
        ok = h < np.uint64(1 << (2 * KC))
        out[todo[ok]] = feistel(h[ok])
        todo = todo[~ok]
    assert np.unique(out).size == out.size and (pass_bits(feistel(out)) == bits.astype(np.int64)).all()
    return out


def key_record(keys):
    """One record of these keys in order, each 31 bases and one N, at the shipped
    target: data, idx, lg; every key in list 0."""
    keys = np.asarray(keys, dtype=np.uint64)
    data = np.concatenate([kmer_bytes(keys), np.zeros(1, np.uint8)])
    idx = np.array([0, data.size], dtype=np.int64)
    lg = plan(idx, KC, 1).lg[0]
    assert lg == lg_for(keys.size) and in_list0(keys, lg).all()
    return data, idx, lg


_cases = {}


def cached(fn):
    def get(*args):
        if (fn.__name__, args) not in _cases:
            c = fn(*args)
            c.name = "%s%s" % (fn.__name__, args)
            c.exp = None
            _cases[(fn.__name__, args)] = c
        return _cases[(fn.__name__, args)]
    get.__name__ = fn.__name__
    return get


def case_of(data, idx, k=KC, forward=True, keys=None, lg=None, laid=True, **facts):
    """An input: `keys` the constructed keys of record 0's list 0 (None: random
    records), `laid`: also compared with np_count."""
    return types.SimpleNamespace(data=data, idx=idx, k=k, forward=forward, keys=keys, lg=lg, laid=laid,
                                 facts=types.SimpleNamespace(**facts))


def expected(oracle, c):
    """The oracle's result of a case (and np_count's), computed once and shared."""
    if c.exp is None:
        exp = oracle.count_canonical(c.data, c.idx, c.k, forward=c.forward)
        for a in exp:
            a.setflags(write=False)
        c.laid_sets = np_count(c.data, c.idx, c.k, forward=c.forward) if c.laid else None
        c.exp = exp
    return c.exp


# A. list length -------------------------------------------------------------
HOOK_C, HOOK_B = 2000, 3000
HOOK_NS = (HOOK_C - 1, HOOK_C, HOOK_C + 1, HOOK_B, HOOK_B + 1)
SHIPPED_NS = (COMMON.cap, COMMON.cap + 1, BIG.cap, BIG.cap + 1)


@cached
def random_list_case(n):
    """A random record of n + 30 bases: one list of exactly n keys (canonical)."""
    rng = np.random.default_rng(5000 + n)
    R = Records(rng)
    R.add(bases(rng, n + KC - 1))
    data, idx = R.done()
    return case_of(data, idx, forward=False, lg=0, n=n)


@cached
def short_record_case(k, alone, nbases):
    """A record of k - 1 bases (no window) or k bases (one), alone or between
    ordinary records."""
    rng = np.random.default_rng(5100 + 10 * k + nbases)
    R = Records(rng)
    if not alone:
        R.add(bases(rng, 500, 0.02))
    r = R.add(bases(rng, nbases))
    if not alone:
        R.add(bases(rng, 3000, 0.02))
        R.add(bases(rng, 2 * k - 1 - nbases))  # the other of the two
        R.add(bases(rng, 200))
    data, idx = R.done()
    return case_of(data, idx, k=k, forward=False, r=r, windows=nbases - k + 1)


@cached
def shipped_cap_case(n):
    """A record whose list 0 holds exactly n distinct keys (the others none)."""
    rng = np.random.default_rng(5200 + n)
    keys = random_keys(rng, n, lg_for(n))
    data, idx, lg = key_record(keys)
    return case_of(data, idx, keys=keys, lg=lg, n=n)


# B, G. staged results -------------------------------------------------------
LG_GEN = 7  # the constructed records have at most 2^7 lists at the shipped target


def staged_keys(rng, inst, n_base, nres, pure, lg):
    """Keys of one list whose mirror gives exactly `nres` results.  Mixed: n_base
    random distinct keys, then keys written again one at a time (once more, every
    fourth four times more) wherever that does not overshoot: a key written again
    fails its slot, and every distinct key of that slot becomes a result.  Pure: no
    slot of the n_base keys fails, and only keys alone in their slot are written
    again, three times more each, so that every result has count 4: whichever results
    land past the stage, their counts are escaped to pc."""
    S = 1 << inst.slots_lg
    if pure:
        pool = random_keys(rng, 3 * n_base, lg)
        hp = feistel(pool)
        _, first = np.unique(hp & np.uint64(16 * S - 1), return_index=True)  # one key per (slot, sub)
        keys = pool[np.sort(first)[:n_base]]
    else:
        keys = random_keys(rng, n_base, lg)
    assert keys.size == n_base
    slot = (feistel(keys) & np.uint64(S - 1)).astype(np.int64)
    per_slot = np.bincount(slot, minlength=S)
    m0 = list_mirror(feistel(keys), inst)
    if pure:
        assert m0.nres == 0
        alone = np.flatnonzero(per_slot[slot] == 1)[:nres]
        assert alone.size == nres
        extra = np.repeat(keys[alone], 3)
    else:
        failing, have, extra, j = m0.fail.copy(), m0.nres, [], 0
        for i in range(n_base):
            if have == nres:
                break
            s = slot[i]
            if failing[s] or have + per_slot[s] > nres:
                continue
            extra += [keys[i]] * (4 if j % 4 == 0 else 1)
            j += 1
            failing[s] = True
            have += per_slot[s]
        assert have == nres
        extra = np.array(extra, dtype=np.uint64)
    return np.concatenate([keys, extra])


def staged_params(inst_name, where):
    inst = INSTANCES[inst_name]
    nres = inst.rc + where
    pure = where > 0
    n_base = {("common", False): 3000, ("common", True): 2000 + 3 * max(0, where - 1),
              ("big", False): 6000, ("big", True): 4096}[(inst_name, pure)]
    return inst, nres, pure, n_base


@cached
def staged_case(inst_name, where):
    """A record whose list 0 has exactly kRc + where results in this instance."""
    inst, nres, pure, n_base = staged_params(inst_name, where)
    rng = np.random.default_rng(5300 + 10 * inst.slots_lg + where)
    keys = staged_keys(rng, inst, n_base, nres, pure, LG_GEN)
    data, idx, lg = key_record(keys)
    return case_of(data, idx, keys=keys, lg=lg, inst=inst, nres=nres, pure=pure)


G_OVER = 100
G_LG_WINDOWS, G_LF = 17, 6  # lay: 2^13 lists at 32 windows per list


@cached
def split_copy_case():
    """Record 0: random, 2^13 lists under lay's target, a launch group of its own.
    Record 1 (lay): a list 0 of kRc + 100 results, every one of count 4."""
    inst, nres, pure, n_base = staged_params("common", G_OVER)
    rng = np.random.default_rng(5900)
    keys = staged_keys(rng, inst, n_base, nres, pure, 7 + G_LF)
    d1, i1, laid, _, target = lay([keys], G_LG_WINDOWS, G_LF)
    assert (laid == keys).all()
    d0 = np.append(bases(rng, (1 << G_LG_WINDOWS) + 1 + KC - 1), np.uint8(0))
    data = np.concatenate([d0, d1])
    idx = np.array([0, d0.size, d0.size + d1.size], dtype=np.int64)
    return case_of(data, idx, keys=keys, lg=7 + G_LF, inst=inst, nres=nres, pure=True, target=target, laid=False)


# C. slot population ---------------------------------------------------------
@cached
def slot_case(inst_name):
    """Five groups, each in a slot of its own of list 0, and 40 keys elsewhere:
    slot 5: 15 keys on subs 0..14, one written twice (16 keys, fails: the pairwise
            dedup with both tiers of its reads);
    slot 6: 16 keys on all subs, one written twice (17 keys: crowded);
    slot 7: one key 128 times; slot 8: one key 129 times (one pivot chunk, and two);
    slot 9: two keys, 64 and 65 times, interleaved."""
    inst = INSTANCES[inst_name]
    rng = np.random.default_rng(5400 + inst.slots_lg)
    s = inst.slots_lg
    total = 16 + 17 + 128 + 129 + 129 + 40
    lg = lg_for(total)
    low = lambda slot, subs: [slot | (su << s) for su in subs]
    g16 = keys_with_low17(rng, low(5, range(15)), lg)
    g17 = keys_with_low17(rng, low(6, range(16)), lg)
    one128, one129 = keys_with_low17(rng, low(7, [3]) + low(8, [11]), lg)
    two = keys_with_low17(rng, low(9, [2, 9]), lg)
    pool = random_keys(rng, 80, lg)
    other = pool[~np.isin(feistel(pool) & np.uint64((1 << s) - 1), np.arange(5, 10).astype(np.uint64))][:40]
    assert other.size == 40
    inter = np.empty(129, dtype=np.uint64)
    inter[0::2], inter[1::2] = two[1], two[0]  # 65 and 64
    keys = np.concatenate([other[:20], g16, g16[3:4], g17, g17[7:8], np.repeat(one128, 128), other[20:30],
                           np.repeat(one129, 129), inter, other[30:]])
    assert keys.size == total
    data, idx, lg = key_record(keys)
    return case_of(data, idx, keys=keys, lg=lg, inst=inst, slots={5: 16, 6: 17, 7: 128, 8: 129, 9: 129},
                   nhot=4, group_results=15 + 16 + 1 + 1 + 2, other=other)


# D. kHotMax -----------------------------------------------------------------
@cached
def hot_case(inst_name, nkeys):
    """nkeys distinct keys in slots of their own, each written 17 times (crowded),
    and one more written 16 times (fails, not crowded: exactly kSortMaxM)."""
    inst = INSTANCES[inst_name]
    rng = np.random.default_rng(5500 + inst.slots_lg + nkeys)
    total = 17 * nkeys + 16
    lg = lg_for(total)
    pool = random_keys(rng, 4 * nkeys, lg)
    _, first = np.unique(feistel(pool) & np.uint64((1 << inst.slots_lg) - 1), return_index=True)
    pick = pool[np.sort(first)[:nkeys + 1]]
    assert pick.size == nkeys + 1
    keys = rng.permutation(np.concatenate([np.repeat(pick[:nkeys], 17), np.repeat(pick[nkeys:], 16)]))
    data, idx, lg = key_record(keys)
    return case_of(data, idx, keys=keys, lg=lg, inst=inst, n=total, nhot=nkeys, nres=nkeys + 1)


# E. the chain and the launch groups -----------------------------------------
CHAIN_TARGET = 16


def random_case(rng, windows, k, target, **facts):
    R = Records(rng)
    for w in windows:
        if w is None:
            R.empty()
        elif isinstance(w, np.ndarray):
            R.add(w)
        else:
            R.add(bases(rng, w + k - 1))
    data, idx = R.done()
    return case_of(data, idx, k=k, forward=False, laid=False, target=target, **facts)


@cached
def chain_case(which):
    rng = np.random.default_rng(5600 + which)
    k = KC
    if which == 1:  # three records of 8192 lists: each a group of its own
        return random_case(rng, [131072] * 3, k, CHAIN_TARGET, lists=[8192] * 3, groups=[(0, 1), (1, 2), (2, 3)],
                           zero=[0, 1, 2])
    if which == 2:  # 4096 lists each: records 0 and 1 share a group, record 2 is alone
        return random_case(rng, [65536] * 3, k, CHAIN_TARGET, lists=[4096] * 3, groups=[(0, 2), (2, 3)], zero=[0, 2])
    if which == 3:  # 8193 one-list records at the shipped target: the last starts the second group
        return random_case(rng, [10] * 8193, k, 4096, lists=[1] * 8193, groups=[(0, 8192), (8192, 8193)],
                           zero=[0, 8192])
    # ten records without a window of each kind, an 8192-list record, records without a window
    n_run = lambda n: np.full(n, N_BYTE, dtype=np.uint8)
    none = [None, bases(rng, 5), n_run(100), None, bases(rng, k - 1), n_run(40), None, bases(rng, 1), n_run(k), None]
    tail = [None, None, bases(rng, 7), n_run(50), None]
    return random_case(rng, none + [131072] + tail, k, CHAIN_TARGET,
                       lists=[1, 1, 8, 1, 1, 1, 1, 1, 1, 1, 8192, 1, 1, 1, 2, 1],
                       groups=[(0, 10), (10, 11), (11, 16)], zero=list(range(16)), big=10)


# F. table kernel ------------------------------------------------------------
TABLE_NS = (PASS_DISTINCT, PASS_DISTINCT + 1, RES_KEYS, RES_KEYS + 1)


@cached
def table_case(kind):
    rng = np.random.default_rng(5700 + (kind if isinstance(kind, int) else len(kind)))
    if isinstance(kind, int):  # a list 0 of exactly `kind` distinct keys
        keys = random_keys(rng, kind, lg_for(kind))
    elif kind == "one_pass_of_two":  # 4096 distinct keys, all in pass 0 of 2
        pool = random_keys(rng, 3 * 4096, lg_for(4096))
        keys = pool[pass_of(feistel(pool), 2) == 0][:4096]
        assert keys.size == 4096
    else:  # one key 4096 times
        assert kind == "one_key"
        keys = np.repeat(random_keys(rng, 1, lg_for(4096)), 4096)
    data, idx, lg = key_record(keys)
    return case_of(data, idx, keys=keys, lg=lg, n=keys.size)


PASS_CAP = 8
PASS_PREFIX = MAX_PASSES - 2  # all pass bits but the lowest: the keys' passes are the last two


@cached
def pass_bits_case(nkeys):
    """A one-list record: 16 keys, eight with pass bits 1...10 and eight with
    1...11 (they part only at P = 2^17); or 100 keys that agree on all 17 bits."""
    rng = np.random.default_rng(5800 + nkeys)
    bits = [PASS_PREFIX | (i & 1) for i in range(16)] if nkeys == 16 else [PASS_PREFIX | 1] * nkeys
    keys = keys_with_pass_bits(rng, bits)
    data, idx, lg = key_record(keys)
    assert lg == 0
    return case_of(data, idx, keys=keys, lg=lg, n=nkeys, bits=np.array(bits, dtype=np.int64))


def waves_of(n, bits):
    """Pass bits per wave of the table kernel (key i of a resident list: thread
    i mod 512), for lists whose bits do not depend on the order within a wave."""
    assert n <= 512
    return [bits[a:a + 64] for a in range(0, n, 64)]


# ---------------------------------------------------------------------------
# CPU only: the mirrors, and every input's claims from the oracle alone
# ---------------------------------------------------------------------------
def words_one_by_one(h, inst):
    """slot_words restated on the 32-bit words themselves: one add of
    1 + 2^(16 + sub) per key, wrapping."""
    S = 1 << inst.slots_lg
    word = [0] * S
    for x in h:
        x = int(x)
        word[x & (S - 1)] = (word[x & (S - 1)] + 1 + (0x10000 << ((x >> inst.slots_lg) & 15))) & 0xFFFFFFFF
    cnt = np.array([w & 0xFFFF for w in word])
    return cnt, np.array([bin(w >> 16).count("1") for w in word]) == cnt


@pytest.mark.parametrize("inst", (COMMON, BIG), ids=lambda i: i.name)
def test_slot_words_mirror(inst):
    """slot_words against the words added one key at a time; the verdict on its
    known edges; feistel its own inverse."""
    rng = np.random.default_rng(600 + inst.slots_lg)
    h = rng.integers(0, 1 << 62, size=3000, dtype=np.uint64)
    h = np.concatenate([h, h[:300], h[:40], np.repeat(h[500:503], 20)])  # repeats, a crowded slot or three
    cnt, dist = slot_words(h, inst)
    c1, d1 = words_one_by_one(h, inst)
    np.testing.assert_array_equal(cnt, c1)
    np.testing.assert_array_equal(dist, d1)
    uh, uc = np.unique(h, return_counts=True)
    c2, d2 = slot_words(uh, inst, uc)  # keys with counts == keys written out
    np.testing.assert_array_equal(cnt, c2)
    np.testing.assert_array_equal(dist, d2)
    assert (feistel(feistel(h)) == h).all()
    s = inst.slots_lg
    mk = lambda slot, subs: np.array([(7 + i) << 17 | su << s | slot for i, su in enumerate(subs)], dtype=np.uint64)
    m = list_mirror(mk(1, range(16)), inst)  # 16 keys on 16 subs: the largest slot that passes
    assert (m.nsk, m.na, m.nres, m.nhot) == (0, 16, 0, 0)
    m = list_mirror(mk(2, [15, 15]), inst)   # the sum carries out of the word
    assert (m.nsk, m.na, m.nres, m.nhot) == (2, 0, 2, 0)
    m = list_mirror(np.concatenate([mk(3, range(16)), mk(3, [4])[:1]]), inst)  # 17 keys, one sub twice: crowded
    assert (m.nsk, m.nres, m.nhot) == (17, 17, 1)
    m = list_mirror(np.repeat(mk(4, [9]), 16), inst)  # one key 16 times: fails, not crowded
    assert (m.nsk, m.nres, m.nhot, m.small_results) == (16, 1, 0, 0)


def test_pass_mirror():
    """pass_of: pass q of P splits into 2q and 2q + 1 of 2P; table_split on the two
    pass-bit inputs; the initial passes at kPassDistinct and kMaxInitPasses."""
    h = np.random.default_rng(601).integers(0, 1 << 62, size=5000, dtype=np.uint64)
    assert (pass_of(h, 1) == 0).all()
    for P in (1, 2, 16, 1 << 16):
        assert (pass_of(h, 2 * P) >> 1 == pass_of(h, P)).all() and pass_of(h, P).max() < P
    assert (pass_of(h, MAX_PASSES) == pass_bits(h)).all() and np.unique(pass_of(h, 2)).size == 2
    assert [initial_passes(n) for n in (1, 2048, 2049, 4096, 4097, 8192, 8193, 1 << 20)] == [1, 1, 2, 2, 3, 4, 5, 16]
    c = pass_bits_case(16)
    assert table_split(waves_of(16, c.facts.bits), 16, PASS_CAP) == MAX_PASSES
    assert table_split(waves_of(16, c.facts.bits), 16, PASS_CAP - 1) is None
    c = pass_bits_case(100)
    assert table_split(waves_of(100, c.facts.bits), 100, PASS_CAP) is None
    assert table_split(waves_of(100, c.facts.bits), 100, CLAIM_W) == 1


def test_launch_groups_mirror():
    assert launch_groups([8192, 8192]) == [(0, 1), (1, 2)]
    assert launch_groups([4096, 4096, 4096]) == [(0, 2), (2, 3)]
    assert launch_groups([4096, 4097]) == [(0, 1), (1, 2)]
    assert launch_groups([1] * 8193) == [(0, 8192), (8192, 8193)]
    assert launch_groups([1, 32768, 1, 1]) == [(0, 1), (1, 2), (2, 4)]


def list0_mirror(oracle, c, inst):
    """The mirror of list 0 of the constructed record, from the oracle's keys and
    counts; proves first that the record's keys are the laid ones and all in list 0."""
    exp = expected(oracle, c)
    r = len(c.idx) - 2  # the constructed record is the call's last
    a, b = int(exp[2][r]), int(exp[2][r + 1])
    ek, ec = exp[0][a:b], exp[1][a:b]
    lk, lc = np.unique(c.keys, return_counts=True)
    np.testing.assert_array_equal(ek, lk)
    np.testing.assert_array_equal(ec.astype(np.int64), lc)
    if c.laid:
        np.testing.assert_array_equal(c.laid_sets[r][0], lk)
        np.testing.assert_array_equal(c.laid_sets[r][1], lc)
    if c.lg:
        per_list = np.bincount(list_of(ek, c.lg), weights=ec, minlength=1 << c.lg).astype(np.int64)
        assert per_list[0] == c.keys.size and per_list[1:].sum() == 0
        if r == 0:
            np.testing.assert_array_equal(per_list, oracle_list_counts(exp, c.lg))
    return list_mirror(feistel(ek), inst, ec), feistel(ek), ec


@pytest.mark.parametrize("n", HOOK_NS + (0, 1))
def test_inputs_random_list_of_exactly_n(oracle, n):
    c = random_list_case(n) if n > 1 else short_record_case(KC, True, KC - 1 + n)
    exp = expected(oracle, c)
    assert plan(c.idx, KC, 1).lg == [0] and int(exp[1].astype(np.int64).sum()) == n


@pytest.mark.parametrize("n", SHIPPED_NS)
def test_inputs_list0_of_exactly_n_at_the_shipped_caps(oracle, n):
    c = shipped_cap_case(n)
    assert c.lg == plan(c.idx, KC, 1).lg[0] == (6 if n <= COMMON.cap + 1 else 7)
    _, h, counts = list0_mirror(oracle, c, COMMON)
    route, m, _ = k4_route(h, counts)
    assert route == {6080: "common", 6081: "big", 12288: "big", 12289: "table1"}[n]
    if m is not None:
        assert m.n == n and m.nhot == 0


@pytest.mark.parametrize("where", (-1, 0, 1))
@pytest.mark.parametrize("inst_name", ("common", "big"))
def test_inputs_results_at_the_stage(oracle, inst_name, where):
    c = staged_case(inst_name, where)
    m, _, _ = list0_mirror(oracle, c, c.facts.inst)
    inst = c.facts.inst
    assert m.nres == inst.rc + where == c.facts.nres and m.rcap == inst.rc and m.nhot == 0
    assert (COMMON.cap if inst is BIG else 1) < m.n <= inst.cap
    if where > 0:  # whichever results are past the stage, some have escaped counts
        assert m.small_results == 0
    else:
        assert 0 < m.small_results < m.nres


def test_inputs_split_copy_record(oracle):
    c = split_copy_case()
    m, _, _ = list0_mirror(oracle, c, COMMON)
    assert m.nres == COMMON.rc + G_OVER and m.rcap == COMMON.rc and m.n <= COMMON.cap and m.small_results == 0
    P = plan(c.idx, KC, 1, c.facts.target)
    assert P.lg == [13, 13] and launch_groups([1 << g for g in P.lg]) == [(0, 1), (1, 2)]
    assert max_list_length(expected(oracle, c), P.lg, [0]) <= COMMON.rc


@pytest.mark.parametrize("inst_name", ("common", "big"))
def test_inputs_slot_groups(oracle, inst_name):
    c = slot_case(inst_name)
    m, _, _ = list0_mirror(oracle, c, c.facts.inst)
    for slot, count in c.facts.slots.items():
        assert m.cnt[slot] == count and m.fail[slot], (slot, count)
    other = list_mirror(feistel(c.facts.other), c.facts.inst)
    assert m.nhot == c.facts.nhot == 4 and m.nres == c.facts.group_results + other.nres
    assert m.nsk == sum(c.facts.slots.values()) + other.nsk and m.na == other.na > 0


@pytest.mark.parametrize("nkeys", (HOT_MAX, HOT_MAX + 1))
@pytest.mark.parametrize("inst_name", ("common", "big"))
def test_inputs_crowded_slots_at_khotmax(oracle, inst_name, nkeys):
    c = hot_case(inst_name, nkeys)
    m, _, _ = list0_mirror(oracle, c, c.facts.inst)
    assert (m.n, m.nsk, m.nres, m.nhot) == (17 * nkeys + 16, 17 * nkeys + 16, nkeys + 1, nkeys)
    assert sorted(m.cnt[m.cnt > 0]) == [16] + [17] * nkeys  # one slot each


def max_list_length(exp, lgs, records):
    """The longest list (windows) of these records, from the oracle's canonical keys."""
    out = 0
    for r in records:
        a, b = int(exp[2][r]), int(exp[2][r + 1])
        if b > a:
            lists = list_of(exp[0][a:b], lgs[r]) if lgs[r] else np.zeros(b - a, np.int64)
            out = max(out, int(np.bincount(lists, weights=exp[1][a:b]).max()))
    return out


@pytest.mark.parametrize("which", (1, 2, 3, 4))
def test_inputs_chain_records_and_groups(oracle, which):
    """Lists per record and launch groups by the mirrors; no list is long enough to
    queue a copy for another reason than an unknown record start (nres <= n <= kRc)."""
    c = chain_case(which)
    P = plan(c.idx, c.k, 1, c.facts.target)
    assert [1 << g for g in P.lg] == c.facts.lists
    assert launch_groups(c.facts.lists) == c.facts.groups
    exp = expected(oracle, c)
    assert max_list_length(exp, P.lg, range(len(P.lg))) <= COMMON.rc
    if which == 4:
        off = exp[2].astype(np.int64)
        assert (off[:11] == 0).all() and (off[11:] == off[11]).all() and off[11] > 100_000
        size = np.diff(c.idx)  # zero bytes; fewer than k bases (and the terminator); all N
        assert (size[[0, 3, 6, 9]] == 0).all() and (0 < size[[1, 4, 7]]).all() and (size[[1, 4, 7]] <= c.k).all()
        assert all((c.data[c.idx[r]:c.idx[r + 1] - 1] == N_BYTE).all() and size[r] > c.k for r in (2, 5, 8))


@pytest.mark.parametrize("kind", TABLE_NS + ("one_pass_of_two", "one_key"))
def test_inputs_table_lists(oracle, kind):
    c = table_case(kind)
    _, h, counts = list0_mirror(oracle, c, COMMON)
    n = int(counts.astype(np.int64).sum())
    assert n == c.facts.n
    if kind == "one_key":
        assert h.size == 1 and n == 4096 and initial_passes(n) == 2
    elif kind == "one_pass_of_two":
        # 8 waves of 512 keys each, every key distinct and in pass 0 of 2: 512 claims > kClaimW
        assert h.size == n == 8 * 512 and initial_passes(n) == 2 and (pass_of(h, 2) == 0).all() and 512 > CLAIM_W
    else:
        assert h.size == n == kind
        assert initial_passes(n) == {2048: 1, 2049: 2, 8192: 4, 8193: 5}[n] and (n <= RES_KEYS) == (kind != 8193)


@pytest.mark.parametrize("nkeys", (16, 100))
def test_inputs_pass_bits(oracle, nkeys):
    c = pass_bits_case(nkeys)
    _, h, counts = list0_mirror(oracle, c, COMMON)
    assert h.size == nkeys and (counts == 1).all()
    bits = np.sort(pass_bits(h))
    if nkeys == 16:
        assert list(bits) == [PASS_PREFIX] * 8 + [PASS_PREFIX + 1] * 8
    else:
        assert (bits == MAX_PASSES - 1).all()


# ---------------------------------------------------------------------------
# GPU: running and comparing
# ---------------------------------------------------------------------------
@pytest.fixture
def diag(kmc):
    """The diagnostic library; leaving the context restores every hook."""
    with kmc.diag() as D:
        yield D


def fallback(D, nrec=1):
    ent, pairs = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
    assert D.kmc_diag_canon_fallback(ctypes.byref(ent), ctypes.byref(pairs)) == 0
    per = (ctypes.c_ulonglong * max(nrec, 1))()
    q3 = (ctypes.c_ulonglong * 3)()
    assert D.kmc_diag_canon_fallback_detail(per, nrec, q3) == 0
    return types.SimpleNamespace(ent=ent.value, pairs=pairs.value, per=list(per)[:nrec], q3=tuple(q3))


def both_paths(kmc, oracle, cuda, D, c, msg, modes=(1, 0)):
    """The case with direct output and (mode 0) through pk and canon_place_kernel,
    each against the oracle (and np_count); returns the oracle's result and the
    direct-output call's read-backs.  A call with direct output off leaves them as
    they were."""
    exp = expected(oracle, c)
    flags = kmc.CANON_FORWARD if c.forward else 0
    nrec = len(c.idx) - 1
    fb = None
    for mode in modes:
        assert D.kmc_diag_canon_direct(mode) == 0
        before = fallback(D, nrec)
        got = run(kmc, cuda, c.data, c.idx, c.k, flags)
        assert_equal(got, exp, "%s direct=%d" % (msg, mode), c.laid_sets)
        after = fallback(D, nrec)
        if mode:
            fb = after
        else:
            assert after == before, "a call with direct output off changed the fallback read-backs"
    assert D.kmc_diag_canon_direct(1) == 0
    return exp, fb


def show(msg, fb, **more):
    print("%s: queued big %d table %d + %d, fallback entries %d pairs %d%s"
          % ((msg,) + fb.q3 + (fb.ent, fb.pairs, "".join(", %s %s" % kv for kv in more.items()))))


def check_one_list(kmc, oracle, cuda, D, c, msg, c_cap=COMMON.cap, b_cap=BIG.cap, want=None):
    """A call whose only list with keys is list 0 of record 0: both paths, the queue
    counts and the fallback copies the mirror gives for that list."""
    exp, fb = both_paths(kmc, oracle, cuda, D, c, msg)
    route, m, q3 = k4_route(feistel(exp[0]), exp[1], c_cap, b_cap)
    if m is None:
        show(msg + " -> " + route, fb, P=initial_passes(int(exp[1].astype(np.int64).sum())))
    else:
        show(msg + " -> " + route, fb, n=m.n, nsk=m.nsk, na=m.na, nres=m.nres, nhot=m.nhot, rcap=m.rcap)
    if want is not None:
        assert route == want, (route, want)
    assert fb.q3 == q3, (fb.q3, q3)
    assert (fb.ent, fb.pairs) == fallback_of(route, m, exp[0].size)
    assert fb.per == [fb.pairs]
    return m, fb


# ---------------------------------------------------------------------------
# A. list length at each instance's cap
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", HOOK_NS)
def test_list_length_at_the_hooked_caps(kmc, oracle, cuda, diag, n):
    """sort_cap(2000), sort_cap_big(3000): lists of 1999 and 2000 keys stay in the
    common instance, 2001 and 3000 go to the big one, 3001 to the table kernel."""
    assert diag.kmc_diag_canon_sort_cap(HOOK_C) == 0 and diag.kmc_diag_canon_sort_cap_big(HOOK_B) == 0
    want = "common" if n <= HOOK_C else "big" if n <= HOOK_B else "table1"
    check_one_list(kmc, oracle, cuda, diag, random_list_case(n), "n=%d" % n, HOOK_C, HOOK_B, want)


@gpu
@pytest.mark.parametrize("k", (31, 5))
@pytest.mark.parametrize("alone", (True, False))
def test_lists_of_no_key_and_one_key(kmc, oracle, cuda, diag, alone, k):
    """A record of exactly k - 1 bases (its list has no key) and one of exactly k
    bases (one key), alone in the call and between ordinary records."""
    for nbases in (k - 1, k):
        c = short_record_case(k, alone, nbases)
        exp, fb = both_paths(kmc, oracle, cuda, diag, c, "k=%d alone=%s bases=%d" % (k, alone, nbases))
        show("k=%d alone=%s %d bases" % (k, alone, nbases), fb)
        r = c.facts.r
        assert int(exp[2][r + 1] - exp[2][r]) == c.facts.windows == nbases - k + 1
        assert fb.q3 == (0, 0, 0)
        if alone:
            assert (fb.ent, fb.pairs) == (0, 0)


@gpu
@pytest.mark.parametrize("n", SHIPPED_NS)
def test_list_length_at_the_shipped_caps(kmc, oracle, cuda, diag, n):
    """List 0 of exactly 6080 keys (common instance), 6081 and 12288 (big instance:
    its last thread's last register holds a key), 12289 (table kernel); no hook."""
    c = shipped_cap_case(n)
    want = {6080: "common", 6081: "big", 12288: "big", 12289: "table1"}[n]
    m, _ = check_one_list(kmc, oracle, cuda, diag, c, "n=%d" % n, want=want)
    assert m is None or m.n == n


# ---------------------------------------------------------------------------
# B. staged results at kRc
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("where", (-1, 0, 1))
@pytest.mark.parametrize("inst_name", ("common", "big"))
def test_results_at_the_stage_capacity(kmc, oracle, cuda, diag, inst_name, where):
    """kRc - 1, kRc and kRc + 1 results (1024 in the common instance, 2048 in the big
    one, forced there with sort_cap(1)) in a list of record 0, whose start is known:
    no copy at or below kRc, exactly one of nres - kRc pairs above it (count 4:
    escaped to pc)."""
    c = staged_case(inst_name, where)
    if inst_name == "big":
        assert diag.kmc_diag_canon_sort_cap(1) == 0
    m, fb = check_one_list(kmc, oracle, cuda, diag, c, "%s nres=kRc%+d" % (inst_name, where),
                           1 if inst_name == "big" else COMMON.cap, want=inst_name)
    assert m.nres == c.facts.inst.rc + where and m.rcap == c.facts.inst.rc
    assert (fb.ent, fb.pairs) == ((1, where) if where > 0 else (0, 0))


# ---------------------------------------------------------------------------
# C. slot population, D. kHotMax
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("inst_name", ("common", "big"))
def test_slots_of_16_17_128_129_keys(kmc, oracle, cuda, diag, inst_name):
    """slot_case: the pairwise dedup with its second tier full, a slot one key past
    it, pivots of 128 and 129 copies, two interleaved pivots."""
    c = slot_case(inst_name)
    if inst_name == "big":
        assert diag.kmc_diag_canon_sort_cap(1) == 0
    m, fb = check_one_list(kmc, oracle, cuda, diag, c, inst_name, 1 if inst_name == "big" else COMMON.cap,
                           want=inst_name)
    assert m.nhot == 4 and (fb.ent, fb.pairs) == (0, 0)


@gpu
@pytest.mark.parametrize("nkeys", (HOT_MAX, HOT_MAX + 1))
@pytest.mark.parametrize("inst_name", ("common", "big"))
def test_crowded_slots_at_khotmax(kmc, oracle, cuda, diag, inst_name, nkeys):
    """128 crowded slots (and one of exactly 16 keys, not crowded) stay in K4s; 129
    send the list to the table kernel's second launch, and all its pairs through
    the fallback copy."""
    c = hot_case(inst_name, nkeys)
    if inst_name == "big":
        assert diag.kmc_diag_canon_sort_cap(1) == 0
    m, fb = check_one_list(kmc, oracle, cuda, diag, c, "%s nhot=%d" % (inst_name, nkeys),
                           1 if inst_name == "big" else COMMON.cap, want=inst_name if nkeys <= HOT_MAX else "table2")
    assert m.nhot == nkeys
    assert (fb.q3[2], fb.ent, fb.pairs) == ((0, 0, 0) if nkeys <= HOT_MAX else (1, 1, nkeys + 1))


# ---------------------------------------------------------------------------
# E. the reservation chain and the launch groups (direct output only)
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", (1, 2, 3, 4))
def test_chain_publishes_every_group_start(kmc, oracle, cuda, diag, which):
    """chain_case: a list copies its pairs through the fallback only when it found
    its record's start unknown (no list here is long enough for any other reason), and
    every list of the first record of a launch group runs after every list of the
    records before it: the chain must have published that record's start.  So the
    records that start a group have 0 fallback pairs -- 1: all three; 2: records 0
    and 2 (record 1 shares record 0's launch: at most its distinct keys); 3: record
    0 and record 8192, the second group, behind 8192 one-list records; 4: the 8192-list
    record behind ten records without a window, and the empty records."""
    c = chain_case(which)
    assert diag.kmc_diag_canon_list_target(c.facts.target) == 0
    exp, fb = both_paths(kmc, oracle, cuda, diag, c, "chain %d" % which, modes=(1,))
    per = np.array(fb.per, dtype=np.int64)
    distinct = np.diff(exp[2].astype(np.int64))
    show("chain %d" % which, fb, groups=c.facts.groups, fallback_records=int((per > 0).sum()),
         first=list(np.flatnonzero(per > 0)[:4]))
    assert fb.q3 == (0, 0, 0) and int(per.sum()) == fb.pairs and (per <= distinct).all()
    assert per[c.facts.zero].sum() == 0, "a record that starts a launch group found its start unpublished"
    if which in (1, 4):
        assert (fb.ent, fb.pairs) == (0, 0)


# ---------------------------------------------------------------------------
# F. table kernel
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", TABLE_NS + ("one_pass_of_two", "one_key"))
def test_table_kernel_pass_and_residency_edges(kmc, oracle, cuda, diag, kind):
    """sort_cap(0), list 0 of 2048 / 2049 keys (P = 1, 2), 8192 / 8193 (held in
    registers, reloaded per pass), 4096 distinct keys of one pass of two (every wave
    claims 512 > kClaimW at the shipped cap: the pass overflows and splits), one
    key 4096 times (the wave queue refilled)."""
    assert diag.kmc_diag_canon_sort_cap(0) == 0
    check_one_list(kmc, oracle, cuda, diag, table_case(kind), "table %s" % kind, 0, 0, want="table1")


@gpu
def test_table_kernel_splits_to_its_last_pass_bit(kmc, oracle, cuda, diag):
    """claim_cap(8): sixteen keys, eight and eight, that part only in the lowest of
    the 17 pass bits: exact at P = 2^17."""
    c = pass_bits_case(16)
    assert table_split(waves_of(16, c.facts.bits), 16, PASS_CAP) == MAX_PASSES
    assert diag.kmc_diag_canon_sort_cap(0) == 0 and diag.kmc_diag_canon_claim_cap(PASS_CAP) == 0
    _, fb = check_one_list(kmc, oracle, cuda, diag, c, "P=2^17", 0, 0, want="table1")
    assert (fb.ent, fb.pairs) == (1, 16)


@gpu
def test_table_kernel_out_of_pass_bits_is_invalid_arg(kmc, oracle, cuda, diag):
    """claim_cap(8): 100 keys that agree on all 17 pass bits cannot be split (the
    guarded kErrPasses path): KMC_ERR_INVALID_ARG, and the next call, an ordinary
    input in the same library-owned workspace, equals the oracle."""
    c = pass_bits_case(100)
    assert table_split(waves_of(100, c.facts.bits), 100, PASS_CAP) is None
    after = random_case(np.random.default_rng(5810), [3000, 1, 700], 21, 4096)
    after.exp = None
    assert diag.kmc_diag_canon_sort_cap(0) == 0 and diag.kmc_diag_canon_claim_cap(PASS_CAP) == 0
    for mode in (1, 0):
        assert diag.kmc_diag_canon_direct(mode) == 0
        with pytest.raises(kmc.KmcError) as ei:
            run(kmc, cuda, c.data, c.idx, c.k, kmc.CANON_FORWARD)
        assert ei.value.code == ERR_INVALID_ARG
        _, fb = both_paths(kmc, oracle, cuda, diag, after, "after kErrPasses, direct=%d" % mode, modes=(mode,))
        if mode:
            show("after kErrPasses", fb)
            assert fb.q3 == (0, 3, 0)


# ---------------------------------------------------------------------------
# G. a list split between the direct write-out and a queued copy
# ---------------------------------------------------------------------------
@gpu
def test_list_split_between_write_out_and_copy_in_record_1(kmc, oracle, cuda, diag):
    """split_copy_case: record 1's start is known (record 0 is a launch group of its
    own), so its list 0 writes its staged pairs in place and queues exactly one copy,
    of the nres - kRc results past the stage; canon_fallback_kernel adds record 1's
    start to the copy's offset."""
    c = split_copy_case()
    assert diag.kmc_diag_canon_list_target(c.facts.target) == 0
    exp, fb = both_paths(kmc, oracle, cuda, diag, c, "split copy", modes=(1,))
    show("split copy", fb, per_record=fb.per, nres=c.facts.nres)
    assert fb.q3 == (0, 0, 0) and fb.per == [0, G_OVER] and (fb.ent, fb.pairs) == (1, G_OVER)
