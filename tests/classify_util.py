"""Host-side model of the per-record source votes (test_classify_gpu.py,
test_classify_cli.py): helpers, no tests, no device.  It extends sketch_match_util.model:

labels(): a dict hash -> bitmask built from the sources' records, one bit per source, for
the k-mers below `limit` (the hash is a bijection of the canonical key, so the dict is
keyed by what the oracle's keys hash to).
model(): the oracle's per-record keys and counts, each key's multiplicity in the set
(a hit) and its mask in the dict, then plain integer counting: score(r, g), the smallest
source with the largest score, that score and the runner-up's.
`limit` is never computed here: it is the device's stats[1]."""
import numpy as np

import sketch_match_util as M
import sketch_screen_util as U
import sketch_util as S
from sketch_screen_util import FWD, SOFT

NONE = 0xFFFFFFFF


def labels(oracle, sources, k, limit, everything, flags=0, seed=S.DEFAULT_SEED):
    """{hash: mask} of the sources [(g, (data, idx)), ...] for the hashes that are sampled."""
    lab = {}
    for g, (data, idx) in sources:
        h, _ = U.mixture_hashes(oracle, data, idx, k, flags, seed)
        for x in h if everything else h[h < np.uint64(limit)]:
            lab[int(x)] = lab.get(int(x), 0) | (1 << g)
    return lab


def model(oracle, data, idx, k, mix, lab, ns, limit, everything, m=1, flags=0, seed=S.DEFAULT_SEED):
    """(windows, sampled, hits, best, best_hits, next_hits: uint32 [n]; scores uint32
    [n, ns]; stats [4]) of the records (data, idx) against the set `mix` labelled `lab`."""
    win, smp, hit, stats = M.model(oracle, data, idx, k, mix, limit, everything, m, flags, seed)
    keys, counts, off = oracle.count_canonical(data, idx, k, soft=bool(flags & SOFT), forward=bool(flags & FWD))
    n = idx.size - 1
    h = S.hash_keys(np.asarray(keys, dtype=np.uint64), seed)
    sampled = np.ones(h.size, bool) if everything else h < np.uint64(limit)
    is_hit = sampled & (U.multiplicities(mix, h) >= max(int(m), 1))
    off = np.asarray(off).astype(np.int64)
    scores = np.zeros((n, ns), dtype=np.int64)
    for r in range(n):
        for e in range(int(off[r]), int(off[r + 1])):
            if is_hit[e]:
                mask = lab.get(int(h[e]), 0)
                for g in range(ns):
                    if (mask >> g) & 1:
                        scores[r, g] += int(counts[e])
    best = np.full(n, NONE, dtype=np.uint32)
    bh = np.zeros(n, dtype=np.uint32)
    nh = np.zeros(n, dtype=np.uint32)
    for r in range(n):
        top = int(scores[r].max())
        if top > 0:
            b = int(np.argmax(scores[r]))  # the first of the largest
            best[r], bh[r] = b, top
            rest = np.delete(scores[r], b)
            nh[r] = int(rest.max()) if rest.size else 0
    return win, smp, hit, best, bh, nh, scores.astype(np.uint32), stats


def host(res):
    """SketchAccum.classify's tensors as (windows, sampled, hits, best, best_hits,
    next_hits: uint32 arrays or None; scores uint32 [n, ns] or None; stats [4] ints or None)."""
    arr = [t.cpu().numpy().view(np.uint32) if t is not None else None for t in res[:7]]
    st = res[7]
    return tuple(arr) + ([int(x) for x in st.cpu().numpy().view(np.uint64)] if st is not None else None,)


NAMES = ("windows", "sampled", "hits", "best", "best_hits", "next_hits", "scores")


def assert_classify(got, exp, msg=""):
    """Every output that was asked for equals the model's, exactly."""
    for name, g, e in zip(NAMES, got[:7], exp[:7]):
        if g is not None:
            np.testing.assert_array_equal(g, e, err_msg="%s %s" % (msg, name))
    if got[7] is not None:
        assert got[7] == exp[7], "%s: stats %s, expected %s" % (msg, got[7], exp[7])


def assert_same(a, b, msg=""):
    """Two results of the device are the same bits."""
    for name, x, y in zip(NAMES, a[:7], b[:7]):
        if x is not None and y is not None:
            np.testing.assert_array_equal(x, y, err_msg="%s %s" % (msg, name))
    if a[7] is not None and b[7] is not None:
        assert a[7] == b[7], msg


def select(listed, best, bh, nh, source, margin):
    """kmc_classify_select's formula (uint32 arithmetic)."""
    lst = np.ones(best.size, bool) if listed is None else listed != 0
    diff = (bh.astype(np.uint32) - nh.astype(np.uint32)).astype(np.uint32)
    return (lst & (best == np.uint32(source)) & (diff >= np.uint32(margin))).astype(np.uint32)


def tsv_lines(file_index, path, got, paths, min_hits=1, min_fraction=0.0, margin=1):
    """(the file's lines of read_sources.tsv, its lines of read_sources_summary.tsv, the
    listed records' assigned source or -1, per record and None when not listed) from the
    model's outputs of all its records; paths: the sources' files."""
    win, smp, hit, best, bh, nh = got[:6]
    ns = len(paths)
    rows, assigned = [], []
    nbest, nass, none, nobest = [0] * ns, [0] * ns, 0, 0
    for r in range(hit.size):
        if not (int(hit[r]) >= min_hits and float(int(hit[r])) >= min_fraction * float(int(smp[r]))):
            assigned.append(None)
            continue
        b = int(best[r])
        src = "-" if b == NONE else str(b)
        rows.append("%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d" % (file_index, r, int(win[r]), int(smp[r]), int(hit[r]), src,
                                                        int(bh[r]), int(nh[r])))
        if b != NONE:
            nbest[b] += 1
        else:
            nobest += 1
        if b != NONE and int(bh[r]) - int(nh[r]) >= margin:
            nass[b] += 1
            assigned.append(b)
        else:
            none += 1
            assigned.append(-1)
    lines = ["%d\t%d\t%s\t%d\t%d" % (file_index, g, paths[g], nbest[g], nass[g]) for g in range(ns)]
    lines.append("%d\t-\t-\t%d\t%d" % (file_index, nobest, none))
    return rows, lines, assigned
