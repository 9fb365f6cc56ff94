"""Host-side model of the per-record match against the abundance accumulator
(test_sketch_match_gpu.py, test_sketch_match_cli.py): helpers, no tests, no device.

model(): the expected windows, sampled, hits and stats of kmc_match_from_accum from the
oracle's per-record keys and counts (oracle.count_canonical), their hashes
(sketch_util.hash_keys) and the set, which is sketch_screen_util.mixture_hashes of what
was added.  `limit` is never computed here: it is the device's stats[1], which
spectrum_util.check_limit holds against the level's bound."""
import numpy as np

import sketch_screen_util as U
import sketch_util as S
from sketch_screen_util import FWD, SOFT

FILL = int(S.FILL)


def model(oracle, data, idx, k, mix, limit, everything, M=1, flags=0, seed=S.DEFAULT_SEED):
    """(windows, sampled, hits: uint32 [n]; stats [4] as Python ints) of the records
    (data, idx) against the set `mix` = (hashes ascending, counts)."""
    keys, counts, off = oracle.count_canonical(data, idx, k, soft=bool(flags & SOFT), forward=bool(flags & FWD))
    n = idx.size - 1
    c = np.asarray(counts).astype(np.int64)
    h = S.hash_keys(np.asarray(keys, dtype=np.uint64), seed)
    rec = np.repeat(np.arange(n), np.diff(np.asarray(off).astype(np.int64)))
    smp = np.ones(h.size, bool) if everything else h < np.uint64(limit)
    hit = smp & (U.multiplicities(mix, h) >= max(int(M), 1))
    out = []
    for sel in (np.ones(h.size, bool), smp, hit):
        v = np.zeros(n, dtype=np.int64)
        np.add.at(v, rec[sel], c[sel])
        out.append(v)
    stats = [1 if everything else 0, int(limit), int(out[1].sum()), int(out[2].sum())]
    return tuple((v & 0xFFFFFFFF).astype(np.uint32) for v in out) + (stats,)


def host(res):
    """SketchAccum.match's tensors as (windows, sampled, hits: uint32 arrays or None,
    stats: [4] Python ints or None)."""
    win, smp, hit, st = res
    arr = [t.cpu().numpy().view(np.uint32) if t is not None else None for t in (win, smp, hit)]
    return tuple(arr) + ([int(x) for x in st.cpu().numpy().view(np.uint64)] if st is not None else None,)


def assert_match(got, exp, msg=""):
    """Every output that was asked for equals the model's, exactly."""
    for name, g, e in zip(("windows", "sampled", "hits"), got[:3], exp[:3]):
        if g is not None:
            np.testing.assert_array_equal(g, e, err_msg="%s %s" % (msg, name))
    if got[3] is not None:
        assert got[3] == exp[3], "%s: stats %s, expected %s" % (msg, got[3], exp[3])


def tsv_lines(file_index, path, got, min_hits=1, min_fraction=0.0):
    """(the file's lines of read_matches.tsv, its line of read_matches_summary.tsv) from
    the (windows, sampled, hits, stats) of all its records."""
    win, smp, hit, stats = got
    rows = []
    for r in range(hit.size):
        if int(hit[r]) >= min_hits and float(int(hit[r])) >= min_fraction * float(int(smp[r])):
            rows.append("%d\t%d\t%d\t%d\t%d" % (file_index, r, int(win[r]), int(smp[r]), int(hit[r])))
    line = "\t".join(str(x) for x in (file_index, path, hit.size, len(rows), stats[1], stats[0], stats[2], stats[3]))
    return rows, line
