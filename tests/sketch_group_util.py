"""Host-side expectation of the grouped sketches (test_sketch_group_gpu.py,
test_sketch_group_cli.py): per record the canonical oracle's distinct keys
(oracle.count_canonical), per group np.unique of its records' keys, then
sketch_util.sketch_expected over the group offsets.  Plain numpy, no device."""
import numpy as np

import sketch_util as S

SOFT, FWD = 1, 2


def clamp_offsets(group_offsets, n):
    return np.clip(np.asarray(group_offsets, dtype=np.int64), 0, n)


def grouped_expected(oracle, data, idx, group_offsets, k, s, flags=0, seed=S.DEFAULT_SEED):
    """(rows uint64 [groups, s], sizes uint32 [groups]) of the groups
    [group_offsets[g], group_offsets[g+1]) of the records of (data, idx); offsets are
    clamped to the record count, a descending pair is an empty group."""
    n = idx.size - 1
    ek, _, eo = oracle.count_canonical(data, idx, k, soft=bool(flags & SOFT), forward=bool(flags & FWD))
    ek = np.asarray(ek, dtype=np.uint64)
    eo = np.asarray(eo).astype(np.int64)
    go = clamp_offsets(group_offsets, n)
    keys, off = [], [0]
    for g in range(go.size - 1):
        a, b = int(go[g]), int(go[g + 1])
        u = np.unique(ek[eo[a]:eo[b]]) if b > a else np.zeros(0, np.uint64)
        keys.append(u)
        off.append(off[-1] + u.size)
    keys = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
    return S.sketch_expected(keys, None, np.asarray(off, dtype=np.uint64), go.size - 1, s, seed)


def merged_expected(rows, sizes, group_offsets, s):
    """Bottom-s of the union of the sketch rows of every group (kmc_sketch_merge_groups)."""
    rows = np.asarray(rows, dtype=np.uint64)
    go = clamp_offsets(group_offsets, rows.shape[0])
    out = np.full((go.size - 1, s), S.FILL, dtype=np.uint64)
    osz = np.zeros(go.size - 1, dtype=np.uint32)
    for g in range(go.size - 1):
        a, b = int(go[g]), int(go[g + 1])
        parts = [rows[r, :min(int(sizes[r]), s)] for r in range(a, b)]
        u = np.unique(np.concatenate(parts))[:s] if parts else np.zeros(0, np.uint64)
        out[g, :u.size] = u
        osz[g] = u.size
    return out, osz
