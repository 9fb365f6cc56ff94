"""Host-side expectations shared by the sparse pairwise-distance tests
(test_sparse_dist_gpu.py, test_sparse_dist_cli.py): plain numpy, no device."""
import numpy as np


def pair_sums(keys, counts, off, n):
    """Exact S_ij (uint64) in packed-triangle order from per-record lists with
    distinct keys per record: S_ij = sum over shared keys of min(c_i, c_j)."""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts).astype(np.uint64)
    off = np.asarray(off).astype(np.int64)
    recs = []
    for s in range(n):
        a, b = int(off[s]), int(off[s + 1])
        o = np.argsort(keys[a:b], kind="stable")
        recs.append((keys[a:b][o], counts[a:b][o]))
    out = np.zeros(n * (n - 1) // 2, dtype=np.uint64)
    q = 0
    for i in range(n):
        for j in range(i + 1, n):
            _, ia, ib = np.intersect1d(recs[i][0], recs[j][0], assume_unique=True, return_indices=True)
            out[q] = np.minimum(recs[i][1][ia], recs[j][1][ib]).sum(dtype=np.uint64)
            q += 1
    return out


def distances_from_sums(S, lens, k):
    """float32(1) - float32(S) / float32(min(len_i, len_j) - k + 1), packed triangle."""
    lens = np.asarray(lens, dtype=np.int64)
    n = lens.size
    i, j = np.triu_indices(n, 1)  # row-major: the packed triangle's order
    den = (np.minimum(lens[i], lens[j]) - k + 1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(1) - np.asarray(S, dtype=np.uint64).astype(np.float32) / den


def shuffle_within_records(rng, keys, counts, off):
    keys, counts = keys.copy(), counts.copy()
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        o = rng.permutation(b - a)
        keys[a:b], counts[a:b] = keys[a:b][o], counts[a:b][o]
    return keys, counts


def lists_from_dense(rng, dense):
    """Per-record lists of the non-zero bins of a (bins, n) matrix: key = bin
    index, count = bin value, order shuffled within each record."""
    nb, n = dense.shape
    keys, counts, off = [], [], [0]
    for s in range(n):
        code = np.nonzero(dense[:, s])[0]
        keys.append(code.astype(np.uint64))
        counts.append(dense[code, s].astype(np.uint32))
        off.append(off[-1] + code.size)
    keys = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
    counts = np.concatenate(counts) if counts else np.zeros(0, np.uint32)
    off = np.asarray(off, dtype=np.uint64)
    keys, counts = shuffle_within_records(rng, keys, counts, off)
    return keys, counts, off


def lists_from_triplets(rng, code, rec, count, n):
    """The same lists from (code, record, count) triplets of the non-zero bins."""
    code, rec, count = np.asarray(code), np.asarray(rec), np.asarray(count)
    nz = count != 0
    code, rec, count = code[nz], rec[nz], count[nz]
    o = np.argsort(rec, kind="stable")
    keys = code[o].astype(np.uint64)
    counts = count[o].astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(np.bincount(rec, minlength=n)[:n])]).astype(np.uint64)
    keys, counts = shuffle_within_records(rng, keys, counts, off)
    return keys, counts, off


def canonical_expected(oracle, data, idx, k, soft=False, forward=False):
    """Distances of the host canonical oracle's counts (exact S, numpy)."""
    keys, counts, off = oracle.count_canonical(data, idx, k, soft=soft, forward=forward)
    n = idx.size - 1
    return distances_from_sums(pair_sums(keys, counts, off, n), np.diff(idx) - 1, k)
