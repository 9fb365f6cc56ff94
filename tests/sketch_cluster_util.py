"""Host-side oracle of kmc_sketch_cluster (test_sketch_cluster_gpu.py): the pairs'
shared and denom by the union / intersect rule of sketch_util.distances_expected,
the link rule in float64, a plain union-find, and labels as the component minimum.
Plain numpy, no device.  After it, the row builders the GPU tests share."""
import numpy as np

import sketch_query_util as Q
import sketch_util as S


def links(shared, denom, min_jaccard, size_i=None, size_j=None):
    """The link rule on arrays of counts: denom > 0 and float64(shared) >= min_jaccard *
    float64(denom), and neither row empty when the pairs' row sizes are given (an empty
    row has shared 0 of denom > 0 with a row that is not, which min_jaccard == 0 alone
    would accept: an empty row is a singleton at every threshold)."""
    shared, denom = np.asarray(shared), np.asarray(denom)
    on = (denom > 0) & (shared.astype(np.float64) >= np.float64(min_jaccard) * denom.astype(np.float64))
    if size_i is not None:
        on &= (np.asarray(size_i) > 0) & (np.asarray(size_j) > 0)
    return on


def components(n, pairs):
    """(labels uint32 [n], index uint32 [n], count) of the graph on n records with the
    edges `pairs`: the smallest index of each record's component, that component's
    rank among all components ordered by it, and the number of components."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in pairs:
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    roots = np.array([find(x) for x in range(n)], dtype=np.int64)
    low = np.full(n, n, dtype=np.int64)
    np.minimum.at(low, roots, np.arange(n))
    labels = low[roots] if n else roots
    reps = np.unique(labels)
    index = np.searchsorted(reps, labels)
    return labels.astype(np.uint32), index.astype(np.uint32), int(reps.size)


def triangle_pairs(n):
    """(i, j) of the packed upper triangle, in its order."""
    return np.triu_indices(n, 1)


def cluster_from_counts(sizes, shared, denom, min_jaccard):
    """The clusters of the packed triangle's counts of rows with these sizes."""
    sizes = np.asarray(sizes)
    n = sizes.size
    i, j = triangle_pairs(n)
    on = links(shared, denom, min_jaccard, sizes[i], sizes[j])
    return components(n, zip(i[on], j[on]))


def pair_counts_packed(rows, sizes, s):
    """(shared uint32, denom uint32) over the packed upper triangle by the merge rule of
    sketch_util.distances_expected (U = the s smallest of A u B, denom = |U|, shared =
    |U n A n B|), all pairs at once: the two rows of a pair are sorted together, a value
    of both rows shows as an equal neighbour, and a value's rank among the distinct ones
    says whether it is in U.  For rows whose values are below FILL (the tests' are).
    test_sketch_cluster_args.py holds it against distances_expected."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, s)
    n = rows.shape[0]
    sz = np.minimum(np.asarray(sizes).astype(np.int64), s)
    real = np.arange(s)[None, :] < sz[:, None]
    assert not (rows[real] == S.FILL).any()
    vals = np.where(real, rows, S.FILL)
    shared = np.zeros(n * (n - 1) // 2, dtype=np.uint32)
    denom = np.zeros_like(shared)
    i, j = triangle_pairs(n)
    step = max(1, (1 << 22) // (2 * s))  # pairs per block: 32 MB of values
    for at in range(0, i.size, step):
        a, b = i[at:at + step], j[at:at + step]
        both = np.sort(np.concatenate([vals[a], vals[b]], axis=1), axis=1)
        present = both != S.FILL
        twin = np.zeros_like(present)
        twin[:, 1:] = (both[:, 1:] == both[:, :-1]) & present[:, 1:]
        rank = np.cumsum(present & ~twin, axis=1)  # of a value among the distinct ones, from 1
        shared[at:at + step] = (twin & (rank <= s)).sum(axis=1)
        denom[at:at + step] = np.minimum(rank[:, -1], s)
    return shared, denom


def cluster_expected(rows, sizes, s, min_jaccard):
    """(labels, index, count) of sketch rows [n, s] with their sizes."""
    n = np.asarray(rows).reshape(-1, s).shape[0]
    shared, denom = pair_counts_packed(rows, sizes, s)
    return cluster_from_counts(np.asarray(sizes)[:n], shared, denom, min_jaccard)


# row builders ----------------------------------------------------------------------------
class Values:
    """Distinct random uint64 values, handed out in runs that never repeat."""

    def __init__(self, seed, count):
        rng = np.random.default_rng(seed)
        v = np.unique(rng.integers(1, (1 << 64) - 1, size=count + 64, dtype=np.uint64))
        self.v = rng.permutation(v)[:count]
        self.at = 0

    def take(self, m):
        assert self.at + m <= self.v.size
        out = self.v[self.at:self.at + m]
        self.at += m
        return out


def place(lists, order, n, s):
    """Q.pack of n rows: lists[t] becomes row order[t]; the rows not named are empty."""
    rows = [[] for _ in range(n)]
    for t, v in zip(order, lists):
        rows[int(t)] = v
    return Q.pack(rows, s)


def chain_lists(vals, length, s, keep):
    """`length` full rows of s values; neighbours share `keep` values, rows two apart
    s - 2 (s - keep) at the most (none when keep <= s / 2)."""
    step = s - keep
    pool = vals.take(s + step * (length - 1))
    return [pool[t * step:t * step + s] for t in range(length)]
