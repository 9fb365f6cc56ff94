"""Host-side oracle of kmc_sketch_links and kmc_sketch_links_rect
(test_sketch_links_gpu.py): the pair counts of a query x reference rectangle by the merge
rule of sketch_cluster_util.pair_counts_packed, and the listed pairs of either shape as
sorted tables of (i, j, shared, denom).  Plain numpy, no device.
test_sketch_links_args.py holds the counts against sketch_util.distances_expected."""
import numpy as np

import sketch_cluster_util as C
import sketch_util as S


def _values(rows, sizes, s):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, s)
    sz = np.minimum(np.asarray(sizes).astype(np.int64), s)
    real = np.arange(s)[None, :] < sz[:, None]
    assert not (rows[real] == S.FILL).any()
    return np.where(real, rows, S.FILL)


def pair_counts_rect(qrows, qsizes, rrows, rsizes, s):
    """(shared uint32 [m, n], denom uint32 [m, n]) of every query row against every
    reference row: U = the s smallest of A u B, denom = |U|, shared = |U n A n B|, all
    pairs at once as pair_counts_packed does it (the two rows sorted together, a value
    of both shows as an equal neighbour, its rank among the distinct values says
    whether it is in U).  For rows whose values are below FILL."""
    q, r = _values(qrows, qsizes, s), _values(rrows, rsizes, s)
    m, n = q.shape[0], r.shape[0]
    shared = np.zeros(m * n, dtype=np.uint32)
    denom = np.zeros_like(shared)
    i, j = np.divmod(np.arange(m * n), max(n, 1))
    step = max(1, (1 << 22) // (2 * s))
    for at in range(0, i.size, step):
        a, b = i[at:at + step], j[at:at + step]
        both = np.sort(np.concatenate([q[a], r[b]], axis=1), axis=1)
        present = both != S.FILL
        twin = np.zeros_like(present)
        twin[:, 1:] = (both[:, 1:] == both[:, :-1]) & present[:, 1:]
        rank = np.cumsum(present & ~twin, axis=1)
        shared[at:at + step] = (twin & (rank <= s)).sum(axis=1)
        denom[at:at + step] = np.minimum(rank[:, -1], s)
    return shared.reshape(m, n), denom.reshape(m, n)


def table(i, j, shared, denom):
    """uint32 [L, 4] of (i, j, shared, denom), sorted by (i, j)."""
    t = np.stack([np.asarray(x).astype(np.uint32) for x in (i, j, shared, denom)], axis=1).reshape(-1, 4)
    return t[np.lexsort((t[:, 1], t[:, 0]))]


def links_from_counts(sizes, shared, denom, min_jaccard):
    """The listed pairs i < j of the packed triangle's counts of rows with these sizes."""
    sizes = np.asarray(sizes)
    i, j = C.triangle_pairs(sizes.size)
    on = C.links(shared, denom, min_jaccard, sizes[i], sizes[j])
    return table(i[on], j[on], np.asarray(shared)[on], np.asarray(denom)[on])


def links_expected(rows, sizes, s, min_jaccard):
    """kmc_sketch_links' set of sketch rows [n, s] with their sizes, as a table."""
    shared, denom = C.pair_counts_packed(rows, sizes, s)
    return links_from_counts(np.asarray(sizes)[:np.asarray(rows).reshape(-1, s).shape[0]], shared, denom, min_jaccard)


def rect_links_from_counts(qsizes, rsizes, shared, denom, min_jaccard):
    """The listed pairs of the rectangle's counts [m, n]."""
    shared, denom = np.asarray(shared), np.asarray(denom)
    m, n = shared.shape
    qi, rj = np.divmod(np.arange(m * n), max(n, 1))
    on = C.links(shared.reshape(-1), denom.reshape(-1), min_jaccard, np.asarray(qsizes)[qi], np.asarray(rsizes)[rj])
    return table(qi[on], rj[on], shared.reshape(-1)[on], denom.reshape(-1)[on])


def rect_links_expected(qrows, qsizes, rrows, rsizes, s, min_jaccard):
    """kmc_sketch_links_rect's set as a table."""
    shared, denom = pair_counts_rect(qrows, qsizes, rrows, rsizes, s)
    return rect_links_from_counts(qsizes, rsizes, shared, denom, min_jaccard)


def tri_index(i, j, n):
    """Where the pair i < j stands in the packed upper triangle of n rows."""
    i, j = np.asarray(i).astype(np.int64), np.asarray(j).astype(np.int64)
    return i * n - i * (i + 1) // 2 + (j - i - 1)
