"""Host-side oracle of the sketch search (test_sketch_query_gpu.py): the query x
reference rectangle by the union / intersect rule of sketch_util.distances_expected,
and the nearest references ordered on the integers with fractions.Fraction.  Plain
numpy, no device."""
from fractions import Fraction

import numpy as np

import sketch_util as S

NO_REF = np.uint32(0xFFFFFFFF)


def pair_counts(a, b, s):
    """(shared, denom) of two ascending rows: U = the s smallest of a u b, shared = |U n a n b|."""
    u = np.union1d(a, b)[:s]
    both = np.intersect1d(a, b, assume_unique=True)
    return np.intersect1d(u, both, assume_unique=True).size, u.size


def row_sets(rows, sizes, s):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, s)
    return [rows[r, :min(int(sizes[r]), s)] for r in range(rows.shape[0])]


def rect_expected(qrows, qsizes, rrows, rsizes, s, k):
    """(out float32, shared uint32, denom uint32), each [m, n]."""
    qa, ra = row_sets(qrows, qsizes, s), row_sets(rrows, rsizes, s)
    m, n = len(qa), len(ra)
    out = np.zeros((m, n), dtype=np.float32)
    shared = np.zeros((m, n), dtype=np.uint32)
    denom = np.zeros((m, n), dtype=np.uint32)
    for i in range(m):
        for j in range(n):
            sh, dn = pair_counts(qa[i], ra[j], s)
            shared[i, j], denom[i, j] = sh, dn
            out[i, j] = S.mash_formula(sh, dn, k)
    return out, shared, denom


def ranking(shared, denom, min_shared):
    """The participating references of one query (its rows of the rectangle), best first."""
    part = [r for r in range(shared.size) if denom[r] > 0 and shared[r] >= min_shared]
    return sorted(part, key=lambda r: (-Fraction(int(shared[r]), int(denom[r])), r))


def nearest_expected(rect, top, min_shared):
    """(refs uint32, shared uint32, denom uint32, dist float32, each [m, top]; counts
    uint32 [m]) from rect_expected's triple, the unused slots filled."""
    out, shared, denom = rect
    m = out.shape[0]
    refs = np.full((m, top), NO_REF, dtype=np.uint32)
    sh = np.zeros((m, top), dtype=np.uint32)
    dn = np.zeros((m, top), dtype=np.uint32)
    dist = np.full((m, top), np.nan, dtype=np.float32)
    counts = np.zeros(m, dtype=np.uint32)
    for q in range(m):
        best = ranking(shared[q], denom[q], min_shared)[:top]
        c = len(best)
        counts[q] = c
        refs[q, :c] = best
        sh[q, :c] = shared[q, best]
        dn[q, :c] = denom[q, best]
        dist[q, :c] = out[q, best]
    return refs, sh, dn, dist, counts


def pack(lists, s):
    """(rows uint64 [n, s], sizes uint32 [n]) of ascending value lists, FILL after each."""
    rows = np.full((len(lists), s), S.FILL, dtype=np.uint64)
    sizes = np.zeros(len(lists), dtype=np.uint32)
    for r, v in enumerate(lists):
        v = np.sort(np.asarray(v, dtype=np.uint64))
        assert v.size <= s and np.unique(v).size == v.size
        rows[r, :v.size] = v
        sizes[r] = v.size
    return rows, sizes
