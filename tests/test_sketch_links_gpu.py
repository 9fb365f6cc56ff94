"""GPU parity of kmc_sketch_links and kmc_sketch_links_rect against the numpy oracle of
tests/sketch_links_util.py, against the triangle and the rectangle of distances bit for
bit, and against the clustering.  Every case runs in libkmc.so and in libkmc_diag.so,
whose distance tiles (512 staged values, at most 4 rows) put a few records through many
tiles and whose LDS buffer of a tile's pairs holds 16 entries:

    build  s     path                n
    diag   64    staged, T = 4       3, 4, 5, 11, 37
    diag   128   rows in global      10
    ship   64    staged, T = 32      31, 32, 33, 67, 70
    ship   4096  rows in global      10

The order of the entries is unspecified: every comparison sorts by (i, j) first, or goes
through kmc.sketch_links' capacity=None form, which does.  The structures are those of
test_sketch_cluster_gpu.py.
"""
import numpy as np
import pytest

import sketch_cluster_util as C
import sketch_links_util as L
import sketch_query_util as Q
import sketch_util as S
import stream_util as T
from sketch_util import dev, which

pytestmark = pytest.mark.gpu

LIBS = ["ship", "diag"]
cached = S.cache()
K = 21
POISON32 = 0x5A5A5A5A

SHAPES = [("diag", 64, n) for n in (3, 4, 5, 11, 37)] + [("diag", 128, 10)] + \
         [("ship", 64, n) for n in (31, 32, 33, 67, 70)] + [("ship", 4096, 10)]


def dev_rows(rows, sizes, cuda):
    return dev(rows.view(np.int64), cuda), dev(sizes.view(np.int32), cuda)


def u32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def listed(out):
    """(table uint32 [L, 4] sorted by (i, j), dist as uint32 bit patterns in that order, num_links)
    of a wrapper's triple whose first num_links entries are written."""
    links, dist, count = out
    n = int(count.cpu().numpy()[0])
    t = u32(links).reshape(-1, 4)[:n]
    order = np.lexsort((t[:, 1], t[:, 0]))
    return t[order], None if dist is None else u32(dist)[:n][order], n


def gpu_links(kmc, cuda, rows, sizes, mj, **kw):
    import torch
    out = kmc.sketch_links(*dev_rows(rows, sizes, cuda), K, mj, **kw)
    torch.cuda.synchronize()
    return listed(out)


def assert_table(got, exp, msg):
    table, _, count = got
    assert count == exp.shape[0], "%s num_links %d, expected %d" % (msg, count, exp.shape[0])
    np.testing.assert_array_equal(table, exp, err_msg="%s entries" % msg)


# 1. the set of pairs: structures x shapes ----------------------------------------------------
def order_with(rng, n, fixed):
    """A permutation of 0..n-1 (chain position -> record) with order[t] = r for (t, r) in fixed."""
    rest = [r for r in rng.permutation(n).tolist() if r not in fixed.values()]
    return [fixed[t] if t in fixed else rest.pop() for t in range(n)]


def chain(rng, vals, n, s):
    """Only neighbours share values (half a row): n - 1 links."""
    order = order_with(rng, n, {n // 2: 0})
    return C.place(C.chain_lists(vals, n, s, s // 2), order, n, s) + (0.1,)


def star(rng, vals, n, s):
    """Every leaf holds an eighth of the centre's values and nothing else: shared = s / 8 of
    denom = s, the rule's boundary at 0.125 (exact in double).  The centre is the last record."""
    centre = vals.take(s)
    lists = [centre] + [rng.choice(centre, size=s // 8, replace=False) for _ in range(n - 1)]
    return C.place(lists, [n - 1] + list(range(n - 1)), n, s) + (0.125,)


def bridge(rng, vals, n, s):
    """Two chains joined by the one pair (n - 2, n - 1), the last pair of the last tile."""
    order = order_with(rng, n, {n // 2 - 1: n - 2, n // 2: n - 1})
    return C.place(C.chain_lists(vals, n, s, s // 2), order, n, s) + (0.1,)


def singletons(rng, vals, n, s):
    """No pair shares a value: L = 0, nothing is written."""
    return Q.pack([vals.take(int(rng.integers(1, s + 1))) for _ in range(n)], s) + (1.0 / 16384,)


def identical(rng, vals, n, s):
    """min_jaccard = 1 on copies of one row lists every pair: every tile's LDS buffer is full."""
    return Q.pack([vals.take(s)] * n, s) + (1.0,)


def empties(rng, vals, n, s):
    """min_jaccard = 0 lists every pair of rows that are not empty, whatever they share, and
    no pair of an empty row (the first and the last record), whose shared 0 of denom > 0
    would pass the product rule."""
    pool = vals.take(2 * s)
    empty = {0, n - 1} if n > 3 else {0}
    lists = [[] if r in empty else rng.choice(pool, size=int(rng.integers(1, s + 1)), replace=False) for r in range(n)]
    return Q.pack(lists, s) + (0.0,)


def exact(rng, vals, n, s):
    """min_jaccard = 1 lists only shared == denom: copies of a full row and copies of a short
    row; a copy with one value replaced pairs with nothing."""
    g = max(1, n // 3)
    bases = [vals.take(s if b % 2 == 0 else s // 2) for b in range(g)]
    lists = []
    for r in range(n):
        v = bases[r % g].copy()
        if r // g == 2:
            v[int(rng.integers(0, v.size))] = vals.take(1)[0]
        lists.append(v)
    return C.place(lists, rng.permutation(n).tolist(), n, s) + (1.0,)


def overlap(rng, vals, n, s):
    """stream_util.overlap_rows: rows of random size out of one pool, one of them empty."""
    return T.overlap_rows(4100 + n, n, s) + (0.3,)


STRUCTURES = {"chain": chain, "star": star, "bridge": bridge, "singletons": singletons, "identical": identical,
              "empties": empties, "exact": exact}


def structure_case(name, n, s):
    def make():
        seed = 1000 * n + s + 7 * (list(STRUCTURES).index(name) if name in STRUCTURES else 11)
        rng = np.random.default_rng(seed)
        rows, sizes, mj = (STRUCTURES.get(name) or overlap)(rng, C.Values(seed + 1, (n + 2) * s + n), n, s)
        exp = L.links_expected(rows, sizes, s, mj)
        pairs = n * (n - 1) // 2
        if name == "identical":
            assert exp.shape[0] == pairs
        elif name == "singletons":
            assert exp.shape[0] == 0
        else:
            assert 1 <= exp.shape[0] < pairs, "%s n=%d s=%d: %d of %d pairs listed" % (name, n, s, exp.shape[0], pairs)
        return rows, sizes, mj, exp
    return cached((name, n, s), make)


@pytest.mark.parametrize("name", list(STRUCTURES))
@pytest.mark.parametrize("lib,s,n", SHAPES)
def test_structures(kmc, cuda, lib, s, n, name):
    rows, sizes, mj, exp = structure_case(name, n, s)
    with which(kmc, lib):
        assert_table(gpu_links(kmc, cuda, rows, sizes, mj), exp, "%s %s n=%d s=%d" % (name, lib, n, s))


@pytest.mark.parametrize("lib", LIBS)
def test_overlapping_rows(kmc, cuda, lib):
    rows, sizes, mj, exp = structure_case("overlap", 37, 64)
    with which(kmc, lib):
        assert_table(gpu_links(kmc, cuda, rows, sizes, mj), exp, lib)


# 2. equal to the triangle, bit for bit -----------------------------------------------------------
def triangle_of(kmc, cuda, rows, sizes):
    """(out as uint32 bit patterns, shared, denom) of kmc_sketch_distances."""
    import torch
    out, sh, dn = kmc.sketch_distances(*dev_rows(rows, sizes, cuda), K, with_counts=True)
    torch.cuda.synchronize()
    return u32(out), u32(sh), u32(dn)


@pytest.mark.parametrize("lib,name,n,s", [("diag", "overlap", 37, 64), ("diag", "chain", 10, 128), ("diag", "exact", 11, 64),
                                          ("ship", "overlap", 37, 64), ("ship", "star", 70, 64), ("ship", "chain", 10, 4096)])
def test_entries_are_the_triangles(kmc, cuda, lib, name, n, s):
    """The pairs of kmc.sketch_distances(with_counts=True) that pass the rule on the host are
    the listed set, and every entry's shared, denom and dist are the triangle's at
    tri_index(i, j), the float compared as its bit pattern."""
    rows, sizes, mj, _ = structure_case(name, n, s)
    with which(kmc, lib):
        out, sh, dn = triangle_of(kmc, cuda, rows, sizes)
        table, dist, count = gpu_links(kmc, cuda, rows, sizes, mj)
    exp = L.links_from_counts(sizes, sh, dn, mj)
    assert 0 < exp.shape[0] < n * (n - 1) // 2
    assert_table((table, dist, count), exp, lib)
    at = L.tri_index(table[:, 0], table[:, 1], n)
    np.testing.assert_array_equal(table[:, 2], sh[at])
    np.testing.assert_array_equal(table[:, 3], dn[at])
    np.testing.assert_array_equal(dist, out[at])


# 3. consistent with the clustering -----------------------------------------------------------------
@pytest.mark.parametrize("lib,name,n", [("diag", "overlap", 37), ("diag", "bridge", 37), ("diag", "exact", 11),
                                        ("ship", "overlap", 37), ("ship", "bridge", 70), ("ship", "star", 67)])
def test_components_of_the_list_are_the_clusters(kmc, cuda, lib, name, n):
    import torch
    rows, sizes, mj, _ = structure_case(name, n, 64)
    with which(kmc, lib):
        table, _, _ = gpu_links(kmc, cuda, rows, sizes, mj)
        labels, index, count = kmc.sketch_cluster(*dev_rows(rows, sizes, cuda), mj)
        torch.cuda.synchronize()
    exp = C.components(n, table[:, :2].tolist())
    np.testing.assert_array_equal(u32(labels), exp[0])
    np.testing.assert_array_equal(u32(index), exp[1])
    assert u32(count).tolist() == [exp[2]]


# 4. the rule's boundary ----------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_boundary_of_the_rule(kmc, cuda, lib):
    """Rows 1 and 3 hold 64 values each and share the 32 smallest; the 64 smallest of their
    union are row 1: shared 32 of denom 64.  0.5 * 64 == 32 lists the pair; the next double
    above 0.5 does not."""
    s = 64
    v = np.sort(C.Values(11, 4 * s).take(4 * s))
    lists = [v[2 * s:3 * s], v[:s], v[3 * s:4 * s], np.concatenate([v[:32], v[s:s + 32]])]
    rows, sizes = Q.pack(lists, s)
    sh, dn = C.pair_counts_packed(rows, sizes, s)
    assert (sh[4], dn[4]) == (32, 64) and sh.sum() == 32  # pair (1, 3) of the packed triangle
    above = float(np.nextafter(0.5, 1))
    with which(kmc, lib):
        for mj, exp in ((0.5, [[1, 3, 32, 64]]), (above, [])):
            assert L.links_expected(rows, sizes, s, mj).tolist() == exp
            table, _, count = gpu_links(kmc, cuda, rows, sizes, mj)
            assert table.tolist() == exp and count == len(exp), "min_jaccard=%r" % mj


# 5. capacity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib,name,n", [("diag", "identical", 11), ("ship", "chain", 70)])
def test_capacity(kmc, cuda, lib, name, n):
    """num_links is L whatever the capacity; exactly min(L, capacity) entries are written, at
    the front, distinct and of the listed set with its counts and the triangle's float;
    nothing is written from `capacity` on.  Each call runs twice on the same outputs: the
    second finds the first one's entries and count there.  diag: 55 pairs of 11 copies of one
    row, every tile's buffer full and the capacities inside a tile's block; ship: the 69 links
    of a chain, spread over the tiles of 70 records."""
    import torch
    rows, sizes, mj, exp = structure_case(name, n, 64)
    total = exp.shape[0]
    assert total >= 40
    d = dev_rows(rows, sizes, cuda)
    with which(kmc, lib):
        out, _, _ = triangle_of(kmc, cuda, rows, sizes)
        known = {(int(i), int(j)): (int(a), int(b), int(out[L.tri_index(i, j, n)])) for i, j, a, b in exp}
        for cap in (0, 1, total - 1, total, total + 7):
            links = torch.full((cap + 8, 4), POISON32, dtype=torch.int32, device=cuda)
            dist = torch.full((cap + 8,), POISON32, dtype=torch.int32, device=cuda).view(torch.float32)
            count = torch.full((1,), POISON32, dtype=torch.int64, device=cuda)
            for _ in range(2):
                got = kmc.sketch_links(*d, K, mj, capacity=cap, out=(links, dist, count) if cap else (None, None, count))
                torch.cuda.synchronize()
                assert (got[0] is None and got[1] is None) if cap == 0 else (got[0] is links and got[1] is dist)
                assert count.tolist() == [total], "capacity %d" % cap
                t, f = u32(links).reshape(-1, 4), u32(dist)
                written = (t != POISON32).any(axis=1)
                keep = min(total, cap)
                assert written[:keep].all() and not written[keep:].any(), "capacity %d: entries %s" % (cap, np.nonzero(written)[0])
                assert (f[keep:] == POISON32).all() and (t[keep:] == POISON32).all(), "capacity %d" % cap
                pairs = [tuple(r) for r in t[:keep, :2].tolist()]
                assert len(set(pairs)) == keep, "capacity %d: an entry twice" % cap
                for e in range(keep):
                    assert pairs[e] in known, "capacity %d: entry %d %r is not listed" % (cap, e, pairs[e])
                    assert (int(t[e, 2]), int(t[e, 3]), int(f[e])) == known[pairs[e]], "capacity %d: entry %d" % (cap, e)


# 6. the rectangle -----------------------------------------------------------------------------------
def rect_rows(seed, m, s):
    """m rows out of one pool of 2 s values shared by every seed's set: sizes random, the middle
    row empty when there are at least two."""
    pool = np.unique(np.random.default_rng(77).integers(1, (1 << 64) - 1, size=2 * s + 64, dtype=np.uint64))[:2 * s]
    rng = np.random.default_rng(seed)
    sizes = [0 if (m > 1 and r == m // 2) else int(rng.integers(1, s + 1)) for r in range(m)]
    return Q.pack([rng.choice(pool, size=z, replace=False) for z in sizes], s)


def gpu_links_rect(kmc, cuda, q, qs, r, rs, mj):
    import torch
    out = kmc.sketch_links_rect(*dev_rows(q, qs, cuda), *dev_rows(r, rs, cuda), K, mj)
    torch.cuda.synchronize()
    return listed(out)


@pytest.mark.parametrize("lib,m,n", [("diag", 1, 5), ("diag", 5, 1), ("diag", 4, 4), ("diag", 9, 13), ("ship", 33, 70)])
def test_rectangle(kmc, cuda, lib, m, n):
    """Entries equal the host filter of kmc.sketch_distances_rect(with_counts=True), bit for
    bit, and the numpy oracle's table."""
    import torch
    s, mj = 64, 0.1
    (q, qs), (r, rs) = rect_rows(100 + m, m, s), rect_rows(200 + n, n, s)
    exp = L.rect_links_expected(q, qs, r, rs, s, mj)
    assert 1 <= exp.shape[0] < m * n
    assert m == 1 or (qs == 0).any()
    assert n == 1 or (rs == 0).any()
    with which(kmc, lib):
        out, sh, dn = kmc.sketch_distances_rect(*dev_rows(q, qs, cuda), *dev_rows(r, rs, cuda), K, with_counts=True)
        torch.cuda.synchronize()
        table, dist, count = gpu_links_rect(kmc, cuda, q, qs, r, rs, mj)
    out, sh, dn = u32(out).reshape(m, n), u32(sh).reshape(m, n), u32(dn).reshape(m, n)
    assert_table((table, dist, count), exp, "%s %d x %d" % (lib, m, n))
    np.testing.assert_array_equal(L.rect_links_from_counts(qs, rs, sh, dn, mj), exp)
    np.testing.assert_array_equal(table[:, 2], sh[table[:, 0], table[:, 1]])
    np.testing.assert_array_equal(table[:, 3], dn[table[:, 0], table[:, 1]])
    np.testing.assert_array_equal(dist, out[table[:, 0], table[:, 1]])


@pytest.mark.parametrize("lib,n", [("diag", 13), ("ship", 37)])
def test_rectangle_of_one_set_with_itself(kmc, cuda, lib, n):
    """(a, a) for every row that is not empty, both orientations of every pair
    kmc_sketch_links lists, and nothing else."""
    s, mj = 64, 0.1
    rows, sizes = T.overlap_rows(4300 + n, n, s)
    with which(kmc, lib):
        tri, tdist, _ = gpu_links(kmc, cuda, rows, sizes, mj)
        table, dist, count = gpu_links_rect(kmc, cuda, rows, sizes, rows, sizes, mj)
    assert 0 < tri.shape[0] < n * (n - 1) // 2 and (sizes == 0).any()
    assert_table((table, dist, count), L.rect_links_expected(rows, sizes, rows, sizes, s, mj), lib)
    same = table[:, 0] == table[:, 1]
    assert table[same][:, 0].tolist() == [a for a in range(n) if sizes[a] > 0]
    np.testing.assert_array_equal(table[same][:, 2], table[same][:, 3])
    assert (dist[same] == 0).all()  # +0.0f
    up, low = table[:, 0] < table[:, 1], table[:, 0] > table[:, 1]
    np.testing.assert_array_equal(table[up], tri)
    np.testing.assert_array_equal(dist[up], tdist)
    mirrored = table[low][:, [1, 0, 2, 3]]
    order = np.lexsort((mirrored[:, 1], mirrored[:, 0]))
    np.testing.assert_array_equal(mirrored[order], tri)
    np.testing.assert_array_equal(dist[low][order], tdist)
    assert count == 2 * tri.shape[0] + int(same.sum())


# 7. trivial sizes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_trivial_sizes(kmc, cuda, lib):
    """No pair to judge: KMC_OK with null rows, num_links = 0 and the outputs untouched."""
    import torch
    links = torch.full((8, 4), POISON32, dtype=torch.int32, device=cuda)
    dist = torch.full((8,), POISON32, dtype=torch.int32, device=cuda)
    count = torch.full((1,), POISON32, dtype=torch.int64, device=cuda)
    real = dev_rows(*T.overlap_rows(1, 3, 64), cuda)
    p, st = kmc._dptr, kmc._stream(None)
    with which(kmc, lib):
        lib_ = kmc.lib()
        calls = [lambda n=n: lib_.kmc_sketch_links(None, None, n, 64, K, 0.5, p(links), p(dist), 8, p(count), st)
                 for n in (0, 1)]
        calls += [lambda m=m, n=n: lib_.kmc_sketch_links_rect(None, None, m, None, None, n, 64, K, 0.0, p(links), p(dist),
                                                              8, p(count), st) for m, n in ((0, 5), (5, 0), (0, 0))]
        # one side empty, the other side's rows real
        calls += [lambda: lib_.kmc_sketch_links_rect(None, None, 0, p(real[0]), p(real[1]), 3, 64, K, 0.0, p(links),
                                                     p(dist), 8, p(count), st),
                  lambda: lib_.kmc_sketch_links(p(real[0]), p(real[1]), 1, 64, K, 0.0, p(links), p(dist), 8, p(count), st)]
        for c, call in enumerate(calls):
            count.fill_(POISON32)
            assert call() == 0, c
            torch.cuda.synchronize()
            assert count.tolist() == [0], c
            assert (u32(links) == POISON32).all() and (u32(dist) == POISON32).all(), c
        # the wrappers on tensors of no row
        none = (torch.empty((0, 64), dtype=torch.int64, device=cuda), torch.empty(0, dtype=torch.int32, device=cuda))
        for out in (kmc.sketch_links(*none, K, 0.5), kmc.sketch_links_rect(*none, *real, K, 0.0),
                    kmc.sketch_links_rect(*real, *none, K, 0.0)):
            assert out[0].shape == (0, 4) and out[1].shape == (0,) and out[2].tolist() == [0]


# 8. a side stream --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delay(kmc, cuda):
    kmc.lib()
    cycles, ms = T.sleep_cycles(T.DELAY_MS)
    assert ms >= 0.9 * T.DELAY_MS, "the delay spins %.1f ms, not %.1f" % (ms, T.DELAY_MS)
    return cycles


@pytest.fixture(scope="module")
def streams(kmc, cuda, delay):
    return T.side_streams(kmc, cuda, delay)


@pytest.mark.parametrize("lib", LIBS)
def test_side_stream_gives_the_null_streams_result(kmc, cuda, lib, delay, streams):
    """stream_util's late-input call: the rows arrive on the side stream behind a delay and
    the outputs, num_links among them, are poisoned there; the call returns while the delay
    spins, and the snapshot taken on that stream holds the real rows' set (sorted before it
    is compared: the order is unspecified)."""
    import torch
    n, s, mj = 12, 64, 0.25
    P = [T.overlap_rows(4200 + w, n, s) for w in (0, 1)]
    rows = [dev(p[0].view(np.int64), cuda) for p in P]
    sizes = [dev(p[1].view(np.int32), cuda) for p in P]
    live = [(rows[0].clone(), rows[0], rows[1]), (sizes[0].clone(), sizes[0], sizes[1])]
    cap = n * (n - 1) // 2
    outs = [torch.empty((cap, 4), dtype=torch.int32, device=cuda), torch.empty(cap, dtype=torch.float32, device=cuda),
            torch.empty(1, dtype=torch.int64, device=cuda)]

    def check(got, e, msg):
        links, dist, count = (np.ascontiguousarray(g) for g in got)
        total = int(count[0])
        assert total == e[0].shape[0], "%s num_links" % msg
        t = links.view(np.uint32).reshape(-1, 4)
        order = np.lexsort((t[:total, 1], t[:total, 0]))
        np.testing.assert_array_equal(t[:total][order], e[0], err_msg=msg)
        np.testing.assert_array_equal(dist.view(np.uint32)[:total][order], e[1], err_msg="%s dist" % msg)
        assert (t[total:] == POISON32).all(), "%s: written beyond num_links" % msg

    with which(kmc, lib):
        # the null stream's result: the oracle's table, and the floats the snapshot is held against
        exp = {}
        for i, w in enumerate(("decoy", "real")):
            table, dist, count = gpu_links(kmc, cuda, *P[i], mj)
            assert_table((table, dist, count), L.links_expected(*P[i], s, mj), "null stream, %s" % w)
            assert 0 < count < cap
            exp[w] = (table, dist)
        call = T.Call("sketch_links", live, outs,
                      lambda w, st: kmc.sketch_links(live[0][0], live[1][0], K, mj, capacity=cap, out=outs, stream=st) and None,
                      exp, check, lambda e: e)
        T.late_call(call, streams[0], delay)
