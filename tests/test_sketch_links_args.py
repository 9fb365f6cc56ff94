"""kmc_sketch_links and kmc_sketch_links_rect on a CPU-only host: the symbols exist, every
argument error is returned before any device is touched and in the header's order, the
count-only form passes those checks, and the ctypes mirror of kmc_sketch_link is 16 bytes.
The numpy oracle of the GPU tests (sketch_links_util.py) is checked here against the one
of the sketch tests."""
import ctypes
import subprocess

import numpy as np

import sketch_cluster_util as C
import sketch_links_util as L
import sketch_query_util as Q
import sketch_util as S

NAMES = ["kmc_sketch_links", "kmc_sketch_links_rect"]
OK, INVALID, BAD_K, ALIGNMENT = 0, 1001, 1002, 1003
MAX_SEQS = 1 << 31  # KMC_SPARSE_MAX_SEQS


def test_header_and_libraries_have_the_symbols(kmc):
    names = kmc.header_symbols()
    for n in NAMES:
        assert n in names
        assert getattr(kmc.lib(), n).argtypes is not None
        with kmc.diag() as D:
            assert getattr(D, n).argtypes is not None
    for path in (kmc.LIB_PATH, kmc.DIAG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        assert set(NAMES) <= exported
    lib = kmc.lib()
    assert len(lib.kmc_sketch_links.argtypes) == 11 and len(lib.kmc_sketch_links_rect.argtypes) == 14
    assert lib.kmc_version() == 200


def test_link_entry_is_16_bytes(kmc):
    assert ctypes.sizeof(kmc.SketchLink) == 16
    assert [f[0] for f in kmc.SketchLink._fields_] == ["i", "j", "shared", "denom"]
    assert [getattr(kmc.SketchLink, f).offset for f in ("i", "j", "shared", "denom")] == [0, 4, 8, 12]


_buf = (ctypes.c_char * 256)()
_base = ctypes.addressof(_buf) + (-ctypes.addressof(_buf)) % 16  # a 16-byte aligned host address


def _p(on, skew=0):
    """Null or a host address that is never dereferenced (arguments are checked first)."""
    return ctypes.c_void_p(_base + skew) if on else None


def tri(lib, rows=1, sizes=1, n=3, s=16, k=21, j=0.5, links=1, dist=1, cap=4, count=1, skew=0):
    return lib.kmc_sketch_links(_p(rows), _p(sizes), n, s, k, j, _p(links, skew), _p(dist), cap, _p(count), None)


def rect(lib, q=1, qs=1, m=2, r=1, rs=1, n=3, s=16, k=21, j=0.5, links=1, dist=1, cap=4, count=1, skew=0):
    return lib.kmc_sketch_links_rect(_p(q), _p(qs), m, _p(r), _p(rs), n, s, k, j, _p(links, skew), _p(dist), cap,
                                     _p(count), None)


def test_argument_errors_need_no_device_and_keep_their_order(kmc):
    def check(lib):
        for f in (tri, rect):
            # each error alone
            for k in (0, -1, 32, 99):
                assert f(lib, k=k) == BAD_K, k
            assert f(lib, s=0) == INVALID and f(lib, s=kmc.SKETCH_MAX_SIZE + 1) == INVALID
            assert f(lib, n=MAX_SEQS + 1) == INVALID
            for j in (float("nan"), -0.1, 1.5, float("inf"), -float("inf"), np.nextafter(1.0, 2.0), -5e-324):
                assert f(lib, j=j) == INVALID, j
            assert f(lib, count=0) == INVALID
            assert f(lib, links=0) == INVALID and f(lib, links=0, dist=0) == INVALID  # capacity 4 and no list
            for skew in (1, 4, 8, 15):
                assert f(lib, skew=skew) == ALIGNMENT, skew
            # the order: k, then the invalid arguments, then the alignment
            assert f(lib, k=0, s=0) == BAD_K and f(lib, k=0, count=0) == BAD_K and f(lib, k=0, skew=4) == BAD_K
            assert f(lib, k=32, j=2.0, links=0) == BAD_K
            for bad in (dict(s=0), dict(n=MAX_SEQS + 1), dict(j=2.0), dict(count=0)):
                assert f(lib, skew=4, **bad) == INVALID, bad
            # the trivial sizes are judged like any other
            assert f(lib, n=0, s=0) == INVALID and f(lib, n=0, j=2.0) == INVALID and f(lib, n=0, count=0) == INVALID
            assert f(lib, n=0, k=0) == BAD_K and f(lib, n=0, links=0) == INVALID and f(lib, n=0, skew=8) == ALIGNMENT
        assert rect(lib, m=MAX_SEQS + 1) == INVALID and rect(lib, m=MAX_SEQS + 1, n=0) == INVALID
        # null rows or sizes while there is a pair to judge, before the alignment
        assert tri(lib, rows=0) == INVALID and tri(lib, sizes=0) == INVALID and tri(lib, rows=0, n=2, skew=4) == INVALID
        for name in ("q", "qs", "r", "rs"):
            assert rect(lib, **{name: 0}) == INVALID, name
            assert rect(lib, m=1, n=1, skew=4, **{name: 0}) == INVALID, name
        # ... and not without one: only the alignment is left to refuse
        assert tri(lib, rows=0, sizes=0, n=1, skew=4) == ALIGNMENT and tri(lib, rows=0, sizes=0, n=0, skew=4) == ALIGNMENT
        assert rect(lib, q=0, qs=0, r=0, rs=0, m=0, skew=4) == ALIGNMENT
        assert rect(lib, q=0, qs=0, r=0, rs=0, n=0, skew=4) == ALIGNMENT

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def test_count_only_form_passes_the_argument_checks(kmc):
    """capacity 0 with null links and null dist.  Without a device the call fails at its first
    HIP call, the zeroing of num_links, with HIP's error and none of the library's argument
    errors; with one, the call of no record is made for real."""
    import torch
    refused = (INVALID, BAD_K, ALIGNMENT, 1004)
    if not torch.cuda.is_available():
        def check(lib):
            assert tri(lib, links=0, dist=0, cap=0) not in (OK,) + refused
            assert rect(lib, links=0, dist=0, cap=0) not in (OK,) + refused
            assert tri(lib, links=0, dist=0, cap=0, rows=0, sizes=0, n=1) not in (OK,) + refused

        check(kmc.lib())
        with kmc.diag() as D:
            check(D)
        return
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    none = torch.empty((0, 16), dtype=torch.int64, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda")
    links, dist, got = kmc.sketch_links(*none, 21, 0.5, capacity=0, out=(None, None, count))
    assert links is None and dist is None and got is count and count.tolist() == [0]


def test_oracle_counts_of_the_rectangle():
    """pair_counts_rect is the merge rule of sketch_util.distances_expected (through
    sketch_query_util.pair_counts for the pairs the triangle does not hold), and the listed
    tables are the pairs sketch_cluster_util.links accepts."""
    rng = np.random.default_rng(3)
    s, n = 16, 12
    pool = np.unique(rng.integers(1, (1 << 64) - 1, size=3 * s, dtype=np.uint64))
    lists = [rng.choice(pool, size=int(z), replace=False) for z in [s, 0, 1, s - 1, 0] + list(rng.integers(0, s + 1, n - 5))]
    rows, sizes = Q.pack(lists, s)
    _, sh, dn = S.distances_expected(rows, sizes, s, 21)
    rsh, rdn = L.pair_counts_rect(rows, sizes, rows, sizes, s)
    i, j = C.triangle_pairs(n)
    np.testing.assert_array_equal(rsh[i, j], sh)
    np.testing.assert_array_equal(rdn[i, j], dn)
    np.testing.assert_array_equal(rsh, rsh.T)
    np.testing.assert_array_equal(rdn, rdn.T)
    np.testing.assert_array_equal(np.diag(rsh), sizes)
    np.testing.assert_array_equal(np.diag(rdn), sizes)
    assert L.tri_index(i, j, n).tolist() == list(range(n * (n - 1) // 2))
    # two different sets, one of them short
    qsh, qdn = L.pair_counts_rect(rows[:5], sizes[:5], rows[3:], sizes[3:], s)
    sets = Q.row_sets(rows, sizes, s)
    for a in range(5):
        for b in range(n - 3):
            assert (qsh[a, b], qdn[a, b]) == Q.pair_counts(sets[a], sets[3 + b], s), (a, b)
    assert L.pair_counts_rect(rows[:0], sizes[:0], rows, sizes, s)[0].shape == (0, n)
    # the tables: the triangle's pairs that pass the rule, and both orientations and the diagonal in the square
    for mj in (0.0, 0.2, 1.0):
        t = L.links_expected(rows, sizes, s, mj)
        on = C.links(sh, dn, mj, sizes[i], sizes[j])
        assert t.tolist() == [[int(a), int(b), int(x), int(y)] for a, b, x, y in zip(i[on], j[on], sh[on], dn[on])]
        r = L.rect_links_expected(rows, sizes, rows, sizes, s, mj)
        up = r[r[:, 0] < r[:, 1]]
        assert up.tolist() == t.tolist()
        assert sorted(map(tuple, r[r[:, 0] > r[:, 1]][:, [1, 0, 2, 3]].tolist())) == sorted(map(tuple, t.tolist()))
        assert r[r[:, 0] == r[:, 1]][:, 0].tolist() == [x for x in range(n) if sizes[x] > 0]
    assert L.links_expected(rows, sizes, s, 0.0).shape[0] == (int((sizes > 0).sum()) * (int((sizes > 0).sum()) - 1)) // 2
