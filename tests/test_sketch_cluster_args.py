"""kmc_sketch_cluster, its size query and kmc_mash_jaccard_of_distance on a CPU-only
host: the symbols exist, every argument error is returned before any device is
touched, and the distance-to-Jaccard conversion is the formula of the header.  The
numpy oracle of the GPU tests (sketch_cluster_util.py) is checked here against the
one of the sketch tests."""
import ctypes
import math
import subprocess

import numpy as np

import sketch_cluster_util as C
import sketch_util as S

NAMES = ["kmc_sketch_cluster", "kmc_sketch_cluster_workspace_size", "kmc_mash_jaccard_of_distance"]
OK, INVALID = 0, 1001
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
    L = kmc.lib()
    assert L.kmc_sketch_cluster_workspace_size.restype is ctypes.c_size_t
    assert L.kmc_mash_jaccard_of_distance.restype is ctypes.c_double
    assert len(L.kmc_sketch_cluster.argtypes) == 11
    assert L.kmc_version() == 200


_buf = (ctypes.c_char * 256)()


def _p(on):
    """Null or a host address that is never dereferenced (arguments are checked first)."""
    return ctypes.c_void_p(ctypes.addressof(_buf)) if on else None


def cluster(L, rows=1, sizes=1, n=3, s=16, j=0.5, labels=1, index=1, count=0):
    return L.kmc_sketch_cluster(_p(rows), _p(sizes), n, s, j, _p(labels), _p(index), _p(count), None, 0, None)


def test_argument_errors_need_no_device(kmc):
    def check(L):
        assert cluster(L, s=0) == INVALID and cluster(L, s=kmc.SKETCH_MAX_SIZE + 1) == INVALID
        assert cluster(L, n=MAX_SEQS + 1) == INVALID
        for j in (float("nan"), -0.1, 1.5, float("inf"), -float("inf"), np.nextafter(1.0, 2.0), -5e-324):
            assert cluster(L, j=j) == INVALID, j
        assert cluster(L, labels=0) == INVALID and cluster(L, labels=0, n=0) == INVALID
        assert cluster(L, rows=0) == INVALID and cluster(L, sizes=0) == INVALID
        # no record: no work, whatever the rows; the limits are still judged
        for j in (0.0, 1.0, 0.5):
            assert cluster(L, n=0, rows=0, sizes=0, index=0, j=j) == OK
        assert cluster(L, n=0, s=0) == INVALID and cluster(L, n=0, j=2.0) == INVALID

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def round256(x):
    return (x + 255) & ~255


def test_size_query(kmc):
    f = kmc.sketch_cluster_workspace_size
    assert f(0) == 0 and f(MAX_SEQS + 1) == 0 and f(5, device=-1) == 0
    # the header's formula; no device is asked
    for n in (1, 2, 63, 64, 65, 4096, 4097, 100_000, MAX_SEQS):
        exp = 2 * round256(4 * n) + round256(8 * (n + 1)) + round256(8 * ((n + 4095) // 4096))
        assert f(n) == exp, n
        with kmc.diag():
            assert f(n) == exp, n


def test_jaccard_of_distance(kmc):
    f = kmc.mash_jaccard_of_distance
    for k in (1, 21, 31):
        assert f(0.0, k) == 1.0
        last = 1.0
        for d in np.linspace(0.0, 1.0, 201)[1:]:
            j = f(d, k)
            assert 0.0 < j < last, (d, k)
            last = j
    for d, k in ((-0.01, 21), (1.01, 21), (float("nan"), 21), (float("inf"), 21), (0.05, 0), (0.05, 32), (0.05, -1)):
        assert math.isnan(f(d, k)), (d, k)
    rng = np.random.default_rng(1)
    for d in list(rng.random(200)) + [1.0, 0.05, 0.01, 1e-300]:
        for k in (1, 16, 21, 31):
            e = math.exp(-k * d)
            exp = e / (2.0 - e)
            assert abs(f(d, k) - exp) <= math.ulp(exp), (d, k)
    with kmc.diag() as D:
        assert D.kmc_mash_jaccard_of_distance(0.05, 21) == f(0.05, 21)


def test_oracle_counts_and_components():
    """pair_counts_packed is the merge rule of sketch_util.distances_expected, and
    components gives the minimum of every component and its rank."""
    rng = np.random.default_rng(2)
    s, n = 16, 12
    pool = np.unique(rng.integers(1, (1 << 64) - 1, size=3 * s, dtype=np.uint64))
    lists = [rng.choice(pool, size=int(z), replace=False) for z in [s, 0, 1, s - 1, 0] + list(rng.integers(0, s + 1, n - 5))]
    rows, sizes = C.Q.pack(lists, s)
    _, sh, dn = S.distances_expected(rows, sizes, s, 21)
    fsh, fdn = C.pair_counts_packed(rows, sizes, s)
    np.testing.assert_array_equal(fsh, sh)
    np.testing.assert_array_equal(fdn, dn)
    labels, index, count = C.components(7, [(5, 3), (3, 6), (1, 4)])
    assert labels.tolist() == [0, 1, 2, 3, 1, 3, 3] and index.tolist() == [0, 1, 2, 3, 1, 3, 3] and count == 4
    labels, index, count = C.components(5, [(4, 2), (1, 3)])
    assert labels.tolist() == [0, 1, 2, 1, 2] and index.tolist() == [0, 1, 2, 1, 2] and count == 3
    assert C.components(0, [])[2] == 0
    assert C.links([32, 32, 0, 0, 1], [64, 64, 0, 5, 1], 0.5).tolist() == [True, True, False, False, True]
    assert C.links([32], [64], np.nextafter(0.5, 1)).tolist() == [False]
    assert C.links([0, 0], [0, 3], 0.0).tolist() == [False, True]
    assert C.links([0, 0, 2], [0, 3, 3], 0.0, [0, 0, 2], [0, 3, 3]).tolist() == [False, False, True]
