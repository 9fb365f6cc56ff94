"""kmc_sketch_screen_index_size, _build, _count and _results on a CPU-only host: the
symbols exist, every argument error is returned before any device is touched, and
the size query is the header's formula."""
import ctypes
import subprocess

NAMES = ["kmc_sketch_screen_index_size", "kmc_sketch_screen_build", "kmc_sketch_screen_count",
         "kmc_sketch_screen_results"]
OK, INVALID, BAD_K, ALIGNMENT, WORKSPACE = 0, 1001, 1002, 1003, 1004
MAX_VALUES = 1 << 30  # KMC_SCREEN_MAX_VALUES


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
    assert L.kmc_sketch_screen_index_size.restype is ctypes.c_size_t
    assert [len(getattr(L, n).argtypes) for n in NAMES] == [2, 7, 10, 11]
    assert L.kmc_version() == 200
    assert kmc.SCREEN_MAX_VALUES == MAX_VALUES


_buf = (ctypes.c_char * 1024)()
_base = (ctypes.addressof(_buf) + 255) & ~255


def _p(on, at=0):
    """Null or a 256-byte aligned host address (+ at) that is never dereferenced
    (arguments are checked first)."""
    return ctypes.c_void_p(_base + at) if on else None


BIG = 1 << 40  # index_bytes no size exceeds here


def build(L, r=1, rs=1, n=3, s=16, index=1, at=0, nbytes=BIG):
    return L.kmc_sketch_screen_build(_p(r), _p(rs), n, s, _p(index, at), nbytes, None)


def count(L, index=1, at=0, nbytes=BIG, data=1, idx=1, n=2, data_bytes=64, k=21, flags=0):
    return L.kmc_sketch_screen_count(_p(index, at), nbytes, _p(data), _p(idx), n, data_bytes, k, flags, 42, None)


def results(L, index=1, at=0, nbytes=BIG, r=1, rs=1, n=3, s=16, k=21, shared=1):
    return L.kmc_sketch_screen_results(_p(index, at), nbytes, _p(r), _p(rs), n, s, k, _p(shared), None, None, None)


def test_build_argument_errors_need_no_device(kmc):
    def check(L):
        size = L.kmc_sketch_screen_index_size(3, 16)
        assert build(L, s=0) == INVALID and build(L, s=kmc.SKETCH_MAX_SIZE + 1) == INVALID
        assert build(L, n=MAX_VALUES // 16 + 1) == INVALID and build(L, n=MAX_VALUES + 1, s=1) == INVALID
        for name in ("r", "rs", "index"):
            assert build(L, **{name: 0}) == INVALID, name
        assert build(L, nbytes=size - 1) == WORKSPACE and build(L, nbytes=0) == WORKSPACE
        for at in (1, 8, 16, 128):
            assert build(L, at=at) == ALIGNMENT, at
        assert build(L, nbytes=size - 1, at=8) == WORKSPACE  # the size is judged before the alignment
        # no reference and no index: nothing to do; the limits are still judged
        assert build(L, n=0, r=0, rs=0, index=0) == OK
        assert build(L, n=0, s=0, index=0) == INVALID
        assert build(L, n=0, r=0, rs=0, nbytes=8) == WORKSPACE  # an index given: the empty index needs its bytes

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def test_count_argument_errors_need_no_device(kmc):
    def check(L):
        smallest = L.kmc_sketch_screen_index_size(0, 1)
        assert count(L, k=0) == BAD_K and count(L, k=32) == BAD_K and count(L, k=-1) == BAD_K
        assert count(L, flags=4) == INVALID and count(L, flags=0x80000000) == INVALID
        assert count(L, n=(1 << 40) + 1) == INVALID and count(L, data_bytes=1 << 62) == INVALID
        for name in ("index", "data", "idx"):
            assert count(L, **{name: 0}) == INVALID, name
        assert count(L, nbytes=smallest - 1) == WORKSPACE
        assert count(L, at=64) == ALIGNMENT
        assert count(L, k=32, flags=4) == BAD_K  # k is judged first
        # no record: no work, whatever the pointers, and the index is not touched
        assert count(L, n=0, index=0, data=0, idx=0, nbytes=0) == OK
        assert count(L, n=0, k=0) == BAD_K and count(L, n=0, flags=8) == INVALID

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def test_results_argument_errors_need_no_device(kmc):
    def check(L):
        smallest = L.kmc_sketch_screen_index_size(0, 1)
        assert results(L, k=0) == BAD_K and results(L, k=32) == BAD_K
        assert results(L, s=0) == INVALID and results(L, s=kmc.SKETCH_MAX_SIZE + 1) == INVALID
        assert results(L, n=MAX_VALUES // 16 + 1) == INVALID
        for name in ("index", "r", "rs", "shared"):
            assert results(L, **{name: 0}) == INVALID, name
        assert results(L, nbytes=smallest - 1) == WORKSPACE
        assert results(L, at=32) == ALIGNMENT
        assert results(L, k=32, s=0) == BAD_K  # k is judged first
        assert results(L, n=0, index=0, r=0, rs=0, shared=0, nbytes=0) == OK
        assert results(L, n=0, s=0) == INVALID

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def formula(num_refs, sketch_size, room):
    """include/kmc.h: 256 + round256(4 C) + 8 C, C = max(8, room * values rounded up
    to a power of two); room = 4 (libkmc.so), 2 (libkmc_diag.so)."""
    c = 8
    while c < room * num_refs * sketch_size:
        c *= 2
    return 256 + (4 * c + 255) // 256 * 256 + 8 * c


def test_size_query(kmc):
    f = kmc.sketch_screen_index_size
    shapes = [(0, 1), (1, 1), (1, 2), (1, 3), (2, 1), (3, 16), (12, 1000), (100, 1000), (1000, 1000), (5, 16384),
              (1 << 16, 16384), (1 << 30, 1)]

    def check(room):
        assert f(2, 0) == 0 and f(2, kmc.SKETCH_MAX_SIZE + 1) == 0
        assert f(MAX_VALUES // 16 + 1, 16) == 0 and f(MAX_VALUES + 1, 1) == 0 and f(1 << 63, 2) == 0
        for n, s in shapes:
            assert f(n, s) == formula(n, s, room), (n, s)
        assert f(0, 1) == 256 + 256 + 64
        # monotone in both arguments
        for s in (1, 7, 1000):
            sizes = [f(n, s) for n in (0, 1, 2, 3, 10, 1000, 10 ** 5)]
            assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
        for n in (1, 12, 1000):
            sizes = [f(n, s) for s in (1, 2, 64, 1000, 1024, 1025, 16384)]
            assert sizes == sorted(sizes) and sizes[0] < sizes[-1]

    check(4)
    with kmc.diag():
        check(2)
