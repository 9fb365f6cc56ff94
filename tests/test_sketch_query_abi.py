"""kmc_sketch_distances_rect, kmc_sketch_nearest and its size query on a CPU-only
host: the symbols exist, and every argument error is returned before any device is
touched."""
import ctypes
import subprocess

NAMES = ["kmc_sketch_distances_rect", "kmc_sketch_nearest", "kmc_sketch_nearest_workspace_size"]
OK, INVALID, BAD_K = 0, 1001, 1002
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
    assert L.kmc_sketch_nearest_workspace_size.restype is ctypes.c_size_t
    assert len(L.kmc_sketch_distances_rect.argtypes) == 12
    assert len(L.kmc_sketch_nearest.argtypes) == 18
    assert len(L.kmc_sketch_nearest_workspace_size.argtypes) == 5
    assert L.kmc_version() == 200
    assert kmc.NEAREST_MAX_TOP == 1024


_buf = (ctypes.c_char * 256)()


def _p(on, at=0):
    """Null or a host address that is never dereferenced (arguments are checked first)."""
    return ctypes.c_void_p(ctypes.addressof(_buf) + at) if on else None


def rect(L, q=1, qs=1, m=2, r=1, rs=1, n=3, s=16, k=21, out=1):
    return L.kmc_sketch_distances_rect(_p(q), _p(qs), m, _p(r), _p(rs), n, s, k, _p(out), None, None, None)


def nearest(L, q=1, qs=1, m=2, r=1, rs=1, n=3, s=16, k=21, top=4, min_shared=1, refs=1, counts=1):
    return L.kmc_sketch_nearest(_p(q), _p(qs), m, _p(r), _p(rs), n, s, k, top, min_shared, _p(refs), None, None, None,
                                _p(counts), None, 0, None)


def test_rect_argument_errors_need_no_device(kmc):
    def check(L):
        assert rect(L, k=0) == BAD_K and rect(L, k=32) == BAD_K and rect(L, k=-1) == BAD_K
        assert rect(L, s=0) == INVALID and rect(L, s=kmc.SKETCH_MAX_SIZE + 1) == INVALID
        for name in ("q", "qs", "r", "rs", "out"):
            assert rect(L, **{name: 0}) == INVALID, name
        assert rect(L, m=MAX_SEQS + 1) == INVALID and rect(L, n=MAX_SEQS + 1) == INVALID
        # either count 0: no work, whatever the pointers
        assert rect(L, m=0, q=0, qs=0, out=0) == OK and rect(L, n=0, r=0, rs=0, out=0) == OK
        assert rect(L, m=0, k=32) == BAD_K  # k is judged first, as by kmc_sketch_distances

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def test_nearest_argument_errors_need_no_device(kmc):
    def check(L):
        assert nearest(L, k=0) == BAD_K and nearest(L, k=32) == BAD_K
        assert nearest(L, s=0) == INVALID and nearest(L, s=kmc.SKETCH_MAX_SIZE + 1) == INVALID
        assert nearest(L, top=0) == INVALID and nearest(L, top=kmc.NEAREST_MAX_TOP + 1) == INVALID
        assert nearest(L, n=(1 << 32) - 1) == INVALID and nearest(L, m=MAX_SEQS + 1) == INVALID
        assert nearest(L, refs=0) == INVALID and nearest(L, counts=0) == INVALID
        for name in ("q", "qs", "r", "rs"):
            assert nearest(L, **{name: 0}) == INVALID, name
        assert nearest(L, k=32, s=0) == BAD_K  # k is judged first
        # no query: no work, whatever the pointers; the limits are still judged
        assert nearest(L, m=0, q=0, qs=0, r=0, rs=0, refs=0, counts=0) == OK
        assert nearest(L, m=0, top=0) == INVALID

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def test_size_query_is_zero_on_bad_arguments(kmc):
    f = kmc.sketch_nearest_workspace_size
    assert f(2, 3, 0, 4) == 0 and f(2, 3, kmc.SKETCH_MAX_SIZE + 1, 4) == 0
    assert f(2, 3, 16, 0) == 0 and f(2, 3, 16, kmc.NEAREST_MAX_TOP + 1) == 0
    assert f(2, (1 << 32) - 1, 16, 4) == 0 and f(MAX_SEQS + 1, 3, 16, 4) == 0
    assert f(2, 3, 16, 4, device=-1) == 0
    # nothing to search: no workspace, and no device asked
    assert f(0, 3, 16, 4) == 0 and f(2, 0, 16, 4) == 0
