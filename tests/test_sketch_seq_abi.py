"""kmc_sketch_from_sequences on a CPU-only host: the symbols exist, and every
argument error is returned before any device is touched."""
import ctypes

NAMES = ["kmc_sketch_from_sequences", "kmc_sketch_from_sequences_workspace_size"]
OK, INVALID, BAD_K = 0, 1001, 1002


def test_header_and_libraries_have_the_symbols(kmc):
    names = kmc.header_symbols()
    for n in NAMES:
        assert n in names
        assert hasattr(kmc.lib(), n)
        with kmc.diag() as D:
            assert hasattr(D, n)
    assert kmc.lib().kmc_version() == 200


def call(L, data=1, indices=1, n=3, data_bytes=64, k=21, flags=0, s=16, seed=42, sk=1, sz=1):
    """Null or a host address that is never dereferenced (arguments are checked first)."""
    buf = (ctypes.c_char * 64)()
    p = lambda on: ctypes.c_void_p(ctypes.addressof(buf)) if on else None
    return L.kmc_sketch_from_sequences(p(data), p(indices), n, data_bytes, k, flags, s, seed, p(sk), p(sz), None, 0,
                                       None)


def test_argument_errors_need_no_device(kmc):
    def check(L):
        assert call(L, k=0) == BAD_K and call(L, k=32) == BAD_K and call(L, k=-1) == BAD_K
        assert call(L, s=0) == INVALID and call(L, s=kmc.SKETCH_MAX_SIZE + 1) == INVALID
        assert call(L, flags=4) == INVALID and call(L, flags=1 | 2 | 8) == INVALID
        assert call(L, indices=0) == INVALID and call(L, sk=0) == INVALID and call(L, sz=0) == INVALID
        assert call(L, data=0, data_bytes=1) == INVALID
        # k is judged first, as by the canonical counter; then no record, no work
        assert call(L, k=32, s=0) == BAD_K
        assert call(L, n=0, data=0, indices=0, sk=0, sz=0, data_bytes=0) == OK
        assert call(L, n=0, s=0) == INVALID

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def test_size_query_is_zero_on_bad_arguments(kmc):
    f = kmc.sketch_from_sequences_workspace_size
    assert f(0, 1000, 16) == 0
    assert f(3, 1000, 0) == 0 and f(3, 1000, kmc.SKETCH_MAX_SIZE + 1) == 0
    assert f(3, 1000, 16, device=-1) == 0
    assert f((1 << 40) + 1, 1000, 16) == 0


def test_binding_signature(kmc):
    L = kmc.lib()
    assert L.kmc_sketch_from_sequences_workspace_size.restype is ctypes.c_size_t
    assert len(L.kmc_sketch_from_sequences.argtypes) == 13
