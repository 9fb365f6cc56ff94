"""kmc_sketch_from_sequences_grouped and kmc_sketch_merge_groups on a CPU-only host:
the symbols exist, and every argument error is returned before any device is touched."""
import ctypes

NAMES = ["kmc_sketch_from_sequences_grouped", "kmc_sketch_from_sequences_grouped_workspace_size",
         "kmc_sketch_merge_groups"]
OK, INVALID, BAD_K = 0, 1001, 1002


def test_header_and_libraries_have_the_symbols(kmc):
    names = kmc.header_symbols()
    for n in NAMES:
        assert n in names
        assert getattr(kmc.lib(), n).argtypes is not None
        with kmc.diag() as D:
            assert getattr(D, n).argtypes is not None
    L = kmc.lib()
    assert L.kmc_sketch_from_sequences_grouped_workspace_size.restype is ctypes.c_size_t
    assert len(L.kmc_sketch_from_sequences_grouped.argtypes) == 15
    assert len(L.kmc_sketch_merge_groups.argtypes) == 9
    assert L.kmc_version() == 200


_buf = (ctypes.c_char * 256)()


def _p(on, at=0):
    """Null or a host address that is never dereferenced (arguments are checked first)."""
    return ctypes.c_void_p(ctypes.addressof(_buf) + at) if on else None


def grouped(L, data=1, indices=1, n=3, data_bytes=64, groups=1, ng=2, k=21, flags=0, s=16, seed=42, sk=1, sz=1):
    return L.kmc_sketch_from_sequences_grouped(_p(data), _p(indices), n, data_bytes, _p(groups), ng, k, flags, s, seed,
                                               _p(sk), _p(sz), None, 0, None)


def merge(L, rows_in=1, sizes_in=1, rows=0, groups=1, ng=0, s=2, out=1, sizes_out=1, out_at=128, sizes_at=192):
    return L.kmc_sketch_merge_groups(_p(rows_in), _p(sizes_in, 64), rows, _p(groups, 96), ng, s, _p(out, out_at),
                                     _p(sizes_out, sizes_at), None)


def test_grouped_argument_errors_need_no_device(kmc):
    def check(L):
        assert grouped(L, k=0) == BAD_K and grouped(L, k=32) == BAD_K and grouped(L, k=-1) == BAD_K
        assert grouped(L, s=0) == INVALID and grouped(L, s=kmc.SKETCH_MAX_SIZE + 1) == INVALID
        assert grouped(L, flags=4) == INVALID and grouped(L, flags=1 | 2 | 8) == INVALID
        assert grouped(L, indices=0) == INVALID and grouped(L, sk=0) == INVALID and grouped(L, sz=0) == INVALID
        assert grouped(L, data=0, data_bytes=1) == INVALID
        assert grouped(L, groups=0) == INVALID
        assert grouped(L, ng=(1 << 40) + 1) == INVALID and grouped(L, n=(1 << 40) + 1) == INVALID
        assert grouped(L, k=32, s=0) == BAD_K  # k is judged first, as by the ungrouped call
        # no group, or no record: no work, whatever the pointers
        assert grouped(L, ng=0, groups=0, data=0, indices=0, sk=0, sz=0) == OK
        assert grouped(L, n=0, data=0, indices=0, sk=0, sz=0, data_bytes=0) == OK
        assert grouped(L, ng=0, s=0) == INVALID and grouped(L, n=0, groups=0) == INVALID

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def test_merge_groups_argument_errors_need_no_device(kmc):
    def check(L):
        assert merge(L, s=0, ng=1) == INVALID and merge(L, s=kmc.SKETCH_MAX_SIZE + 1, ng=1) == INVALID
        assert merge(L, ng=(1 << 40) + 1) == INVALID and merge(L, rows=(1 << 40) + 1, ng=1) == INVALID
        assert merge(L, ng=1, groups=0) == INVALID
        assert merge(L, ng=1, out=0) == INVALID and merge(L, ng=1, sizes_out=0) == INVALID
        assert merge(L, ng=1, rows=1, rows_in=0) == INVALID and merge(L, ng=1, rows=1, sizes_in=0) == INVALID
        # the output over the input: rows of 2 x 8 bytes at 0 and at 8; sizes at 64 and at 66
        assert merge(L, ng=1, rows=1, out_at=8) == INVALID
        assert merge(L, ng=1, rows=1, sizes_at=66) == INVALID
        assert merge(L, ng=0, groups=0, out=0, sizes_out=0, rows_in=0, sizes_in=0) == OK

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def test_size_query_is_zero_on_bad_arguments(kmc):
    f = kmc.sketch_from_sequences_grouped_workspace_size
    assert f(0, 2, 1000, 16) == 0 and f(3, 0, 1000, 16) == 0
    assert f(3, 2, 1000, 0) == 0 and f(3, 2, 1000, kmc.SKETCH_MAX_SIZE + 1) == 0
    assert f(3, 2, 1000, 16, device=-1) == 0
    assert f((1 << 40) + 1, 2, 1000, 16) == 0 and f(3, (1 << 40) + 1, 1000, 16) == 0
