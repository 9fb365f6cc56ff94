"""kmc_pair_distances_sparse: the entry points exist in header, library and
binding, and their argument errors are returned before any device call."""
import ctypes


def test_sparse_entry_points_declared_and_exported(kmc):
    names = kmc.header_symbols()
    L = kmc.lib()
    for fn in ("kmc_pair_distances_sparse", "kmc_pair_distances_sparse_workspace_size"):
        assert fn in names
        assert hasattr(L, fn)
        assert getattr(L, fn).argtypes is not None


def test_sparse_argument_errors_need_no_device(kmc):
    L = kmc.lib()
    f = L.kmc_pair_distances_sparse
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))  # never dereferenced: every call below returns early
    # k outside 1..KMC_CANON_MAX_K, with null pointers
    assert f(None, None, None, 0, None, 5, 0, None, None, 0, None) == 1002
    assert f(None, None, None, 0, None, 5, 32, None, None, 0, None) == 1002
    # fewer than two records: nothing to do
    assert f(None, None, None, 0, None, 0, 31, None, None, 0, None) == 0
    assert f(None, None, None, 0, None, 1, 31, None, None, 0, None) == 0
    # null out / rec_offsets / indices
    assert f(p, p, p, 4, p, 3, 31, None, None, 0, None) == 1001
    assert f(p, p, None, 4, p, 3, 31, p, None, 0, None) == 1001
    assert f(p, p, p, 4, None, 3, 31, p, None, 0, None) == 1001
    # null keys or counts with entries
    assert f(None, p, p, 4, p, 3, 31, p, None, 0, None) == 1001
    assert f(p, None, p, 4, p, 3, 31, p, None, 0, None) == 1001
    # more records than the packed record id holds
    assert f(p, p, p, 4, p, (1 << 31) + 1, 31, p, None, 0, None) == 1001


def test_sparse_size_query_bad_arguments(kmc):
    L = kmc.lib()
    assert L.kmc_pair_distances_sparse_workspace_size(0, 100, 0) == 0
    assert L.kmc_pair_distances_sparse_workspace_size(1, 100, 0) == 0
    assert L.kmc_pair_distances_sparse_workspace_size((1 << 31) + 1, 100, 0) == 0
    assert kmc.pair_distances_sparse_workspace_size(1, 0) == 0
