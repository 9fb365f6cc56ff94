"""kmc_sketch_from_counts / kmc_sketch_distances / kmc_sketch_workspace_size: the
entry points exist in header, library and binding, their argument errors and
zero-work cases return before any device call, and the host oracle's hash
inverts (tests/sketch_util.py)."""
import ctypes

import numpy as np

import sketch_util as S

FNS = ("kmc_sketch_from_counts", "kmc_sketch_distances", "kmc_sketch_workspace_size")


def _p():
    buf = (ctypes.c_char * 64)()
    return buf, ctypes.c_void_p(ctypes.addressof(buf))  # never dereferenced: every call returns early


def test_sketch_entry_points_declared_and_exported(kmc):
    names = kmc.header_symbols()
    L = kmc.lib()
    for fn in FNS:
        assert fn in names
        assert hasattr(L, fn)
        assert getattr(L, fn).argtypes is not None
    assert kmc.SKETCH_MAX_SIZE == 16384 and kmc.SKETCH_DEFAULT_SEED == 42
    assert L.kmc_version() == 200


def test_sketch_from_counts_argument_errors_need_no_device(kmc):
    f = kmc.lib().kmc_sketch_from_counts
    _buf, p = _p()
    # keys, counts, rec_offsets, num_entries, num_seqs, s, seed, min_count, sketches, sizes, ws, ws_bytes, stream
    assert f(p, p, p, 4, 3, 0, 42, 1, p, p, None, 0, None) == 1001          # sketch_size 0
    assert f(p, p, p, 4, 3, 16385, 42, 1, p, p, None, 0, None) == 1001      # above KMC_SKETCH_MAX_SIZE
    assert f(p, p, None, 4, 3, 16, 42, 1, p, p, None, 0, None) == 1001      # null rec_offsets
    assert f(p, p, p, 4, 3, 16, 42, 1, None, p, None, 0, None) == 1001      # null sketches
    assert f(p, p, p, 4, 3, 16, 42, 1, p, None, None, 0, None) == 1001      # null sketch_sizes
    assert f(None, p, p, 4, 3, 16, 42, 1, p, p, None, 0, None) == 1001      # null keys with entries
    assert f(p, None, p, 4, 3, 16, 42, 2, p, p, None, 0, None) == 1001      # null counts with min_count > 1
    assert f(p, p, p, (1 << 40) + 1, 3, 16, 42, 1, p, p, None, 0, None) == 1001
    # no records: nothing to do, whatever the pointers
    assert f(None, None, None, 0, 0, 16, 42, 1, None, None, None, 0, None) == 0
    assert f(None, None, None, 0, 0, 16384, 42, 0, None, None, None, 0, None) == 0
    # ... but a bad sketch size is still refused
    assert f(None, None, None, 0, 0, 0, 42, 1, None, None, None, 0, None) == 1001


def test_sketch_distances_argument_errors_need_no_device(kmc):
    f = kmc.lib().kmc_sketch_distances
    _buf, p = _p()
    # sketches, sizes, num_seqs, s, k, out, shared, denom, stream
    assert f(None, None, 5, 16, 0, None, None, None, None) == 1002
    assert f(None, None, 5, 16, 32, None, None, None, None) == 1002
    assert f(None, None, 0, 16, 21, None, None, None, None) == 0
    assert f(None, None, 1, 16, 31, None, None, None, None) == 0
    assert f(None, p, 3, 16, 21, p, None, None, None) == 1001
    assert f(p, None, 3, 16, 21, p, None, None, None) == 1001
    assert f(p, p, 3, 16, 21, None, None, None, None) == 1001
    assert f(p, p, 3, 0, 21, p, None, None, None) == 1001
    assert f(p, p, 3, 16385, 21, p, None, None, None) == 1001


def test_sketch_size_query_bad_arguments(kmc):
    L = kmc.lib()
    assert L.kmc_sketch_workspace_size(8, 100, 0, 0) == 0
    assert L.kmc_sketch_workspace_size(8, 100, 16385, 0) == 0
    assert L.kmc_sketch_workspace_size(8, (1 << 40) + 1, 16, 0) == 0
    assert L.kmc_sketch_workspace_size(8, 100, 16, -1) == 0
    assert kmc.sketch_workspace_size(0, 0, 16) == 0


def test_oracle_hash_is_splitmix_and_inverts(kmc):
    rng = np.random.default_rng(1)
    keys = np.concatenate([rng.integers(0, 1 << 62, size=1000, dtype=np.uint64),
                           np.array([0, 1, (1 << 64) - 1], dtype=np.uint64)])
    for seed in (0, 42, (1 << 64) - 1):
        h = S.hash_keys(keys, seed)
        np.testing.assert_array_equal(h[:50], np.array([int(kmc.splitmix64_np(int(k) ^ seed, 0)) for k in keys[:50]],
                                                       dtype=np.uint64))
        np.testing.assert_array_equal(S.unhash(h, seed), keys)
        assert np.unique(h).size == np.unique(keys).size
    edge = np.array([0, (1 << 64) - 1, 1 << 63], dtype=np.uint64)
    np.testing.assert_array_equal(S.hash_keys(S.unhash(edge, 42), 42), edge)
