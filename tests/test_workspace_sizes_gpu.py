"""The four *_workspace_size entry points against recorded values.

tests/golden/workspace_sizes.json was recorded on an MI355X with the library built
from the commit before the workspace layouts moved to csrc/kmc_workspace.h: every
layout must keep its total byte for byte.  The sizes depend on the device's CU
count (grid sizes enter the layouts), so the file stores it and the test asserts
it.  Only size queries: nothing is allocated or launched.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")

# radix (9 <= k <= 13): radix_plan takes sampled mode from kSampledMinPerList * n * NBK
# windows on, NBK = 4^k >> low_bits(k) buckets per record (kmc_radix.hip)
SAMPLED_MIN_PER_LIST = 256 * 1024


def _radix_nbk(k):
    low = min(2 * k - 6, 16 if k >= 12 else 15)
    return 1 << (2 * k - low)


def _offsets(lengths):
    """Record offsets of records of these lengths, each followed by its terminator."""
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64) + 1)]).astype(np.int64)


def compute_sizes(kmc, device):
    """{case name: bytes} of every case, in a fixed order."""
    out = {}
    for k in (3, 6, 8):
        for n, nbytes in ((1, 16), (10, 1 << 20), (10, 10 ** 10)):
            out["dense k=%d n=%d bytes=%d" % (k, n, nbytes)] = kmc.dense_workspace_size(k, n, nbytes, device)
    for k in (9, 11, 13):
        out["radix exact k=%d n=3 bytes=%d" % (k, 1 << 20)] = kmc.dense_workspace_size(k, 3, 1 << 20, device)
        nbytes = SAMPLED_MIN_PER_LIST * _radix_nbk(k)  # n = 1: the first size that samples
        out["radix sampled k=%d n=1 bytes=%d" % (k, nbytes)] = kmc.dense_workspace_size(k, 1, nbytes, device)
    a = kmc.DenseArgs()  # one k = 8 shard, its windows strictly inside the data it reads
    a.k, a.num_seqs = 8, 10
    a.read_lo, a.read_hi = 0, 1 << 24
    a.win_lo, a.win_hi = 1234567, 7654321
    out["dense_ex k=8 n=10 win=[1234567,7654321)"] = kmc.dense_ex_workspace_size(a, device)
    for k in (11, 31):
        for lengths in ([0, 5, 40000, 1, 333333, 64], [3000000, 1, 1000001], [100]):
            out["canonical k=%d lengths=%s" % (k, lengths)] = kmc.canonical_workspace_size(_offsets(lengths), k, device)
    for n, k in ((2, 3), (6, 8), (64, 13), (1000, 4)):
        out["distances n=%d k=%d" % (n, k)] = kmc.pair_distances_workspace_size(n, k, device)
    return out


def test_workspace_sizes_match_the_recorded_ones(kmc, cuda):
    import ctypes

    import torch
    with open(GOLDEN) as f:
        gold = json.load(f)
    device = torch.cuda.current_device()
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    assert cus == gold["cus"], "the sizes were recorded on a device with %d CUs, this one has %d" % (gold["cus"], cus)
    got = compute_sizes(kmc, device)
    assert list(got) == list(gold["sizes"])
    for name, size in got.items():
        print(name, size)
        assert size == gold["sizes"][name], name
    assert all(v > 0 for n, v in got.items() if not n.startswith("distances"))
    # refused arguments give 0 (the cases of test_abi.py, here with a device behind them)
    L = kmc.lib()
    bad = np.array([0, 100, 50], dtype=np.int64)
    assert L.kmc_count_canonical_workspace_size(bad.ctypes.data_as(ctypes.c_void_p), 2, 21, device) == 0
    assert L.kmc_count_canonical_workspace_size(None, 2, 21, device) == 0
    assert L.kmc_count_canonical_workspace_size(bad.ctypes.data_as(ctypes.c_void_p), 1, 40, device) == 0
