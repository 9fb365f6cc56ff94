"""Caller workspaces at the edges of what the bind step (csrc/kmc_workspace.h)
accepts, for the entry points whose own tests do not pin them already
(test_sparse_caller_workspace, test_sketch_caller_workspace, test_seq_caller_workspace
and test_canonical_unaligned_data_and_caller_workspace hold the others): a
workspace of exactly the queried size gives the result of the library's own
buffer, one byte less is KMC_ERR_WORKSPACE, and a workspace 8 bytes into a larger
tensor is refused by the canonical counter (KMC_ERR_ALIGNMENT) and taken by the
direct sketcher.  The codes are read from include/kmc.h.
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


_codes = {}


def err(kmc, name):
    """The value of an error code of include/kmc.h (the header is read once)."""
    if not _codes:
        with open(kmc.HEADER) as f:
            _codes.update((n, int(v)) for n, v in re.findall(r"\b(KMC_ERR_\w+)\s*=\s*(\d+)", f.read()))
    assert name in _codes, "%s is not an enumerator of kmc.h" % name
    return _codes[name]


def records(seed, lengths):
    """ACGT records with a few N, each followed by its 0 terminator."""
    rng = np.random.default_rng(seed)
    parts = [np.append(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=n, p=[.24, .24, .24, .24, .04]),
                       np.uint8(0)) for n in lengths]
    idx = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return np.concatenate(parts), idx


def dev(x, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def refused(kmc, code, call):
    import torch
    with pytest.raises(kmc.KmcError) as ei:
        call()
        torch.cuda.synchronize()
    assert ei.value.code == code


@pytest.mark.parametrize("k", [8, 11])  # the packed dense kernel and the radix path
def test_count_dense_caller_workspace(kmc, oracle, cuda, k):
    import torch
    data, idx = records(80 + k, [5000, 3, 70001, 1025])
    d, di = dev(data, cuda), dev(idx, cuda)
    exp, _ = oracle.count_dense(data, idx, k)
    out = torch.empty((1 << (2 * k), idx.size - 1), dtype=torch.int32, device=cuda)
    # kmc_count_dense is kmc_count_dense_ex over [0, data_bytes): the _ex query is its exact size
    need = kmc.dense_ex_workspace_size(kmc.dense_args(d, di, k, out), torch.cuda.current_device())
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
    got, _ = kmc.count_dense(d, di, k, workspace=ws, out=out)
    kmc.dense_status_check()
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    refused(kmc, err(kmc, "KMC_ERR_WORKSPACE"), lambda: kmc.count_dense(d, di, k, workspace=ws[: need - 1], out=out))


def test_pair_distances_split_caller_workspace(kmc, cuda):
    """k = 13 with three records: the bin axis is split, the only plan with a workspace."""
    import torch
    n, k = 3, 13
    nb = 1 << (2 * k)
    gen = torch.Generator(device=cuda).manual_seed(13)
    counts = torch.zeros((nb, n), dtype=torch.int32, device=cuda)
    hot = torch.randint(0, nb, (100_000,), generator=gen, device=cuda)
    for s in range(n):  # overlapping windows of the hot codes: every pair shares some
        mine = hot[20_000 * s: 20_000 * s + 60_000]
        counts[mine, s] = torch.randint(1, 9, mine.shape, generator=gen, device=cuda, dtype=torch.int32)
    lens = counts.sum(dim=0, dtype=torch.int64) + k - 1
    di = torch.cat([torch.zeros(1, dtype=torch.int64, device=cuda), torch.cumsum(lens + 1, 0)])
    need = kmc.pair_distances_workspace_size(n, k, torch.cuda.current_device())
    assert need == 8 * n * (n - 1) // 2
    exp = kmc.pair_distances(counts, di, k)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
    got = kmc.pair_distances(counts, di, k, workspace=ws)
    torch.cuda.synchronize()
    assert ((exp > 0) & (exp < 1)).all()
    assert torch.equal(got, exp)
    refused(kmc, err(kmc, "KMC_ERR_WORKSPACE"), lambda: kmc.pair_distances(counts, di, k, workspace=ws[: need - 1]))


def test_canonical_workspace_one_byte_short_or_shifted(kmc, cuda):
    import torch
    data, idx = records(21, [0, 5, 4000, 1, 3333, 64])
    d, di = dev(data, cuda), dev(idx, cuda)
    need = kmc.canonical_workspace_size(idx, 21, torch.cuda.current_device())
    assert need > 0
    big = torch.empty(need + 256, dtype=torch.uint8, device=cuda)
    assert big.data_ptr() % 256 == 0
    exp = kmc.count_canonical(d, di, 21, workspace=big[:need])
    torch.cuda.synchronize()
    assert exp[0].numel() > 0
    refused(kmc, err(kmc, "KMC_ERR_WORKSPACE"), lambda: kmc.count_canonical(d, di, 21, workspace=big[: need - 1]))
    # large enough, but not on a 256-byte boundary
    refused(kmc, err(kmc, "KMC_ERR_ALIGNMENT"), lambda: kmc.count_canonical(d, di, 21, workspace=big[8: 8 + need]))
    # size is checked before alignment
    refused(kmc, err(kmc, "KMC_ERR_WORKSPACE"), lambda: kmc.count_canonical(d, di, 21, workspace=big[8: 7 + need]))


def test_sketch_from_sequences_takes_a_workspace_shifted_by_8(kmc, cuda):
    import torch
    data, idx = records(15, [700, 0, 2500, 14, 1201])
    d, di = dev(data, cuda), dev(idx, cuda)
    need = kmc.sketch_from_sequences_workspace_size(idx.size - 1, data.size, 16, torch.cuda.current_device())
    assert need > 0
    big = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=cuda)
    assert big.data_ptr() % 256 == 0
    rows, sizes = kmc.sketch_from_sequences(d, di, 15, 16, workspace=big[:need])
    srows, ssizes = kmc.sketch_from_sequences(d, di, 15, 16, workspace=big[8: 8 + need])
    torch.cuda.synchronize()
    assert int(sizes.max()) == 16 and int(sizes.min()) == 0
    assert torch.equal(srows, rows) and torch.equal(ssizes, sizes)
    # not a multiple of 8: refused, after the size check
    refused(kmc, err(kmc, "KMC_ERR_ALIGNMENT"),
            lambda: kmc.sketch_from_sequences(d, di, 15, 16, workspace=big[4: 4 + need]))
    refused(kmc, err(kmc, "KMC_ERR_WORKSPACE"),
            lambda: kmc.sketch_from_sequences(d, di, 15, 16, workspace=big[4: 3 + need]))
