"""The device FASTA parser (csrc/kmc_fasta_gpu.hip) at its tile, thread and scan
boundaries: every result bit-exact, data and indices, against the host loader
kmc_fasta_load (uncapped), which test_loader.py pins to the reference and
test_fasta_util.py pins to a plain restatement on exactly these inputs.

Sizes follow the constants of the source (kFpPer 64, kFpTile 16384, kLsPer 16,
kLsTile 4096, kFpBlock 256, kScanTile 4096, kChunk 64 MiB); fasta_util.py holds
them and the input builders."""
import ctypes

import numpy as np
import pytest

import fasta_util as F

pytestmark = pytest.mark.gpu

KMC_OK, KMC_ERR_INVALID_ARG, KMC_ERR_ALIGNMENT, KMC_ERR_CAPACITY = 0, 1001, 1003, 1009   # include/kmc.h
SENTINEL = -0x5A5A5A5A5A5A5A5B


def host_expected(kmc, tmp_path, raw):
    """[(data, indices)] of the host loader for dialects 0 and 1."""
    path = str(tmp_path / "h.fa")
    with open(path, "wb") as f:
        f.write(raw)
    return [kmc.load_fasta(path, dialect, 0)[:2] for dialect in (0, 1)]


def to_device(cuda, raw):
    import torch
    if not raw:
        return torch.zeros(0, dtype=torch.uint8, device=cuda)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(cuda)


def same_as_host(kmc, cuda, tmp_path, raw, msg="", stream=None):
    exp = host_expected(kmc, tmp_path, raw)
    dev = to_device(cuda, raw)
    for dialect in (0, 1):
        data, idx = kmc.parse_fasta_device(dev, dialect, stream=stream)
        np.testing.assert_array_equal(idx.cpu().numpy(), exp[dialect][1], err_msg="%s dialect %d indices" % (msg, dialect))
        np.testing.assert_array_equal(data.cpu().numpy(), exp[dialect][0], err_msg="%s dialect %d data" % (msg, dialect))


def direct(kmc, raw_ptr, n, dialect, data_ptr, data_cap, idx_ptr, idx_cap):
    """kmc_fasta_parse_device itself, without the wrapper's padding and retry:
    (return code, *num_seqs, *data_bytes)."""
    import torch
    ns, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = kmc.lib().kmc_fasta_parse_device(ctypes.c_void_p(raw_ptr), n, dialect, ctypes.c_void_p(data_ptr), data_cap,
                                          ctypes.c_void_p(idx_ptr), idx_cap, ctypes.byref(ns), ctypes.byref(nb),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, ns.value, nb.value


# a. ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(F.MOTIFS))
def test_motifs_on_thread_and_tile_boundaries(kmc, cuda, tmp_path, name):
    """Every byte of the motif at B - 1, B, B + 1 for B in {64, 128, 16384 - 64,
    16384, 32768, 3 * 16384}, after an open record and after none: walk()'s
    line-start rule at a thread's and a tile's first byte."""
    for cid, raw in F.motif_cases(name):
        same_as_host(kmc, cuda, tmp_path, raw, cid)


# b. ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,ending", F.SIZE_CASES)
def test_file_sizes(kmc, cuda, tmp_path, n, ending):
    same_as_host(kmc, cuda, tmp_path, F.size_input(n, ending), "%d %s" % (n, ending))


# c. ---------------------------------------------------------------------------
TRAILER = (b"\n>x\nACGT\n\n>y\nTT" * 6)[:80]


@pytest.mark.parametrize("which", ["n17", "n65", "n16385", "n49151", "motif"])
def test_bytes_after_raw_bytes_are_ignored(kmc, cuda, tmp_path, which):
    """raw inside a larger device buffer, followed by more FASTA text; n is no
    multiple of 16, so load64's byte-wise tail decides what is read."""
    import torch
    raw = {"n17": lambda: F.size_input(17, "base"), "n65": lambda: F.size_input(65, "base"),
           "n16385": lambda: F.size_input(F.FP_TILE + 1, "nl"), "n49151": lambda: F.size_input(3 * F.FP_TILE - 1, "base"),
           "motif": lambda: F.one_motif_input("nl_header", F.FP_TILE, 1)}[which]()
    n = len(raw)
    assert n % 64 and n % 16 and len(TRAILER) == 80
    exp = host_expected(kmc, tmp_path, raw)
    buf = to_device(cuda, raw + TRAILER + bytes(16))
    for dialect in (0, 1):
        data = torch.empty(n + 16, dtype=torch.uint8, device=cuda)
        idx = torch.empty(exp[dialect][1].size, dtype=torch.int64, device=cuda)
        rc, ns, nb = direct(kmc, buf.data_ptr(), n, dialect, data.data_ptr(), n + 16, idx.data_ptr(), idx.numel())
        assert (rc, ns, nb) == (KMC_OK, exp[dialect][1].size - 1, exp[dialect][0].size)
        np.testing.assert_array_equal(idx.cpu().numpy(), exp[dialect][1])
        np.testing.assert_array_equal(data[:nb].cpu().numpy(), exp[dialect][0])


# d. ---------------------------------------------------------------------------
def nothing_past_the_end(kmc, cuda, tmp_path, raw, msg):
    import torch
    n = len(raw)
    exp = host_expected(kmc, tmp_path, raw)
    dev = to_device(cuda, raw + bytes(-n % 16))
    cap = (n + 1 + 3) & ~3
    for dialect in (0, 1):
        exp_data, exp_idx = exp[dialect]
        data = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=cuda)
        idx = torch.full((exp_idx.size + 16,), SENTINEL, dtype=torch.int64, device=cuda)
        rc, ns, nb = direct(kmc, dev.data_ptr(), n, dialect, data.data_ptr(), cap, idx.data_ptr(), exp_idx.size)
        assert (rc, ns, nb) == (KMC_OK, exp_idx.size - 1, exp_data.size), msg
        data, idx = data.cpu().numpy(), idx.cpu().numpy()
        np.testing.assert_array_equal(data[:nb], exp_data, err_msg=msg)
        np.testing.assert_array_equal(idx[:ns + 1], exp_idx, err_msg=msg)
        assert (data[nb:] == 0xA5).all(), "%s dialect %d: bytes written at or after *data_bytes" % (msg, dialect)
        assert (idx[ns + 1:] == SENTINEL).all(), "%s dialect %d: indices written after [num_seqs]" % (msg, dialect)


@pytest.mark.parametrize("t,r", F.KEEP_CASES)
def test_nothing_past_the_end_tile_keeping(kmc, cuda, tmp_path, t, r):
    nothing_past_the_end(kmc, cuda, tmp_path, F.tile_keeping(t, r), "keep %d %d" % (t, r))


@pytest.mark.parametrize("name,at,j", [("nl_header", F.FP_TILE, 0), ("base_eof", 3 * F.FP_TILE - 1, 0)])
def test_nothing_past_the_end_motifs(kmc, cuda, tmp_path, name, at, j):
    nothing_past_the_end(kmc, cuda, tmp_path, F.one_motif_input(name, at, j), name)


# e. ---------------------------------------------------------------------------
@pytest.mark.parametrize("t,r", F.KEEP_CASES)
def test_tile_keeping(kmc, cuda, tmp_path, t, r):
    """Tile 1 keeps t bytes at an output offset = r (mod 4): fp_write_kernel's head
    and tail bytes, a tile inside one output dword, neighbours sharing a dword."""
    same_as_host(kmc, cuda, tmp_path, F.tile_keeping(t, r), "keep %d %d" % (t, r))


@pytest.mark.parametrize("name", F.DROPPED_TILE_CASES)
def test_wholly_dropped_tiles(kmc, cuda, tmp_path, name):
    same_as_host(kmc, cuda, tmp_path, F.dropped_tile_input(name), name)


# f. ---------------------------------------------------------------------------
def test_every_byte_value(kmc, cuda, tmp_path):
    """nl_bits (a carry trick) and walk (byte compares) agree on every byte value."""
    same_as_host(kmc, cuda, tmp_path, F.byte_values_input(), "byte values")


# g. ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.CARRY_CASES)
def test_line_scan_carry(kmc, cuda, tmp_path, name):
    """More than 256 line tiles: fp_lscan_top_kernel's carry into its second round."""
    same_as_host(kmc, cuda, tmp_path, F.carry_input(name), name)


# h. ---------------------------------------------------------------------------
def test_load_device_above_128_mib(kmc, cuda, tmp_path):
    """Three staging chunks (the first pinned buffer reused behind its event) and
    8194 raw tiles: three scan tiles, bsum carrying between them in all three scans."""
    import torch
    path = str(tmp_path / "big.fa")
    F.write_big(path, F.BIG_BYTES)
    exp_data, exp_idx, _ = kmc.load_fasta(path, 0, 0)
    data, idx = kmc.load_fasta_device(path, 0, 0)
    torch.cuda.synchronize()
    assert idx.numel() == exp_idx.size and data.numel() == exp_data.size
    np.testing.assert_array_equal(idx.cpu().numpy(), exp_idx)
    exp_dev = torch.from_numpy(exp_data).to(cuda)
    if not torch.equal(data, exp_dev):
        first = int(torch.nonzero(data != exp_dev)[0])
        pytest.fail("data differs from the host loader, first at output byte %d" % first)
    del data, idx, exp_dev, exp_data
    exp_data, exp_idx, _ = kmc.load_fasta(path, 1, 0)
    data, idx = kmc.load_fasta_device(path, 1, 0)
    torch.cuda.synchronize()
    assert (idx.numel(), data.numel()) == (exp_idx.size, exp_data.size)


# i. ---------------------------------------------------------------------------
def test_workspace_reuse_small_after_large(kmc, cuda, tmp_path):
    """The grow-only workspaces: a small parse after a large one, then large again."""
    big = F.carry_input("open_across")
    for k, raw in enumerate((big, b">h\nAC\nGT\nA\n", b"\n\n\n", b"", big)):
        same_as_host(kmc, cuda, tmp_path, raw, "parse %d" % k)


# j. ---------------------------------------------------------------------------
def test_side_stream(kmc, cuda, tmp_path):
    """The wrapper's stream= argument: the side stream is also made current, so
    the wrapper's own padding copy is ordered before the kernels."""
    import torch
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        same_as_host(kmc, cuda, tmp_path, F.one_motif_input("nl_cr_text", 2 * F.FP_TILE, 2), "side stream", stream=s)
    s.synchronize()


# k. ---------------------------------------------------------------------------
def test_abi_errors(kmc, cuda, tmp_path):
    import torch
    raw = b">a\nACGT\nAC\n\n>b\nT|T\n>c\nG"
    n = len(raw)
    exp = host_expected(kmc, tmp_path, raw)
    dev = to_device(cuda, raw + bytes(32))
    data = torch.zeros(n + 32, dtype=torch.uint8, device=cuda)
    idx = torch.full((16,), SENTINEL, dtype=torch.int64, device=cuda)
    R, D, I = dev.data_ptr(), data.data_ptr(), idx.data_ptr()
    assert direct(kmc, R, n, 2, D, n + 16, I, 16)[0] == KMC_ERR_INVALID_ARG
    assert direct(kmc, R + 1, n, 0, D, n + 16, I, 16)[0] == KMC_ERR_ALIGNMENT
    assert direct(kmc, R, n, 0, D + 1, n + 16, I, 16)[0] == KMC_ERR_ALIGNMENT
    assert direct(kmc, R, n, 0, D, n, I, 16)[0] == KMC_ERR_CAPACITY
    assert direct(kmc, R, n, 0, D, n + 16, None, 16)[0] == KMC_ERR_INVALID_ARG
    assert (idx.cpu().numpy() == SENTINEL).all() and not data.cpu().numpy().any()   # refused calls write nothing
    for dialect in (0, 1):
        exp_data, exp_idx = exp[dialect]
        nrec = exp_idx.size - 1
        assert nrec == (2, 3)[dialect]
        idx.fill_(SENTINEL)
        rc, ns, _ = direct(kmc, R, n, dialect, D, n + 16, I, nrec)
        assert (rc, ns) == (KMC_ERR_CAPACITY, nrec)
        assert (idx.cpu().numpy() == SENTINEL).all()
        rc, ns, nb = direct(kmc, R, n, dialect, D, n + 16, I, nrec + 1)
        assert (rc, ns, nb) == (KMC_OK, nrec, exp_data.size)
        np.testing.assert_array_equal(idx.cpu().numpy()[:nrec + 1], exp_idx)
        assert (idx.cpu().numpy()[nrec + 1:] == SENTINEL).all()
        np.testing.assert_array_equal(data.cpu().numpy()[:nb], exp_data)
    # raw_bytes = 0
    idx.fill_(SENTINEL)
    for args in ((R, D), (None, None)):
        idx[0] = SENTINEL
        rc, ns, nb = direct(kmc, args[0], 0, 0, args[1], 0, I, 1)
        assert (rc, ns, nb) == (KMC_OK, 0, 0)
        got = idx.cpu().numpy()
        assert got[0] == 0 and (got[1:] == SENTINEL).all()
