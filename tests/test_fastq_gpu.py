"""The device FASTQ parser and the batch reader (csrc/kmc_fastq_gpu.hip): every output
bit for bit that of fastq_util.parse, the plain restatement of the record rules,
which test_fastq_util.py pins to the host FASTA loader.

T = 64 raw bytes per thread (kFpPer), B = 16384 per block (kFpTile), 256 records per
block of the validation (kFqVBlock), 4096 elements per block of the scans
(kScanTile): fastq_util.py holds them and the input builders."""
import ctypes
import os
import random
import threading

import numpy as np
import pytest

import fastq_util as Q

pytestmark = pytest.mark.gpu

KMC_OK, KMC_ERR_CAPACITY, KMC_ERR_FORMAT = 0, 1009, 1012   # include/kmc.h
SENTINEL = -0x5A5A5A5A5A5A5A5B
T, B = Q.T, Q.B


def to_device(cuda, raw):
    import torch
    if not raw:
        return torch.zeros(0, dtype=torch.uint8, device=cuda)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(cuda)


def same_as_restatement(kmc, cuda, raw, final=True, msg="", stream=None):
    """The wrapper's result against fastq_util.parse: the records and `consumed`, or the
    FormatError's record index."""
    dev = to_device(cuda, raw)
    try:
        exp = Q.parse_np(raw, final)
    except Q.FormatError as e:
        with pytest.raises(kmc.KmcError) as got:
            kmc.parse_fastq_device(dev, final, stream=stream)
        assert (got.value.code, got.value.record) == (KMC_ERR_FORMAT, e.record_index), msg
        return None
    data, idx, used = kmc.parse_fastq_device(dev, final, stream=stream)
    assert used == exp[2], msg
    np.testing.assert_array_equal(idx.cpu().numpy(), exp[1], err_msg=msg + " indices")
    np.testing.assert_array_equal(data.cpu().numpy(), exp[0], err_msg=msg + " data")
    return data, idx


def direct(kmc, raw_ptr, n, final, data_ptr, data_cap, idx_ptr, idx_cap):
    """kmc_fastq_parse_device itself: (return code, *num_seqs, *data_bytes, *consumed)."""
    import torch
    ns, nb, used = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = kmc.lib().kmc_fastq_parse_device(ctypes.c_void_p(raw_ptr), n, final, ctypes.c_void_p(data_ptr), data_cap,
                                          ctypes.c_void_p(idx_ptr), idx_cap, ctypes.byref(ns), ctypes.byref(nb),
                                          ctypes.byref(used), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, ns.value, nb.value, used.value


# a. ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(Q.EDGE_TEXTS)))
def test_edge_texts(kmc, cuda, case):
    text, final1, final0 = Q.EDGE_TEXTS[case]
    for final, exp in ((True, final1), (False, final0)):
        got = same_as_restatement(kmc, cuda, text, final, "%r final %d" % (text, final))
        if isinstance(exp, int):
            assert got is None
        else:
            seqs, used = exp
            data, idx = got
            assert idx.numel() == len(seqs) + 1 and data.cpu().numpy().tobytes() == b"".join(s + b"\0" for s in seqs)
    # more hand-written shapes of the same rules
    for text in (b"@a\nAC\n+\nII\r", b"@a\r\nAC\r\r\n+\r\nIII\r\n", b"@a\nAC\n+\nII\n\r\n\n", b"@a\n\n+\n",
                 b"@a\nAC\n+\nII\n\n\n\n\n", b"@a\nA\n+\nI\nb\nA\n+\nI\n@c\nA\n-\nI\n", b"x", b"\n\n\n", b"@\n\n+\n\n@\n\n+\n\n"):
        for final in (True, False):
            same_as_restatement(kmc, cuda, text, final, "%r final %d" % (text, final))


# b. ---------------------------------------------------------------------------
@pytest.mark.parametrize("crlf", [False, True])
def test_thread_and_tile_boundaries(kmc, cuda, crlf):
    """A 3-base sequence line starting at B - T - 2 + d for d in 0 .. 2T + 4: each of the
    record's four newlines, the '\\r', and the first and last sequence byte on every
    position around a thread edge and the tile edge (header and '+' lines are two and
    one byte from the sequence, the quality three bytes after it)."""
    for d in range(2 * T + 5):
        raw, seqs = Q.boundary_input(d, crlf)
        got = same_as_restatement(kmc, cuda, raw, True, "d=%d" % d)
        exp_data, exp_idx = Q.expected_of(seqs)
        np.testing.assert_array_equal(got[0].cpu().numpy(), exp_data)
    # not final, and cut inside the last record: four complete records
    raw, _ = Q.boundary_input(T + 1, crlf)
    same_as_restatement(kmc, cuda, raw[:-5], False, "cut")


# c. ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_short_reads():
    """70 000 reads of 0..3 bases (280 000 lines: 69 line tiles of the validation's 256
    records... and 18 scan tiles of records), one read of 100 000 bases (a line across
    six raw tiles) in the middle."""
    rng = random.Random(31)
    a, sa = Q.write_fastq(rng, 35000, lo=0, hi=3)
    long_seq, long_q = Q.random_read(rng, 100000, 100000)
    b, sb = Q.write_fastq(rng, 35000, lo=0, hi=3, final_newline=False)
    raw = a + Q.record(long_seq, long_q, b"long") + b
    return raw, Q.parse_np(raw, True), Q.parse_np(raw, False), len(sa) + 1 + len(sb)


def test_record_scan_and_line_array_boundaries(kmc, cuda, many_short_reads):
    raw, exp1, exp0, nreads = many_short_reads
    assert exp1[1].size == nreads + 1 == 70002 and exp0[1].size == nreads
    dev = to_device(cuda, raw)
    for final, exp in ((True, exp1), (False, exp0)):
        data, idx, used = kmc.parse_fastq_device(dev, final)
        assert used == exp[2]
        np.testing.assert_array_equal(idx.cpu().numpy(), exp[1])
        np.testing.assert_array_equal(data.cpu().numpy(), exp[0])


# d. ---------------------------------------------------------------------------
def plant(raw, seqs_before, kind):
    """raw with the record that follows `seqs_before` records broken (raw holds '\\n' lines)."""
    lines = raw.split(b"\n")
    at = 4 * seqs_before
    if kind == "header":
        lines[at] = b"x" + lines[at][1:]
    elif kind == "plus":
        lines[at + 2] = b"-" + lines[at + 2][1:]
    else:
        lines[at + 3] = lines[at + 3] + b"I"
    return b"\n".join(lines)


@pytest.mark.parametrize("second,kind", [(4097, "header"), (4097, "length"), (1800, "plus")])
def test_first_bad_record_is_the_smallest(kmc, cuda, second, kind):
    """Violations at records `second` and 311 (4097: another block of the validation and
    another raw tile; 1800: another tile's line range): 311 is reported, and nothing
    is written to data or indices."""
    import torch
    rng = random.Random(4)
    raw, seqs = Q.write_fastq(rng, 5000, lo=0, hi=120)
    lines_per_tile = raw[:B].count(b"\n")
    assert 4 * 311 // lines_per_tile != 4 * second // lines_per_tile
    bad = plant(plant(raw, second, kind), 311, "length" if kind == "header" else "header")
    with pytest.raises(Q.FormatError) as e:
        Q.parse(bad)
    assert e.value.record_index == 311
    n = len(bad)
    dev = to_device(cuda, bad + bytes(-n % 16))
    cap = (n // 2 + 1 + 3) & ~3
    for final in (1, 0):
        data = torch.full((cap + 4096,), 0xA5, dtype=torch.uint8, device=cuda)
        idx = torch.full((5001 + 16,), SENTINEL, dtype=torch.int64, device=cuda)
        rc, ns, _, _ = direct(kmc, dev.data_ptr(), n, final, data.data_ptr(), cap, idx.data_ptr(), 5001)
        assert (rc, ns) == (KMC_ERR_FORMAT, 311)
        assert (data.cpu().numpy() == 0xA5).all() and (idx.cpu().numpy() == SENTINEL).all()
    # the second one alone is found too, and a clean parse leaves the guard region alone
    with pytest.raises(kmc.KmcError) as got:
        kmc.parse_fastq_device(to_device(cuda, plant(raw, second, kind)))
    assert got.value.record == second
    exp_data, exp_idx, _ = Q.parse_np(raw)
    dev = to_device(cuda, raw + bytes(-len(raw) % 16))
    cap = len(raw) // 2 + 1
    data = torch.full(((cap + 3 & ~3) + 4096,), 0xA5, dtype=torch.uint8, device=cuda)
    idx = torch.full((5001 + 16,), SENTINEL, dtype=torch.int64, device=cuda)
    rc, ns, nb, used = direct(kmc, dev.data_ptr(), len(raw), 1, data.data_ptr(), cap, idx.data_ptr(), 5001)
    assert (rc, ns, nb, used) == (KMC_OK, 5000, exp_data.size, len(raw))
    data, idx = data.cpu().numpy(), idx.cpu().numpy()
    np.testing.assert_array_equal(data[:nb], exp_data)
    np.testing.assert_array_equal(idx[:5001], exp_idx)
    assert (data[nb:] == 0xA5).all() and (idx[5001:] == SENTINEL).all()


# e. ---------------------------------------------------------------------------
def test_capacity(kmc, cuda):
    import torch
    rng = random.Random(9)
    raw, seqs = Q.write_fastq(rng, 40, lo=0, hi=50)
    exp_data, exp_idx, _ = Q.parse_np(raw)
    n = len(raw)
    dev = to_device(cuda, raw + bytes(-n % 16))
    data = torch.zeros(n // 2 + 17, dtype=torch.uint8, device=cuda)
    idx = torch.full((64,), SENTINEL, dtype=torch.int64, device=cuda)
    rc, ns, _, _ = direct(kmc, dev.data_ptr(), n, 1, data.data_ptr(), n // 2 + 1, idx.data_ptr(), 40)
    assert (rc, ns) == (KMC_ERR_CAPACITY, 40)
    assert (idx.cpu().numpy() == SENTINEL).all() and not data.cpu().numpy().any()
    rc, ns, nb, used = direct(kmc, dev.data_ptr(), n, 1, data.data_ptr(), n // 2 + 1, idx.data_ptr(), 41)
    assert (rc, ns, nb, used) == (KMC_OK, 40, exp_data.size, n)
    np.testing.assert_array_equal(idx.cpu().numpy()[:41], exp_idx)
    assert (idx.cpu().numpy()[41:] == SENTINEL).all()
    # raw_bytes = 0
    idx.fill_(SENTINEL)
    rc, ns, nb, used = direct(kmc, None, 0, 1, None, 0, idx.data_ptr(), 1)
    assert (rc, ns, nb, used) == (KMC_OK, 0, 0, 0)
    got = idx.cpu().numpy()
    assert got[0] == 0 and (got[1:] == SENTINEL).all()


# f. ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads300():
    rng = random.Random(300)
    return Q.write_fastq(rng, 300, lo=0, hi=200)


def read_all(kmc, path, batch, copy=True):
    """The batches of a reader, concatenated with the offsets rebased: (data, idx, batches)."""
    datas, idxs, base, batches = [], [np.zeros(1, dtype=np.int64)], 0, 0
    with kmc.FastqReader(str(path), batch, copy=copy) as rd:
        for data, idx in rd:
            d, i = data.cpu().numpy(), idx.cpu().numpy()
            assert i[0] == 0 and i[-1] == d.size
            datas.append(d)
            idxs.append(i[1:] + base)
            base += d.size
            batches += 1
        for _ in range(3):  # after the end: the end marker, again and again
            assert rd.next_batch() is None
    return np.concatenate(datas) if datas else np.zeros(0, np.uint8), np.concatenate(idxs), batches


@pytest.mark.parametrize("shape", ["plain", "no_final_newline", "blank_lines", "crlf"])
def test_reader_batches_equal_one_parse(kmc, cuda, tmp_path, shape):
    rng = random.Random(301)
    kw = {"plain": {}, "no_final_newline": {"final_newline": False}, "blank_lines": {"blank_lines": 3},
          "crlf": {"crlf": True, "final_newline": False}}[shape]
    raw, seqs = Q.write_fastq(rng, 300, lo=0, hi=200, **kw)
    path = tmp_path / "reads.fq"
    path.write_bytes(raw)
    exp_data, exp_idx, _ = Q.parse_np(raw)
    counts = {}
    for batch in (16, 64, 4096, 0):
        data, idx, counts[batch] = read_all(kmc, path, batch, copy=batch != 4096)
        np.testing.assert_array_equal(idx, exp_idx, err_msg="batch %d" % batch)
        np.testing.assert_array_equal(data, exp_data, err_msg="batch %d" % batch)
    assert counts[0] == 1 and counts[4096] >= len(raw) // 4200 and counts[16] > counts[4096]
    # the whole-file loader, and its plain truncation
    data, idx = kmc.load_fastq_device(str(path))
    np.testing.assert_array_equal(idx.cpu().numpy(), exp_idx)
    np.testing.assert_array_equal(data.cpu().numpy(), exp_data)
    data, idx = kmc.load_fastq_device(str(path), 7)
    np.testing.assert_array_equal(idx.cpu().numpy(), exp_idx[:8])
    np.testing.assert_array_equal(data.cpu().numpy(), exp_data[:exp_idx[7]])


def test_reader_truncated_record_and_empty_file(kmc, cuda, tmp_path, reads300):
    raw, seqs = reads300
    cut = raw[:raw.rindex(b"\n+")]  # the last record loses its '+' and quality lines
    with pytest.raises(Q.FormatError) as e:
        Q.parse(cut)
    assert e.value.record_index == 299
    path = tmp_path / "cut.fq"
    path.write_bytes(cut)
    for batch in (64, 4096, 0):
        with kmc.FastqReader(str(path), batch) as rd:
            with pytest.raises(kmc.KmcError) as got:
                for _ in rd:
                    pass
            assert (got.value.code, got.value.record) == (KMC_ERR_FORMAT, 299)
            with pytest.raises(kmc.KmcError) as again:   # a failed reader stays failed
                rd.next_batch()
            assert again.value.record == 299
    with pytest.raises(kmc.KmcError) as got:
        kmc.load_fastq_device(str(path))
    assert (got.value.code, got.value.record) == (KMC_ERR_FORMAT, 299)
    # a record broken in the middle of the file: its index within the whole file
    bad = tmp_path / "bad.fq"
    bad.write_bytes(plant(raw, 150, "plus"))
    with kmc.FastqReader(str(bad), 1024) as rd:
        with pytest.raises(kmc.KmcError) as got:
            for _ in rd:
                pass
        assert got.value.record == 150
    empty = tmp_path / "empty.fq"
    empty.write_bytes(b"")
    data, idx, batches = read_all(kmc, empty, 64)
    assert data.size == 0 and idx.tolist() == [0] and batches == 1


def test_reader_on_a_pipe(kmc, cuda, reads300):
    raw, seqs = reads300
    exp_data, exp_idx, _ = Q.parse_np(raw)
    r, w = os.pipe()

    def feed():
        with os.fdopen(w, "wb") as f:
            for a in range(0, len(raw), 1000):   # short writes: read() returns pieces
                f.write(raw[a:a + 1000])
                f.flush()

    th = threading.Thread(target=feed)
    th.start()
    try:
        data, idx, batches = read_all(kmc, "/dev/fd/%d" % r, 4096)
    finally:
        th.join()
        os.close(r)
    np.testing.assert_array_equal(idx, exp_idx)
    np.testing.assert_array_equal(data, exp_data)
    assert batches >= len(raw) // 4200


# g. ---------------------------------------------------------------------------
def test_stream_order_count_per_batch(kmc, cuda, tmp_path, reads300):
    """The consumer enqueues sketch_screen_count on each batch (the reader's own
    buffers) on a side stream and synchronises only after the last batch: the next
    call's writes are ordered behind the count."""
    import torch
    raw, seqs = reads300
    path = tmp_path / "reads.fq"
    path.write_bytes(raw)
    k, s = 11, 64
    data, idx, _ = kmc.parse_fastq_device(to_device(cuda, raw))
    nrefs = 40
    ridx = idx[:nrefs + 1].clone()
    rows, sizes = kmc.sketch_from_sequences(data, ridx, k, s, data_bytes=int(ridx[-1]))
    whole = kmc.sketch_screen_build(rows, sizes)
    kmc.sketch_screen_count(whole, data, idx, k)
    exp = [t.cpu().numpy() for t in kmc.sketch_screen_results(whole, rows, sizes, k)]
    assert exp[0].max() > 0
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    index = kmc.sketch_screen_build(rows, sizes, stream=side)
    batches = 0
    with kmc.FastqReader(str(path), 4096, stream=side, copy=False) as rd:
        for bdata, bidx in rd:
            kmc.sketch_screen_count(index, bdata, bidx, k, stream=side)
            batches += 1
        got = kmc.sketch_screen_results(index, rows, sizes, k, stream=side)
        side.synchronize()
    assert batches > 5
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g.cpu().numpy(), e)


# h. ---------------------------------------------------------------------------
def test_parse_then_count(kmc, oracle, cuda):
    import torch
    rng = random.Random(50)
    raw, seqs = Q.write_fastq(rng, 50, lo=0, hi=300)
    exp_data, exp_idx, _ = Q.parse_np(raw)
    data, idx, _ = kmc.parse_fastq_device(to_device(cuda, raw))
    out, inv = kmc.count_dense(data, idx, 8, invalid=True)
    torch.cuda.synchronize()
    exp, exp_inv = oracle.count_dense(exp_data, exp_idx, 8)
    np.testing.assert_array_equal(out.cpu().numpy(), exp)
    np.testing.assert_array_equal(inv.cpu().numpy(), exp_inv)


def test_side_stream_and_workspace_reuse(kmc, cuda, many_short_reads):
    """A small parse after a large one, then large again (the grow-only scratch), on a
    side stream (the wrapper's padding copy is ordered before the kernels)."""
    import torch
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        for raw in (many_short_reads[0][:200000], b"@h\nAC\n+\nII\n", b"", Q.boundary_input(5)[0]):
            same_as_restatement(kmc, cuda, raw, False, stream=s)
    s.synchronize()
