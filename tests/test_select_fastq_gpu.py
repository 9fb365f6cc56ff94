"""Where a record's raw text is (kmc_fastq_parse_device_ex, the reader with
KMC_FASTQ_KEEP_RAW), the selection rule on the device (kmc_match_select) and the three
calls chained: match, select, compaction."""
import ctypes
import random

import numpy as np
import pytest

import fastq_util as Q
import select_util as S
from test_fastq_gpu import to_device

pytestmark = pytest.mark.gpu

FORMAT = 1012


def texts():
    """(name, raw, final): '\\n' and '\\r\\n' files, with and without a final newline, with
    trailing blank lines, and a piece that ends in an unfinished record."""
    out = []
    for crlf in (False, True):
        for final_newline in (True, False):
            raw, _ = Q.write_fastq(random.Random(3), 90, 0, 300, crlf=crlf, final_newline=final_newline)
            out.append(("crlf=%d newline=%d" % (crlf, final_newline), raw, True))
        raw, _ = Q.write_fastq(random.Random(4), 90, 0, 300, crlf=crlf, blank_lines=3)
        out.append(("crlf=%d blank lines" % crlf, raw, True))
        raw, _ = Q.write_fastq(random.Random(5), 90, 0, 300, crlf=crlf)
        out.append(("crlf=%d unfinished" % crlf, raw + b"@next\r\nACGT\n+", False))
        out.append(("crlf=%d unfinished, final bytes of a line" % crlf, raw[:-1 - crlf], False))
    out.append(("empty", b"", True))
    out.append(("no complete record", b"@r\nAC\n+\nII", False))
    return out


TEXTS = texts()


@pytest.mark.parametrize("case", range(len(TEXTS)), ids=[t[0] for t in TEXTS])
def test_raw_indices_equal_the_model(kmc, cuda, case):
    name, raw, final = TEXTS[case]
    assert len(raw) > S.B or len(raw) < 20
    dev = to_device(cuda, raw)
    data, idx, used, ridx = kmc.parse_fastq_device(dev, final, raw_indices=True)
    exp = S.raw_offsets(raw, final)
    got = ridx.cpu().numpy()
    np.testing.assert_array_equal(got, exp, err_msg=name)
    e_data, e_idx, e_used = Q.parse_np(raw, final)
    assert used == e_used and (got[-1] == used or (final and raw.rstrip(b"\r\n") != raw))
    # record r's text holds its four lines: the sequence is the one the parser gave
    seqs = data.cpu().numpy().tobytes().split(b"\0")[:-1] if len(e_idx) > 1 else []
    for r in (0, len(seqs) // 2, len(seqs) - 1) if seqs else ():
        lines = raw[got[r]:got[r + 1]].split(b"\n")
        assert lines[0][:1] == b"@" and lines[1].rstrip(b"\r") == seqs[r] and lines[2][:1] == b"+", (name, r)
    # with raw_indices == NULL every output is kmc_fastq_parse_device's, bit for bit
    plain = kmc.parse_fastq_device(dev, final)
    assert plain[2] == used
    np.testing.assert_array_equal(plain[0].cpu().numpy(), data.cpu().numpy())
    np.testing.assert_array_equal(plain[1].cpu().numpy(), idx.cpu().numpy())
    np.testing.assert_array_equal(idx.cpu().numpy(), e_idx)
    np.testing.assert_array_equal(data.cpu().numpy(), e_data)


def test_null_raw_indices_is_the_plain_call(kmc, cuda):
    """kmc_fastq_parse_device_ex(..., NULL) against kmc_fastq_parse_device on the same
    buffers: the same counts, consumed, data and indices."""
    import torch
    raw, _ = Q.write_fastq(random.Random(6), 200, 0, 300)
    raw += b"@unfinished\nAC"
    dev = to_device(cuda, raw + b"\0" * 16)
    L = kmc.lib()
    outs = []
    for ex in (False, True):
        data = torch.full((len(raw) // 2 + 17,), 0x5A, dtype=torch.uint8, device=cuda)
        idx = torch.full((400,), -7, dtype=torch.int64, device=cuda)
        ns, nb, used = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        args = [kmc._dptr(dev), len(raw), 0, kmc._dptr(data), len(raw) // 2 + 1, kmc._dptr(idx), 400, ctypes.byref(ns),
                ctypes.byref(nb), ctypes.byref(used)]
        rc = L.kmc_fastq_parse_device_ex(*args, None, kmc._stream(None)) if ex else \
            L.kmc_fastq_parse_device(*args, kmc._stream(None))
        torch.cuda.synchronize()
        outs.append((rc, ns.value, nb.value, used.value, data.cpu().numpy(), idx.cpu().numpy()))
    assert outs[0][:4] == outs[1][:4] == (0, 200, outs[0][2], len(raw) - len(b"@unfinished\nAC"))
    np.testing.assert_array_equal(outs[0][4], outs[1][4])
    np.testing.assert_array_equal(outs[0][5], outs[1][5])


@pytest.mark.parametrize("bad", [0, 77, 199])
def test_malformed_input_gives_the_same_code_and_index(kmc, cuda, bad):
    raw, seqs = Q.write_fastq(random.Random(7), 200, 1, 300, trap=False)
    at = S.raw_offsets(raw)[bad]
    broken = raw[:at] + b"#" + raw[at + 1:]  # the record's '@'
    for raw_indices in (False, True):
        with pytest.raises(kmc.KmcError) as e:
            kmc.parse_fastq_device(to_device(cuda, broken), True, raw_indices=raw_indices)
        assert (e.value.code, e.value.record) == (FORMAT, bad)


def batches(kmc, path, batch, keep_raw):
    """[(data, indices, raw text of the batch's records or None)] as host values."""
    out = []
    with kmc.FastqReader(str(path), batch, copy=False, keep_raw=keep_raw) as rd:
        for data, idx in rd:
            text = None
            if keep_raw:
                raw, ridx = rd.raw()
                r = ridx.cpu().numpy()
                assert r.size == idx.numel() and r[0] == 0 and raw.numel() == r[-1]
                text = raw.cpu().numpy().tobytes()
                np.testing.assert_array_equal(r, S.raw_offsets(text, True)[:r.size])
            out.append((data.cpu().numpy().copy(), idx.cpu().numpy().copy(), text))
        if keep_raw:
            assert rd.raw() is None  # after the last batch
    return out


@pytest.mark.parametrize("crlf,final_newline", [(False, True), (True, True), (False, False)])
def test_reader_keeps_the_raw_text_of_every_batch(kmc, cuda, tmp_path, crlf, final_newline):
    raw, _ = Q.write_fastq(random.Random(8), 40, 20, 150, crlf=crlf, final_newline=final_newline)
    path = tmp_path / "reads.fq"
    path.write_bytes(raw)
    with_raw, without = batches(kmc, path, 2048, True), batches(kmc, path, 2048, False)
    assert len(with_raw) == len(without) >= 3
    assert b"".join(b[2] for b in with_raw) == raw
    for a, b in zip(with_raw, without):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


def test_reader_raw_of_a_file_with_blank_lines_at_the_end(kmc, cuda, tmp_path):
    raw, _ = Q.write_fastq(random.Random(9), 10, 20, 150, blank_lines=2)
    path = tmp_path / "reads.fq"
    path.write_bytes(raw)
    got = batches(kmc, path, 1 << 20, True)
    assert len(got) == 1 and got[0][2] == raw[:-2]  # the blank lines belong to no record


def test_match_select_equals_the_host_expression(kmc, cuda):
    import torch
    rng = np.random.default_rng(50)
    n = 5000
    smp = rng.integers(0, 200, size=n).astype(np.uint32)
    hit = np.minimum(rng.integers(0, 200, size=n), smp).astype(np.uint32)
    smp[:50] = 0                       # sampled == 0: 0 >= F * 0
    hit[:50] = 0
    smp[50:60], hit[50:60] = 0xFFFFFFFF, 0xFFFFFFFF
    smp[60:70], hit[60:70] = 0xFFFFFFFF, 0xFFFFFFFE
    smp[70:80], hit[70:80] = 10, np.arange(10)   # F * sampled on either side of an integer
    d_smp, d_hit = (torch.from_numpy(a.view(np.int32)).to(cuda) for a in (smp, hit))
    some = False
    for h, f in ((1, 0.0), (0, 0.0), (0, 0.3), (3, 0.5), (1, 0.1), (1, 1.0), (0, 1.0), (2, 1 / 3), (1, 0.7), (0xFFFFFFFF, 0.0),
                 (1, 0.30000000000000004), (1, 0.29999999999999993)):
        exp = np.array([int(a) >= h and float(a) >= f * float(s) for s, a in zip(smp, hit)])
        some = some or any((f * float(s)) % 1 for s in smp)
        keep, kept = kmc.match_select(d_smp, d_hit, h, f)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(keep.cpu().numpy(), exp.astype(np.int32), err_msg=str((h, f)))
        assert int(kept.item()) == int(exp.sum()), (h, f)
        if f == 0.0:  # sampled may be NULL
            keep2, kept2 = kmc.match_select(None, d_hit, h, f, count=False)
            torch.cuda.synchronize()
            assert kept2 is None
            np.testing.assert_array_equal(keep2.cpu().numpy(), exp.astype(np.int32))
    assert some  # products that are no integers were among them
    keep, kept = kmc.match_select(d_smp[:0], d_hit[:0], 1, 0.5)
    torch.cuda.synchronize()
    assert keep.numel() == 0 and int(kept.item()) == 0


def test_match_select_then_compaction_then_match(kmc, cuda):
    """The three calls on one stream: the hits of a match select records of the parsed
    (data, indices); the result with its dst_offsets is a record buffer again, and its
    match gives the selected rows of the match on the whole batch.  The hits themselves
    are a valid keep."""
    import torch
    rng = random.Random(11)
    ref = bytes(rng.choices(b"ACGT", k=3000))
    reads = []
    for i in range(120):
        n = rng.randint(25, 150)
        at = rng.randrange(len(ref) - n)
        reads.append(ref[at:at + n] if i % 3 else bytes(rng.choices(b"ACGT", k=n)))
    raw = b"".join(Q.record(r, b"I" * len(r), b"read%d" % i) for i, r in enumerate(reads))
    assert len(raw) > S.B
    k = 21
    ref_t = torch.from_numpy(np.frombuffer(ref + b"\0", np.uint8).copy()).to(cuda)
    ref_i = torch.tensor([0, len(ref) + 1], dtype=torch.int64, device=cuda)
    dev = to_device(cuda, raw)
    data, idx, _, ridx = kmc.parse_fastq_device(dev, True, raw_indices=True)
    with kmc.SketchAccum(1, k, log2_slots=16) as acc:
        acc.add(ref_t, ref_i)
        win, smp, hit, _ = acc.match(data, idx)
        keep, kept = kmc.match_select(smp, hit, 5, 0.5)
        for flags in (keep, hit):
            dst, doff, counts = kmc.select_records(data, idx, flags)
            torch.cuda.synchronize()
            nk, nb = (int(x) for x in counts.cpu().numpy())
            rows = np.flatnonzero(flags.cpu().numpy())
            assert 0 < nk == rows.size < len(reads)
            sub = acc.match(dst[:nb], doff[:nk + 1])
            torch.cuda.synchronize()
            for whole, part in zip((win, smp, hit), sub[:3]):
                np.testing.assert_array_equal(part.cpu().numpy(), whole.cpu().numpy()[rows])
            assert dst[:nb].cpu().numpy().tobytes() == b"".join(reads[r] + b"\0" for r in rows)
        assert int(kept.item()) == int(keep.sum().item())
        # and the reads themselves, cut from the raw text with the same flags
        text, _, counts = kmc.select_records(dev, ridx, keep, offsets_out=False)
        rest, _, rcounts = kmc.select_records(dev, ridx, keep, invert=True, offsets_out=False)
        torch.cuda.synchronize()
        flags = keep.cpu().numpy()
        rec = [Q.record(r, b"I" * len(r), b"read%d" % i) for i, r in enumerate(reads)]
        assert text[:int(counts[1])].cpu().numpy().tobytes() == b"".join(x for x, f in zip(rec, flags) if f)
        assert rest[:int(rcounts[1])].cpu().numpy().tobytes() == b"".join(x for x, f in zip(rec, flags) if not f)
