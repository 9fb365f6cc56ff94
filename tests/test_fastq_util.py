"""fastq_util.parse, the plain restatement of the FASTQ record rules (include/kmc.h),
on hand-written cases, and pinned to the reference-pinned host FASTA loader: reads
that are non-empty and hold no '|' give the same record buffer whether they are
parsed as FASTQ or loaded as one-line-per-read FASTA.  No device."""
import random

import numpy as np
import pytest

import fastq_util as Q


def outcome(raw, final):
    try:
        data, idx, consumed = Q.parse(raw, final)
    except Q.FormatError as e:
        return e.record_index
    return [data[idx[k]:idx[k + 1] - 1] for k in range(len(idx) - 1)], consumed


@pytest.mark.parametrize("case", range(len(Q.EDGE_TEXTS)))
def test_edge_texts(case):
    text, final1, final0 = Q.EDGE_TEXTS[case]
    assert outcome(text, True) == final1
    assert outcome(text, False) == final0


def test_hand_written_rules():
    # verbatim bytes: no case folding, no '|' mapping, N stays; the terminator is one '\0'
    data, idx, used = Q.parse(b"@a b\nacgtN|x\n+a b\n!!!!!!!\n")
    assert (data, idx, used) == (b"acgtN|x\0", [0, 8], 26)
    # '@' and '+' as first quality characters are not headers
    assert outcome(b"@a\nAC\n+\n@+\n@b\nGT\n+\n+@\n", True) == ([b"AC", b"GT"], 22)
    # one '\r' before the '\n' is dropped, a second one is text (and counts for the length)
    assert outcome(b"@a\r\nAC\r\r\n+\r\nIII\r\n", True) == ([b"AC\r"], 17)
    assert outcome(b"@a\r\nAC\r\r\n+\r\nII\r\n", True) == 0
    # a '\r' at the very end of a final input without a last '\n'
    assert outcome(b"@a\nAC\n+\nII\r", True) == ([b"AC"], 11)
    assert outcome(b"@a\nAC\n+\nII\r", False) == ([], 0)
    # leftover lines of a final input: empty ones (also "\r") pass, text does not
    assert outcome(b"@a\nAC\n+\nII\n\r\n\n", True) == ([b"AC"], 14)
    assert outcome(b"@a\nAC\n+\nII\n@b\n", True) == 1
    assert outcome(b"@a\nAC\n+\nII\n\n\n\n\n", True) == 1      # four blank lines are a record without '@'
    assert outcome(b"@a\n\n+\n", True) == 0                     # three ended lines and nothing after: not a record
    # multi-line FASTQ breaks a rule
    assert outcome(b"@a\nAC\nGT\n+\nIIII\n", True) == 0
    # not final: what follows the last complete record is neither consumed nor judged
    assert outcome(b"@a\nAC\n+\nII\ngarbage\nmore", False) == ([b"AC"], 11)
    assert outcome(b"@a\nAC\n+\nII\n@b\nG\n+\n", False) == ([b"AC"], 11)
    # the smallest bad record is reported
    assert outcome(b"@a\nA\n+\nI\nb\nA\n+\nI\n@c\nA\n-\nI\n", True) == 1
    with pytest.raises(Q.FormatError) as e:
        Q.parse(b"x")
    assert e.value.record_index == 0


def test_writer_knobs():
    rng = random.Random(5)
    for kw in ({}, {"crlf": True}, {"final_newline": False}, {"blank_lines": 3}, {"crlf": True, "final_newline": False},
               {"lo": 0, "hi": 3}, {"crlf": True, "blank_lines": 2}):
        raw, seqs = Q.write_fastq(rng, 60, **kw)
        data, idx, used = Q.parse_np(raw)
        exp_data, exp_idx = Q.expected_of(seqs)
        np.testing.assert_array_equal(data, exp_data)
        np.testing.assert_array_equal(idx, exp_idx)
        assert used == len(raw)
    raw, seqs = Q.write_fastq(rng, 200, lo=0, hi=20)
    assert any(len(s) == 0 for s in seqs) and any(b"N" in s for s in seqs) and any(s != s.upper() for s in seqs)
    quals = raw.split(b"\n")[3::4]
    assert any(q.startswith(b"@") for q in quals) and any(q.startswith(b"+") for q in quals)
    for d in (0, 1, 64, 66, 132):
        for crlf in (False, True):
            raw, seqs = Q.boundary_input(d, crlf)
            assert len(raw) == 3 * Q.B and raw.index(b"GAT") == Q.B - Q.T - 2 + d
            np.testing.assert_array_equal(Q.parse_np(raw)[0], Q.expected_of(seqs)[0])


@pytest.mark.parametrize("crlf,final_newline", [(False, True), (True, True), (False, False)])
def test_same_records_as_the_host_fasta_loader(kmc, tmp_path, crlf, final_newline):
    rng = random.Random(77)
    raw, seqs = Q.write_fastq(rng, 250, lo=1, hi=300, crlf=crlf, final_newline=final_newline)
    assert all(seqs) and not any(b"|" in s for s in seqs)
    path = tmp_path / "reads.fa"
    path.write_bytes(Q.as_fasta(seqs))
    exp_data, exp_idx, _ = kmc.load_fasta(str(path), kmc.DIALECT_NONL, 0)
    data, idx, used = Q.parse_np(raw)
    assert used == len(raw)
    np.testing.assert_array_equal(idx, exp_idx)
    np.testing.assert_array_equal(data, exp_data)
