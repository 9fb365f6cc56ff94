"""The host loader kmc_fasta_load against fasta_util.parse_expected (a plain
restatement of the record rules) on every input that test_fasta_boundaries_gpu.py
feeds to the GPU parser, both dialects: the GPU tests' oracle is right on exactly
those inputs, and the builders place what they claim (their own assertions run
here too).  The > 128 MiB file is left to the GPU test."""
import random

import numpy as np
import pytest

import fasta_util as F


def host_equals_expected(kmc, tmp_path, raw, msg=""):
    path = str(tmp_path / "u.fa")
    with open(path, "wb") as f:
        f.write(raw)
    for dialect in (0, 1):
        exp_data, exp_idx = F.parse_expected(raw, dialect)
        data, idx, _ = kmc.load_fasta(path, dialect, 0)
        np.testing.assert_array_equal(idx, exp_idx, err_msg="%s dialect %d indices" % (msg, dialect))
        np.testing.assert_array_equal(data, exp_data, err_msg="%s dialect %d data" % (msg, dialect))


@pytest.mark.parametrize("text,d0,d1", [
    (b"", (b"", [0]), None),
    (b">h\nAC\nGT\n", (b"ACGT\0", [0, 5]), None),
    (b">h\nA|C\n\nskipped\n>g\n\nTT", (b"A\0C\0TT\0", [0, 4, 7]), None),
    (b">a\nAC\n>b\nGT\n", (b"AC>bGT\0", [0, 7]), (b"AC\0GT\0", [0, 3, 6])),
    (b">h\n\rAC\nGT\n", (b"\rACGT\0", [0, 6]), None),
    (b">h\nAC\r\n\r\nGT\n", (b"AC\r\0", [0, 4]), None),
    (b"AC\n>h\n>g\n", (b"", [0]), None),
])
def test_parse_expected_by_hand(text, d0, d1):
    """The restatement itself on records small enough to read off."""
    for dialect, want in ((0, d0), (1, d1 or d0)):
        data, idx = F.parse_expected(text, dialect)
        assert data.tobytes() == want[0] and idx.tolist() == want[1], (text, dialect)


def test_filler_lengths_and_states():
    rng = random.Random(5)
    for nbytes in list(range(F.FILLER_MIN, 40)) + [63, 64, 1000, 16383, 70001]:
        for end in ("in", "out"):
            for midline in (False, True):
                for entry in (b"", b">h\n", b">h\nAC\n", b">h\nAC"):   # entered in any state, also inside a line
                    txt = F.filler(rng, nbytes, end, midline)
                    assert len(txt) == nbytes and txt.endswith(b"\n") != midline
                    for dialect in (0, 1):
                        assert F.end_state(entry + txt, dialect) == (F.IN if end == "in" else F.OUT)
    big = F.filler(rng, 200_000, "out")
    for piece in (b"\n>", b"\r\n", b"\n\n", b"|", b"\nskipped "):
        assert piece in big
    with pytest.raises(ValueError):
        F.filler(rng, F.FILLER_MIN - 1, "in")


@pytest.mark.parametrize("name", list(F.MOTIFS))
def test_motifs(kmc, tmp_path, name):
    cases = F.motif_cases(name)
    motif = F.MOTIFS[name][0]
    assert len(cases) == len(F.MOTIF_BOUNDARIES) * 3 * len(motif) * 2
    for cid, raw in cases:
        host_equals_expected(kmc, tmp_path, raw, cid)


@pytest.mark.parametrize("n,ending", F.SIZE_CASES)
def test_sizes(kmc, tmp_path, n, ending):
    host_equals_expected(kmc, tmp_path, F.size_input(n, ending))


@pytest.mark.parametrize("t,r", F.KEEP_CASES)
def test_tile_keeping(kmc, tmp_path, t, r):
    host_equals_expected(kmc, tmp_path, F.tile_keeping(t, r))


@pytest.mark.parametrize("name", F.DROPPED_TILE_CASES)
def test_dropped_tiles(kmc, tmp_path, name):
    host_equals_expected(kmc, tmp_path, F.dropped_tile_input(name))


def test_byte_values(kmc, tmp_path):
    host_equals_expected(kmc, tmp_path, F.byte_values_input())


@pytest.mark.parametrize("name", F.CARRY_CASES)
def test_carry_inputs(kmc, tmp_path, name):
    raw = F.carry_input(name)
    assert F.line_of(raw, len(raw)) >= F.CARRY_LINE + 2 * F.LS_TILE
    host_equals_expected(kmc, tmp_path, raw, name)


def test_big_pattern(kmc, tmp_path):
    """The repeated pattern of the > 128 MiB file, over enough repeats to cross tiles."""
    path = str(tmp_path / "b.fa")
    F.write_big(path, 5 * F.FP_TILE + 77)
    with open(path, "rb") as f:
        raw = f.read()
    p = F.big_pattern()
    assert len(raw) == 5 * F.FP_TILE + 77 and raw[:len(p)] == p and raw[len(p):2 * len(p)] == p
    assert F.BIG_BYTES > 2 * F.CHUNK + F.FP_TILE and -(-F.BIG_BYTES // F.FP_TILE) > 2 * F.SCAN_TILE
    host_equals_expected(kmc, tmp_path, raw)
