"""The FASTQ record rules of include/kmc.h restated in plain Python, and a random FASTQ
writer.  No device: test_fastq_util.py checks the restatement on hand-written cases
and pins it to the host FASTA loader; test_fastq_gpu.py then pins the GPU parser
(csrc/kmc_fastq_gpu.hip) to it bit for bit.

Sizes follow the constants of kmc_text.h / kmc_fastq_gpu.hip / kmc_scan.h (when one
changes, these change with it):
    kFpPer    64      raw bytes per thread (T)
    kFpTile   16384   raw bytes per block (B)
    kFqVBlock 256     records per block of the validation
    kScanTile 4096    elements per block of excl_scan_u32

`rng` is a random.Random everywhere."""
import numpy as np

T = 64
B = 16384
V_BLOCK = 256
SCAN_TILE = 4096


class FormatError(Exception):
    """record_index: the smallest 0-based index of a record that breaks a rule, or
    the number of complete records when only the leftover lines of a final input do."""

    def __init__(self, record_index):
        super().__init__("malformed FASTQ at record %d" % record_index)
        self.record_index = record_index


def _strip_cr(line):
    return line[:-1] if line.endswith(b"\r") else line


def parse(raw, final=True):
    """(data bytes, indices list [n + 1], consumed) of the complete records of raw."""
    pieces = raw.split(b"\n")
    tail = pieces.pop()            # the bytes after the last '\n'
    ended = len(pieces)            # lines ended by '\n'
    lines = [_strip_cr(ln) for ln in pieces]
    if final and tail:             # bytes after the last '\n' are a line when there are any
        lines.append(_strip_cr(tail))
    nrec = (len(lines) if final else ended) // 4
    out = bytearray()
    idx = [0]
    for r in range(nrec):
        head, seq, plus, qual = lines[4 * r:4 * r + 4]
        if not head.startswith(b"@") or not plus.startswith(b"+") or len(qual) != len(seq):
            raise FormatError(r)
        out += seq + b"\0"
        idx.append(len(out))
    if final:
        if any(lines[4 * nrec:]):
            raise FormatError(nrec)
        consumed = len(raw)
    else:
        consumed = sum(len(ln) + 1 for ln in pieces[:4 * nrec])
    return bytes(out), idx, consumed


def parse_np(raw, final=True):
    data, idx, consumed = parse(raw, final)
    return np.frombuffer(data, dtype=np.uint8), np.array(idx, dtype=np.int64), consumed


# ---------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------
_BASES = b"ACGT"
_QUALS = bytes(range(33, 75))  # Phred+33, '!' .. 'J': holds '@' (31) and '+' (10)


def random_read(rng, lo, hi, lower=0.0, n_rate=0.0):
    """(sequence, quality) of a length in lo..hi."""
    n = rng.randint(lo, hi)
    seq = bytearray(rng.choices(_BASES, k=n))
    for i in range(n):
        x = rng.random()
        if x < n_rate:
            seq[i] = ord("N")
        elif x < n_rate + lower:
            seq[i] |= 0x20
    return bytes(seq), bytes(rng.choices(_QUALS, k=n))


def record(seq, qual, name=b"r", eol=b"\n", plus=b"+"):
    return b"@" + name + eol + seq + eol + plus + eol + qual + eol


def write_fastq(rng, nreads, lo=0, hi=200, crlf=False, final_newline=True, blank_lines=0, trap=True, lower=0.02,
                n_rate=0.02):
    """(raw bytes, [sequences]).  trap: every third non-empty quality starts with '@'
    and every third with '+', the two Phred characters a line-guessing parser trips
    on.  Some '+' lines repeat the name, as old files do."""
    eol = b"\r\n" if crlf else b"\n"
    out = bytearray()
    seqs = []
    for i in range(nreads):
        # (an empty last read without its final newline would lose its quality line altogether)
        last_unended = i == nreads - 1 and not final_newline
        seq, qual = random_read(rng, max(lo, 1) if last_unended else lo, max(hi, 1), lower, n_rate)
        if trap and qual and i % 3:
            qual = (b"@" if i % 3 == 1 else b"+") + qual[1:]
        name = b"read%d len=%d" % (i, len(seq))
        out += record(seq, qual, name, eol, b"+" + name if i % 5 == 0 else b"+")
        seqs.append(seq)
    if not final_newline and out:
        del out[-len(eol):]
    out += eol * blank_lines
    return bytes(out), seqs


def as_fasta(seqs):
    """The reads as one-line-per-read FASTA (for reads that are non-empty and hold no '|')."""
    return b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs))


def expected_of(seqs):
    data = b"".join(s + b"\0" for s in seqs)
    idx = np.cumsum([0] + [len(s) + 1 for s in seqs]).astype(np.int64)
    return np.frombuffer(data, dtype=np.uint8), idx


# the issue's edge texts: (text, final=1 result, final=0 result); a result is
# ([sequences], consumed) or the FormatError index
EDGE_TEXTS = [
    (b"", ([], 0), ([], 0)),
    (b"\n", ([], 1), ([], 0)),
    (b"@h\nAC\n+\nII", ([b"AC"], 10), ([], 0)),
    (b"@h\nAC\n+\nII\n", ([b"AC"], 11), ([b"AC"], 11)),
    (b"@h\n\n+\n\n", ([b""], 7), ([b""], 7)),
    (b"@h\r\nAC\r\n+\r\nII\r\n", ([b"AC"], 15), ([b"AC"], 15)),
    (b"@h\nAC\n+\nII\n\n\n", ([b"AC"], 13), ([b"AC"], 11)),
    (b"@h\nAC\n+\nI\n", 0, 0),
    (b"h\nAC\n+\nII\n", 0, 0),
    (b"@h\nAC\n-\nII\n", 0, 0),
    (b"@h\nAC\n+\nII\n@g\nA", 1, ([b"AC"], 11)),
    (b"@h\nAC\n+\n@I\n@g\nG\n+\n+\n", ([b"AC", b"G"], 20), ([b"AC", b"G"], 20)),
]


def boundary_input(d, crlf=False):
    """One record whose header is padded so that its 3-base sequence line starts at raw
    offset B - T - 2 + d, then 4 ordinary records, padded by their headers to three
    tiles of raw bytes: (raw, [sequences])."""
    eol = b"\r\n" if crlf else b"\n"
    start = B - T - 2 + d
    name = b"x" * (start - 1 - len(eol))
    seqs = [b"GAT", b"ACGTACGTAC", b"T", b"", b"CCGGN"]
    out = bytearray(record(seqs[0], b"+@I", name, eol))
    assert out.index(b"GAT") == start
    for i, s in enumerate(seqs[1:]):
        room = (3 * B - len(out)) // (4 - i) if i < 3 else 3 * B - len(out)
        pad = room - (len(s) * 2 + 2 + 4 * len(eol))
        out += record(s, b"I" * len(s), b"p" * pad, eol)
    assert len(out) == 3 * B
    return bytes(out), seqs
