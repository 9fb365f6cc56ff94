"""Inputs for the device FASTA parser (csrc/kmc_fasta_gpu.hip) aimed at its tile,
thread and scan boundaries, and a plain restatement of the record rules to check
them with.  Pure Python, no device: test_fasta_util.py pins the host loader to
parse_expected() on every input below, test_fasta_boundaries_gpu.py then pins the
GPU parser to the host loader on the same inputs.

The sizes follow the constants of kmc_fasta_gpu.hip / kmc_scan.h (when one of
them changes, these change with it):
    kFpPer   64       raw bytes per thread
    kFpBlock 256      threads per block
    kFpTile  16384    raw bytes per block (kFpBlock * kFpPer)
    kLsPer   16       lines per thread in the line scan
    kLsTile  4096     lines per line-scan block (kFpBlock * kLsPer)
    kScanTile 4096    elements per block of excl_scan_u32
    kChunk   64 MiB   staging chunk of kmc_fasta_load_device

`rng` is a random.Random everywhere (small draws are much cheaper than numpy's)."""
import functools
import random

import numpy as np

FP_PER = 64
FP_BLOCK = 256
FP_TILE = FP_PER * FP_BLOCK
LS_PER = 16
LS_TILE = FP_BLOCK * LS_PER
SCAN_TILE = 4096
CHUNK = 64 << 20
# the first line (0-based) of the second round of fp_lscan_top_kernel's carry loop
CARRY_LINE = FP_BLOCK * LS_TILE

OUT, OUT_NEW, IN = 0, 1, 2

_ALPHABET = b"ACGTNacgt|"
_POOL = bytes(random.Random(20240).choices(_ALPHABET, weights=[21, 21, 21, 21, 6, 2, 2, 2, 2, 2], k=1 << 16))
_NAMES = bytes(random.Random(20241).choices(b"abcdefghijklmnopqrstuvwxyz0123456789 _.>|", k=1 << 12))


# ---------------------------------------------------------------------------
# the record rules, restated
# ---------------------------------------------------------------------------
def _machine(raw, dialect, want_src=False):
    """The three-state line machine of kmc_fasta_gpu.hip's header comment over
    raw.split('\\n').  Returns (data, indices, state before end of input, src);
    src[i] is the raw offset that produced output byte i (an appended byte's own
    offset, a closing '\\0' at its line's '\\n'; len(raw) where there is none)."""
    out = bytearray()
    idx = []
    src = [] if want_src else None
    state = OUT
    lines = raw.split(b"\n")
    if lines[-1] == b"":  # a last piece without '\n' is a line only when non-empty
        lines.pop()
    pos = 0
    for ln in lines:
        c = ln[:1]
        if state == IN:
            if c == b"" or c == b"\r" or (c == b">" and dialect == 1):
                out.append(0)
                if want_src:
                    src.append(pos + len(ln))
                state = OUT_NEW if c == b">" else OUT
            else:
                out += ln.replace(b"|", b"\0")
                if want_src:
                    src.extend(range(pos, pos + len(ln)))
        elif c == b">":
            state = OUT_NEW
        elif state == OUT_NEW and c != b"":
            idx.append(len(out))
            out += ln.replace(b"|", b"\0")
            if want_src:
                src.extend(range(pos, pos + len(ln)))
            state = IN
        pos += len(ln) + 1
    end_state = state
    if state == IN:
        out.append(0)
        if want_src:
            src.append(len(raw))
    idx.append(len(out))
    return (np.frombuffer(bytes(out), dtype=np.uint8), np.asarray(idx, dtype=np.int64), end_state,
            np.asarray(src, dtype=np.int64) if want_src else None)


def parse_expected(raw, dialect):
    """(data uint8, indices int64 [records + 1]) of raw FASTA bytes: dialect 0 is
    importSeqs, 1 is importSeqsNoNL (a '>' line also closes a record)."""
    data, idx, _, _ = _machine(raw, dialect)
    return data, idx


def end_state(raw, dialect):
    """State after the last line of raw (a partial last line included)."""
    return _machine(raw, dialect)[2]


def kept_sources(raw, dialect):
    """Raw offset behind every output byte (see _machine)."""
    return _machine(raw, dialect, want_src=True)[3]


def line_of(raw, pos):
    """0-based number of the line that holds raw[pos]."""
    return raw.count(b"\n", 0, pos)


# ---------------------------------------------------------------------------
# filler and placement
# ---------------------------------------------------------------------------
def _seq(rng, n):
    o = rng.randrange(len(_POOL) - n) if n < len(_POOL) else 0
    s = _POOL[o:o + n]
    return s if len(s) == n else (_POOL * (n // len(_POOL) + 1))[:n]


def _name(rng, n):
    o = rng.randrange(len(_NAMES) - n)
    return _NAMES[o:o + n]


_RESERVE = 8   # the exact-length last segment of a filler takes at least this much
FILLER_MIN = _RESERVE


def filler(rng, nbytes, end_state_, midline=False):
    """FASTA text of exactly nbytes bytes: headers, sequence lines over ACGTNacgt|,
    blank lines, CRLF lines, skipped lines.  Whatever state it is entered in, and
    in both dialects, it leaves the machine in end_state_: "in" (inside a record) or
    "out" (between records, no header pending).  midline: the text ends inside a
    line (of the record, or a skipped one) instead of after a '\\n'."""
    assert end_state_ in ("in", "out")
    if nbytes < FILLER_MIN:
        raise ValueError("filler needs at least %d bytes" % FILLER_MIN)
    parts = []
    have = 0
    room = nbytes - _RESERVE
    while True:
        rec = []
        x = rng.random()
        if x < 0.1:
            rec.append(b"\n")
        elif x < 0.15:
            rec.append(b"skipped " + _seq(rng, rng.randrange(1, 30)) + b"\n")
        rec.append(b">" + _name(rng, rng.randrange(0, 24)) + b"\n")
        if rng.random() < 0.1:
            rec.append(b"\n")
        for _ in range(rng.randrange(0, 5)):
            rec.append(_seq(rng, rng.randrange(1, 200)))
            rec.append(b"\r\n" if rng.random() < 0.1 else b"\n")
        x = rng.random()
        if x < 0.6:
            rec.append(b"\n")
        elif x < 0.75:
            rec.append(b"\r\n")
        piece = b"".join(rec)
        if have + len(piece) > room:
            break
        parts.append(piece)
        have += len(piece)
    rem = nbytes - have  # >= _RESERVE
    if end_state_ == "in":
        if midline:   # ">name\n" + b bases
            b = rng.randrange(1, rem - 1)
            parts.append(b">" + _name(rng, rem - 2 - b) + b"\n" + _seq(rng, b))
        else:         # ">name\n" + b bases + "\n"
            b = rng.randrange(1, rem - 2)
            parts.append(b">" + _name(rng, rem - 3 - b) + b"\n" + _seq(rng, b) + b"\n")
    else:
        if midline:   # a line, a blank line (closes whatever is open), a skipped line
            b = rng.randrange(1, rem - 2)
            parts.append(_seq(rng, rem - 2 - b) + b"\n\n" + _seq(rng, b))
        else:
            parts.append(_seq(rng, rem - 2) + b"\n\n")
    txt = b"".join(parts)
    assert len(txt) == nbytes
    return txt


def place(motif, at, byte_of_motif, total, rng, open_before=True, midline=True):
    """Text of `total` bytes (None: the motif ends the file) in which byte
    byte_of_motif of motif sits at raw offset `at`, with filler before and after.
    Before the motif a record is open (or none is, nor a header pending), and the
    text stands inside a line (midline) or at a line start."""
    start = at - byte_of_motif
    before = filler(rng, start, "in" if open_before else "out", midline)
    want = IN if open_before else OUT
    for dialect in (0, 1):
        assert end_state(before, dialect) == want
    assert before.endswith(b"\n") != midline
    txt = before + motif
    if total is not None:
        room = total - len(txt)
        assert room >= 0
        txt += filler(rng, room, rng.choice(("in", "out")), rng.random() < 0.3) if room >= FILLER_MIN \
            else b"AC\nGT\nA"[:room]
        assert len(txt) == total
    assert txt[at] == motif[byte_of_motif] and txt[start:start + len(motif)] == motif
    return txt


# (a) motifs on thread and tile boundaries ----------------------------------
# name -> (motif, the motif follows a partial line, the motif ends the file)
MOTIFS = {
    "nl_header": (b"\n>h\n", True, False),
    "nl_nl": (b"\n\n", True, False),
    "crlf_eol": (b"\r\n", True, False),        # CRLF ending of a line
    "cr_line": (b"\r\n", False, False),        # a line that starts with '\r'
    "nl_crlf": (b"\n\r\n", True, False),
    "nl_cr_text": (b"\n\rAC\n", True, False),
    "bar": (b"|", True, False),
    "nl_bar_nl": (b"\n|\n", True, False),
    "gt_midline": (b">", True, False),
    "nl_gt_eof": (b"\n>", True, True),
    "base_eof": (b"A", True, True),
}
MOTIF_BOUNDARIES = (FP_PER, 2 * FP_PER, FP_TILE - FP_PER, FP_TILE, 2 * FP_TILE, 3 * FP_TILE)
MOTIF_TOTAL = 4 * FP_TILE + 4321   # 4-5 tiles, odd


def motif_cases(name):
    """[(id, raw)]: every byte of the motif at B - 1, B and B + 1 for each boundary B,
    after an open record and after none."""
    motif, midline, at_eof = MOTIFS[name]
    rng = random.Random("motif " + name)
    out = []
    for B in MOTIF_BOUNDARIES:
        for at in (B - 1, B, B + 1):
            for j in range(len(motif)):
                for open_before in (True, False):
                    raw = place(motif, at, j, None if at_eof else MOTIF_TOTAL, rng, open_before, midline)
                    out.append(("%s[%d]@%d %s" % (name, j, at, "open" if open_before else "closed"), raw))
    return out


def one_motif_input(name, at, j, open_before=True):
    motif, midline, at_eof = MOTIFS[name]
    return place(motif, at, j, None if at_eof else MOTIF_TOTAL, random.Random("one " + name), open_before, midline)


# (b) file sizes --------------------------------------------------------------
SIZES = (1, 15, 16, 17, 63, 64, 65, FP_TILE - 1, FP_TILE, FP_TILE + 1, 2 * FP_TILE, 3 * FP_TILE - 1)
ENDINGS = {"nl": b"\n", "base": b"A", "nlnl": b"\n\n"}
# (a one-byte file cannot end in two newlines)
SIZE_CASES = [(n, e) for n in SIZES for e in ENDINGS if n >= len(ENDINGS[e])]


def size_input(n, ending):
    """A file of exactly n bytes: an open record up to the ending."""
    end = ENDINGS[ending]
    body = n - len(end)
    rng = random.Random("size %d %s" % (n, ending))
    txt = (filler(rng, body, "in", midline=True) if body >= FILLER_MIN else b">\nACGTAC"[:body]) + end
    assert len(txt) == n and txt.endswith(end)
    return txt


# (e) kept bytes per tile ------------------------------------------------------
def dropped(rng, nbytes):
    """nbytes of whole lines that a machine between records drops: text not
    starting with '>' and blank lines."""
    parts = []
    have = 0
    while nbytes - have > 64:
        p = b"\n" if rng.random() < 0.2 else b"x" + _seq(rng, rng.randrange(0, 50)) + b"\n"
        parts.append(p)
        have += len(p)
    rem = nbytes - have
    if rem:
        parts.append(b"y" * (rem - 1) + b"\n")
    return b"".join(parts)


KEEP_CASES = [(t, r) for t in range(6) for r in range(4)]


def tile_keeping(t, r):
    """Text whose tile 1, raw bytes [16384, 32768), keeps exactly t output bytes
    that start at an output offset = r (mod 4); everything else in that tile is
    dropped (skipped lines, blank lines, the start of a header longer than a
    tile).  The kept bytes are the end of a record opened in tile 0 (t = 0: it is
    closed there) and the next kept byte comes from tile 3, so for t < 4 the
    neighbours write into the dword(s) tile 1 writes to."""
    rng = random.Random("keep %d %d" % (t, r))
    if t == 0:
        L0 = 4 * 9 + ((r - 1) % 4)                       # L0 bases + the closing '\0'
        rec = b">a\n" + _seq(rng, L0).replace(b"|", b"A") + b"\n\n"
        head = dropped(rng, FP_TILE - 700 - len(rec)) + rec
    else:
        L0 = 4 * (7 + t) + r                             # bases of the record in tile 0
        rec = b">a\n" + _seq(rng, L0 + t - 1) + b"\n\n"  # t - 1 bases in tile 1, the blank line's '\n' closes
        head = dropped(rng, FP_TILE + t + 1 - len(rec)) + rec
        assert len(head) == FP_TILE + t + 1
    txt = head + dropped(rng, FP_TILE + 5000 - len(head))
    txt += b">" + b"h" * (FP_TILE + 12000) + b"\n"       # from tile 1 through tile 2 into tile 3
    assert len(txt) // FP_TILE == 3
    txt += b"ACGTACG\nTT|A\n\n" + dropped(rng, 300) + b">c\nGAT"
    for dialect in (0, 1):
        src = kept_sources(txt, dialect)
        assert int(((src >= FP_TILE) & (src < 2 * FP_TILE)).sum()) == t, (t, r)
        assert int((src < FP_TILE).sum()) % 4 == r, (t, r)
        assert int(((src >= 2 * FP_TILE) & (src < 3 * FP_TILE)).sum()) == 0
    return txt


DROPPED_TILE_CASES = ("header_40000", "newlines_40000", "crlf_20000", "crlf_20000_after_header")


def dropped_tile_input(name):
    """Shapes in which whole tiles keep nothing (at most a closing byte)."""
    mid = {"header_40000": b"\n>" + b"h" * 39998 + b"\nTT|GA\nC\n",   # (met between records: dropped in both dialects)
           "newlines_40000": b"\n" * 40000,      # 64 lines per thread, one tile's lines over four line tiles
           "crlf_20000": b"\r\n" * 20000,
           "crlf_20000_after_header": b">z\n" + b"\r\n" * 20000}[name]
    txt = b">a\nACGTA\nCC\n" + mid + b">b\nTT|GA\nC\n\nskipped\n>c\nG"
    for dialect in (0, 1):
        src = kept_sources(txt, dialect)
        assert int(((src >= FP_TILE) & (src < 2 * FP_TILE)).sum()) == 0, name
    return txt


# (f) every byte value ---------------------------------------------------------
SPECIAL_BYTES = (0x8A, 0x0B, 0x09, 0x8D, 0xBE, 0xFC, 0x00, 0xFF)


@functools.lru_cache(maxsize=None)
def byte_values_input():
    """Three tiles of records whose header and sequence lines draw from every byte
    value but '\\n'; each special byte also stands at a line start that is a
    thread's first byte, as a thread's last byte, and at both tile boundaries."""
    rng = random.Random("bytes")
    every = bytes(b for b in range(256) if b != 0x0A)
    parts = []
    have = 0
    while have < 3 * FP_TILE:
        rec = [b">" + bytes(rng.choices(every, k=rng.randrange(0, 40))) + b"\n"]
        for _ in range(rng.randrange(1, 4)):
            # (a leading 'A' keeps most lines from changing class by chance; some do not get one)
            rec.append((b"A" if rng.random() < 0.8 else b"") + bytes(rng.choices(every, k=rng.randrange(1, 120))) + b"\n")
        rec.append(b"\n")
        p = b"".join(rec)
        parts.append(p)
        have += len(p)
    raw = bytearray(b"".join(parts)[:3 * FP_TILE])
    spots = [q for q in range(FP_PER * 3, 3 * FP_TILE, FP_PER * 7)]
    for i, q in enumerate(spots):
        s = SPECIAL_BYTES[i % len(SPECIAL_BYTES)]
        if (i // len(SPECIAL_BYTES)) % 2 == 0:
            raw[q - 1] = 0x0A   # the line starts at the thread's first byte
            raw[q] = s
        else:
            raw[q - 1] = s      # the thread's last byte
    for k, B in enumerate((FP_TILE, 2 * FP_TILE)):
        raw[B - 2] = 0x0A
        raw[B - 1] = SPECIAL_BYTES[k]
        raw[B] = 0x0A
        raw[B + 1] = SPECIAL_BYTES[k + 2]
    raw = bytes(raw)
    assert set(raw) == set(range(256))
    for s in SPECIAL_BYTES:
        assert any(raw[q] == s and raw[q - 1] == 0x0A for q in range(FP_PER, len(raw), FP_PER)), s
        assert any(raw[q - 1] == s for q in range(FP_PER, len(raw), FP_PER)), s
    for dialect in (0, 1):
        data, idx = parse_expected(raw, dialect)
        assert data.size > len(raw) // 4 and idx.size > 100
    return raw


# (g) the line scan's carry ----------------------------------------------------
# 3-line records with a period of 5 lines (header, three lines, blank): 5 divides
# neither kLsPer nor kLsTile, so records straddle every boundary of the line scan.
_REC_TEMPLATES = (b">r\nAC\nGTA\nC\n\n", b">s1\nA\nCG|\nTTGA\n\n", b">\nGATTA\nC\nAG\n\n", b">t t\nTG\nCA\nN\n\n",
                  b">u\nACGTAC\nG\nTT\n\n", b">vv\nC\nA\nGGT\n\n", b">w\nTA\nCCG\nA\n\n")
_REC_BLOCK = b"".join(_REC_TEMPLATES)   # 7 records, 35 lines, an odd number of bytes
CARRY_CASES = ("open_across", "header_at_-1", "header_at_0", "header_at_+1", "close_at_0")
CARRY_TOTAL_LINES = 1_100_000


def _records(nrec):
    return _REC_BLOCK * (nrec // 7) + b"".join(_REC_TEMPLATES[:nrec % 7])


@functools.lru_cache(maxsize=None)
def carry_input(name):
    """About 1.1 M lines, so that fp_lscan_top_kernel's loop goes round twice
    (line CARRY_LINE = 256 * 4096 is the first of the second round).
      open_across    one record of 10 000 short lines from before CARRY_LINE - 4096
                     to after CARRY_LINE + 4096; the file ends inside a record
      header_at_d    a header line at exactly CARRY_LINE + d (3-line records around it)
      close_at_0     a record of 5 000 lines closed by a blank line at CARRY_LINE"""
    assert len(_REC_BLOCK) % 2 == 1 and _REC_BLOCK.count(b"\n") == 35
    if name.startswith("header_at_"):
        d = int(name[len("header_at_"):])
        shift = (CARRY_LINE + d) % 5                     # headers at lines = shift (mod 5)
        txt = b"\n" * shift + _records((CARRY_TOTAL_LINES - shift) // 5)
        at = CARRY_LINE + d
        marks = [(at, b">")]
    else:
        nlong = 10_000 if name == "open_across" else 5_000
        first = CARRY_LINE - 5_001                       # the long record's header line
        assert first % 5 == 0
        long_rec = b">long\n" + b"".join((b"AC\n", b"G\n", b"T|A\n")[i % 3] for i in range(nlong)) + b"\n"
        after = first + nlong + 2
        tail = _records((CARRY_TOTAL_LINES - after) // 5)
        if name == "open_across":
            tail += b">end\nAC\nG"                        # open at end of input: the carry decides the last '\0'
            marks = [(first, b">"), (CARRY_LINE - LS_TILE, b"G"), (CARRY_LINE + LS_TILE, b"A"), (after - 1, b"\n")]
            assert first < CARRY_LINE - LS_TILE and after - 1 > CARRY_LINE + LS_TILE
        else:
            marks = [(first, b">"), (CARRY_LINE - 1, b"G"), (CARRY_LINE, b"\n"), (CARRY_LINE + 1, b">")]
        txt = _records(first // 5) + long_rec + tail
    # the builder's own check: line numbers around CARRY_LINE
    starts = np.flatnonzero(np.frombuffer(txt, dtype=np.uint8) == 0x0A) + 1
    assert starts.size + (not txt.endswith(b"\n")) > CARRY_LINE + LS_TILE
    for line, first_byte in marks:
        o = int(starts[line - 1])
        assert txt[o:o + 1] == first_byte, (name, line)
    return txt


# (h) above 128 MiB -------------------------------------------------------------
BIG_BYTES = 2 * CHUNK + FP_TILE + 4097    # a third staging chunk, 8194 raw tiles: three scan tiles
BIG_BYTES_SMALLER = CHUNK + FP_TILE + 4097


def big_pattern():
    """A few KB of records, odd in length, so that tile contents drift from one
    repeat to the next."""
    p = filler(random.Random("big"), 4099, "out")
    assert len(p) % 2 == 1
    return p


def write_big(path, nbytes):
    p = big_pattern()
    block = p * 1024
    with open(path, "wb") as f:
        left = nbytes
        while left > 0:
            f.write(block[:left])
            left -= min(left, len(block))
