"""kmc_select_records restated in plain Python, and the helper the GPU tests call it
through.  No tests here.

Sizes follow kmc_text.h (when one changes, these change with it):
    kFpPer    64      source bytes per thread (T)
    kFpTile   16384   source bytes per block (B)
and the kernel stores whole dwords (4 bytes) between a partial head and tail."""
import numpy as np

T = 64
B = 16384
GUARD = 0xA5


def model(src, offsets, keep, invert=False):
    """(kept bytes, their offsets int64 [kept + 1], (records, bytes)) of the records
    src[offsets[r]:offsets[r+1]] with (keep[r] != 0) != invert; offsets clamped."""
    src = bytes(src)
    off = np.clip(np.asarray(offsets, dtype=np.int64), 0, len(src))
    sel = [r for r in range(len(off) - 1) if (int(keep[r]) != 0) != bool(invert)]
    recs = [src[off[r]:max(off[r + 1], off[r])] for r in sel]
    out = b"".join(recs)
    doff = np.cumsum([0] + [len(x) for x in recs]).astype(np.int64)
    return out, doff, (len(sel), len(out))


def offsets_of(lens, first=0):
    return (first + np.cumsum([0] + list(lens))).astype(np.int64)


def random_bytes(rng, n):
    """n bytes, none of them the guard byte."""
    a = rng.integers(0, 255, size=n, dtype=np.uint8)
    a[a == GUARD] = 0
    return a


def select(kmc, src, offsets, keep, invert=False, capacity=None, src_shift=0, dst_shift=0, workspace=None,
           stream=None, offsets_out=True, guard=64):
    """One call on the device.  src is placed src_shift bytes behind an aligned
    address, dst dst_shift bytes behind one, with `guard` bytes of GUARD on either
    side of dst[0, capacity).  Returns (dst bytes [min(capacity, kept bytes)],
    dst_offsets [kept + 1] or None, (records, bytes)); asserts the guards."""
    import torch
    src = np.frombuffer(bytes(src), dtype=np.uint8)
    n = src.size
    cap = n if capacity is None else capacity
    dev = torch.device("cuda:0")
    with kmc._on(stream):
        s_buf = torch.zeros(n + 32, dtype=torch.uint8, device=dev)
        s_t = s_buf[src_shift:src_shift + n]
        s_t.copy_(torch.from_numpy(src.copy()))
        off_t = torch.from_numpy(np.asarray(offsets, dtype=np.int64).copy()).to(dev)
        keep_t = torch.from_numpy(np.asarray(keep, dtype=np.uint32).view(np.int32).copy()).to(dev)
        d_buf = torch.full((cap + 2 * guard + 8,), GUARD, dtype=torch.uint8, device=dev)
        d_t = d_buf[guard + dst_shift:guard + dst_shift + cap]
        counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    dst, doff, counts = kmc.select_records(s_t, off_t, keep_t, invert=invert, capacity=cap, offsets_out=offsets_out,
                                           src_bytes=n, workspace=workspace, out=(d_t, counts), stream=stream)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    c = tuple(int(x) for x in counts.cpu().numpy())
    whole = d_buf.cpu().numpy()
    lo = guard + dst_shift
    assert (whole[:lo] == GUARD).all() and (whole[lo + cap:] == GUARD).all(), "bytes outside dst[0, dst_cap) were written"
    got = whole[lo:lo + min(cap, c[1])].tobytes()
    if c[1] <= cap:
        assert (whole[lo + c[1]:lo + cap] == GUARD).all(), "bytes behind the kept ones were written"
    return got, (doff.cpu().numpy()[:c[0] + 1] if doff is not None else None), c


def check(kmc, src, offsets, keep, invert=False, **kw):
    """select() equals model(), byte for byte."""
    exp, eoff, ecounts = model(src, offsets, keep, invert)
    got, goff, counts = select(kmc, src, offsets, keep, invert, **kw)
    assert counts == ecounts, (counts, ecounts)
    assert got == exp, "kept bytes differ (first at %d of %d)" % (
        next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp))), len(exp))
    if goff is not None:
        np.testing.assert_array_equal(goff, eoff)
    return exp


def raw_offsets(raw, final=True):
    """raw_indices of kmc_fastq_parse_device_ex for well-formed input: where the '@' of
    every complete record is, then the offset just past the last record's fourth line
    (its '\\n' included when there is one)."""
    starts = [0]
    for i, b in enumerate(raw):
        if b == 0x0A:
            starts.append(i + 1)
    ended = len(starts) - 1                     # lines ended by '\n'
    lines = ended + (1 if final and len(raw) > starts[-1] else 0)
    nrec = (lines if final else ended) // 4
    starts.append(len(raw))                     # where an unended last line stops
    return np.array([starts[4 * r] for r in range(nrec)] + [min(starts[4 * nrec], len(raw))], dtype=np.int64)
