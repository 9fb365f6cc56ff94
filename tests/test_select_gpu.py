"""kmc_select_records on the GPU against select_util.model, byte for byte.  The
geometry that can go wrong is the 16 KiB source tile (B), the 64-byte thread span (T)
and the 4-byte store, so every buffer is a few tiles at the most."""
import numpy as np
import pytest

import select_util as S
from select_util import B, T

pytestmark = pytest.mark.gpu


def generic(seed=5, nrec=300, hi=400):
    """(src, offsets, rng): about 3.5 tiles of records of 0..hi bytes, a tenth of them empty."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, hi, size=nrec)
    lens[rng.random(nrec) < 0.1] = 0
    lens[:3] = (0, 0, 5)   # empty records first
    lens[-2:] = (7, 0)     # and last
    off = S.offsets_of(lens)
    return S.random_bytes(rng, int(off[-1])).tobytes(), off, rng


SELECTIONS = ["none", "all", "alternating", "first", "last", "random"]


def selection(name, n, rng):
    keep = np.zeros(n, dtype=np.uint32)
    if name == "all":
        keep[:] = 1
    elif name == "alternating":
        keep[::2] = 1
    elif name == "first":
        keep[0] = 1
    elif name == "last":
        keep[-1] = 1
    elif name == "random":
        keep[:] = rng.random(n) < 0.5
    return keep


@pytest.mark.parametrize("name", SELECTIONS)
def test_selections_and_their_inverse(kmc, cuda, name):
    src, off, rng = generic()
    assert len(src) > 3 * B
    keep = selection(name, len(off) - 1, rng)
    a = S.check(kmc, src, off, keep, invert=False)
    b = S.check(kmc, src, off, keep, invert=True)
    assert len(a) + len(b) == len(src)
    if name == "first":  # records 0 and 1 are empty, and so is the last
        keep[:] = 0
        keep[2] = 1
        assert S.check(kmc, src, off, keep) == src[:5]
        keep[:] = 0
        keep[-2] = 1
        assert S.check(kmc, src, off, keep) == src[-7:]


def test_any_non_zero_value_selects(kmc, cuda):
    src, off, rng = generic(seed=6)
    n = len(off) - 1
    keep = rng.choice(np.array([0, 0, 1, 2, 0x80000000, 0xFFFFFFFF, 0x100, 0x10000], dtype=np.uint32), size=n)
    assert (keep == 0x80000000).any() and (keep == 0).any()
    S.check(kmc, src, off, keep)
    S.check(kmc, src, off, keep, invert=True)
    S.check(kmc, src, off, keep, invert=7)  # any non-zero invert


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_records_that_end_at_a_tile_boundary(kmc, cuda, d):
    """Record 1 ends at B + d, record 3 at 2 B + d and starts a thread span before it; kept
    and dropped in turn, so that a tile's output range begins or ends at the boundary."""
    lens = [100, B + d - 100, B - T, T, 3, 0, 500]
    off = S.offsets_of(lens)
    assert off[2] == B + d and off[4] == 2 * B + d
    rng = np.random.default_rng(10 + d)
    src = S.random_bytes(rng, int(off[-1])).tobytes()
    for keep in ([1, 1, 0, 0, 1, 1, 1], [0, 1, 0, 1, 0, 0, 0], [1, 0, 1, 0, 1, 0, 1], [0, 0, 0, 1, 0, 0, 0], [1] * 7):
        S.check(kmc, src, off, keep)
        S.check(kmc, src, off, keep, invert=True)


def test_a_record_of_three_tiles_between_short_ones(kmc, cuda):
    lens = [9, 150, 40 * 1024, 33, 150]
    off = S.offsets_of(lens, first=B - 200)  # the long record starts shortly before a tile boundary
    rng = np.random.default_rng(21)
    src = S.random_bytes(rng, int(off[-1]) + 10).tobytes()
    for keep in ([1, 1, 1, 1, 1], [0, 0, 1, 0, 0], [1, 1, 0, 1, 1], [0, 1, 0, 1, 0]):
        S.check(kmc, src, off, keep)


def test_many_records_in_a_thread_span(kmc, cuda):
    """5000 six-byte records, the smallest FASTQ record: ten and more per 64 bytes."""
    n = 5000
    rng = np.random.default_rng(22)
    src = b"@\n\n+\n\n" * n
    marked = bytearray(src)
    for r in range(n):  # (tell the records apart: the header's '@' becomes a letter)
        marked[6 * r] = 65 + r % 26
    off = S.offsets_of([6] * n)
    for keep in (rng.random(n) < 0.5, np.arange(n) % 3 == 0, np.ones(n)):
        S.check(kmc, bytes(marked), off, keep.astype(np.uint32))
        S.check(kmc, bytes(marked), off, keep.astype(np.uint32), invert=True)


def test_runs_of_empty_records(kmc, cuda):
    """Thousands of empty records at one position, inside a span and at a tile boundary."""
    lens = [10] + [0] * 3000 + [B - 10] + [0] * 3000 + [1, 0, 0, 2, 70, 0]
    off = S.offsets_of(lens)
    rng = np.random.default_rng(23)
    src = S.random_bytes(rng, int(off[-1])).tobytes()
    n = len(lens)
    for keep in (np.ones(n), rng.random(n) < 0.5, np.array(lens) == 0, np.array(lens) != 0):
        S.check(kmc, src, off, keep.astype(np.uint32))


@pytest.mark.parametrize("src_shift", [0, 1, 2, 3])
def test_output_offsets_mod_4_and_misaligned_buffers(kmc, cuda, src_shift):
    """The kept range of the second tile starts at output offset `first` mod 4 (the first
    record has 1..4 bytes and the long one behind it crosses the tile boundary), src lies
    src_shift bytes behind an aligned address and dst 0..3 bytes behind one."""
    rng = np.random.default_rng(30 + src_shift)
    for first in (1, 2, 3, 4):
        lens = [first, 2, B + 300, 1, 2, 3, 90]
        off = S.offsets_of(lens)
        src = S.random_bytes(rng, int(off[-1])).tobytes()
        for keep in ([1, 0, 1, 0, 1, 0, 1], [1, 1, 1, 1, 1, 1, 1], [0, 0, 1, 1, 0, 1, 0]):
            S.check(kmc, src, off, keep, src_shift=src_shift, dst_shift=(first + src_shift) % 4)
    S.check(kmc, src, off, [1] * 7, src_shift=src_shift + 12)  # 13..15 bytes behind a 16-byte boundary


def test_bytes_outside_the_records_and_clamped_offsets(kmc, cuda):
    rng = np.random.default_rng(40)
    src = S.random_bytes(rng, 2 * B + 777).tobytes()
    n = len(src)
    # leading and trailing bytes belong to no record
    off = S.offsets_of([50, 0, B, 20], first=300)
    assert off[-1] < n - B // 2
    for keep in ([1, 1, 1, 1], [0, 0, 1, 0], [1, 0, 0, 1]):
        S.check(kmc, src, off, keep)
    # offsets beyond src_bytes, and below 0, are clamped
    off = np.array([-5, 10, B + 1, n - 3, n + 100, n + 200, 1 << 50], dtype=np.int64)
    for keep in ([1] * 6, [0, 1, 0, 1, 0, 1], [0, 0, 0, 1, 1, 1]):
        exp = S.check(kmc, src, off, keep)
    assert exp == src[n - 3:]
    # no record: counts are zeros, dst_offsets[0] = 0, nothing is written
    got, doff, counts = S.select(kmc, src, np.array([5], dtype=np.int64), np.zeros(0, dtype=np.uint32))
    assert got == b"" and counts == (0, 0) and doff.tolist() == [0]
    # records, but no byte
    got, doff, counts = S.select(kmc, b"", np.zeros(4, dtype=np.int64), [1, 0, 1])
    assert got == b"" and counts == (2, 0) and doff.tolist() == [0, 0, 0]


def test_offsets_that_do_not_ascend_touch_nothing_else(kmc, cuda):
    """An unspecified result, but the guards around dst stay (select asserts them) and
    the counts are those of the clamped lengths."""
    rng = np.random.default_rng(41)
    src = S.random_bytes(rng, 2 * B).tobytes()
    off = np.array([B, 100, 2 * B, 0, B + 5, 7, 2 * B, 2 * B], dtype=np.int64)
    for cap in (None, 1000):
        _, _, counts = S.select(kmc, src, off, [1] * 7, capacity=cap, offsets_out=False)
        assert counts == (7, (2 * B - 100) + (B + 5) + (2 * B - 7))


def test_capacity_below_the_kept_bytes_then_a_second_call(kmc, cuda):
    src, off, rng = generic(seed=7)
    keep = selection("random", len(off) - 1, rng)
    exp, eoff, ecounts = S.model(src, off, keep)
    assert ecounts[1] > B + 1000
    for cap in (B + 1, 5, 1, ecounts[1] - 1):
        got, doff, counts = S.select(kmc, src, off, keep, capacity=cap)  # the guards behind dst + cap are asserted
        assert counts == ecounts
        np.testing.assert_array_equal(doff, eoff)
    got, _, counts = S.select(kmc, src, off, keep, capacity=counts[1])  # again, with exactly the room
    assert got == exp and counts == ecounts
    # count only: dst is NULL
    got, doff, counts = S.select(kmc, src, off, keep, capacity=0)
    assert got == b"" and counts == ecounts
    np.testing.assert_array_equal(doff, eoff)
    _, doff, counts = S.select(kmc, src, off, keep, capacity=0, offsets_out=False, invert=True)
    assert doff is None and counts == (len(keep) - ecounts[0], len(src) - ecounts[1])


def test_caller_workspace_of_exactly_the_size(kmc, cuda):
    import torch
    src, off, rng = generic(seed=8)
    n = len(off) - 1
    keep = selection("random", n, rng)
    need = kmc.select_records_workspace_size(n, len(src))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
    a = S.check(kmc, src, off, keep, workspace=ws)
    ws.fill_(0xFF)
    b = S.check(kmc, src, off, keep, invert=True, workspace=ws)
    assert a == S.check(kmc, src, off, keep) and b == S.check(kmc, src, off, keep, invert=True)  # NULL workspace
    small = torch.empty(need - 1, dtype=torch.uint8, device=cuda)
    with pytest.raises(kmc.KmcError) as e:
        S.select(kmc, src, off, keep, workspace=small)
    assert e.value.code == 1004
    with pytest.raises(kmc.KmcError) as e:
        S.select(kmc, src, off, keep, workspace=torch.empty(need + 8, dtype=torch.uint8, device=cuda)[4:])
    assert e.value.code == 1003


def test_overlap_is_refused(kmc, cuda):
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    off = torch.tensor([0, 10, 1000], dtype=torch.int64, device=cuda)
    keep = torch.ones(2, dtype=torch.int32, device=cuda)
    counts = torch.zeros(2, dtype=torch.int64, device=cuda)
    for lo, hi in ((0, 1000), (999, 1100), (500, 600)):
        with pytest.raises(kmc.KmcError) as e:
            kmc.select_records(buf[:1000], off, keep, out=(buf[lo:hi], counts))
        assert e.value.code == 1001
    dst, doff, counts = kmc.select_records(buf[:1000], off, keep, out=(buf[1000:2000], counts))  # adjacent: accepted
    assert counts.tolist() == [2, 1000]


def test_on_a_side_stream_behind_late_input(kmc, cuda):
    """The call on a non-blocking side stream behind a device-side delay, its inputs
    written on that stream after the delay (stream_util): the result is the late
    input's, so every launch and memset of the call is on the caller's stream."""
    import torch
    import stream_util as U
    cycles, _ = U.sleep_cycles(U.DELAY_MS)
    s, _ = U.side_streams(kmc, cuda, cycles)
    src, off, rng = generic(seed=9)
    n = len(off) - 1
    real = {"src": np.frombuffer(src, np.uint8), "off": off, "keep": selection("random", n, rng)}
    decoy = {"src": real["src"][::-1].copy(), "off": S.offsets_of(np.diff(off)[::-1]), "keep": 1 - real["keep"]}
    dev = {w: {k: torch.from_numpy((v.view(np.int32) if k == "keep" else v).copy()).to(cuda)
               for k, v in d.items()} for w, d in (("real", real), ("decoy", decoy))}
    live = {k: torch.empty_like(v) for k, v in dev["real"].items()}
    dst = torch.empty(len(src), dtype=torch.uint8, device=cuda)
    doff = torch.empty(n + 1, dtype=torch.int64, device=cuda)
    counts = torch.empty(2, dtype=torch.int64, device=cuda)
    ws = torch.empty(kmc.select_records_workspace_size(n, len(src)), dtype=torch.uint8, device=cuda)

    def run(which, stream):
        kmc.select_records(live["src"], live["off"], live["keep"], offsets_out=doff, workspace=ws, out=(dst, counts),
                           stream=stream)

    def expect(d):
        out, eoff, ecounts = S.model(d["src"].tobytes(), d["off"], d["keep"])
        return out, eoff, ecounts

    def check(got, exp, msg):
        g_dst, g_off, g_counts = got[:3]
        assert tuple(int(x) for x in g_counts) == exp[2], msg
        assert g_dst[:exp[2][1]].tobytes() == exp[0], msg
        np.testing.assert_array_equal(g_off[:exp[2][0] + 1], exp[1], err_msg=msg)

    call = U.Call("select_records", [(live[k], dev["decoy"][k], dev["real"][k]) for k in ("src", "off", "keep")],
                  [dst, doff, counts], run, {"real": expect(real), "decoy": expect(decoy)}, check,
                  lambda e: (np.frombuffer(e[0], np.uint8), e[1], np.array(e[2])), ws=ws)
    U.late_call(call, s, cycles)
