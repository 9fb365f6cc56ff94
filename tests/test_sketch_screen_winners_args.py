"""kmc_sketch_screen_winners and its size query on a CPU-only host: the symbols exist, every
refusal comes back before any device is touched (results' errors in results' order, then
the workspace's), and the size query is the header's formula, 0 on bad arguments and
monotone in both numbers."""
import ctypes
import subprocess

from test_sketch_screen_abi import ALIGNMENT, BAD_K, BIG, INVALID, MAX_VALUES, OK, WORKSPACE, _p
from test_sketch_screen_abi import formula as index_formula

NAMES = ["kmc_sketch_screen_winners_workspace_size", "kmc_sketch_screen_winners"]


def test_header_and_libraries_have_the_symbols(kmc):
    names = kmc.header_symbols()
    for n in NAMES:
        assert n in names
        assert getattr(kmc.lib(), n).argtypes is not None
        with kmc.diag() as D:
            assert getattr(D, n).argtypes is not None
    for path in (kmc.LIB_PATH, kmc.DIAG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        assert set(NAMES) <= exported
    L = kmc.lib()
    assert L.kmc_sketch_screen_winners_workspace_size.restype is ctypes.c_size_t
    assert [len(getattr(L, n).argtypes) for n in NAMES] == [2, 14]
    assert callable(kmc.sketch_screen_winners) and callable(kmc.sketch_screen_winners_workspace_size)


def winners(L, index=1, at=0, nbytes=BIG, r=1, rs=1, n=3, s=16, k=21, won=1, ws=1, ws_at=0, ws_bytes=None):
    """The pointers are host addresses that are never dereferenced; ws_bytes None: exactly the query's."""
    if ws_bytes is None:
        ws_bytes = L.kmc_sketch_screen_winners_workspace_size(nbytes, n)
    return L.kmc_sketch_screen_winners(_p(index, at), nbytes, _p(r), _p(rs), n, s, k, _p(won), None, None, None,
                                       _p(ws, 512 + ws_at), ws_bytes, None)


def test_winners_argument_errors_need_no_device(kmc):
    def check(L):
        smallest = L.kmc_sketch_screen_index_size(0, 1)
        nbytes = L.kmc_sketch_screen_index_size(3, 16)
        need = L.kmc_sketch_screen_winners_workspace_size(nbytes, 3)
        assert need > 0
        # results' refusals, in results' order
        assert winners(L, k=0) == BAD_K and winners(L, k=32) == BAD_K and winners(L, k=-1) == BAD_K
        assert winners(L, s=0) == INVALID and winners(L, s=kmc.SKETCH_MAX_SIZE + 1) == INVALID
        assert winners(L, n=MAX_VALUES // 16 + 1) == INVALID and winners(L, n=MAX_VALUES + 1, s=1) == INVALID
        for name in ("index", "r", "rs", "won"):
            assert winners(L, nbytes=nbytes, **{name: 0}) == INVALID, name
        assert winners(L, nbytes=smallest - 1, ws_bytes=BIG) == WORKSPACE and winners(L, nbytes=0, ws_bytes=BIG) == WORKSPACE
        for at in (8, 32, 128):
            assert winners(L, nbytes=nbytes, at=at) == ALIGNMENT, at  # a misaligned index
        assert winners(L, k=32, s=0) == BAD_K  # k is judged first
        assert winners(L, nbytes=smallest - 1, at=8, ws_bytes=BIG) == WORKSPACE  # the size before the alignment
        # then the workspace: its size, then its alignment
        assert winners(L, nbytes=nbytes, ws_bytes=need - 1) == WORKSPACE
        assert winners(L, nbytes=nbytes, ws_bytes=8) == WORKSPACE
        for at in (1, 4, 7):
            assert winners(L, nbytes=nbytes, ws_at=at, ws_bytes=need + 8) == ALIGNMENT, at
        assert winners(L, nbytes=nbytes, ws_at=4, ws_bytes=need - 1) == WORKSPACE
        assert winners(L, nbytes=nbytes, at=8, ws_bytes=need - 1) == ALIGNMENT  # the index before the workspace
        assert winners(L, nbytes=nbytes, won=0, ws_bytes=0) == INVALID
        # a larger index asks for more owner words: the workspace of the smaller one is short
        assert winners(L, nbytes=4 * nbytes, ws_bytes=need) == WORKSPACE
        # no row: nothing to do, whatever the pointers; the limits are still judged
        assert winners(L, n=0, index=0, r=0, rs=0, won=0, ws=0, nbytes=0, ws_bytes=0) == OK
        assert winners(L, n=0, s=0) == INVALID and winners(L, n=0, k=0) == BAD_K

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def slots_within(index_bytes):
    """The largest power of two C in 8..2^32 whose index layout fits index_bytes."""
    c = 8
    while c < 1 << 32 and 256 + (4 * 2 * c + 255) // 256 * 256 + 8 * 2 * c <= index_bytes:
        c *= 2
    return c


def formula(index_bytes, num_refs):
    """include/kmc.h: 8 (C' + 1) + 4 num_refs, each array rounded up to 256 bytes."""
    return (8 * (slots_within(index_bytes) + 1) + 255) // 256 * 256 + (4 * num_refs + 255) // 256 * 256


def test_size_query(kmc):
    f = kmc.sketch_screen_winners_workspace_size

    def check(room):
        smallest = kmc.sketch_screen_index_size(0, 1)
        assert smallest == 256 + 256 + 64
        assert f(smallest - 1, 3) == 0 and f(0, 3) == 0
        assert f(smallest, 0) == 0 and f(BIG, 0) == 0
        assert f(smallest, MAX_VALUES + 1) == 0 and f(BIG, 1 << 63) == 0
        assert f(smallest, 1) == 256 + 256 and f(smallest, 65) == 256 + 512
        for n, s in [(1, 1), (3, 16), (12, 1000), (1000, 1000), (5, 16384)]:
            nbytes = kmc.sketch_screen_index_size(n, s)
            assert nbytes == index_formula(n, s, room)
            slots = (nbytes - 256) // 12  # 4 C + 8 C, C >= 64: nothing is rounded
            if slots >= 64:
                assert slots_within(nbytes) == slots and slots_within(nbytes - 1) == slots // 2
            for extra in (0, 1, 255, nbytes):
                assert f(nbytes + extra, n) == formula(nbytes + extra, n), (n, s, extra)
        assert f(1 << 62, 1 << 30) == formula(1 << 62, 1 << 30) == 8 * (1 << 32) + 256 + 4 * (1 << 30)
        # monotone in both arguments
        for n in (1, 7, 1000):
            sizes = [f(b, n) for b in (smallest, 1000, 1 << 12, (1 << 12) + 1, 1 << 20, 10 ** 8, 1 << 40)]
            assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
        for b in (smallest, 1 << 20):
            sizes = [f(b, n) for n in (1, 2, 64, 65, 1000, 10 ** 6, MAX_VALUES)]
            assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
        assert isinstance(f(smallest, 1), int)

    check(4)
    with kmc.diag():
        check(2)
