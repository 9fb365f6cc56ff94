"""kmc_sketch_accum_* without a device: the symbols exist, every argument error is
returned before any device is touched, and the size query is the header's formula.
Where a device is present (the file runs there too) create succeeds, and the errors
that need a live handle are judged on one; without a device create must say
KMC_ERR_NOMEM, and those errors are judged in test_sketch_accum_gpu.py."""
import ctypes
import subprocess

NAMES = ["kmc_sketch_accum_device_bytes", "kmc_sketch_accum_create", "kmc_sketch_accum_add",
         "kmc_sketch_accum_finish", "kmc_sketch_accum_reset", "kmc_sketch_accum_free"]
OK, INVALID, BAD_K, NOMEM = 0, 1001, 1002, 1006
MIN_LG, MAX_LG, PER = 4, 30, 4096

_buf = (ctypes.c_char * 64)()


def _p(on):
    """Null or a host address that is never dereferenced (arguments are checked first)."""
    return ctypes.c_void_p(ctypes.addressof(_buf)) if on else None


def create(L, s=16, k=21, flags=0, lg=4, out=True):
    h = ctypes.c_void_p()
    rc = L.kmc_sketch_accum_create(s, k, flags, 42, lg, ctypes.byref(h) if out else None)
    return rc, h


def libs(kmc):
    yield kmc.lib()
    with kmc.diag() as D:
        yield D


def test_header_and_libraries_have_the_symbols(kmc):
    names = kmc.header_symbols()
    assert len([n for n in names if n.startswith("kmc_sketch_accum_")]) == 6
    assert "typedef struct kmc_sketch_accum kmc_sketch_accum;" in open(kmc.HEADER).read()  # the seventh name
    for L in libs(kmc):
        for n in NAMES:
            assert n in names and getattr(L, n).argtypes is not None
        assert L.kmc_sketch_accum_device_bytes.restype is ctypes.c_size_t
        assert [len(getattr(L, n).argtypes) for n in NAMES] == [2, 6, 6, 6, 2, 1]
        assert L.kmc_version() == 200
    for path in (kmc.LIB_PATH, kmc.DIAG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert (kmc.SKETCH_ACCUM_MIN_LOG2_SLOTS, kmc.SKETCH_ACCUM_MAX_LOG2_SLOTS) == (MIN_LG, MAX_LG)
    assert callable(kmc.SketchAccum) and callable(kmc.sketch_accum_device_bytes)


def test_create_argument_errors_need_no_device(kmc):
    for L in libs(kmc):
        for k in (0, -1, 32):
            assert create(L, k=k)[0] == BAD_K, k
        assert create(L, k=32, s=0)[0] == BAD_K  # k is judged first
        for s in (0, kmc.SKETCH_MAX_SIZE + 1):
            assert create(L, s=s)[0] == INVALID, s
        for flags in (4, 8, 0x80000000):
            assert create(L, flags=flags)[0] == INVALID, flags
        for lg in (1, 3, MAX_LG + 1, 64):
            assert create(L, lg=lg)[0] == INVALID, lg
        assert create(L, out=False)[0] == INVALID


def test_null_handle_and_null_outputs(kmc):
    for L in libs(kmc):
        assert L.kmc_sketch_accum_add(None, _p(1), _p(1), 1, 8, None) == INVALID
        assert L.kmc_sketch_accum_add(None, None, None, 0, 0, None) == INVALID  # the handle before num_seqs == 0
        assert L.kmc_sketch_accum_finish(None, 1, _p(1), _p(1), None, None) == INVALID
        assert L.kmc_sketch_accum_reset(None, None) == INVALID
        L.kmc_sketch_accum_free(None)  # nothing


def live_handle_errors(L, h):
    """The errors of add and finish that are judged on a live handle, before any launch."""
    add = L.kmc_sketch_accum_add
    assert add(h, _p(1), _p(1), (1 << 40) + 1, 8, None) == INVALID
    assert add(h, _p(1), None, 1, 8, None) == INVALID
    assert add(h, None, _p(1), 1, 8, None) == INVALID
    assert add(h, _p(1), _p(1), 1, 1 << 62, None) == INVALID
    assert add(h, _p(1), _p(1), 1, (1 << 64) - 1, None) == INVALID
    assert add(h, None, None, 0, 1 << 63, None) == OK  # no record: nothing is judged but the handle, N unchanged
    assert L.kmc_sketch_accum_finish(h, 1, None, _p(1), None, None) == INVALID
    assert L.kmc_sketch_accum_finish(h, 1, _p(1), None, None, None) == INVALID


def test_create_without_a_device_is_nomem_and_a_live_handle_judges_the_rest(kmc):
    for L in libs(kmc):
        rc, h = create(L)
        if rc == OK:  # a device is present
            try:
                live_handle_errors(L, h)
            finally:
                L.kmc_sketch_accum_free(h)
        else:
            assert rc == NOMEM and not h.value


def r256(x):
    return (x + 255) // 256 * 256


def formula(s, lg):
    """include/kmc.h: 256 + 2 (8 C + 4 C) and the select's workspace for one record (256
    bins of 8 bytes, three words), each array rounded up to 256 bytes; lg = 0: C the
    power of two at or above 4096 s."""
    if lg == 0:
        lg = MIN_LG
        while (1 << lg) < PER * s:
            lg += 1
    c = 1 << lg
    return 256 + 2 * (r256(8 * c) + r256(4 * c)) + 256 * 8 + 3 * 256


def test_device_bytes(kmc):
    f = kmc.sketch_accum_device_bytes
    for _ in libs(kmc):
        assert f(0) == 0 and f(kmc.SKETCH_MAX_SIZE + 1) == 0 and f(16, 3) == 0 and f(16, MAX_LG + 1) == 0
        assert f(16, 1) == 0 and f(0, 8) == 0
        for s in (1, 2, 16, 1000, 1024, 1025, kmc.SKETCH_MAX_SIZE):
            for lg in (0, MIN_LG, 5, 8, 20, 28, MAX_LG):
                assert f(s, lg) == formula(s, lg), (s, lg)
        assert f(16, 4) == 4096 and f(1000) == formula(1000, 22) and f(kmc.SKETCH_MAX_SIZE) == formula(1, 26)
        # monotone in both arguments
        for s in (1, 1000, kmc.SKETCH_MAX_SIZE):
            sizes = [f(s, lg) for lg in range(MIN_LG, MAX_LG + 1)]
            assert sizes == sorted(sizes) and len(set(sizes[1:])) == len(sizes) - 1  # (16 and 32 slots: one 256-byte unit)
        sizes = [f(s) for s in (1, 2, 3, 64, 1000, 1024, 1025, 4096, kmc.SKETCH_MAX_SIZE)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
        for lg in (MIN_LG, 16, MAX_LG):
            sizes = [f(s, lg) for s in (1, 64, 1000, kmc.SKETCH_MAX_SIZE)]
            assert sizes == sorted(sizes)
