"""kmc_fastq_parse_device, _load_device, _open, _next and _close on a CPU-only host:
the symbols exist, KMC_ERR_FORMAT has its text, every argument error is returned
before any device is touched, and a reader opens and closes without one."""
import ctypes
import subprocess

NAMES = ["kmc_fastq_parse_device", "kmc_fastq_load_device", "kmc_fastq_open", "kmc_fastq_next", "kmc_fastq_close"]
OK, INVALID, ALIGNMENT, IO, CAPACITY, FORMAT = 0, 1001, 1003, 1005, 1009, 1012


def test_header_and_libraries_have_the_symbols(kmc):
    names = kmc.header_symbols()
    for n in NAMES:
        assert n in names
        assert getattr(kmc.lib(), n).argtypes is not None
    for path in (kmc.LIB_PATH, kmc.DIAG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
        assert set(NAMES) <= exported
    L = kmc.lib()
    assert [len(getattr(L, n).argtypes) for n in NAMES] == [11, 7, 3, 6, 1]
    assert kmc.KMC_ERR_FORMAT == FORMAT
    assert kmc.error_string(FORMAT) == "input is not well-formed FASTQ"
    assert L.kmc_version() == 200
    e = kmc.KmcError(FORMAT, "x", 7)
    assert e.code == FORMAT and e.record == 7 and "record 7" in str(e)
    assert kmc.KmcError(INVALID, "x").record is None


_buf = (ctypes.c_char * 1024)()
_base = (ctypes.addressof(_buf) + 255) & ~255


def _p(on, at=0):
    """Null or a 256-byte aligned host address (+ at) that is never dereferenced
    (arguments are checked first)."""
    return ctypes.c_void_p(_base + at) if on else None


def parse(L, raw=1, raw_at=0, n=100, final=1, data=1, data_at=0, cap=51, idx=1, ns=1, nb=1, used=1):
    outs = [ctypes.c_uint64(0) for _ in range(3)]
    args = [ctypes.byref(o) if on else None for o, on in zip(outs, (ns, nb, used))]
    return L.kmc_fastq_parse_device(_p(raw, raw_at), n, final, _p(data, data_at), cap, _p(idx), 1 << 20, *args, None)


def test_parse_argument_errors_need_no_device(kmc):
    def check(L):
        for name in ("raw", "data", "idx", "ns", "nb", "used"):
            assert parse(L, **{name: 0}) == INVALID, name
        assert parse(L, n=1 << 33) == INVALID and parse(L, n=(1 << 33) + 5, cap=1 << 40) == INVALID
        for at in (1, 4, 8):
            assert parse(L, raw_at=at) == ALIGNMENT, at
        for at in (1, 2, 3):
            assert parse(L, data_at=at) == ALIGNMENT, at
        # data_cap below raw_bytes / 2 + 1
        assert parse(L, n=100, cap=50) == CAPACITY and parse(L, n=101, cap=50) == CAPACITY
        assert parse(L, n=1, cap=0) == CAPACITY and parse(L, n=(1 << 33) - 1, cap=(1 << 32) - 1) == CAPACITY
        assert parse(L, raw_at=8, cap=0) == ALIGNMENT  # the alignment is judged before the capacity

    check(kmc.lib())
    with kmc.diag() as D:
        check(D)


def test_load_and_reader_argument_errors_need_no_device(kmc, tmp_path):
    L = kmc.lib()
    d, ix, h = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    nb, ns = ctypes.c_uint64(0), ctypes.c_uint64(0)
    B = ctypes.byref
    missing = str(tmp_path / "absent.fq").encode()
    assert L.kmc_fastq_load_device(None, 0, B(d), B(nb), B(ix), B(ns), None) == INVALID
    assert L.kmc_fastq_load_device(missing, 0, None, B(nb), B(ix), B(ns), None) == INVALID
    assert L.kmc_fastq_load_device(missing, 0, B(d), B(nb), B(ix), None, None) == INVALID
    assert L.kmc_fastq_load_device(missing, 0, B(d), B(nb), B(ix), B(ns), None) == IO
    assert L.kmc_fastq_open(None, 0, B(h)) == INVALID and L.kmc_fastq_open(missing, 0, None) == INVALID
    assert L.kmc_fastq_open(missing, 0, B(h)) == IO and not h.value
    assert L.kmc_fastq_open(missing, 1 << 32, B(h)) == INVALID
    assert L.kmc_fastq_next(None, B(d), B(nb), B(ix), B(ns), None) == INVALID
    L.kmc_fastq_close(None)
    # an existing file opens and closes without a device
    path = tmp_path / "reads.fq"
    path.write_bytes(b"@r\nACGT\n+\nIIII\n")
    for batch in (0, 1, 16, 4096):
        assert L.kmc_fastq_open(str(path).encode(), batch, B(h)) == OK and h.value
        assert L.kmc_fastq_next(h, None, B(nb), B(ix), B(ns), None) == INVALID
        L.kmc_fastq_close(h)
    with kmc.FastqReader(str(path), 64) as rd:
        assert rd._h.value
    assert not rd._h.value
    try:
        kmc.FastqReader(missing)
        raise AssertionError("a missing file opened")
    except kmc.KmcError as e:
        assert e.code == IO and e.record is None
