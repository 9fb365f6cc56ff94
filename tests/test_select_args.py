"""kmc_select_records, kmc_match_select, kmc_fastq_parse_device_ex, kmc_fastq_open_ex and
kmc_fastq_raw on a CPU-only host: the symbols exist in the header and in both libraries,
every argument error is returned before any device is touched (the pointers handed in
are never dereferenced), the size query takes host numbers only, and the kmc binary
refuses --write-recruited / --write-rest where they cannot apply before any device or
file is touched."""
import ctypes
import os
import subprocess

from test_sketch_accum_args import libs

NAMES = ["kmc_select_records_workspace_size", "kmc_select_records", "kmc_match_select", "kmc_fastq_parse_device_ex",
         "kmc_fastq_open_ex", "kmc_fastq_raw"]
OK, INVALID, ALIGNMENT, IO, WORKSPACE, CAPACITY = 0, 1001, 1003, 1005, 1004, 1009

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")

_buf = (ctypes.c_char * 8192)()
_base = (ctypes.addressof(_buf) + 255) & ~255


def _p(on, at=0):
    """Null or a 256-byte aligned host address (+ at) that is never dereferenced."""
    return ctypes.c_void_p(_base + at) if on else None


def test_header_and_libraries_have_the_symbols(kmc):
    names = kmc.header_symbols()
    for n in NAMES:
        assert n in names
    for L in libs(kmc):
        assert [len(getattr(L, n).argtypes) for n in NAMES] == [2, 13, 8, 12, 4, 4]
    for path in (kmc.LIB_PATH, kmc.DIAG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert kmc.KMC_FASTQ_KEEP_RAW == 1 and "#define KMC_FASTQ_KEEP_RAW 1u" in open(kmc.HEADER).read()
    assert kmc.error_string(WORKSPACE) and kmc.KMC_ERR_CAPACITY == CAPACITY
    assert callable(kmc.select_records) and callable(kmc.match_select) and callable(kmc.FastqReader.raw)


def select(L, src=1, off=1, n=4, nbytes=100, keep=1, invert=0, dst=1, dst_at=4096, cap=100, doff=1, counts=1, ws=0, ws_at=0,
           ws_bytes=0):
    return L.kmc_select_records(_p(src), _p(off, 1024), n, nbytes, _p(keep, 2048), invert, _p(dst, dst_at), cap,
                                _p(doff, 3072), _p(counts, 3584), _p(ws, 6144 + ws_at), ws_bytes, None)


def test_select_argument_errors_need_no_device(kmc):
    for L in libs(kmc):
        for name in ("off", "keep", "counts"):
            assert select(L, **{name: 0}) == INVALID, name
            assert select(L, n=0, nbytes=0, cap=0, **{name: 0}) == INVALID, name  # judged before num_recs == 0
        assert select(L, src=0) == INVALID                      # null src, bytes above 0
        assert select(L, dst=0) == INVALID                      # null dst, capacity above 0
        assert select(L, n=(1 << 40) + 1) == INVALID
        assert select(L, nbytes=1 << 62, cap=0, dst=0) == INVALID
        assert select(L, nbytes=(1 << 62) + 9, cap=0, dst=0) == INVALID
        # overlap: the byte ranges share a byte (src = base + [0, 100))
        for at, cap in ((0, 100), (99, 1), (50, 10), (-20, 21), (-20, 1000)):
            assert select(L, dst_at=at, cap=cap) == INVALID, (at, cap)
        # a caller workspace: too small, then misaligned (no device is needed for either)
        need = L.kmc_select_records_workspace_size(4, 100)
        assert need > 0
        assert select(L, ws=1, ws_bytes=need - 1) == WORKSPACE
        assert select(L, ws=1, ws_at=4, ws_bytes=need - 1) == WORKSPACE   # the size is judged first
        for at in (1, 2, 4):
            assert select(L, ws=1, ws_at=at, ws_bytes=need) == ALIGNMENT, at


def test_size_query_takes_host_numbers_only(kmc):
    for L in libs(kmc):
        f = L.kmc_select_records_workspace_size
        assert f.restype is ctypes.c_size_t
        assert f((1 << 40) + 1, 0) == 0 and f(1, 1 << 62) == 0
        sizes = [f(n, 1 << 20) for n in (0, 1, 2, 255, 256, 4096, 4097, 10 ** 6, 10 ** 7, 1 << 40)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
        assert f(1000, 0) == f(1000, (1 << 62) - 1)  # the bytes do not enter
        # the header's formula: every array rounded up to 256 bytes
        r = lambda x: (x + 255) & ~255
        for n in (0, 1, 4096, 4097, 10 ** 6):
            assert f(n, 0) == r(4 * n) + r(8 * n) + 2 * r(8 * (n + 1)) + r(8 * ((n + 4095) // 4096 + 1)), n


def match_select(L, smp=1, hit=1, n=4, min_hits=1, frac=0.5, keep=1, kept=1):
    return L.kmc_match_select(_p(smp), _p(hit, 1024), n, min_hits, frac, _p(keep, 2048), _p(kept, 3072), None)


def test_match_select_argument_errors_need_no_device(kmc):
    for L in libs(kmc):
        for frac in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):
            assert match_select(L, frac=frac) == INVALID, frac
            assert match_select(L, frac=frac, n=0) == INVALID, frac
        assert match_select(L, hit=0) == INVALID and match_select(L, keep=0) == INVALID
        assert match_select(L, smp=0, frac=0.25) == INVALID
        assert match_select(L, n=(1 << 40) + 1) == INVALID


def parse_ex(L, raw=1, raw_at=0, n=100, data=1, data_at=0, cap=51, idx=1, ns=1, ridx=1):
    outs = [ctypes.c_uint64(0) for _ in range(3)]
    args = [ctypes.byref(o) for o in outs]
    if not ns:
        args[0] = None
    return L.kmc_fastq_parse_device_ex(_p(raw, raw_at), n, 1, _p(data, data_at), cap, _p(idx, 2048), 1 << 20, *args,
                                       _p(ridx, 3072), None)


def test_parse_ex_argument_errors_are_those_of_parse(kmc):
    for L in libs(kmc):
        for ridx in (0, 1):
            for name in ("raw", "data", "idx", "ns"):
                assert parse_ex(L, ridx=ridx, **{name: 0}) == INVALID, name
            assert parse_ex(L, ridx=ridx, n=1 << 33) == INVALID
            assert parse_ex(L, ridx=ridx, raw_at=8) == ALIGNMENT and parse_ex(L, ridx=ridx, data_at=2) == ALIGNMENT
            assert parse_ex(L, ridx=ridx, n=100, cap=50) == CAPACITY


def test_reader_flags_and_raw_refusals(kmc, tmp_path):
    L = kmc.lib()
    B = ctypes.byref
    h, raw, ridx, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(7)
    path = tmp_path / "reads.fq"
    path.write_bytes(b"@r\nACGT\n+\nIIII\n")
    name = str(path).encode()
    assert L.kmc_fastq_open_ex(None, 0, 1, B(h)) == INVALID and L.kmc_fastq_open_ex(name, 0, 1, None) == INVALID
    assert L.kmc_fastq_open_ex(str(tmp_path / "absent.fq").encode(), 0, 1, B(h)) == IO and not h.value
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert L.kmc_fastq_open_ex(name, 0, flags, B(h)) == INVALID and not h.value, flags
    assert L.kmc_fastq_open_ex(name, 1 << 32, 1, B(h)) == INVALID
    assert L.kmc_fastq_raw(None, B(raw), B(nb), B(ridx)) == INVALID
    # flags == 0 is kmc_fastq_open: no raw text
    for opened in (lambda: L.kmc_fastq_open_ex(name, 64, 0, B(h)), lambda: L.kmc_fastq_open(name, 64, B(h))):
        assert opened() == OK and h.value
        assert L.kmc_fastq_raw(h, B(raw), B(nb), B(ridx)) == INVALID and not raw.value and nb.value == 0
        L.kmc_fastq_close(h)
    # with the flag: null arguments, and no batch yet
    assert L.kmc_fastq_open_ex(name, 64, 1, B(h)) == OK and h.value
    assert L.kmc_fastq_raw(h, None, B(nb), B(ridx)) == INVALID
    assert L.kmc_fastq_raw(h, B(raw), None, B(ridx)) == INVALID
    assert L.kmc_fastq_raw(h, B(raw), B(nb), None) == INVALID
    assert L.kmc_fastq_raw(h, B(raw), B(nb), B(ridx)) == INVALID and not raw.value and not ridx.value
    L.kmc_fastq_close(h)
    with kmc.FastqReader(str(path), 64, keep_raw=True) as rd:
        try:
            rd.raw()
            raise AssertionError("raw() before the first batch")
        except kmc.KmcError as e:
            assert e.code == INVALID


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, timeout=120)


def write_option_checks(tmp_path):
    """--write-recruited and --write-rest, judged before any device or file is touched
    (also run by test_select_cli.py, where a device is present)."""
    out = run(["--help"]).stdout.decode()
    assert "--write-recruited" in out and "--write-rest" in out
    assert "recruited_<f>.fastq" in out and "rest_<f>.fastq" in out and "one more raw batch of device memory" in out
    fq, fa, odd = tmp_path / "absent.fq", tmp_path / "absent.fa", tmp_path / "absent.reads"
    rc = ["--canonical", "-k", 21, "--accum-slots", 20]
    bad = [
        (["--canonical", "-k", 21, "--write-recruited", fa], b"--write-recruited and --write-rest write the reads of --recruit"),
        (["--canonical", "-k", 21, "--write-rest", fa], b"--write-recruited and --write-rest write the reads of --recruit"),
        (["--write-recruited", "--write-rest", fa], b"write the reads of --recruit"),
        (rc + ["--recruit", fa, "--write-recruited", fa], b"%s is not FASTQ" % str(fa).encode()),
        (rc + ["--recruit", fq, "--recruit", odd, "--write-rest", fa], b"%s is not FASTQ" % str(odd).encode()),
        (rc + ["--recruit", fq, "--format", "fasta", "--write-recruited", "--write-rest", fa],
         b"%s is not FASTQ" % str(fq).encode()),
        (["-k", 8, "--accum-slots", 20, "--recruit", fq, "--write-recruited", fa], b"--recruit needs --canonical"),
    ]
    for args, msg in bad:
        r = run(args)
        assert r.returncode == 2, (args, r.stderr[:200])
        assert msg in r.stderr and b"usage:" in r.stderr, (args, r.stderr[:300])
        assert not list(tmp_path.glob("*.fastq")) and not os.path.exists("recruited_0.fastq")
    # accepted: what fails is the missing device or input (1), not the options
    for args in (rc + ["--recruit", fq, "--write-recruited", "--out", tmp_path, fa],
                 rc + ["--recruit", fq, "--write-rest", "--write-recruited", "--out", tmp_path, fa],
                 rc + ["--recruit", odd, "--format", "fastq", "--write-rest", "--out", tmp_path, fq]):
        assert run(args).returncode == 1, args


def test_write_option_combinations(tmp_path):
    write_option_checks(tmp_path)
