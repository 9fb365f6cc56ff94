"""kmc_match_from_accum without a device: the symbol exists in the header and in both
libraries, the refusals that need no live handle come back before any device is
touched, and the kmc binary judges the option combinations of --recruit before any
device or file is touched.  Where a device is present (the file runs there too) the
refusals that are judged on a live handle are checked on one, as test_sketch_accum_args
does; without a device they are judged in test_sketch_match_gpu.py."""
import ctypes
import os
import subprocess

from test_sketch_accum_args import create, libs

NAME = "kmc_match_from_accum"
OK, INVALID, NOMEM = 0, 1001, 1006

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")

_buf = (ctypes.c_char * 64)()


def _p(on):
    """Null or a host address that is never dereferenced (arguments are checked first)."""
    return ctypes.c_void_p(ctypes.addressof(_buf)) if on else None


def test_header_and_libraries_have_the_symbol(kmc):
    names = kmc.header_symbols()
    assert NAME in names
    for L in libs(kmc):
        assert len(getattr(L, NAME).argtypes) == 11
    for path in (kmc.LIB_PATH, kmc.DIAG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert NAME in set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert callable(kmc.SketchAccum.match)


def test_null_handle_needs_no_device(kmc):
    for L in libs(kmc):
        f = getattr(L, NAME)
        assert f(None, _p(1), _p(1), 1, 8, 1, _p(1), _p(1), _p(1), _p(1), None) == INVALID
        assert f(None, None, None, 0, 0, 1, None, None, None, None, None) == INVALID  # the handle before num_seqs == 0
        assert f(None, _p(1), _p(1), (1 << 40) + 1, 8, 0, None, None, _p(1), None, None) == INVALID


def live_handle_errors(L, h):
    """The refusals judged on a live handle, before any launch."""
    f = getattr(L, NAME)
    assert f(h, _p(1), _p(1), 1, 8, 1, _p(1), _p(1), None, _p(1), None) == INVALID       # null hits
    assert f(h, _p(1), None, 1, 8, 1, None, None, _p(1), None, None) == INVALID         # null indices
    assert f(h, None, _p(1), 1, 8, 1, None, None, _p(1), None, None) == INVALID         # null data, bytes above 0
    assert f(h, _p(1), _p(1), (1 << 40) + 1, 8, 1, None, None, _p(1), None, None) == INVALID
    assert f(h, _p(1), _p(1), 1, 1 << 62, 1, None, None, _p(1), None, None) == INVALID
    assert f(h, _p(1), None, 0, 0, 1, None, None, _p(1), None, None) == INVALID         # judged before num_seqs == 0


def test_a_live_handle_judges_the_rest(kmc):
    for L in libs(kmc):
        rc, h = create(L)
        if rc == OK:  # a device is present
            try:
                live_handle_errors(L, h)
            finally:
                L.kmc_sketch_accum_free(h)
        else:  # no device: no handle to judge them on (test_sketch_match_gpu.test_optional_outputs does)
            assert rc == NOMEM and not h.value


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, timeout=120)


def recruit_option_checks(tmp_path):
    """The option combinations of --recruit, judged before any device or file is touched
    (also run by test_sketch_match_cli.py, where a device is present)."""
    out = run(["--help"]).stdout.decode()
    assert "--recruit FILE" in out and "--min-hits H" in out and "--min-fraction F" in out
    assert "read_matches.tsv" in out and "read_matches_summary.tsv" in out
    fq, fa = tmp_path / "absent.fq", tmp_path / "absent.fa"
    rc = ["--canonical", "-k", 21, "--recruit", fq, "--accum-slots", 20]
    bad = [
        (["-k", 8, "--recruit", fq, "--accum-slots", 20, fa], b"--recruit needs --canonical"),
        (["--canonical", "-k", 21, "--recruit", fq, fa], b"--recruit needs --accum-slots"),
        (["--canonical", "-k", 21, "--recruit", fq, "--accum-slots", 0, fa], b"--recruit needs --accum-slots"),
        (rc + ["--sketch", 64, fa], b"--recruit matches reads against the k-mers of the input files"),
        (rc + ["--sketch", 64, "--sketch-direct", "--screen", fq, fa], b"--recruit matches"),
        (rc + ["--sketch", 64, "--sketch-direct", "--query", fq, fa], b"--recruit matches"),
        (rc + ["--sketch", 64, "--cluster", 0.1, fa], b"--recruit matches"),
        (rc + ["--sketch", 64, "--pairs", 0.1, fa], b"--recruit matches"),
        (rc + ["--distances", fa], b"--recruit matches"),
        (rc + ["--sketch", 64, "--sketch-direct", "--per-file", "--spectrum", 256, fa], b"--recruit matches"),
        (rc + ["--min-abundance", "auto", fa], b"--min-abundance auto"),
        (rc + ["--max-seqs", 5, fa], b"--recruit reads every file whole"),
        (rc + ["--min-abundance", 2, "--max-seqs", 5, fa], b"--recruit reads every file whole"),
        (rc + ["--min-hits", -1, fa], b"--min-hits"),
        (rc + ["--min-fraction", 1.5, fa], b"--min-fraction"),
        (rc + ["--min-fraction", "x", fa], b"--min-fraction"),
        (["--canonical", "-k", 21, "--min-hits", 2, fa], b"--min-hits and --min-fraction"),
        (["--canonical", "-k", 21, "--min-fraction", 0.5, fa], b"--min-hits and --min-fraction"),
    ]
    for args, msg in bad:
        r = run(args)
        assert r.returncode == 2, (args, r.stderr[:200])
        assert msg in r.stderr and b"usage:" in r.stderr, (args, r.stderr[:300])
    # accepted: what fails is the missing device or input (1), not the options
    for args in (rc + [fa], rc + [fa, fq], rc + ["--max-seqs", 0, fa],
                 rc + ["--recruit", fa, "--min-abundance", 2, "--min-hits", 3, "--min-fraction", 0.5, "--batch", 4096, fa]):
        assert run(args).returncode == 1, args


def test_recruit_option_combinations(tmp_path):
    recruit_option_checks(tmp_path)
