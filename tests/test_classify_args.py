"""The classify entry points without a device: the symbols exist in the header and in both
libraries, the refusals that need no live handle come back before any device is touched,
the workspace query gives 0 for what the call refuses, and the kmc binary judges the
option combinations of --classify before any device or file is touched.  The refusals
judged on a live handle are test_classify_gpu.test_arguments_on_a_live_handle's."""
import ctypes
import os
import subprocess

from test_sketch_accum_args import libs

NAMES = {"kmc_label_accum": 7, "kmc_classify_workspace_size": 4, "kmc_classify_from_accum": 18,
         "kmc_classify_select": 10}
OK, INVALID = 0, 1001

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")

_buf = (ctypes.c_char * 64)()
P = ctypes.c_void_p(ctypes.addressof(_buf))  # a host address that is never dereferenced (arguments are checked first)


def test_header_and_libraries_have_the_symbols(kmc):
    names = kmc.header_symbols()
    for name, nargs in NAMES.items():
        assert name in names
        for L in libs(kmc):
            assert len(getattr(L, name).argtypes) == nargs
    for path in (kmc.LIB_PATH, kmc.DIAG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert callable(kmc.SketchAccum.label) and callable(kmc.SketchAccum.classify) and callable(kmc.classify_select)
    assert kmc.CLASSIFY_MAX_SOURCES == 32 and kmc.CLASSIFY_NONE == 0xFFFFFFFF


def test_null_handle_needs_no_device(kmc):
    for L in libs(kmc):
        f = L.kmc_classify_from_accum
        assert f(None, P, P, 1, 8, 2, 1, P, P, P, P, P, P, P, P, None, 0, None) == INVALID
        assert f(None, None, None, 0, 0, 1, 1, None, None, None, None, None, None, None, None, None, 0, None) == INVALID
        g = L.kmc_label_accum
        assert g(None, P, P, 1, 8, 0, None) == INVALID
        assert g(None, None, None, 0, 0, 0, None) == INVALID  # the handle before num_seqs == 0
        assert g(None, P, P, 1, 8, 32, None) == INVALID


def test_select_refusals_need_no_device(kmc):
    for L in libs(kmc):
        f = L.kmc_classify_select
        assert f(None, P, P, P, 1, 32, 1, P, None, None) == INVALID  # source >= 32
        assert f(None, P, P, P, 0, 32, 1, P, None, None) == INVALID  # judged before num_seqs == 0
        assert f(P, None, P, P, 1, 0, 1, P, None, None) == INVALID
        assert f(P, P, None, P, 1, 0, 1, P, None, None) == INVALID
        assert f(P, P, P, None, 1, 0, 1, P, None, None) == INVALID
        assert f(P, P, P, P, 1, 0, 1, None, None, None) == INVALID
        assert f(None, P, P, P, (1 << 40) + 1, 0, 1, P, None, None) == INVALID


def test_workspace_query_zeros(kmc):
    for L in libs(kmc):
        q = L.kmc_classify_workspace_size
        assert q(1, 100, 0, 0) == 0 and q(1, 100, 33, 0) == 0
        assert q((1 << 40) + 1, 100, 2, 0) == 0
        assert q(1, 1 << 62, 2, 0) == 0
        assert q(1, 100, 2, -1) == 0
    assert kmc.classify_workspace_size(1, 100, 0) == 0


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, timeout=120)


def classify_option_checks(tmp_path):
    """The option combinations of --classify, judged before any device or file is touched
    (also run by test_classify_cli.py, where a device is present)."""
    out = run(["--help"]).stdout.decode()
    assert "--classify" in out and "--min-margin D" in out and "--write-sources" in out
    assert "read_sources.tsv" in out and "read_sources_summary.tsv" in out and "source_<f>_<g>.fastq" in out
    fq, fa, fb = tmp_path / "absent.fq", tmp_path / "absent.fa", tmp_path / "absent2.fa"
    rc = ["--canonical", "-k", 21, "--recruit", fq, "--accum-slots", 20]
    bad = [
        (["--canonical", "-k", 21, "--classify", fa], b"--classify, --min-margin and --write-sources"),
        (["--canonical", "-k", 21, "--min-margin", 2, fa], b"--classify, --min-margin and --write-sources"),
        (["--canonical", "-k", 21, "--write-sources", fa], b"--classify, --min-margin and --write-sources"),
        (rc + ["--write-sources", fa], b"need --classify"),
        (rc + ["--min-margin", 1, fa], b"need --classify"),
        (rc + ["--classify", "--min-margin", -1, fa], b"--min-margin"),
        (rc + ["--classify", "--min-margin", "x", fa], b"--min-margin"),
        (["--canonical", "-k", 21, "--recruit", fa, "--accum-slots", 20, "--classify", "--write-sources", fa, fb],
         b"--write-sources writes FASTQ records"),
        (rc + ["--classify"] + [tmp_path / ("in%d.fa" % i) for i in range(33)], b"32 sources apart at most"),
    ]
    for args, msg in bad:
        r = run(args)
        assert r.returncode == 2, (args, r.stderr[:200])
        assert msg in r.stderr and b"usage:" in r.stderr, (args, r.stderr[:300])
    # accepted: what fails is the missing device or input (1), not the options
    for args in (rc + ["--classify", fa, fb], rc + ["--classify", "--min-margin", 0, "--write-sources", fa],
                 rc + ["--classify"] + [tmp_path / ("in%d.fa" % i) for i in range(32)]):
        assert run(args).returncode == 1, args


def test_classify_option_combinations(tmp_path):
    classify_option_checks(tmp_path)


def test_a_fifo_is_refused_before_anything_is_read(tmp_path):
    """An input that cannot be read twice: refused while the options are judged; nobody ever
    opens the FIFO, so a driver that did would block until the time limit."""
    fifo, fa = tmp_path / "pipe.fa", tmp_path / "absent.fa"
    os.mkfifo(fifo)
    r = run(["--canonical", "-k", 21, "--recruit", tmp_path / "absent.fq", "--accum-slots", 20, "--classify", fa, fifo])
    assert r.returncode == 2 and b"is not a regular file" in r.stderr and b"pipe.fa" in r.stderr, r.stderr
