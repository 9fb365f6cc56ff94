"""kmc_spectrum_from_accum and kmc_spectrum_summarize without a device: the symbols
exist, argument errors come back before any device is touched, the summary equals the
Python model of spectrum_util (integers equal, doubles bit for bit), and the kmc
binary judges the option combinations of --spectrum and --min-abundance auto before
any device or file is touched."""
import ctypes
import os
import subprocess

import numpy as np

import spectrum_util as P

NAMES = ["kmc_spectrum_from_accum", "kmc_spectrum_summarize"]
OK, INVALID = 0, 1001
FILL = P.FILL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")
SK = ["--canonical", "--sketch", 64, "--sketch-direct", "-k", 21]

_buf = (ctypes.c_char * 64)()


def _p(on):
    """Null or a host address that is never dereferenced (arguments are checked first)."""
    return ctypes.c_void_p(ctypes.addressof(_buf)) if on else None


def libs(kmc):
    yield kmc.lib()
    with kmc.diag() as D:
        yield D


def test_header_and_libraries_have_the_symbols(kmc):
    names = kmc.header_symbols()
    assert len([n for n in names if n.startswith("kmc_sketch_accum_")]) == 6
    assert "#define KMC_SPECTRUM_MAX_BINS 8192" in open(kmc.HEADER).read()
    for L in libs(kmc):
        for n in NAMES:
            assert n in names and getattr(L, n).argtypes is not None
        assert [len(getattr(L, n).argtypes) for n in NAMES] == [5, 4]
        assert L.kmc_version() == 200
    for path in (kmc.LIB_PATH, kmc.DIAG_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert set(NAMES) <= set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert kmc.SPECTRUM_MAX_BINS == P.MAX_BINS == 8192
    assert callable(kmc.SketchAccum.spectrum) and callable(kmc.spectrum_summarize)


def test_null_handle_needs_no_device(kmc):
    for L in libs(kmc):
        assert L.kmc_spectrum_from_accum(None, 256, _p(1), _p(1), None) == INVALID
        assert L.kmc_spectrum_from_accum(None, 256, None, None, None) == INVALID
        assert L.kmc_spectrum_from_accum(None, 0, _p(1), None, None) == INVALID


def test_summarize_refuses_bad_arguments(kmc):
    hist = (ctypes.c_uint64 * 8)(0, 5, 3, 1, 2, 4, 1, 0)
    out = kmc.SpectrumSummary()
    for L in libs(kmc):
        f = L.kmc_spectrum_summarize
        assert f(hist, 8, FILL, ctypes.byref(out)) == OK
        assert f(None, 8, FILL, ctypes.byref(out)) == INVALID
        assert f(hist, 8, FILL, None) == INVALID
        for B in (0, 1, 8193, 1 << 31):
            assert f(hist, B, FILL, ctypes.byref(out)) == INVALID, B
        assert f(hist, 8, 0, ctypes.byref(out)) == INVALID
        assert f(hist, 2, 1, ctypes.byref(out)) == OK


def read_like(B, valley=4, peak=30):
    """Error k-mers falling from bin 1, a valley, a coverage peak, an empty tail."""
    h = [0] * B
    for c in range(1, valley):
        h[c] = 9000 >> (2 * (c - 1)) | 1
    for c in range(valley, min(2 * peak, B - 1)):
        h[c] = max(1, 400 - 3 * (c - peak) ** 2)
    return h


LIMITS = [FILL, 1 << 54, 0x00C3_9A5D_7711_0F2B]  # unbounded, a level's bound, an odd `lost` value

HISTS = {
    "read-like": (read_like(64), dict(valley=4, peak=30, min_abundance=4, saturated=0)),
    "monotone": ([0, 900, 400, 100, 50, 20, 9, 3], dict(valley=0, peak=0, min_abundance=1, genome_size=0.0)),
    "monotone, empty tail": ([0, 900, 400, 100, 0, 0, 0, 0, 0, 0], dict(valley=0, peak=0, min_abundance=1,
                                                                      genome_size=0.0)),
    "assembly": ([0, 3980] + [0] * 254, dict(valley=0, peak=0, min_abundance=1, genome_size=0.0)),
    "ties at the peak": ([0, 50, 7, 3, 20, 90, 14, 90, 90, 6, 0, 0], dict(valley=3, peak=5)),
    "plateau is a valley": ([0, 50, 7, 7, 3, 40, 2, 0], dict(valley=2, peak=5)),
    "valley at B - 3": ([0, 50, 30, 20, 10, 5, 9, 1], dict(valley=5, peak=6, saturated=1)),
    "rise only into the last bin": ([0, 50, 30, 20, 10, 5, 4, 77], dict(valley=0, peak=0, min_abundance=1,
                                                                         saturated=1, genome_size=0.0)),
    "empty valley floor": ([0, 50, 4, 0, 0, 0, 6, 30, 8, 0, 0, 0], dict(valley=5, peak=7)),
    "B = 2": ([0, 12], dict(valley=0, peak=0, min_abundance=1, saturated=1, sampled_distinct=12, sampled_total=12)),
    "B = 2, nothing": ([3, 0], dict(valley=0, saturated=0, sampled_distinct=0, sampled_total=0)),
    "B = 3": ([0, 5, 9], dict(valley=0, peak=0, min_abundance=1, saturated=1, sampled_distinct=14, sampled_total=23)),
    "non-zero last bin": (read_like(40, 3, 25)[:39] + [17], dict(valley=3, peak=25, saturated=1)),
    "first bin below the second": ([0, 2, 9, 4, 1, 0], dict(valley=1, peak=2, min_abundance=1)),
    "wrapped count in bin 0": ([5, 40, 3, 30, 2, 0], dict(valley=2, peak=3)),
    "total wraps at 2^64": ([0, 1 << 63, 1 << 62, 1 << 61, 9], dict(valley=0, saturated=1, sampled_total=(3 << 61) + 36)),
    "all bins": ([0] + [(c * 2654435761) % 1000 for c in range(1, 8192)], {}),
}


def test_summary_equals_the_model_bit_for_bit(kmc):
    for name, (hist, known) in HISTS.items():
        for limit in LIMITS:
            exp = P.summarize(hist, limit)
            for f, v in known.items():
                assert getattr(exp, f) == v, "the model, %s: %s is %s" % (name, f, getattr(exp, f))
            assert exp.scale == (1.0 if limit == FILL else 2.0 ** 64 / limit) and exp.scale >= 1.0
            for L in libs(kmc):
                got = kmc.spectrum_summarize(np.array(hist, dtype=np.uint64), limit)
                P.assert_summary(got, exp, "%s limit=%d" % (name, limit))
    # the genome size of the read-like one: the k-mers from the valley on over the peak
    h = HISTS["read-like"][0]
    s = P.summarize(h, 1 << 54)
    assert s.scale == 1024.0 and s.genome_size == 1024.0 * sum(c * h[c] for c in range(4, 64)) / 30
    # int64 bit patterns (the tensors of SketchAccum.spectrum) are taken as uint64
    wrapped = np.array([0, -1, 5], dtype=np.int64)
    assert kmc.spectrum_summarize(wrapped, FILL).sampled_distinct == (FILL + 5) & FILL


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, timeout=120)


def test_spectrum_option_combinations(tmp_path):
    out = run(["--help"]).stdout.decode()
    assert "--spectrum B" in out and "auto" in out and "--spectrum B [--min-abundance auto]" in out
    fq, fa = tmp_path / "absent.fq", tmp_path / "absent.fa"
    pf = SK + ["--per-file"]
    bad = [
        ["--spectrum", 256, fa],                                        # nothing it needs
        ["--canonical", "--spectrum", 256, fa],
        ["--canonical", "--sketch", 64, "--spectrum", 256, fa],         # no --sketch-direct
        SK + ["--spectrum", 256, fa],                                   # no --per-file
        SK + ["--spectrum", 256, "--query", fq, fa],
        SK + ["--spectrum", 256, "--screen", fq, fa],
        ["--canonical", "--sketch", 64, "--per-file", "--spectrum", 256, fa],
        pf + ["--spectrum", 0, fa], pf + ["--spectrum", 1, fa], pf + ["--spectrum", 8193, fa],
        pf + ["--spectrum", -5, fa], pf + ["--spectrum", "auto", fa],
        pf + ["--spectrum", 256, "--max-seqs", 5, fa],
        pf + ["--min-abundance", "auto", "--max-seqs", 5, fa],
        SK + ["--min-abundance", "auto", fa],                           # no --per-file
        ["--min-abundance", "auto", fa],
        pf + ["--accum-slots", 20, fa], pf + ["--batch", 4096, fa],     # without both they stay refused
        pf + ["--spectrum", 256, "--accum-slots", 3, fa], pf + ["--spectrum", 256, "--batch", -1, fa],
        pf + ["--min-abundance", 0, fa], pf + ["--min-abundance", -1, fa], pf + ["--min-abundance", 1 << 32, fa],
        pf + ["--min-abundance", "automatic", fa], pf + ["--min-abundance", "", fa],
        pf + ["--spectrum", 256, "--min-abundance", 0, fa],
    ]
    for args in bad:
        r = run(args)
        assert r.returncode == 2, (args, r.stderr[:200])
        assert b"usage:" in r.stderr, (args, r.stderr[:200])
    assert run(pf + [fa, "--spectrum"]).returncode == 2
    assert run(pf + ["--min-count", 2, "--spectrum", 256, fa]).returncode == 2  # --sketch-direct never counts
    # accepted: what fails is the missing device or input (1), not the options
    for args in (pf + ["--spectrum", 256, fq], pf + ["--spectrum", 2, fa, fq], pf + ["--spectrum", 8192, fa],
                 pf + ["--spectrum", 256, "--accum-slots", 20, fa],
                 pf + ["--spectrum", 256, "--accum-slots", 20, "--batch", 4096, "--max-seqs", 0, fq],
                 pf + ["--spectrum", 256, "--min-abundance", 2, fq],
                 pf + ["--min-abundance", "auto", fq], pf + ["--min-abundance", "auto", "--accum-slots", 20, fa],
                 pf + ["--spectrum", 512, "--min-abundance", "auto", "--batch", 4096, fq, fa],
                 pf + ["--min-abundance", "auto", "--query", fq, fa],
                 pf + ["--min-abundance", "auto", "--screen", fq, fa],
                 pf + ["--spectrum", 256, "--query", fq, fa], pf + ["--spectrum", 256, "--screen", fq, fa],
                 pf + ["--spectrum", 256, "--cluster", 0.1, fa],
                 pf + ["--spectrum", 256, "--format", "fastq", "/dev/stdin"]):
        assert run(args).returncode == 1, args
