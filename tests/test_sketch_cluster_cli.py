"""`kmc --canonical --sketch S [--sketch-direct] [--per-file] --cluster D input.fa`: the
option is parsed and its combinations judged before any device or file is touched.
What the run writes is checked on the GPU (test_sketch_cluster_gpu.py)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_help_lists_the_cluster_option():
    r = run(["--help"])
    assert r.returncode == 0
    assert "--cluster" in r.stdout and "clusters.tsv" in r.stdout and "kmc_sketch_cluster" in r.stdout


def test_cluster_option_combinations(tmp_path):
    fa, other = tmp_path / "absent.fa", tmp_path / "absent_other.fa"
    counted = ["--canonical", "--sketch", 64, "-k", 21]
    direct = counted + ["--sketch-direct"]
    bad = [
        ["--cluster", 0.05],                                     # nothing it needs
        ["--canonical", "--cluster", 0.05],                      # no --sketch
        ["--canonical", "--sketch-direct", "--cluster", 0.05],   # no --sketch
        ["--sketch", 64, "--cluster", 0.05],                     # no --canonical
        direct + ["--cluster", 0.05, "--query", other],
        direct + ["--cluster", 0.05, "--screen", other],
        direct + ["--query", other, "--top", 0, "--cluster", 0.05],
        direct + ["--cluster", -0.01],
        direct + ["--cluster", 1.01],
        direct + ["--cluster", "nan"],
        direct + ["--cluster", "inf"],
        direct + ["--cluster", "0.05x"],
        direct + ["--cluster", ""],
        direct + ["--cluster", "-1e-300"],
    ]
    for args in bad:
        r = run(args + [fa])
        assert r.returncode == 2, args
        assert "usage:" in r.stderr, args
    # accepted: what fails is the missing device or input (1), not the options, wherever they stand
    good = [
        counted + ["--cluster", 0.05],
        counted + ["--cluster", 0.05, "--min-count", 2],
        direct + ["--cluster", 0.05],
        direct + ["--cluster", 0],
        direct + ["--cluster", 1],
        direct + ["--cluster", "1e-3"],
        ["--cluster", 0.5] + direct,
        direct + ["--per-file", "--cluster", 0.05],
        direct + ["--per-file", "--min-abundance", 2, "--cluster", 0.05],
    ]
    for args in good:
        assert run(args + [fa]).returncode == 1, args
    assert run(direct + ["--per-file", "--cluster", 0.05, fa, other]).returncode == 1
    # without --per-file a second input file is refused as before
    r = run(direct + ["--cluster", 0.05, fa, other])
    assert r.returncode == 2 and "more than one input file" in r.stderr
    # an option that lost its value
    assert run(direct + [fa, "--cluster"]).returncode == 2
