"""`kmc --canonical --distances`: step 2 on the canonical counts, written to the
two CSVs of --out with the dense path's "%f\\n" writer."""
import os
import subprocess

import numpy as np
import pytest

import golden_util as G
import sparse_dist_util as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")
RANDOM_FA = os.path.join(G.GOLDEN, "random.fa")
CSVS = ("parallel_results.csv", "sequential_results.csv")


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_distances_option_is_parsed(tmp_path):
    assert "--distances" in run(["--help"]).stdout
    # accepted with and without --canonical: what fails below is the missing input (1), not the option (2)
    assert run(["--distances", tmp_path / "absent.fa"]).returncode == 1
    assert run(["--canonical", "--distances", "-k", "31", tmp_path / "absent.fa"]).returncode == 1
    # the existing option errors stay
    assert run(["--canonical", "--distances", "-k", "32", "x.fa"]).returncode == 2
    assert run(["--distances", "-k", "14", "x.fa"]).returncode == 2
    assert run(["--distances"]).returncode == 2


def assert_csv_matches(path, exp, msg):
    with open(path) as f:
        lines = f.read().splitlines()
    exp = np.asarray(exp, dtype=np.float32)
    assert len(lines) == exp.size, msg
    for i, (line, e) in enumerate(zip(lines, exp)):
        if np.isnan(e):
            assert np.isnan(float(line)), "%s line %d: %s vs nan" % (msg, i, line)
        else:
            assert line == "%f" % e, "%s line %d: %s vs %f" % (msg, i, line, e)


@pytest.mark.gpu
def test_cli_canonical_distances_csv(cuda, oracle, tmp_path):
    g = G.load("random", "nonl")
    exp = U.canonical_expected(oracle, g["data"], G.full_indices(g), 31)
    r = run(["-q", "--canonical", "--distances", "-k", 31, "--dialect", "nonl", "--out", tmp_path, RANDOM_FA])
    assert r.returncode == 0, r.stderr
    for name in CSVS:
        assert_csv_matches(tmp_path / name, exp, name)


@pytest.mark.gpu
def test_cli_canonical_without_distances_writes_no_csv(cuda, tmp_path):
    r = run(["-q", "--canonical", "-k", 31, "--dialect", "nonl", "--out", tmp_path, RANDOM_FA])
    assert r.returncode == 0, r.stderr
    assert not any((tmp_path / name).exists() for name in CSVS)
