"""`kmc --canonical --sketch S`: MinHash sketches of the canonical counts and their
Mash distances, written to sketch_results.csv in --out with the "%f\\n" writer."""
import os
import subprocess

import numpy as np
import pytest

import golden_util as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")
RANDOM_FA = os.path.join(G.GOLDEN, "random.fa")


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_sketch_options_are_parsed(tmp_path):
    out = run(["--help"]).stdout
    assert "--sketch" in out and "--min-count" in out
    # without --canonical: a usage error (2), before the input is looked at
    for args in (["--sketch", 64], ["--min-count", 2], ["--sketch", 64, "--min-count", 2, "-k", 5]):
        r = run(args + [tmp_path / "absent.fa"])
        assert r.returncode == 2, args
        assert "usage:" in r.stderr
    assert run(["--canonical", "--sketch", 0, "x.fa"]).returncode == 2
    assert run(["--canonical", "--sketch", 16385, "x.fa"]).returncode == 2
    assert run(["--canonical", "--sketch"]).returncode == 2
    # accepted with --canonical: what fails is the missing input (1), not the option
    assert run(["--canonical", "--sketch", 64, "--min-count", 2, "-k", 21, tmp_path / "absent.fa"]).returncode == 1


def binding_distances(kmc, cuda, k, s, min_count=1):
    import torch
    g = G.load("random", "nonl")
    data, idx = g["data"], G.full_indices(g)
    d = torch.from_numpy(np.ascontiguousarray(data)).to(cuda)
    di = torch.from_numpy(idx).to(cuda)
    keys, counts, off = kmc.count_canonical(d, di, k)
    sk, sz = kmc.sketch_from_counts(keys, counts, off, s, min_count=min_count)
    out = kmc.sketch_distances(sk, sz, k)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_csv(path, exp):
    with open(path) as f:
        lines = f.read().splitlines()
    assert len(lines) == exp.size
    for i, (line, e) in enumerate(zip(lines, exp)):
        if np.isnan(e):
            assert np.isnan(float(line)), "line %d: %s vs nan" % (i, line)
        else:
            assert line == "%f" % e, "line %d: %s vs %f" % (i, line, e)


@pytest.mark.gpu
def test_cli_sketch_csv(kmc, cuda, tmp_path):
    exp = binding_distances(kmc, cuda, 21, 64)
    assert exp.size > 0
    r = run(["-k", 21, "--canonical", "--sketch", 64, "--dialect", "nonl", "--out", tmp_path, RANDOM_FA])
    assert r.returncode == 0, r.stderr
    assert "Sketch (s=64):" in r.stdout and "Sketch distances:" in r.stdout
    assert_csv(tmp_path / "sketch_results.csv", exp)
    assert not (tmp_path / "parallel_results.csv").exists()
    # -q prints no progress lines; --min-count reaches the library
    out2 = tmp_path / "q"
    out2.mkdir()
    r = run(["-q", "-k", 5, "--canonical", "--sketch", 64, "--min-count", 2, "--dialect", "nonl", "--out", out2,
             RANDOM_FA])
    assert r.returncode == 0, r.stderr
    assert "Sketch" not in r.stdout
    assert_csv(out2 / "sketch_results.csv", binding_distances(kmc, cuda, 5, 64, min_count=2))


@pytest.mark.gpu
def test_cli_sketch_with_distances_writes_all_three(cuda, tmp_path):
    r = run(["-q", "-k", 21, "--canonical", "--sketch", 64, "--distances", "--dialect", "nonl", "--out", tmp_path,
             RANDOM_FA])
    assert r.returncode == 0, r.stderr
    sizes = [len(open(tmp_path / name).read().splitlines())
             for name in ("sketch_results.csv", "parallel_results.csv", "sequential_results.csv")]
    assert sizes[0] > 0 and sizes[0] == sizes[1] == sizes[2]
