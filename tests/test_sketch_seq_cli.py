"""`kmc --canonical --sketch S --sketch-direct`: the sketches come straight from the
record buffer (kmc_sketch_from_sequences); sketch_results.csv is the file the run
without the flag writes."""
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


def test_sketch_direct_option_is_parsed(tmp_path):
    assert "--sketch-direct" in run(["--help"]).stdout
    absent = tmp_path / "absent.fa"
    ok = ["--canonical", "--sketch", 64, "--sketch-direct", "-k", 21]
    for args in (["--sketch-direct"], ["--canonical", "--sketch-direct"], ["--sketch", 64, "--sketch-direct"],
                 ok + ["--min-count", 2], ok + ["--counts", tmp_path / "c.tsv"], ok + ["--distances"]):
        r = run(args + [absent])
        assert r.returncode == 2, args
        assert "usage:" in r.stderr
    # accepted: what fails is the missing input (1), not the options; --min-count 1 filters nothing
    assert run(ok + [absent]).returncode == 1
    assert run(ok + ["--min-count", 1, absent]).returncode == 1


@pytest.mark.gpu
def test_cli_sketch_direct_csv(kmc, cuda, tmp_path):
    import torch
    k, s = 21, 64
    g = G.load("random", "nonl")
    d = torch.from_numpy(np.ascontiguousarray(g["data"])).to(cuda)
    di = torch.from_numpy(G.full_indices(g)).to(cuda)
    exp = kmc.sketch_distances(*kmc.sketch_from_sequences(d, di, k, s), k)
    torch.cuda.synchronize()
    exp = exp.cpu().numpy()
    assert exp.size > 0
    outs = []
    for name, extra in (("direct", ["--sketch-direct"]), ("counts", [])):
        out = tmp_path / name
        out.mkdir()
        r = run(["-k", k, "--canonical", "--sketch", s, "--dialect", "nonl", "--out", out, RANDOM_FA] + extra)
        assert r.returncode == 0, r.stderr
        assert "Sketch (s=64):" in r.stdout and "Sketch distances:" in r.stdout
        # the canonical counter's progress line only without the flag
        assert ("Canonical k=21" in r.stdout) == (name == "counts")
        outs.append(open(out / "sketch_results.csv", "rb").read())
    assert outs[0] == outs[1]
    lines = outs[0].decode().splitlines()
    assert len(lines) == exp.size
    for i, (line, e) in enumerate(zip(lines, exp)):
        assert np.isnan(float(line)) if np.isnan(e) else line == "%f" % e, "line %d: %s vs %f" % (i, line, e)
