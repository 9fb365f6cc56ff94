"""`kmc --canonical --sketch S --sketch-direct --per-file a.fa b.fa ...`: every input
file is one sketch of all its records (kmc_sketch_from_sequences_grouped), and
sketch_results.csv is the packed triangle over the files in command-line order."""
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


def test_per_file_option_is_parsed(tmp_path):
    assert "--per-file" in run(["--help"]).stdout
    a, b = tmp_path / "absent_a.fa", tmp_path / "absent_b.fa"
    ok = ["--canonical", "--sketch", 64, "--sketch-direct", "--per-file", "-k", 21]
    for args in (["--per-file"], ["--canonical", "--per-file"], ["--canonical", "--sketch", 64, "--per-file"],
                 ["--sketch", 64, "--sketch-direct", "--per-file"], ["--canonical", "--sketch-direct", "--per-file"],
                 ok + ["--min-count", 2], ok + ["--distances"]):
        r = run(args + [a, b])
        assert r.returncode == 2, args
        assert "usage:" in r.stderr
    # accepted: what fails is the missing input (1), not the options, wherever the flag stands
    assert run(ok + [a, b]).returncode == 1
    assert run(ok[:-3] + ["-k", 21, a, b, "--per-file"]).returncode == 1
    assert run(ok + [a]).returncode == 1
    # without the flag a second file is refused as before
    r = run(ok[:4] + [a, b])
    assert r.returncode == 2 and "more than one input file" in r.stderr


def split_records(path, parts):
    """The '>' records of a FASTA file, dealt in order into `parts` lists of whole records."""
    recs, cur = [], None
    for line in open(path):
        if line.startswith(">"):
            cur = []
            recs.append(cur)
        if cur is not None:
            cur.append(line)
    cuts = [len(recs) * i // parts for i in range(parts + 1)]
    return [recs[cuts[i]:cuts[i + 1]] for i in range(parts)]


@pytest.mark.gpu
def test_cli_per_file_csv(kmc, cuda, tmp_path):
    import torch
    k, s = 21, 64
    g = G.load("random", "nonl")
    d = torch.from_numpy(np.ascontiguousarray(g["data"])).to(cuda)
    di = torch.from_numpy(G.full_indices(g)).to(cuda)
    files, counts, bufs = [], [], []
    for i, recs in enumerate(split_records(RANDOM_FA, 3)):
        p = tmp_path / ("part%d.fa" % i)
        p.write_text("".join("".join(r) for r in recs))
        files.append(p)
        pdata, pidx, _ = kmc.load_fasta(str(p), kmc.DIALECT_NONL, 0)
        counts.append(pidx.size - 1)
        bufs.append(pdata)
    # the three files hold the original buffer's records, in order
    np.testing.assert_array_equal(np.concatenate(bufs), g["data"])
    assert sum(counts) == di.numel() - 1 and min(counts) >= 1
    go = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=cuda)
    rows, sizes = kmc.sketch_from_sequences_grouped(d, di, go, k, s)
    exp = kmc.sketch_distances(rows, sizes, k)
    torch.cuda.synchronize()
    exp, sizes = exp.cpu().numpy(), sizes.cpu().numpy()
    assert exp.size == 3
    out = tmp_path / "out"
    out.mkdir()
    r = run(["-k", k, "--canonical", "--sketch", s, "--sketch-direct", "--per-file", "--dialect", "nonl", "--out", out]
            + files)
    assert r.returncode == 0, r.stderr
    for i, p in enumerate(files):
        assert "File %d: %s: %d records, sketch size %d" % (i, p, counts[i], sizes[i]) in r.stdout
    lines = open(out / "sketch_results.csv").read().splitlines()
    assert len(lines) == exp.size
    for i, (line, e) in enumerate(zip(lines, exp)):
        assert np.isnan(float(line)) if np.isnan(e) else line == "%f" % e, "line %d: %s vs %f" % (i, line, e)
