"""`kmc --canonical --sketch S --sketch-direct --query q.fa [--top T] [--min-shared M]
refs.fa`: the options are parsed and their combinations judged before any device or
file is touched.  What the run writes is checked on the GPU (test_sketch_query_gpu.py)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_help_lists_the_query_options():
    out = run(["--help"]).stdout
    for opt in ("--query", "--top", "--min-shared"):
        assert opt in out
    assert "query_results.tsv" in out and "query_distances.csv" in out


def test_query_option_combinations(tmp_path):
    refs, query = tmp_path / "absent_refs.fa", tmp_path / "absent_query.fa"
    ok = ["--canonical", "--sketch", 64, "--sketch-direct", "-k", 21]
    bad = [
        ["--query", query],                                            # nothing it needs
        ["--canonical", "--query", query],                             # no --sketch
        ["--canonical", "--sketch", 64, "--query", query],             # no --sketch-direct
        ["--sketch", 64, "--sketch-direct", "--query", query],         # no --canonical
        ["--canonical", "--sketch-direct", "--query", query],          # no --sketch
        ok + ["--top", 3],                                             # --top without --query
        ok + ["--min-shared", 2],                                      # --min-shared without --query
        ok + ["--per-file", "--top", 0],
        ok + ["--query", query, "--top", 1025],
        ok + ["--query", query, "--top", -1],
        ok + ["--query", query, "--min-shared", -1],
    ]
    for args in bad:
        r = run(args + [refs])
        assert r.returncode == 2, args
        assert "usage:" in r.stderr, args
    # accepted: what fails is the missing device or input (1), not the options, wherever they stand
    good = [
        ok + ["--query", query],
        ok + ["--query", query, "--top", 0],
        ok + ["--query", query, "--top", 1024, "--min-shared", 0],
        ["--query", query, "--top", 1] + ok,
        ok + ["--per-file", "--query", query, "--top", 5],
    ]
    for args in good:
        assert run(args + [refs]).returncode == 1, args
    assert run(ok + ["--per-file", "--query", query, refs, tmp_path / "absent_more.fa"]).returncode == 1
    # without --per-file a second reference file is refused as before
    r = run(ok + ["--query", query, refs, tmp_path / "absent_more.fa"])
    assert r.returncode == 2 and "more than one input file" in r.stderr
    # an option that lost its value
    assert run(ok + [refs, "--query"]).returncode == 2
