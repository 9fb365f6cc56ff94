"""`kmc ... --screen reads.fa --winner-takes-all refs.fa`: screen_results.tsv credits every
found sketch value to the best reference that holds it (kmc_sketch_screen_winners) and
gains the column shared_all.  The option combinations are judged before any device or
file is touched; without the option the file is what it was."""
import numpy as np
import pytest

import sketch_screen_util as U
import sketch_screen_winners_util as W
import sketch_util as S
from test_sketch_screen_cli import RANDOM_FA, expected_lines, run, sequences, write_fasta


NEEDS = "kmc: --winner-takes-all credits the values of --screen"


def test_winner_takes_all_option_combinations(tmp_path):
    out = run(["--help"]).stdout
    assert "--winner-takes-all" in out and "shared_all" in out and "kmc_sketch_screen_winners" in out
    refs, reads = tmp_path / "absent_refs.fa", tmp_path / "absent_reads.fa"
    ok = ["--canonical", "--sketch", 64, "--sketch-direct", "-k", 21]
    bad = [
        (["--winner-takes-all"], NEEDS),
        (ok + ["--winner-takes-all"], NEEDS),
        (ok + ["--per-file", "--winner-takes-all"], NEEDS),
        (ok + ["--winner-takes-all", "--query", reads], NEEDS),
        (ok + ["--winner-takes-all", "--cluster", "0.1"], NEEDS),
    ]
    for args, message in bad:
        r = run(args + [refs])
        assert r.returncode == 2, args
        assert "usage:" in r.stderr and message in r.stderr, (args, r.stderr[:200])
    # accepted: what fails is the missing device or input (1), not the options, wherever they stand
    for args in (ok + ["--screen", reads, "--winner-takes-all"], ["--winner-takes-all", "--screen", reads] + ok,
                 ok + ["--per-file", "--winner-takes-all", "--screen", reads],
                 ok + ["--screen", reads, "--screen", refs, "--winner-takes-all", "-q"]):
        assert run(args + [refs]).returncode == 1, args
    # it takes no value: the next word is the input file
    r = run(ok + ["--screen", reads, "--winner-takes-all", refs, tmp_path / "absent_more.fa"])
    assert r.returncode == 2 and "more than one input file" in r.stderr


def mutated(seq, every, shift):
    """seq with every `every`-th base, from `shift` on, replaced by the next base of ACGT."""
    b = bytearray(seq.encode())
    for i in range(shift, len(b), every):
        b[i] = b"CGTA"[b"ACGT".index(b[i])]
    return b.decode()


@pytest.mark.gpu
def test_cli_winner_takes_all_tsv(kmc, oracle, cuda, tmp_path):
    """Three reference files, one genome each: r0 and r1 are near-identical (r1 is r0 with a
    base in 400 changed), r2 is unrelated; the mixture holds r0.  Plainly screened, r1 is
    nearly as contained as r0; with --winner-takes-all r0 takes what the two share."""
    k, s = 21, 64
    g = sequences(RANDOM_FA)
    r0 = write_fasta(tmp_path / "r0.fa", [g[0][:3000], g[0][3000:6000]])
    r1 = write_fasta(tmp_path / "r1.fa", [mutated(g[0][:6000], 400, 123)])
    r2 = write_fasta(tmp_path / "r2.fa", [g[2][:6000]])
    reads = write_fasta(tmp_path / "reads.fa", [g[0][:3000], g[0][3000:6000], g[1][:2000]])
    out = tmp_path / "out"
    out.mkdir()
    base = ["-k", k, "--canonical", "--sketch", s, "--sketch-direct", "--dialect", "nonl", "--out", out, "--per-file",
            "--screen", reads]
    paths = [r0, r1, r2]
    files = [kmc.load_fasta(str(p), kmc.DIALECT_NONL, 0)[:2] for p in paths]
    plain, sh, sizes, med = expected_lines(kmc, oracle, files, [reads], k, s, paths=paths)

    r = run(base + paths)
    assert r.returncode == 0, r.stderr
    assert "Screen results:" in r.stdout and "Screen winners:" not in r.stdout
    assert open(out / "screen_results.tsv").read().splitlines() == plain

    r = run(base + ["--winner-takes-all"] + paths)
    assert r.returncode == 0, r.stderr
    assert "Screen winners:" in r.stdout and "Screen results:" not in r.stdout
    # the oracle's lines from the same rows
    data, idx, _ = kmc.load_fasta(str(reads), kmc.DIALECT_NONL, 0)
    mix = U.mixture_hashes(oracle, data, idx, k)
    rows = np.full((3, s), S.FILL, dtype=np.uint64)
    for i, (fd, fi) in enumerate(files):
        keys, _, _ = oracle.count_canonical(fd, fi, k)
        h = np.sort(S.hash_keys(np.unique(keys)))[:s]
        rows[i, :h.size] = h
        assert h.size == s == sizes[i]
    won, mwon, ident, all_ = W.winners_expected(mix, rows, sizes, s, k)
    assert list(all_) == list(sh)
    assert all_[0] == s and s // 2 < all_[1] < s and all_[2] == 0, "r1 is nearly as contained as r0 in the plain screen"
    assert won[0] == s and 0 <= won[1] < all_[1] // 4 and won[2] == 0, "r0 takes what the two share"
    exp = ["%d\t%d\t%d\t%d\t%f\t%d\t%s" % (i, won[i], sizes[i], mwon[i], ident[i], all_[i], paths[i]) for i in range(3)]
    got = open(out / "screen_results.tsv").read().splitlines()
    assert got == exp
    assert got != plain

    # quiet: no timing line; without --per-file the path column goes and shared_all is last
    r = run(["-k", k, "--canonical", "--sketch", s, "--sketch-direct", "--dialect", "nonl", "--max-seqs", 0, "--out", out,
             "-q", "--screen", reads, "--winner-takes-all", r0])
    assert r.returncode == 0, r.stderr
    assert "Screen winners" not in r.stdout
    lines = open(out / "screen_results.tsv").read().splitlines()
    assert len(lines) == 2 and all(len(x.split("\t")) == 6 for x in lines)
