"""`kmc --canonical --sketch S [--sketch-direct] [--per-file] --pairs D [--query FILE] input.fa`:
pairs.tsv and query_pairs.tsv hold the binding's sorted lists of the rows the binding
sketches from the same files, line for line; the option's combinations are judged before
any device or file is touched.  Inputs, mutation and the choice of D are those of
test_sketch_cluster_gpu.py's driver tests."""
import numpy as np
import pytest

import sketch_util as S
from sketch_util import dev
from test_sketch_cluster_gpu import mutated, pick_distance, run, write_fasta

K, SKETCH = 21, 64


def u32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def lines_of(links, dist):
    """The driver's lines of a binding's sorted list."""
    return ["%d\t%d\t%d\t%d\t%f" % (i, j, sh, dn, float(d)) for (i, j, sh, dn), d in
            zip(u32(links).reshape(-1, 4).tolist(), dist.cpu().numpy())]


def nine_records(rng):
    base = [S.bases(rng, 3000) for _ in range(4)]
    return base, [base[0], base[1], mutated(rng, base[2], 0.02), base[0].copy(), base[2], base[3],
                  mutated(rng, base[1], 0.02), base[3].copy(), mutated(rng, base[2], 0.02)]


def rows_of(kmc, cuda, path):
    data, idx, _ = kmc.load_fasta(str(path), kmc.DIALECT_NONL, 0)
    return kmc.sketch_from_sequences(dev(data, cuda), dev(idx, cuda), K, SKETCH), idx.size - 1


@pytest.mark.gpu
def test_cli_pairs(kmc, cuda, tmp_path):
    """A few random records, exact copies of some and copies with about 2 % substitutions:
    the copies and each mutant with its original are within D, and no other pair: two
    mutants of one original are not."""
    import torch
    rng = np.random.default_rng(8)
    _, records = nine_records(rng)
    fa = tmp_path / "records.fa"
    write_fasta(fa, records)
    (rows, sizes), n = rows_of(kmc, cuda, fa)
    assert n == len(records)
    _, sh, dn = kmc.sketch_distances(rows, sizes, K, with_counts=True)
    torch.cuda.synchronize()
    D = pick_distance(u32(sh), u32(dn), K)
    links, dist, count = kmc.sketch_links(rows, sizes, K, kmc.mash_jaccard_of_distance(D, K))
    assert u32(links).reshape(-1, 4)[:, :2].tolist() == [[0, 3], [1, 6], [2, 4], [4, 8], [5, 7]] and count.tolist() == [5]
    exp = lines_of(links, dist)
    opts = ["-k", K, "--canonical", "--sketch", SKETCH, "--dialect", "nonl", "--max-seqs", 0]
    for name, more in (("direct", ["--sketch-direct"]), ("counted", [])):
        out = tmp_path / name
        out.mkdir()
        r = run(opts + more + ["--out", out, "--pairs", D, fa])
        assert r.returncode == 0, r.stderr
        assert "5 pairs within %g of 9 records" % D in r.stdout
        assert not (out / "sketch_results.csv").exists() and not (out / "clusters.tsv").exists()
        assert open(out / "pairs.tsv").read().splitlines() == exp
    # without --pairs: what the run wrote before, and no pairs.tsv
    out = tmp_path / "plain"
    out.mkdir()
    r = run(opts + ["--sketch-direct", "--out", out, fa])
    assert r.returncode == 0, r.stderr
    assert (out / "sketch_results.csv").exists() and not (out / "pairs.tsv").exists()
    assert len(open(out / "sketch_results.csv").read().splitlines()) == 36
    assert "pairs within" not in r.stdout
    # --pairs 0: the threshold is Jaccard 1, the copies alone
    out = tmp_path / "zero"
    out.mkdir()
    r = run(opts + ["--sketch-direct", "--out", out, "--pairs", 0, fa])
    assert r.returncode == 0, r.stderr
    assert open(out / "pairs.tsv").read().splitlines() == ["0\t3\t64\t64\t0.000000", "5\t7\t64\t64\t0.000000"]


@pytest.mark.gpu
def test_cli_pairs_per_file(kmc, cuda, tmp_path):
    """--per-file on three files: the third holds the second one's records with about 2 %
    substitutions, the first is unrelated."""
    import torch
    rng = np.random.default_rng(9)
    a = [S.bases(rng, 3000), S.bases(rng, 2000)]
    sets = [[S.bases(rng, 4000)], a, [mutated(rng, r, 0.02) for r in a]]
    files, rows, sizes = [], [], []
    for f, recs in enumerate(sets):
        p = tmp_path / ("file%d.fa" % f)
        write_fasta(p, recs)
        files.append(p)
        data, idx, _ = kmc.load_fasta(str(p), kmc.DIALECT_NONL, 0)
        go = torch.tensor([0, idx.size - 1], dtype=torch.int64, device=cuda)
        r, z = kmc.sketch_from_sequences_grouped(dev(data, cuda), dev(idx, cuda), go, K, SKETCH)
        rows.append(r)
        sizes.append(z)
    rows, sizes = torch.cat(rows), torch.cat(sizes)
    _, sh, dn = kmc.sketch_distances(rows, sizes, K, with_counts=True)
    torch.cuda.synchronize()
    D = pick_distance(u32(sh), u32(dn), K)
    links, dist, count = kmc.sketch_links(rows, sizes, K, kmc.mash_jaccard_of_distance(D, K))
    assert u32(links).reshape(-1, 4)[:, :2].tolist() == [[1, 2]]
    out = tmp_path / "out"
    out.mkdir()
    r = run(["-k", K, "--canonical", "--sketch", SKETCH, "--sketch-direct", "--per-file", "--dialect", "nonl", "--out", out,
             "--pairs", D] + files)
    assert r.returncode == 0, r.stderr
    assert "1 pairs within %g of 3 records" % D in r.stdout
    assert not (out / "sketch_results.csv").exists()
    assert open(out / "pairs.tsv").read().splitlines() == lines_of(links, dist)


@pytest.mark.gpu
def test_cli_query_pairs(kmc, cuda, tmp_path):
    """--query FILE --pairs D: the rectangle's list of FILE's records against the input's."""
    import torch
    rng = np.random.default_rng(8)
    base, records = nine_records(rng)
    queries = [base[2].copy(), S.bases(rng, 2500), mutated(rng, base[0], 0.02), base[3][:2000]]
    fa, qa = tmp_path / "records.fa", tmp_path / "queries.fa"
    write_fasta(fa, records)
    write_fasta(qa, queries)
    (r, rs), n = rows_of(kmc, cuda, fa)
    (q, qs), m = rows_of(kmc, cuda, qa)
    assert (m, n) == (4, 9)
    _, sh, dn = kmc.sketch_distances_rect(q, qs, r, rs, K, with_counts=True)
    torch.cuda.synchronize()
    D = pick_distance(u32(sh).reshape(-1), u32(dn).reshape(-1), K)
    links, dist, count = kmc.sketch_links_rect(q, qs, r, rs, K, kmc.mash_jaccard_of_distance(D, K))
    pairs = u32(links).reshape(-1, 4)[:, :2].tolist()
    # the copy of base 2 finds it and its mutants, the mutant of base 0 both copies of it, the prefix of
    # base 3 both copies of that; the random query nothing
    assert pairs == [[0, 2], [0, 4], [0, 8], [2, 0], [2, 3], [3, 5], [3, 7]] and count.tolist() == [7]
    out = tmp_path / "out"
    out.mkdir()
    opts = ["-k", K, "--canonical", "--sketch", SKETCH, "--sketch-direct", "--dialect", "nonl", "--max-seqs", 0]
    res = run(opts + ["--out", out, "--query", qa, "--pairs", D, fa])
    assert res.returncode == 0, res.stderr
    assert "%d pairs within %g of 4 queries and 9 records" % (len(pairs), D) in res.stdout
    assert open(out / "query_pairs.tsv").read().splitlines() == lines_of(links, dist)
    for name in ("query_results.tsv", "query_distances.csv", "sketch_results.csv", "pairs.tsv"):
        assert not (out / name).exists(), name


def test_help_lists_the_pairs_option():
    r = run(["--help"])
    assert r.returncode == 0
    assert "--pairs" in r.stdout and "pairs.tsv" in r.stdout and "query_pairs.tsv" in r.stdout
    assert "kmc_sketch_links" in r.stdout and "kmc_sketch_links_rect" in r.stdout


def test_pairs_option_combinations(tmp_path):
    """The excluded combinations exit 2, each with its message; the accepted ones fail only
    at the missing device or input (1)."""
    fa, other = tmp_path / "absent.fa", tmp_path / "absent_other.fa"
    counted = ["--canonical", "--sketch", 64, "-k", 21]
    direct = counted + ["--sketch-direct"]
    bad = [
        (["--pairs", 0.05], "--pairs lists the pairs of the sketches"),                            # nothing it needs
        (["--canonical", "--pairs", 0.05], "--pairs lists the pairs of the sketches"),             # no --sketch
        (["--sketch", 64, "--pairs", 0.05], "need --canonical"),                                   # no --canonical
        (direct + ["--pairs", 0.05, "--cluster", 0.05], "--pairs and --cluster exclude each other"),
        (direct + ["--cluster", 0.05, "--pairs", 0.05], "--pairs and --cluster exclude each other"),
        (direct + ["--pairs", 0.05, "--screen", other], "--pairs and --screen exclude each other"),
        (direct + ["--pairs", 0.05, "--query", other, "--top", 5], "not with --top"),
        (direct + ["--query", other, "--top", 0, "--pairs", 0.05], "not with --top"),
        (counted + ["--pairs", 0.05, "--query", other], "--query needs"),                          # --query is direct only
    ] + [(direct + ["--pairs", v], "--pairs takes a Mash distance in 0..1")
         for v in (-0.01, 1.01, "nan", "inf", "0.05x", "", "-1e-300")]
    for args, message in bad:
        r = run(args + [fa])
        assert r.returncode == 2, args
        assert message in r.stderr and "usage:" in r.stderr, (args, r.stderr[:200])
    good = [
        counted + ["--pairs", 0.05],
        counted + ["--pairs", 0.05, "--min-count", 2],
        direct + ["--pairs", 0.05],
        direct + ["--pairs", 0],
        direct + ["--pairs", 1],
        direct + ["--pairs", "1e-3"],
        ["--pairs", 0.5] + direct,
        direct + ["--per-file", "--pairs", 0.05],
        direct + ["--per-file", "--min-abundance", 2, "--pairs", 0.05],
        direct + ["--pairs", 0.05, "--query", other],
        direct + ["--per-file", "--pairs", 0.05, "--query", other],
        direct + ["--pairs", 0.05, "--query", other, "--min-shared", 0],
    ]
    for args in good:
        assert run(args + [fa]).returncode == 1, args
    assert run(direct + ["--per-file", "--pairs", 0.05, fa, other]).returncode == 1
    # an option that lost its value
    assert run(direct + [fa, "--pairs"]).returncode == 2
