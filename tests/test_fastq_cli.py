"""`kmc --format auto|fasta|fastq` and `--screen-batch`: FASTQ inputs of the main file,
--query, --per-file and --screen, the last one streamed batch by batch.  The option
combinations are judged before any device or file is touched; on the GPU the FASTQ
runs must write byte for byte what the same reads give as FASTA."""
import os
import random
import subprocess

import pytest

import fastq_util as Q
import golden_util as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")
RANDOM_FA = os.path.join(G.GOLDEN, "random.fa")


def run(args, stdin=None):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, timeout=120, input=stdin)


def test_format_option_combinations(tmp_path):
    out = run(["--help"]).stdout.decode()
    assert "--format" in out and "--screen-batch" in out and "fastq" in out
    fq, fa, reads = tmp_path / "absent.fq", tmp_path / "absent.fa", tmp_path / "absent_reads.FASTQ"
    sk = ["--canonical", "--sketch", 64, "--sketch-direct", "-k", 21]
    bad = [
        ["--host-loader", fq], ["--gpus", 2, fq], ["--dropin", fq],
        ["--format", "fastq", "--host-loader", fa], ["--format", "fastq", "--gpus", 2, fa],
        ["--format", "fastq", "--dropin", fa], ["--host-loader", tmp_path / "absent.FQ"],
        sk + ["--host-loader", "--screen", reads, fa], sk + ["--host-loader", "--query", fq, fa],
    ]
    for args in bad:
        r = run(args)
        assert r.returncode == 2, args
        assert b"FASTQ" in r.stderr, (args, r.stderr[:200])
    r = run(["--format", "fastx", fa])
    assert r.returncode == 2 and b"unknown format" in r.stderr
    assert run([fa, "--format"]).returncode == 2 and run(sk + ["--screen", reads, "--screen-batch", fa]).returncode == 2
    r = run(["--screen-batch", 1024, fa])
    assert r.returncode == 2 and b"--screen-batch" in r.stderr
    assert run(sk + ["--screen", reads, "--screen-batch", -1, fa]).returncode == 2
    # accepted: what fails is the missing device or input (1), not the options
    for args in ([fq], ["--format", "fastq", fa], ["--format", "fasta", "--host-loader", fq],
                 sk + ["--screen", reads, "--screen-batch", 1024, fa], sk + ["--per-file", fq, fq],
                 sk + ["--query", fq, fa], sk + ["--format", "fastq", "--screen", "/dev/stdin", fa]):
        assert run(args).returncode == 1, args
    # .fa names still exit as before: 1 for the missing device or input, 2 for the old refusals
    for args in ([fa], ["--host-loader", fa], ["--gpus", 2, fa], ["--dropin", fa], sk + ["--screen", fa, fa]):
        assert run(args).returncode == 1, args
    assert run(["--gpus", 2, "--dropin", fa]).returncode == 2
    r = run(sk + ["--screen", fa, fa, tmp_path / "absent_more.fa"])
    assert r.returncode == 2 and b"more than one input file" in r.stderr


def sequences(path):
    seqs = []
    for line in open(path):
        if line.startswith(">"):
            seqs.append("")
        elif seqs:
            seqs[-1] += line.strip()
    return [s.encode() for s in seqs]


def write_fasta(path, seqs):
    path.write_bytes(b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    return path


def write_fastq(path, seqs, rng):
    """The reads as FASTQ, with the quality traps of fastq_util."""
    out = bytearray()
    for i, s in enumerate(seqs):
        q = bytes(rng.choices(b"@+IF#", k=len(s)))
        out += Q.record(s, q, b"read/%d" % i, plus=b"+read/%d" % i if i % 4 == 0 else b"+")
    path.write_bytes(bytes(out))
    return path


def draw_reads(rng, genomes, n, lo=30, hi=150):
    reads = []
    for _ in range(n):
        g = rng.choice(genomes)
        ln = rng.randint(lo, hi)
        a = rng.randrange(0, len(g) - ln)
        reads.append(g[a:a + ln])
    return reads


@pytest.mark.gpu
def test_cli_fastq_screen_equals_fasta(cuda, tmp_path):
    k, s = 21, 64
    g = sequences(RANDOM_FA)
    assert len(g) == 3 and min(len(x) for x in g) >= 6000
    rng = random.Random(2024)
    refs = write_fasta(tmp_path / "refs.fa", [g[0][:2000], g[1][:3000], g[1][3000:6000], g[2][3000:5000], g[2][:15]])
    reads = draw_reads(rng, [g[0], g[1][:3500]], 400)   # nothing of g[1][3500:] or g[2]
    more = draw_reads(rng, [g[1][2000:5000]], 150)
    fa, fa2 = write_fasta(tmp_path / "reads.fa", reads), write_fasta(tmp_path / "more.fa", more)
    fq, fq2 = write_fastq(tmp_path / "reads.fastq", reads, rng), write_fastq(tmp_path / "more.FQ", more, rng)
    base = ["-k", k, "--canonical", "--sketch", s, "--sketch-direct", "--dialect", "nonl", "--max-seqs", 0]

    def screen(name, args, stdin=None, refs=refs):
        out = tmp_path / name
        out.mkdir()
        r = run(base + ["--out", out] + args + [refs], stdin)
        assert r.returncode == 0, r.stderr
        return (out / "screen_results.tsv").read_bytes(), r.stdout.decode()

    exp, _ = screen("fa", ["--screen", fa, "--screen", fa2])
    lines = [ln.split("\t") for ln in exp.decode().splitlines()]
    assert len(lines) == 5 and int(lines[0][1]) > 0 and int(lines[3][1]) == 0 and lines[4][4] == "nan"
    got, log = screen("fq_1024", ["--screen-batch", 1024, "--screen", fq, "--screen", fq2])
    assert got == exp
    nbatch = [int(ln.split(" batches")[0].split()[-1]) for ln in log.splitlines() if ln.startswith("Screen: ")]
    assert len(nbatch) == 2 and nbatch[0] >= os.path.getsize(fq) // 1100 and nbatch[1] >= 10
    assert "Screen: %s: 400 records, %d bytes, " % (fq, sum(len(r) + 1 for r in reads)) in log
    got, log = screen("fq_default", ["--screen", fq, "--screen", fq2])
    assert got == exp and "400 records" in log and " 1 batches" in log
    # mixed: one FASTQ and one FASTA mixture
    got, _ = screen("mixed", ["--screen", fq, "--screen", fa2])
    assert got == exp
    # on stdin, forced (for every file of the command: the references are FASTQ here too)
    both = fq.read_bytes() + fq2.read_bytes()
    refs_fq = write_fastq(tmp_path / "refs_as_reads.txt", sequences(refs), rng)
    got, log = screen("stdin", ["--format", "fastq", "--screen-batch", 4096, "--screen", "/dev/stdin"], stdin=both,
                      refs=refs_fq)
    assert got == exp and "550 records" in log
    # a malformed mixture: exit 1 with the record's index within the whole file
    bad = tmp_path / "bad.fq"
    lines = fq.read_bytes().split(b"\n")
    lines[4 * 321 + 2] = b"-"
    bad.write_bytes(b"\n".join(lines))
    for batch in (1024, 0):
        r = run(base + ["--out", tmp_path, "--screen-batch", batch, "--screen", bad, refs])
        assert r.returncode == 1 and ("kmc: %s: malformed FASTQ at record 321\n" % bad).encode() in r.stderr, r.stderr


@pytest.mark.gpu
def test_cli_fastq_inputs_equal_fasta(cuda, tmp_path):
    k, s = 21, 64
    g = sequences(RANDOM_FA)
    rng = random.Random(7)
    samples = [draw_reads(rng, [g[0], g[1]], 300, 60, 200), draw_reads(rng, [g[1], g[2]], 300, 60, 200)]
    fas = [write_fasta(tmp_path / ("s%d.fa" % i), r) for i, r in enumerate(samples)]
    fqs = [write_fastq(tmp_path / ("s%d.fq" % i), r, rng) for i, r in enumerate(samples)]
    base = ["-k", k, "--canonical", "--sketch", s, "--sketch-direct", "--dialect", "nonl"]

    def sketch(name, args, result="sketch_results.csv"):
        out = tmp_path / name
        out.mkdir()
        r = run(base + ["--out", out] + args)
        assert r.returncode == 0, r.stderr
        return (out / result).read_bytes(), r.stdout.decode()

    # --per-file: two samples, each sketched as one genome
    exp, _ = sketch("pf_fa", ["--per-file"] + fas)
    got, log = sketch("pf_fq", ["--per-file"] + fqs)
    assert got == exp and len(exp.splitlines()) == 1 and "%s: 300 records" % fqs[0] in log
    # the main input, with --max-seqs as a plain truncation
    exp, _ = sketch("main_fa", ["--max-seqs", 0, write_fasta(tmp_path / "first20.fa", samples[0][:20])])
    got, log = sketch("main_fq", ["--max-seqs", 20, fqs[0]])
    assert got == exp and len(exp.splitlines()) == 190 and "20 sequences read" in log
    # --query in FASTQ against FASTA references
    refs = write_fasta(tmp_path / "refs.fa", [g[0], g[1], g[2]])
    exp, _ = sketch("q_fa", ["--max-seqs", 0, "--query", fas[1], refs], "query_results.tsv")
    got, _ = sketch("q_fq", ["--max-seqs", 0, "--query", fqs[1], refs], "query_results.tsv")
    assert got == exp and exp
    # a malformed main input
    bad = tmp_path / "bad.fq"
    bad.write_bytes(fqs[0].read_bytes()[:-40])
    r = run(base + ["--out", tmp_path, bad])
    assert r.returncode == 1 and ("kmc: %s: malformed FASTQ at record 299\n" % bad).encode() in r.stderr, r.stderr
