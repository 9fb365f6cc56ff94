"""`kmc --per-file --min-abundance M [--accum-slots LOG2] [--batch BYTES]`: every file of a
--per-file set is one pass of the abundance accumulator, a FASTQ file streamed batch
by batch.  The option combinations are judged before any device or file is touched;
on the GPU sketch_results.csv must hold the distances of the rows kmc.SketchAccum
makes from the same records."""
import os
import random
import subprocess

import numpy as np
import pytest

import fastq_util as Q
from sketch_util import pack

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")
SK = ["--canonical", "--sketch", 64, "--sketch-direct", "-k", 21]


def run(args, stdin=None):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, timeout=120, input=stdin)


def test_min_abundance_option_combinations(tmp_path):
    out = run(["--help"]).stdout.decode()
    assert "--min-abundance" in out and "--accum-slots" in out and "--batch" in out
    fq, fa = tmp_path / "absent.fq", tmp_path / "absent.fa"
    pf = SK + ["--per-file"]
    bad = [
        ["--min-abundance", 2, fa],                                     # nothing it needs
        ["--canonical", "--min-abundance", 2, fa],
        ["--canonical", "--sketch", 64, "--min-abundance", 2, fa],      # no --sketch-direct
        SK + ["--min-abundance", 2, fa],                                # no --per-file
        SK + ["--min-abundance", 2, "--query", fq, fa],
        SK + ["--min-abundance", 2, "--screen", fq, fa],
        ["--canonical", "--sketch", 64, "--per-file", "--min-abundance", 2, fa],
        pf + ["--min-abundance", 0, fa], pf + ["--min-abundance", -1, fa], pf + ["--min-abundance", 1 << 32, fa],
        pf + ["--min-abundance", 2, "--max-seqs", 5, fa],
        pf + ["--accum-slots", 20, fa], pf + ["--batch", 4096, fa],     # they shape --min-abundance's pass
        SK + ["--screen", fq, "--batch", 4096, fa],
        pf + ["--min-abundance", 2, "--accum-slots", 3, fa], pf + ["--min-abundance", 2, "--accum-slots", 31, fa],
        pf + ["--min-abundance", 2, "--batch", -1, fa], pf + ["--min-abundance", 2, "--batch", 1 << 32, fa],
    ]
    for args in bad:
        r = run(args)
        assert r.returncode == 2, (args, r.stderr[:200])
        assert b"usage:" in r.stderr, (args, r.stderr[:200])
    assert run(pf + [fa, "--min-abundance"]).returncode == 2
    # the existing refusal stays: --min-count above 1 never goes with --sketch-direct
    r = run(pf + ["--min-count", 2, fa])
    assert r.returncode == 2 and b"--sketch-direct never counts" in r.stderr
    assert run(pf + ["--min-count", 2, "--min-abundance", 2, fa]).returncode == 2
    # accepted: what fails is the missing device or input (1), not the options
    for args in (pf + ["--min-abundance", 2, fq], pf + ["--min-abundance", 1, fa, fq],
                 pf + ["--min-abundance", 2, "--accum-slots", 4, "--batch", 4096, fq],
                 pf + ["--min-abundance", 2, "--accum-slots", 0, "--batch", 0, "--max-seqs", 0, fa],
                 pf + ["--min-abundance", 2, "--format", "fastq", "/dev/stdin"],
                 pf + ["--min-abundance", 3, "--query", fq, fa], pf + ["--min-abundance", 2, "--screen", fq, fa],
                 pf + ["--min-abundance", 2, "--screen", fq, "--screen-batch", 1024, "--batch", 2048, fa]):
        assert run(args).returncode == 1, args


def fastq_of(seqs, rng):
    """The reads as plain FASTQ (fastq_util.record), for the stdin run's third file."""
    return b"".join(Q.record(s, bytes(rng.choices(b"IF#", k=len(s))), b"read/%d" % i) for i, s in enumerate(seqs))


@pytest.mark.gpu
def test_cli_min_abundance_equals_sketch_accum(kmc, cuda, tmp_path):
    import torch
    k, s, m = 21, 64, 2
    rng = random.Random(99)

    def write(n, **kw):  # fastq_util.write_fastq: quality traps, '+name' lines, N bytes
        return Q.write_fastq(rng, n, lo=30, hi=150, lower=0.0, n_rate=0.01, **kw)
    (w1, s1), (w2, s2) = write(120, crlf=True), write(60, crlf=True, final_newline=False)
    (w3, s3), (w4, s4) = write(120), write(60)
    # a.fastq: CRLF, no final newline; its first 120 reads twice, 60 once.  b.fq: the same shape of
    # other reads.  c.fa: half of either file's repeated reads, twice: related to both
    samples = [s1 + s1 + s2, s3 + s3 + s4, s1[:60] + s3[:60] + s1[:60] + s3[:60]]
    raws = [w1 + w1 + w2, w3 + w3 + w4]
    assert raws[0].count(b"\r\n") == 4 * 300 - 1 and not raws[0].endswith(b"\n") and b"\r" not in raws[1]
    assert Q.parse(raws[0])[1][-1] == sum(len(r) + 1 for r in samples[0])
    files = [tmp_path / "a.fastq", tmp_path / "b.fq", tmp_path / "c.fa"]
    files[0].write_bytes(raws[0])
    files[1].write_bytes(raws[1])
    files[2].write_bytes(Q.as_fasta(samples[2]))

    # the rows kmc.SketchAccum makes of the same records, and their distances
    rows = torch.empty((3, s), dtype=torch.int64, device=cuda)
    sizes = torch.empty(3, dtype=torch.int32, device=cuda)
    with kmc.SketchAccum(s, k) as acc:
        for f, reads in enumerate(samples):
            acc.reset()
            data, idx = pack([np.frombuffer(r, np.uint8) for r in reads])
            acc.add(torch.from_numpy(data.copy()).to(cuda), torch.from_numpy(idx).to(cuda))
            _, _, st = acc.finish(m, out=(rows[f], sizes[f:f + 1]))
            assert int(st[0]) == 1
    dist = kmc.sketch_distances(rows, sizes, k)
    torch.cuda.synchronize()
    exp = "".join("%f\n" % v for v in dist.cpu().numpy()).encode()
    d = dist.cpu().numpy()  # pairs (a, b), (a, c), (b, c)
    assert int(sizes.min()) == s and d[0] == 1.0 and 0.0 < d[1] < 1.0 and 0.0 < d[2] < 1.0

    base = ["-k", k, "--canonical", "--sketch", s, "--sketch-direct", "--dialect", "nonl", "--per-file"]

    def sketch(name, args, stdin=None):
        out = tmp_path / name
        out.mkdir()
        r = run(base + ["--out", out] + args, stdin)
        assert r.returncode == 0, r.stderr
        return (out / "sketch_results.csv").read_bytes(), r.stdout.decode()

    got, log = sketch("files", ["--min-abundance", m, "--batch", 4096] + files)
    assert got == exp and len(exp.splitlines()) == 3
    lines = [ln for ln in log.splitlines() if ln.startswith("File ")]
    assert len(lines) == 3 and all("300 records" in ln for ln in lines[:2]) and "240 records, 1 batches" in lines[2]
    assert all("sketch size %d, j 0, complete 1" % s in ln for ln in lines)
    nbatch = [int(ln.split(" batches")[0].split()[-1]) for ln in lines]
    assert nbatch[0] >= len(raws[0]) // 4200 and nbatch[0] > 10 and nbatch[1] > 10
    # without the filter the k-mers of the reads that occur once are sketched too
    plain, _ = sketch("plain", files)
    assert plain != exp
    # the first file on stdin (every file of the command is FASTQ then: the FASTA sample as reads)
    third = tmp_path / "c_as_reads.txt"
    third.write_bytes(fastq_of(samples[2], rng))
    got, log = sketch("stdin", ["--min-abundance", m, "--batch", 4096, "--format", "fastq", "/dev/stdin", files[1],
                                third], stdin=raws[0])
    assert got == exp and "File 0: /dev/stdin: 300 records" in log
    # a table too small for the file: exit 1, naming the option
    r = run(base + ["--out", tmp_path, "--min-abundance", m, "--accum-slots", 4, files[0]])
    assert r.returncode == 1 and b"--accum-slots" in r.stderr, r.stderr
    # as the reference set of a query: the rows are the same, so a sample finds itself
    qout = tmp_path / "query"
    qout.mkdir()
    r = run(base + ["--out", qout, "--min-abundance", m, "--query", files[1]] + files)
    assert r.returncode == 0, r.stderr
    first = (qout / "query_results.tsv").read_text().splitlines()[0].split("\t")
    assert first[:3] == ["0", "1", "1"] and first[3] == first[4] == str(s)  # query 0, rank 1: reference 1, itself
