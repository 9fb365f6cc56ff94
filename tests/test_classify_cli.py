"""`kmc --canonical --recruit reads.fastq --classify --accum-slots L host.fa phage.fa`: the
two reference files of test_sketch_match_cli.case() are the sources 0 and 1 (the second
holds 300 bases of the first again, so some reads tie), its 42 reads in FASTQ, with CRLF
line ends in some records and no final newline, are classified in several batches.
read_sources.tsv and read_sources_summary.tsv must be, line for line, what
classify_util.model gives; read_matches*.tsv and recruited_0.fastq must be the bytes of a
run without --classify; source_0_<g>.fastq must hold exactly the assigned records' raw
bytes in order."""
import os
import random
import subprocess

import pytest

import classify_util as C
import fastq_util as Q
import sketch_match_util as M
import sketch_screen_util as U
from test_classify_args import classify_option_checks
from test_sketch_match_cli import BATCH, K, SLOTS, case, records_of

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")
HEADER = "file\trecord\twindows\tsampled\thits\tsource\tsource_hits\tnext_hits"
SUMMARY = "file\tsource\tpath\tbest\tassigned"


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, timeout=120)


def test_cli_classify_equals_the_model(oracle, cuda, tmp_path):
    refs, reads = case()
    rng = random.Random(79)
    raw = [Q.record(r, bytes(rng.choices(b"IF#", k=len(r))), b"read/%d" % i, eol=b"\r\n" if i % 5 == 2 else b"\n")
           for i, r in enumerate(reads)]
    raw[-1] = raw[-1][:-1]  # no final newline
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(raw))
    fa = [tmp_path / "host.fa", tmp_path / "phage.fa"]
    for path, seqs in zip(fa, refs):
        path.write_bytes(Q.as_fasta(seqs))
    base = ["-k", K, "--canonical", "--dialect", "nonl", "--accum-slots", SLOTS, "--batch", BATCH, "--recruit", fq,
            "--write-recruited"]

    def recruit(name, args):
        out = tmp_path / name
        out.mkdir()
        r = run(base + ["--out", out] + args + fa)
        assert r.returncode == 0, r.stderr
        assert r.stderr == b"", r.stderr
        return out

    sets = [records_of(f) for f in refs]
    mix = U.mixture_hashes(oracle, *records_of([s for f in refs for s in f]), K)
    lab = C.labels(oracle, list(enumerate(sets)), K, M.FILL, True)
    exp = C.model(oracle, *records_of(reads), K, mix, lab, 2, M.FILL, True)
    plain = recruit("plain", ["--min-hits", 3])
    assert not (plain / "read_sources.tsv").exists()
    for name, args, margin in (("defaults", [], 1), ("margin0", ["--min-margin", 0], 0), ("margin40", ["--min-margin", 40], 40)):
        out = recruit(name, ["--min-hits", 3, "--classify", "--write-sources"] + args)
        rows, lines, assigned = C.tsv_lines(0, fq, exp, [str(p) for p in fa], 3, 0.0, margin)
        assert (out / "read_sources.tsv").read_text().splitlines() == [HEADER] + rows, name
        assert (out / "read_sources_summary.tsv").read_text().splitlines() == [SUMMARY] + lines, name
        for same in ("read_matches.tsv", "read_matches_summary.tsv", "recruited_0.fastq"):
            assert (out / same).read_bytes() == (plain / same).read_bytes(), (name, same)
        for g in (0, 1):
            want = b"".join(raw[r] for r in range(len(reads)) if assigned[r] == g)
            assert (out / ("source_0_%d.fastq" % g)).read_bytes() == want, (name, g)
        if margin == 1:
            got = [assigned.count(g) for g in (0, 1, -1)]
            assert min(got) > 0, got  # both sources and ties (the repeat) occur
            assert any(assigned[r] == -1 and exp[4][r] == exp[5][r] > 0 for r in range(len(reads)))
            assert assigned[len(reads) - 1] is not None and any(assigned[r] is not None for r in range(2, len(reads), 5))
    # without --write-sources no source file; a FASTA --recruit file is classified whole
    again = tmp_path / "again.fa"
    again.write_bytes(Q.as_fasta(reads[:4]))
    out = tmp_path / "fasta"
    out.mkdir()
    r = run(["-k", K, "--canonical", "--dialect", "nonl", "--accum-slots", SLOTS, "--out", out, "--recruit", again,
             "--classify"] + fa)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    first = tuple(v[:4] for v in exp[:6])
    rows, lines, _ = C.tsv_lines(0, again, first, [str(p) for p in fa])
    assert (out / "read_sources.tsv").read_text().splitlines() == [HEADER] + rows
    assert (out / "read_sources_summary.tsv").read_text().splitlines() == [SUMMARY] + lines
    assert not list(out.glob("source_*"))


def test_cli_classify_option_combinations(tmp_path):
    classify_option_checks(tmp_path)


def test_cli_classify_refuses_33_inputs_and_a_fifo(tmp_path):
    fq = tmp_path / "reads.fq"
    fq.write_bytes(Q.record(b"ACGT" * 10, b"I" * 40))
    files = []
    for i in range(33):
        files.append(tmp_path / ("in%d.fa" % i))
        files[-1].write_bytes(b">s\nACGTACGTACGTACGTACGTACGTAA\n")
    base = ["-k", K, "--canonical", "--accum-slots", SLOTS, "--out", tmp_path, "--recruit", fq, "--classify"]
    r = run(base + files)
    assert r.returncode == 2 and b"32 sources apart at most" in r.stderr, r.stderr
    fifo = tmp_path / "pipe.fa"
    os.mkfifo(fifo)
    r = run(base + files[:2] + [fifo])  # nobody writes to the FIFO: a driver that opened it would block
    assert r.returncode == 2 and b"is not a regular file" in r.stderr, r.stderr
    assert not (tmp_path / "read_matches.tsv").exists()
    assert run(base + files[:32]).returncode == 0
