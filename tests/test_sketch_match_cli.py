"""`kmc --canonical --recruit reads.fastq --accum-slots L host.fa phage.fa`: two small
reference FASTA files are the k-mer set, 42 reads in FASTQ (pieces of either reference
from either strand, some with substitutions, some unrelated) are matched against it in
several batches.  read_matches.tsv and read_matches_summary.tsv must be, line for line,
what sketch_match_util.model gives for the same records: the oracle's keys and counts
looked up in the oracle's multiset of the two references.  The table holds everything
(2^16 slots for 5 kbase), so the limit is unbounded and nothing is sampled.  Then: files
of no record, a table of 16 slots that refuses k-mers (the summary's limit is a refused
hash, the model is taken at it, and stderr names --accum-slots), and the refused option
combinations."""
import os
import random
import subprocess

import numpy as np
import pytest

import fastq_util as Q
import sketch_match_util as M
import sketch_screen_util as U
from sketch_util import bases, pack
from test_sketch_match_args import recruit_option_checks

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")
K, SLOTS, BATCH = 21, 16, 2048
HEADER = "file\trecord\twindows\tsampled\thits"
SUMMARY = "file\tpath\trecords\tlisted\tlimit\texact\tsampled\thits"


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, timeout=120)


def case():
    """(references: two lists of sequences, the second file holding a repeat of the first's;
    reads)."""
    rng = random.Random(77)
    host = [bytes(rng.choices(b"ACGT", k=n)) for n in (1800, 900)]
    phage = [bytes(rng.choices(b"ACGT", k=1500)) + host[0][200:500]]  # 300 bases of the host again: count 2
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    reads = []
    for i in range(42):
        n = rng.randint(30, 150)
        if i % 4 == 3:
            reads.append(bytes(rng.choices(b"ACGT", k=n)))
            continue
        src = rng.choice(host + phage)
        at = rng.randrange(len(src) - n + 1)
        r = bytearray(src[at:at + n])
        if rng.random() < 0.5:
            r = bytearray(bytes(r).translate(comp)[::-1])
        if i % 4 == 2:
            for p in rng.sample(range(n), 2):
                r[p] = rng.choice([b for b in b"ACGT" if b != r[p]])
        reads.append(bytes(r))
    reads[5] = b"ACGTN" * 8   # no valid window
    reads[9] = b"ACGT"        # shorter than k
    return [host, phage], reads


def records_of(seqs):
    return pack([np.frombuffer(s, np.uint8) for s in seqs])


def expected(oracle, refs, reads, m):
    mix = U.mixture_hashes(oracle, *records_of([s for f in refs for s in f]), K)
    return M.model(oracle, *records_of(reads), K, mix, M.FILL, True, m)


def test_cli_recruit_equals_the_model(oracle, cuda, tmp_path):
    refs, reads = case()
    rng = random.Random(78)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(Q.record(r, bytes(rng.choices(b"IF#", k=len(r))), b"read/%d" % i)
                            for i, r in enumerate(reads)))
    fa = [tmp_path / "host.fa", tmp_path / "phage.fa"]
    for path, seqs in zip(fa, refs):
        path.write_bytes(Q.as_fasta(seqs))
    again = tmp_path / "again.fa"  # a FASTA --recruit file: matched whole
    again.write_bytes(Q.as_fasta(reads[:4]))
    base = ["-k", K, "--canonical", "--dialect", "nonl", "--accum-slots", SLOTS, "--batch", BATCH, "--recruit", fq,
            "--recruit", again]

    def recruit(name, args):
        out = tmp_path / name
        out.mkdir()
        r = run(base + ["--out", out] + args + fa)
        assert r.returncode == 0, r.stderr
        assert r.stderr == b"", r.stderr  # nothing was lost
        return ((out / "read_matches.tsv").read_text().splitlines(),
                (out / "read_matches_summary.tsv").read_text().splitlines(), r.stdout.decode())

    for name, args, m, h, f in (("defaults", [], 1, 1, 0.0), ("filtered", ["--min-hits", 3, "--min-fraction", 0.5], 1, 3, 0.5),
                                ("twice", ["--min-abundance", 2], 2, 1, 0.0)):
        exp = expected(oracle, refs, reads, m)
        first = tuple(v[:4] for v in exp[:3]) + ([1, M.FILL, int(exp[1][:4].sum()), int(exp[2][:4].sum())],)
        rows0, line0 = M.tsv_lines(0, fq, exp, h, f)
        rows1, line1 = M.tsv_lines(1, again, first, h, f)
        lines, summary, log = recruit(name, args)
        assert lines == [HEADER] + rows0 + rows1, name
        assert summary == [SUMMARY, line0, line1], name
        assert 0 < len(rows0) < len(reads), name
        done = [ln for ln in log.splitlines() if ln.startswith("Recruit 0: ")]
        assert len(done) == 1 and int(done[0].split(" batches")[0].split()[-1]) >= 3, log
    exp1, exp2 = expected(oracle, refs, reads, 1), expected(oracle, refs, reads, 2)
    assert (exp1[2] == exp1[0]).any() and ((exp1[2] > 0) & (exp1[2] < exp1[0])).any() and (exp1[0] == 0).any()
    assert 0 < exp2[3][3] < exp1[3][3]  # only the repeat has count 2


def test_cli_recruit_files_of_no_record(oracle, cuda, tmp_path):
    """A FASTQ file of no byte (no batch) and a FASTA file of no record (one batch of no
    record) get their summary lines, with the set's limit and exact."""
    refs, reads = case()
    fa = tmp_path / "host.fa"
    fa.write_bytes(Q.as_fasta(refs[0]))
    nothing, header_only, some = tmp_path / "nothing.fq", tmp_path / "none.fa", tmp_path / "some.fa"
    nothing.write_bytes(b"")
    header_only.write_bytes(b">none\n")
    some.write_bytes(Q.as_fasta(reads[:3]))
    r = run(["-k", K, "--canonical", "--dialect", "nonl", "--accum-slots", SLOTS, "--out", tmp_path, "--recruit", nothing,
             "--recruit", header_only, "--recruit", some, fa])
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    mix = U.mixture_hashes(oracle, *records_of(refs[0]), K)
    exp = M.model(oracle, *records_of(reads[:3]), K, mix, M.FILL, True)
    rows, line = M.tsv_lines(2, some, exp)
    assert (tmp_path / "read_matches.tsv").read_text().splitlines() == [HEADER] + rows
    assert (tmp_path / "read_matches_summary.tsv").read_text().splitlines() == [
        SUMMARY, "0\t%s\t0\t0\t%d\t1\t0\t0" % (nothing, M.FILL), "1\t%s\t0\t0\t%d\t1\t0\t0" % (header_only, M.FILL), line]


LOST_LG, LOST_J = 4, 10  # 16 slots; 4096 bytes: ceil(4096 / 2^10) = 4 = C / 4


def lost_records(oracle):
    """The first 8 records of 511 bases (4096 bytes: level 10 with 16 slots, about 4 hashes
    below its bound are expected) of which more than C / 2 = 8 distinct hashes lie below
    the bound, so that inserts are refused.  Found on the CPU."""
    for seed in range(4000):
        rng = np.random.default_rng(9000 + seed)
        recs = [bases(rng, 511) for _ in range(8)]
        h, _ = U.mixture_hashes(oracle, *pack(recs), K)
        if int((h < np.uint64(1 << (64 - LOST_J))).sum()) > (1 << LOST_LG) // 2:
            return recs
    raise AssertionError("no input among 4000 loses an insert: change the case")


def test_cli_recruit_from_a_table_that_lost_inserts(oracle, cuda, tmp_path):
    recs = lost_records(oracle)
    data, idx = pack(recs)
    assert data.size == 4096
    fa = tmp_path / "set.fa"
    fa.write_bytes(Q.as_fasta([r.tobytes() for r in recs]))
    r = run(["-k", K, "--canonical", "--dialect", "nonl", "--accum-slots", LOST_LG, "--out", tmp_path, "--recruit", fa, fa])
    assert r.returncode == 0, r.stderr
    assert r.stderr.count(b"\n") == 1 and b"--accum-slots" in r.stderr, r.stderr  # one line names the option
    summary = (tmp_path / "read_matches_summary.tsv").read_text().splitlines()
    limit, exact = int(summary[1].split("\t")[4]), int(summary[1].split("\t")[5])
    assert exact == 0 and 0 < limit < 1 << (64 - LOST_J)  # a refused hash, below the level's bound
    exp = M.model(oracle, data, idx, K, U.mixture_hashes(oracle, data, idx, K), limit, False)
    rows, line = M.tsv_lines(0, fa, exp)
    assert summary == [SUMMARY, line]
    assert (tmp_path / "read_matches.tsv").read_text().splitlines() == [HEADER] + rows
    assert exp[3][2] == exp[3][3] > 0 and (exp[1] < exp[0]).all()  # every sampled window is of a tracked key


def test_cli_recruit_option_combinations(tmp_path):
    recruit_option_checks(tmp_path)
