"""`kmc --recruit reads.fastq --write-recruited --write-rest`: on the fixture of
test_sketch_match_cli.py (two small FASTA references, 42 reads, --batch 2048 so that
several batches occur) recruited_<f>.fastq must be exactly the raw text of the records
read_matches.tsv lists for file f, in order, and rest_<f>.fastq the others; the two
.tsv files are byte for byte those of the same run without the options."""
import random
import subprocess

import pytest

import fastq_util as Q
import select_util as S
from test_select_args import KMC, write_option_checks
from test_sketch_match_cli import BATCH, K, SLOTS, case

pytestmark = pytest.mark.gpu


def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, timeout=120)


def fastq_records(reads, seed, eol=b"\n", first=0):
    rng = random.Random(seed)
    return [Q.record(r, bytes(rng.choices(b"IF#@+", k=len(r))), b"read/%d extra words" % (first + i), eol,
                     b"+" if i % 3 else b"+read/%d" % (first + i)) for i, r in enumerate(reads)]


def listed_of(out, f):
    """The record numbers read_matches.tsv lists for file f, and `listed` of the summary."""
    rows = [ln.split("\t") for ln in (out / "read_matches.tsv").read_text().splitlines()[1:]]
    summary = [ln.split("\t") for ln in (out / "read_matches_summary.tsv").read_text().splitlines()[1:]]
    return [int(r[1]) for r in rows if int(r[0]) == f], int(summary[f][3])


def recruit(tmp_path, name, fa, files, args):
    out = tmp_path / name
    out.mkdir()
    cmd = ["-k", K, "--canonical", "--dialect", "nonl", "--accum-slots", SLOTS, "--batch", BATCH, "--out", out]
    for f in files:
        cmd += ["--recruit", f]
    r = run(cmd + args + fa)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return out, r.stdout


def references(tmp_path):
    refs, reads = case()
    fa = [tmp_path / "host.fa", tmp_path / "phage.fa"]
    for path, seqs in zip(fa, refs):
        path.write_bytes(Q.as_fasta(seqs))
    return fa, reads


def split_records(text):
    at = S.raw_offsets(text)
    return [text[i:j] for i, j in zip(at[:-1], at[1:])]


def check_outputs(out, f, recs, recruited=True, rest=True):
    rows, listed = listed_of(out, f)
    assert listed == len(rows)
    got = None
    if recruited:
        got = (out / ("recruited_%d.fastq" % f)).read_bytes()
        assert got == b"".join(recs[r] for r in rows)
        assert len(S.raw_offsets(got)) - 1 == listed  # the records written are the records listed
    else:
        assert not (out / ("recruited_%d.fastq" % f)).exists()
    if rest:
        others = (out / ("rest_%d.fastq" % f)).read_bytes()
        assert others == b"".join(x for r, x in enumerate(recs) if r not in set(rows))
        if recruited:  # the two together hold every input record once
            assert len(got) + len(others) == sum(len(x) for x in recs)
            assert sorted(split_records(got) + split_records(others)) == sorted(recs)
    else:
        assert not (out / ("rest_%d.fastq" % f)).exists()
    return rows


def test_recruited_and_rest_are_the_raw_text_of_the_listed_records(cuda, tmp_path):
    fa, reads = references(tmp_path)
    recs = fastq_records(reads, 1)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(recs))
    plain, log0 = recruit(tmp_path, "plain", fa, [fq], [])
    assert not list(plain.glob("*.fastq"))
    for name, args, a, b in (("both", ["--write-recruited", "--write-rest"], True, True),
                             ("recruited", ["--write-recruited"], True, False), ("rest", ["--write-rest"], False, True),
                             ("filtered", ["--min-hits", 3, "--min-fraction", 0.5, "--write-rest", "--write-recruited"], True, True)):
        out, log = recruit(tmp_path, name, fa, [fq], args)
        rows = check_outputs(out, 0, recs, a, b)
        assert 0 < len(rows) < len(reads)
        done = [ln for ln in log.decode().splitlines() if ln.startswith("Recruit 0: ")]
        assert len(done) == 1 and int(done[0].split(" batches")[0].split()[-1]) >= 3, log
        if name != "filtered":  # the .tsv files and stdout are those of the run without the options
            for tsv in ("read_matches.tsv", "read_matches_summary.tsv"):
                assert (out / tsv).read_bytes() == (plain / tsv).read_bytes(), (name, tsv)
            assert log == log0
    assert len(listed_of(tmp_path / "filtered", 0)[0]) < len(listed_of(plain, 0)[0])


@pytest.mark.parametrize("shape", ["crlf", "no last newline", "blank lines"])
def test_line_ends_round_trip(cuda, tmp_path, shape):
    fa, reads = references(tmp_path)
    recs = fastq_records(reads, 2, b"\r\n" if shape == "crlf" else b"\n")
    tail = b""
    if shape == "no last newline":
        recs[-1] = recs[-1][:-1]
    if shape == "blank lines":
        tail = b"\n\n"
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(b"".join(recs) + tail)
    out, _ = recruit(tmp_path, "out", fa, [fq], ["--write-recruited", "--write-rest"])
    rows = check_outputs(out, 0, recs)
    assert 0 < len(rows) < len(reads)
    if shape == "no last newline":  # the last record goes where it belongs, as it is
        last = "recruited_0.fastq" if len(reads) - 1 in rows else "rest_0.fastq"
        assert (out / last).read_bytes().endswith(recs[-1]) and not recs[-1].endswith(b"\n")


def test_two_recruit_files_and_a_file_of_no_record(cuda, tmp_path):
    fa, reads = references(tmp_path)
    first, second = fastq_records(reads[:30], 3), fastq_records(reads[30:], 4, first=30)
    fq = [tmp_path / "a.fq", tmp_path / "b.fq", tmp_path / "nothing.fq", tmp_path / "blank.fq"]
    fq[0].write_bytes(b"".join(first))
    fq[1].write_bytes(b"".join(second))
    fq[2].write_bytes(b"")
    fq[3].write_bytes(b"\n")
    out, _ = recruit(tmp_path, "out", fa, fq, ["--write-recruited", "--write-rest"])
    plain, _ = recruit(tmp_path, "plain", fa, fq, [])
    for tsv in ("read_matches.tsv", "read_matches_summary.tsv"):
        assert (out / tsv).read_bytes() == (plain / tsv).read_bytes(), tsv
    assert check_outputs(out, 0, first) and check_outputs(out, 1, second)
    for f in (2, 3):
        assert check_outputs(out, f, []) == []
        assert (out / ("recruited_%d.fastq" % f)).read_bytes() == b"" == (out / ("rest_%d.fastq" % f)).read_bytes()
    assert sorted(p.name for p in out.glob("*.fastq")) == sorted(
        "%s_%d.fastq" % (w, f) for w in ("recruited", "rest") for f in range(4))


def test_an_output_that_cannot_be_written_ends_the_run(cuda, tmp_path):
    """A failed write names the file: /dev/full takes no byte."""
    fa, reads = references(tmp_path)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(fastq_records(reads, 5)))
    out = tmp_path / "out"
    out.mkdir()
    (out / "recruited_0.fastq").symlink_to("/dev/full")
    r = run(["-k", K, "--canonical", "--dialect", "nonl", "--accum-slots", SLOTS, "--batch", BATCH, "--out", out, "--recruit", fq,
             "--write-recruited"] + fa)
    assert r.returncode == 1 and b"cannot write" in r.stderr and b"recruited_0.fastq" in r.stderr, r.stderr


def test_write_option_combinations(tmp_path):
    write_option_checks(tmp_path)
