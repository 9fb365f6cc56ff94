#!/usr/bin/env python3
"""fastqbench.py — the device FASTQ parser and the streamed screen, measured
(profiles/pr_fastq.jsonl, one JSON line per measurement).

  parse   kmc_fastq_parse_device on --mbytes MB of synthetic 150-base reads already
          in device memory, beside kmc_fasta_parse_device on the same reads as
          one-line-per-read FASTA: raw bytes per second of each (HIP events around
          the call, warm-up, median of --runs; both calls synchronise inside, so the
          window holds their read-backs too).
  screen  `kmc --screen` end to end: the reads as a FASTQ file, streamed at the default
          batch, beside the same reads as a FASTA file read whole: wall time of the
          process and the peak of the device memory in use, sampled with
          torch.cuda.mem_get_info from this process while the child runs.

  --select  (instead of the two above; profiles/pr_select_records.jsonl)
          kmc_select_records on the same raw FASTQ bytes with a random half of the
          records kept, beside kmc_fastq_parse_device on the same buffer in the same
          process (the selection reads the raw bytes once and writes half of them, the
          parser passes over them three times); the count-only call and the call that
          drops every record, which are the per-record passes alone; and `kmc --recruit
          ... --write-recruited` end to end on the reads as a file, beside the same run
          without the option (process wall time, page cache warm).

The reads are drawn on the device from a fixed seed; the files are written once into
--tmp."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "dna-kmeres-parallel_amd"))

import torch  # noqa: E402

import kmc  # noqa: E402

KMC = os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")
READ = 150


def make_texts(nreads, dev):
    """(fastq, fasta) uint8 device tensors of nreads 150-base reads: '@r<9 digits>', the
    bases, '+', a quality line; '>r<9 digits>' and the bases."""
    g = torch.Generator(device=dev)
    g.manual_seed(150)
    lut = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
    bases = lut[torch.randint(0, 4, (nreads, READ), generator=g, device=dev)]
    qual = torch.randint(33, 74, (nreads, READ), generator=g, device=dev, dtype=torch.uint8)
    num = torch.arange(nreads, device=dev)
    digits = torch.stack([(num // 10 ** p) % 10 + 48 for p in range(8, -1, -1)], dim=1).to(torch.uint8)
    nl = torch.full((nreads, 1), 10, dtype=torch.uint8, device=dev)

    def col(text):
        return torch.tensor(list(text), dtype=torch.uint8, device=dev).repeat(nreads, 1)

    fastq = torch.cat([col(b"@r"), digits, nl, bases, nl, col(b"+\n"), qual, nl], dim=1).reshape(-1)
    fasta = torch.cat([col(b">r"), digits, nl, bases, nl], dim=1).reshape(-1)
    return fastq, fasta


def timed(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "runs": runs}


def parse_bench(fastq, fasta, nreads, runs):
    import ctypes
    dev = fastq.device
    L = kmc.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    idx = torch.empty(nreads + 1, dtype=torch.int64, device=dev)
    out = []
    for name, raw in (("fastq", fastq), ("fasta", fasta)):
        n = raw.numel()
        cap = n // 2 + 1 if name == "fastq" else n + 16
        data = torch.empty(cap + 16, dtype=torch.uint8, device=dev)
        ns, nb, used = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

        def call():
            if name == "fastq":
                rc = L.kmc_fastq_parse_device(raw.data_ptr(), n, 1, data.data_ptr(), cap, idx.data_ptr(), nreads + 1,
                                              ctypes.byref(ns), ctypes.byref(nb), ctypes.byref(used), st)
            else:
                rc = L.kmc_fasta_parse_device(raw.data_ptr(), n, kmc.DIALECT_NONL, data.data_ptr(), cap, idx.data_ptr(),
                                              nreads + 1, ctypes.byref(ns), ctypes.byref(nb), st)
            assert rc == 0 and ns.value == nreads and nb.value == nreads * (READ + 1), (name, rc, ns.value, nb.value)

        t = timed(call, runs)
        t.update(bench="parse", format=name, raw_bytes=n, reads=nreads,
                 raw_gb_per_s=n / (t["ms_median"] * 1e-3) / 1e9)
        out.append(t)
        del data
    return out


def select_bench(fastq, nreads, runs):
    import ctypes
    dev = fastq.device
    L = kmc.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = fastq.numel()
    rec = 2 * READ + 16
    ridx = torch.arange(nreads + 1, dtype=torch.int64, device=dev) * rec
    g = torch.Generator(device=dev)
    g.manual_seed(151)
    half = (torch.rand(nreads, generator=g, device=dev) < 0.5).to(torch.int32)
    none = torch.zeros(nreads, dtype=torch.int32, device=dev)
    dst = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.empty(kmc.select_records_workspace_size(nreads, n), dtype=torch.uint8, device=dev)
    kept = int(half.sum().item())
    out = []
    for name, keep, cap, expect in (("half kept", half, n, kept), ("count only", half, 0, kept), ("all dropped", none, n, 0)):
        def call():
            rc = L.kmc_select_records(fastq.data_ptr(), ridx.data_ptr(), nreads, n, keep.data_ptr(), 0,
                                      dst.data_ptr() if cap else None, cap, None, counts.data_ptr(), ws.data_ptr(),
                                      ws.numel(), st)
            assert rc == 0, rc

        t = timed(call, runs)
        assert counts.tolist() == [expect, expect * rec], (name, counts.tolist())
        t.update(bench="select", case=name, raw_bytes=n, reads=nreads, kept_bytes=expect * rec,
                 raw_gb_per_s=n / (t["ms_median"] * 1e-3) / 1e9)
        out.append(t)
    # the half that was kept is the text of those records
    some = torch.nonzero(half)[:3, 0].tolist()
    for i, r in enumerate(some):
        assert torch.equal(dst[i * rec:(i + 1) * rec], fastq[r * rec:(r + 1) * rec])
    idx = torch.empty(nreads + 1, dtype=torch.int64, device=dev)
    data = torch.empty(n // 2 + 17, dtype=torch.uint8, device=dev)
    ns, nb, used = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

    def parse():
        rc = L.kmc_fastq_parse_device(fastq.data_ptr(), n, 1, data.data_ptr(), n // 2 + 1, idx.data_ptr(), nreads + 1,
                                      ctypes.byref(ns), ctypes.byref(nb), ctypes.byref(used), st)
        assert rc == 0 and ns.value == nreads, (rc, ns.value)

    t = timed(parse, runs)
    t.update(bench="select", case="parse of the same buffer", raw_bytes=n, reads=nreads,
             raw_gb_per_s=n / (t["ms_median"] * 1e-3) / 1e9)
    out.append(t)
    out.append({"bench": "select", "case": "ratio", "select_over_parse": out[0]["ms_median"] / t["ms_median"]})
    return out


def recruit_bench(fastq, fasta, nreads, runs, tmp):
    """`kmc --recruit reads.fastq` with and without --write-recruited: the first 1000 reads are
    the k-mer set, so 1000 of the reads and whatever shares a 21-mer with them are written."""
    os.makedirs(tmp, exist_ok=True)
    reads = os.path.join(tmp, "reads.fastq")
    fastq.cpu().numpy().tofile(reads)
    refs = os.path.join(tmp, "refs.fa")
    with open(refs, "wb") as f:
        f.write(fasta[:1000 * (READ + 13)].cpu().numpy().tobytes())
    base = [KMC, "-q", "-k", "21", "--canonical", "--dialect", "nonl", "--accum-slots", "20", "--recruit", reads]
    out, tsv = [], {}
    for name, extra in (("plain", []), ("write-recruited", ["--write-recruited"])):
        d = os.path.join(tmp, "recruit_" + name)
        os.makedirs(d, exist_ok=True)
        walls = []
        for i in range(runs + 1):  # the first run warms the page cache
            wall, _, _ = run_sampled(base + extra + ["--out", d, refs])
            if i:
                walls.append(wall)
        tsv[name] = open(os.path.join(d, "read_matches.tsv"), "rb").read()
        row = {"bench": "recruit", "case": name, "file_bytes": os.path.getsize(reads), "reads": nreads,
               "wall_s_median": statistics.median(walls), "wall_s_min": min(walls), "wall_s_max": max(walls), "runs": runs}
        if extra:
            row["written_bytes"] = os.path.getsize(os.path.join(d, "recruited_0.fastq"))
            row["listed"] = tsv[name].count(b"\n") - 1
        out.append(row)
    assert tsv["plain"] == tsv["write-recruited"], "read_matches.tsv differs"
    return out


def run_sampled(args):
    """Wall time of a child process and the peak device memory in use while it runs."""
    free0, _ = torch.cuda.mem_get_info()
    low = [free0]
    stop = threading.Event()

    def sample():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.005)

    th = threading.Thread(target=sample)
    th.start()
    t0 = time.perf_counter()
    r = subprocess.run(args, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    stop.set()
    th.join()
    assert r.returncode == 0, r.stderr
    return wall, free0 - low[0], r.stdout


def screen_bench(fastq, fasta, nreads, runs, tmp):
    os.makedirs(tmp, exist_ok=True)
    paths = {}
    for name, raw in (("fastq", fastq), ("fasta", fasta)):
        paths[name] = os.path.join(tmp, "reads." + ("fastq" if name == "fastq" else "fa"))
        raw.cpu().numpy().tofile(paths[name])
    refs = os.path.join(tmp, "refs.fa")
    host = fasta[:1000 * (READ + 13)].cpu().numpy().tobytes()  # the first 1000 reads as references
    with open(refs, "wb") as f:
        f.write(host)
    base = [KMC, "-q", "-k", "21", "--canonical", "--sketch", "64", "--sketch-direct", "--dialect", "nonl", "--max-seqs",
            "0"]
    out, tsv = [], {}
    for name in ("fastq", "fasta"):
        d = os.path.join(tmp, "out_" + name)
        os.makedirs(d, exist_ok=True)
        args = base + ["--out", d, "--screen", paths[name], refs]
        walls, peaks = [], []
        for i in range(runs + 1):  # the first run warms the page cache
            wall, peak, _ = run_sampled(args)
            if i:
                walls.append(wall)
                peaks.append(peak)
        tsv[name] = open(os.path.join(d, "screen_results.tsv"), "rb").read()
        out.append({"bench": "screen", "format": name, "file_bytes": os.path.getsize(paths[name]), "reads": nreads,
                    "wall_s_median": statistics.median(walls), "wall_s_min": min(walls), "wall_s_max": max(walls),
                    "peak_device_bytes": max(peaks), "runs": runs,
                    "path": "streamed, 256 MiB batches" if name == "fastq" else "whole file"})
    assert tsv["fastq"] == tsv["fasta"], "the two screens differ"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, default=1000, help="FASTQ raw bytes, in MB")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--screen-runs", type=int, default=3)
    ap.add_argument("--tmp", default="/tmp/fastqbench")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pr_fastq.jsonl"))
    ap.add_argument("--skip-screen", action="store_true")
    ap.add_argument("--select", action="store_true", help="kmc_select_records and --write-recruited instead")
    a = ap.parse_args()
    if a.select and a.out.endswith("pr_fastq.jsonl"):
        a.out = os.path.join(REPO, "profiles", "pr_select_records.jsonl")
    if not torch.cuda.is_available():
        sys.exit("fastqbench: no GPU (a measurement needs one)")
    dev = torch.device("cuda:0")
    nreads = a.mbytes * 1000000 // (2 * READ + 16)  # '@r' + 9 digits + '+' + 4 newlines
    fastq, fasta = make_texts(nreads, dev)
    if a.select:
        rows = select_bench(fastq, nreads, a.runs)
        if not a.skip_screen:
            rows += recruit_bench(fastq, fasta, nreads, a.screen_runs, a.tmp)
    else:
        rows = parse_bench(fastq, fasta, nreads, a.runs)
        if not a.skip_screen:
            rows += screen_bench(fastq, fasta, nreads, a.screen_runs, a.tmp)
    note = {"device": torch.cuda.get_device_name(0), "clock_note": "shared machine, clocks not pinned; medians of repeated runs"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            r.update(note)
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
