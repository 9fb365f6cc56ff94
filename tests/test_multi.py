"""Sharding and the N>1 path on CPU: shard plans, and world_size-2 gloo runs of
the shard + all_reduce driver with the oracle as the per-shard counter (the
checker stands in for the HIP kernel; the GPU tests check the kernel's shards)."""
import os
import socket

import numpy as np
import pytest


def _records(seed, lens):
    rng = np.random.default_rng(seed)
    recs = []
    for L in lens:
        s = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=L, p=[.24, .24, .24, .24, .04])
        recs.append(np.append(s, np.uint8(0)))
    data = np.concatenate(recs)
    idx = np.concatenate([[0], np.cumsum([r.size for r in recs])]).astype(np.int64)
    return data, idx


@pytest.mark.parametrize("n", [1, 2, 3, 8, 13])
def test_plan_shards_cover_disjoint_aligned(kmc, n):
    data, idx = _records(1, [10_000, 1, 70_000, 5000, 123_457])
    k = 5
    plan = kmc.plan_shards(idx, k, n)
    assert len(plan) == n
    assert plan[0][0] == idx[0] and plan[-1][1] == idx[-1]
    for (a, b, rl, rh), nxt in zip(plan, plan[1:] + [None]):
        assert a <= b and rl == a and rh == min(b + k - 1, idx[-1])
        if nxt is not None:
            assert nxt[0] == b and b % 4096 == 0
    sizes = [b - a for a, b, _, _ in plan]
    assert max(sizes) - min(sizes) <= 2 * 4096


def test_plan_shards_sum_to_full_with_oracle(kmc, oracle):
    data, idx = _records(2, [50_000, 3, 30_000])
    full, inv = oracle.count_dense(data, idx, 6)
    for n in (2, 5, 64):
        acc = np.zeros_like(full)
        ainv = np.zeros_like(inv)
        for a, b, rl, rh in kmc.plan_shards(idx, 6, n):
            p, pi = oracle.count_dense(data, idx, 6, win=(a, b))
            acc += p
            ainv += pi
        np.testing.assert_array_equal(acc, full)
        np.testing.assert_array_equal(ainv, inv)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, k, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    sys.path[:0] = [os.path.join(repo, "dna-kmeres-parallel_amd"), os.path.join(repo, "oracle")]
    import torch
    import torch.distributed as dist

    import kmc_dist
    import oracle

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    data, idx = _records(3, [40_000, 2, 90_001, 7, 60_000])

    def cpu_counter(d, ix, kk, shard):  # the checker standing in for the HIP kernel
        part, _ = oracle.count_dense(d, ix, kk, win=(shard[0], shard[1]))
        return torch.from_numpy(part)

    out = kmc_dist.count_sharded(data, idx, k, cpu_counter)
    full, _ = oracle.count_dense(data, idx, k)
    q.put((rank, bool(np.array_equal(out.numpy(), full)), int(out.sum())))
    dist.destroy_process_group()


@pytest.mark.parametrize("k", [3, 8])
def test_gloo_world2_shard_allreduce(k):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, k, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _ in res), res
    assert res[0][2] == res[1][2]


def _overlap_worker(rank, world, port, steps, q):
    """bench.py's overlapped steps with a CPU stand-in for the count: each step
    overwrites the whole matrix (rank- and step-specific values in this rank's
    columns, zeros elsewhere, as kmc_count_dense_ex does); after the async gloo
    all-reduces every matrix must hold the sum over ranks of its last step."""
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    import torch
    import torch.distributed as dist

    import bench

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    nb, n_loc = 64, 3
    n_tot = n_loc * world
    bufs = [torch.full((nb, n_tot), -7, dtype=torch.int32) for _ in range(2)]
    last_step = [None, None]

    def count(j):
        i = last_step[j]
        bufs[j].zero_()
        cols = torch.arange(n_loc, dtype=torch.int32) + rank * n_loc
        bufs[j][:, rank * n_loc:(rank + 1) * n_loc] = (i * 1000 + cols)[None, :] + torch.arange(nb, dtype=torch.int32)[:, None]

    step, drain = bench.overlapped_steps(bufs, count, world, dist.all_reduce)
    ok = True
    for i in range(steps):
        j = i % 2
        last_step[j] = i
        step(i)
    drain()
    for j in range(2):
        i = last_step[j]
        exp = (i * 1000 + torch.arange(n_tot, dtype=torch.int32))[None, :] + torch.arange(nb, dtype=torch.int32)[:, None]
        ok = ok and bool(torch.equal(bufs[j], exp))
    q.put((rank, ok))
    dist.destroy_process_group()


def _spawn(target, world, *args):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    return res


def test_gloo_world2_bench_overlapped_allreduce():
    res = _spawn(_overlap_worker, 2, 7)
    assert all(ok for _, ok in res), res


def _bench_step_worker(rank, world, port, scaling, records, L, k, steps, q):
    """bench.py's step driver exactly as the GPU run uses it (rank_plan: which
    bytes a rank holds and which windows it counts; overlapped_steps: count, then
    the async all-reduce), with the rank's bytes generated on the host
    (synth_host_range, the twin of kmc_synth_fill_range) and the oracle as the
    counter over the rank's window range of the global offsets."""
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    sys.path[:0] = [repo, os.path.join(repo, "dna-kmeres-parallel_amd"), os.path.join(repo, "oracle")]
    import torch
    import torch.distributed as dist

    import bench
    import kmc
    import oracle

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seed = bench.SEED_BASE + k
    plan = bench.rank_plan(scaling, world, rank, records, L, k)
    n_tot, idx = plan["n_tot"], plan["indices"]
    base, hold_hi = plan["hold"]
    win_lo, win_hi = plan["win"]
    read_lo, read_hi = plan["read"]
    held = kmc.synth_host_range(base, hold_hi, L, seed)
    # the oracle indexes the global buffer: the held bytes go to their global
    # offsets and every other byte is 'A', so a count that read outside
    # [read_lo, read_hi) would show
    total = int(idx[-1])
    glob = np.full(total, ord("A"), dtype=np.uint8)
    glob[read_lo:read_hi] = held[read_lo - base:read_hi - base]
    bufs = [torch.full((1 << (2 * k), n_tot), -1, dtype=torch.int32) for _ in range(2)]

    def count(j):
        part, _ = oracle.count_dense(glob, idx, k, win=(win_lo, win_hi))
        bufs[j].copy_(torch.from_numpy(part))

    step, drain = bench.overlapped_steps(bufs, count, world, dist.all_reduce)
    for i in range(steps):
        step(i)
    drain()
    full, _ = oracle.count_dense(kmc.synth_host_range(0, total, L, seed), idx, k)
    ok = all(bool(np.array_equal(b.numpy(), full)) for b in bufs[:min(steps, 2)])
    sums_ok = bool((bufs[0].to(torch.int64).sum(dim=0) == L - k + 1).all())
    q.put((rank, ok, sums_ok, (win_lo, win_hi)))
    dist.destroy_process_group()


@pytest.mark.parametrize("world,scaling,records,L,k", [
    (2, "strong", 5, 9_000, 8),   # shard cuts inside records
    (4, "strong", 5, 9_000, 4),
    (4, "strong", 3, 1_000, 3),   # 3003 bytes < one 4 KiB cut: three empty shards
    (2, "weak", 3, 5_000, 8),
    (4, "weak", 2, 3_000, 5),
    (8, "weak", 10, 2_000, 8),    # C5's plan: 10 records per rank, 8 ranks
    (8, "strong", 10, 20_000, 8),  # the headline's plan at 8 ranks (cuts inside records)
])
def test_gloo_bench_step_driver(world, scaling, records, L, k):
    res = _spawn(_bench_step_worker, world, scaling, records, L, k, 3)
    assert all(ok and sums for _, ok, sums, _ in res), res
    wins = sorted(w for *_, w in res)
    # the ranks' window ranges tile the job's buffer exactly
    assert wins[0][0] == 0 and all(a[1] == b[0] for a, b in zip(wins, wins[1:]))
    n_tot = records if scaling == "strong" else records * world
    assert wins[-1][1] == n_tot * (L + 1)


def test_bench_rank_plan_single_gpu_is_whole_buffer(kmc):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    for scaling in ("strong", "weak"):
        p = bench.rank_plan(scaling, 1, 0, 10, 1_000_000_000, 8)
        assert p["n_tot"] == 10 and p["win"] == (0, 10 * 1_000_000_001) and p["read"] == p["win"]
        assert p["hold"] == (0, 10 * 1_000_000_001)
    # 8-way strong plan of the 10 Gbase job: 4 KiB-aligned cuts, halo k-1, 16-aligned buffers
    plans = [bench.rank_plan("strong", 8, r, 10, 1_000_000_000, 8) for r in range(8)]
    for r, p in enumerate(plans):
        lo, hi = p["win"]
        assert p["read"] == (lo, min(hi + 7, 10 * 1_000_000_001)) and p["base"] % 16 == 0
        if r:
            assert lo % 4096 == 0 and plans[r - 1]["win"][1] == lo
        assert abs((hi - lo) - 1_250_000_001) <= 4096


def test_synth_host_range_matches_whole_records(kmc):
    whole = kmc.synth_host(4, 1000, seed=0x5EED0008)
    for lo, hi in [(0, 4004), (1, 17), (999, 1003), (1000, 1001), (2500, 4004), (7, 7)]:
        np.testing.assert_array_equal(kmc.synth_host_range(lo, hi, 1000, 0x5EED0008), whole[lo:hi])


def test_bench_host_histogram_matches_oracle(oracle):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    import kmc as _k
    b = _k.synth_host_range(123, 123 + 50_000, 1_000_000, 0x5EED0008)
    for k in (1, 5, 8):
        exp, _ = oracle.count_dense(np.append(b, np.uint8(0)), np.array([0, b.size + 1], dtype=np.int64), k)
        np.testing.assert_array_equal(bench.host_kmer_hist(b, k), exp[:, 0])


def _finalize_worker(rank, world, port, full, q):
    """bench.finalize (everything after the timed region) at world 2 with gloo on
    CPU tensors: the N > 1 line must carry the node roofline fraction, the RCCL
    world size and backend and, with --full, the all-reduce time and the reference
    CPU path on rank 0."""
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    sys.path[:0] = [repo, os.path.join(repo, "dna-kmeres-parallel_amd"), os.path.join(repo, "oracle")]
    import torch
    import torch.distributed as dist

    import bench
    import kmc

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    k, L, records = 8, 200_000, 4
    args = bench.parse(["--gpus", str(world), "--steps", "5", "--cpu-sample", "30000", "--cpu-threads", "2",
                        "--allreduce-reps", "3", "--k", str(k), "--records", str(records), "--record-len", str(L)]
                       + (["--full"] if full else []))
    plan = bench.rank_plan("strong", world, rank, records, L, k)
    base, hold_hi = plan["hold"]
    data = torch.from_numpy(kmc.synth_host_range(base, hold_hi, L, bench.SEED_BASE + k).copy())
    matrix = torch.zeros((1 << (2 * k), records), dtype=torch.int32)
    win = plan["win"]
    alg = (win[1] - win[0]) + 4 * (1 << (2 * k)) * records
    kern_ms = 0.5 + rank  # rank 1 is the slow one
    steps = [kern_ms + 0.1 * i for i in range(5)]  # per-step kernel times: median kern_ms + 0.2
    res = bench.finalize(args, world, rank, "gloo", data, matrix, L, k, records, win, 0.01 * (1 + rank), kern_ms,
                         alg, timer="host", step_ms=steps)
    q.put((rank, res))
    dist.destroy_process_group()


def test_gloo_world2_bench_line_fields():
    res = dict(_spawn(_finalize_worker, 2, True))
    assert res[1] is None
    r = res[0]
    assert r["full"] is True
    assert r["n_gpus"] == 2 and r["config"]["rccl_world"] == 2 and r["config"]["backend"] == "gloo"
    assert "reserved_cus" in r["config"] and "rccl_max_channels" in r["config"]
    # the untimed clock settle is reported beside W (finalize alone ran none)
    assert r["warmup"] == 14 and r["settle"]["ms"] == 150.0 and r["settle"]["launches"] == 0
    # max over ranks: rank 1's elapsed and kernel time
    assert abs(r["ms_per_step"] - 0.02 / 5 * 1e3) < 1e-9 and r["roofline"]["kernel_ms"] == 1.5
    rf = r["roofline"]
    # per-step spread of the slowest rank (rank 1: 1.5 .. 1.9 ms)
    assert abs(rf["kernel_ms_median"] - 1.7) < 1e-9 and rf["kernel_ms_min"] == 1.5 and abs(rf["kernel_ms_max"] - 1.9) < 1e-9
    assert rf["build_id"] is None and rf["traffic"] is None  # host timer: no GPU build measured
    for key in ("achieved", "frac", "node_achieved", "node_frac", "node_peak", "alg_bytes_per_kmer"):
        assert rf[key] > 0, key
    assert rf["node_peak"] == 2 * rf["peak"]
    # node fraction = value x algorithmic bytes per k-mer / (N x peak)
    assert abs(rf["node_frac"] - r["value"] * rf["alg_bytes_per_kmer"] / 1e9 / (2 * rf["peak"])) < 1e-12
    assert r["allreduce"]["ms"] > 0 and r["allreduce"]["bytes"] == 4 * 65536 * 4
    cb = r["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] == 2 and cb["kind"] in ("reference", "port")


def test_gloo_world2_plain_bench_line_leaves_the_extras_to_full():
    """Without --full the line keeps the headline fields and the roofline of the
    timed steps, and neither times the all-reduce alone nor runs the CPU baseline."""
    res = dict(_spawn(_finalize_worker, 2, False))
    assert res[1] is None
    r = res[0]
    assert r["full"] is False and "cpu_baseline" not in r and r["allreduce"]["ms"] is None
    assert r["metric"].startswith("k-mers/sec") and r["unit"] == "k-mers/s" and r["dtype"] == "u8"
    assert r["higher_is_better"] is True and r["steps"] == 5
    # max over ranks of the timed region over its steps, and k-mers of the job over that time
    assert abs(r["ms_per_step"] - 0.02 / 5 * 1e3) < 1e-9
    assert abs(r["value"] - 4 * (200_000 - 8 + 1) * 5 / 0.02) < 1e-3
    assert r["roofline"]["kernel_ms"] == 1.5 and r["roofline"]["node_frac"] > 0


def test_bench_steps_and_full_options():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_bench_dump_outputs_is_exact_and_its_sample_is_fixed(tmp_path, monkeypatch):
    """--dump-outputs: counts.npy holds the int32 matrix exactly as float64; above
    the size limit it holds the same seeded positions of the matrix on every run."""
    import torch

    import bench
    m = torch.arange(-6, 6, dtype=torch.int32).reshape(4, 3) * 178_956_970  # up to the int32 range
    bench.dump_outputs(str(tmp_path / "a"), m)
    got = np.load(tmp_path / "a" / "counts.npy")
    assert got.dtype == np.float64 and got.shape == (4, 3)
    np.testing.assert_array_equal(got.astype(np.int64), m.numpy().astype(np.int64))
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 1000)
    big = torch.arange(50_000, dtype=torch.int32).reshape(500, 100)
    bench.dump_outputs(str(tmp_path / "b"), big)
    bench.dump_outputs(str(tmp_path / "c"), big + 1)
    b, c = np.load(tmp_path / "b" / "counts.npy"), np.load(tmp_path / "c" / "counts.npy")
    assert b.ndim == 1 and 900 < b.size <= 1000 and b.dtype == np.float64
    assert np.all(np.diff(b) > 0) and b.min() >= 0 and b.max() < 50_000  # ascending positions of the matrix
    np.testing.assert_array_equal(c, b + 1)  # the same positions in another run


def test_multi_refuses_a_record_of_2p31_windows_on_the_host(kmc):
    """kmc_count_multi splits records over devices, so no shard's own device check
    sees 2^31 windows of one record; the host offsets are checked first
    (KMC_ERR_RECORD_TOO_LONG) before any HIP call.  A record of 2^31 - 1 windows
    passes that check (and then needs a device: not RECORD_TOO_LONG)."""
    import ctypes
    L = kmc.lib()
    buf = (ctypes.c_char * 64)()
    out = (ctypes.c_int32 * 16)()
    for k, extra, too_long in ((3, 0, True), (3, -1, False), (8, 0, True), (1, 5, True)):
        idx = np.array([0, 10, 10 + (1 << 31) + k + extra], dtype=np.int64)
        rc = L.kmc_count_multi(ctypes.cast(buf, ctypes.c_void_p), idx.ctypes.data_as(ctypes.c_void_p), 2,
                               int(idx[-1]), k, 1, None, ctypes.cast(out, ctypes.c_void_p), None)
        assert (rc == kmc.KMC_ERR_RECORD_TOO_LONG) == too_long, (k, extra, rc)


def test_count_sharded_refuses_a_record_of_2p31_windows():
    """The torch.distributed path (kmc_dist.count_sharded) makes the same host check
    before it counts or all-reduces anything."""
    import kmc
    import kmc_dist
    idx = np.array([0, 100, 100 + (1 << 31) + 8], dtype=np.int64)
    with pytest.raises(kmc.KmcError) as ei:
        kmc_dist.count_sharded(None, idx, 8, counter=None, group=None)
    assert ei.value.code == kmc.KMC_ERR_RECORD_TOO_LONG
    kmc_dist.check_record_windows(idx - np.array([0, 0, 1]), 8)  # 2^31 - 1 windows: accepted


def test_bench_pmc_entries_are_tied_to_the_build(tmp_path, kmc):
    """bench.py reports a PMC traffic / LDS figure only from an entry taken on the
    build it runs (the id of libkmc.so's count_dense_kernel code object): a
    matching entry is used, an entry of another build or one without an id is not."""
    import json
    import bench
    bid = bench.dense_code_object_id(kmc.LIB_PATH)
    assert bid is not None and len(bid) == 16
    assert bench.dense_code_object_id(kmc.DIAG_LIB_PATH) not in (None, bid)  # another build of the kernel
    e = {"k": 8, "data_bytes": 1000, "hbm_bytes_per_launch": 1234.0}
    p = tmp_path / "pmc.json"
    for entry, want in ((dict(e, build_id=bid), 1234.0), (dict(e, build_id="0" * 16), None), (e, None)):
        p.write_text(json.dumps([entry]))
        assert bench.pmc_traffic(str(p), 8, 1000, bid) == want
    lds = {"k": 8, "lds_busy_frac": 0.9}
    for entry, ok in ((dict(lds, build_id=bid), True), (dict(lds, build_id="x"), False), (lds, False)):
        p.write_text(json.dumps(entry))
        assert (bench.lds_floor(str(p), 8, bid) is not None) == ok
