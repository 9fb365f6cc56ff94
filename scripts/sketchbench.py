#!/usr/bin/env python3
"""sketchbench.py — times kmc_sketch_from_counts, kmc_sketch_distances and
kmc_pair_distances_sparse on the same canonical lists (HIP events, warm-up, median
of --runs) and writes one JSON line per (input, sketch size) to --out
(profiles/pr_sketch.jsonl).  With --direct: kmc_sketch_from_sequences beside the
two-step path kmc_count_canonical_hash + kmc_sketch_from_counts on the same inputs
(rows asserted equal, both workspace sizes), and on one all-A record
(profiles/pr_sketch_direct.jsonl).  With --grouped: kmc_sketch_from_sequences_grouped
beside the ungrouped call, the ungrouped call + kmc_sketch_merge_groups and the
distances on group rows and on record rows (profiles/pr_sketch_grouped.jsonl).
With --query: kmc_sketch_nearest and kmc_sketch_distances_rect (alone and followed by
torch.topk) beside kmc_sketch_distances over the concatenation of queries and
references, on synthetic rows (profiles/pr_sketch_query.jsonl).
With --screen: kmc_sketch_screen_build, _count and _results of 1000 references of
1 Mbase (and of 100 of 5 kbase) in a mixture of 1000 x 1 Mbase, beside
kmc_sketch_from_sequences_grouped over the same mixture as one group, the same walk
plus the set upkeep (profiles/pr_sketch_screen.jsonl); kmc_sketch_screen_winners on the
same counted index beside _results, and once more on a redundant collection: the same
rows as 50 groups of 20 that share 90 % of their values (--out
profiles/pr_screen_winners.jsonl).
With --accum: kmc_sketch_accum_add over the same mixture, as one call and as 16 calls
(j rises and purges happen), and kmc_sketch_accum_finish, beside kmc_sketch_screen_count
against the 1000-reference index and kmc_sketch_from_sequences_grouped with one group:
the parent commit's code on the same walk (profiles/pr_sketch_accum.jsonl); and
kmc_spectrum_from_accum of the same table with 256 and 8192 bins, beside _finish
(--out profiles/pr_spectrum.jsonl).
With --cluster: kmc_sketch_cluster beside kmc_sketch_distances on the same rows, unrelated
rows and 64-member clusters of near-identical rows (profiles/pr_sketch_cluster.jsonl).
With --links: kmc_sketch_links, count-only and with a fitting capacity, beside
kmc_sketch_distances with counts and kmc_sketch_cluster on those rows
(profiles/pr_sketch_links.jsonl).  With --classify: kmc_classify_from_accum beside
kmc_match_from_accum, kmc_label_accum beside kmc_sketch_accum_add
(profiles/pr_classify.jsonl).

Inputs (synthetic, generated on the device):
  iid          8 x 50 Mbase independent records, k = 31
  copies_1pct  record 0 and 7 copies of it with 1 % substitutions, k = 31; the Mash
               distance of (0, i) is recorded next to the 0.01 substitution rate
  many         4096 x 100 kbase independent records, k = 21: the regime the sketch is
               for (the exact path leaves its LDS pair matrix above 64 records)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "dna-kmeres-parallel_amd"))

import torch  # noqa: E402

import kmc  # noqa: E402


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


def timed_wall(fn, runs, warmup=1):
    """Host clock from an idle device to an idle device: what a caller waits for.
    The measure for a path that synchronises and allocates inside (count_canonical)."""
    import time
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "runs": runs}


def make_input(name, records, record_len, dev):
    data = torch.empty(records * (record_len + 1), dtype=torch.uint8, device=dev)
    kmc.synth_fill(data, records, record_len, 0x5EED0008)
    if name == "copies_1pct":
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        rows = data.view(records, record_len + 1)
        lut = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)  # ACGT
        code = torch.zeros(256, dtype=torch.int64, device=dev)
        code[lut.long()] = torch.arange(4, device=dev)
        base = rows[0, :record_len].clone()
        for r in range(1, records):
            hit = torch.rand(record_len, device=dev, generator=g) < 0.01
            step = torch.randint(1, 4, (record_len,), device=dev, generator=g)
            sub = lut[(code[base.long()] + step) % 4]  # always another base
            rows[r, :record_len] = torch.where(hit, sub, base)
    idx = torch.from_numpy(kmc.synth_indices(records, record_len)).to(dev)
    return data, idx


def direct_main(args, dev, shapes):
    """--direct: the one-pass sketcher against the two-step path, in this process and
    on this device.  The baseline is the two-step path as a caller runs it
    (count_canonical reads the distinct total back; its output arrays hold 12 bytes
    per input byte), timed as a whole and with the sketch stage alone."""
    with open(args.out, "w") as out:
        for name in args.inputs.split(","):
            records, record_len, k = shapes[name]
            record_len = max(int(record_len * args.scale), k + 1)
            data, idx = make_input(name, records, record_len, dev)
            idx_host = idx.cpu().numpy()
            keys, counts, off = kmc.count_canonical(data, idx, k)
            torch.cuda.synchronize()
            for s in (int(x) for x in args.sizes.split(",")):
                two = kmc.sketch_from_counts(keys, counts, off, s)
                one = kmc.sketch_from_sequences(data, idx, k, s)
                torch.cuda.synchronize()
                assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]), (name, s)
                rec = {
                    "input": name, "records": records, "record_len": record_len, "k": k, "sketch_size": s,
                    "entries": int(keys.numel()), "rows_equal": True,
                    "workspace_bytes_direct": kmc.sketch_from_sequences_workspace_size(records, data.numel(), s),
                    "workspace_bytes_two_step": kmc.canonical_workspace_size(idx_host, k)
                    + kmc.sketch_workspace_size(records, keys.numel(), s),
                    "list_bytes_two_step": 12 * int(data.numel()),
                    "kmc_sketch_from_sequences": timed(lambda: kmc.sketch_from_sequences(data, idx, k, s), args.runs),
                    "kmc_sketch_from_counts": timed(lambda: kmc.sketch_from_counts(keys, counts, off, s), args.runs),
                    # host clock, idle to idle, for the path that synchronises inside and for each half
                    "two_step_wall": timed_wall(lambda: kmc.sketch_from_counts(*kmc.count_canonical(data, idx, k), s),
                                                max(args.runs // 2, 3)),
                    "count_canonical_wall": timed_wall(lambda: kmc.count_canonical(data, idx, k),
                                                       max(args.runs // 2, 3)),
                    "sketch_from_sequences_wall": timed_wall(lambda: kmc.sketch_from_sequences(data, idx, k, s),
                                                             args.runs),
                }
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
            del keys, counts, off, data
            torch.cuda.empty_cache()
        # the degenerate record: one key, so the set never fills and every window passes
        # the threshold; each is found in the set by a binary search and is not staged
        n_a = max(int(50_000_000 * args.scale), 64)
        data = torch.full((n_a + 1,), 65, dtype=torch.uint8, device=dev)
        data[n_a] = 0
        idx = torch.tensor([0, n_a + 1], dtype=torch.int64, device=dev)
        for s in (int(x) for x in args.sizes.split(",")):
            sk, sz = kmc.sketch_from_sequences(data, idx, 31, s)
            torch.cuda.synchronize()
            assert int(sz[0]) == 1 and int(sk[0, 1]) == -1  # the key of poly-A (= poly-T) alone, then the fill
            rec = {"input": "all_a", "records": 1, "record_len": n_a, "k": 31, "sketch_size": s,
                   "kmc_sketch_from_sequences": timed(lambda: kmc.sketch_from_sequences(data, idx, 31, s), args.runs)}
            out.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)


def grouped_main(args, dev):
    """--grouped: kmc_sketch_from_sequences_grouped beside the paths the parent commit
    offers for the same rows: the ungrouped call (identity grouping), the ungrouped call
    followed by kmc_sketch_merge_groups, and kmc_sketch_distances on the group rows
    beside the record rows.  Rows are asserted equal before anything is timed."""
    shapes = [  # name, groups, records per group, record length, k, sketch sizes, time the record distances
        ("identity", 4096, 1, 100_000, 21, (1000, 10000), False),
        ("draft_assembly", 8, 500, 100_000, 21, (1000,), True),
        ("read_set", 4, 650_000, 150, 21, (1000,), False),
    ]
    only = set(args.inputs.split(",")) if args.inputs != "iid,copies_1pct,many" else None
    runs = 5
    with open(args.out, "a") as out:
        for name, groups, per, record_len, k, sizes, rec_dist in shapes:
            if only is not None and name not in only:
                continue
            record_len = max(int(record_len * args.scale), k + 1) if name != "read_set" else record_len
            if name == "read_set":
                per = max(int(per * args.scale), 1)
            records = groups * per
            data, idx = make_input("many", records, record_len, dev)
            go = torch.arange(0, records + 1, per, dtype=torch.int64, device=dev)
            for s in sizes:
                grp = kmc.sketch_from_sequences_grouped(data, idx, go, k, s)
                rec_rows = kmc.sketch_from_sequences(data, idx, k, s)
                via = rec_rows if per == 1 else kmc.sketch_merge_groups(*rec_rows, go)
                torch.cuda.synchronize()
                assert torch.equal(grp[0], via[0]) and torch.equal(grp[1], via[1]), (name, s)
                rec = {
                    "input": name, "groups": groups, "records": records, "record_len": record_len, "k": k,
                    "sketch_size": s, "rows_equal": True,
                    "workspace_bytes_grouped": kmc.sketch_from_sequences_grouped_workspace_size(
                        records, groups, data.numel(), s),
                    "workspace_bytes_ungrouped": kmc.sketch_from_sequences_workspace_size(records, data.numel(), s),
                    "ungrouped_row_bytes": 8 * s * records,
                    "kmc_sketch_from_sequences_grouped": timed(
                        lambda: kmc.sketch_from_sequences_grouped(data, idx, go, k, s), runs),
                    "kmc_sketch_from_sequences": timed(lambda: kmc.sketch_from_sequences(data, idx, k, s), runs),
                }
                if per > 1:
                    rec["kmc_sketch_merge_groups"] = timed(lambda: kmc.sketch_merge_groups(*rec_rows, go), runs)
                    rec["kmc_sketch_distances_groups"] = timed(lambda: kmc.sketch_distances(*grp, k), runs)
                    if rec_dist:
                        rec["kmc_sketch_distances_records"] = timed(lambda: kmc.sketch_distances(*rec_rows, k), runs)
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
                del grp, rec_rows, via
                torch.cuda.empty_cache()
            del data, idx, go
            torch.cuda.empty_cache()


def synthetic_rows(n, s, dev, seed):
    """n full rows of s ascending values: a third of each row comes from a shared pool of
    4 s values (so pairs share a few values and the hits differ), the rest is its own."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    own = torch.randint(0, 1 << 62, (n, s), dtype=torch.int64, device=dev, generator=g)
    pool = torch.randint(0, 1 << 62, (4 * s,), dtype=torch.int64, device=dev, generator=g)
    pick = torch.randint(0, 4 * s, (n, s // 3), device=dev, generator=g)
    own[:, :s // 3] = pool[pick]
    rows = torch.sort(own, dim=1).values
    # distinct within a row: a repeated value moves up by its position (random 62-bit values: rare)
    dup = torch.zeros_like(rows, dtype=torch.bool)
    dup[:, 1:] = rows[:, 1:] == rows[:, :-1]
    rows = torch.sort(rows + dup * torch.arange(1, s + 1, device=dev), dim=1).values
    return rows.contiguous(), torch.full((n,), s, dtype=torch.int32, device=dev)


def query_main(args, dev):
    """--query: m queries in n references.  kmc_sketch_nearest, kmc_sketch_distances_rect,
    the rectangle followed by torch.topk, and the parent commit's only route:
    kmc_sketch_distances over the m + n rows.  The hits are asserted equal to the
    rectangle's best before anything is timed."""
    m, k, top = 64, 21, 10
    shapes = [(4096, 1000), (65536, 1000), (4096, 10000)]
    with open(args.out, "w") as out:
        for n, s in shapes:
            n = max(int(n * args.scale), top + 1)
            q, qs = synthetic_rows(m, s, dev, 1)
            r, rs = synthetic_rows(n, s, dev, 2)
            r[:m:2] = q[:m:2]  # half of the queries are in the collection
            both, both_s = torch.cat([q, r]), torch.cat([qs, rs])
            refs, sh, dn, dist, counts = kmc.sketch_nearest(q, qs, r, rs, k, top)
            rect, rsh, rdn = kmc.sketch_distances_rect(q, qs, r, rs, k, with_counts=True)
            torch.cuda.synchronize()
            assert int(counts.min()) == top
            rows = torch.arange(m, device=dev)[:, None]
            assert torch.equal(rsh[rows, refs.long()], sh) and torch.equal(rdn[rows, refs.long()], dn)
            assert torch.equal(rect[rows, refs.long()], dist)
            # the i-th hit's J is the i-th largest of the row (exact in double: both numbers <= 16384)
            j_all = (rsh.double() / rdn.double()) * (rsh >= 1)
            assert torch.equal(torch.topk(j_all, top, dim=1).values, sh.double() / dn.double())
            pairs_all = (m + n) * (m + n - 1) // 2
            rec = {
                "queries": m, "refs": n, "sketch_size": s, "k": k, "top": top,
                "pairs_rect": m * n, "pairs_all_pairs": pairs_all, "hits_equal_rect": True,
                "workspace_bytes_nearest": kmc.sketch_nearest_workspace_size(m, n, s, top),
                "rect_bytes": 4 * m * n, "all_pairs_bytes": 4 * pairs_all,
                "kmc_sketch_nearest": timed(lambda: kmc.sketch_nearest(q, qs, r, rs, k, top), args.runs),
                "kmc_sketch_distances_rect": timed(lambda: kmc.sketch_distances_rect(q, qs, r, rs, k), args.runs),
                "rect_then_topk": timed(
                    lambda: torch.topk(kmc.sketch_distances_rect(q, qs, r, rs, k), top, dim=1, largest=False),
                    args.runs),
            }
            if 4 * pairs_all <= 16 << 30:  # the parent commit's route, where its triangle fits
                # s = 10000 runs from global memory: fewer runs
                rec["kmc_sketch_distances_all_pairs"] = timed(lambda: kmc.sketch_distances(both, both_s, k),
                                                              3 if s > 2048 else args.runs, warmup=1)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(json.dumps(rec), flush=True)
            del q, r, both, rect, rsh, rdn, j_all
            torch.cuda.empty_cache()


def clustered_rows(n, s, dev, seed, members=64, changed=0.02):
    """n full rows in groups of `members`: every row of a group is the group's base row
    (synthetic_rows) with about `changed` of its values replaced by values of its own."""
    base, _ = synthetic_rows((n + members - 1) // members, s, dev, seed)
    rows = base.repeat_interleave(members, dim=0)[:n].clone()
    g = torch.Generator(device=dev)
    g.manual_seed(seed + 1)
    hit = torch.rand((n, s), device=dev, generator=g) < changed
    rows[hit] = torch.randint(0, 1 << 62, (int(hit.sum()),), dtype=torch.int64, device=dev, generator=g)
    rows = torch.sort(rows, dim=1).values
    dup = torch.zeros_like(rows, dtype=torch.bool)
    dup[:, 1:] = rows[:, 1:] == rows[:, :-1]
    rows = torch.sort(rows + dup * torch.arange(1, s + 1, device=dev), dim=1).values
    return rows.contiguous(), torch.full((n,), s, dtype=torch.int32, device=dev)


def cluster_main(args, dev):
    """--cluster: kmc_sketch_cluster at the Jaccard threshold of Mash distance 0.05 beside
    kmc_sketch_distances, the existing code that reads the same rows through the same
    tiles, in one process.  unrelated: no pair is linked; clustered: groups of 64 rows
    that differ in 2 % of their values.  The labels are asserted before anything is
    timed.  The margin is DESIGN.md 4.3c's: the clustering may be slower than the
    triangle by at most twice the spread (max - min) of the triangle's own runs."""
    k, s, members = 21, 1000, 64
    mj = kmc.mash_jaccard_of_distance(0.05, k)
    with open(args.out, "w") as out:
        for n in (4096, 65536):
            n = max(int(n * args.scale), 2 * members)
            runs = args.runs if n <= 8192 else max(5, args.runs // 2)
            for name, make in (("unrelated", synthetic_rows), ("clustered", clustered_rows)):
                rows, sizes = make(n, s, dev, 3)
                labels, index, count = kmc.sketch_cluster(rows, sizes, mj)
                torch.cuda.synchronize()
                ids = torch.arange(n, device=dev, dtype=torch.int32)
                exp = ids if name == "unrelated" else ids // members * members
                assert torch.equal(labels, exp), name
                assert torch.equal(index, ids if name == "unrelated" else ids // members)
                assert int(count) == (n if name == "unrelated" else (n + members - 1) // members)
                tri_out = torch.empty(n * (n - 1) // 2, dtype=torch.float32, device=dev)
                ws = torch.empty(kmc.sketch_cluster_workspace_size(n), dtype=torch.uint8, device=dev)
                outs = (labels, index, count)
                tri = timed(lambda: kmc.sketch_distances(rows, sizes, k, out=(tri_out, None, None)), runs, warmup=1)
                clu = timed(lambda: kmc.sketch_cluster(rows, sizes, mj, workspace=ws, out=outs), runs, warmup=1)
                only = timed(lambda: kmc.sketch_cluster(rows, sizes, mj, workspace=ws, out=(labels, None, None)), runs,
                             warmup=1)
                spread = tri["ms_max"] - tri["ms_min"]
                rec = {
                    "collection": name, "rows": n, "sketch_size": s, "k": k, "max_dist": 0.05, "min_jaccard": mj,
                    "members": members if name == "clustered" else 1, "clusters": int(count),
                    "pairs": n * (n - 1) // 2, "triangle_bytes": 4 * (n * (n - 1) // 2),
                    "workspace_bytes_cluster": kmc.sketch_cluster_workspace_size(n), "same_root_skip": False,
                    "kmc_sketch_distances": tri, "kmc_sketch_cluster": clu, "kmc_sketch_cluster_labels_only": only,
                    "triangle_spread_ms": spread,
                    "cluster_minus_triangle_ms": clu["ms_median"] - tri["ms_median"],
                    "within_margin": clu["ms_median"] <= tri["ms_median"] + 2 * spread,
                }
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
                del rows, sizes, tri_out, ws, labels, index, count
                torch.cuda.empty_cache()


def links_main(args, dev):
    """--links: kmc_sketch_links at the Jaccard threshold of Mash distance 0.05 on the rows of
    --cluster, count-only and with a capacity that fits, beside the two yardsticks that read
    the same rows through the same tiles in the same process: kmc_sketch_distances with its
    counts (the only route to the list before) and kmc_sketch_cluster.  unrelated: no pair is
    listed; clustered: 64-member groups, 2016 pairs each.  The list is asserted (its count,
    every pair inside a group, the components equal to the clustering's labels) before
    anything is timed."""
    k, s, members = 21, 1000, 64
    mj = kmc.mash_jaccard_of_distance(0.05, k)
    with open(args.out, "w") as out:
        for n in (4096, 65536):
            n = max(int(n * args.scale), 2 * members)
            runs = args.runs if n <= 8192 else max(3, args.runs // 3)
            pairs = n * (n - 1) // 2
            for name, make in (("unrelated", synthetic_rows), ("clustered", clustered_rows)):
                rows, sizes = make(n, s, dev, 3)
                links, dist, count = kmc.sketch_links(rows, sizes, k, mj)  # (sorted, exact capacity)
                total = int(count)
                groups, last = divmod(n, members)
                exp = 0 if name == "unrelated" else groups * (members * (members - 1) // 2) + last * (last - 1) // 2
                assert total == exp == links.shape[0], (name, total, exp)
                labels, _, _ = kmc.sketch_cluster(rows, sizes, mj, index=False)
                if total:
                    assert torch.equal(links[:, 0] // members, links[:, 1] // members) and bool((links[:, 0] < links[:, 1]).all())
                    assert torch.equal(labels[links[:, 0].long()], labels[links[:, 1].long()])
                    assert torch.unique((links[:, 0].long() << 32) | links[:, 1].long()).numel() == total
                    assert bool((links[:, 2].double() >= mj * links[:, 3].double()).all()) and float(dist.max()) <= 0.05
                cap = max(total, 1)
                outs = (torch.empty((cap, 4), dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.float32, device=dev),
                        count)
                ws = torch.empty(kmc.sketch_cluster_workspace_size(n), dtype=torch.uint8, device=dev)
                only = timed(lambda: kmc.sketch_links(rows, sizes, k, mj, capacity=0, out=(None, None, count)), runs, warmup=1)
                fit = timed(lambda: kmc.sketch_links(rows, sizes, k, mj, capacity=cap, out=outs), runs, warmup=1)
                assert int(count) == total
                clu = timed(lambda: kmc.sketch_cluster(rows, sizes, mj, workspace=ws, out=(labels, None, None)), runs, warmup=1)
                rec = {
                    "collection": name, "rows": n, "sketch_size": s, "k": k, "max_dist": 0.05, "min_jaccard": mj,
                    "members": members if name == "clustered" else 1, "pairs": pairs, "links": total,
                    "list_bytes": 20 * total, "triangle_with_counts_bytes": 12 * pairs,
                    "kmc_sketch_links_count_only": only, "kmc_sketch_links": fit, "kmc_sketch_cluster_labels_only": clu,
                    "links_over_cluster": fit["ms_median"] / clu["ms_median"],
                    "count_only_over_cluster": only["ms_median"] / clu["ms_median"],
                }
                del outs, ws, links, dist
                torch.cuda.empty_cache()
                free = torch.cuda.mem_get_info(dev)[0]
                if 12 * pairs <= free - (4 << 30):  # the triangle with its counts, where it fits
                    tri_out = tuple(torch.empty(pairs, dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.int32))
                    tri = timed(lambda: kmc.sketch_distances(rows, sizes, k, with_counts=True, out=tri_out), runs, warmup=1)
                    rec["kmc_sketch_distances_with_counts"] = tri
                    rec["links_over_triangle"] = fit["ms_median"] / tri["ms_median"]
                    del tri_out
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
                del rows, sizes, labels, count
                torch.cuda.empty_cache()


def screen_main(args, dev):
    """--screen: references in a mixture.  Half of the references are cut from the
    mixture (reference r, r even, is the head of mixture record r); shared == size is
    asserted for them, and no more than chance hits for the others, before anything is
    timed.  The
    yardstick for count is the grouped sketch of the whole mixture, on the same buffer.
    winners runs on the same counted index as results, with a caller's workspace; with
    nothing shared between rows its numbers are asserted to be results' own."""
    k, s, records = 21, 1000, 1000
    record_len = max(int(1_000_000 * args.scale), 5000)
    mix = torch.empty(records * (record_len + 1), dtype=torch.uint8, device=dev)
    kmc.synth_fill(mix, records, record_len, 0x5EED0008)
    midx = torch.from_numpy(kmc.synth_indices(records, record_len)).to(dev)
    one_group = torch.tensor([0, records], dtype=torch.int64, device=dev)
    grouped = timed(lambda: kmc.sketch_from_sequences_grouped(mix, midx, one_group, k, s), args.runs)
    with open(args.out, "a") as out:
        for name, nrefs, ref_len in (("genomes", 1000, record_len), ("viruses", 100, 5000)):
            refs = torch.empty(nrefs * (ref_len + 1), dtype=torch.uint8, device=dev)
            kmc.synth_fill(refs, nrefs, ref_len, 0x5EED0009)
            refs.view(nrefs, ref_len + 1)[::2] = mix.view(records, record_len + 1)[:nrefs:2, :ref_len + 1]
            refs.view(nrefs, ref_len + 1)[:, ref_len] = 0
            ridx = torch.from_numpy(kmc.synth_indices(nrefs, ref_len)).to(dev)
            sk, sz = kmc.sketch_from_sequences(refs, ridx, k, s)
            del refs
            index = kmc.sketch_screen_build(sk, sz)
            kmc.sketch_screen_count(index, mix, midx, k)
            sh, med, ident = kmc.sketch_screen_results(index, sk, sz, k)
            torch.cuda.synchronize()
            assert torch.equal(sh[::2], sz[::2]) and int(sz.min()) == s, name
            # (chance hits: 10^9 windows against 2.2 x 10^12 canonical 21-mers, 0.45 expected per reference)
            assert int(sh[1::2].max()) <= 10, (name, "a reference that is not in the mixture shares", int(sh[1::2].max()))
            assert int(med[::2].min()) == 1 and float(ident[::2].min()) == 1.0, (name, int(med[::2].min()))
            ws = torch.empty(kmc.sketch_screen_winners_workspace_size(index, nrefs), dtype=torch.uint8, device=dev)
            won, wmed, wident, wall = kmc.sketch_screen_winners(index, sk, sz, k, workspace=ws)
            torch.cuda.synchronize()
            # (a chance hit is a value of the mixture record it hits, mostly one of that record's smallest: when
            # the record is a reference too, the two contest it and the contained one wins)
            assert torch.equal(wall, sh) and bool((won <= wall).all()) and int(won.sum()) == distinct_found(index, sk, k), name
            assert int((sh[::2] - won[::2]).max()) <= 10 and torch.equal(wmed[::2], med[::2]), name
            # the share of the mixture's windows at or below the largest indexed value: what the prefilter passes
            top = int(sk.max()) if int(sk.min()) >= 0 else None  # (as int64: every value below 2^63)
            rec = {
                "input": name, "refs": nrefs, "ref_len": ref_len, "mixture_records": records,
                "mixture_record_len": record_len, "k": k, "sketch_size": s, "contained_found_whole": True,
                "chance_hits_max": int(sh[1::2].max()),
                "index_bytes": int(index.numel()), "winners_workspace_bytes": int(ws.numel()),
                "prefilter_pass_fraction": None if top is None else top / 2.0 ** 64,
                "kmc_sketch_screen_build": timed(lambda: kmc.sketch_screen_build(sk, sz, index=index), args.runs),
                "kmc_sketch_screen_count": timed(lambda: kmc.sketch_screen_count(index, mix, midx, k), args.runs),
                "kmc_sketch_screen_results": timed(lambda: kmc.sketch_screen_results(index, sk, sz, k), args.runs),
                "kmc_sketch_screen_winners": timed(lambda: kmc.sketch_screen_winners(index, sk, sz, k, workspace=ws),
                                                   args.runs),
                "kmc_sketch_from_sequences_grouped": grouped,
            }
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(json.dumps(rec), flush=True)
            if name == "genomes":
                rec = screen_redundant(args, dev, sk, mix, midx, k, s)
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
            del sk, sz, index, ws
            torch.cuda.empty_cache()


def distinct_found(index, rows, k):
    """How many distinct values of the rows the index holds with a multiplicity above 0:
    the results of one-value rows.  The sum of winners' won must be this number."""
    values = torch.unique(rows.reshape(-1)).reshape(-1, 1)
    ones = torch.ones(values.shape[0], dtype=torch.int32, device=rows.device)
    found, _, _ = kmc.sketch_screen_results(index, values, ones, k, median=False, identity=False)
    return int(found.sum())


def screen_redundant(args, dev, sk, mix, midx, k, s):
    """The "genomes" rows as a redundant collection: 50 groups of 20 rows; row j of a group
    keeps its own first s / 10 values and takes the other 9 s / 10 from the group's row 0.
    Every second row is in the mixture, so in each group row 0 (all found, the smallest
    index) wins the shared values, the other rows that are in the mixture win their own
    s / 10, and the rows that are not win nothing but chance hits: asserted before timing,
    with the sum of won against the number of distinct found values."""
    n, group, own = int(sk.shape[0]), 20, s // 10
    assert n % group == 0
    rows = sk.view(n // group, group, s).clone()
    rows[:, :, own:] = rows[:, :1, own:]
    rows = rows.view(n, s).contiguous()
    sz = torch.full((n,), s, dtype=torch.int32, device=dev)
    index = kmc.sketch_screen_build(rows, sz)
    kmc.sketch_screen_count(index, mix, midx, k)
    ws = torch.empty(kmc.sketch_screen_winners_workspace_size(index, n), dtype=torch.uint8, device=dev)
    sh, _, _ = kmc.sketch_screen_results(index, rows, sz, k)
    won, _, _, wall = kmc.sketch_screen_winners(index, rows, sz, k, workspace=ws)
    torch.cuda.synchronize()
    won_g, sh_g = won.view(-1, group), sh.view(-1, group)
    assert torch.equal(wall, sh) and int(sh_g[:, ::2].min()) == s and int(sh_g[:, 1::2].min()) >= s - own
    assert bool((won <= wall).all()) and int(won.sum()) == distinct_found(index, rows, k)
    # (but for the few values that two groups hold by chance)
    assert int(won_g[:, 0].min()) >= s - 10 and int(won_g[:, 2::2].min()) >= own - 10 and int(won_g[:, 2::2].max()) == own
    assert int(won_g[:, 1::2].max()) <= 10, int(won_g[:, 1::2].max())
    return {
        "input": "genomes_redundant", "refs": n, "groups": n // group, "rows_per_group": group, "shared_fraction": 0.9,
        "k": k, "sketch_size": s, "index_bytes": int(index.numel()), "winners_workspace_bytes": int(ws.numel()),
        "won_sum": int(won.sum()), "shared_sum": int(sh.sum()),
        "kmc_sketch_screen_results": timed(lambda: kmc.sketch_screen_results(index, rows, sz, k), args.runs),
        "kmc_sketch_screen_winners": timed(lambda: kmc.sketch_screen_winners(index, rows, sz, k, workspace=ws), args.runs),
    }


def accum_main(args, dev):
    """--accum: the abundance accumulator on the --screen mode's mixture, in this process.
    The yardsticks are the screen count (walk, hash and prefilter only) and the grouped
    sketch of one group (walk plus LDS set upkeep) on the same buffer.  Every timed add
    starts from a reset accumulator (reset is timed alone too); the row of the one-call
    and of the 16-call pass are asserted equal to the grouped sketch before anything is
    timed (m = 1; what m = 2 keeps, the chance repeats among 10^9 random windows that lie
    below the threshold, is recorded)."""
    k, s, records, calls = 21, 1000, 1000, 16
    record_len = max(int(1_000_000 * args.scale), 5000)
    mix = torch.empty(records * (record_len + 1), dtype=torch.uint8, device=dev)
    kmc.synth_fill(mix, records, record_len, 0x5EED0008)
    midx = torch.from_numpy(kmc.synth_indices(records, record_len)).to(dev)
    one_group = torch.tensor([0, records], dtype=torch.int64, device=dev)
    # the screen mode's "genomes" index
    refs = torch.empty(records * (record_len + 1), dtype=torch.uint8, device=dev)
    kmc.synth_fill(refs, records, record_len, 0x5EED0009)
    refs.view(records, record_len + 1)[::2] = mix.view(records, record_len + 1)[::2]
    sk, sz = kmc.sketch_from_sequences(refs, midx, k, s)
    del refs
    index = kmc.sketch_screen_build(sk, sz)
    # the 16 calls: consecutive records, offsets from each piece's first byte
    cuts = [records * c // calls for c in range(calls + 1)]
    pieces = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = a * (record_len + 1), b * (record_len + 1)
        pieces.append((mix[lo:hi], (midx[a:b + 1] - lo).contiguous()))
    lg = max((4096 * s - 1).bit_length(), kmc.SKETCH_ACCUM_MIN_LOG2_SLOTS)  # the default table (kmc.h)
    levels, n = [], 0
    for d, _ in pieces:
        n += int(d.numel())
        levels.append(next(j for j in range(64) if -(-n // (1 << j)) <= (1 << lg) // 4))
    acc = kmc.SketchAccum(s, k)

    def whole():
        acc.reset()
        acc.add(mix, midx)

    def in_calls():
        acc.reset()
        for d, i in pieces:
            acc.add(d, i)

    grp = kmc.sketch_from_sequences_grouped(mix, midx, one_group, k, s)
    stats = {}
    for name, fn in (("one_call", whole), ("16_calls", in_calls)):
        fn()
        row, size, st = acc.finish(1)
        none = acc.finish(2, stats=False)
        torch.cuda.synchronize()
        assert torch.equal(row, grp[0][0]) and int(size[0]) == int(grp[1][0]) == s and int(st[0]) == 1, name
        stats[name] = [int(x) for x in st.cpu().numpy().view(np.uint64)] + [int(none[1][0])]
    rec = {
        "mixture_records": records, "mixture_record_len": record_len, "k": k, "sketch_size": s,
        "log2_slots": lg, "device_bytes": kmc.sketch_accum_device_bytes(s), "calls": calls,
        "levels_of_the_16_calls": levels, "final_j": levels[-1], "rows_equal_grouped": True,
        # complete, limit, tracked, qualifying at m = 1; then the size of the m = 2 row
        "stats_one_call": stats["one_call"], "stats_16_calls": stats["16_calls"],
        "kmc_sketch_accum_reset": timed(lambda: acc.reset(), args.runs),
        "reset_and_add_one_call": timed(whole, args.runs),
        "reset_and_add_16_calls": timed(in_calls, args.runs),
        "kmc_sketch_accum_finish": timed(lambda: acc.finish(2), args.runs),
        # the spectrum of the same table (the state the 16 calls left), 256 and 8192 bins
        "kmc_spectrum_from_accum_256": timed(lambda: acc.spectrum(256), args.runs),
        "kmc_spectrum_from_accum_8192": timed(lambda: acc.spectrum(8192), args.runs),
        "kmc_sketch_screen_count": timed(lambda: kmc.sketch_screen_count(index, mix, midx, k), args.runs),
        "kmc_sketch_from_sequences_grouped": timed(
            lambda: kmc.sketch_from_sequences_grouped(mix, midx, one_group, k, s), args.runs),
    }
    acc.close()
    with open(args.out, "a") as out:
        out.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def match_main(args, dev):
    """--match: kmc_match_from_accum on a read set (2.6 M records of 150 bases) and on long
    records (8 x 50 Mbase), k = 21, against a table of 2^26 slots filled from 100 Mbase;
    half of each input is drawn from what was added, half is unrelated.  Beside it, in this
    process, the piece-per-workgroup walks on the same bytes: kmc_sketch_accum_add (into a
    second accumulator, reset before every add; reset is timed alone and subtracted) and
    kmc_sketch_screen_count against the index of the set's sketch.  The outputs of a call
    are asserted equal to a second call's before anything is timed; HIP events, 2 warm-ups,
    median of 5."""
    k, lg, runs = 21, 26, 5
    set_len = max(int(50_000_000 * args.scale), 5000)
    sdata = torch.empty(2 * (set_len + 1), dtype=torch.uint8, device=dev)
    kmc.synth_fill(sdata, 2, set_len, 0x5EED0008)
    sidx = torch.from_numpy(kmc.synth_indices(2, set_len)).to(dev)
    acc, other = kmc.SketchAccum(1, k, log2_slots=lg), kmc.SketchAccum(1, k, log2_slots=lg)
    acc.add(sdata, sidx)
    sk, sz = kmc.sketch_from_sequences(sdata, sidx, k, 1000)
    index = kmc.sketch_screen_build(sk, sz)

    def reads():
        n, ln = max(int(2_600_000 * args.scale), 64), 150
        d = torch.empty(n * (ln + 1), dtype=torch.uint8, device=dev)
        kmc.synth_fill(d, n, ln, 0x5EED0010)
        step = max((sdata.numel() - ln) // (n // 2 + 1), 1)
        d.view(n, ln + 1)[::2, :ln] = sdata.unfold(0, ln, step)[:(n + 1) // 2]  # pieces of the set, every `step` bytes
        return d, torch.from_numpy(kmc.synth_indices(n, ln)).to(dev), n, ln

    def long_records():
        n, ln = 8, set_len
        d = torch.empty(n * (ln + 1), dtype=torch.uint8, device=dev)
        kmc.synth_fill(d, n, ln, 0x5EED0011)
        d.view(n, ln + 1)[::2] = sdata.view(2, ln + 1).repeat(2, 1)
        return d, torch.from_numpy(kmc.synth_indices(n, ln)).to(dev), n, ln

    with open(args.out, "a") as out:
        for name, make in (("read_set", reads), ("long_records", long_records)):
            d, i, n, ln = make()
            one, two = acc.match(d, i), acc.match(d, i)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(one, two)), name
            win, smp, hit, st = one
            st = [int(x) for x in st.cpu().numpy().view(np.uint64)]
            # (a read cut over the end of one of the set's records holds its terminator and loses windows)
            assert n * (ln - k + 1) - 2 * ln <= int(win.long().sum()) <= n * (ln - k + 1)
            assert st[2] == int(smp.long().sum()) and st[3] == int(hit.long().sum())
            frac = (hit[::2].long().sum().item() / max(smp[::2].long().sum().item(), 1),
                    hit[1::2].long().sum().item() / max(smp[1::2].long().sum().item(), 1))
            assert frac[0] > 0.98 and frac[1] < 0.01, (name, frac)  # (a piece over the set's record end loses windows)

            def reset_and_add():
                other.reset()
                other.add(d, i)
            rec = {
                "input": name, "records": n, "record_len": ln, "k": k, "log2_slots": lg, "set_bases": 2 * set_len,
                "stats": st, "hit_fraction_drawn": frac[0], "hit_fraction_unrelated": frac[1],
                "outputs_equal_second_call": True,
                "kmc_match_from_accum": timed(lambda: acc.match(d, i), runs),
                "kmc_match_from_accum_hits_only": timed(
                    lambda: acc.match(d, i, windows=False, sampled=False, stats=False), runs),
                "reset_and_add": timed(reset_and_add, runs),
                "kmc_sketch_accum_reset": timed(lambda: other.reset(), runs),
                "kmc_sketch_screen_count": timed(lambda: kmc.sketch_screen_count(index, d, i, k), runs),
            }
            add_ms = rec["reset_and_add"]["ms_median"] - rec["kmc_sketch_accum_reset"]["ms_median"]
            rec["kmc_sketch_accum_add_ms"] = add_ms
            rec["match_over_screen_count"] = rec["kmc_match_from_accum"]["ms_median"] / \
                rec["kmc_sketch_screen_count"]["ms_median"]
            rec["match_over_add"] = rec["kmc_match_from_accum"]["ms_median"] / add_ms
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(json.dumps(rec), flush=True)
            del d, i, one, two, win, smp, hit
            torch.cuda.empty_cache()
    acc.close()
    other.close()


def classify_main(args, dev):
    """--classify: kmc_classify_from_accum beside kmc_match_from_accum on --match's two
    workloads (2.6 M reads of 150 bases, 8 x 50 Mbase; k = 21, a table of 2^26 slots filled
    from 100 Mbase, half of each input drawn from it), with 2, 8 and 32 sources, each with
    and without `scores`; the set is cut into as many equal pieces as there are sources and
    piece g labelled g, so a hit window votes for one source.  And kmc_label_accum
    of the whole set as one source beside kmc_sketch_accum_add of it (reset timed alone and
    subtracted).  windows, sampled, hits and stats are asserted equal to the match's, the
    votes with and without scores to each other and best_hits to the scores' largest,
    before anything is timed; HIP events, 2 warm-ups, median of 7."""
    k, lg, runs = 21, 26, 7
    set_len = max(int(50_000_000 * args.scale), 5000)
    sdata = torch.empty(2 * (set_len + 1), dtype=torch.uint8, device=dev)
    kmc.synth_fill(sdata, 2, set_len, 0x5EED0008)
    sidx = torch.from_numpy(kmc.synth_indices(2, set_len)).to(dev)
    acc, other = kmc.SketchAccum(1, k, log2_slots=lg), kmc.SketchAccum(1, k, log2_slots=lg)
    acc.add(sdata, sidx)

    def label_pieces(ns):
        """piece g of the set's bytes is source g (a record's terminator ends a window)"""
        cuts = np.linspace(0, sdata.numel(), ns + 1).astype(np.int64)
        acc.reset()
        acc.add(sdata, sidx)
        for g in range(ns):
            acc.label(sdata, torch.from_numpy(cuts[g:g + 2].copy()).to(dev), g)

    def reads():
        n, ln = max(int(2_600_000 * args.scale), 64), 150
        d = torch.empty(n * (ln + 1), dtype=torch.uint8, device=dev)
        kmc.synth_fill(d, n, ln, 0x5EED0010)
        step = max((sdata.numel() - ln) // (n // 2 + 1), 1)
        d.view(n, ln + 1)[::2, :ln] = sdata.unfold(0, ln, step)[:(n + 1) // 2]
        return d, torch.from_numpy(kmc.synth_indices(n, ln)).to(dev), n, ln

    def long_records():
        n, ln = 8, set_len
        d = torch.empty(n * (ln + 1), dtype=torch.uint8, device=dev)
        kmc.synth_fill(d, n, ln, 0x5EED0011)
        d.view(n, ln + 1)[::2] = sdata.view(2, ln + 1).repeat(2, 1)
        return d, torch.from_numpy(kmc.synth_indices(n, ln)).to(dev), n, ln

    def reset_and_add():
        other.reset()
        other.add(sdata, sidx)
    other.reset()
    other.add(sdata, sidx)
    turn = [0]

    def label_next():  # a new source every call: every key's word takes the atomic OR
        other.label(sdata, sidx, turn[0] % 32)
        turn[0] += 1
    label = {"set_bases": 2 * set_len, "k": k, "log2_slots": lg,
             "kmc_label_accum": timed(label_next, runs),
             "reset_and_add": timed(reset_and_add, runs),
             "kmc_sketch_accum_reset": timed(lambda: other.reset(), runs)}
    label["kmc_sketch_accum_add_ms"] = label["reset_and_add"]["ms_median"] - label["kmc_sketch_accum_reset"]["ms_median"]
    label["label_over_add"] = label["kmc_label_accum"]["ms_median"] / label["kmc_sketch_accum_add_ms"]
    with open(args.out, "a") as out:
        out.write(json.dumps(label) + "\n")
        print(json.dumps(label), flush=True)
        for name, make in (("read_set", reads), ("long_records", long_records)):
            d, i, n, ln = make()
            ws = torch.empty(kmc.classify_workspace_size(n, d.numel(), 32, torch.cuda.current_device()),
                             dtype=torch.uint8, device=dev)
            plain = acc.match(d, i)
            match_ms = timed(lambda: acc.match(d, i), runs)
            for ns in (2, 8, 32):
                label_pieces(ns)
                full = acc.classify(d, i, ns, scores=True, workspace=ws)
                bare = acc.classify(d, i, ns, workspace=ws)
                torch.cuda.synchronize()
                assert all(torch.equal(a, b) for a, b in zip(full[:3] + (full[7],), plain)), (name, ns)
                assert all(torch.equal(a, b) for a, b in zip(full[:6], bare[:6])), (name, ns)
                assert torch.equal(full[6].max(dim=1).values, full[4]), (name, ns)
                # (a k-mer over a cut has no label, one that two pieces hold has two: a few in 10^8)
                votes, hits = int(full[6][::2].long().sum().item()), int(full[2][::2].long().sum().item())
                assert abs(votes - hits) <= 0.01 * hits, (name, ns, votes, hits)
                rec = {
                    "input": name, "records": n, "record_len": ln, "k": k, "log2_slots": lg, "set_bases": 2 * set_len,
                    "num_sources": ns, "workspace_bytes": ws.numel(), "outputs_equal_match": True,
                    "assigned": int((full[4] > full[5]).sum().item()),
                    "kmc_match_from_accum": match_ms,
                    "kmc_classify_from_accum": timed(lambda: acc.classify(d, i, ns, workspace=ws), runs),
                    "kmc_classify_from_accum_scores": timed(lambda: acc.classify(d, i, ns, scores=True, workspace=ws), runs),
                }
                rec["classify_over_match"] = rec["kmc_classify_from_accum"]["ms_median"] / match_ms["ms_median"]
                rec["classify_scores_over_match"] = rec["kmc_classify_from_accum_scores"]["ms_median"] / match_ms["ms_median"]
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
                del full, bare
            del d, i, plain, ws
            torch.cuda.empty_cache()
    acc.close()
    other.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "pr_sketch.jsonl"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--inputs", default="iid,copies_1pct,many")
    ap.add_argument("--sizes", default="1000,10000")
    ap.add_argument("--scale", type=float, default=1.0, help="scales the record lengths (a quick rehearsal: 0.01)")
    ap.add_argument("--direct", action="store_true",
                    help="time kmc_sketch_from_sequences beside kmc_count_canonical_hash + kmc_sketch_from_counts "
                         "(rows asserted equal) and on all_a; --out profiles/pr_sketch_direct.jsonl")
    ap.add_argument("--grouped", action="store_true",
                    help="time kmc_sketch_from_sequences_grouped beside kmc_sketch_from_sequences (+ "
                         "kmc_sketch_merge_groups) on identity, draft_assembly and read_set (--inputs picks among "
                         "them; rows asserted equal; 2 warm-ups, median of 5); appends to "
                         "--out profiles/pr_sketch_grouped.jsonl")
    ap.add_argument("--query", action="store_true",
                    help="time kmc_sketch_nearest and kmc_sketch_distances_rect beside kmc_sketch_distances over "
                         "queries and references together: 64 queries in 4096 and 65536 references of s = 1000 and "
                         "in 4096 of s = 10000, synthetic rows (hits asserted equal to the rectangle's; 2 warm-ups, "
                         "median of --runs); --out profiles/pr_sketch_query.jsonl")
    ap.add_argument("--screen", action="store_true",
                    help="time kmc_sketch_screen_build, _count and _results of 1000 references of 1 Mbase and of "
                         "100 of 5 kbase (s = 1000, k = 21, half of them cut from the mixture: asserted found "
                         "whole) in a synthetic mixture of 1000 x 1 Mbase, beside kmc_sketch_from_sequences_grouped "
                         "over the mixture as one group (2 warm-ups, median of --runs); appends to "
                         "--out profiles/pr_sketch_screen.jsonl; kmc_sketch_screen_winners beside _results, also on a "
                         "redundant collection: --out profiles/pr_screen_winners.jsonl")
    ap.add_argument("--accum", action="store_true",
                    help="time kmc_sketch_accum_add of the --screen mixture (1000 x 1 Mbase, s = 1000, k = 21) as one "
                         "call and as 16 calls, and kmc_sketch_accum_finish, beside kmc_sketch_screen_count against "
                         "the 1000-reference index and kmc_sketch_from_sequences_grouped with one group (rows "
                         "asserted equal; 2 warm-ups, median of --runs); appends to --out "
                         "profiles/pr_sketch_accum.jsonl")
    ap.add_argument("--cluster", action="store_true",
                    help="time kmc_sketch_cluster beside kmc_sketch_distances on the same rows: 4096 and 65536 rows "
                         "of s = 1000, unrelated and in 64-member clusters of near-identical rows (labels asserted; "
                         "1 warm-up, median of --runs, of at least 5 at 65536 rows); --out "
                         "profiles/pr_sketch_cluster.jsonl")
    ap.add_argument("--links", action="store_true",
                    help="time kmc_sketch_links, count-only and with a fitting capacity, beside kmc_sketch_distances "
                         "with counts (where the triangle fits) and kmc_sketch_cluster on the rows of --cluster (the "
                         "list asserted; 1 warm-up, median of --runs, of a third of them and at least 3 at 65536 "
                         "rows); --out profiles/pr_sketch_links.jsonl")
    ap.add_argument("--match", action="store_true",
                    help="time kmc_match_from_accum on 2.6 M reads of 150 bases and on 8 x 50 Mbase (k = 21, half of "
                         "each drawn from the set) against a table of 2^26 slots filled from 100 Mbase, beside "
                         "kmc_sketch_accum_add and kmc_sketch_screen_count on the same records (outputs asserted equal "
                         "to a second call's; 2 warm-ups, median of 5); appends to --out "
                         "profiles/pr_accum_match.jsonl")
    ap.add_argument("--classify", action="store_true",
                    help="time kmc_classify_from_accum with 2, 8 and 32 sources, with and without scores, beside "
                         "kmc_match_from_accum on --match's two workloads, and kmc_label_accum beside "
                         "kmc_sketch_accum_add (outputs asserted equal to the match's; 2 warm-ups, median of 7); "
                         "appends to --out profiles/pr_classify.jsonl")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.classify:
        return classify_main(args, dev)
    if args.match:
        return match_main(args, dev)
    if args.links:
        return links_main(args, dev)
    if args.cluster:
        return cluster_main(args, dev)
    if args.accum:
        return accum_main(args, dev)
    if args.screen:
        return screen_main(args, dev)
    if args.query:
        return query_main(args, dev)
    if args.grouped:
        return grouped_main(args, dev)
    shapes = {"iid": (8, 50_000_000, 31), "copies_1pct": (8, 50_000_000, 31), "many": (4096, 100_000, 21)}
    if args.direct:
        return direct_main(args, dev, shapes)
    with open(args.out, "w") as out:
        for name in args.inputs.split(","):
            records, record_len, k = shapes[name]
            record_len = max(int(record_len * args.scale), k + 1)
            data, idx = make_input(name, records, record_len, dev)
            keys, counts, off = kmc.count_canonical(data, idx, k)
            torch.cuda.synchronize()
            del data
            exact = timed(lambda: kmc.pair_distances_sparse(keys, counts, off, idx, k), args.runs)
            exact_d = kmc.pair_distances_sparse(keys, counts, off, idx, k)[:7].cpu().tolist()
            for s in (int(x) for x in args.sizes.split(",")):
                sk, sz = kmc.sketch_from_counts(keys, counts, off, s)
                # 8.4e6 pairs at s = 10000 run from global memory for about a second: fewer runs
                druns = 3 if records > 1000 and s > 2048 else args.runs
                rec = {
                    "input": name, "records": records, "record_len": record_len, "k": k, "sketch_size": s,
                    "entries": int(keys.numel()), "digit_bits": 8,
                    "workspace_bytes": kmc.sketch_workspace_size(records, keys.numel(), s),
                    "kmc_sketch_from_counts": timed(lambda: kmc.sketch_from_counts(keys, counts, off, s), args.runs),
                    "kmc_sketch_distances": timed(lambda: kmc.sketch_distances(sk, sz, k), druns, warmup=1),
                    "kmc_pair_distances_sparse": exact,
                    "exact_dist_first7": exact_d,
                }
                d, sh, dn = kmc.sketch_distances(sk, sz, k, with_counts=True)
                torch.cuda.synchronize()
                rec["mash_dist_first7"] = d[:7].cpu().tolist()
                rec["shared_first7"] = sh[:7].cpu().tolist()
                rec["denom_first7"] = dn[:7].cpu().tolist()
                if name == "copies_1pct":
                    rec["substitution_rate"] = 0.01
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(json.dumps(rec), flush=True)
            del keys, counts, off
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
