"""GPU parity of kmc_sketch_cluster against the numpy oracle of
tests/sketch_cluster_util.py: labels, cluster_index and num_clusters are compared
exactly.  Every case runs in libkmc.so and in libkmc_diag.so, whose distance tiles
(512 staged values, at most 4 rows) put a few records through many tiles:

    build  s     path                n
    diag   64    staged, T = 4       3, 4, 5, 11, 37
    diag   128   rows in global      10
    ship   64    staged, T = 32      31, 32, 33, 67, 70
    ship   4096  rows in global      10

Rows are built directly (sorted random uint64 with planted overlaps), and the record
order is permuted so that a cluster's smallest index is not where its linking starts.
"""
import os
import subprocess

import numpy as np
import pytest

import sketch_cluster_util as C
import sketch_query_util as Q
import sketch_util as S
import stream_util as T
from sketch_util import dev, which

pytestmark = pytest.mark.gpu

LIBS = ["ship", "diag"]
cached = S.cache()
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMC = os.environ.get("KMC_BIN") or os.path.join(REPO, "dna-kmeres-parallel_amd", "bin", "kmc")

SHAPES = [("diag", 64, n) for n in (3, 4, 5, 11, 37)] + [("diag", 128, 10)] + \
         [("ship", 64, n) for n in (31, 32, 33, 67, 70)] + [("ship", 4096, 10)]
TILE = {("diag", 64): 4, ("diag", 128): 4, ("ship", 64): 32, ("ship", 4096): 8}


def dev_rows(rows, sizes, cuda):
    return dev(rows.view(np.int64), cuda), dev(sizes.view(np.int32), cuda)


def u32(t):
    return None if t is None else t.cpu().numpy().view(np.uint32)


def gpu_cluster(kmc, cuda, rows, sizes, min_jaccard, **kw):
    import torch
    labels, index, count = kmc.sketch_cluster(*dev_rows(rows, sizes, cuda), min_jaccard, **kw)
    torch.cuda.synchronize()
    return u32(labels), u32(index), u32(count)


def assert_cluster(got, exp, msg):
    labels, index, count = got
    np.testing.assert_array_equal(labels, exp[0], err_msg="%s labels" % msg)
    np.testing.assert_array_equal(index, exp[1], err_msg="%s cluster_index" % msg)
    assert count.tolist() == [exp[2]], "%s num_clusters" % msg


def linked_pairs(rows, sizes, s, min_jaccard):
    """[(i, j)] of the oracle's linked pairs."""
    sh, dn = C.pair_counts_packed(rows, sizes, s)
    i, j = C.triangle_pairs(rows.shape[0])
    on = C.links(sh, dn, min_jaccard, sizes[i], sizes[j])
    return list(zip(i[on].tolist(), j[on].tolist()))


# 1. structures x shapes ------------------------------------------------------------------
def order_with(rng, n, fixed):
    """A permutation of 0..n-1 (chain position -> record) with order[t] = r for (t, r) in fixed."""
    rest = [r for r in rng.permutation(n).tolist() if r not in fixed.values()]
    return [fixed[t] if t in fixed else rest.pop() for t in range(n)]


def chain(rng, vals, n, s):
    """Only neighbours share values (half a row), so transitivity alone joins the ends;
    record 0 is the middle of the chain, its neighbours are spread over the tiles."""
    order = order_with(rng, n, {n // 2: 0})
    rows, sizes = C.place(C.chain_lists(vals, n, s, s // 2), order, n, s)
    pairs = linked_pairs(rows, sizes, s, 0.1)
    assert sorted(pairs) == sorted((min(a, b), max(a, b)) for a, b in zip(order, order[1:]))
    return rows, sizes, 0.1, lambda e: e[2] == 1 and not e[0].any()


def star(rng, vals, n, s):
    """Every leaf holds an eighth of the centre's values and nothing else: shared = s / 8
    of denom = s, the rule's boundary at 0.125 (exact in double).  The centre is the last
    record."""
    centre = vals.take(s)
    lists = [centre] + [rng.choice(centre, size=s // 8, replace=False) for _ in range(n - 1)]
    rows, sizes = C.place(lists, [n - 1] + list(range(n - 1)), n, s)
    return rows, sizes, 0.125, lambda e: e[2] == 1 and not e[0].any()


def bridge(rng, vals, n, s):
    """Two chains joined by the one pair (n - 2, n - 1), the last pair of the last tile."""
    order = order_with(rng, n, {n // 2 - 1: n - 2, n // 2: n - 1})
    rows, sizes = C.place(C.chain_lists(vals, n, s, s // 2), order, n, s)
    pairs = linked_pairs(rows, sizes, s, 0.1)
    assert (n - 2, n - 1) in pairs and len(pairs) == n - 1
    assert C.components(n, [p for p in pairs if p != (n - 2, n - 1)])[2] == 2
    return rows, sizes, 0.1, lambda e: e[2] == 1


def singletons(rng, vals, n, s):
    lists = [vals.take(int(rng.integers(1, s + 1))) for _ in range(n)]
    rows, sizes = Q.pack(lists, s)
    return rows, sizes, 1.0 / 16384, lambda e: e[2] == n and e[0].tolist() == list(range(n))


def identical(rng, vals, n, s):
    rows, sizes = Q.pack([vals.take(s)] * n, s)
    return rows, sizes, 1.0, lambda e: e[2] == 1 and not e[0].any()


def empties(rng, vals, n, s):
    """min_jaccard = 0 links every pair of rows that are not empty, whatever they share: they
    are one cluster; an empty row (the first and the last record among them) is a singleton
    even here, where its shared 0 of denom > 0 would pass the product rule."""
    pool = vals.take(2 * s)
    empty = {0, n - 1} if n > 3 else {0}
    lists = [[] if r in empty else rng.choice(pool, size=int(rng.integers(1, s + 1)), replace=False) for r in range(n)]
    rows, sizes = Q.pack(lists, s)
    return rows, sizes, 0.0, lambda e: e[2] == len(empty) + 1 and \
        e[0].tolist() == [r if r in empty else 1 for r in range(n)]


def exact(rng, vals, n, s):
    """min_jaccard = 1 links only shared == denom: copies of a full row and copies of a
    short row are clusters; a copy with one value replaced is not in them."""
    g = max(1, n // 3)
    bases = [vals.take(s if b % 2 == 0 else s // 2) for b in range(g)]
    lists = []
    for r in range(n):
        v = bases[r % g].copy()
        if r // g == 2:
            v[int(rng.integers(0, v.size))] = vals.take(1)[0]
        lists.append(v)
    order = rng.permutation(n).tolist()
    rows, sizes = C.place(lists, order, n, s)
    near = sum(1 for r in range(n) if r // g == 2)
    return rows, sizes, 1.0, lambda e: e[2] == g + near


STRUCTURES = {"chain": chain, "star": star, "bridge": bridge, "singletons": singletons, "identical": identical,
              "empties": empties, "exact": exact}


def structure_case(name, n, s):
    def make():
        seed = 1000 * n + s + 7 * list(STRUCTURES).index(name)
        rng = np.random.default_rng(seed)
        rows, sizes, mj, holds = STRUCTURES[name](rng, C.Values(seed + 1, (n + 2) * s + n), n, s)
        exp = C.cluster_expected(rows, sizes, s, mj)
        assert holds(exp), "%s n=%d s=%d: the oracle's clusters are not the planted ones" % (name, n, s)
        return rows, sizes, mj, exp
    return cached((name, n, s), make)


@pytest.mark.parametrize("name", list(STRUCTURES))
@pytest.mark.parametrize("lib,s,n", SHAPES)
def test_structures(kmc, cuda, lib, s, n, name):
    rows, sizes, mj, exp = structure_case(name, n, s)
    assert n > 2 * TILE[(lib, s)] or n in (TILE[(lib, s)] - 1, TILE[(lib, s)], TILE[(lib, s)] + 1, 10)
    with which(kmc, lib):
        assert_cluster(gpu_cluster(kmc, cuda, rows, sizes, mj), exp, "%s %s n=%d s=%d" % (name, lib, n, s))


# 2. the rule's boundary ----------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_boundary_of_the_rule(kmc, cuda, lib):
    """Rows 1 and 3 hold 64 values each and share the 32 smallest; the 64 smallest of
    their union are row 1: shared 32 of denom 64.  0.5 * 64 == 32 links them; the next
    double above 0.5 does not."""
    s = 64
    v = np.sort(C.Values(11, 4 * s).take(4 * s))
    lists = [v[2 * s:3 * s], v[:s], v[3 * s:4 * s], np.concatenate([v[:32], v[s:s + 32]])]
    rows, sizes = Q.pack(lists, s)
    sh, dn = C.pair_counts_packed(rows, sizes, s)
    assert (sh[4], dn[4]) == (32, 64) and sh.sum() == 32  # pair (1, 3) of the packed triangle
    above = float(np.nextafter(0.5, 1))
    with which(kmc, lib):
        for mj, labels in ((0.5, [0, 1, 2, 1]), (above, [0, 1, 2, 3])):
            exp = C.cluster_expected(rows, sizes, s, mj)
            assert exp[0].tolist() == labels
            assert_cluster(gpu_cluster(kmc, cuda, rows, sizes, mj), exp, "min_jaccard=%r" % mj)


# 3. a random graph near its percolation point ----------------------------------------------
def percolation_case(seed):
    def make():
        n, s, block = 300, 16, 4
        rng = np.random.default_rng(50 + seed)
        vals = C.Values(60 + seed, n * s + 200 * block)
        lists = [[] for _ in range(n)]
        for _ in range(160):  # a mean degree near 1
            i, j = rng.choice(n, size=2, replace=False)
            if len(lists[i]) + block <= s and len(lists[j]) + block <= s:
                v = vals.take(block).tolist()
                lists[i] += v
                lists[j] += v
        lists = [v + vals.take(s - len(v)).tolist() for v in lists]
        rows, sizes = Q.pack(lists, s)
        exp = C.cluster_expected(rows, sizes, s, 1.0 / s)
        return rows, sizes, 1.0 / s, exp
    return cached(("percolation", seed), make)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_graph_near_percolation(kmc, cuda, seed):
    """n = 300, s = 16, links planted as blocks of 4 values from a shared pool, linked at
    one shared value among the 16 smallest of the union: trees of many sizes, whose
    unions meet in every order."""
    rows, sizes, mj, exp = percolation_case(seed)
    biggest = np.bincount(exp[0]).max()
    print("seed %d: %d clusters, the largest of %d" % (seed, exp[2], biggest))
    assert 100 < exp[2] < 290 and biggest >= 5
    assert_cluster(gpu_cluster(kmc, cuda, rows, sizes, mj), exp, "seed %d" % seed)


# 4. the same linked set as the triangle --------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_links_are_the_triangles(kmc, cuda, lib):
    """The pairs of kmc_sketch_distances(with_counts=True) that pass the rule on the host,
    through the oracle's union-find, give the device's labels."""
    import torch
    n, s, mj = 37, 64, 0.3
    rows, sizes = T.overlap_rows(4100, n, s)
    d_rows, d_sizes = dev_rows(rows, sizes, cuda)
    with which(kmc, lib):
        _, sh, dn = kmc.sketch_distances(d_rows, d_sizes, 21, with_counts=True)
        labels, index, count = kmc.sketch_cluster(d_rows, d_sizes, mj)
        torch.cuda.synchronize()
    exp = C.cluster_from_counts(sizes, u32(sh), u32(dn), mj)
    assert 1 < exp[2] < n - 1
    assert_cluster((u32(labels), u32(index), u32(count)), exp, lib)
    assert_cluster((u32(labels), u32(index), u32(count)), C.cluster_expected(rows, sizes, s, mj), lib + " oracle")


# 5. the workspace ----------------------------------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_caller_workspace(kmc, cuda, lib):
    import torch
    rows, sizes, mj, exp = structure_case("bridge", 37 if lib == "diag" else 70, 64)
    n = rows.shape[0]
    d = dev_rows(rows, sizes, cuda)
    with which(kmc, lib):
        need = kmc.sketch_cluster_workspace_size(n, cuda.index or 0)
        assert need >= 4 * 256
        own = kmc.sketch_cluster(*d, mj)
        torch.cuda.synchronize()
        assert_cluster(tuple(u32(x) for x in own), exp, "library workspace")
        ws = torch.empty(need + 8, dtype=torch.uint8, device=cuda)
        for _ in range(2):  # the second call finds the first one's state in the workspace
            ws.fill_(0xFF)
            got = kmc.sketch_cluster(*d, mj, workspace=ws[:need])
            torch.cuda.synchronize()
            assert_cluster(tuple(u32(x) for x in got), exp, "caller workspace")
        with pytest.raises(kmc.KmcError) as ei:
            kmc.sketch_cluster(*d, mj, workspace=ws[:need - 1])
        assert ei.value.code == 1004
        with pytest.raises(kmc.KmcError) as ei:
            kmc.sketch_cluster(*d, mj, workspace=ws[1:need + 1])
        assert ei.value.code == 1003


# 6. the optional outputs, one record, no record -------------------------------------------------
@pytest.mark.parametrize("lib", LIBS)
def test_optional_outputs(kmc, cuda, lib):
    import torch
    rows, sizes, mj, exp = structure_case("exact", 11 if lib == "diag" else 33, 64)
    n = rows.shape[0]
    d = dev_rows(rows, sizes, cuda)

    def outs(index, count):
        return (torch.full((n,), -1, dtype=torch.int32, device=cuda),
                torch.full((n,), -1, dtype=torch.int32, device=cuda) if index else None,
                torch.full((1,), -1, dtype=torch.int32, device=cuda) if count else None)

    with which(kmc, lib):
        for index, count in ((False, True), (True, False), (False, False)):
            labels, idx, cnt = kmc.sketch_cluster(*d, mj, out=outs(index, count))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(u32(labels), exp[0])
            if index:
                np.testing.assert_array_equal(u32(idx), exp[1])
            if count:
                assert u32(cnt).tolist() == [exp[2]]
        labels, idx, cnt = kmc.sketch_cluster(*d, mj, index=False)
        torch.cuda.synchronize()
        assert idx is None and cnt is None
        np.testing.assert_array_equal(u32(labels), exp[0])
        # one record, empty or not, at either end of the range
        for row in (0, int(np.argmax(sizes))):
            for j in (0.0, 1.0):
                got = gpu_cluster(kmc, cuda, rows[row:row + 1], sizes[row:row + 1] * 0 if row == 0 else sizes[row:row + 1], j)
                assert [x.tolist() for x in got] == [[0], [0], [1]]
        # no record: the count alone is written
        none = (torch.empty((0, 64), dtype=torch.int64, device=cuda), torch.empty(0, dtype=torch.int32, device=cuda))
        labels, idx, cnt = kmc.sketch_cluster(*none, 0.5)
        torch.cuda.synchronize()
        assert labels.numel() == 0 and idx.numel() == 0 and cnt.tolist() == [0]
        assert kmc.sketch_cluster_workspace_size(0) == 0


# 7. a side stream -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delay(kmc, cuda):
    kmc.lib()
    cycles, ms = T.sleep_cycles(T.DELAY_MS)
    assert ms >= 0.9 * T.DELAY_MS, "the delay spins %.1f ms, not %.1f" % (ms, T.DELAY_MS)
    return cycles


@pytest.fixture(scope="module")
def streams(kmc, cuda, delay):
    return T.side_streams(kmc, cuda, delay)


@pytest.mark.parametrize("lib", LIBS)
def test_side_stream_gives_the_null_streams_result(kmc, cuda, lib, delay, streams):
    """stream_util's late-input call: the rows arrive on the side stream behind a delay,
    the workspace is refilled and the outputs poisoned there; the call returns while the
    delay spins and the snapshot taken on that stream is the real rows' result, the one
    the null stream's call gives."""
    import torch
    n, s, mj = 12, 64, 0.25
    P = [T.overlap_rows(4200 + w, n, s) for w in (0, 1)]
    rows = [dev(p[0].view(np.int64), cuda) for p in P]
    sizes = [dev(p[1].view(np.int32), cuda) for p in P]
    live = [(rows[0].clone(), rows[0], rows[1]), (sizes[0].clone(), sizes[0], sizes[1])]
    exp = {w: C.cluster_expected(*P[i], s, mj) for i, w in enumerate(("decoy", "real"))}
    outs = [torch.empty(n, dtype=torch.int32, device=cuda), torch.empty(n, dtype=torch.int32, device=cuda),
            torch.empty(1, dtype=torch.int32, device=cuda)]

    def check(got, e, msg):
        assert_cluster(tuple(np.ascontiguousarray(g).view(np.uint32) for g in got), e, msg)

    with which(kmc, lib):
        ws = torch.empty(kmc.sketch_cluster_workspace_size(n, cuda.index or 0), dtype=torch.uint8, device=cuda)
        null = gpu_cluster(kmc, cuda, *P[1], mj)
        assert_cluster(null, exp["real"], "null stream")
        call = T.Call("sketch_cluster", live, outs,
                      lambda w, st: kmc.sketch_cluster(live[0][0], live[1][0], mj, workspace=ws, out=outs, stream=st) and None,
                      exp, check, lambda e: (e[0], e[1], np.array([e[2]])), ws=ws)
        T.late_call(call, streams[0], delay)


# 8. the driver ----------------------------------------------------------------------------------
def run(args):
    return subprocess.run([KMC] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def mutated(rng, rec, rate):
    out = rec.copy()
    hit = rng.random(rec.size) < rate
    out[hit] = (np.searchsorted(np.frombuffer(b"ACGT", np.uint8), out[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4
    out[hit] = np.frombuffer(b"ACGT", np.uint8)[out[hit]]
    return out


def write_fasta(path, records):
    with open(path, "w") as f:
        for i, r in enumerate(records):
            f.write(">r%d\n%s\n" % (i, bytes(r).decode()))


def read_clusters(path):
    t = [[int(x) for x in line.split("\t")] for line in open(path).read().splitlines()]
    assert all(len(f) == 4 for f in t)
    return np.array(t, dtype=np.int64).reshape(-1, 4)


def pick_distance(sh, dn, k):
    """The first D of a short list whose Jaccard threshold no pair's shared / denom comes
    near: the host's exp is then not what decides a link."""
    import kmc
    sh, dn = sh[dn > 0].astype(np.float64), dn[dn > 0].astype(np.float64)
    for D in (0.05, 0.04, 0.06, 0.03, 0.07):
        if not (np.abs(sh / dn - kmc.mash_jaccard_of_distance(D, k)) < 1e-9).any():
            return D
    raise AssertionError("every candidate distance has a pair at its threshold")


def check_tsv(path, labels, index):
    t = read_clusters(path)
    n = labels.size
    assert t.shape == (n, 4)
    np.testing.assert_array_equal(t[:, 0], np.arange(n))
    np.testing.assert_array_equal(t[:, 1], labels)
    np.testing.assert_array_equal(t[:, 2], index)
    np.testing.assert_array_equal(t[:, 3], np.bincount(labels, minlength=n)[labels])


def test_cli_cluster(kmc, cuda, tmp_path):
    """A few random records, exact copies of some and copies with about 2 % substitutions:
    clusters.tsv holds the binding's clusters of the rows sketch_from_sequences gives for
    the same file."""
    import torch
    k, s = 21, 64
    rng = np.random.default_rng(8)
    base = [S.bases(rng, 3000) for _ in range(4)]
    records = [base[0], base[1], mutated(rng, base[2], 0.02), base[0].copy(), base[2], base[3], mutated(rng, base[1], 0.02),
               base[3].copy(), mutated(rng, base[2], 0.02)]
    fa = tmp_path / "records.fa"
    write_fasta(fa, records)
    data, idx, _ = kmc.load_fasta(str(fa), kmc.DIALECT_NONL, 0)
    assert idx.size - 1 == len(records)
    rows, sizes = kmc.sketch_from_sequences(dev(data, cuda), dev(idx, cuda), k, s)
    _, sh, dn = kmc.sketch_distances(rows, sizes, k, with_counts=True)
    torch.cuda.synchronize()
    D = pick_distance(u32(sh), u32(dn), k)
    labels, index, count = (u32(x) for x in kmc.sketch_cluster(rows, sizes, kmc.mash_jaccard_of_distance(D, k)))
    assert labels.tolist() == [0, 1, 2, 0, 2, 5, 1, 5, 2] and count.tolist() == [4]
    opts = ["-k", k, "--canonical", "--sketch", s, "--dialect", "nonl", "--max-seqs", 0]
    for name, more in (("direct", ["--sketch-direct"]), ("counted", [])):
        out = tmp_path / name
        out.mkdir()
        r = run(opts + more + ["--out", out, "--cluster", D, fa])
        assert r.returncode == 0, r.stderr
        assert "4 clusters of 9 records" in r.stdout
        assert not (out / "sketch_results.csv").exists()
        check_tsv(out / "clusters.tsv", labels, index)
    # without --cluster: what the run wrote before, and no clusters.tsv
    out = tmp_path / "plain"
    out.mkdir()
    r = run(opts + ["--sketch-direct", "--out", out, fa])
    assert r.returncode == 0, r.stderr
    assert (out / "sketch_results.csv").exists() and not (out / "clusters.tsv").exists()
    assert len(open(out / "sketch_results.csv").read().splitlines()) == 36


def test_cli_cluster_per_file(kmc, cuda, tmp_path):
    """--per-file on three files: the second holds the first one's records with about 2 %
    substitutions, the third is unrelated."""
    import torch
    k, s = 21, 64
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
        r, z = kmc.sketch_from_sequences_grouped(dev(data, cuda), dev(idx, cuda), go, k, s)
        rows.append(r)
        sizes.append(z)
    rows, sizes = torch.cat(rows), torch.cat(sizes)
    _, sh, dn = kmc.sketch_distances(rows, sizes, k, with_counts=True)
    torch.cuda.synchronize()
    D = pick_distance(u32(sh), u32(dn), k)
    labels, index, count = (u32(x) for x in kmc.sketch_cluster(rows, sizes, kmc.mash_jaccard_of_distance(D, k)))
    assert labels.tolist() == [0, 1, 1]
    out = tmp_path / "out"
    out.mkdir()
    r = run(["-k", k, "--canonical", "--sketch", s, "--sketch-direct", "--per-file", "--dialect", "nonl", "--out", out,
             "--cluster", D] + files)
    assert r.returncode == 0, r.stderr
    assert not (out / "sketch_results.csv").exists()
    check_tsv(out / "clusters.tsv", labels, index)
