"""Host-side oracle shared by the sketch tests (test_sketch_abi.py,
test_sketch_gpu.py, test_sketch_cli.py): plain numpy with uint64 wrap-around
arithmetic, no device.  After it, the helpers the GPU test files of the sketch and
sparse-distance paths have in common."""
import contextlib

import numpy as np

_U = np.uint64
GOLDEN_GAMMA = 0x9E3779B97F4A7C15
MUL1 = 0xBF58476D1CE4E5B9
MUL2 = 0x94D049BB133111EB
INV1 = pow(MUL1, -1, 1 << 64)
INV2 = pow(MUL2, -1, 1 << 64)
FILL = np.uint64(0xFFFFFFFFFFFFFFFF)
DEFAULT_SEED = 42


def hash_keys(keys, seed=DEFAULT_SEED):
    """h(key) = splitmix64 output 0 of the stream seeded with key ^ seed."""
    keys = np.asarray(keys, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (keys ^ _U(seed)) + _U(GOLDEN_GAMMA)
        z = (z ^ (z >> _U(30))) * _U(MUL1)
        z = (z ^ (z >> _U(27))) * _U(MUL2)
        return z ^ (z >> _U(31))


def _unxorshift(y, sh):
    """x with x ^ (x >> sh) == y: the shift repeated until it falls off."""
    x = y.copy()
    t = y >> _U(sh)
    while t.any():
        x ^= t
        t = t >> _U(sh)
    return x


def unhash(h, seed=DEFAULT_SEED):
    """The key with hash_keys(key, seed) == h."""
    h = np.asarray(h, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = _unxorshift(h, 31)
        z = _unxorshift(z * _U(INV2), 27)
        z = _unxorshift(z * _U(INV1), 30)
        return (z - _U(GOLDEN_GAMMA)) ^ _U(seed)


def sketch_expected(keys, counts, off, n, s, seed=DEFAULT_SEED, min_count=1):
    """(rows uint64 [n, s], sizes uint32 [n]): per record, offsets clamped to
    len(keys), filter, hash, np.sort, [:s]; FILL after the sketch."""
    keys = np.asarray(keys, dtype=np.uint64)
    E = keys.size
    off = np.minimum(np.asarray(off).astype(np.uint64), _U(E)).astype(np.int64)
    rows = np.full((n, s), FILL, dtype=np.uint64)
    sizes = np.zeros(n, dtype=np.uint32)
    for r in range(n):
        a, b = int(off[r]), int(off[r + 1])
        kk = keys[a:b]
        if min_count > 1:
            kk = kk[np.asarray(counts)[a:b].astype(np.uint64) >= _U(min_count)]
        h = np.sort(hash_keys(kk, seed))[:s]
        rows[r, :h.size] = h
        sizes[r] = h.size
    return rows, sizes


def mash_formula(shared, denom, k):
    """The distance of one pair from its two counts: float64, cast to float32."""
    if denom == 0:
        return np.float32(np.nan)
    if shared == 0:
        return np.float32(1.0)
    if shared == denom:
        return np.float32(0.0)
    j = np.float64(shared) / np.float64(denom)
    d = -np.log(2.0 * j / (1.0 + j)) / np.float64(k)
    return np.float32(min(d, 1.0))


def distances_expected(rows, sizes, s, k):
    """(out float32, shared uint32, denom uint32) over the packed upper triangle:
    per pair np.union1d(A, B)[:s], intersected with both."""
    rows = np.asarray(rows, dtype=np.uint64)
    n = rows.shape[0]
    sets = [rows[r, :min(int(sizes[r]), s)] for r in range(n)]
    npairs = n * (n - 1) // 2
    out = np.zeros(npairs, dtype=np.float32)
    shared = np.zeros(npairs, dtype=np.uint32)
    denom = np.zeros(npairs, dtype=np.uint32)
    q = 0
    for i in range(n):
        for j in range(i + 1, n):
            u = np.union1d(sets[i], sets[j])[:s]
            both = np.intersect1d(sets[i], sets[j], assume_unique=True)
            sh = np.intersect1d(u, both, assume_unique=True).size
            shared[q], denom[q] = sh, u.size
            out[q] = mash_formula(sh, u.size, k)
            q += 1
    return out, shared, denom


# helpers of the GPU test files ---------------------------------------------------------
def which(kmc, lib):
    """The library a case runs in: libkmc_diag.so inside the context, else libkmc.so."""
    return kmc.diag() if lib == "diag" else contextlib.nullcontext()


def dev(x, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def cache():
    """cached(key, make) over a store of its own: make() runs once per key."""
    store = {}

    def cached(key, make):
        if key not in store:
            store[key] = make()
        return store[key]
    return cached


def bases(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(n))


def pack(records):
    """Records (uint8 base arrays) -> (data with a 0 terminator after each, int64 offsets)."""
    parts, idx = [], [0]
    for r in records:
        parts += [np.asarray(r, dtype=np.uint8), np.zeros(1, np.uint8)]
        idx.append(idx[-1] + len(r) + 1)
    return np.concatenate(parts), np.asarray(idx, dtype=np.int64)


def assert_sketch(got, exp, msg=""):
    (rows, sizes), (erows, esizes) = got, exp
    np.testing.assert_array_equal(sizes, esizes, err_msg="%s sizes" % msg)
    assert rows.shape == erows.shape, msg
    bad = np.nonzero((rows != erows).any(axis=1))[0]
    assert bad.size == 0, "%s: rows %s differ" % (msg, bad[:5])
