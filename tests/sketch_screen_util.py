"""Host-side oracle of the screen (test_sketch_screen_gpu.py, test_sketch_screen_cli.py):
the canonical oracle's keys and counts of every record of the mixture, summed per key
over all records and hashed (sketch_util.hash_keys); shared, the lower median and the
multiplicities of a reference row follow with numpy.  Integers throughout, compared
bit for bit; the identity in float64, cast to float32.  After it, the helpers the two
test files share.  No device."""
import numpy as np

import sketch_util as S

SOFT, FWD = 1, 2


def mixture_hashes(oracle, data, idx, k, flags=0, seed=S.DEFAULT_SEED, first=0):
    """(hashes uint64 ascending, counts int64): every distinct hash among the valid
    windows of the records from `first` on and how many windows have it."""
    keys, counts, off = oracle.count_canonical(data, idx, k, soft=bool(flags & SOFT), forward=bool(flags & FWD))
    keys, counts = keys[int(off[first]):], counts[int(off[first]):]
    uniq, inv = np.unique(np.asarray(keys, dtype=np.uint64), return_inverse=True)
    tot = np.zeros(uniq.size, dtype=np.int64)
    np.add.at(tot, inv, np.asarray(counts).astype(np.int64))
    h = S.hash_keys(uniq, seed)
    order = np.argsort(h)
    return h[order], tot[order]


def multiplicities(mix, values):
    """The count of each of `values` in the mixture, 0 when absent."""
    h, c = mix
    values = np.asarray(values, dtype=np.uint64)
    pos = np.searchsorted(h, values)
    ok = pos < h.size
    ok[ok] = h[pos[ok]] == values[ok]
    out = np.zeros(values.size, dtype=np.int64)
    out[ok] = c[pos[ok]]
    return out


def identity_formula(shared, size, k):
    if size == 0:
        return np.float32(np.nan)
    if shared == 0:
        return np.float32(0.0)
    if shared == size:
        return np.float32(1.0)
    return np.float32(np.power(np.float64(shared) / np.float64(size), 1.0 / np.float64(k)))


def screen_expected(mix, rows, sizes, s, k):
    """(shared uint32 [n], median uint32 [n], identity float32 [n]) of the rows."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, s)
    n = rows.shape[0]
    shared = np.zeros(n, dtype=np.uint32)
    median = np.zeros(n, dtype=np.uint32)
    ident = np.zeros(n, dtype=np.float32)
    for r in range(n):
        size = min(int(sizes[r]), s)
        m = np.sort(multiplicities(mix, rows[r, :size]))
        m = m[m > 0]
        shared[r] = m.size
        if m.size:
            median[r] = m[(m.size - 1) // 2] & 0xFFFFFFFF
        ident[r] = identity_formula(m.size, size, k)
    return shared, median, ident


# helpers of the GPU test files ---------------------------------------------------------
def device_records(cuda, data, idx, shift=0):
    """A device copy of `data` that starts `shift` bytes after a 16-byte boundary, and the offsets."""
    import torch
    buf = torch.zeros(shift + data.size + 16, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 16 == 0
    d = buf[shift:shift + data.size]
    d.copy_(torch.from_numpy(np.ascontiguousarray(data)))
    return d, torch.from_numpy(np.ascontiguousarray(idx)).to(cuda)


def host_results(res):
    """kmc.sketch_screen_results' tensors as (shared uint32, median uint32, identity float32)."""
    sh, med, ident = res
    return (sh.cpu().numpy().view(np.uint32), med.cpu().numpy().view(np.uint32) if med is not None else None,
            ident.cpu().numpy() if ident is not None else None)


def assert_identity(out, eout, msg):
    """NaN, 0.0 and 1.0 bit for bit, the rest within one float32 ulp (as
    test_sketch_query_gpu.assert_floats compares distances)."""
    assert out.shape == eout.shape, msg
    special = np.isnan(eout) | (eout == 1.0) | (eout == 0.0)
    gb, eb = out.view(np.uint32).astype(np.int64), eout.view(np.uint32).astype(np.int64)
    assert (gb[special] == eb[special]).all(), "%s: special values differ" % msg
    ulp = np.abs(gb[~special] - eb[~special])  # positive finite floats: bit patterns are ordered
    print("%s: %d floats, %d special, max ulp %d" % (msg, out.size, int(special.sum()), int(ulp.max(initial=0))))
    assert (ulp <= 1).all(), "%s: max %d ulp" % (msg, int(ulp.max()))


def assert_screen(got, exp, msg=""):
    np.testing.assert_array_equal(got[0], exp[0], err_msg="%s shared" % msg)
    if got[1] is not None:
        np.testing.assert_array_equal(got[1], exp[1], err_msg="%s median" % msg)
    if got[2] is not None:
        assert_identity(got[2], exp[2], "%s identity" % msg)


def index_multiplicities(kmc, index, values, cuda):
    """The multiplicity the index holds of each of `values`, read through the public
    interface: the results of one-value rows (shared 1: the median is the value's)."""
    import torch
    values = np.asarray(values, dtype=np.uint64).reshape(-1, 1)
    rows = torch.from_numpy(values.view(np.int64)).to(cuda)
    sizes = torch.ones(values.shape[0], dtype=torch.int32, device=cuda)
    sh, med, _ = kmc.sketch_screen_results(index, rows, sizes, 21, identity=False)
    torch.cuda.synchronize()
    return sh.cpu().numpy().view(np.uint32).astype(np.int64) * med.cpu().numpy().view(np.uint32).astype(np.int64)
