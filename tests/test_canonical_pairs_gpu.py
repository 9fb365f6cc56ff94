"""The canonical back end's pair format across its tag boundary: a
pair is a list value with the count in its two top bits, tags 0..2 for counts 1..3
and tag 3 for "the count is in pc".  Every writer of pairs (K4s's two emit paths,
the table kernel's write-out) and every reader (canon_place_kernel,
canon_fallback_kernel), and the staged write-out that bypasses the format, must
agree with the CPU oracle on counts on both sides of 3 | 4, at the smallest input
that reaches each of them.

Inputs: one record of at most 4096 windows (one list): a random unit of u bases
repeated c times, c = 1..5 with u * c ~ 4000, so that interior k-mers occur c - 1
or c times.  c = 2 (u = 2000; once more under another seed) yields ~2000 results
from failing slots, more than the 1024 K4s stages: the results past that go
through emit_pair and a second queued copy.  So does c = 3 (u = 1333): every key
that occurs twice or more is such a result, so an input with more than 1024 of
them (by the oracle) must queue a copy, and the others (c = 1, 4, 5) none.
`mixed` (a unit of 1200 twice, one of 400 four times) is past the stage too, with
escaped counts among the results past 1024.

Paths, by the diagnostic hooks: direct output with the shipped caps (K4s, staged
write-out); direct output off (K4s -> pk -> canon_place_kernel); no counting sort
at all, direct output on (table kernel -> pk -> canon_fallback_kernel) and off
(table kernel -> pk -> canon_place_kernel).  The fallback counters are those of the
last direct-output call: a call with direct output off must leave them unchanged,
which is all they can say about it."""
import ctypes

import numpy as np
import pytest

KS = (31, 13)
# name -> ((unit length, copies), ...) and seed
INPUTS = {
    "c1": (((4000, 1),), 101),
    "c2": (((2000, 2),), 102),
    "c3": (((1333, 3),), 103),
    "c4": (((1000, 4),), 104),
    "c5": (((800, 5),), 105),
    "c2_past_stage": (((2000, 2),), 202),
    "mixed": (((1200, 2), (400, 4)), 303),
}
STAGED_RESULTS = 1024  # K4sLds::rc of the common instance
PATHS = ("direct", "placed", "table_direct", "table_placed")


def _record(name):
    parts, seed = INPUTS[name]
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    seq = np.concatenate([np.tile(rng.choice(acgt, size=u), c) for u, c in parts])
    data = np.append(seq, np.uint8(0))
    idx = np.array([0, data.size], dtype=np.int64)
    assert data.size - max(KS) <= 4096 and data.size - min(KS) <= 4096  # one list
    return data, idx


_expected = {}


def _oracle(oracle, name, k):
    """(data, idx, keys, counts, offsets) of an input, computed once and shared."""
    if (name, k) not in _expected:
        data, idx = _record(name)
        ek, ec, eo = oracle.count_canonical(data, idx, k)
        for a in (data, idx, ek, ec, eo):
            a.setflags(write=False)
        _expected[(name, k)] = (data, idx, ek, ec, eo)
    return _expected[(name, k)]


@pytest.mark.parametrize("k", KS)
def test_inputs_straddle_the_tag_boundary(oracle, k):
    """The oracle alone: input c holds counts c - 1 and c, so the set has counts on
    both sides of 3 | 4, c4 (and mixed) in one list."""
    for name, (parts, _) in INPUTS.items():
        counts = _oracle(oracle, name, k)[3]
        for _, c in parts:
            assert (counts == c).sum() > 100, (name, k, c)
        if len(parts) == 1 and parts[0][1] > 1:
            assert (counts == parts[0][1] - 1).any(), (name, k)
    for name in ("c4", "mixed"):
        counts = _oracle(oracle, name, k)[3]
        assert (counts <= 3).any() and (counts >= 4).any(), (name, k)
    assert _oracle(oracle, "c3", k)[3].max() == 3 and (_oracle(oracle, "c5", k)[3] == 4).any()


@pytest.fixture
def diag(kmc):
    """The diagnostic library; leaving the context restores every hook."""
    with kmc.diag() as D:
        yield D


def _fallback(D):
    ent, pairs = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
    assert D.kmc_diag_canon_fallback(ctypes.byref(ent), ctypes.byref(pairs)) == 0
    per = (ctypes.c_ulonglong * 1)()
    q3 = (ctypes.c_ulonglong * 3)()
    assert D.kmc_diag_canon_fallback_detail(per, 1, q3) == 0
    return ent.value, pairs.value, tuple(q3)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_pairs_match_oracle(kmc, oracle, cuda, diag, name, k, path):
    import torch
    data, idx, ek, ec, eo = _oracle(oracle, name, k)
    direct = path in ("direct", "table_direct")
    if path.startswith("table"):
        assert diag.kmc_diag_canon_sort_cap(0) == 0
    if not direct:
        assert diag.kmc_diag_canon_direct(0) == 0
    before = _fallback(diag)
    keys, counts, off = kmc.count_canonical(torch.tensor(data, device=cuda), torch.tensor(idx, device=cuda), k)
    torch.cuda.synchronize()
    gk, gc, go = keys.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32), off.cpu().numpy()
    ent, pairs, (big, table1, table2) = after = _fallback(diag)
    print("%s k=%d %s: distinct %d, fallback entries %d pairs %d, queued big %d table %d + %d"
          % (name, k, path, gk.size, ent, pairs, big, table1, table2))
    np.testing.assert_array_equal(go.astype(np.uint64), eo, err_msg="record offsets")
    o = np.argsort(gk, kind="stable")
    np.testing.assert_array_equal(gk[o], ek, err_msg="keys")
    np.testing.assert_array_equal(gc[o], ec, err_msg="counts")
    if path == "direct":  # K4s took the list; only the results past the stage are copied
        assert (big, table1, table2) == (0, 0, 0)
        if int((ec >= 2).sum()) > STAGED_RESULTS:  # c2, c2_past_stage, c3, mixed
            assert name not in ("c1", "c4", "c5")
            assert ent >= 1 and 0 < pairs < gk.size
        else:
            assert ent == 0 and pairs == 0
    elif path == "table_direct":  # the one list queued to the table kernel's first launch, one copy
        assert (big, table1, table2) == (0, 1, 0)
        assert ent == 1 and pairs == gk.size
    else:  # not a direct-output call
        assert after == before
