"""The late-input harness of test_streams_gpu.py: helpers, no tests.

A call of the library is made on a side stream `s` behind a device-side delay
(torch.cuda._sleep).  While the delay spins, everything the call may read holds a
decoy (valid input of the same shape), its caller workspace holds zeros and its
outputs a poison pattern; the real input, a 0xFF fill of the workspace and a fresh
poison of the outputs are enqueued on `s` after the delay and before the call.  A
launch or memset that the library (or the wrapper in kmc.py) puts on another stream
runs during the delay: it reads the decoy, or its zeroing is overwritten by the 0xFF
fill; outputs finished by work on another stream miss the snapshot taken on `s`;
outputs never written show as poison.  Nothing but `s` is synchronised.

torch.cuda.Stream() is created non-blocking (hipStreamNonBlocking), so the null
stream does not order against it: non_blocking() reads the flag back through
hipStreamGetFlags.  That is not enough: HIP maps streams onto a few hardware queues,
and a launch misplaced on a stream that shares `s`'s queue runs in enqueue order,
after the delay and the late input, and passes (seen on the MI355X: the memset of
kmc_pair_distances moved to the null stream went unnoticed in two of three cases).
side_streams() therefore picks `s` (and the control's second stream) among torch's
pool streams by showing that null-stream work completes while a delay spins on it.

Time of one call of each entry point at the shapes of test_streams_gpu.py, between
two events around the warm-up call on an MI355X (ms; the case's first call, so the
loading of its code objects is inside: an upper bound of the device time), ship
library / diagnostic library where both run:

    dropin_count 1.48             count_dense k=5 0.05, k=8 0.35, k=11 1.86 (sampled 2.05)
    count_dense_ex k=8 0.14       pair_distances n=20 k=4 0.60, k=3 0.03, n=3 k=9 0.06
    min_kmeres2 (12 rows) 0.10    count_canonical k=21 1.46, k=31 0.25
    pair_distances_sparse 0.54    synth_fill 0.30, synth_fill_range 0.02
    sketch_from_counts s=64 0.68 / 0.60, s=1000 0.24 / 0.15
    sketch_from_sequences s=16 1.07 / 1.23, s=1000 0.23 / 3.55
    sketch_from_sequences_grouped s=16 0.28 / 0.36, s=1000 0.24 / 3.55
    sketch_merge_groups 0.05 / 0.03        sketch_distances 0.04 / 0.03
    sketch_distances_rect 0.58 / 0.48      sketch_nearest 0.05 / 0.04
    longest: 3.55 -> delay 36 ms (about 2.4 million _sleep cycles per ms on that machine)

The delay is DELAY_FACTOR times the longest of them and never below MIN_DELAY_MS,
so that a misplaced operation certainly completes inside it and the host certainly
finishes enqueueing inside it.  The two control cases of the test file prove on the
machine at hand that it is long enough: there the library is handed a second side
stream and must be seen to read the decoy.
"""
import ctypes

import numpy as np

POISON = 0x5A
LONGEST_CALL_MS = 3.6   # the table's largest entry, rounded up
DELAY_FACTOR = 10
MIN_DELAY_MS = 30.0
DELAY_MS = max(MIN_DELAY_MS, DELAY_FACTOR * LONGEST_CALL_MS)

WARM_MS = {}   # name -> event time of the case's warm-up call (first call: code loading included)


def non_blocking(kmc, stream):
    """hipStreamGetFlags(stream) & hipStreamNonBlocking."""
    hip = kmc._hip()
    flags = ctypes.c_uint(0)
    rc = hip.hipStreamGetFlags(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(flags))
    assert rc == 0, "hipStreamGetFlags: %d" % rc
    return bool(flags.value & 0x01)


def sleep_cycles(ms):
    """(cycles, measured ms): the count at which torch.cuda._sleep spins for `ms`,
    scaled from one timed probe after a warm-up, and the time of one sleep of it."""
    import torch
    probe = 2_000_000
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda._sleep(probe)
    torch.cuda.synchronize()
    e[0].record()
    torch.cuda._sleep(probe)
    e[1].record()
    torch.cuda.synchronize()
    cycles = int(probe * ms / e[0].elapsed_time(e[1])) + 1
    e[2].record()
    torch.cuda._sleep(cycles)
    e[3].record()
    torch.cuda.synchronize()
    return cycles, e[2].elapsed_time(e[3])


def runs_beside(s, other, cycles):
    """True when work enqueued on `other` (None: the null stream) is done while a delay
    still spins on `s`.  HIP maps its streams onto a few hardware queues (4 by default);
    two streams that share one run in enqueue order, so a launch misplaced on `other`
    would still wait for the delay and the late input, and pass unseen.  No race: the
    marker is waited for, then `s` is asked once."""
    import torch
    o = other if other is not None else torch.cuda.default_stream()
    marker = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
    with torch.cuda.stream(o):
        marker.fill_(1)
    o.synchronize()
    beside = not s.query()
    s.synchronize()
    return beside


def side_streams(kmc, cuda, cycles, candidates=16):
    """(s, t): two non-blocking side streams out of torch's pool such that the null
    stream and `t` both run beside a delay on `s` (runs_beside)."""
    import torch
    pool = [torch.cuda.Stream(device=cuda) for _ in range(candidates)]
    for x in pool:
        assert non_blocking(kmc, x), "torch.cuda.Stream() is a blocking stream: the null stream orders against it"
    s = next((x for x in pool if runs_beside(x, None, cycles)), None)
    assert s is not None, "no side stream of %d runs beside the null stream" % candidates
    t = next((x for x in pool if x is not s and runs_beside(s, x, cycles) and runs_beside(x, None, cycles)), None)
    assert t is not None, "no second side stream runs beside the first"
    return s, t


def poison(t):
    t.reshape(-1).view(dtype=_u8()).fill_(POISON)


def _u8():
    import torch
    return torch.uint8


def same(a, b):
    """Two tuples of host values hold the same bits (NaN == NaN)."""
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=np.asarray(x).dtype.kind == "f")
                                    for x, y in zip(a, b))


class Call:
    """One entry-point call of the harness.
      ins     [(live, decoy, real)]: the device tensor the call reads and device copies
              of its two contents (same shape)
      outs    the device tensors the call writes (poisoned before it)
      zeroed  device tensors the contract wants zeroed by the caller (status words);
              read back after the outputs
      ws      the caller workspace or None
      run     run(which, stream) makes the call through kmc.py with stream=stream and
              the host arguments of input `which`; may return a list of further results
              (tensors, cloned on the stream, or host values)
      exp     {"decoy": ..., "real": ...}: what check() compares with
      check   check(got, exp, msg), got = the host copies of outs + zeroed + run's list
      flat    the two expectations as tuples of arrays: they must differ, or a call
              that read the decoy would pass"""

    def __init__(self, name, ins, outs, run, exp, check, flat, ws=None, zeroed=()):
        self.name, self.ins, self.outs, self.run, self.exp, self.check = name, ins, list(outs), run, exp, check
        self.ws, self.zeroed = ws, list(zeroed)
        assert not same(flat(exp["decoy"]), flat(exp["real"])), "%s: the decoy's result is the real one" % name

    def stage(self, which, ws_byte):
        """Enqueue on the current stream: the inputs of `which`, the workspace fill,
        the poison of the outputs, the zeroing of the status words."""
        for live, decoy, real in self.ins:
            live.copy_(real if which == "real" else decoy, non_blocking=True)
        if self.ws is not None:
            self.ws.fill_(ws_byte)
        for t in self.outs:
            poison(t)
        for t in self.zeroed:
            t.zero_()

    def results(self):
        return self.outs + self.zeroed


def _host(x):
    import torch
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _clone(x):
    import torch
    return x.clone() if isinstance(x, torch.Tensor) else x


def warm_up(call):
    """The call once on the decoy on the default stream (code objects loaded, the
    library's own buffers allocated), timed with events and checked."""
    import torch
    call.stage("decoy", 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    extra = call.run("decoy", None) or []
    e1.record()
    torch.cuda.synchronize()
    WARM_MS[call.name] = e0.elapsed_time(e1)
    call.check([_host(x) for x in call.results() + list(extra)], call.exp["decoy"], "%s warm-up (decoy)" % call.name)


def late_call(call, s, cycles, asynchronous=True):
    """Warm-up, then the late-input steps on side stream `s` (module docstring);
    asserts that the call returned while the delay was still spinning when the entry
    point is documented as asynchronous, and that the snapshot taken on `s` is the
    result of the real input."""
    import torch
    warm_up(call)
    call.stage("decoy", 0)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        call.stage("real", 0xFF)
        extra = call.run("real", s) or []
        busy = not s.query()
        snaps = [_clone(x) for x in call.results() + list(extra)]
    s.synchronize()
    if asynchronous:
        assert busy, "%s: the call returned only after the delay on its stream had ended: it waited for the " \
                     "device (or the delay is too short for the host's enqueueing)" % call.name
    call.check([_host(x) for x in snaps], call.exp["real"], "%s late input" % call.name)


def control_call(call, s, t, cycles):
    """The same late input on `s`, but the library is handed the second side stream
    `t`: its work runs during the delay and must give the DECOY's result.  Reads
    valid memory only (the workspace and the outputs are left to `t` alone)."""
    import torch
    warm_up(call)
    call.stage("decoy", 0)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        for live, _, real in call.ins:
            live.copy_(real, non_blocking=True)
        extra = call.run("real", t) or []
        busy = not s.query()
    t.synchronize()
    still = not s.query()
    s.synchronize()
    assert busy and still, "%s: the delay on s had ended before the work on t was done (busy after the call: %s, " \
                           "after t: %s): no late-input test of this file proves anything" % (call.name, busy, still)
    call.check([_host(x) for x in call.results() + list(extra)], call.exp["decoy"],
               "%s control (library on a second stream: the decoy's result)" % call.name)


# inputs ------------------------------------------------------------------------------
LENS_REAL = [0, 5, 3000, 40_000, 1, 70_001]
LENS_DECOY = [70_001, 1, 40_000, 5, 3000, 0]
ALPHABET = b"ACGTNacgt"
WEIGHTS = (.2, .2, .2, .2, .04, .04, .04, .04, .04)   # test_hash_gpu.test_canonical_random_vs_oracle's


def records(seed, lens, alphabet=ALPHABET, weights=WEIGHTS, related=0.03):
    """test_hash_gpu.random_records of these lengths; then every record but the
    longest takes the longest one's prefix except at a fraction `related` of its
    positions, so that records share k-mers and their distances are not all 1."""
    from test_hash_gpu import random_records
    rng = np.random.default_rng(seed)
    data, idx = random_records(rng, lens, alphabet, weights)
    lens = np.diff(idx) - 1
    big = int(np.argmax(lens))
    src = data[idx[big]:idx[big] + lens[big]].copy()
    for r in range(len(lens)):
        if r != big and lens[r] > 0:
            keep = rng.random(int(lens[r])) < related
            rec = data[idx[r]:idx[r] + lens[r]]
            rec[~keep] = src[:lens[r]][~keep]
    return data, idx


def overlap_rows(seed, n, s):
    """(rows uint64 [n, s], sizes uint32 [n]) drawn from one pool of 2 s values: row 0
    full, row 1 empty, the others of random size, so that pairs share values."""
    import sketch_query_util as Q
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(1, (1 << 64) - 1, size=2 * s + 64, dtype=np.uint64))[:2 * s]
    sizes = [s, 0] + [int(rng.integers(1, s + 1)) for _ in range(n - 2)]
    return Q.pack([rng.choice(pool, size=z, replace=False) for z in sizes], s)


def padded(a, n):
    """`a` followed by zeros up to n elements."""
    out = np.zeros(n, dtype=a.dtype)
    out[:a.size] = a
    return out
