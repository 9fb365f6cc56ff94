"""Host-side model of the abundance spectrum (test_spectrum_args.py, test_spectrum_gpu.py,
test_spectrum_cli.py): helpers, no tests, no device.

model(): the expected hist and stats of kmc_spectrum_from_accum from the oracle's hashes
and exact multiplicities (sketch_screen_util.mixture_hashes).  `limit` is never computed
here: it is the device's stats[1], which check_limit() holds against the level's bound.

summarize(): kmc_spectrum_summarize with the expressions of include/kmc.h, one IEEE
operation per double, so the library's doubles must have the same bits.  The valley is
the first bin that is not above a NON-EMPTY next bin: under `hist[c] <= hist[c + 1]`
alone the two empty bins past the last count of any spectrum shorter than its bins
(every assembly: hist = 0, n, 0, 0, ...) would be a valley, and such a file must have
none (min_abundance 1)."""
import collections
import math

import numpy as np

FILL = (1 << 64) - 1
M64 = FILL
MAX_BINS = 8192

Summary = collections.namedtuple("Summary", ["scale", "sampled_distinct", "sampled_total", "distinct", "total", "valley",
                                             "peak", "min_abundance", "saturated", "genome_size"])
INT_FIELDS = ("sampled_distinct", "sampled_total", "valley", "peak", "min_abundance", "saturated")
DOUBLE_FIELDS = ("scale", "distinct", "total", "genome_size")


def model(mix, limit, everything, B):
    """(hist uint64 [B], stats [4] as Python ints) for the (hashes, counts) of the oracle."""
    h, c = mix
    c = np.asarray(c, dtype=np.int64)
    below = c if everything else c[np.asarray(h, dtype=np.uint64) < np.uint64(limit)]
    hist = np.bincount(np.minimum(below, B - 1), minlength=B).astype(np.uint64)
    return hist, [1 if everything else 0, int(limit), int(below.size), int(below.sum())]


def check_limit(stats, j, lossless=None):
    """The device's limit against the level's bound, as test_sketch_accum_gpu.check does;
    returns (limit, everything)."""
    bound = FILL if j == 0 else 1 << (64 - j)
    exact, limit = int(stats[0]), int(stats[1])
    assert limit <= bound, "limit above 2^(64 - j)"
    if lossless is True:
        assert limit == bound, "something was lost"
    if lossless is False:
        assert limit < bound, "nothing was lost"
    everything = j == 0 and limit == FILL
    assert exact == (1 if everything else 0)
    return limit, everything


def host(hist, stats=None):
    """SketchAccum.spectrum's tensors as (uint64 array, [4] Python ints or None)."""
    h = hist.cpu().numpy().view(np.uint64)
    return h, ([int(x) for x in stats.cpu().numpy().view(np.uint64)] if stats is not None else None)


def summarize(hist, limit):
    hist = [int(x) for x in hist]
    B = len(hist)
    assert 2 <= B <= MAX_BINS and 0 < limit <= FILL
    scale = 1.0 if limit == FILL else math.ldexp(1.0, 64) / float(limit)
    sampled_distinct = sum(hist[c] for c in range(1, B)) & M64
    sampled_total = sum(c * hist[c] for c in range(1, B)) & M64
    distinct = scale * float(sampled_distinct)
    total = scale * float(sampled_total)
    valley = next((c for c in range(1, B - 2) if hist[c + 1] > 0 and hist[c] <= hist[c + 1]), 0)
    peak = 0
    if valley > 0:
        peak = valley + 1
        for c in range(valley + 2, B - 1):
            if hist[c] > hist[peak]:
                peak = c
    min_abundance = valley if valley > 0 else 1
    saturated = 1 if hist[B - 1] > 0 else 0
    genome_size = 0.0
    if peak > 0:
        solid = sum(c * hist[c] for c in range(valley, B)) & M64
        genome_size = (scale * float(solid)) / float(peak)
    return Summary(scale, sampled_distinct, sampled_total, distinct, total, valley, peak, min_abundance, saturated,
                   genome_size)


def bits(x):
    return np.float64(x).view(np.uint64)


def assert_summary(got, exp, msg=""):
    """Integers equal, doubles bit-equal."""
    for f in INT_FIELDS:
        assert int(getattr(got, f)) == int(getattr(exp, f)), "%s: %s %s != %s" % (msg, f, getattr(got, f), getattr(exp, f))
    for f in DOUBLE_FIELDS:
        assert bits(getattr(got, f)) == bits(getattr(exp, f)), "%s: %s %r != %r" % (msg, f, getattr(got, f),
                                                                                   getattr(exp, f))


def g6(x):
    """printf's %.6g."""
    return "%.6g" % x


def tsv_lines(index, path, hist, stats, summary, used):
    """(the file's lines of spectrum.tsv, its line of spectrum_summary.tsv)."""
    rows = ["%d\t%d\t%d\t%s" % (index, c, int(hist[c]), g6(summary.scale * float(int(hist[c]))))
            for c in range(1, len(hist)) if int(hist[c]) > 0]
    line = "\t".join([str(index), str(path), str(stats[1]), g6(summary.scale), str(stats[2]), str(stats[3]),
                      g6(summary.distinct), g6(summary.total), str(summary.valley), str(summary.peak), str(used),
                      str(summary.saturated), g6(summary.genome_size)])
    return rows, line
