// kmc_spectrum.cpp — what is read off an abundance spectrum (kmc_spectrum_from_accum's
// hist, copied to the host): the scale of the sample, the estimated distinct and total
// k-mers, the valley between the error k-mers and the coverage peak, the peak, the
// minimum abundance the valley suggests and the genome size.  Host only; every double
// is one IEEE operation on the operands kmc.h states, so a model with the same
// expressions gives the same bits.
#include <cmath>
#include <cstdint>

#include "kmc.h"

extern "C" int kmc_spectrum_summarize(const uint64_t *hist, uint32_t num_bins, uint64_t limit,
                                      kmc_spectrum_summary *out) {
    if (!hist || !out || num_bins < 2 || num_bins > KMC_SPECTRUM_MAX_BINS || limit == 0) return KMC_ERR_INVALID_ARG;
    const uint32_t B = num_bins;
    kmc_spectrum_summary s;
    s.scale = limit == UINT64_MAX ? 1.0 : std::ldexp(1.0, 64) / (double)limit;
    s.sampled_distinct = 0;
    s.sampled_total = 0;
    for (uint32_t c = 1; c < B; ++c) {
        s.sampled_distinct += hist[c];
        s.sampled_total += (uint64_t)c * hist[c];
    }
    s.distinct = s.scale * (double)s.sampled_distinct;
    s.total = s.scale * (double)s.sampled_total;
    // the last bin is a tail, not a count: it is neither a valley's rise nor a peak
    s.valley = 0;
    for (uint32_t c = 1; c + 3 <= B; ++c)
        if (hist[c + 1] > 0 && hist[c] <= hist[c + 1]) {
            s.valley = c;
            break;
        }
    s.peak = 0;
    if (s.valley > 0) {
        s.peak = s.valley + 1;
        for (uint32_t c = s.valley + 2; c + 2 <= B; ++c)
            if (hist[c] > hist[s.peak]) s.peak = c;
    }
    s.min_abundance = s.valley > 0 ? s.valley : 1u;
    s.saturated = hist[B - 1] > 0 ? 1u : 0u;
    s.genome_size = 0.0;
    if (s.peak > 0) {
        uint64_t solid = 0;
        for (uint32_t c = s.valley; c < B; ++c) solid += (uint64_t)c * hist[c];
        const double scaled = s.scale * (double)solid;
        s.genome_size = scaled / (double)s.peak;
    }
    *out = s;
    return KMC_OK;
}
