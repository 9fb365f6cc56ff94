// kmc_dist_common.h — what the dense (kmc_dist.hip) and the sparse
// (kmc_dist_sparse.hip) pairwise-distance paths share: the packed-triangle index,
// the record length, the distance expression, and the kernel that turns exact
// uint64 pair sums into distances.  One definition, so the two paths cannot drift
// apart in a rounding or an index.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace kmc {
namespace {

// packed upper triangle, row-major: getIdxTriangularMatrixRowMajor(i+1, j-i, n)
// (kernels.h:46-48) = n*i - i*(i-1)/2 + (j - i) - (i + 1)
__device__ __forceinline__ int64_t tri_index(int64_t i, int64_t j, int64_t n) {
    return n * i - (i * (i - 1)) / 2 + (j - i) - (i + 1);
}

// The CPU formula, main.cu:614: 1 - (float)sum / (minLength - k + 1), the long
// denominator converted to float by the usual arithmetic conversions.
__device__ __forceinline__ float distance_of(uint64_t s, int64_t li, int64_t lj, int k) {
    const int64_t m = li < lj ? li : lj;
    return 1.0f - (float)s / (float)(m - k + 1);
}

// Inverts q = tri_index(i, j, n).  Row i of the strict upper triangle of n starts at
// tri_row_start(i, n) = tri_index(i, i + 1, n); tri_row is the row i <= n - 2 with
// tri_row_start(i) <= q < tri_row_start(i + 1), found by search from a float guess.
__device__ __forceinline__ int64_t tri_row_start(int64_t i, int64_t n) {
    return i * (2 * n - i - 1) / 2;  // n i - i (i + 1) / 2, one product (even: i or 2n - 1 - i is)
}

__device__ __forceinline__ int64_t tri_row(int64_t q, int64_t n) {
    const double nn = (double)n;
    int64_t i = (int64_t)((2 * nn - 1 - sqrt((2 * nn - 1) * (2 * nn - 1) - 8.0 * (double)q)) / 2);
    if (i < 0) i = 0;
    if (i > n - 2) i = n - 2;
    while (i > 0 && tri_row_start(i, n) > q) --i;
    while (i + 2 < n && tri_row_start(i + 1, n) <= q) ++i;
    return i;
}

__device__ __forceinline__ int64_t rec_len(const int64_t *idx, int64_t s) { return idx[s + 1] - idx[s] - 1; }

// acc[pair] -> out[pair] over the n(n-1)/2 pairs of the packed triangle
__global__ __launch_bounds__(256) void pair_finish_kernel(const unsigned long long *acc, const int64_t *indices,
                                                          int64_t n, int k, float *out) {
    const int64_t npairs = n * (n - 1) / 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < npairs; q += (int64_t)gridDim.x * 256) {
        const int64_t i = tri_row(q, n), j = q - tri_row_start(i, n) + i + 1;
        out[q] = distance_of(acc[q], rec_len(indices, i), rec_len(indices, j), k);
    }
}

inline void launch_pair_finish(const unsigned long long *acc, const int64_t *indices, int64_t n, int k, float *out,
                               hipStream_t stream) {
    const int64_t npairs = n * (n - 1) / 2;
    int64_t blocks = (npairs + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, acc, indices, n, k, out);
}

}  // namespace
}  // namespace kmc
