// Exact order statistics of |x|, the quantile's interpolation, the division by a device scalar and the nan-median over a few rows:
// what hybrid[...] and mangio-crepe do to a track before and after the estimators.
//   * abs_select: radix select over the bit pattern of |x| (sign bit cleared; non-negative floats order like uint32, so -0,
//     denormals and +inf need no case of their own), four passes of eight bits from the top.  Every workgroup keeps an LDS histogram
//     of the pass's digit over the elements whose higher bits equal the prefix chosen so far and adds it to the pass's global
//     histogram; a one-workgroup kernel then finds the bucket that holds the rank, extends the prefix and takes the buckets below
//     off the rank.  Two ranks (k and k or k + 1) are carried with a prefix each: they share one histogram until they part.
//     Integer atomics only, so the result is exact and does not depend on the order of execution.  NaNs are counted in the first
//     pass; any NaN makes both results NaN (numpy's quantile).
//   * quantile_lerp: numpy's _lerp on the two values, every operation rounded on its own.
//   * div_scalar: x[i] / *s, IEEE division.
//   * nanmedian_rows: one column a thread, at most eight rows: the values sorted in registers with the NaNs last, the two middle ones
//     (the same one twice for an odd count) added to +0, then halved -- numpy.ma.median's arithmetic, which np.nanmedian takes for short axes.
#include "reduce.h"

#include <cmath>

namespace aicg {

constexpr int kSelectTile = 2048;                   // elements a workgroup histograms per step (8 a thread); tests/test_select.py names it
constexpr int kSelectPasses = 4;                    // 8 bits each
constexpr long kSelectMaxN = 1L << 27;
constexpr int kNanMedianMaxRows = 8;

// workspace, in 32-bit words: prefix[2], rank[2], NaN count, 3 unused, then hist[pass][rank][256]
constexpr int kSelPrefix = 0, kSelRank = 2, kSelNan = 4, kSelHist = 8;
constexpr int kSelectWords = kSelHist + kSelectPasses * 2 * 256;

__global__ void __launch_bounds__(256) select_init_kernel(unsigned* __restrict__ ws, unsigned rank_lo, unsigned rank_hi) {
    for (int i = threadIdx.x; i < kSelectWords; i += 256) ws[i] = i == kSelRank ? rank_lo : i == kSelRank + 1 ? rank_hi : 0u;
}

__global__ void __launch_bounds__(256) select_hist_kernel(const float* __restrict__ x, long n, int pass, unsigned* __restrict__ ws) {
    __shared__ unsigned h[2][256];
    __shared__ int nan_sh[4];
    const int shift = 24 - 8 * pass;
    const unsigned mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    const unsigned p0 = ws[kSelPrefix], p1 = ws[kSelPrefix + 1];
    const bool two = p0 != p1;
    h[0][threadIdx.x] = 0u;
    h[1][threadIdx.x] = 0u;
    __syncthreads();
    int nans = 0;
    for (long base = (long)blockIdx.x * kSelectTile; base < n; base += (long)gridDim.x * kSelectTile) {
        const long end = lmin(n, base + kSelectTile);
        for (long i = base + threadIdx.x; i < end; i += 256) {
            const unsigned key = (unsigned)__float_as_int(x[i]) & 0x7fffffffu;
            nans += key > 0x7f800000u;
            const unsigned d = (key >> shift) & 255u;
            if ((key & mask) == p0) atomicAdd(&h[0][d], 1u);
            if (two && (key & mask) == p1) atomicAdd(&h[1][d], 1u);
        }
    }
    __syncthreads();
    unsigned* g = ws + kSelHist + pass * 512;
    if (h[0][threadIdx.x]) atomicAdd(&g[threadIdx.x], h[0][threadIdx.x]);
    if (two && h[1][threadIdx.x]) atomicAdd(&g[256 + threadIdx.x], h[1][threadIdx.x]);
    if (pass == 0) {
        nans = block_sum(nans, nan_sh);
        if (threadIdx.x == 0 && nans) atomicAdd(&ws[kSelNan], (unsigned)nans);
    }
}

// One workgroup, one bucket a thread: the bucket whose span [below, below + count) holds the rank extends the prefix.  The last
// pass writes the two values.
__global__ void __launch_bounds__(256) select_pick_kernel(int pass, unsigned* __restrict__ ws, float* __restrict__ out2) {
    __shared__ unsigned c[2][256];
    const int shift = 24 - 8 * pass, t = threadIdx.x;
    const unsigned p0 = ws[kSelPrefix], p1 = ws[kSelPrefix + 1];
    const unsigned* g = ws + kSelHist + pass * 512;
    c[0][t] = g[t];
    c[1][t] = p0 != p1 ? g[256 + t] : g[t];
    const unsigned r[2] = {ws[kSelRank], ws[kSelRank + 1]}, p[2] = {p0, p1};
    const bool nan = ws[kSelNan] != 0u;
    __syncthreads();
    for (int j = 0; j < 2; ++j) {
        unsigned below = 0u;
        for (int i = 0; i < t; ++i) below += c[j][i];
        if (r[j] >= below && r[j] - below < c[j][t]) {
            const unsigned prefix = p[j] | ((unsigned)t << shift);
            ws[kSelPrefix + j] = prefix;
            ws[kSelRank + j] = r[j] - below;
            if (pass == kSelectPasses - 1) out2[j] = __builtin_bit_cast(float, nan ? 0x7fc00000u : prefix);
        }
    }
}

#pragma clang fp contract(off)  // numpy rounds the difference, the product and the sum separately
__global__ void quantile_lerp_kernel(const float* __restrict__ ab, float t, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float a = ab[0], b = ab[1], d = b - a;
    float r = a + d * t;
    if (t >= 0.5f) r = b - d * (1.f - t);
    out[0] = r;
}

__device__ __forceinline__ float fdiv_ieee(float a, float b) {
#ifdef AICG_EMULATED
    return a / b;
#else
    return __fdiv_rn(a, b);
#endif
}

__global__ void __launch_bounds__(256) div_scalar_kernel(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ y, long n) {
    const float d = s[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = fdiv_ieee(x[i], d);
}

#pragma clang fp contract(off)
__global__ void __launch_bounds__(256) nanmedian_rows_kernel(const double* __restrict__ stack, int k, long n, double* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double kNan = __builtin_bit_cast(double, 0x7ff8000000000000LL);
    double v[kNanMedianMaxRows];
    int m = 0;
#pragma unroll
    for (int r = 0; r < kNanMedianMaxRows; ++r) {
        v[r] = r < k ? stack[(long)r * n + i] : kNan;
        m += v[r] == v[r];
    }
    // odd-even transposition sort, NaNs last: unrolled compare-exchanges of neighbours, so v stays in registers; stable
#pragma unroll
    for (int round = 0; round < kNanMedianMaxRows; ++round) {
#pragma unroll
        for (int q = round & 1; q + 1 < kNanMedianMaxRows; q += 2) {
            const double a = v[q], b = v[q + 1];
            const bool swap = (a != a && b == b) || a > b;
            v[q] = swap ? b : a;
            v[q + 1] = swap ? a : b;
        }
    }
    double lo = 0.0, hi = 0.0;
#pragma unroll
    for (int q = 0; q < kNanMedianMaxRows; ++q) {
        if (q == (m - 1) / 2) lo = v[q];
        if (q == m / 2) hi = v[q];
    }
    out[i] = m == 0 ? kNan : ((0.0 + lo) + hi) / 2.0;   // numpy.ma's sum starts from +0: a median of -0 comes out as +0
}

static int select_shape(const char* who, int64_t n) {
    if (n < 1 || n > kSelectMaxN) return fail(AICG_E_SHAPE, "%s: n %lld outside [1, 2^27]", who, (long long)n);
    return AICG_OK;
}

}  // namespace aicg

using namespace aicg;

extern "C" int aicg_abs_select_workspace_bytes(int64_t n) {
    if (int rc = select_shape("aicg_abs_select_workspace_bytes", n)) return rc;
    return kSelectWords * (int)sizeof(unsigned);
}

extern "C" int aicg_abs_select_f32(const float* x, int64_t n, int64_t rank_lo, int64_t rank_hi, float* out2, void* workspace, void* stream) {
    if (int rc = select_shape("aicg_abs_select_f32", n)) return rc;
    if (!x || !out2 || !workspace) return fail(AICG_E_ARG, "aicg_abs_select_f32: null pointer");
    if (rank_lo < 0 || rank_hi >= n || (rank_hi != rank_lo && rank_hi != rank_lo + 1))
        return fail(AICG_E_ARG, "aicg_abs_select_f32: ranks %lld, %lld of %lld", (long long)rank_lo, (long long)rank_hi, (long long)n);
    hipStream_t st = (hipStream_t)stream;
    unsigned* ws = (unsigned*)workspace;
    hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(256), 0, st, ws, (unsigned)rank_lo, (unsigned)rank_hi);
    const unsigned grid = grid_1d(ldiv_up((long)n, kSelectTile / 256));
    for (int pass = 0; pass < kSelectPasses; ++pass) {
        hipLaunchKernelGGL(select_hist_kernel, dim3(grid), dim3(256), 0, st, x, (long)n, pass, ws);
        hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(256), 0, st, pass, ws, out2);
    }
    return check_launch("select_hist_kernel");
}

extern "C" int aicg_quantile_lerp(const float* ab, float t, float* out, void* stream) {
    if (!ab || !out) return fail(AICG_E_ARG, "aicg_quantile_lerp: null pointer");
    hipLaunchKernelGGL(quantile_lerp_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ab, t, out);
    return check_launch("quantile_lerp_kernel");
}

extern "C" int aicg_div_scalar(const float* x, const float* s, float* y, int64_t n, void* stream) {
    if (n < 0 || n >= (1L << 40)) return fail(AICG_E_SHAPE, "aicg_div_scalar: n %lld", (long long)n);
    if (n == 0) return AICG_OK;
    if (!x || !s || !y) return fail(AICG_E_ARG, "aicg_div_scalar: null pointer");
    hipLaunchKernelGGL(div_scalar_kernel, dim3(grid_1d((long)n)), dim3(256), 0, (hipStream_t)stream, x, s, y, (long)n);
    return check_launch("div_scalar_kernel");
}

extern "C" int aicg_nanmedian_rows(const double* stack, int k, int64_t n, double* out, void* stream) {
    if (k < 1 || k > kNanMedianMaxRows || n < 0 || n >= (1L << 31) * 256)
        return fail(AICG_E_SHAPE, "aicg_nanmedian_rows: %d rows of %lld", k, (long long)n);
    if (n == 0) return AICG_OK;
    if (!stack || !out) return fail(AICG_E_ARG, "aicg_nanmedian_rows: null pointer");
    hipLaunchKernelGGL(nanmedian_rows_kernel, dim3((unsigned)ldiv_up((long)n, 256L)), dim3(256), 0, (hipStream_t)stream, stack, k, (long)n, out);
    return check_launch("nanmedian_rows_kernel");
}
