// Stems handed from one stage of a cover to the next in HBM: the head and the tail of run_mdx (reference src/mdx.py:257-280)
// without the WAV file, the host numpy passes and the wait for the peak in between.
//   * aicg_stem_normalise: the previous stage's 16-bit PCM stem (read as x / 32768, as the WAV reader does) or the first stage's
//     float file -> two rows of wave / peak, with peak = max(max(x), |min(x)|) = max |x| left in device memory;
//   * aicg_mdx_stems_pcm16: separated * peak and wave - (separated * peak) * compensation -> the two 16-bit PCM stems.
// numpy rounds after every operation of those lines, so nothing here may be contracted into a fused multiply-add, and the division
// is the IEEE-rounded one (hipcc's default for `/` on float; no reciprocal multiply).
// Both are single passes bound by HBM: 4 frames per thread and step, 16-byte loads and stores.  Row 1 of a (2, n) signal starts at
// n floats, which is 16-byte aligned only when n % 4 == 0; float rows are therefore accessed through a 4-byte aligned vector type
// (common.h's float4_u).
// Non-finite samples are not numpy's: the peak is a maximum of |x| bit patterns taken with fmaxf, which skips a NaN where np.max
// returns it, and the PCM conversion clips a NaN to -32768.  A silent stem (peak 0) divides by zero as numpy does.
#include "reduce.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace aicg {

constexpr int kFmtPcm16 = 0, kFmtF32 = 1;   // aicg_stem_normalise's in_format

// max |x| over `total` floats
__global__ void __launch_bounds__(256) stem_peak_f32_kernel(const float* __restrict__ x, long total, unsigned* __restrict__ peak_bits) {
    float m = 0.f;
    const long groups = total / 4;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(x)[g];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    if (blockIdx.x == 0 && (long)threadIdx.x < total - groups * 4) m = fmaxf(m, fabsf(x[groups * 4 + threadIdx.x]));
    peak_commit(m, peak_bits);
}

// max |x / 32768| over `total` 16-bit samples: the largest magnitude as an integer (-32768 gives 32768), scaled once (exact)
__global__ void __launch_bounds__(256) stem_peak_pcm16_kernel(const short* __restrict__ x, long total, unsigned* __restrict__ peak_bits) {
    int m = 0;
    const long groups = total / 8;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
        const short8_t v = reinterpret_cast<const short8_t*>(x)[g];
        const short s[8] = {v.lo.x, v.lo.y, v.lo.z, v.lo.w, v.hi.x, v.hi.y, v.hi.z, v.hi.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) m = imax(m, s[j] < 0 ? -(int)s[j] : (int)s[j]);
    }
    if (blockIdx.x == 0 && (long)threadIdx.x < total - groups * 8) {
        const int s = x[groups * 8 + threadIdx.x];
        m = imax(m, s < 0 ? -s : s);
    }
    peak_commit((float)m * (1.0f / 32768.0f), peak_bits);
}

// frames f .. f + 3 of channel c (a mono input serves both rows) as floats
template <int FMT, int C>
__device__ __forceinline__ float4_u stem_load4(const void* __restrict__ x, long n, long f, int c) {
    if (FMT == kFmtF32) return *reinterpret_cast<const float4_u*>((const float*)x + (C == 2 ? c * n : 0) + f);
    const float k = 1.0f / 32768.0f;   // a power of two: the product is the exact quotient
    if (C == 1) {
        const short4_t v = *reinterpret_cast<const short4_t*>((const short*)x + f);
        return float4_u{(float)v.x * k, (float)v.y * k, (float)v.z * k, (float)v.w * k};
    }
    const short8_t v = *reinterpret_cast<const short8_t*>((const short*)x + 2 * f);
    return c == 0 ? float4_u{(float)v.lo.x * k, (float)v.lo.z * k, (float)v.hi.x * k, (float)v.hi.z * k}
                  : float4_u{(float)v.lo.y * k, (float)v.lo.w * k, (float)v.hi.y * k, (float)v.hi.w * k};
}
template <int FMT, int C>
__device__ __forceinline__ float stem_load1(const void* __restrict__ x, long n, long f, int c) {
    if (FMT == kFmtF32) return ((const float*)x)[(C == 2 ? c * n : 0) + f];
    return (float)((const short*)x)[C == 2 ? 2 * f + c : f] * (1.0f / 32768.0f);
}

// out[c][f] = x[c][f] / peak (`wave /= peak`, src/mdx.py:259)
template <int FMT, int C>
__global__ void __launch_bounds__(256) stem_divide_kernel(const void* __restrict__ x, float* __restrict__ out, long n,
                                                          const float* __restrict__ peak) {
    const float p = *peak;
    const long groups = n / 4;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float4_u v = stem_load4<FMT, C>(x, n, 4 * g, c);
            float4_u r;
            r.x = v.x / p; r.y = v.y / p; r.z = v.z / p; r.w = v.w / p;
            *reinterpret_cast<float4_u*>(out + c * n + 4 * g) = r;
        }
    }
    if (blockIdx.x == 0 && (long)threadIdx.x < n - groups * 4) {
        const long f = groups * 4 + threadIdx.x;
        for (int c = 0; c < 2; ++c) out[c * n + f] = stem_load1<FMT, C>(x, n, f, c) / p;
    }
}

// soundfile's 16-bit PCM of a float, as audio_io.write_wav_pcm16 computes it in float64: rint(clip(y, -1, 32767 / 32768) * 32768),
// ties to even.  Both clip bounds are floats, so the clipped value is the float64 one; its product with 2^15 is exact in float32
// (a change of exponent, at most 2^15 in size); rintf rounds that same number the same way: float32 is enough.
__device__ __forceinline__ short stem_pcm16(float y) {
    y = fminf(fmaxf(y, -1.0f), 32767.0f / 32768.0f);
    return (short)(int)rintf(y * 32768.0f);
}

struct StemPair { short main, inv; };
// s = separated * peak; inverted = wave - s * compensation: three float32 roundings, as numpy makes them (src/mdx.py:264,280)
__device__ __forceinline__ StemPair stem_pair(float w, float sep, float p, float comp) {
    const float s = sep * p;
    const float t = s * comp;
    const float d = w - t;
    return StemPair{stem_pcm16(s), stem_pcm16(d)};
}

__global__ void __launch_bounds__(256) mdx_stems_pcm16_kernel(const float* __restrict__ wave, const float* __restrict__ sep,
                                                              const float* __restrict__ peak, float comp, long n,
                                                              short* __restrict__ main_out, short* __restrict__ inv_out) {
    const float p = *peak;
    const long groups = n / 4;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
        const long f = 4 * g;
        const float4_u w0 = *reinterpret_cast<const float4_u*>(wave + f), w1 = *reinterpret_cast<const float4_u*>(wave + n + f);
        const float4_u s0 = *reinterpret_cast<const float4_u*>(sep + f), s1 = *reinterpret_cast<const float4_u*>(sep + n + f);
        const StemPair a0 = stem_pair(w0.x, s0.x, p, comp), b0 = stem_pair(w1.x, s1.x, p, comp);
        const StemPair a1 = stem_pair(w0.y, s0.y, p, comp), b1 = stem_pair(w1.y, s1.y, p, comp);
        const StemPair a2 = stem_pair(w0.z, s0.z, p, comp), b2 = stem_pair(w1.z, s1.z, p, comp);
        const StemPair a3 = stem_pair(w0.w, s0.w, p, comp), b3 = stem_pair(w1.w, s1.w, p, comp);
        if (main_out)
            reinterpret_cast<short8_t*>(main_out)[g] = short8_t{{a0.main, b0.main, a1.main, b1.main}, {a2.main, b2.main, a3.main, b3.main}};
        if (inv_out)
            reinterpret_cast<short8_t*>(inv_out)[g] = short8_t{{a0.inv, b0.inv, a1.inv, b1.inv}, {a2.inv, b2.inv, a3.inv, b3.inv}};
    }
    if (blockIdx.x == 0 && (long)threadIdx.x < n - groups * 4) {
        const long f = groups * 4 + threadIdx.x;
        for (int c = 0; c < 2; ++c) {
            const StemPair r = stem_pair(wave[c * n + f], sep[c * n + f], p, comp);
            if (main_out) main_out[2 * f + c] = r.main;
            if (inv_out) inv_out[2 * f + c] = r.inv;
        }
    }
}

template <int FMT, int C>
static void launch_divide(const void* x, float* out, long n, const float* peak, hipStream_t s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(stem_divide_kernel<FMT, C>), dim3(grid_1d(n / 4)), dim3(256), 0, s, x, out, n, peak);
}

}  // namespace aicg

using namespace aicg;

extern "C" int aicg_stem_normalise(const void* x, int in_format, int n_channels, int64_t n, float* out, float* peak, void* stream) {
    if (in_format != kFmtPcm16 && in_format != kFmtF32)
        return fail(AICG_E_ARG, "aicg_stem_normalise: input format %d (0 = int16 frames x channels, 1 = float32 channels x frames)", in_format);
    if (n_channels < 1 || n_channels > 2 || n < 0)
        return fail(AICG_E_SHAPE, "aicg_stem_normalise: %d channels, n %lld", n_channels, (long long)n);
    if (!peak || (n > 0 && (!x || !out))) return fail(AICG_E_ARG, "aicg_stem_normalise: null pointer");
    if (((uintptr_t)x | (uintptr_t)out) & 15) return fail(AICG_E_ARG, "aicg_stem_normalise: buffers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(peak, 0, sizeof(float), s);
    if (n == 0) return AICG_OK;
    const long total = (long)n * n_channels;
    if (in_format == kFmtF32)
        hipLaunchKernelGGL(stem_peak_f32_kernel, dim3(grid_1d(total / 4)), dim3(256), 0, s, (const float*)x, total, (unsigned*)peak);
    else
        hipLaunchKernelGGL(stem_peak_pcm16_kernel, dim3(grid_1d(total / 8)), dim3(256), 0, s, (const short*)x, total, (unsigned*)peak);
    const int rc = check_launch("stem_peak_kernel");
    if (rc != AICG_OK) return rc;
    if (in_format == kFmtF32) {
        if (n_channels == 2) launch_divide<kFmtF32, 2>(x, out, (long)n, peak, s); else launch_divide<kFmtF32, 1>(x, out, (long)n, peak, s);
    } else {
        if (n_channels == 2) launch_divide<kFmtPcm16, 2>(x, out, (long)n, peak, s); else launch_divide<kFmtPcm16, 1>(x, out, (long)n, peak, s);
    }
    return check_launch("stem_divide_kernel");
}

extern "C" int aicg_mdx_stems_pcm16(const float* wave, const float* separated, const float* peak, float compensation, int64_t n,
                                    int16_t* main_out, int16_t* inverted_out, void* stream) {
    if (n < 0) return fail(AICG_E_SHAPE, "aicg_mdx_stems_pcm16: n %lld", (long long)n);
    if (!main_out && !inverted_out) return fail(AICG_E_ARG, "aicg_mdx_stems_pcm16: both outputs are null");
    if (!peak || (n > 0 && (!wave || !separated))) return fail(AICG_E_ARG, "aicg_mdx_stems_pcm16: null pointer");
    if ((((uintptr_t)wave | (uintptr_t)separated) & 3) || (((uintptr_t)main_out | (uintptr_t)inverted_out) & 15))
        return fail(AICG_E_ARG, "aicg_mdx_stems_pcm16: inputs must be 4-byte, outputs 16-byte aligned");
    if (main_out && main_out == inverted_out) return fail(AICG_E_ARG, "aicg_mdx_stems_pcm16: the two outputs are the same buffer");
    if (n == 0) return AICG_OK;
    hipLaunchKernelGGL(mdx_stems_pcm16_kernel, dim3(grid_1d(n / 4)), dim3(256), 0, (hipStream_t)stream, wave, separated, peak,
                       compensation, (long)n, (short*)main_out, (short*)inverted_out);
    return check_launch("mdx_stems_pcm16_kernel");
}
