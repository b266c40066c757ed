// The tail of song_cover_pipeline on the device (reference src/main.py:206-233):
//   * add_audio_effects: pedalboard HighpassFilter -> Compressor(ratio 4, -15 dB) -> Reverb, i.e. JUCE's first-order IIR
//     high-pass, dsp::Compressor with a peak BallisticsFilter, and juce::Reverb (Freeverb);
//   * combine_audio: pydub apply_gain / overlay, i.e. audioop.mul, tostereo, ratecv and add on 16-bit PCM.
// The effects are recurrences.  A call is cut into segments; each segment restarts W samples early from zero state (W from the
// decay constants, chosen by the caller) and only stores its own samples, so that segments run in parallel.  A segment whose
// warm-up would reach the call's start begins there from the carried state instead, so a single-segment call is exactly the
// sequential recurrence.  Float arithmetic follows the JUCE sources operation for operation, without contraction.
// The mix is exact integer / double arithmetic: one thread per output frame, one pass.
#include "common.h"

#pragma clang fp contract(off)

namespace aicg {

// Freeverb tunings at 44.1 kHz (juce::Reverb); the right channel adds kSpread to each
__device__ __host__ inline int fx_comb_tuning(int j) {
    switch (j) {
        case 0: return 1116; case 1: return 1188; case 2: return 1277; case 3: return 1356;
        case 4: return 1422; case 5: return 1491; case 6: return 1557; default: return 1617;
    }
}
__device__ __host__ inline int fx_ap_tuning(int j) {
    switch (j) { case 0: return 556; case 1: return 441; case 2: return 341; default: return 225; }
}
constexpr int kSpread = 23;
constexpr int kCombs = 8, kAps = 4;
constexpr int kHead = 20;                                  // per-channel state header: 8 x last, 8 x comb pos, 4 x all-pass pos
constexpr int kRevThreads = 64;
__device__ __host__ inline int fx_comb_len(int sr, int c, int j) { return (sr * (fx_comb_tuning(j) + c * kSpread)) / 44100; }
__device__ __host__ inline int fx_ap_len(int sr, int c, int j) { return (sr * (fx_ap_tuning(j) + c * kSpread)) / 44100; }

// floats of reverb state per channel (channel 1's delay lines are the longer ones; channel 0 leaves the tail unused)
__host__ inline long fx_reverb_stride(int sr) {
    long s = kHead;
    for (int j = 0; j < kCombs; ++j) s += fx_comb_len(sr, 1, j);
    for (int j = 0; j < kAps; ++j) s += fx_ap_len(sr, 1, j);
    return s;
}
__device__ __host__ inline int fx_reverb_block(int sr) {  // samples per step: no delay line is shorter, so a step reads only older values
    int b = kRevThreads;
    for (int j = 0; j < kCombs; ++j) b = imin(b, fx_comb_len(sr, 0, j));
    for (int j = 0; j < kAps; ++j) b = imin(b, fx_ap_len(sr, 0, j));
    return b;
}

struct FxDynParams {
    float b0, b1, a1;          // high-pass: y = b0 x + s; s = b1 x - a1 y
    float cte_at, cte_rl;      // ballistics: env = e + (e > env ? cte_at : cte_rl) (env - e)
    float thr, thr_inv, ratio_inv;
    int flags;                 // 1: high-pass, 2: compressor
};

// One lane per (segment, channel).  state_in / state_out: [C][2] = (high-pass state, envelope).
__global__ void __launch_bounds__(256) fx_dyn_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ st_in,
                                                     float* __restrict__ st_out, int C, long n, long seg, long warm, int n_seg,
                                                     FxDynParams p) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)n_seg * C) return;
    const int c = (int)(t % C);
    const long g = t / C;
    const long s0 = g * seg, e = lmin(n, s0 + seg);
    long a = s0 - warm;
    float s = 0.f, env = 0.f;
    if (a <= 0) {
        a = 0;
        if (st_in) { s = st_in[2 * c]; env = st_in[2 * c + 1]; }
    }
    const float* xc = x + (long)c * n;
    float* yc = y + (long)c * n;
    for (long i = a; i < e; ++i) {
        float v = xc[i];
        if (p.flags & 1) {
            const float o = p.b0 * v + s;
            s = p.b1 * v - p.a1 * o;
            v = o;
        }
        if (p.flags & 2) {
            const float ab = fabsf(v);
            const float cte = ab > env ? p.cte_at : p.cte_rl;
            env = ab + cte * (env - ab);
            const float gain = env < p.thr ? 1.f : powf(env * p.thr_inv, p.ratio_inv - 1.f);
            v = gain * v;
        }
        if (i >= s0) yc[i] = v;
    }
    if (e == n) { st_out[2 * c] = s; st_out[2 * c + 1] = env; }
}

struct FxRevParams {
    float gain, damp, feedback, wet1, wet2, dry;
};

// One workgroup (one wave) per segment, all channels.  Dynamic LDS per channel: the 8 comb delay lines back to back, then the 4
// all-pass lines; after the channels: x[C][B], comb input[B], comb outputs[C][8][B].
// A step of B samples: (1) stage x and the comb input, (2) lane (c, j) runs comb j of channel c serially over the step (the only
// serial part: `last`), (3) thread t sums sample t's combs in order and runs it through the all-pass chain -- every all-pass read
// in the step is of a value written before the step, since no line is shorter than B -- then mixes wet and dry.
// State layout per channel (stride fx_reverb_stride floats): last[8], comb pos[8], all-pass pos[4] (positions as exact floats),
// comb lines, all-pass lines.
template <int C>
__global__ void __launch_bounds__(kRevThreads) fx_reverb_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                const float* __restrict__ st_in, float* __restrict__ st_out, long n,
                                                                long seg, long warm, int sr, long stride, FxRevParams p) {
    HIP_DYNAMIC_SHARED(float, smem)
    const int tid = threadIdx.x;
    const int B = fx_reverb_block(sr);
    long lines = 0;  // floats of delay line per channel in LDS
    for (int j = 0; j < kCombs; ++j) lines += fx_comb_len(sr, 1, j);
    for (int j = 0; j < kAps; ++j) lines += fx_ap_len(sr, 1, j);
    float* xs = smem + C * lines;
    float* inp = xs + C * B;
    float* co = inp + B;

    const long s0 = (long)blockIdx.x * seg, e = lmin(n, s0 + seg);
    long a = s0 - warm;
    const bool carried = a <= 0;
    if (carried) a = 0;

    // this thread's comb lane (tid < 8 C) and the all-pass positions every thread tracks
    const int lc = tid >> 3, lj = tid & 7;
    const bool comb_lane = tid < kCombs * C;
    int L = 1, cpos = 0, coff = 0;
    float last = 0.f;
    int apos[C][kAps], alen[C][kAps], aoff[C][kAps];
    for (int c = 0; c < C; ++c) {
        int off = 0;
        for (int j = 0; j < kCombs; ++j) {
            const int l = fx_comb_len(sr, c, j);
            if (comb_lane && c == lc && j == lj) { L = l; coff = c * (int)lines + off; }
            off += fx_comb_len(sr, 1, j);
        }
        for (int j = 0; j < kAps; ++j) {
            alen[c][j] = fx_ap_len(sr, c, j);
            aoff[c][j] = c * (int)lines + off;
            off += fx_ap_len(sr, 1, j);
        }
    }
    // initial state: carried, or zero lines at the positions the sequential run has at sample a
    for (int c = 0; c < C; ++c) {
        const float* hs = st_in ? st_in + (long)c * stride : nullptr;
        for (int j = 0; j < kAps; ++j) {
            const long p0 = hs ? (long)hs[16 + j] : 0;
            apos[c][j] = (int)((p0 + (carried ? 0 : a)) % alen[c][j]);
        }
        if (comb_lane && c == lc) {
            const long p0 = hs ? (long)hs[8 + lj] : 0;
            cpos = (int)((p0 + (carried ? 0 : a)) % L);
            last = (carried && hs) ? hs[lj] : 0.f;
        }
        for (long i = tid; i < lines; i += kRevThreads)
            smem[c * lines + i] = (carried && hs) ? hs[kHead + i] : 0.f;
    }
    __syncthreads();

    for (long i0 = a; i0 < e; i0 += B) {
        const int cnt = (int)lmin(B, e - i0);
        if (tid < cnt) {
            const float x0 = x[i0 + tid];
            xs[tid] = x0;
            if (C == 2) {
                const float x1 = x[n + i0 + tid];
                xs[B + tid] = x1;
                inp[tid] = (x0 + x1) * p.gain;
            } else {
                inp[tid] = x0 * p.gain;
            }
        }
        __syncthreads();
        if (comb_lane) {
            float* __restrict__ buf = smem + coff;
            float* __restrict__ out = co + (lc * kCombs + lj) * B;
            const float d1 = 1.0f - p.damp;
            int idx = cpos;
            for (int i = 0; i < cnt; ++i) {
                const float o = buf[idx];
                last = (o * d1) + (last * p.damp);
                buf[idx] = inp[i] + (last * p.feedback);
                out[i] = o;
                idx = idx + 1 == L ? 0 : idx + 1;
            }
            cpos = idx;
        }
        __syncthreads();
        if (tid < cnt) {
            float w[2] = {0.f, 0.f};  // (C == 1 leaves w[1] unused)
            for (int c = 0; c < C; ++c) {
                float s = 0.f;
                for (int j = 0; j < kCombs; ++j) s += co[(c * kCombs + j) * B + tid];
                for (int j = 0; j < kAps; ++j) {
                    int k = apos[c][j] + tid;
                    if (k >= alen[c][j]) k -= alen[c][j];
                    float* ab = smem + aoff[c][j];
                    const float b = ab[k];
                    ab[k] = s + (b * 0.5f);
                    s = b - s;
                }
                w[c] = s;
            }
            if (i0 + tid >= s0) {
                if (C == 2) {
                    y[i0 + tid] = ((w[0] * p.wet1) + (w[1] * p.wet2)) + (xs[tid] * p.dry);
                    y[n + i0 + tid] = ((w[1] * p.wet1) + (w[0] * p.wet2)) + (xs[B + tid] * p.dry);
                } else {
                    y[i0 + tid] = (w[0] * p.wet1) + (xs[tid] * p.dry);
                }
            }
        }
        for (int c = 0; c < C; ++c)
            for (int j = 0; j < kAps; ++j) {
                apos[c][j] += cnt;
                if (apos[c][j] >= alen[c][j]) apos[c][j] -= alen[c][j];
            }
        __syncthreads();
    }

    if (e == n) {  // the last segment hands its state on
        for (int c = 0; c < C; ++c) {
            float* hs = st_out + (long)c * stride;
            for (long i = tid; i < lines; i += kRevThreads) hs[kHead + i] = smem[c * lines + i];
            if (tid < kAps) hs[16 + tid] = (float)apos[c][tid];
            if (comb_lane && c == lc) { hs[lj] = last; hs[8 + lj] = (float)cpos; }
        }
    }
}

// Empty call: the state passes through unchanged (zero when none was given)
__global__ void __launch_bounds__(256) fx_copy_state_kernel(const float* __restrict__ in, float* __restrict__ out, long len) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (long)gridDim.x * blockDim.x) out[i] = in ? in[i] : 0.f;
}

// ---- 16-bit PCM mix (pydub on audioop) ---------------------------------------------------------------------------------------

// audioop.mul, width 2: fbound(sample * factor) -- saturate, then floor
__device__ __forceinline__ int pcm16_mul(int v, double f) {
    double r = (double)v * f;
    if (r > 32767.0) r = 32767.0;
    else if (r < -32767.0) r = -32768.0;
    return (int)floor(r);
}

struct Pcm16Src {
    const short* data;  // [frames][ch]
    long frames;        // frames in the source
    long len;           // frames after conversion (0: the source takes no part)
    int ch;
    long rin, rout;     // gcd-reduced rates of audioop.ratecv (1, 1 = no conversion)
    double g1, g2;      // the two apply_gain factors, in order
};

// Frame m, channel c of src after apply_gain twice, tostereo (factor 1) and ratecv (fresh state, weights 1/0): output m is
// produced after input k = ceil(m rin / rout) has been read, with d = k rout - m rin in [0, rout), prev = input k-1 (0 before the
// first), cur = input k, both scaled by 2^16.
__device__ __forceinline__ int pcm16_conv(const Pcm16Src& s, long m, int c) {
    const int sc = s.ch == 1 ? 0 : c;
    const long k = (m * s.rin + s.rout - 1) / s.rout;
    const long d = k * s.rout - m * s.rin;
    const int cur = pcm16_mul(pcm16_mul(s.data[k * s.ch + sc], s.g1), s.g2) * 65536;
    const int prev = k > 0 ? pcm16_mul(pcm16_mul(s.data[(k - 1) * s.ch + sc], s.g1), s.g2) * 65536 : 0;
    const int v = (int)(((double)prev * (double)d + (double)cur * (double)(s.rout - d)) / (double)s.rout);
    return v >> 16;
}

// a.overlay(b) after pydub's _sync: out has `frames` frames (a's converted length, sliced / zero-padded to pydub's millisecond
// length), b is added with saturation over its converted length, truncated to the output.
__global__ void __launch_bounds__(256) pcm16_overlay_kernel(Pcm16Src a, Pcm16Src b, short* __restrict__ out, long frames, int ch) {
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < frames; m += (long)gridDim.x * blockDim.x) {
        for (int c = 0; c < ch; ++c) {
            int v = m < a.len ? pcm16_conv(a, m, c) : 0;
            if (m < b.len) {
                v += pcm16_conv(b, m, c);
                v = v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
            }
            out[m * ch + c] = (short)v;
        }
    }
}

// float (C, n) -> interleaved 16-bit PCM [n][C]: round to nearest (ties to even) of clamp(x, -1, 1) * 32767
__global__ void __launch_bounds__(256) fx_to_pcm16_kernel(const float* __restrict__ x, short* __restrict__ out, int C, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n * C; i += (long)gridDim.x * blockDim.x) {
        const long f = i / C;
        const int c = (int)(i - f * C);
        double v = (double)x[(long)c * n + f];
        v = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);
        out[i] = (short)(int)rint(v * 32767.0);
    }
}


static long gcd_l(long a, long b) {
    while (b) { const long t = a % b; a = b; b = t; }
    return a;
}

}  // namespace aicg

using namespace aicg;

extern "C" int aicg_fx_reverb_state_size(int sample_rate, int64_t* floats_per_channel) {
    if (!floats_per_channel) return fail(AICG_E_ARG, "aicg_fx_reverb_state_size: null pointer");
    if (sample_rate < 8000 || sample_rate > 384000) return fail(AICG_E_ARG, "aicg_fx_reverb_state_size: sample rate %d", sample_rate);
    *floats_per_channel = fx_reverb_stride(sample_rate);
    return AICG_OK;
}

extern "C" int aicg_fx_dynamics(const float* x, float* y, const float* state_in, float* state_out, int n_channels, int64_t n,
                                int64_t seg_len, int64_t warm, float b0, float b1, float a1, float cte_attack, float cte_release,
                                float threshold, float threshold_inv, float ratio_inv, int flags, void* stream) {
    if (!state_out || (n > 0 && (!x || !y))) return fail(AICG_E_ARG, "aicg_fx_dynamics: null pointer");
    if (state_in == state_out) return fail(AICG_E_ARG, "aicg_fx_dynamics: state_in and state_out must differ");
    if (flags & ~3) return fail(AICG_E_ARG, "aicg_fx_dynamics: flags %d", flags);
    if (n_channels < 1 || n_channels > 2 || n < 0 || warm < 0) return fail(AICG_E_SHAPE, "aicg_fx_dynamics: %d channels, n %lld, warm %lld",
                                                                             n_channels, (long long)n, (long long)warm);
    if (n == 0) {
        hipLaunchKernelGGL(fx_copy_state_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, state_in, state_out, (long)(2 * n_channels));
        return check_launch("fx_copy_state_kernel");
    }
    const long seg = seg_len <= 0 || seg_len > n ? (long)n : (long)seg_len;
    const long n_seg = ((long)n + seg - 1) / seg;
    FxDynParams p{b0, b1, a1, cte_attack, cte_release, threshold, threshold_inv, ratio_inv, flags};
    const long lanes = n_seg * n_channels;
    hipLaunchKernelGGL(fx_dyn_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, state_in,
                       state_out, n_channels, (long)n, seg, (long)warm, (int)n_seg, p);
    return check_launch("fx_dyn_kernel");
}

extern "C" int aicg_fx_reverb(const float* x, float* y, const float* state_in, float* state_out, int n_channels, int64_t n,
                              int sample_rate, int64_t seg_len, int64_t warm, float gain, float damp, float feedback, float wet1,
                              float wet2, float dry, void* stream) {
    if (!state_out || (n > 0 && (!x || !y))) return fail(AICG_E_ARG, "aicg_fx_reverb: null pointer");
    if (state_in == state_out) return fail(AICG_E_ARG, "aicg_fx_reverb: state_in and state_out must differ");
    if (sample_rate < 8000 || sample_rate > 384000) return fail(AICG_E_ARG, "aicg_fx_reverb: sample rate %d", sample_rate);
    if (n_channels < 1 || n_channels > 2 || n < 0 || warm < 0) return fail(AICG_E_SHAPE, "aicg_fx_reverb: %d channels, n %lld, warm %lld",
                                                                           n_channels, (long long)n, (long long)warm);
    const long stride = fx_reverb_stride(sample_rate);
    if (n == 0) {
        hipLaunchKernelGGL(fx_copy_state_kernel, dim3(grid_1d(stride * n_channels)), dim3(256), 0, (hipStream_t)stream, state_in,
                           state_out, stride * n_channels);
        return check_launch("fx_copy_state_kernel");
    }
    const int B = fx_reverb_block(sample_rate);
    const size_t lds = sizeof(float) * ((size_t)n_channels * (stride - kHead) + (size_t)n_channels * B + B + (size_t)n_channels * kCombs * B);
    if (lds > 160 * 1024) return fail(AICG_E_LDS, "aicg_fx_reverb: %zu bytes of delay lines at %d Hz x %d channels", lds, sample_rate, n_channels);
    const long seg = seg_len <= 0 || seg_len > n ? (long)n : (long)seg_len;
    const long n_seg = ((long)n + seg - 1) / seg;
    FxRevParams p{gain, damp, feedback, wet1, wet2, dry};
    auto kern = n_channels == 2 ? fx_reverb_kernel<2> : fx_reverb_kernel<1>;
    allow_dynamic_lds((const void*)kern, lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)n_seg), dim3(kRevThreads), lds, (hipStream_t)stream, x, y, state_in, state_out, (long)n,
                       seg, (long)warm, sample_rate, stride, p);
    return check_launch("fx_reverb_kernel");
}

extern "C" int aicg_fx_to_pcm16(const float* x, int16_t* out, int n_channels, int64_t n, void* stream) {
    if (n > 0 && (!x || !out)) return fail(AICG_E_ARG, "aicg_fx_to_pcm16: null pointer");
    if (n_channels < 1 || n < 0) return fail(AICG_E_SHAPE, "aicg_fx_to_pcm16: %d channels, n %lld", n_channels, (long long)n);
    if (n == 0) return AICG_OK;
    hipLaunchKernelGGL(fx_to_pcm16_kernel, dim3(grid_1d(n * n_channels)), dim3(256), 0, (hipStream_t)stream, x, (short*)out, n_channels, (long)n);
    return check_launch("fx_to_pcm16_kernel");
}

extern "C" int aicg_pcm16_mix(const int16_t* a, int a_channels, int a_rate, int64_t a_frames, double a_gain1, double a_gain2,
                              const int16_t* b, int b_channels, int b_rate, int64_t b_frames, double b_gain1, double b_gain2,
                              int16_t* out, int64_t out_frames, void* stream) {
    if (out_frames > 0 && !out) return fail(AICG_E_ARG, "aicg_pcm16_mix: null pointer");
    if ((a_frames > 0 && !a) || (b_frames > 0 && !b)) return fail(AICG_E_ARG, "aicg_pcm16_mix: null pointer");
    if (a_rate <= 0 || b_rate <= 0) return fail(AICG_E_ARG, "aicg_pcm16_mix: sample rates %d, %d", a_rate, b_rate);
    if (a_channels < 1 || a_channels > 2 || b_channels < 1 || b_channels > 2 || a_frames < 0 || b_frames < 0 || out_frames < 0)
        return fail(AICG_E_SHAPE, "aicg_pcm16_mix: channels %d, %d; frames %lld, %lld, %lld", a_channels, b_channels,
                    (long long)a_frames, (long long)b_frames, (long long)out_frames);
    if (out_frames == 0) return AICG_OK;
    const int ch = imax(a_channels, b_channels);
    const long rate = lmax(a_rate, b_rate);
    auto src = [&](const int16_t* d, int c, long r, long frames, double g1, double g2) {
        Pcm16Src s{(const short*)d, frames, 0, c, 1, 1, g1, g2};
        if (frames > 0) {
            const long g = gcd_l(r, rate);
            if (r != rate) { s.rin = r / g; s.rout = rate / g; }
            s.len = (frames - 1) * s.rout / s.rin + 1;  // audioop.ratecv's output length with a fresh state
        }
        return s;
    };
    const Pcm16Src sa = src(a, a_channels, a_rate, a_frames, a_gain1, a_gain2);
    const Pcm16Src sb = src(b, b_channels, b_rate, b_frames, b_gain1, b_gain2);
    hipLaunchKernelGGL(pcm16_overlay_kernel, dim3(grid_1d(out_frames)), dim3(256), 0, (hipStream_t)stream, sa, sb, (short*)out,
                       (long)out_frames, ch);
    return check_launch("pcm16_overlay_kernel");
}
