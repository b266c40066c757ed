// f0_method "dio" on the device (reference src/vc_infer_pipeline.py:300-309: pyworld.dio, pyworld.stonemask, scipy's medfilt): WORLD's
// DIO -- Morise, Kawahara, Katayose (2009), "Fast and reliable F0 estimation method based on the period extraction of vocal fold
// vibration of singing voice and speech"; Morise et al. (2016), "WORLD" -- restated (tests/world_dio_ref.py):
//   * sum_f64_partials_kernel: the global mean, float64 partial sums added in a fixed order;
//   * dio_lowcut_kernel: the 2 round(sr / 50) + 1 tap low-cut as one FIR pass over the mean-removed signal, written with the margin of
//     2 half[0] samples on either side that the widest band filter reads (nothing is cut between the two filters);
//   * dio_band_kernel<EMIT>: one workgroup per (tile of 1024 samples, band): the Nuttall FIR from one LDS tile plus halo, taps in LDS,
//     float64 accumulation; the four kinds of zero crossing found on the tile and its first difference.  A crossing between sample i and
//     i + 1 belongs to the tile that holds i.  EMIT = false counts them per tile, dio_scan_kernel turns the counts into offsets, EMIT =
//     true filters again and writes (integer sample index, fp32 fraction) in ascending order -- no capacity to overflow;
//   * dio_candidates_kernel: per frame and band the bracketing interval of each kind by binary search, the linear interpolation, the mean
//     and the deviation of the four;
//   * dio_repair_kernel: one workgroup -- best band per frame, the four repair steps; steps 3 and 4 walk on one wave, bands across lanes;
//   * stonemask_kernel: one workgroup per frame, the <= 6 harmonic bins of the two windowed spectra as direct DFT sums;
//   * medfilt3_kernel.
// No atomics, and the sums over a wave and over the whole signal are reduce.h's, which defines their order: two calls give the same bits.
#include "reduce.h"

#include <cmath>

namespace aicg {

constexpr int kDioThreads = 256;
constexpr int kDioTile = 1024;                      // samples a workgroup of the band bank owns (4 a thread)
constexpr int kDioMaxBands = 16;
constexpr int kDioMaxTaps = 2048;                   // the longest filter the LDS tile is laid out for
constexpr int kStoneMaxWindow = 4096;
constexpr double kDioEps = 1e-12;                   // the safeguard in denominators
constexpr float kDioRejected = 1.0e17f;             // 100000 / (0 + 1e-12): the score of a rejected candidate
constexpr double kStoneFloor = 40.0;

struct DioGeom {
    long n, n_frames, n_tiles;
    int n_bands, lowcut, pad, vrm;
    int half[kDioMaxBands];
    double boundary[kDioMaxBands];
    long count_scratch, repair_scratch, index_ints;
};

static int dio_geom(const char* who, int sr, long n, double fp, double fl, double ceil, double cio, DioGeom* g) {
    if (sr < 1000 || sr > 384000) return fail(AICG_E_ARG, "%s: sample rate %d", who, sr);
    if (!(fp > 0.0) || !(fl > 0.0) || !(ceil > fl) || ceil > 0.5 * sr || !(cio > 0.0))
        return fail(AICG_E_ARG, "%s: frame period %g ms, range %g .. %g at %d Hz, %g channels an octave", who, fp, fl, ceil, sr, cio);
    if (n < 0 || n >= (1L << 31) / (2 * kDioMaxBands)) return fail(AICG_E_SHAPE, "%s: n %ld", who, n);   // event offsets are 32-bit
    g->n = n;
    g->n_frames = (long)(1000.0 * (double)n / (double)sr / fp) + 1;
    const long nb = 1 + (long)(log2(ceil / fl) * cio);
    if (nb < 1 || nb > kDioMaxBands) return fail(AICG_E_SHAPE, "%s: %ld bands (1 .. %d)", who, nb, kDioMaxBands);
    g->n_bands = (int)nb;
    for (int b = 0; b < g->n_bands; ++b) {
        g->boundary[b] = fl * pow(2.0, ((double)b + 1.0) / cio);
        g->half[b] = (int)mround((double)sr / g->boundary[b] / 2.0);
        if (g->half[b] < 1 || 4 * g->half[b] > kDioMaxTaps)
            return fail(AICG_E_SHAPE, "%s: band %d needs %d taps (4 .. %d)", who, b, 4 * g->half[b], kDioMaxTaps);
    }
    g->lowcut = 2 * (int)mround((double)sr / 50.0) + 1;
    if (g->lowcut > kDioMaxTaps) return fail(AICG_E_SHAPE, "%s: a low-cut of %d taps at %d Hz (at most %d)", who, g->lowcut, sr, kDioMaxTaps);
    g->pad = 2 * g->half[0];
    g->vrm = 2 * (int)(0.5 + 1000.0 / fp / fl) + 1;
    g->n_tiles = lmax(1, ldiv_up(n, (long)kDioTile));
    g->count_scratch = (long)sizeof(double) * kSumPartials + (long)sizeof(float) * (n + 2 * g->pad);
    g->repair_scratch = g->n_frames * 16 + 64;
    g->index_ints = 2 * 4 * g->n_bands * g->n_tiles + 4 * g->n_bands + 1;
    return AICG_OK;
}

// ---- low-cut --------------------------------------------------------------------------------------------------------------------
// out[j] = sum_k tr[k] xs[j + k], float64, for the j this thread owns (j = tid, tid + 256, ...)
__device__ __forceinline__ double dio_fir_at(const double* tr, const double* xs, int K, int j) {
    double a0 = 0.0, a1 = 0.0;
    int k = 0;
    for (; k + 1 < K; k += 2) {
        a0 = fma(tr[k], xs[j + k], a0);
        a1 = fma(tr[k + 1], xs[j + k + 1], a1);
    }
    if (k < K) a0 = fma(tr[k], xs[j + k], a0);
    return a0 + a1;
}

// lc[q] = the low-cut signal at position q - pad, q in [0, n + 2 pad): sum_k h[k] y(p + c - k), y = x - mean inside [0, n), 0 outside
__global__ void __launch_bounds__(kDioThreads) dio_lowcut_kernel(const float* __restrict__ x, long n, const double* __restrict__ part,
                                                                 const double* __restrict__ taps, int N, int pad, float* __restrict__ lc) {
    HIP_DYNAMIC_SHARED(double, smem)
    double* tr = smem;              // [N] reversed taps
    double* xs = smem + N;          // [kDioTile + N - 1]
    const int tid = threadIdx.x, c = (N - 1) / 2;
    const double mean = sum_of_partials(part, kSumPartials) / (double)n;
    const long q0 = (long)blockIdx.x * kDioTile, total = n + 2 * (long)pad;
    for (int k = tid; k < N; k += kDioThreads) tr[k] = taps[N - 1 - k];
    for (int m = tid; m < kDioTile + N - 1; m += kDioThreads) {
        const long j = q0 - pad - c + m;
        xs[m] = (j >= 0 && j < n) ? (double)x[j] - mean : 0.0;
    }
    __syncthreads();
    for (int j = tid; j < kDioTile; j += kDioThreads)
        if (q0 + j < total) lc[q0 + j] = (float)dio_fir_at(tr, xs, N, j);
}

// ---- the band bank and the crossings -------------------------------------------------------------------------------------------------
struct DioBands {
    int n_bands, pad;
    int half[kDioMaxBands];
    int tap_off[kDioMaxBands];      // where band b's 4 half[b] taps start in the table
};

// counts of the four kinds in 16 bits each
__device__ __forceinline__ unsigned dio_scan_wave(unsigned v) {
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(v, o, 64);
        if ((int)(threadIdx.x & 63) >= o) v += t;
    }
    return v;
}

template <bool EMIT>
__global__ void __launch_bounds__(kDioThreads) dio_band_kernel(const float* __restrict__ lc, long n, const double* __restrict__ taps, DioBands bp,
                                                               long n_tiles, int* __restrict__ counts, const int* __restrict__ offs,
                                                               int* __restrict__ ev_ip, float* __restrict__ ev_fr, float* __restrict__ band_out) {
    HIP_DYNAMIC_SHARED(double, smem)
    __shared__ unsigned wtot[2][4];
    const int tid = threadIdx.x, band = blockIdx.y, h = bp.half[band], K = 4 * h;
    const long tile = blockIdx.x, i0 = tile * kDioTile, total = n + 2 * (long)bp.pad;
    double* tr = smem;                                                  // [K]
    double* xs = smem + K;                                              // [kDioTile + 2 + K - 1]
    float* sf = reinterpret_cast<float*>(xs + kDioTile + 2 + K - 1);    // [kDioTile + 2]: s(i0 + j)
    for (int k = tid; k < K; k += kDioThreads) tr[k] = taps[bp.tap_off[band] + K - 1 - k];
    for (int m = tid; m < kDioTile + 2 + K - 1; m += kDioThreads) {
        const long q = i0 + 2 * h - K + 1 + m + bp.pad;                 // index into lc of position i0 + 2 h - K + 1 + m
        xs[m] = (q >= 0 && q < total) ? (double)lc[q] : 0.0;
    }
    __syncthreads();
    for (int j = tid; j < kDioTile + 2; j += kDioThreads) {
        const float v = i0 + j < n ? (float)dio_fir_at(tr, xs, K, j) : 0.f;
        sf[j] = v;
        if (band_out && j < kDioTile && i0 + j < n) band_out[(long)band * n + i0 + j] = v;
    }
    __syncthreads();
    // four samples a thread; kind 0 / 1: s, -s (needs i + 1 < n); kind 2 / 3: the forward difference and its negative (needs i + 2 < n)
    unsigned c01 = 0, c23 = 0;
    unsigned char hit[4];
    float fr01[4], fr23[4];
    for (int e = 0; e < 4; ++e) {
        const int j = 4 * tid + e;
        const long i = i0 + j;
        const float a = sf[j], b = sf[j + 1], c = sf[j + 2];
        const float d0 = b - a, d1 = c - b;
        unsigned m = 0;
        if (i + 1 < n) m |= (a > 0.f && b <= 0.f) ? 1u : ((a < 0.f && b >= 0.f) ? 2u : 0u);
        if (i + 2 < n) m |= (d0 > 0.f && d1 <= 0.f) ? 4u : ((d0 < 0.f && d1 >= 0.f) ? 8u : 0u);
        hit[e] = (unsigned char)m;
        fr01[e] = (m & 3u) ? a / (a - b) : 0.f;
        fr23[e] = (m & 12u) ? d0 / (d0 - d1) : 0.f;
        c01 += (m & 1u) + ((m & 2u) << 15);
        c23 += ((m & 4u) >> 2) + ((m & 8u) << 13);
    }
    const unsigned i01 = dio_scan_wave(c01), i23 = dio_scan_wave(c23);
    if ((tid & 63) == 63) { wtot[0][tid >> 6] = i01; wtot[1][tid >> 6] = i23; }
    __syncthreads();
    unsigned b01 = 0, b23 = 0, t01 = 0, t23 = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < (tid >> 6)) { b01 += wtot[0][w]; b23 += wtot[1][w]; }
        t01 += wtot[0][w]; t23 += wtot[1][w];
    }
    const long row = (long)band * 4;
    if (!EMIT) {
        if (tid == 0) {
            counts[(row + 0) * n_tiles + tile] = (int)(t01 & 0xffffu);
            counts[(row + 1) * n_tiles + tile] = (int)(t01 >> 16);
            counts[(row + 2) * n_tiles + tile] = (int)(t23 & 0xffffu);
            counts[(row + 3) * n_tiles + tile] = (int)(t23 >> 16);
        }
    } else {
        const unsigned e01 = b01 + i01 - c01, e23 = b23 + i23 - c23;    // exclusive prefixes
        long at[4] = {offs[(row + 0) * n_tiles + tile] + (long)(e01 & 0xffffu), offs[(row + 1) * n_tiles + tile] + (long)(e01 >> 16),
                      offs[(row + 2) * n_tiles + tile] + (long)(e23 & 0xffffu), offs[(row + 3) * n_tiles + tile] + (long)(e23 >> 16)};
        for (int e = 0; e < 4; ++e) {
            const int ip = (int)(i0 + 4 * tid + e + 1);                 // one-based index of sample i
            const unsigned m = hit[e];
            if (m & 1u) { ev_ip[at[0]] = ip; ev_fr[at[0]++] = fr01[e]; }
            if (m & 2u) { ev_ip[at[1]] = ip; ev_fr[at[1]++] = fr01[e]; }
            if (m & 4u) { ev_ip[at[2]] = ip; ev_fr[at[2]++] = fr23[e]; }
            if (m & 8u) { ev_ip[at[3]] = ip; ev_fr[at[3]++] = fr23[e]; }
        }
    }
}

// exclusive scan of counts[rows * n_tiles] as one vector; row_start[r] = offs[r n_tiles], row_start[rows] = the total
__global__ void __launch_bounds__(64) dio_scan_kernel(const int* __restrict__ counts, int* __restrict__ offs, int* __restrict__ row_start, int rows,
                                                      long n_tiles) {
    const int lane = threadIdx.x;
    const long total = (long)rows * n_tiles;
    unsigned run = 0;
    for (long e0 = 0; e0 < total; e0 += 64) {
        const long e = e0 + lane;
        const unsigned c = e < total ? (unsigned)counts[e] : 0u;
        const unsigned inc = dio_scan_wave(c);
        if (e < total) {
            offs[e] = (int)(run + inc - c);
            if (e % n_tiles == 0) row_start[e / n_tiles] = (int)(run + inc - c);
        }
        run += __shfl(inc, 63, 64);
    }
    if (lane == 0) row_start[rows] = (int)run;
}

// ---- candidates ---------------------------------------------------------------------------------------------------------------------
struct DioCandParams {
    long n_frames;
    int n_bands;
    double fs, frame_period;
    float floor_hz, ceil_hz;
    float boundary[kDioMaxBands];
};

// twice the location of interval k (between crossings k and k + 1), in samples
__device__ __forceinline__ double dio_loc2(const int* ip, const float* fr, int k) {
    return (double)(ip[k] + ip[k + 1]) + (double)fr[k] + (double)fr[k + 1];
}
__device__ __forceinline__ float dio_interval_f0(const int* ip, const float* fr, int k, float fs) {
    return fs / ((float)(ip[k + 1] - ip[k]) + (fr[k + 1] - fr[k]));
}

__global__ void __launch_bounds__(256) dio_candidates_kernel(const int* __restrict__ ev_ip, const float* __restrict__ ev_fr,
                                                             const int* __restrict__ row_start, float* __restrict__ cand,
                                                             float* __restrict__ score, DioCandParams p) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n_frames) return;
    const double tpos = (double)i * p.frame_period / 1000.0 * p.fs;
    for (int b = 0; b < p.n_bands; ++b) {
        float y[4];
        bool voiced = true;
        for (int kind = 0; kind < 4; ++kind) voiced = voiced && (row_start[b * 4 + kind + 1] - row_start[b * 4 + kind] - 1 > 2);
        float c = 0.f, sc = kDioRejected;
        if (voiced) {
            for (int kind = 0; kind < 4; ++kind) {
                const int r0 = row_start[b * 4 + kind], m = row_start[b * 4 + kind + 1] - r0 - 1;    // m intervals
                const int* ip = ev_ip + r0;
                const float* fr = ev_fr + r0;
                int lo = 0, hi = m;                       // the number of locations <= tpos
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (dio_loc2(ip, fr, mid) <= 2.0 * tpos) lo = mid + 1; else hi = mid;
                }
                const int j = imin(imax(lo - 1, 0), m - 2);
                const double l0 = 0.5 * dio_loc2(ip, fr, j), l1 = 0.5 * dio_loc2(ip, fr, j + 1);
                const float s = (float)((tpos - l0) / (l1 - l0));
                const float f0 = dio_interval_f0(ip, fr, j, (float)p.fs), f1 = dio_interval_f0(ip, fr, j + 1, (float)p.fs);
                y[kind] = f0 + s * (f1 - f0);
            }
            c = (((y[0] + y[1]) + y[2]) + y[3]) / 4.f;
            const float e0 = y[0] - c, e1 = y[1] - c, e2 = y[2] - c, e3 = y[3] - c;
            const float sd = sqrtf((((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3) / 3.f);
            const float B = p.boundary[b];
            const bool bad = c > B || c < B / 2.f || c > p.ceil_hz || c < p.floor_hz || !(fabsf(c) <= 3.0e38f);
            sc = bad ? kDioRejected : sd / (c + (float)kDioEps);
            c = bad ? 0.f : c;
        }
        cand[(long)b * p.n_frames + i] = c;
        score[(long)b * p.n_frames + i] = sc;
    }
}

// ---- best contour and repair -----------------------------------------------------------------------------------------------------------
// One extension (steps 3 and 4) on wave 0: from frame `from` in direction `step` up to `limit`, the band candidate nearest
// (3 f[j] - f[j - step]) / 2, stopping when it is further than allowed_range (relative).  Bands across lanes, first minimum.
__device__ __forceinline__ void dio_extend(double* f, const float* __restrict__ cand, long L, int nb, long from, long limit, int step,
                                           double allowed, int lane) {
#pragma clang fp contract(off)
    if (from == limit) return;
    double cur = f[from], past = f[from - step];
    float cn = lane < nb ? cand[(long)lane * L + from + step] : 0.f;
    for (long j = from; j != limit; j += step) {
        const long t = j + step;
        const double cv = (double)cn;
        if (t != limit && lane < nb) cn = cand[(long)lane * L + t + step];      // the next frame's candidates are on their way
        const double ref = (3.0 * cur - past) / 2.0;
        double err = lane < nb ? fabs(ref - cv) : INFINITY, best = cv;
        int idx = lane;
        for (int o = 1; o < kDioMaxBands; o <<= 1) {
            const double oe = __shfl_xor(err, o, 64), ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(idx, o, 64);
            if (oe < err || (oe == err && oi < idx)) { err = oe; best = ob; idx = oi; }
        }
        best = __shfl(best, 0, 64);
        if (!(fabs(1.0 - best / ref) <= allowed)) best = 0.0;
        if (lane == 0) f[t] = best;
        if (best == 0.0) break;
        past = cur;
        cur = best;
    }
    __threadfence();   // lane 0's stores are read by every lane at the start of the next extension
}

__global__ void __launch_bounds__(256) dio_repair_kernel(const float* __restrict__ cand, const float* __restrict__ score, int nb, long L, int vrm,
                                                         double allowed, double* __restrict__ fa, int* __restrict__ ends, int* __restrict__ starts,
                                                         double* __restrict__ f0_out) {
#pragma clang fp contract(off)
    __shared__ unsigned wt[2][4];
    __shared__ unsigned base_s[2];
    const int tid = threadIdx.x;
    if (L <= vrm) {
        for (long i = tid; i < L; i += 256) f0_out[i] = 0.0;
        return;
    }
    // best band (first minimum of the score), with the first and last vrm frames zeroed: step 1's base
    for (long i = tid; i < L; i += 256) {
        float bs = score[i], bc = cand[i];
        for (int b = 1; b < nb; ++b) {
            const float s = score[(long)b * L + i];
            if (bs > s) { bs = s; bc = cand[(long)b * L + i]; }
        }
        f0_out[i] = (i < vrm || i >= L - vrm) ? 0.0 : (double)bc;
    }
    __syncthreads();
    // step 1: a frame whose relative jump from its predecessor reaches allowed_range goes
    for (long i = tid; i < L; i += 256) {
        double v = 0.0;
        if (i >= vrm) {
            const double a = f0_out[i], b = f0_out[i - 1];
            v = fabs((a - b) / (kDioEps + a)) < allowed ? a : 0.0;
        }
        fa[i] = v;
    }
    __syncthreads();
    // step 2: a frame stays only if every frame within (vrm - 1) / 2 of it is voiced
    const int c = (vrm - 1) / 2;
    for (long i = tid; i < L; i += 256) {
        double v = fa[i];
        if (i >= c && i < L - c)
            for (int j = -c; j <= c; ++j)
                if (fa[i + j] == 0.0) { v = 0.0; break; }
        f0_out[i] = v;
    }
    if (tid < 2) base_s[tid] = 0;
    __syncthreads();
    // section ends (last voiced frame) and starts (first voiced frame), ascending
    for (long i0 = 0; i0 < L; i0 += 256) {
        const long i = i0 + tid;
        const bool in = i >= 1 && i < L;
        const double a = in ? f0_out[i] : 0.0, b = in ? f0_out[i - 1] : 0.0;
        const unsigned e = in && a == 0.0 && b != 0.0, s = in && b == 0.0 && a != 0.0;
        const unsigned v = e | (s << 16), inc = dio_scan_wave(v);
        if ((tid & 63) == 63) wt[0][tid >> 6] = inc;
        __syncthreads();
        unsigned before = 0, all = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < (tid >> 6)) before += wt[0][w];
            all += wt[0][w];
        }
        const unsigned ex = before + inc - v;
        if (e) ends[base_s[0] + (ex & 0xffffu)] = (int)(i - 1);
        if (s) starts[base_s[1] + (ex >> 16)] = (int)i;
        __syncthreads();
        if (tid == 0) { base_s[0] += all & 0xffffu; base_s[1] += all >> 16; }
        __syncthreads();
    }
    const int n_ends = (int)base_s[0], n_starts = (int)base_s[1];
    // steps 3 and 4 in place, one wave
    if (tid < 64) {
        for (int s = 0; s < n_ends; ++s)
            dio_extend(f0_out, cand, L, nb, ends[s], s == n_ends - 1 ? L - 1 : (long)ends[s + 1], 1, allowed, tid);
        for (int s = n_starts - 1; s >= 0; --s)
            dio_extend(f0_out, cand, L, nb, starts[s], s == 0 ? 1L : (long)starts[s - 1], -1, allowed, tid);
    }
}

// ---- StoneMask -----------------------------------------------------------------------------------------------------------------------
struct StoneParams {
    long n, n_frames;
    double fs, frame_period;
};

// the amplitude-weighted instantaneous frequency over nh harmonics of f (P, Q: power and cross term of the bins, in the order asked)
__device__ __forceinline__ double stone_fix(const float* P, const float* Q, const int* bin, int nh, int fft_size, double fs) {
#pragma clang fp contract(off)
    float num = 0.f, den = 0.f;
    for (int k = 1; k <= nh; ++k) {
        const float p = P[k - 1];
        const float inst = p == 0.f ? 0.f : (float)((double)bin[k - 1] * fs / (double)fft_size) + Q[k - 1] / p * (float)(fs / 2.0 / 3.14159265358979323846);
        const float a = sqrtf(p);
        num += a * inst;
        den += a * (float)k;
    }
    return (double)num / ((double)den + kDioEps);
}

__global__ void __launch_bounds__(kDioThreads) stonemask_kernel(const float* __restrict__ x, const double* __restrict__ f0_in,
                                                                double* __restrict__ f0_out, StoneParams p) {
#pragma clang fp contract(off)
    __shared__ float wa[kStoneMaxWindow], wd[kStoneMaxWindow], wn[kStoneMaxWindow];
    __shared__ float red[4][4];
    __shared__ float P[6], Q[6];
    __shared__ int bin[6];
    __shared__ double tent_s;
    const int tid = threadIdx.x;
    for (long fi = blockIdx.x; fi < p.n_frames; fi += gridDim.x) {
        const double f0 = f0_in[fi];
        if (!(f0 > kStoneFloor && f0 <= p.fs / 12.0)) {
            if (tid == 0) f0_out[fi] = 0.0;
            continue;
        }
        const double t = (double)fi * p.frame_period / 1000.0;
        const int half = (int)(1.5 * p.fs / f0 + 1.0), W = 2 * half + 1;
        const int fft_size = 1 << (2 + (31 - __builtin_clz((unsigned)W)));
        const long idx0 = mround((t - (double)half / p.fs) * p.fs + 0.001);
        for (int j = tid; j < W; j += kDioThreads) {
            const double tm = (((double)(idx0 + j) - 1.0) / p.fs - t) / ((double)W / p.fs);
            wn[j] = (float)(0.42 + 0.5 * cos(2.0 * 3.14159265358979323846 * tm) + 0.08 * cos(4.0 * 3.14159265358979323846 * tm));
        }
        __syncthreads();
        for (int j = tid; j < W; j += kDioThreads) {
            const float v = x[lmax(0, lmin(p.n - 1, idx0 + j - 1))];
            const float d = j == 0 ? -wn[1] / 2.f : (j == W - 1 ? wn[W - 2] / 2.f : -(wn[j + 1] - wn[j - 1]) / 2.f);
            wa[j] = v * wn[j];
            wd[j] = v * d;
        }
        __syncthreads();
        double f = f0, result = 0.0;
        for (int pass = 0; pass < 2; ++pass) {
            const int nh = pass == 0 ? 2 : imin((int)(p.fs / 2.0 / f), 6);
            for (int k = 1; k <= nh; ++k) {
                const int b = (int)mround(f * (double)fft_size / p.fs * (double)k);
                float re = 0.f, im = 0.f, dre = 0.f, dim = 0.f;
                for (int j = tid; j < W; j += kDioThreads) {
                    const int r = (int)(((long)b * j) & (fft_size - 1));
                    float sn, cs;
                    sincospif(2.f * (float)r / (float)fft_size, &sn, &cs);
                    re += wa[j] * cs; im -= wa[j] * sn;
                    dre += wd[j] * cs; dim -= wd[j] * sn;
                }
                for (int o = 32; o > 0; o >>= 1) {   // four of reduce.h's wave_sum, interleaved
                    re += __shfl_xor(re, o, 64); im += __shfl_xor(im, o, 64);
                    dre += __shfl_xor(dre, o, 64); dim += __shfl_xor(dim, o, 64);
                }
                if ((tid & 63) == 0) { red[tid >> 6][0] = re; red[tid >> 6][1] = im; red[tid >> 6][2] = dre; red[tid >> 6][3] = dim; }
                __syncthreads();
                if (tid == 0) {
                    const float R = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0], I = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
                    const float DR = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2], DI = ((red[0][3] + red[1][3]) + red[2][3]) + red[3][3];
                    P[k - 1] = R * R + I * I;
                    Q[k - 1] = R * DI - I * DR;
                    bin[k - 1] = b;
                }
                __syncthreads();
            }
            if (tid == 0) tent_s = stone_fix(P, Q, bin, nh, fft_size, p.fs);
            __syncthreads();
            const double got = tent_s;
            __syncthreads();
            if (pass == 0) {
                if (!(got > 0.0 && got <= 2.0 * f0)) break;     // the first estimate is rejected: the result stays 0
                f = got;
            } else {
                result = got;
            }
        }
        if (result <= 0.0 || result > p.fs / 12.0 || fabs(result - f0) > 0.2 * f0) result = f0;
        if (tid == 0) f0_out[fi] = result;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) medfilt3_kernel(const double* __restrict__ in, double* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double a = i > 0 ? in[i - 1] : 0.0, b = in[i], c = i + 1 < n ? in[i + 1] : 0.0;
    out[i] = fmax(fmin(a, b), fmin(fmax(a, b), c));
}

static int dio_launch_repair(const float* cand, const float* score, int n_bands, long n_frames, int vrm, double allowed, void* scratch,
                             double* f0_out, hipStream_t st) {
    double* fa = (double*)scratch;
    int* ends = (int*)(fa + n_frames);
    int* starts = ends + n_frames + 4;
    hipLaunchKernelGGL(dio_repair_kernel, dim3(1), dim3(256), 0, st, cand, score, n_bands, n_frames, vrm, allowed, fa, ends, starts, f0_out);
    return check_launch("dio_repair_kernel");
}

}  // namespace aicg

using namespace aicg;

extern "C" int aicg_world_dio_geometry(int sample_rate, int64_t n, double frame_period, double f0_floor, double f0_ceil, double channels_in_octave,
                                       int64_t* geom, double* boundary) {
    if (!geom || !boundary) return fail(AICG_E_ARG, "aicg_world_dio_geometry: null pointer");
    DioGeom g;
    const int rc = dio_geom("aicg_world_dio_geometry", sample_rate, (long)n, frame_period, f0_floor, f0_ceil, channels_in_octave, &g);
    if (rc != AICG_OK) return rc;
    geom[0] = g.n_frames; geom[1] = g.n_bands; geom[2] = g.n_tiles; geom[3] = g.lowcut; geom[4] = g.pad; geom[5] = g.vrm;
    geom[6] = g.count_scratch; geom[7] = g.repair_scratch; geom[8] = g.index_ints; geom[9] = kDioTile;
    for (int b = 0; b < kDioMaxBands; ++b) {
        geom[10 + b] = b < g.n_bands ? g.half[b] : 0;
        boundary[b] = b < g.n_bands ? g.boundary[b] : 0.0;
    }
    return AICG_OK;
}

static void dio_bands(const DioGeom& g, DioBands* bp) {
    bp->n_bands = g.n_bands;
    bp->pad = g.pad;
    int off = g.lowcut;
    for (int b = 0; b < kDioMaxBands; ++b) {
        bp->half[b] = b < g.n_bands ? g.half[b] : 0;
        bp->tap_off[b] = off;
        off += 4 * bp->half[b];
    }
}

static size_t dio_band_lds(int half) { return sizeof(double) * (size_t)(4 * half + kDioTile + 2 + 4 * half - 1) + sizeof(float) * (kDioTile + 2); }

extern "C" int aicg_world_dio_count(const float* x, int64_t n, int sample_rate, double frame_period, double f0_floor, double f0_ceil,
                                    double channels_in_octave, const double* taps, void* scratch, int* index, float* band_out, void* stream) {
    DioGeom g;
    const int rc = dio_geom("aicg_world_dio_count", sample_rate, (long)n, frame_period, f0_floor, f0_ceil, channels_in_octave, &g);
    if (rc != AICG_OK) return rc;
    if (!taps || !scratch || !index || (n > 0 && !x)) return fail(AICG_E_ARG, "aicg_world_dio_count: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rows = 4 * g.n_bands;
    int* counts = index;
    int* offs = index + (long)rows * g.n_tiles;
    int* row_start = offs + (long)rows * g.n_tiles;
    if (n == 0) {
        (void)hipMemsetAsync(index, 0, sizeof(int) * (size_t)g.index_ints, st);
        return AICG_OK;
    }
    double* part = (double*)scratch;
    float* lc = (float*)(part + kSumPartials);
    hipLaunchKernelGGL(sum_f64_partials_kernel, dim3(kSumPartials), dim3(256), 0, st, x, (long)n, part);
    int rc2 = check_launch("sum_f64_partials_kernel");
    if (rc2 != AICG_OK) return rc2;
    const size_t lds_lc = sizeof(double) * (size_t)(2 * g.lowcut + kDioTile - 1);
    allow_dynamic_lds((const void*)dio_lowcut_kernel, lds_lc);
    hipLaunchKernelGGL(dio_lowcut_kernel, dim3((unsigned)ldiv_up(n + 2 * (long)g.pad, (long)kDioTile)), dim3(kDioThreads), lds_lc, st, x, (long)n,
                       (const double*)part, taps, g.lowcut, g.pad, lc);
    rc2 = check_launch("dio_lowcut_kernel");
    if (rc2 != AICG_OK) return rc2;
    DioBands bp;
    dio_bands(g, &bp);
    const size_t lds = dio_band_lds(g.half[0]);
    allow_dynamic_lds((const void*)dio_band_kernel<false>, lds);
    hipLaunchKernelGGL(dio_band_kernel<false>, dim3((unsigned)g.n_tiles, (unsigned)g.n_bands), dim3(kDioThreads), lds, st, (const float*)lc, (long)n,
                       taps, bp, g.n_tiles, counts, (const int*)offs, (int*)nullptr, (float*)nullptr, band_out);
    rc2 = check_launch("dio_band_kernel");
    if (rc2 != AICG_OK) return rc2;
    hipLaunchKernelGGL(dio_scan_kernel, dim3(1), dim3(64), 0, st, (const int*)counts, offs, row_start, rows, g.n_tiles);
    return check_launch("dio_scan_kernel");
}

extern "C" int aicg_world_dio(int64_t n, int sample_rate, double frame_period, double f0_floor, double f0_ceil, double channels_in_octave,
                              double allowed_range, const double* taps, const void* scratch, const int* index, int64_t n_events, int* ev_ip,
                              float* ev_fr, void* repair_scratch, float* cand, float* score, double* f0_out, void* stream) {
    DioGeom g;
    const int rc = dio_geom("aicg_world_dio", sample_rate, (long)n, frame_period, f0_floor, f0_ceil, channels_in_octave, &g);
    if (rc != AICG_OK) return rc;
    if (!(allowed_range > 0.0)) return fail(AICG_E_ARG, "aicg_world_dio: allowed range %g", allowed_range);
    if (n_events < 0 || n_events > 2 * (int64_t)(n + 4) * g.n_bands) return fail(AICG_E_ARG, "aicg_world_dio: %lld events", (long long)n_events);
    if (!taps || !scratch || !index || !ev_ip || !ev_fr || !repair_scratch || !cand || !score || !f0_out)
        return fail(AICG_E_ARG, "aicg_world_dio: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rows = 4 * g.n_bands;
    const int* offs = index + (long)rows * g.n_tiles;
    const int* row_start = offs + (long)rows * g.n_tiles;
    if (n > 0 && n_events > 0) {
        const float* lc = (const float*)((const double*)scratch + kSumPartials);
        DioBands bp;
        dio_bands(g, &bp);
        const size_t lds = dio_band_lds(g.half[0]);
        allow_dynamic_lds((const void*)dio_band_kernel<true>, lds);
        hipLaunchKernelGGL(dio_band_kernel<true>, dim3((unsigned)g.n_tiles, (unsigned)g.n_bands), dim3(kDioThreads), lds, st, lc, (long)n, taps, bp,
                           g.n_tiles, (int*)nullptr, offs, ev_ip, ev_fr, (float*)nullptr);
        const int rc2 = check_launch("dio_band_kernel");
        if (rc2 != AICG_OK) return rc2;
    }
    DioCandParams p;
    p.n_frames = g.n_frames; p.n_bands = g.n_bands; p.fs = (double)sample_rate; p.frame_period = frame_period;
    p.floor_hz = (float)f0_floor; p.ceil_hz = (float)f0_ceil;
    for (int b = 0; b < kDioMaxBands; ++b) p.boundary[b] = b < g.n_bands ? (float)g.boundary[b] : 0.f;
    hipLaunchKernelGGL(dio_candidates_kernel, dim3((unsigned)ldiv_up(g.n_frames, 256L)), dim3(256), 0, st, (const int*)ev_ip, (const float*)ev_fr,
                       row_start, cand, score, p);
    const int rc3 = check_launch("dio_candidates_kernel");
    if (rc3 != AICG_OK) return rc3;
    return dio_launch_repair(cand, score, g.n_bands, g.n_frames, g.vrm, allowed_range, repair_scratch, f0_out, st);
}

extern "C" int aicg_world_dio_repair(const float* cand, const float* score, int n_bands, int64_t n_frames, double frame_period, double f0_floor,
                                     double allowed_range, void* scratch, double* f0_out, void* stream) {
    if (n_bands < 1 || n_bands > kDioMaxBands) return fail(AICG_E_SHAPE, "aicg_world_dio_repair: %d bands (1 .. %d)", n_bands, kDioMaxBands);
    if (n_frames < 0 || n_frames >= (1L << 31)) return fail(AICG_E_SHAPE, "aicg_world_dio_repair: %lld frames", (long long)n_frames);
    if (!(frame_period > 0.0) || !(f0_floor > 0.0) || !(allowed_range > 0.0))
        return fail(AICG_E_ARG, "aicg_world_dio_repair: frame period %g, floor %g, allowed range %g", frame_period, f0_floor, allowed_range);
    if (n_frames == 0) return AICG_OK;
    if (!cand || !score || !scratch || !f0_out) return fail(AICG_E_ARG, "aicg_world_dio_repair: null pointer");
    const int vrm = 2 * (int)(0.5 + 1000.0 / frame_period / f0_floor) + 1;
    return dio_launch_repair(cand, score, n_bands, (long)n_frames, vrm, allowed_range, scratch, f0_out, (hipStream_t)stream);
}

extern "C" int aicg_stonemask(const float* x, int64_t n, int sample_rate, double frame_period, const double* f0, int64_t n_frames, double* f0_out,
                              void* stream) {
    if (sample_rate < 1000 || sample_rate > 384000 || !(frame_period > 0.0)) return fail(AICG_E_ARG, "aicg_stonemask: %d Hz, frame period %g", sample_rate, frame_period);
    if (n < 1 || n >= (1L << 40) || n_frames < 0 || n_frames >= (1L << 31)) return fail(AICG_E_SHAPE, "aicg_stonemask: n %lld, %lld frames", (long long)n, (long long)n_frames);
    if (2 * (long)(1.5 * sample_rate / kStoneFloor + 1.0) + 1 > kStoneMaxWindow)
        return fail(AICG_E_SHAPE, "aicg_stonemask: the window at %d Hz is above %d samples", sample_rate, kStoneMaxWindow);
    if (n_frames == 0) return AICG_OK;
    if (!x || !f0 || !f0_out) return fail(AICG_E_ARG, "aicg_stonemask: null pointer");
    StoneParams p;
    p.n = (long)n; p.n_frames = (long)n_frames; p.fs = (double)sample_rate; p.frame_period = frame_period;
    hipLaunchKernelGGL(stonemask_kernel, dim3((unsigned)lmin((long)n_frames, 4096L)), dim3(kDioThreads), 0, (hipStream_t)stream, x, f0, f0_out, p);
    return check_launch("stonemask_kernel");
}

extern "C" int aicg_medfilt3(const double* f0, int64_t n, double* out, void* stream) {
    if (n < 0 || n >= (1L << 40)) return fail(AICG_E_SHAPE, "aicg_medfilt3: n %lld", (long long)n);
    if (n == 0) return AICG_OK;
    if (!f0 || !out || f0 == out) return fail(AICG_E_ARG, "aicg_medfilt3: null or aliased pointer");
    hipLaunchKernelGGL(medfilt3_kernel, dim3((unsigned)ldiv_up((long)n, 256L)), dim3(256), 0, (hipStream_t)stream, f0, out, (long)n);
    return check_launch("medfilt3_kernel");
}
