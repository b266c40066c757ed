// f0_method "pm" on the device (reference src/vc_infer_pipeline.py:279-294, parselmouth's Sound.to_pitch_ac): Praat's autocorrelation
// pitch -- Boersma (1993), "Accurate short-term analysis of the fundamental frequency and the harmonics-to-noise ratio of a sampled
// sound" -- in three stages:
//   * sum_f64_partials_kernel / pitch_ac_peak_kernel: the global mean (float64 partial sums, added in a fixed order) and the global
//     peak max |x - mean| (peak_commit on the mean-removed signal);
//   * pitch_ac_frame_kernel: one workgroup per frame -- mean removal, Hanning window, autocorrelation through two 2048-point complex
//     FFTs in LDS (forward decimation in frequency, |X|^2 in the scrambled order, the mirrored decimation in time back: no reordering
//     pass), normalisation by the window's autocorrelation, maxima, sinc-interpolated strengths, the 14 strongest, golden-section
//     refinement.  A group of 16 lanes shares one interpolation sum; its partial sums meet in a fixed butterfly;
//   * pitch_ac_nodes_kernel / pitch_ac_path_kernel: Praat's Pitch_pathFinder in float64 -- node values and log2 f of every candidate in
//     parallel, then one wave walks the frames (four predecessors per lane), back-pointers in scratch, backtracking through LDS.
// Nothing here uses a floating-point atomic, and the sums over a wave, a workgroup and the whole signal are reduce.h's, which defines
// their order: two calls give the same bits.
#include "cplx.h"
#include "reduce.h"

#include <cmath>

namespace aicg {

constexpr int kAcThreads = 256;
constexpr int kAcGroup = 16;                        // lanes that share one sinc interpolation
constexpr int kAcGroups = kAcThreads / kAcGroup;    // = the most candidates a frame can keep, the unvoiced one included
constexpr int kAcDepthStrength = 30, kAcDepthRefine = 70, kAcDepthRefineHigh = 700;
constexpr int kAcGoldenSteps = 20;                  // bracket [k - 1, k + 1] -> 2 * 0.618^20 = 1.3e-4 samples
constexpr float kAcGolden = 0.61803398874989484820f;
constexpr int kAcMaxFft = 4096;

struct AcGeom {
    long nw, nfft, maxlag, brent, n_frames;
    double t1s, step;            // first frame centre and frame step, in samples
    long cand_scratch, path_scratch;
};

static int ac_geom(const char* who, int sr, long n, double dt, double fl, double ceil, AcGeom* g) {
    if (sr < 1000 || sr > 384000) return fail(AICG_E_ARG, "%s: sample rate %d", who, sr);
    if (!(dt > 0.0) || !(fl > 0.0) || !(ceil > fl) || ceil > 0.5 * sr) return fail(AICG_E_ARG, "%s: time step %g, pitch range %g .. %g at %d Hz", who, dt, fl, ceil, sr);
    if (n < 0 || n >= (1L << 40)) return fail(AICG_E_SHAPE, "%s: n %ld", who, n);
    const double dx = 1.0 / (double)sr, dur = (double)n * dx;
    long nw = (long)floor(3.0 / fl / dx);
    const long half = nw / 2 - 1;
    nw = 2 * half;
    if (nw < 8) return fail(AICG_E_ARG, "%s: a window of %ld samples (pitch floor %g at %d Hz)", who, nw, fl, sr);
    g->nw = nw;
    g->maxlag = lmin(nw / 3 + 2, nw);
    g->brent = nw / 2;
    long nfft = 1;
    while ((double)nfft < 1.5 * (double)nw) nfft *= 2;
    g->nfft = nfft;
    if (nfft > kAcMaxFft) return fail(AICG_E_SHAPE, "%s: a %ld-point FFT (pitch floor %g at %d Hz); at most %d", who, nfft, fl, sr, kAcMaxFft);
    if (dur < 3.0 / fl) return fail(AICG_E_SHAPE, "%s: %ld samples are shorter than one window (3 / %g s)", who, n, fl);
    g->n_frames = (long)floor((dur - 3.0 / fl) / dt) + 1;
    if (g->n_frames < 1 || nw > n) return fail(AICG_E_SHAPE, "%s: %ld samples are shorter than one window (%ld)", who, n, nw);
    g->step = dt * (double)sr;
    g->t1s = 0.5 * (double)n - 0.5 * (double)(g->n_frames - 1) * g->step;
    g->cand_scratch = (long)sizeof(double) * (kSumPartials + 2);
    g->path_scratch = g->n_frames * (long)(16 * 2 * sizeof(double) + 16);
    return AICG_OK;
}

// ---- global mean and peak --------------------------------------------------------------------------------------------------
// stats[0] = mean (fp32, the same bits in every thread), stats[1] = max |x - mean| (bits of a non-negative float)
__global__ void __launch_bounds__(256) pitch_ac_peak_kernel(const float* __restrict__ x, long n, const double* __restrict__ part, int n_part,
                                                            float* __restrict__ stats) {
    const float mean = (float)(sum_of_partials(part, n_part) / (double)n);
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[0] = mean;
    float m = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(x[i] - mean));
    peak_commit(m, reinterpret_cast<unsigned*>(stats + 1));
}

// ---- the frame stage ---------------------------------------------------------------------------------------------------------
struct AcFrameParams {
    long n, n_frames;
    double t1s, step;
    int nw, nfft, brent, kmax;     // maxima are looked for at lags 2 .. kmax - 1
    int max_cand, list_cap;
    float sr, floor_hz, vthr, sil, octcost;
};

// One radix-4 stage over blocks of L points, in place.  Forward (decimation in frequency): butterfly, then twiddles W_L^{j m}; the
// inverse stage undoes it up to the factor 4: conjugate twiddles, then the conjugate butterfly.  tw[k] = exp(-2 pi i k / N).
template <bool INV>
__device__ __forceinline__ void ac_stage4(float2* z, const float2* tw, int N, int L, int tid) {
    const int q = L >> 2, ts = N / L;
    for (int b = tid; b < (N >> 2); b += kAcThreads) {
        const int j = b & (q - 1), base = ((b - j) << 2) + j;
        float2 a0 = z[base], a1 = z[base + q], a2 = z[base + 2 * q], a3 = z[base + 3 * q];
        if (INV && j) {
            a1 = cmulc(a1, tw[j * ts]);
            a2 = cmulc(a2, tw[2 * j * ts]);
            a3 = cmulc(a3, tw[3 * j * ts]);
        }
        const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), d = csub(a1, a3);
        const float2 t3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);
        float2 y0 = cadd(t0, t2), y1 = cadd(t1, t3), y2 = csub(t0, t2), y3 = csub(t1, t3);
        if (!INV && j) {
            y1 = cmul(y1, tw[j * ts]);
            y2 = cmul(y2, tw[2 * j * ts]);
            y3 = cmul(y3, tw[3 * j * ts]);
        }
        z[base] = y0; z[base + q] = y1; z[base + 2 * q] = y2; z[base + 3 * q] = y3;
    }
    __syncthreads();
}
__device__ __forceinline__ void ac_stage2(float2* z, int N, int tid) {   // blocks of two points: no twiddle, its own inverse up to 2
    for (int b = tid; b < (N >> 1); b += kAcThreads) {
        const float2 a = z[2 * b], c = z[2 * b + 1];
        z[2 * b] = cadd(a, c);
        z[2 * b + 1] = csub(a, c);
    }
    __syncthreads();
}

// r at any integer lag: the normalised autocorrelation is even, r[-k] = r[k], and known for |k| <= brent
__device__ __forceinline__ float ac_r(const float* r, int k, int brent) {
    k = k < 0 ? -k : k;
    return r[k > brent ? brent : k];
}

// This lane's share (terms sub, sub + 16, ...) of the Hann-tapered sinc interpolation of r at `lag` -- Praat's NUM_interpolate_sinc on
// the array r[-brent .. brent]: with ml = floor(lag), phi = lag - ml, the `depth` samples to the left weigh
//   sin(pi phi) (-1)^t / (2 pi (phi + t)) (1 + cos(pi (phi + t) / (phi + depth))),  t = 0 .. depth - 1 at lag ml - t,
// and the ones to the right the same with 1 - phi at lag ml + 1 + t.  depth is cut to the samples the array has on either side.
__device__ __forceinline__ float ac_sinc_part(const float* r, int brent, float lag, int depth, int sub) {
    const float fl = floorf(lag);
    const int ml = (int)fl;
    const float phi = lag - fl;
    if (lag >= (float)brent) return sub == 0 ? r[brent] : 0.f;
    if (lag <= (float)-brent) return sub == 0 ? r[brent] : 0.f;
    if (phi == 0.f) return sub == 0 ? ac_r(r, ml, brent) : 0.f;
    depth = imin(depth, imin(ml + brent + 1, brent - ml));
    if (depth < 1) return sub == 0 ? ac_r(r, (int)floorf(lag + 0.5f), brent) : 0.f;
    const float hs_l = 0.5f * sinpif(phi), hs_r = 0.5f * sinpif(1.f - phi);
    const float inv_l = 1.f / (phi + (float)depth), inv_r = 1.f / (1.f - phi + (float)depth);
    float acc = 0.f;
    for (int t = sub; t < depth; t += kAcGroup) {
        const float sg = (t & 1) ? -1.f : 1.f;
        const float ul = phi + (float)t, ur = 1.f - phi + (float)t;
        const float dl = sg * hs_l / (3.14159265358979323846f * ul) * (1.f + cospif(ul * inv_l));
        const float dr = sg * hs_r / (3.14159265358979323846f * ur) * (1.f + cospif(ur * inv_r));
        acc += ac_r(r, ml - t, brent) * dl;
        acc += ac_r(r, ml + 1 + t, brent) * dr;
    }
    return acc;
}
// the whole sum, in every lane of the group (every lane of the workgroup calls this)
__device__ __forceinline__ float ac_sinc(const float* r, int brent, float lag, int depth, int sub) {
    float v = ac_sinc_part(r, brent, lag, depth, sub);
    for (int o = kAcGroup / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kAcGroup);
    return v;
}

__global__ void __launch_bounds__(kAcThreads) pitch_ac_frame_kernel(const float* __restrict__ x, const float* __restrict__ window,
                                                                    const float* __restrict__ wac, const float* __restrict__ twiddle,
                                                                    const float* __restrict__ stats, float* __restrict__ cand,
                                                                    int* __restrict__ count, AcFrameParams p) {
    HIP_DYNAMIC_SHARED(float, smem)
    const int tid = threadIdx.x, N = p.nfft, nw = p.nw, brent = p.brent;
    float2* z = reinterpret_cast<float2*>(smem);           // [N]
    float2* tw = z + N;                                    // [N]
    float* r = reinterpret_cast<float*>(tw + N);           // [brent + 1]
    float* red = r + brent + 1;                            // [8]
    int* flag = reinterpret_cast<int*>(red + 8);           // [kmax]
    int* mk = flag + p.kmax;                               // [list_cap]: lags of the maxima, ascending
    float* mf = reinterpret_cast<float*>(mk + p.list_cap); // their first frequency estimates
    float* ms = mf + p.list_cap;                           // their strengths
    int* kk = reinterpret_cast<int*>(ms + p.list_cap);     // [kAcGroups]: the candidates kept
    float* kf = reinterpret_cast<float*>(kk + kAcGroups);
    float* ks = kf + kAcGroups;
    int* cnt = reinterpret_cast<int*>(ks + kAcGroups);     // [2]: maxima, candidates kept

    for (int e = tid; e < N; e += kAcThreads) tw[e] = reinterpret_cast<const float2*>(twiddle)[e];
    const float gpeak = stats[1];
    const int grp = tid / kAcGroup, sub = tid % kAcGroup;
    const int odd = __builtin_ctz((unsigned)N) & 1;

    for (long f = blockIdx.x; f < p.n_frames; f += gridDim.x) {
        const long start = (long)floor(p.t1s + (double)f * p.step - 0.5) + 1 - (nw >> 1);
        // ---- mean, local peak, window
        float s = 0.f;
        for (int i = tid; i < nw; i += kAcThreads) {
            const long g = start + i;
            const float v = (g >= 0 && g < p.n) ? x[g] : 0.f;
            z[i] = make_float2(v, 0.f);
            s += v;
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        const float mean = (((red[0] + red[1]) + red[2]) + red[3]) / (float)nw;
        float pk = 0.f;
        for (int i = tid; i < N; i += kAcThreads) {
            if (i < nw) {
                const float v = z[i].x - mean;
                pk = fmaxf(pk, fabsf(v));
                z[i] = make_float2(v * window[i], 0.f);
            } else {
                z[i] = make_float2(0.f, 0.f);
            }
        }
        for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
        if ((tid & 63) == 0) red[4 + (tid >> 6)] = pk;
        __syncthreads();
        const float lpeak = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
        // ---- autocorrelation: forward stages L = N, N / 4, ..., power, the same stages backwards
        int L = N;
        for (; L >= 4; L >>= 2) ac_stage4<false>(z, tw, N, L, tid);
        if (odd) ac_stage2(z, N, tid);
        for (int i = tid; i < N; i += kAcThreads) {
            const float2 v = z[i];
            z[i] = make_float2(v.x * v.x + v.y * v.y, 0.f);
        }
        __syncthreads();
        if (odd) ac_stage2(z, N, tid);
        for (L = odd ? 8 : 4; L <= N; L <<= 2) ac_stage4<true>(z, tw, N, L, tid);
        const float ac0 = z[0].x;
        for (int k = tid; k <= brent; k += kAcThreads) r[k] = ac0 > 0.f ? z[k].x / (ac0 * wac[k]) : 0.f;
        __syncthreads();
        // ---- maxima
        for (int k = tid; k < p.kmax; k += kAcThreads)
            flag[k] = k >= 2 && r[k] > 0.5f * p.vthr && r[k] > r[k - 1] && r[k] >= r[k + 1];
        __syncthreads();
        if (tid == 0) {
            int m = 0;
            if (lpeak > 0.f)
                for (int k = 2; k < p.kmax && m < p.list_cap; ++k)
                    if (flag[k]) mk[m++] = k;
            cnt[0] = m;
        }
        __syncthreads();
        const int n_max = cnt[0];
        for (int m0 = 0; m0 < n_max; m0 += kAcGroups) {
            const int m = m0 + grp, k = m < n_max ? mk[m] : 2;
            const float dr = 0.5f * (r[k + 1] - r[k - 1]), d2r = 2.f * r[k] - r[k - 1] - r[k + 1];
            const float lag = d2r > 0.f ? (float)k + dr / d2r : (float)k;
            float st = ac_sinc(r, brent, lag, kAcDepthStrength, sub);
            if (st > 1.f) st = 1.f / st;
            if (sub == 0 && m < n_max) { mf[m] = p.sr / lag; ms[m] = st; }
        }
        __syncthreads();
        // ---- the strongest max_cand - 1, in the order they were met; a full table gives up its weakest entry by local strength
        if (tid == 0) {
            const int cap = p.max_cand - 1;
            int nc = 0;
            for (int m = 0; m < n_max; ++m) {
                int place = -1;
                if (nc < cap) {
                    place = nc++;
                } else {
                    float weakest = 2.f;
                    for (int c = 0; c < cap; ++c) {
                        const float ls = ks[c] - p.octcost * log2f(p.floor_hz / kf[c]);
                        if (ls < weakest) { weakest = ls; place = c; }
                    }
                    if (ms[m] - p.octcost * log2f(p.floor_hz / mf[m]) <= weakest) place = -1;
                }
                if (place >= 0) { kk[place] = mk[m]; kf[place] = mf[m]; ks[place] = ms[m]; }
            }
            cnt[1] = nc;
        }
        __syncthreads();
        // ---- refinement: group g moves candidate g to the maximum of the depth-70 interpolation inside [k - 1, k + 1]
        const int nc = cnt[1];
        {
            const bool mine = grp < nc;
            const int k = mine ? kk[grp] : 2;
            const int depth = (mine && kf[grp] > 0.3f * p.sr) ? kAcDepthRefineHigh : kAcDepthRefine;
            float a = (float)(k - 1), b = (float)(k + 1);
            float x1 = b - kAcGolden * (b - a), x2 = a + kAcGolden * (b - a);
            float f1 = ac_sinc(r, brent, x1, depth, sub), f2 = ac_sinc(r, brent, x2, depth, sub);
            for (int it = 0; it < kAcGoldenSteps; ++it) {
                const bool left = f1 > f2;
                if (left) { b = x2; x2 = x1; f2 = f1; x1 = b - kAcGolden * (b - a); }
                else { a = x1; x1 = x2; f1 = f2; x2 = a + kAcGolden * (b - a); }
                const float fn = ac_sinc(r, brent, left ? x1 : x2, depth, sub);
                if (left) f1 = fn; else f2 = fn;
            }
            const float xm = 0.5f * (a + b);
            float st = ac_sinc(r, brent, xm, depth, sub);
            if (st > 1.f) st = 1.f / st;
            float* row = cand + (f * p.max_cand + 1 + grp) * 2;
            if (sub == 0 && mine) { row[0] = p.sr / xm; row[1] = st; }
            else if (sub == 0 && 1 + grp < p.max_cand) { row[0] = 0.f; row[1] = 0.f; }
        }
        if (tid == 0) {
            const float inten = gpeak > 0.f ? lpeak / gpeak : 0.f;
            cand[f * p.max_cand * 2] = 0.f;
            cand[f * p.max_cand * 2 + 1] = p.vthr + fmaxf(0.f, 2.f - inten / (p.sil / (1.f + p.vthr)));
            count[f] = 1 + nc;
        }
        __syncthreads();
    }
}

// ---- the path finder ---------------------------------------------------------------------------------------------------------
constexpr double kAcUnvoiced = -1.0e30;   // log2 f of a candidate that is not voiced
constexpr int kAcChunk = 128;             // frames staged in LDS at a time
constexpr int kAcBack = 1024;             // frames backtracked through LDS at a time

// nl[t][c] = (node value, log2 f or kAcUnvoiced) for c < 16
__global__ void __launch_bounds__(256) pitch_ac_nodes_kernel(const float* __restrict__ cand, const int* __restrict__ count,
                                                             double2* __restrict__ nl, long n_frames, int K, double ceiling, double octcost) {
#pragma clang fp contract(off)
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_frames * 16) return;
    const long t = e >> 4;
    const int c = (int)(e & 15);
    double node = 0.0, lf = kAcUnvoiced;
    if (c < imin(imax(count[t], 1), K)) {
        const double f = (double)cand[(t * K + c) * 2], s = (double)cand[(t * K + c) * 2 + 1];
        if (f > 0.0 && f < ceiling) {
            lf = log2(f);
            node = s - octcost * (log2(ceiling) - lf);
        } else {
            node = (double)cand[t * K * 2 + 1];
        }
    }
    nl[e] = make_double2(node, lf);
}

__global__ void __launch_bounds__(64) pitch_ac_path_kernel(const float* __restrict__ cand, const int* __restrict__ count,
                                                           const double2* __restrict__ nl, unsigned char* __restrict__ psi,
                                                           double* __restrict__ f0_out, int* __restrict__ state_out, long n_frames, int K,
                                                           double ojc, double vuc) {
#pragma clang fp contract(off)
    __shared__ double2 stage[kAcChunk * 16];
    __shared__ int scnt[kAcChunk];
    __shared__ unsigned spsi[kAcChunk * 4];   // the chunk's back-pointers, 16 bytes a frame
    __shared__ double dl[2][16], lfp[2][16];
    __shared__ unsigned char back[kAcBack * 16];
    __shared__ unsigned char chosen[kAcBack];
    __shared__ int carry;
    const int lane = threadIdx.x, j = lane >> 2, q = lane & 3;
    int cur = 0, cprev = 0;
    for (long c0 = 0; c0 < n_frames; c0 += kAcChunk) {
        const int nfc = (int)lmin((long)kAcChunk, n_frames - c0);
        for (int e = lane; e < nfc * 16; e += 64) stage[e] = nl[c0 * 16 + e];
        for (int e = lane; e < nfc; e += 64) scnt[e] = imin(imax(count[c0 + e], 1), K);
        __syncthreads();
        for (int tt = 0; tt < nfc; ++tt) {
            const long t = c0 + tt;
            const int cn = scnt[tt];
            const double2 me = stage[tt * 16 + j];
            double best = -INFINITY;
            int bi = 4 * q;
            if (t == 0) {
                best = 0.0;
            } else {
                for (int ii = 0; ii < 4; ++ii) {
                    const int i = 4 * q + ii;
                    if (i >= cprev) break;
                    const double li = lfp[cur][i];
                    const bool vi = li != kAcUnvoiced, vj = me.y != kAcUnvoiced;
                    const double cost = (vi && vj) ? ojc * fabs(li - me.y) : (vi != vj ? vuc : 0.0);
                    const double v = dl[cur][i] - cost;
                    if (v > best) { best = v; bi = i; }
                }
                for (int o = 1; o <= 2; o <<= 1) {
                    const double ov = __shfl_xor(best, o, 64);
                    const int oi = __shfl_xor(bi, o, 64);
                    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
                }
            }
            if (q == 0 && j < cn) {
                dl[cur ^ 1][j] = best + me.x;
                lfp[cur ^ 1][j] = me.y;
                reinterpret_cast<unsigned char*>(spsi)[tt * 16 + j] = (unsigned char)bi;
            }
            cur ^= 1;
            cprev = cn;
            __syncthreads();
        }
        // the chunk's back-pointers leave in one piece: a store to HBM inside the frame loop would be waited for at every barrier
        for (int e = lane; e < nfc * 4; e += 64) reinterpret_cast<unsigned*>(psi + c0 * 16)[e] = spsi[e];
        __syncthreads();
    }
    // the last frame's best state (first maximum), then back through the pointers, a block of frames at a time
    if (lane == 0) {
        double best = -INFINITY;
        int sbest = 0;
        for (int i = 0; i < cprev; ++i)
            if (dl[cur][i] > best) { best = dl[cur][i]; sbest = i; }
        carry = sbest;
    }
    __syncthreads();
    for (long hi = n_frames; hi > 0; hi -= kAcBack) {
        const long lo = lmax(0L, hi - kAcBack);
        const int nb = (int)(hi - lo);
        for (int e = lane; e < nb * 4; e += 64)
            reinterpret_cast<unsigned*>(back)[e] = reinterpret_cast<const unsigned*>(psi + lo * 16)[e];
        __syncthreads();
        if (lane == 0) {
            int sidx = carry;                  // state of frame hi - 1
            for (int tt = nb - 1; tt >= 0; --tt) {
                chosen[tt] = (unsigned char)sidx;
                sidx = back[tt * 16 + sidx];   // state of the frame before (frame 0's pointer is never followed)
            }
            carry = sidx;
        }
        __syncthreads();
        for (int tt = lane; tt < nb; tt += 64) {
            const long t = lo + tt;
            const int sidx = chosen[tt];
            f0_out[t] = (double)cand[(t * K + sidx) * 2];
            if (state_out) state_out[t] = sidx;
        }
        __syncthreads();
    }
}

}  // namespace aicg

using namespace aicg;

extern "C" int aicg_pitch_ac_geometry(int sample_rate, int64_t n, double time_step, double pitch_floor, double pitch_ceiling, int64_t* geom) {
    if (!geom) return fail(AICG_E_ARG, "aicg_pitch_ac_geometry: null pointer");
    AcGeom g;
    const int rc = ac_geom("aicg_pitch_ac_geometry", sample_rate, (long)n, time_step, pitch_floor, pitch_ceiling, &g);
    if (rc != AICG_OK) return rc;
    geom[0] = g.nw; geom[1] = g.nfft; geom[2] = g.maxlag; geom[3] = g.brent; geom[4] = g.n_frames; geom[5] = (int64_t)floor(g.t1s);
    geom[6] = g.cand_scratch; geom[7] = g.path_scratch;
    return AICG_OK;
}

extern "C" int aicg_pitch_ac_candidates(const float* x, int64_t n, int sample_rate, double time_step, double pitch_floor, double pitch_ceiling,
                                        int max_candidates, double voicing_threshold, double silence_threshold, double octave_cost,
                                        const float* window, const float* window_ac, const float* twiddle, void* scratch, float* cand,
                                        int* count, void* stream) {
    AcGeom g;
    const int rc = ac_geom("aicg_pitch_ac_candidates", sample_rate, (long)n, time_step, pitch_floor, pitch_ceiling, &g);
    if (rc != AICG_OK) return rc;
    if (max_candidates < 2 || max_candidates > kAcGroups) return fail(AICG_E_ARG, "aicg_pitch_ac_candidates: %d candidates (2 .. %d)", max_candidates, kAcGroups);
    if (!(silence_threshold > 0.0) || !(voicing_threshold > 0.0)) return fail(AICG_E_ARG, "aicg_pitch_ac_candidates: thresholds %g, %g", voicing_threshold, silence_threshold);
    if (!x || !window || !window_ac || !twiddle || !scratch || !cand || !count) return fail(AICG_E_ARG, "aicg_pitch_ac_candidates: null pointer");
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)scratch;
    float* stats = (float*)(part + kSumPartials);
    (void)hipMemsetAsync(stats, 0, 2 * sizeof(float), st);
    hipLaunchKernelGGL(sum_f64_partials_kernel, dim3(kSumPartials), dim3(256), 0, st, x, (long)n, part);
    int rc2 = check_launch("sum_f64_partials_kernel");
    if (rc2 != AICG_OK) return rc2;
    hipLaunchKernelGGL(pitch_ac_peak_kernel, dim3(grid_1d((long)n)), dim3(256), 0, st, x, (long)n, (const double*)part, kSumPartials, stats);
    rc2 = check_launch("pitch_ac_peak_kernel");
    if (rc2 != AICG_OK) return rc2;
    AcFrameParams p;
    p.n = (long)n; p.n_frames = g.n_frames; p.t1s = g.t1s; p.step = g.step;
    p.nw = (int)g.nw; p.nfft = (int)g.nfft; p.brent = (int)g.brent; p.kmax = (int)lmin(g.maxlag, g.brent);
    p.max_cand = max_candidates; p.list_cap = p.kmax / 2 + 2;
    p.sr = (float)sample_rate; p.floor_hz = (float)pitch_floor; p.vthr = (float)voicing_threshold; p.sil = (float)silence_threshold;
    p.octcost = (float)octave_cost;
    const size_t lds = sizeof(float) * ((size_t)4 * p.nfft + (size_t)p.brent + 1 + 8 + (size_t)p.kmax + 3 * (size_t)p.list_cap + 3 * kAcGroups + 2);
    if (lds > 160 * 1024) return fail(AICG_E_LDS, "aicg_pitch_ac_candidates: %zu bytes for a %d-point FFT", lds, p.nfft);
    allow_dynamic_lds((const void*)pitch_ac_frame_kernel, lds);
    const unsigned grid = (unsigned)lmin(g.n_frames, 1024L);
    hipLaunchKernelGGL(pitch_ac_frame_kernel, dim3(grid), dim3(kAcThreads), lds, st, x, window, window_ac, twiddle, (const float*)stats, cand, count, p);
    return check_launch("pitch_ac_frame_kernel");
}

extern "C" int aicg_pitch_ac_path(const float* cand, const int* count, int64_t n_frames, int max_candidates, double time_step,
                                  double pitch_ceiling, double octave_cost, double octave_jump_cost, double voiced_unvoiced_cost, void* scratch,
                                  double* f0_out, int* state_out, void* stream) {
    if (n_frames < 0 || n_frames >= (1L << 40)) return fail(AICG_E_SHAPE, "aicg_pitch_ac_path: %lld frames", (long long)n_frames);
    if (max_candidates < 1 || max_candidates > 16) return fail(AICG_E_ARG, "aicg_pitch_ac_path: %d candidates (1 .. 16)", max_candidates);
    if (!(time_step > 0.0) || !(pitch_ceiling > 0.0)) return fail(AICG_E_ARG, "aicg_pitch_ac_path: time step %g, ceiling %g", time_step, pitch_ceiling);
    if (n_frames == 0) return AICG_OK;
    if (!cand || !count || !scratch || !f0_out) return fail(AICG_E_ARG, "aicg_pitch_ac_path: null pointer");
    hipStream_t st = (hipStream_t)stream;
    double2* nl = (double2*)scratch;
    unsigned char* psi = (unsigned char*)(nl + n_frames * 16);
    const double c = 0.01 / time_step;
    hipLaunchKernelGGL(pitch_ac_nodes_kernel, dim3((unsigned)ldiv_up((long)n_frames * 16, 256)), dim3(256), 0, st, cand, count, nl, (long)n_frames,
                       max_candidates, pitch_ceiling, octave_cost);
    const int rc = check_launch("pitch_ac_nodes_kernel");
    if (rc != AICG_OK) return rc;
    hipLaunchKernelGGL(pitch_ac_path_kernel, dim3(1), dim3(64), 0, st, cand, count, (const double2*)nl, psi, f0_out, state_out, (long)n_frames,
                       max_candidates, octave_jump_cost * c, voiced_unvoiced_cost * c);
    return check_launch("pitch_ac_path_kernel");
}
