// pitch_shift of song_cover_pipeline on the device (reference src/main.py:138-147, `-pall N`): sox's `pitch` effect restated as its two
// stages:
//   * tempo_wsola_kernel: time-stretch by waveform-similarity overlap-add with sox's `tempo` music defaults (segment 82 ms, search
//     14.68 ms, overlap 12 ms).  The chain over the steps is sequential -- step k's overlap o_k is the input that follows step k-1's
//     chosen offset -- so one persistent workgroup walks one signal; signals are batched over the grid.
//   * resample_ratio_kernel: band-limited resampling by an irrational ratio through a host-built Kaiser-windowed-sinc table
//     (phase rows, linear interpolation between rows), float64 phase and accumulation; one thread per output frame.
// Every read of a signal past its ends is a zero; nothing here uses atomics, so two calls give the same bits.
#include "common.h"

#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace aicg {

constexpr int kWsolaThreads = 1024;   // 16 waves: the 4 SIMDs of one CU, four waves each
constexpr int kWsolaPre = 8;          // next-step window elements a thread keeps in flight in registers during the search
constexpr int kWsolaMaxWaves = kWsolaThreads / 64;

struct WsolaGeom {
    long seg, search, ovl, skip, adv;  // frames; adv = seg - ovl = output frames per step
    long steps, n_out;
};

// sox `tempo` defaults for music in frames at sample_rate, for the tempo factor f (output duration = input duration / f)
static int wsola_geom(const char* who, int sr, double tempo, long n, WsolaGeom* g) {
    if (sr < 8000 || sr > 384000) return fail(AICG_E_ARG, "%s: sample rate %d", who, sr);
    if (!(tempo >= 0.25 && tempo <= 4.0)) return fail(AICG_E_ARG, "%s: tempo factor %g outside [0.25, 4]", who, tempo);
    if (n < 0) return fail(AICG_E_SHAPE, "%s: n %ld", who, n);
    g->seg = llround(sr * 0.082);
    g->search = llround(sr * 0.01468);
    g->ovl = lmax(llround(sr * 0.012), 16) & ~7L;
    g->adv = g->seg - g->ovl;
    g->skip = llround(tempo * (double)g->adv);
    g->n_out = llround((double)n / tempo);
    g->steps = ldiv_up(g->n_out, g->adv);
    if (g->search < 1 || g->adv <= g->ovl || g->skip < 1) return fail(AICG_E_ARG, "%s: degenerate segment geometry at %d Hz", who, sr);
    return AICG_OK;
}

struct WsolaParams {
    long n, n_out;
    int seg, search, ovl, skip, steps;
    int S, L;     // the overlap is cut into S slices of L frames (a multiple of 4) for the search
    int Gp, Wp;   // search rounded up to 4; floats per channel of the window image (Gp + ovl + 4)
};

// One workgroup per signal.  Step k >= 1 (step 0 copies `adv` frames):
//   A  every thread issues its share of the loads for step k + 1 (the search window at (k + 1) skip and the `search + ovl` frames
//      o_{k+1} can come from, neither depends on i_k) into registers, then takes one (4 candidates, one slice of the overlap) item
//      of cost_k: the window slides through registers, one 16-byte LDS read of the window and one of o_k per 16 multiply-adds;
//   B  cost(i) = the slices summed in order; argmin with ties to the lowest i per thread, per wave (shuffles), then over the waves;
//   C  every thread knows i_k: the prefetched values go to LDS (o_{k+1} shifted by i_k), and the step's output -- cross-fade from
//      o_k, then the copy -- is written from the input in HBM while the next search starts.
// With offsets_in the search (A's items and B) is skipped and i_k is read instead.
template <int C>
__global__ void __launch_bounds__(kWsolaThreads) tempo_wsola_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                    int* __restrict__ offs_out, const int* __restrict__ offs_in,
                                                                    WsolaParams p) {
    HIP_DYNAMIC_SHARED(float, smem)
    const int tid = threadIdx.x, nt = blockDim.x;
    const int ovl = p.ovl, search = p.search, Wp = p.Wp, Gp = p.Gp, adv = p.seg - p.ovl, wlen = p.search + p.ovl;
    float* win = smem;                       // [C][Wp]: x[p_k .. p_k + search + ovl), zeros behind
    float* ob = win + C * Wp;                // [C][ovl]: o_k
    float* part = ob + C * ovl;              // [S][Gp]
    float* wbc = part + p.S * Gp;            // per wave: best cost, best offset
    int* wbi = reinterpret_cast<int*>(wbc + kWsolaMaxWaves);

    const int n = (int)p.n, n_out = (int)p.n_out;   // (the host keeps 4 C n and C n_out below 2^31)
    const float* xs = x + (long)blockIdx.x * C * n;
    float* ys = y + (long)blockIdx.x * C * n_out;
    int* oo = offs_out + (long)blockIdx.x * p.steps;
    const int* oi = offs_in ? offs_in + (long)blockIdx.x * p.steps : nullptr;
    // input frame i >= 0 of channel c, zero past the end: one select and the buffer range check, no branch (the host bounds 4 C n below 2^31)
    const BufRsrc rs = make_buf(xs, (unsigned)(C * n) * 4u);
    auto X = [&](int c, int i) { return buf_load_f32(rs, i < n ? (unsigned)(c * n + i) << 2 : kBufOob); };

    // step 0: no overlap yet, the segment's first adv frames are copied
    for (int e = tid; e < adv * C; e += nt) {
        const int c = (C == 2 && e >= adv) ? 1 : 0, j = e - c * adv;
        if (j < n_out) ys[c * n_out + j] = X(c, j);
    }
    if (tid == 0 && p.steps > 0) oo[0] = 0;
    if (!oi) {
        for (int e = tid; e < C * Wp; e += nt) {
            const int c = (C == 2 && e >= Wp) ? 1 : 0, q = e - c * Wp;
            win[e] = q < wlen ? X(c, p.skip + q) : 0.f;
        }
        for (int e = tid; e < C * ovl; e += nt) {
            const int c = (C == 2 && e >= ovl) ? 1 : 0, j = e - c * ovl;
            ob[e] = X(c, adv + j);
        }
        __syncthreads();
    }

    const int G = Gp >> 2;                   // search items: (slice s, candidates 4 gi .. 4 gi + 3), thread tid starts at item tid
    const int s_first = tid / G, g_first = tid - s_first * G, s_step = nt / G, g_step = nt - s_step * G;
    const float fstep = 1.0f / (float)ovl;
    const int tot = 2 * C * wlen;            // prefetch elements: [win_{k+1}: C x wlen][o_{k+1}'s range: C x wlen]
    int iprev = 0;
    for (int k = 1; k < p.steps; ++k) {
        const int pk = k * p.skip;
        auto fetch = [&](int e) {
            const int which = e >= C * wlen, r = e - which * C * wlen;
            const int c = (C == 2 && r >= wlen) ? 1 : 0, q = r - c * wlen;
            return X(c, pk + (which ? adv : p.skip) + q);
        };
        auto stash = [&](int e, float v, int ik) {
            const int which = e >= C * wlen, r = e - which * C * wlen;
            const int c = (C == 2 && r >= wlen) ? 1 : 0, q = r - c * wlen;
            if (!which) win[c * Wp + q] = v;
            else if (q >= ik && q - ik < ovl) ob[c * ovl + q - ik] = v;
        };
        int ik;
        float pre[kWsolaPre];
        if (!oi) {
#pragma unroll
            for (int r = 0; r < kWsolaPre; ++r) {
                const int e = tid + r * nt;
                pre[r] = e < tot ? fetch(e) : 0.f;
            }
            // ---- A: partial costs
            for (int s = s_first, gi = g_first; s < p.S; s += s_step, gi += g_step) {   // item s G + gi, nt items further per turn
                if (gi >= G) { gi -= G; if (++s >= p.S) break; }
                const int i0 = gi << 2;
                const int j0 = s * p.L, j1 = imin(ovl, j0 + p.L);
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                for (int c = 0; c < C; ++c) {
                    const float4* w4 = reinterpret_cast<const float4*>(win + c * Wp + i0);
                    const float4* o4 = reinterpret_cast<const float4*>(ob + c * ovl);
                    float4 lo = w4[j0 >> 2];
                    for (int j = j0; j < j1; j += 4) {
                        const float4 hi = w4[(j >> 2) + 1], o = o4[j >> 2];
                        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                        const float ov[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) {
                                const float d = v[r + jj] - ov[jj];
                                acc[r] = fmaf(d, d, acc[r]);
                            }
                        lo = hi;
                    }
                }
                *reinterpret_cast<float4*>(part + s * Gp + i0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            }
            __syncthreads();
            // ---- B: argmin, ties to the lowest offset
            float bc = INFINITY;
            int bi = INT_MAX;
            auto take = [&](float c2, int i2) {
                if (c2 < bc || (c2 == bc && i2 < bi)) { bc = c2; bi = i2; }
            };
            for (int i = tid; i < search; i += nt) {
                float c = 0.f;
                for (int s = 0; s < p.S; ++s) c += part[s * Gp + i];
                take(c, i);
            }
            for (int m = 32; m >= 1; m >>= 1) {
                const float c2 = __shfl_xor(bc, m, 64);
                const int i2 = __shfl_xor(bi, m, 64);
                take(c2, i2);
            }
            if ((tid & 63) == 0) { wbc[tid >> 6] = bc; wbi[tid >> 6] = bi; }
            __syncthreads();
            bc = INFINITY;
            bi = INT_MAX;
            for (int w = 0; w < (nt >> 6); ++w) take(wbc[w], wbi[w]);
            ik = bi == INT_MAX ? 0 : bi;    // (no finite cost: a signal with NaN or infinity in it)
        } else {
            ik = imin(imax(oi[k], 0), search - 1);
        }
        if (tid == 0) oo[k] = ik;

        // ---- C: hand the next step its window and overlap, write this step's output
        if (!oi) {
#pragma unroll
            for (int r = 0; r < kWsolaPre; ++r) {
                const int e = tid + r * nt;
                if (e < tot) stash(e, pre[r], ik);
            }
            for (int e = tid + kWsolaPre * nt; e < tot; e += nt) stash(e, fetch(e), ik);
        }
        const int obase = k * adv, cur = pk + ik, prev = (k - 1) * p.skip + iprev + adv;
        for (int e = tid; e < adv * C; e += nt) {
            const int c = (C == 2 && e >= adv) ? 1 : 0, j = e - c * adv;
            if (obase + j >= n_out) continue;
            float v = X(c, cur + j);
            if (j < ovl) {
                const float a = fstep * (float)j, b = 1.0f - a;
                v = (X(c, prev + j) * b) + (v * a);
            }
            ys[c * n_out + obase + j] = v;
        }
        iprev = ik;
        if (!oi) __syncthreads();
    }
}

// y[c][m] = sum_t h(m d - t) x[c][t].  With t0 = floor(m d), phi = m d - t0 and t = t0 - j, the filter argument is phi + j for
// j = -half .. half; tab[r][j + half] = h(r / P + j) for r = 0 .. P, and h(phi + j) is read by linear interpolation between rows
// floor(phi P) and the next.  The phase, the interpolation and the sum are float64.  grid.y = signal.
template <int C>
__global__ void __launch_bounds__(256) resample_ratio_kernel(const float* __restrict__ x, float* __restrict__ y, long n_in, long n_out,
                                                             double d, const float* __restrict__ tab, int P, int half) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= n_out) return;
    const float* xs = x + (long)blockIdx.y * C * n_in;
    float* ys = y + (long)blockIdx.y * C * n_out;
    const double pos = (double)m * d;
    const double fl = floor(pos);
    const long t0 = (long)fl;
    const double rp = (pos - fl) * (double)P;
    const int r = imin((int)rp, P - 1);
    const double fr = rp - (double)r;
    const int W = 2 * half + 1;
    const float* row0 = tab + (long)r * W;
    const float* row1 = row0 + W;
    // taps whose sample exists: 0 <= t0 - j < n_in
    const long jlo = lmax(-(long)half, t0 - n_in + 1), jhi = lmin((long)half, t0);
    double acc[C];
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    for (long j = jlo; j <= jhi; ++j) {
        const double h0 = (double)row0[j + half], h1 = (double)row1[j + half];
        const double hv = fma(fr, h1 - h0, h0);
        for (int c = 0; c < C; ++c) acc[c] = fma(hv, (double)xs[(long)c * n_in + t0 - j], acc[c]);
    }
    for (int c = 0; c < C; ++c) ys[(long)c * n_out + m] = (float)acc[c];
}

}  // namespace aicg

using namespace aicg;

extern "C" int aicg_tempo_wsola_geometry(int sample_rate, double tempo, int64_t n, int64_t* geom) {
    if (!geom) return fail(AICG_E_ARG, "aicg_tempo_wsola_geometry: null pointer");
    WsolaGeom g;
    const int rc = wsola_geom("aicg_tempo_wsola_geometry", sample_rate, tempo, (long)n, &g);
    if (rc != AICG_OK) return rc;
    geom[0] = g.seg; geom[1] = g.search; geom[2] = g.ovl; geom[3] = g.skip; geom[4] = g.steps; geom[5] = g.n_out;
    return AICG_OK;
}

extern "C" int aicg_tempo_wsola(const float* x, float* y, int* offsets_out, const int* offsets_in, int n_signals, int n_channels,
                                int64_t n, int sample_rate, double tempo, void* stream) {
    WsolaGeom g;
    const int rc = wsola_geom("aicg_tempo_wsola", sample_rate, tempo, (long)n, &g);
    if (rc != AICG_OK) return rc;
    if (n_channels < 1 || n_channels > 2 || n_signals < 0) return fail(AICG_E_SHAPE, "aicg_tempo_wsola: %d signals of %d channels", n_signals, n_channels);
    if (n_signals == 0 || g.n_out == 0) return AICG_OK;
    if (!y || !offsets_out || (n > 0 && !x)) return fail(AICG_E_ARG, "aicg_tempo_wsola: null pointer");
    // the kernel indexes frames with 32-bit integers (n_out <= 4 n), and the signal's byte offsets are 31-bit buffer offsets
    if (n >= (1L << 27)) return fail(AICG_E_SHAPE, "aicg_tempo_wsola: n %lld", (long long)n);
    WsolaParams p;
    p.n = (long)n; p.n_out = g.n_out;
    p.seg = (int)g.seg; p.search = (int)g.search; p.ovl = (int)g.ovl; p.skip = (int)g.skip; p.steps = (int)g.steps;
    p.Gp = (p.search + 3) & ~3;
    p.Wp = p.Gp + p.ovl + 4;
    const int groups = p.Gp / 4;
    const int s_want = imax(1, imin(kWsolaThreads / groups, p.ovl / 4));
    p.L = (idiv_up(p.ovl, s_want) + 3) & ~3;
    p.S = idiv_up(p.ovl, p.L);
    const size_t lds = sizeof(float) * ((size_t)n_channels * p.Wp + (size_t)n_channels * p.ovl + (size_t)p.S * p.Gp + 2 * kWsolaMaxWaves);
    if (lds > 160 * 1024) return fail(AICG_E_LDS, "aicg_tempo_wsola: %zu bytes of search window at %d Hz x %d channels", lds, sample_rate, n_channels);
    auto kern = n_channels == 2 ? tempo_wsola_kernel<2> : tempo_wsola_kernel<1>;
    allow_dynamic_lds((const void*)kern, lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)n_signals), dim3(kWsolaThreads), lds, (hipStream_t)stream, x, y, offsets_out, offsets_in, p);
    return check_launch("tempo_wsola_kernel");
}

extern "C" int aicg_resample_ratio(const float* x, float* y, int n_signals, int n_channels, int64_t n_in, int64_t n_out, double ratio,
                                   const float* table, int phases, int half_taps, void* stream) {
    if (n_channels < 1 || n_channels > 2 || n_signals < 0 || n_signals > 65535 || n_in < 0 || n_out < 0)
        return fail(AICG_E_SHAPE, "aicg_resample_ratio: %d signals of %d channels, %lld -> %lld frames", n_signals, n_channels,
                    (long long)n_in, (long long)n_out);
    if (!(ratio >= 0.25 && ratio <= 4.0)) return fail(AICG_E_ARG, "aicg_resample_ratio: ratio %g outside [0.25, 4]", ratio);
    if (phases < 1 || phases > (1 << 20) || half_taps < 1 || half_taps > (1 << 20)) return fail(AICG_E_ARG, "aicg_resample_ratio: table of %d phases x %d half taps", phases, half_taps);
    if (n_signals == 0 || n_out == 0) return AICG_OK;
    if (!y || !table || (n_in > 0 && !x)) return fail(AICG_E_ARG, "aicg_resample_ratio: null pointer");
    const dim3 grid((unsigned)ldiv_up(n_out, 256), (unsigned)n_signals);
    if (n_channels == 2)
        hipLaunchKernelGGL(resample_ratio_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, x, y, (long)n_in, (long)n_out, ratio, table, phases, half_taps);
    else
        hipLaunchKernelGGL(resample_ratio_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, y, (long)n_in, (long)n_out, ratio, table, phases, half_taps);
    return check_launch("resample_ratio_kernel");
}
