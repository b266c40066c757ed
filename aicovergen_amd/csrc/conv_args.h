// What every convolution family shares: the argument record the dispatcher fills (ConvArgs) with its output indexing and
// epilogue arithmetic, the compile-time ablation / trace switches, the activation dispatch of the epilogues, and the host helpers
// more than one family's launcher uses.  The kernel generations themselves: conv_kernels.h (the classic implicit GEMMs, with
// conv_ws3.h / conv_ws3s.h / conv_ws3w.h on top), conv_w2d.h, conv_g1.h (with conv_g1s.h / conv_g1k.h / conv_g1w.h).
#pragma once
#include <type_traits>

#include "common.h"

namespace aicg {

// Phase-ablation switches (AICG_CONV_ABLATE bits in ConvArgs::dbg) exist only in builds made with -DAICG_CONV_ABLATION (build.py --dev)
// (tools/): the shipped kernels carry no profiling branches in their hot loops.
#ifdef AICG_CONV_ABLATION
static constexpr bool kAblate = true;
#else
static constexpr bool kAblate = false;
#endif

struct ConvArgs {
    const float* x;
    const float* w;
    const float* w3;   // k8-interleaved image of the same weights (conv_ws3.h), or nullptr
    const float* wsplit;   // bf16 hi / lo image (conv_ws3s.h) when the layer runs in split precision, or nullptr
    const float* bias;
    const float* res;
    float* y;
    int N, Cin_g, H, W, Cout_g, Ho, Wo, KH, KW, sh, sw, ph, pw, dh, dw, groups;
    long x_sn, x_sc, x_sh, y_sn, y_sc, y_sh, r_sn, r_sc, r_sh;
    int pre_act;
    float pre_slope;
    int act;
    float act_slope;
    float out_scale;
    int accumulate;
    int res_first;
    int shuffle;   // 2: GEMM row m / position (ho, wo) -> y[m >> 2][2 ho + ((m >> 1) & 1)][2 wo + (m & 1)] (k = s = 2 ConvTranspose2d)
    int res_mul;   // the residual operand multiplies (U-Net multiplicative skip) instead of adding, after the activation
    // derived tiling
    int TW, TWlog2, TH, TH_in, TW_in, TWp, CHS, BKC, BKClog2, TT, tiles_w, tiles_h, nchunk, taps, Mpad, Cin_pad, xs_elems, xs_total;
    unsigned div_chs, div_twp;  // ceil(2^32 / d) multipliers: idx / d == umulhi(idx, mul) for idx * d < 2^32
    long w_group_stride;
    // Phase stagger (wave-specialised kernels, two workgroups per CU): the consumers of the workgroup that shares a CU with an
    // earlier one start `stagger` shader cycles late, once, in the launch's initial fill (flat block id < stagger_first).
    // Identical tiles that start together stay in lockstep for the whole launch -- both in their prologue, both in their K
    // loop halving the matrix pipe, both in their epilogue with the pipe idle (r2 in-kernel timeline: 17 % of a 96-row MDX
    // tile's lifetime); half a tile out of phase, one workgroup's prologue / epilogue runs under the other's MFMAs.
    int stagger, stagger_first;
    int wide_ok;   // y (and res) rows are 16-byte aligned and TW % 4 == 0: interior tiles may use the float4 epilogue
    int f16;  // aicg_conv_desc.split == 2: fp16 operands on the matrix pipe where the layer's kernel has that form (conv_g1.h, conv_g1w.h)
    int dbg;  // AICG_CONV_ABLATE bits (profiling only): 1 no global loads, 2 no LDS commit, 4 no barriers, 8 no MFMA loop, 16 no epilogue
};

// output / residual element of GEMM row cg (= g * Cout_g + m) at position (ho, wo), relative to the image base
__device__ __forceinline__ long out_index(const ConvArgs& p, int cg, int ho, int wo, long sc, long sh) {
    return p.shuffle ? (long)(cg >> 2) * sc + (long)(2 * ho + ((cg >> 1) & 1)) * sh + 2 * wo + (cg & 1)
                     : (long)cg * sc + (long)ho * sh + wo;
}
// y = [y_old +] out_scale * (act(v [+ r]) [+ r | * r])
__device__ __forceinline__ float combine(const ConvArgs& p, float v, float r, float y_old) {
    if (p.res_first) v += r;
    v = apply_act(v, p.act, p.act_slope);
    if (!p.res_first) v = p.res_mul ? v * r : v + r;
    return v * p.out_scale + y_old;
}

// Optional in-kernel timeline (tools/conv_trace.py builds a private copy of the library with -DAICG_CONV_TRACE): wave 0 of the
// consumers of the first kTraceWgs workgroups records s_memtime at entry, first stage ready, end of the K loop, end of the
// epilogue, plus the hardware id; every `kTraceEvery`-th stage start as well.  Never compiled into the shipped library.
#ifdef AICG_CONV_TRACE
static constexpr int kTraceWgs = 8192, kTraceSlots = 8;
extern __device__ unsigned long long g_conv_trace[kTraceWgs * kTraceSlots];
__device__ __forceinline__ void trace_mark(int wg, int slot) {
    if (wg < kTraceWgs && (threadIdx.x & 63) == 0) g_conv_trace[wg * kTraceSlots + slot] = __builtin_readcyclecounter();
}
__device__ __forceinline__ void trace_val(int wg, int slot, unsigned long long v) {
    if (wg < kTraceWgs && (threadIdx.x & 63) == 0) g_conv_trace[wg * kTraceSlots + slot] = v;
}
// per-stage detail for workgroups 0 .. kTrace2Wgs-1: [wg][role 0 consumer / 1 producer][stage < 32][event]
static constexpr int kTrace2Wgs = 64;
extern __device__ unsigned long long g_conv_trace2[kTrace2Wgs * 2 * 32 * 4];
__device__ __forceinline__ void trace2(int wg, int role, int stage, int ev) {
    if (wg < kTrace2Wgs && stage < 32 && (threadIdx.x & 63) == 0)
        g_conv_trace2[((wg * 2 + role) * 32 + stage) * 4 + ev] = __builtin_readcyclecounter();
}
#else
__device__ __forceinline__ void trace_mark(int, int) {}
__device__ __forceinline__ void trace_val(int, int, unsigned long long) {}
__device__ __forceinline__ void trace2(int, int, int, int) {}
#endif

// Epilogue activation with the common cases resolved at compile time (ACT 0 none, 1 ReLU, 2 leaky ReLU, 3 any: run-time code,
// 4 GELU inline -- conv_g1.h only: ~25 instructions per value where the out-of-line call drains the memory counters per value)
template <int ACT>
__device__ __forceinline__ float act_static(float v, int act, float slope) {
    if (ACT == 0) return v;
    if (ACT == 1) return v > 0.f ? v : 0.f;
    if (ACT == 2) return v > 0.f ? v : v * slope;
    if (ACT == 4) return gelu_erf(v);
    return apply_act(v, act, slope);
}
// epi(full_tag, act_tag): one call, chosen by the layer's activation and by whether the tile lies wholly inside the output
template <typename F>
__device__ __forceinline__ void dispatch_epilogue(int act, bool interior, F&& epi) {
    using T = std::true_type;
    using N = std::false_type;
    if (interior) {
        if (act == AICG_ACT_NONE) epi(T{}, std::integral_constant<int, 0>{});
        else if (act == AICG_ACT_RELU) epi(T{}, std::integral_constant<int, 1>{});
        else if (act == AICG_ACT_LRELU) epi(T{}, std::integral_constant<int, 2>{});
        else epi(T{}, std::integral_constant<int, 3>{});
    } else {
        if (act == AICG_ACT_NONE) epi(N{}, std::integral_constant<int, 0>{});
        else if (act == AICG_ACT_RELU) epi(N{}, std::integral_constant<int, 1>{});
        else if (act == AICG_ACT_LRELU) epi(N{}, std::integral_constant<int, 2>{});
        else epi(N{}, std::integral_constant<int, 3>{});
    }
}

// ceil(2^32 / d): idx / d == umulhi(idx, mul) for idx * d < 2^32 (ConvArgs::div_chs, div_twp)
inline unsigned div_mul(int d) { return (unsigned)((0x100000000ULL + (unsigned long long)d - 1) / (unsigned long long)d); }

}  // namespace aicg
