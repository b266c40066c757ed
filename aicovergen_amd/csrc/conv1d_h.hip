// Half-storage 1-D convolution for the vocoder's ResBlocks (opt-in: AICG_HALF=1 + AICG_HALF_STORE=1), direct form on the fp16 matrix pipe:
//
//   y = [y +] out_scale * (act(conv_{k,d}(pre_act(x)) + bias) + res)          k in {3, 5, 7, 11}, d in {1, 3, 5}, "same" zero padding
//
// x, res and out are EACH fp16 or fp32 in HBM (a stage's first layer reads the transposed convolution's fp32 output, a chain's last
// layer accumulates into the fp32 stage sum, everything between is fp16: half the bytes of the HBM-side 32 / 64 channel stages).
// Rows are T-contiguous with element strides per batch and channel; nothing is assumed about alignment beyond the element's own
// (an fp16 row of odd length or odd offset is not dword-aligned: activations move as single elements, coalesced along T).
//
// Rounding points: the pre-activated input (once per element, at the staging into LDS), the weights (on the host), the store of an
// fp16 output.  fp16 x fp16 products are exact in fp32; accumulation, bias, activation, residual and scale are fp32.
//
// Tiling: a workgroup of four waves owns 256 outputs x (32 | 64) output channels of one batch row.  Per chunk of 32 input channels it
// stages (a) the pre-activated fp16 input tile plus halo ONCE, transposed to [position][channel] (72-byte rows: the B fragment of
// v_mfma_f32_32x32x8_f16 -- four consecutive channels at one position -- is one ds_read_b64, and every tap is the same read at a row
// offset of tap x d), and (b) the chunk's weights in fragment order (one contiguous 512-byte ds_read_b64 per MFMA).  A wave computes
// 64 positions x every output channel of the workgroup: 2 x MT accumulators, each A and B fragment read feeds two MFMAs.
//
// Summation order of an output element: input-channel groups of 8 ascending, taps ascending inside a group, the MFMA's own order
// inside a group of 8 -- independent of the element's position in the tile or the row (zero padding contributes exact zeros), so a
// windowed run reproduces the full run's bits outside the layers' reach.
#include "common.h"

#include <cstdint>

namespace aicg {

static constexpr int C1H_TT = 256;    // output positions per workgroup
static constexpr int C1H_CC = 32;     // input channels per staged chunk
static constexpr int C1H_ROW = 36;    // halves per LDS input row (32 channels + 4: rows 18 dwords apart -> conflict-free b64 reads per 32 lanes)

struct C1hArgs {
    const void* x;
    const unsigned short* w;   // [Cout_pad / 32][Cin / 8][k][2][32][4] fp16: element e of (m-tile, g, tap, h, i) = W[32 m + i][8 g + 4 h + e][tap]
    const float* bias;
    const void* res;
    void* out;
    long x_sn, x_sc, r_sn, r_sc, o_sn, o_sc;
    int Cin, Cout, T, dil;
    int x_h, r_h, o_h;         // 1: fp16 storage, 0: fp32
    int pre_act, act;
    float pre_slope, act_slope, out_scale;
    int accumulate;
};

__device__ __forceinline__ float c1h_load(const void* base, long off, int is_half) {
    if (is_half) return (float)__builtin_bit_cast(_Float16, reinterpret_cast<const unsigned short*>(base)[off]);
    return reinterpret_cast<const float*>(base)[off];
}

__host__ __device__ inline int c1h_x_halves(int k, int dil) { return ((C1H_TT + (k - 1) * dil) * C1H_ROW + 7) & ~7; }
__host__ __device__ inline size_t c1h_lds_bytes(int k, int dil, int mt) {
    return (size_t)2 * (c1h_x_halves(k, dil) + mt * (C1H_CC / 8) * k * 256);
}

template <int K, int MT>
__global__ void __launch_bounds__(256) conv1d_h_kernel(C1hArgs p) {
    HIP_DYNAMIC_SHARED(float4, smem4)
    unsigned short* xs = reinterpret_cast<unsigned short*>(smem4);
    unsigned short* ws = xs + c1h_x_halves(K, p.dil);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int halo = (K - 1) / 2 * p.dil;
    const int rows = C1H_TT + 2 * halo;
    const int t0 = blockIdx.x * C1H_TT;
    const int n = blockIdx.z;
    const int mt0 = blockIdx.y * MT;
    const int ngroups = p.Cin / 8;

    f32x16 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.f;

    const long xrow = (long)n * p.x_sn;
    for (int c0 = 0; c0 < p.Cin; c0 += C1H_CC) {
        const int cc = imin(C1H_CC, p.Cin - c0);   // 32, or 16 in the last chunk
        const int ncig = cc / 8;
        if (c0) __syncthreads();
        // input: four channels of one position per work item (positions along the lanes: coalesced), rounded once, one 8-byte LDS write
        for (int q = wave; q < cc / 4; q += 4) {
            const long cbase = xrow + (long)(c0 + 4 * q) * p.x_sc;
            for (int r = lane; r < rows; r += 64) {
                const int t = t0 - halo + r;
                float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
                if (t >= 0 && t < p.T) {
                    v0 = c1h_load(p.x, cbase + t, p.x_h);
                    v1 = c1h_load(p.x, cbase + p.x_sc + t, p.x_h);
                    v2 = c1h_load(p.x, cbase + 2 * p.x_sc + t, p.x_h);
                    v3 = c1h_load(p.x, cbase + 3 * p.x_sc + t, p.x_h);
                    v0 = apply_act(v0, p.pre_act, p.pre_slope);
                    v1 = apply_act(v1, p.pre_act, p.pre_slope);
                    v2 = apply_act(v2, p.pre_act, p.pre_slope);
                    v3 = apply_act(v3, p.pre_act, p.pre_slope);
                }
                const H4 hq = pack_f16x4(v0, v1, v2, v3);
                uint2 u;
                u.x = hq.x;
                u.y = hq.y;
                *reinterpret_cast<uint2*>(xs + r * C1H_ROW + 4 * q) = u;
            }
        }
        // weights of the chunk: per m-tile one contiguous piece of the packed image, already in fragment order
        const int n16 = ncig * K * 32;   // 16-byte words per m-tile
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const uint4* src = reinterpret_cast<const uint4*>(p.w + ((size_t)(mt0 + m) * ngroups + c0 / 8) * (K * 256));
            uint4* dst = reinterpret_cast<uint4*>(ws + m * ((C1H_CC / 8) * K * 256));
            for (int i = tid; i < n16; i += 256) dst[i] = src[i];
        }
        __syncthreads();
        const unsigned short* xb = xs + (64 * wave + j) * C1H_ROW + 4 * h;
        const unsigned short* wb = ws + (h * 32 + j) * 4;
        for (int g = 0; g < ncig; ++g) {
#pragma unroll
            for (int tap = 0; tap < K; ++tap) {
                const unsigned short* xr = xb + tap * p.dil * C1H_ROW + 8 * g;
                const uint2 b0 = *reinterpret_cast<const uint2*>(xr);
                const uint2 b1 = *reinterpret_cast<const uint2*>(xr + 32 * C1H_ROW);
                const H4 hb0{b0.x, b0.y}, hb1{b1.x, b1.y};
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const uint2 a = *reinterpret_cast<const uint2*>(wb + (m * (C1H_CC / 8) * K + g * K + tap) * 256);
                    const H4 ha{a.x, a.y};
                    acc[m][0] = mfma_f16_32x32x8(ha, hb0, acc[m][0]);
                    acc[m][1] = mfma_f16_32x32x8(ha, hb1, acc[m][1]);
                }
            }
        }
    }

    // epilogue: lane (j, h) holds position j of its 32-wide tile and output channels (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int t = t0 + 64 * wave + 32 * q + j;
            if (t >= p.T) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = 32 * (mt0 + m) + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (co >= p.Cout) continue;
                float v = acc[m][q][r] + (p.bias ? p.bias[co] : 0.f);
                v = apply_act(v, p.act, p.act_slope);
                if (p.res) v += c1h_load(p.res, (long)n * p.r_sn + (long)co * p.r_sc + t, p.r_h);
                v *= p.out_scale;
                const long o = (long)n * p.o_sn + (long)co * p.o_sc + t;
                if (p.accumulate) v = c1h_load(p.out, o, p.o_h) + v;
                if (p.o_h)
                    reinterpret_cast<unsigned short*>(p.out)[o] = __builtin_bit_cast(unsigned short, (_Float16)v);   // round to nearest even
                else
                    reinterpret_cast<float*>(p.out)[o] = v;
            }
        }
    }
}

template <int K, int MT>
static int launch_c1h(const C1hArgs& p, int N, hipStream_t st) {
    const size_t lds = c1h_lds_bytes(K, p.dil, MT);
    if (lds > 64 * 1024) allow_dynamic_lds((const void*)conv1d_h_kernel<K, MT>, lds);
    const int mtiles = idiv_up(p.Cout, 32 * MT);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(conv1d_h_kernel<K, MT>), dim3((unsigned)idiv_up(p.T, C1H_TT), (unsigned)mtiles, (unsigned)N), dim3(256), lds, st, p);
    return check_launch("conv1d_h_kernel");
}

template <int K>
static int launch_c1h_k(const C1hArgs& p, int N, hipStream_t st) {
    // one m-tile for layers of up to 32 output channels; above, pairs (the packed image is padded to whole pairs)
    return p.Cout <= 32 ? launch_c1h<K, 1>(p, N, st) : launch_c1h<K, 2>(p, N, st);
}

}  // namespace aicg

using namespace aicg;

extern "C" int aicg_conv1d_h_supported(int cin, int cout, int k, int dilation) {
    return (cin >= 16 && cin % 16 == 0 && cout >= 16 && cout % 16 == 0 && (k == 3 || k == 5 || k == 7 || k == 11) &&
            (dilation == 1 || dilation == 3 || dilation == 5)) ? 1 : 0;
}

extern "C" int aicg_conv1d_h(const void* x, const void* w_packed, const float* bias, const void* res, void* out, int N, int Cin, int Cout,
                             int64_t T, int k, int dilation, int x_f16, int res_f16, int out_f16, int64_t x_sn, int64_t x_sc, int64_t r_sn,
                             int64_t r_sc, int64_t o_sn, int64_t o_sc, int pre_act, float pre_slope, int act, float act_slope,
                             float out_scale, int accumulate, void* stream) {
    if (!aicg_conv1d_h_supported(Cin, Cout, k, dilation))
        return fail(AICG_E_ARG, "aicg_conv1d_h: needs Cin, Cout multiples of 16, k in {3, 5, 7, 11}, dilation in {1, 3, 5} (Cin %d, Cout %d, k %d, dilation %d)",
                    Cin, Cout, k, dilation);
    if (!x || !w_packed || !out) return fail(AICG_E_ARG, "aicg_conv1d_h: null pointer");
    if ((pre_act != AICG_ACT_NONE && pre_act != AICG_ACT_LRELU) || (act != AICG_ACT_NONE && act != AICG_ACT_LRELU))
        return fail(AICG_E_ARG, "aicg_conv1d_h: activations are none or leaky ReLU (pre_act %d, act %d)", pre_act, act);
    if (N < 0 || N > 65535 || T < 0 || T > 0x7fff0000) return fail(AICG_E_ARG, "aicg_conv1d_h: N %d, T %lld out of range", N, (long long)T);
    auto al = [](const void* q, int f16) { return q == nullptr || ((uintptr_t)q & (f16 ? 1 : 3)) == 0; };
    if (((uintptr_t)w_packed & 15) || !al(x, x_f16) || !al(res, res_f16) || !al(out, out_f16) || ((uintptr_t)bias & 3))
        return fail(AICG_E_ARG, "aicg_conv1d_h: an operand is not aligned to its element (packed weights: 16 bytes)");
    if (N == 0 || T == 0) return AICG_OK;
    C1hArgs p;
    p.x = x;
    p.w = reinterpret_cast<const unsigned short*>(w_packed);
    p.bias = bias;
    p.res = res;
    p.out = out;
    p.x_sn = (long)x_sn, p.x_sc = (long)x_sc, p.r_sn = (long)r_sn, p.r_sc = (long)r_sc, p.o_sn = (long)o_sn, p.o_sc = (long)o_sc;
    p.Cin = Cin, p.Cout = Cout, p.T = (int)T, p.dil = dilation;
    p.x_h = x_f16 ? 1 : 0, p.r_h = res_f16 ? 1 : 0, p.o_h = out_f16 ? 1 : 0;
    p.pre_act = pre_act, p.act = act;
    p.pre_slope = pre_slope, p.act_slope = act_slope, p.out_scale = out_scale;
    p.accumulate = accumulate ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    switch (k) {
        case 3: return launch_c1h_k<3>(p, N, st);
        case 5: return launch_c1h_k<5>(p, N, st);
        case 7: return launch_c1h_k<7>(p, N, st);
        default: return launch_c1h_k<11>(p, N, st);
    }
}
