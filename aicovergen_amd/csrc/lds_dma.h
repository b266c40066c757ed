// Staging HBM into LDS by DMA: the one place for the pieces, their counted wait and the scheduling fence.
//
// A PIECE is one wave-instruction (buffer_load_dwordx4 ... lds / global_load_lds_dwordx4): lane l fetches 16 bytes and the hardware
// writes them to LDS at M0's base + 16 l -- 1 KiB per instruction, lane-linear destination, no staging registers (the accumulators of
// tdf_pair.hip, conv_w2d.h and the conv_g1 family need them).
//
// Why the DMA and its wait are inline asm and not builtins.  With __builtin_amdgcn_global_load_lds (and the raw-buffer form alike) the
// compiler knows the instruction writes LDS, cannot prove that the destination (the OTHER stage buffer) does not alias the fragment
// reads that follow, and puts an `s_waitcnt vmcnt(0)` in front of the first ds_read: every stage then exposes a full HBM round trip
// before its MFMAs (measured on tdf_pair.hip, r3: 10.2 ms for the level-0 block, of which 3.9 ms remained with every MFMA removed).  The
// asm form is invisible to that pass, so NOTHING orders a piece against the LDS reads of its destination but the kernel itself:
//   * dma_wait<N>() at the end of the stage -- the hand-written counted wait: at most N of this wave's vector-memory operations (its
//     pieces, in issue order) are still in flight -- and the LDS-only barrier (common.h lds_barrier) behind it, which publishes the
//     stage to the other waves;
//   * sched_fence() where the order of issue is the point: the compiler moves nothing across it, so a stage's pieces stay where the
//     pipeline wants them (and index arithmetic stays out of an MFMA stream whose registers it would take).
// M0 carries the wave-uniform LDS base of a piece and is saved and restored around it (the compiler does not know the asm uses it).
// A run of pieces under ONE M0 save / restore is dma_run; what that bought is measured there.
#pragma once
#include <cstdint>

#include "common.h"

namespace aicg {

// One piece through a buffer resource: lane l fetches 16 bytes at buffer offset voff (+ the wave-uniform soff) and the hardware writes
// them to lds_wave_base + 16 l.  Offsets >= the resource's num_records (kBufOob) deposit zeros -- a convolution's padding.
__device__ __forceinline__ void dma16(const BufRsrc& r, unsigned voff, unsigned soff, float* lds_wave_base, int lane) {
#ifdef AICG_EMULATED
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned long)voff + 16 <= r.num_records) __builtin_memcpy(&v, r.base + voff + soff, 16);
    *reinterpret_cast<float4*>(lds_wave_base + 4 * lane) = v;
#else
    (void)lane;
    const unsigned lds = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds_wave_base);
    const unsigned so = __builtin_amdgcn_readfirstlane(soff);
    buf_i32x4 rs;   // wave-uniform by construction; say so (a resource the compiler cannot prove uniform lands in VGPRs)
    rs.x = __builtin_amdgcn_readfirstlane(r.d.x); rs.y = __builtin_amdgcn_readfirstlane(r.d.y);
    rs.z = __builtin_amdgcn_readfirstlane(r.d.z); rs.w = __builtin_amdgcn_readfirstlane(r.d.w);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(rs), "s"(lds), "s"(so)
                 : "memory");
#endif
}
// A RUN of N <= 4 pieces of one resource whose LDS destinations are consecutive KiB (piece e lands at lds_base + 1 KiB x e), issued as ONE
// statement with one M0 save / restore (N calls of dma16 are 9 N instructions + a generic-to-LDS pointer cast with its null check
// each; profiles/NOTES.md R6: the probe's L2-resident burst of 48 pieces lands at 44 B per clock and CU, while conv_w2d's waves stood
// ~3 000 cycles per stage in ~150 issue slots of address arithmetic and three exposed LDS reads).
//   SAME: a contiguous slab (the weights) -- every piece uses the per-lane offset v[0] and the wave-uniform `soff`; the instruction's
//         12-bit immediate advances the memory AND the LDS address by 1 KiB x e (LDS_ADDR = M0 base + inst_offset + 16 x lane): N + 4
//         instructions;
//   else: piece e has its own per-lane offsets v[e] (the patch; kBufOob = padding) and M0 itself is advanced: 3 N + 2 instructions.
template <int N, bool SAME>
__device__ __forceinline__ void dma_run(const BufRsrc& r, const unsigned (&v)[4], unsigned soff, float* lds_base, unsigned lds_addr, int lane) {
    static_assert(N >= 1 && N <= 4, "the immediate offset has 12 bits");
#ifdef AICG_EMULATED
    (void)lds_addr;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const unsigned voff = SAME ? v[0] + 1024u * e : v[e];      // the hardware range-checks voff + the immediate (not the scalar offset)
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned long)voff + 16 <= r.num_records) __builtin_memcpy(&q, r.base + voff + soff, 16);
        *reinterpret_cast<float4*>(lds_base + 256 * e + 4 * lane) = q;
    }
#else
    (void)lane; (void)lds_base;
    buf_i32x4 rs;
    rs.x = __builtin_amdgcn_readfirstlane(r.d.x); rs.y = __builtin_amdgcn_readfirstlane(r.d.y);
    rs.z = __builtin_amdgcn_readfirstlane(r.d.z); rs.w = __builtin_amdgcn_readfirstlane(r.d.w);
    const unsigned lds = __builtin_amdgcn_readfirstlane(lds_addr);
    const unsigned so = __builtin_amdgcn_readfirstlane(soff);
    unsigned keep;
#define DMA_HEAD "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
#define DMA_TAIL "s_mov_b32 m0, %0"
#define DMA_BUMP "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
    if constexpr (SAME) {
        if constexpr (N == 1)
            asm volatile(DMA_HEAD "buffer_load_dwordx4 %4, %1, %3 offen lds\n\t" DMA_TAIL
                         : "=&s"(keep) : "s"(rs), "s"(lds), "s"(so), "v"(v[0]) : "memory");
        else if constexpr (N == 2)
            asm volatile(DMA_HEAD "buffer_load_dwordx4 %4, %1, %3 offen lds\n\tbuffer_load_dwordx4 %4, %1, %3 offen offset:1024 lds\n\t" DMA_TAIL
                         : "=&s"(keep) : "s"(rs), "s"(lds), "s"(so), "v"(v[0]) : "memory");
        else if constexpr (N == 3)
            asm volatile(DMA_HEAD "buffer_load_dwordx4 %4, %1, %3 offen lds\n\tbuffer_load_dwordx4 %4, %1, %3 offen offset:1024 lds\n\t"
                         "buffer_load_dwordx4 %4, %1, %3 offen offset:2048 lds\n\t" DMA_TAIL
                         : "=&s"(keep) : "s"(rs), "s"(lds), "s"(so), "v"(v[0]) : "memory");
        else
            asm volatile(DMA_HEAD "buffer_load_dwordx4 %4, %1, %3 offen lds\n\tbuffer_load_dwordx4 %4, %1, %3 offen offset:1024 lds\n\t"
                         "buffer_load_dwordx4 %4, %1, %3 offen offset:2048 lds\n\tbuffer_load_dwordx4 %4, %1, %3 offen offset:3072 lds\n\t" DMA_TAIL
                         : "=&s"(keep) : "s"(rs), "s"(lds), "s"(so), "v"(v[0]) : "memory");
    } else {
        if constexpr (N == 1)
            asm volatile(DMA_HEAD "buffer_load_dwordx4 %4, %1, %3 offen lds\n\t" DMA_TAIL
                         : "=&s"(keep) : "s"(rs), "s"(lds), "s"(so), "v"(v[0]) : "memory");
        else if constexpr (N == 2)
            asm volatile(DMA_HEAD "buffer_load_dwordx4 %4, %1, %3 offen lds\n\t" DMA_BUMP "buffer_load_dwordx4 %5, %1, %3 offen lds\n\t" DMA_TAIL
                         : "=&s"(keep) : "s"(rs), "s"(lds), "s"(so), "v"(v[0]), "v"(v[1]) : "memory", "scc");
        else if constexpr (N == 3)
            asm volatile(DMA_HEAD "buffer_load_dwordx4 %4, %1, %3 offen lds\n\t" DMA_BUMP "buffer_load_dwordx4 %5, %1, %3 offen lds\n\t"
                         DMA_BUMP "buffer_load_dwordx4 %6, %1, %3 offen lds\n\t" DMA_TAIL
                         : "=&s"(keep) : "s"(rs), "s"(lds), "s"(so), "v"(v[0]), "v"(v[1]), "v"(v[2]) : "memory", "scc");
        else
            asm volatile(DMA_HEAD "buffer_load_dwordx4 %4, %1, %3 offen lds\n\t" DMA_BUMP "buffer_load_dwordx4 %5, %1, %3 offen lds\n\t"
                         DMA_BUMP "buffer_load_dwordx4 %6, %1, %3 offen lds\n\t" DMA_BUMP "buffer_load_dwordx4 %7, %1, %3 offen lds\n\t" DMA_TAIL
                         : "=&s"(keep) : "s"(rs), "s"(lds), "s"(so), "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]) : "memory", "scc");
    }
#undef DMA_HEAD
#undef DMA_TAIL
#undef DMA_BUMP
#endif
}
// One piece from a global address: lane l fetches the 16 bytes at its own g, the hardware writes them to lds_wave_base + 16 l.
__device__ __forceinline__ void lds_dma16(const float* g, float* lds_wave_base, int lane) {
#ifdef AICG_EMULATED
    *reinterpret_cast<float4*>(lds_wave_base + 4 * lane) = *reinterpret_cast<const float4*>(g);
#else
    (void)lane;
    const unsigned lds = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds_wave_base);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(g), "s"(lds)
                 : "memory");
#endif
}
// at most N of this wave's DMA pieces are still in flight (0: every one has landed)
template <int N = 0>
__device__ __forceinline__ void dma_wait() {
#ifndef AICG_EMULATED
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#endif
}
__device__ __forceinline__ void sched_fence() {   // nothing moves across
#ifndef AICG_EMULATED
    __builtin_amdgcn_sched_barrier(0);
#endif
}

}  // namespace aicg
