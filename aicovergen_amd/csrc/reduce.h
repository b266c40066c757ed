// Reductions of the signal kernels: over a 64-lane wave, over a 256-thread workgroup (four waves), and the global float64 sum.
// The f0 and hand-over kernels promise the same bits from two calls; that rests on the order of every floating-point addition, and
// this is where the order is defined:
//   * a wave: the xor butterfly with partner distance 32, 16, 8, 4, 2, 1 -- both lanes of a pair add the same two numbers, so all 64
//     lanes end with the same bits;
//   * a workgroup: ((w0 + w1) + w2) + w3 over the four waves' sums;
//   * a whole signal: block b of sum_f64_partials_kernel owns a contiguous share, its thread t adds elements t, t + 256, ... in
//     ascending order, then the two steps above; sum_of_partials adds partials l, l + 64, ... in lane l, then the wave butterfly.
// A maximum is exact, so its order is free; it takes the same butterfly.
#pragma once
#include "common.h"

namespace aicg {

constexpr int kSumPartials = 256;   // blocks of sum_f64_partials_kernel = partial sums a global mean is added from

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// The sum over a 256-thread workgroup, in every thread; sh holds four values.  There is no barrier in front of the store: a caller
// that has read sh since the last barrier places its own.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// part[b] = sum of block b's contiguous share of x, float64 (reduce.hip); launched over kSumPartials blocks of 256 threads
__global__ void __launch_bounds__(256) sum_f64_partials_kernel(const float* __restrict__ x, long n, double* __restrict__ part);

// the total of the partial sums, the same bits in every lane of every wave that calls it
__device__ __forceinline__ double sum_of_partials(const double* __restrict__ part, int n_part) {
    double s = 0.0;
    for (int b = threadIdx.x & 63; b < n_part; b += 64) s += part[b];
    return wave_sum(s);
}

// max over the calling waves into *bits, which the caller zeroed: non-negative floats order like their bit patterns, so this is one
// integer atomic max per wave
__device__ __forceinline__ void peak_commit(float m, unsigned* __restrict__ bits) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(bits, (unsigned)__float_as_int(m));
}

}  // namespace aicg
