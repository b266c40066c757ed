// The one global reduction kernel of reduce.h.
#include "reduce.h"

namespace aicg {

__global__ void __launch_bounds__(256) sum_f64_partials_kernel(const float* __restrict__ x, long n, double* __restrict__ part) {
    __shared__ double ws[4];
    const long per = ldiv_up(n, (long)gridDim.x), lo = (long)blockIdx.x * per, hi = lmin(n, lo + per);
    double s = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += 256) s += (double)x[i];
    s = block_sum(s, ws);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

}  // namespace aicg
