// The one skeleton of the kernels that build a chunk of perturbed rows for the classifier forward (Occlusion / FeatureAblation,
// the Shapley coalitions, FeaturePermutation, the perturbation curves, 2-D occlusion): out[r][:] = row g = row0 + r of the
// method's batch, r < rows, n samples per row.  The rows only select values (x, the baseline, another clip's x, NaN); they are
// memory-bound and tiny next to the forward they feed (one forward row is on the order of a GFLOP, building it moves ~12 B per
// sample), so the skeleton stays simple: a grid-stride loop, one float4 store per item when every row pointer is 16-byte aligned
// and n % 4 == 0 (the caller's `vec`), one scalar store per item otherwise.
//
// A method supplies a Rule, passed to the kernel by value:
//   long   n() const                          samples per row
//   Row    row(long g) const                  the state of row g: its row pointers and whether it is a pad row (a row past the
//                                             method's table: a copy of x[g % B] that reads none of the tables)
//   float4 quad(const Row&, long t) const     samples t .. t + 3 of the row, t % 4 == 0 (only for rules launched with HAS_VEC)
//   float  one(const Row&, long t) const      sample t of the row
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace advh {

template <bool VEC, class Rule>
__global__ __launch_bounds__(256) void build_rows_kernel(Rule rule, long row0, int rows, float* __restrict__ out) {
    const long n = rule.n(), per = VEC ? n / 4 : n, total = (long)rows * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / per, q = i - r * per;
        const auto row = rule.row(row0 + r);
        if constexpr (VEC)
            *(float4*)(out + r * n + q * 4) = rule.quad(row, q * 4);
        else
            out[r * n + q] = rule.one(row, q);
    }
}

// Launches the skeleton for rows [row0, row0 + rows).  HAS_VEC = false: the rule has no quad(), only the scalar form exists.
template <bool HAS_VEC = true, class Rule>
static inline int build_rows(const Rule& rule, bool vec, long row0, int rows, float* out, hipStream_t s) {
    if (rows == 0) return ADVH_OK;
    const dim3 grid(grid_for((long)rows * (vec ? rule.n() / 4 : rule.n())));
    if constexpr (HAS_VEC) {
        if (vec) {
            hipLaunchKernelGGL((build_rows_kernel<true, Rule>), grid, dim3(256), 0, s, rule, row0, rows, out);
            return ADVH_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL((build_rows_kernel<false, Rule>), grid, dim3(256), 0, s, rule, row0, rows, out);
    return ADVH_LAUNCH_CHECK();
}

}  // namespace advh
