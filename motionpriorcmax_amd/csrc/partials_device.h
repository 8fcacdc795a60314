// The finishing pass of the two-phase sums of a learned basis' gradient (grid_traj.hip: k_grid_dphi_sum; curve_basis.hip:
// k_curve_basis_sum): element e of a [P][ne] array of per-workgroup partials summed over p in ONE fixed order -- thread i of 256
// adds p = i, i + 256, ... ascending, then a halving tree over the 256 thread sums in LDS.  No float atomics: bitwise reproducible,
// whatever the order in which the workgroups that wrote the partials ran.  P = 0 gives 0.
#pragma once
#include <hip/hip_runtime.h>

// the sum, valid in thread 0; a workgroup of 256 threads, s: 256 floats of LDS (one barrier behind the last read)
__device__ __forceinline__ float mpc_partials_sum(const float *__restrict__ part, long long P, int ne, int e, float *s) {
    float v = 0.f;
    for (long long p = threadIdx.x; p < P; p += 256) v = v + part[p * ne + e];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + h];
        __syncthreads();
    }
    return s[0];
}
