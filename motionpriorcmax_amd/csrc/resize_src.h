// The source index and weight of a bilinear resize, shared by repr.hip (the fused resize of the centred voxel grid) and
// flow_targets.hip (the ground-truth flow targets): one function, __host__ __device__, IEEE single, no contraction
// (-ffp-contract=off in build.py), so that host and device, and the two translation units, round it the same way.
#pragma once
#include <hip/hip_runtime.h>

// source index and weight of output index j along an axis of `size` entries: F.interpolate(mode='bilinear',
// align_corners=False) -- max(scale * (j + 0.5) - 0.5, 0), the neighbour clamped to the last entry
__host__ __device__ __forceinline__ void repr_src(float scale, int j, int size, int resize, int &i0, int &i1, float &lam) {
    if (!resize) { i0 = i1 = j; lam = 0.f; return; }
    float r = scale * ((float)j + 0.5f) - 0.5f;
    if (r < 0.f) r = 0.f;
    i0 = (int)floorf(r);
    if (i0 > size - 1) i0 = size - 1;
    i1 = i0 + 1 < size ? i0 + 1 : size - 1;
    lam = fminf(fmaxf(r - (float)i0, 0.f), 1.f);
}
