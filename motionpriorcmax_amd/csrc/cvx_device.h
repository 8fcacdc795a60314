// The per-pixel half of the RAFT-spline output head, shared by cvx_curves.hip (trajectories, dense flows, their adjoint) and
// val_metrics.hip (the validation metrics evaluate the same curves in registers): ONE implementation of the softmax weights and
// of the upsampled control values, so that every caller rounds alike (formulas: the head of cvx_curves.hip).
#pragma once
#include "common.h"
#include "dt_device.h"         // M, the element type of the mask: float, mpc_f16 or mpc_bf16 (mpc_ld: exact)

#define CVX_DMAX 16            // control points per axis held in registers (as CURVE_DMAX of curves.hip)

// the softmax weights of pixel (y, x); mb: the mask of the sample, [576][h][w]
template <typename M>
__device__ __forceinline__ void cvx_softmax9(const M *__restrict__ mb, int h, int w, int y, int x, float wk[9]) {
    const int cy = y >> 3, sy = y & 7, cx = x >> 3, sx = x & 7;
    const size_t plane = (size_t)h * w;
    const M *m = mb + (size_t)(sy * 8 + sx) * plane + (size_t)cy * w + cx;
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) { wk[k] = mpc_ld(m + (size_t)k * 64 * plane); mx = fmaxf(mx, wk[k]); }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) { wk[k] = expf(wk[k] - mx); s = s + wk[k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = wk[k] / s;
}

// the upsampled control values of pixel (y, x): ux / uy [j] for control point j (channels j and d + j); pb: the sample's params [2d][h][w]
template <int D, typename M>
__device__ __forceinline__ void cvx_up(const float *__restrict__ pb, const M *__restrict__ mb, int d, int h, int w, int y, int x,
                                       float ux[D], float uy[D]) {
    float wk[9];
    cvx_softmax9(mb, h, w, y, x, wk);
    const int cy = y >> 3, cx = x >> 3;
    const size_t plane = (size_t)h * w;
#pragma unroll
    for (int j = 0; j < D; ++j) ux[j] = uy[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int ny = cy + k / 3 - 1, nx = cx + k % 3 - 1;
        if (ny < 0 || ny >= h || nx < 0 || nx >= w) continue;           // the zero padding: such a term adds 0
        const float *pn = pb + (size_t)ny * w + nx;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (j < d) {
                ux[j] = ux[j] + wk[k] * (8.f * pn[(size_t)j * plane]);
                uy[j] = uy[j] + wk[k] * (8.f * pn[(size_t)(d + j) * plane]);
            }
        }
    }
}
