// The per-pixel body and the partial-sum layout of the flow error metrics (reference src/utils/flow.py:18-70), shared by the two
// kernels that differ only in where the ground truth comes from: decoded fp32 planes + a byte mask (flow.hip: mpc_flow_error) and
// the DSEC 16-bit payload itself (dsec_io.hip: mpc_dsec_flow_error).  Same pixels per thread, same order of the sums.
#pragma once
#include "common.h"

#define FE_BLOCKS 64          // partial-sum workgroups per sample
#define FE_NACC 6             // epe, >1, >2, >3, acos, n_points

struct FeAcc {
    double v[FE_NACC];
};

__device__ __forceinline__ void fe_pixel(float g0, float g1, float p0, float p1, bool em, float ts, bool has_ts,
                                         FeAcc &a) {
    const bool fm = !isinf(g0) && !isinf(g1) && fabsf(g0) > 0.f && fabsf(g1) > 0.f;
    const float m = (fm && em) ? 1.f : 0.f;
    g0 *= m; g1 *= m; p0 *= m; p1 *= m;                       // a product as in flow.py:48-49 (inf * 0 = nan)
    if (has_ts) { g0 *= ts; g1 *= ts; p0 *= ts; p1 *= ts; }
    const float d0 = g0 - p0, d1 = g1 - p1;
    const float epe = sqrtf(d0 * d0 + d1 * d1);
    a.v[0] += (double)epe;
    a.v[1] += epe > 1.f ? 1.0 : 0.0;
    a.v[2] += epe > 2.f ? 1.0 : 0.0;
    a.v[3] += epe > 3.f ? 1.0 : 0.0;
    // channel 0 is "u", channel 1 is "v" (flow.py:63-64)
    float cs = (1.0f + p0 * g0 + p1 * g1) / (sqrtf(1.f + p0 * p0 + p1 * p1) * sqrtf(1.f + g0 * g0 + g1 * g1));
    cs = cs < -1.f ? -1.f : (cs > 1.f ? 1.f : cs);            // torch.clamp keeps nan
    a.v[4] += (double)acosf(cs);
    a.v[5] += (double)m;
}

// flow.hip: k_flow_err_final on `st` -- part [B][FE_BLOCKS][FE_NACC] -> out[5]
void mpc_flow_err_final(const mpc_err_shape *s, const double *part, float *out, hipStream_t st);
