// One event row on the device: its six columns, its LUT cell, its warp and vote weights, its position gradient.  Read by events.hip
// (the loss path), pe_basis.hip and pe_curves.hip (the per-event warps, through pe_device.h) and ev_order.hip (the counting sort).
#pragma once
#include "ev_key_device.h"

struct EvParams {
    int B, M, Mp, nb, T, H, W, sp, hq, wq, P;
    unsigned flags;
};

struct Warped {
    float y, x, w;     // warped position and event weight
    int lut;           // index of the LUT cell (b,bin,iy,ix) -> element offset / (2T) ... see below
    float fy, fx;      // fractional parts
    int y0, x0;        // top-left tap
    int it, iy, ix;    // time bin and LUT cell of the (unwarped) event
};

__device__ __forceinline__ EvParams make_params(const mpc_shape s) {
    EvParams p;
    p.B = s.B; p.M = s.M; p.Mp = s.Mp; p.nb = s.nb; p.T = s.T; p.H = s.H; p.W = s.W;
    p.sp = s.sp; p.hq = s.hq; p.wq = s.wq;
    p.P = (s.flags & MPC_F_POLARITY_SPLIT) ? 2 : 1;
    p.flags = s.flags;
    return p;
}

// Warp one event for reference time `tr`.  `e` = the 6 columns of the event row.
// Returns false if the event contributes nothing (weight exactly 0).
// LUT cell of an event (ev_key_device.h)
__device__ __forceinline__ void warp_cell(const EvParams &p, const float e[6], int b, int tr, Warped &o) {
    const int it = (int)e[4], iy = ev_cell_raw(e[0], p.sp), ix = ev_cell_raw(e[1], p.sp);
    o.it = ev_clamp(it, p.nb); o.iy = ev_clamp(iy, p.hq); o.ix = ev_clamp(ix, p.wq);
    o.lut = (((b * p.nb + o.it) * p.hq + o.iy) * p.wq + o.ix) * p.T + tr;
}

// Warp with the flow `f` of the event's LUT cell already at hand (warp_cell + a read of the table).
__device__ __forceinline__ bool warp_event_with(const EvParams &p, const float e[6], const float2 f, float t_ref, Warped &o) {
    float w = (p.flags & MPC_F_UNIT_WEIGHT) ? 1.0f : e[5];
    float y = e[0], x = e[1];
    if (!(p.flags & MPC_F_NO_WARP)) {
        // focus.py:191: pos = lut + event
        y = f.x + e[0];
        x = f.y + e[1];
    }
    if (p.flags & MPC_F_SCALE_BY_DT) {
        // focus.py:204-206: (1 - clamp(|t - t_ref|, 0, 1)) * w
        const float dt = fminf(fmaxf(fabsf(e[2] - t_ref), 0.f), 1.f);
        w = (1.f - dt) * w;
    }
    if (p.flags & MPC_F_MASK_BORDER) {
        // focus.py:208-214: strict comparisons
        if (y > (float)p.H || x > (float)p.W || y < 0.f || x < 0.f) w = 0.f;
    }
    o.y = y; o.x = x; o.w = w;
    // event_image_converter.py:357-359
    const float y0f = floorf(y + 1e-6f), x0f = floorf(x + 1e-6f);
    o.fy = y - y0f;
    o.fx = x - x0f;
    // positions far outside the image cannot touch it; keep the int conversion defined
    o.y0 = (int)fminf(fmaxf(y0f, -4.f), (float)p.H + 4.f);
    o.x0 = (int)fminf(fmaxf(x0f, -4.f), (float)p.W + 4.f);
    return w != 0.f;
}

__device__ __forceinline__ bool warp_event(const EvParams &p, const float e[6], int b, int tr,
                                           const float *__restrict__ lut, float t_ref, Warped &o) {
    o.lut = -1;
    float2 f = make_float2(0.f, 0.f);
    if (!(p.flags & MPC_F_NO_WARP)) {
        warp_cell(p, e, b, tr, o);
        f = reinterpret_cast<const float2 *>(lut)[o.lut];
    }
    return warp_event_with(p, e, f, t_ref, o);
}

__device__ __forceinline__ void load_event(const float *__restrict__ events, size_t row, float e[6]) {
    const float2 *p = reinterpret_cast<const float2 *>(events + row * 6);
    const float2 a = p[0], b = p[1], c = p[2];
    e[0] = a.x; e[1] = a.y; e[2] = b.x; e[3] = b.y; e[4] = c.x; e[5] = c.y;
}

// per-event gradient w.r.t. the warped position, unscaled
__device__ __forceinline__ void event_pos_grad(const EvParams &p, const Warped &o,
                                               const float *__restrict__ g /* image */, float &gy,
                                               float &gx) {
    const bool yin0 = o.y0 >= 0 && o.y0 < p.H, yin1 = o.y0 + 1 >= 0 && o.y0 + 1 < p.H;
    const bool xin0 = o.x0 >= 0 && o.x0 < p.W, xin1 = o.x0 + 1 >= 0 && o.x0 + 1 < p.W;
    const float g00 = (yin0 && xin0) ? g[(size_t)o.y0 * p.W + o.x0] : 0.f;
    const float g10 = (yin1 && xin0) ? g[(size_t)(o.y0 + 1) * p.W + o.x0] : 0.f;
    const float g01 = (yin0 && xin1) ? g[(size_t)o.y0 * p.W + o.x0 + 1] : 0.f;
    const float g11 = (yin1 && xin1) ? g[(size_t)(o.y0 + 1) * p.W + o.x0 + 1] : 0.f;
    gy = o.w * ((1.f - o.fx) * (g10 - g00) + o.fx * (g11 - g01));
    gx = o.w * ((1.f - o.fy) * (g01 - g00) + o.fy * (g11 - g10));
}
