// The flow metrics of the RAFT-spline validation step (what scripts/trajectory_inference.py logs) as one fused reduction.
//   reference: src/modules/raft_spline.py:88-215 (validation_step), src/modules/utils.py:85-296 (epe_masked, ae_masked,
//   n_pixel_error_masked, calculate_flow_error, calculate_trajectory_flow_error), :335-541 (the Metric classes), :67-74 (the
//   linear-motion baseline).  include/mpcmax.h states the formulas and the key order (MPC_VAL_*).
// In plain torch the step writes [M, B, 2, H, W] predictions and runs a few hundred small operators over them, each re-reading
// predictions and ground truth, with a host synchronisation per `if denominator == 0`.  Here:
//   k_val_evmask    ev_repr -> one byte per pixel (E = any channel != 0); skipped when the caller has the mask
//   k_val_partial   grid (pixel chunk, sample n), 256 threads x `ppt` pixels each.  Curves: `up[2d]` of cvx_device.h once per pixel, the
//                   M dot products with the Bernstein rows, the predictions parked in the thread's own LDS slots (2 M floats a
//                   pixel: they would cost 2 M ppt registers); then step by step: ground truth, validity and the E byte read
//                   once, 16 fp64 sums and 16 integer counts per thread over its pixels, a wave reduction by shuffles, the four
//                   waves in order, one slab per (workgroup, step).  `flows` mode reads the caller's predictions in the place
//                   of the LDS slots.
//   k_val_image     one workgroup per (m, n): the slabs of the image in a fixed order (8 interleaved groups, then the groups in order)
//   k_val_final     one workgroup: the sums over the batch, the per-image quotients of FLOW_METRICS_MULTI, then one thread per key
//                   applies the skip / NaN / + 1e-5 rules and writes values and updated
// No atomics; every count is an integer; the order of every sum is fixed by the shape: bitwise reproducible.
// Per-pixel arithmetic in fp32 with one rounding per operation (-ffp-contract=off), as the reference's; sums in fp64.
#include "common.h"
#include "cvx_device.h"

#define VAL_PPT 4                        // pixels per thread of k_val_partial, at most; fewer where ppt * M * 2 KB of LDS slots would pass 60 KB
#define VAL_NQ 16                        // fp64 sums per slab, and as many counts
// slab layout, k = 0 (no mask), 1 (E && V_m), 2 (V_m):
//   sums   [4k] e over K   [4k + 1] a over K   [4k + 2] e over F   [4k + 3] a over F   [12] e_lin   [13] a_lin   [14] e over E   [15] a over E
//   counts [3k] |K|   [3k + 1] |F|   [3k + 2] #_F(e > 3)   [9 + j] r_{j+1}, no mask   [12] |E|   [13 + j] r_{j+1} over E
// (the [9..15] entries belong to the single-step metrics: only step M - 1 fills them)

__global__ __launch_bounds__(256) void k_val_evmask(const float *__restrict__ ev, uint8_t *__restrict__ out, long long total,
                                                    long long HW, int C) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool in = gi < total;
    const long long n = in ? gi / HW : 0, pix = in ? gi - n * HW : 0;
    const float *p = ev + (size_t)n * C * HW + pix;
    bool any = !in;                                    // (lanes past the end never hold the wave back)
    for (int c = 0; c < C; ++c) {
        if (!any) any = p[(size_t)c * HW] != 0.f;      // true for a NaN, as torch.abs(ev_repr).any(dim=1)
        if ((c & 3) == 3 && __all(any)) break;
    }
    if (in) out[gi] = any ? 1 : 0;
}

// the angle between u = (ax, ay, 1) and v = (bx, by, 1), radians: acos(clamp(u.v / (|u| |v|))) of the reference, evaluated as
// atan2(|u x v|, u.v) -- the same angle in [0, pi] (no clamp needed), without the loss of acos near 1: where prediction and ground
// truth nearly agree, the rounding of the quotient alone (2^-24 beside 1) moves an angle of 0.3 degrees by 1e-3 degrees and biases
// the mean low
__device__ __forceinline__ float val_angle(float ax, float ay, float bx, float by) {
    const float dot = ax * bx + ay * by + 1.f;
    const float cx = ay - by, cy = bx - ax, cz = ax * by - ay * bx;
    return atan2f(sqrtf(cx * cx + cy * cy + cz * cz), dot);
}

template <int D>        // D = 0: predictions from `flows`
__global__ __launch_bounds__(256) void k_val_partial(const float *__restrict__ params, const float *__restrict__ mask,
                                                     const float *__restrict__ basis, const float *__restrict__ flows, float scale,
                                                     const float *__restrict__ ts, const float *__restrict__ gt,
                                                     const uint8_t *__restrict__ valid, const uint8_t *__restrict__ evm,
                                                     double *__restrict__ slab_d, unsigned *__restrict__ slab_i, int B, int M, int d,
                                                     int h, int w, int W, long long HW, int nblk, int ppt) {
    extern __shared__ float s_p[];                        // curves: [ppt][M][2][256] the predictions of this thread's pixels (a thread reads back its own slots only)
    __shared__ float s_b[MPC_VAL_MAX_STEPS * CVX_DMAX];   // the basis [M][d]
    __shared__ double s_d[4][VAL_NQ];
    __shared__ unsigned s_i[4][VAL_NQ];
    const int n = blockIdx.y, tid = threadIdx.x;
    const long long pix0 = (long long)blockIdx.x * 256 * ppt + tid;
    if constexpr (D > 0) {
        for (int i = tid; i < M * d; i += 256) s_b[i] = basis[i];
        __syncthreads();
        const size_t plane = (size_t)h * w;
        for (int q = 0; q < ppt; ++q) {
            const long long pix = pix0 + q * 256;
            if (pix >= HW) break;
            const int y = (int)(pix / W), x = (int)(pix - (long long)y * W);
            float ux[D], uy[D];
            cvx_up<D>(params + (size_t)n * 2 * d * plane, mask + (size_t)n * 576 * plane, d, h, w, y, x, ux, uy);
            for (int m = 0; m < M; ++m) {
                float fy = 0.f, fx = 0.f;                   // (the sums of k_cvx_flow_fwd, term by term)
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    if (k < d) { const float bw = s_b[m * d + k]; fy = fy + bw * uy[k]; fx = fx + bw * ux[k]; }
                }
                s_p[((q * M + m) * 2 + 0) * 256 + tid] = fx * scale;
                s_p[((q * M + m) * 2 + 1) * 256 + tid] = fy * scale;
            }
        }
    }
    const int lane = tid & 63, wv = tid >> 6;
    for (int m = 0; m < M; ++m) {
        const float tsm = ts[m];
        const bool last = m == M - 1;
        const float *g = gt + ((size_t)n * M + m) * 2 * HW;
        const uint8_t *vp = valid ? valid + ((size_t)n * M + m) * HW : nullptr;
        const uint8_t *ep = evm + (size_t)n * HW;
        double f[VAL_NQ];
        unsigned c[VAL_NQ];
#pragma unroll
        for (int i = 0; i < VAL_NQ; ++i) { f[i] = 0.0; c[i] = 0u; }
        for (int q = 0; q < ppt; ++q) {
            const long long pix = pix0 + q * 256;
            if (pix >= HW) break;
            float px, py, qx, qy;                               // P_m and P_{M-1}
            if constexpr (D > 0) {
                px = s_p[((q * M + m) * 2 + 0) * 256 + tid]; py = s_p[((q * M + m) * 2 + 1) * 256 + tid];
                qx = s_p[((q * M + M - 1) * 2 + 0) * 256 + tid]; qy = s_p[((q * M + M - 1) * 2 + 1) * 256 + tid];
            } else {
                const float *pm = flows + ((size_t)m * B + n) * 2 * HW + pix, *pl = flows + ((size_t)(M - 1) * B + n) * 2 * HW + pix;
                px = pm[0] * scale; py = pm[HW] * scale; qx = pl[0] * scale; qy = pl[HW] * scale;
            }
            const float gx = g[pix], gy = g[HW + pix];
            const bool V = vp ? vp[pix] != 0 : true, E = ep[pix] != 0;
            const float dx = px - gx, dy = py - gy;
            const float e = sqrtf(dx * dx + dy * dy);
            const float a = val_angle(px, py, gx, gy);
            const bool nz = gx != 0.f && gy != 0.f && !isinf(gx) && !isinf(gy);     // calculate_flow_error's own mask (utils.py:240-243)
            const bool e3 = e > 3.f;
            const bool K[3] = {true, E && V, V};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (K[k]) {
                    f[4 * k] += (double)e; f[4 * k + 1] += (double)a; c[3 * k] += 1u;
                    if (nz) { f[4 * k + 2] += (double)e; f[4 * k + 3] += (double)a; c[3 * k + 1] += 1u; c[3 * k + 2] += e3 ? 1u : 0u; }
                }
            }
            // the linear-motion baseline: timestamps[m] * P_{M-1} (utils.py:67-74)
            const float bx = tsm * qx, by = tsm * qy;
            const float ex = bx - gx, ey = by - gy;
            f[12] += (double)sqrtf(ex * ex + ey * ey);
            f[13] += (double)val_angle(bx, by, gx, gy);
            if (last) {
                const float rel = e / fmaxf(sqrtf(gx * gx + gy * gy), 1e-6f);
                const bool big = rel >= 0.05f;
                const unsigned r1 = (e > 1.f && big) ? 1u : 0u, r2 = (e > 2.f && big) ? 1u : 0u, r3 = (e3 && big) ? 1u : 0u;
                c[9] += r1; c[10] += r2; c[11] += r3;
                if (E) { f[14] += (double)e; f[15] += (double)a; c[12] += 1u; c[13] += r1; c[14] += r2; c[15] += r3; }
            }
        }
#pragma unroll
        for (int i = 0; i < VAL_NQ; ++i) {
            const double sd = wave_sum_d(f[i]);
            unsigned u = c[i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) u += __shfl_down(u, o, 64);
            if (lane == 0) { s_d[wv][i] = sd; s_i[wv][i] = u; }
        }
        __syncthreads();
        if (tid < VAL_NQ) {
            const size_t o = (((size_t)n * M + m) * nblk + blockIdx.x) * VAL_NQ + tid;
            slab_d[o] = ((s_d[0][tid] + s_d[1][tid]) + s_d[2][tid]) + s_d[3][tid];
            slab_i[o] = s_i[0][tid] + s_i[1][tid] + s_i[2][tid] + s_i[3][tid];
        }
        __syncthreads();
    }
}

// one workgroup per image (n * M + m): thread (grp, q) sums quantity q of the slabs grp, grp + 8, ..; then the eight groups in order
__global__ __launch_bounds__(256) void k_val_image(const double *__restrict__ slab_d, const unsigned *__restrict__ slab_i,
                                                   double *__restrict__ img_d, long long *__restrict__ img_i, int nblk) {
    __shared__ double s_d[8][VAL_NQ];
    __shared__ long long s_i[8][VAL_NQ];
    const int q = threadIdx.x & 15, isint = (threadIdx.x >> 4) & 1, grp = threadIdx.x >> 5;
    const size_t base = (size_t)blockIdx.x * nblk * VAL_NQ + q;
    double sd = 0.0;
    long long si = 0;
    for (int b = grp; b < nblk; b += 8) {
        if (isint) si += (long long)slab_i[base + (size_t)b * VAL_NQ];
        else sd += slab_d[base + (size_t)b * VAL_NQ];
    }
    if (isint) s_i[grp][q] = si; else s_d[grp][q] = sd;
    __syncthreads();
    if (threadIdx.x < 2 * VAL_NQ) {
        if (isint) {
            long long t = 0;
            for (int k = 0; k < 8; ++k) t += s_i[k][q];
            img_i[(size_t)blockIdx.x * VAL_NQ + q] = t;
        } else {
            double t = 0.0;
            for (int k = 0; k < 8; ++k) t += s_d[k][q];
            img_d[(size_t)blockIdx.x * VAL_NQ + q] = t;
        }
    }
}

__global__ __launch_bounds__(256) void k_val_final(const double *__restrict__ img_d, const long long *__restrict__ img_i,
                                                   float *__restrict__ values, int32_t *__restrict__ updated, int B, int M) {
    __shared__ double tot_d[MPC_VAL_MAX_STEPS][VAL_NQ];          // sums over the batch, per step
    __shared__ long long tot_i[MPC_VAL_MAX_STEPS][VAL_NQ];
    __shared__ double pim[MPC_VAL_MAX_STEPS][9];                 // per step and mask set: sum over the images of (sum_F e, #_F(e > 3), sum_F a) / (|F| + 1e-5)
    for (int t = threadIdx.x; t < M * 2 * VAL_NQ; t += 256) {
        const int m = t / (2 * VAL_NQ), r = t - m * 2 * VAL_NQ, q = r & 15;
        if (r < VAL_NQ) {
            double s = 0.0;
            for (int n = 0; n < B; ++n) s += img_d[((size_t)n * M + m) * VAL_NQ + q];
            tot_d[m][q] = s;
        } else {
            long long s = 0;
            for (int n = 0; n < B; ++n) s += img_i[((size_t)n * M + m) * VAL_NQ + q];
            tot_i[m][q] = s;
        }
    }
    for (int t = threadIdx.x; t < M * 9; t += 256) {
        const int m = t / 9, r = t - m * 9, k = r / 3, j = r - k * 3;
        double s = 0.0;
        for (int n = 0; n < B; ++n) {
            const size_t o = ((size_t)n * M + m) * VAL_NQ;
            const double cnt = (double)img_i[o + 3 * k + 1] + 1e-5;                   // utils.py:252
            const double num = j == 0 ? img_d[o + 4 * k + 2] : j == 1 ? (double)img_i[o + 3 * k + 2] : img_d[o + 4 * k + 3];
            s += num / cnt;
        }
        pim[m][r] = s;
    }
    __syncthreads();
    const int key = threadIdx.x;
    if (key >= MPC_VAL_COUNT) return;
    const double deg = 180.0 / 3.14159265358979323846, nan = __longlong_as_double(0x7ff8000000000000ll);
    double v = 0.0;
    int up = 1;
    if (key < MPC_VAL_MULTI) {
        // the single-step metrics: step M - 1, no mask (0..4) or E (5..9)
        const int ev = key >= MPC_VAL_MASKED_SINGLE, j = key - (ev ? MPC_VAL_MASKED_SINGLE : 0), m = M - 1;
        const long long cnt = ev ? tot_i[m][12] : tot_i[m][0];
        if (cnt == 0) { v = nan; up = 0; }                      // EPE skips; NPE raises (utils.py:199): the whole row is unpinned
        else if (j == MPC_VAL_EPE) v = (ev ? tot_d[m][14] : tot_d[m][0]) / (double)cnt;
        else if (j == MPC_VAL_AE) v = (ev ? tot_d[m][15] : tot_d[m][1]) / (double)cnt * deg;
        else v = 100.0 * (double)tot_i[m][(ev ? 13 : 9) + j - MPC_VAL_1PE] / (double)cnt;
    } else if (key >= MPC_VAL_EPE_MULTI_LIN) {
        const int ae = key == MPC_VAL_AE_MULTI_LIN;
        double s = 0.0;
        int used = 0;
        for (int m = 0; m < M; ++m) {
            const double cnt = (double)tot_i[m][0];
            if (ae) s += tot_d[m][13] / cnt * deg;
            else if (tot_i[m][0] > 0) { s += tot_d[m][12] / cnt; ++used; }
        }
        if (ae) v = s / (double)M;
        else if (used) v = s / (double)used;
        else { v = nan; up = 0; }
    } else {
        const int k = (key - MPC_VAL_MULTI) / (5 + MPC_VAL_MAX_STEPS), j = (key - MPC_VAL_MULTI) - k * (5 + MPC_VAL_MAX_STEPS);
        if (j == MPC_VAL_EPE_MULTI) {
            double s = 0.0;
            int used = 0;
            for (int m = 0; m < M; ++m)
                if (tot_i[m][3 * k] > 0) { s += tot_d[m][4 * k] / (double)tot_i[m][3 * k]; ++used; }      // a step with an empty mask is skipped
            if (used) v = s / (double)used;
            else { v = nan; up = 0; }
        } else if (j == MPC_VAL_AE_MULTI) {
            double s = 0.0;
            for (int m = 0; m < M; ++m) s += tot_d[m][4 * k + 1] / (double)tot_i[m][3 * k] * deg;         // 0 / 0 = NaN, as ae_masked
            v = s / (double)M;
        } else if (j < MPC_VAL_EPE_STEP) {
            const int r = 3 * k + (j == MPC_VAL_TEPE ? 0 : j == MPC_VAL_T3PE ? 1 : 2);
            double s = 0.0;
            for (int m = 0; m < M; ++m) s += pim[m][r];
            v = s / ((double)M * (double)B) * (j == MPC_VAL_TAE ? deg : 1.0);
        } else if (j - MPC_VAL_EPE_STEP < M) {
            v = pim[j - MPC_VAL_EPE_STEP][3 * k] / (double)B;
        } else {
            up = 0;
        }
    }
    values[key] = (float)v;
    updated[key] = up;
}

struct val_layout {
    int64_t off_evm, off_slab_d, off_slab_i, off_img_d, off_img_i, total;
    int nblk;
};

static int val_check(const char *who, const mpc_val_shape *s) {
    if (!s) { mpc_set_error("%s: null shape", who); return MPC_E_NULL; }
    if (s->B < 0 || s->M < 1 || s->d < 0 || s->C < 0 || s->H < 1 || s->W < 1) { mpc_set_error("%s: bad B / M / d / C / H / W", who); return MPC_E_SHAPE; }
    if (s->d > 0 && (s->h < 1 || s->w < 1 || s->H != 8 * s->h || s->W != 8 * s->w)) { mpc_set_error("%s: with curves H x W must be 8h x 8w", who); return MPC_E_SHAPE; }
    if (s->d > CVX_DMAX || s->M > MPC_VAL_MAX_STEPS) { mpc_set_error("%s: more than %d control points per axis or more than %d steps", who, CVX_DMAX, MPC_VAL_MAX_STEPS); return MPC_E_UNSUPPORTED; }
    const long long HW = (long long)s->H * s->W;
    if (HW > (1ll << 30) || s->B > 65535 || (long long)s->B * HW * (s->C > 0 ? s->C : 1) > (1ll << 40) || (long long)s->B * 576 * HW / 64 > (1ll << 40)) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    return 0;
}

static int val_ppt(const mpc_val_shape *s) {
    const int fit = 30 / s->M;                      // ppt * M * 2 * 256 floats <= 60 KB (`flows` mode chunks alike: the same order of every sum, the same bits)
    return fit < 1 ? 1 : fit < VAL_PPT ? fit : VAL_PPT;
}

static val_layout val_lay(const mpc_val_shape *s) {
    val_layout L;
    const int64_t HW = (int64_t)s->H * s->W, img = (int64_t)s->B * s->M;
    const int64_t chunk = 256 * (int64_t)val_ppt(s);
    L.nblk = (int)((HW + chunk - 1) / chunk);
    int64_t o = 0;
    L.off_evm = o;    o += mpc_align(s->C > 0 ? (int64_t)s->B * HW : 0);
    L.off_slab_d = o; o += mpc_align(img * L.nblk * VAL_NQ * (int64_t)sizeof(double));
    L.off_slab_i = o; o += mpc_align(img * L.nblk * VAL_NQ * (int64_t)sizeof(unsigned));
    L.off_img_d = o;  o += mpc_align(img * VAL_NQ * (int64_t)sizeof(double));
    L.off_img_i = o;  o += mpc_align(img * VAL_NQ * (int64_t)sizeof(long long));
    L.total = o > 256 ? o : 256;
    return L;
}

extern "C" int64_t mpc_val_metrics_workspace_bytes(const mpc_val_shape *s) {
    int rc = val_check(__func__, s);
    if (rc) return rc;
    return val_lay(s).total;
}

extern "C" int mpc_val_metrics(const mpc_val_shape *s, const float *params, const float *up_mask, const float *basis, const float *flows,
                               float scale, const float *timestamps, const float *flow_gt, const uint8_t *flow_valid, const float *ev_repr,
                               const uint8_t *event_mask, float *values, int32_t *updated, void *ws, void *stream) {
    int rc = val_check(__func__, s);
    if (rc) return rc;
    if (s->B == 0) return 0;
    const bool curves = s->d > 0;
    if (!timestamps || !flow_gt || !values || !updated || !ws || (curves ? (!params || !up_mask || !basis) : !flows)) { mpc_set_error("%s: null argument", __func__); return MPC_E_NULL; }
    if ((s->C > 0) != (ev_repr != nullptr) || (ev_repr != nullptr) == (event_mask != nullptr)) { mpc_set_error("%s: exactly one of ev_repr (C > 0) / event_mask (C = 0)", __func__); return MPC_E_NULL; }
    const val_layout L = val_lay(s);
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)ws;
    const long long HW = (long long)s->H * s->W;
    const uint8_t *evm = event_mask;
    if (ev_repr) {
        uint8_t *out = (uint8_t *)(base + L.off_evm);
        const long long total = (long long)s->B * HW;
        MPC_LAUNCH(k_val_evmask, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ev_repr, out, total, HW, s->C);
        MPC_CHECK_LAUNCH();
        evm = out;
    }
    double *slab_d = (double *)(base + L.off_slab_d), *img_d = (double *)(base + L.off_img_d);
    unsigned *slab_i = (unsigned *)(base + L.off_slab_i);
    long long *img_i = (long long *)(base + L.off_img_i);
    const dim3 grid((unsigned)L.nblk, (unsigned)s->B);
    const int ppt = val_ppt(s);
    const size_t lds = curves ? (size_t)ppt * s->M * 2 * 256 * sizeof(float) : 0;
#define VAL_PARTIAL(DD)                                                                                                         \
    MPC_LAUNCH(k_val_partial<DD>, grid, dim3(256), lds, st, params, up_mask, basis, flows, scale, timestamps, flow_gt, flow_valid, evm, \
               slab_d, slab_i, s->B, s->M, s->d, s->h, s->w, s->W, HW, L.nblk, ppt)
    if (!curves) VAL_PARTIAL(0);
    else if (s->d <= 4) VAL_PARTIAL(4);
    else if (s->d <= 10) VAL_PARTIAL(10);
    else VAL_PARTIAL(CVX_DMAX);
#undef VAL_PARTIAL
    MPC_CHECK_LAUNCH();
    MPC_LAUNCH(k_val_image, dim3((unsigned)(s->B * s->M)), dim3(256), 0, st, slab_d, slab_i, img_d, img_i, L.nblk);
    MPC_CHECK_LAUNCH();
    MPC_LAUNCH(k_val_final, dim3(1), dim3(256), 0, st, img_d, img_i, values, updated, s->B, s->M);
    MPC_CHECK_LAUNCH();
    return 0;
}
