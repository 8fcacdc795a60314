// Contrast objective on the Image of Warped Events: 3x3 Gaussian blur (reflect), Sobel (zero pad),
// gradient-magnitude / variance reductions, and the hand-derived adjoint image.
//   forward  : reference src/utils/event_image_converter.py:170-175 + src/utils/loss.py:4-27,58-87
//   backward : SURVEY.md 8a row A11 (closed form of what autograd does in the reference)
// HBM-bound stencils: every image is read once and written once per kernel, tiles are staged
// in LDS with their halo, reductions use wavefront shuffles and fp64 block partials.
#include "common.h"
#include "bounds.h"
#include "contrast_march.h"
#include <stdlib.h>

// ------------------------------------------------------------------------------------------
// forward: raw -> blurred (+ per-block partial sums)
// grid (ceil(W/64), ceil(H/32), nimg), 256 threads
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_contrast_fwd(const float *__restrict__ raw,
                                                      float *__restrict__ blur,
                                                      double *__restrict__ part, int H, int W,
                                                      int norm_l2, int variance) {
    constexpr int TH = MPC_CT_H, TW = MPC_CT_W;
    __shared__ float s_raw[TH + 4][TW + 4 + 1];
    __shared__ float s_hb[TH + 4][TW + 2 + 1];
    __shared__ float s_bl[TH + 2][TW + 2 + 1];
    __shared__ double s_red[2][4];
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t img_off = (size_t)blockIdx.z * H * W;
    const float *src = raw + img_off;
    float ka, kc;
    blur_taps(ka, kc);

    // stage raw tile with a 2-px halo; coordinates -1 and H (W) are the reflect-padding ring
    for (int i = tid; i < (TH + 4) * (TW + 4); i += 256) {
        const int ly = i / (TW + 4), lx = i - ly * (TW + 4);
        const int y = ty0 - 2 + ly, x = tx0 - 2 + lx;
        float v = 0.f;
        if (y >= -1 && y <= H && x >= -1 && x <= W) v = src[(size_t)reflect1(y, H) * W + reflect1(x, W)];
        s_raw[ly][lx] = v;
    }
    __syncthreads();
    // horizontal pass: columns tx0-1 .. tx0+TW
    for (int i = tid; i < (TH + 4) * (TW + 2); i += 256) {
        const int ly = i / (TW + 2), lx = i - ly * (TW + 2);
        s_hb[ly][lx] = ka * s_raw[ly][lx] + kc * s_raw[ly][lx + 1] + ka * s_raw[ly][lx + 2];
    }
    __syncthreads();
    // vertical pass: rows ty0-1 .. ty0+TH ; zero outside the image (Sobel uses zero padding)
    for (int i = tid; i < (TH + 2) * (TW + 2); i += 256) {
        const int ly = i / (TW + 2), lx = i - ly * (TW + 2);
        const int y = ty0 - 1 + ly, x = tx0 - 1 + lx;
        float v = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W)
            v = ka * s_hb[ly][lx] + kc * s_hb[ly + 1][lx] + ka * s_hb[ly + 2][lx];
        s_bl[ly][lx] = v;
    }
    __syncthreads();

    double acc0 = 0.0, acc1 = 0.0;
    const int cx = tid & 63;
    for (int ry = tid >> 6; ry < TH; ry += 4) {
        const int y = ty0 + ry, x = tx0 + cx;
        if (y < H && x < W) {
            const int ly = ry + 1, lx = cx + 1;
            const float b = s_bl[ly][lx];
            blur[img_off + (size_t)y * W + x] = b;
            if (variance) {
                acc0 += (double)b;
                acc1 += (double)b * (double)b;
            } else {
                const float tl = s_bl[ly - 1][lx - 1], tc = s_bl[ly - 1][lx], tr = s_bl[ly - 1][lx + 1];
                const float ml = s_bl[ly][lx - 1], mr = s_bl[ly][lx + 1];
                const float bl_ = s_bl[ly + 1][lx - 1], bc = s_bl[ly + 1][lx], br = s_bl[ly + 1][lx + 1];
                const float dx = (tr - tl) + 2.f * (mr - ml) + (br - bl_);
                const float dy = (bl_ - tl) + 2.f * (bc - tc) + (br - tr);
                acc0 += norm_l2 ? (double)(dx * dx + dy * dy) : (double)(fabsf(dx) + fabsf(dy));
            }
        }
    }
    const double r0 = block_sum_d<256>(acc0, s_red[0]);
    const double r1 = block_sum_d<256>(acc1, s_red[1]);
    if (tid == 0) {
        const size_t bid = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[2 * bid] = r0;
        part[2 * bid + 1] = r1;
    }
}

// fused forward + adjoint image (gradient magnitude), MARCHING form: contrast_march_body (contrast_march.h, where its description
// lives) on the raw IWE itself.  grid (ceil(W/56), ceil(H/TH), nimg), 64 threads
template <bool L2N, int TH>
__global__ __launch_bounds__(64) void k_contrast_march(const float *__restrict__ raw, float *__restrict__ blur,
                                                       float *__restrict__ gimg, double *__restrict__ part, int H, int W,
                                                       int nslots) {
    contrast_march_body<L2N, TH>(raw, blur, gimg, part, H, W, nslots, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y, gridDim.z);
}

// ------------------------------------------------------------------------------------------
// backward (variance objective): blurred -> Blur^T (x - mean_img)   (unscaled)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_image_means(const double *__restrict__ part,
                                                     float *__restrict__ means, int tiles_per_img,
                                                     int HW) {
    __shared__ double s_red[4];
    const int img = blockIdx.x;
    double a = 0.0;
    for (int i = threadIdx.x; i < tiles_per_img; i += 256) a += part[2 * ((size_t)img * tiles_per_img + i)];
    const double r = block_sum_d<256>(a, s_red);
    if (threadIdx.x == 0) means[img] = (float)(r / (double)HW);
}

__global__ __launch_bounds__(256) void k_contrast_bwd_var(const float *__restrict__ blur,
                                                          const float *__restrict__ means,
                                                          float *__restrict__ gimg, int H, int W) {
    constexpr int TH = MPC_CT_H, TW = MPC_CT_W;
    __shared__ float s_gb[TH + 2][TW + 2 + 1];
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t img_off = (size_t)blockIdx.z * H * W;
    const float mean = means[blockIdx.z];
    float ka, kc;
    blur_taps(ka, kc);
    for (int i = tid; i < (TH + 2) * (TW + 2); i += 256) {
        const int ly = i / (TW + 2), lx = i - ly * (TW + 2);
        const int y = ty0 - 1 + ly, x = tx0 - 1 + lx;
        s_gb[ly][lx] = (y >= 0 && y < H && x >= 0 && x < W) ? blur[img_off + (size_t)y * W + x] - mean : 0.f;
    }
    __syncthreads();
    const int cx = tid & 63;
    for (int ry = tid >> 6; ry < TH; ry += 4) {
        const int y = ty0 + ry, x = tx0 + cx;
        if (y < H && x < W) {
            float acc = 0.f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int qy = y + dy;
                if (qy < 0 || qy >= H) continue;
                const float wy = blurT_w(qy, y, H, ka, kc);
                float row = 0.f;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int qx = x + dx;
                    if (qx < 0 || qx >= W) continue;
                    row += blurT_w(qx, x, W, ka, kc) * s_gb[ry + 1 + dy][cx + 1 + dx];
                }
                acc += wy * row;
            }
            gimg[img_off + (size_t)y * W + x] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------
// finalize: fp64 reduction of the partials -> device scalars
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_finalize(const double *__restrict__ cpart, int n_cblocks,
                                                  int tiles_per_img, int nimg, int HW,
                                                  const double *__restrict__ spart, int n_sblocks,
                                                  double smooth_count, float smooth_weight,
                                                  int variance, float *__restrict__ scal, float *__restrict__ scal_out) {
    __shared__ double s_red[2][16];
    __shared__ double s_var;
    const int tid = threadIdx.x;
    double val = 0.0, gcoef = 0.0;
    // (the thread's share of the smoothness partials is read here, with the contrast partials, not after their reduction:
    // one memory round trip of this single-workgroup kernel instead of two)
    // (eight partials of a thread requested together, then added in index order -- the sums keep their association; one
    // load per loop trip made this kernel a chain of memory round trips: 9 us at C3 for 20k doubles)
    double sm_a = 0.0, sm_b = 0.0;
    for (int i0 = tid; i0 < n_sblocks; i0 += 8 * 1024) {
        double2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 1024;
            v[u] = (i < n_sblocks) ? reinterpret_cast<const double2 *>(spart)[i] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u * 1024 < n_sblocks) { sm_a += v[u].x; sm_b += v[u].y; }
    }
    if (!variance) {
        double a = 0.0;
        for (int i0 = tid; i0 < n_cblocks; i0 += 8 * 1024) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int i = i0 + u * 1024; v[u] = (i < n_cblocks) ? cpart[2 * (size_t)i] : 0.0; }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i0 + u * 1024 < n_cblocks) a += v[u];
        }
        const double tot = block_sum_d<1024>(a, s_red[0]);
        const double N = (double)nimg * (double)HW;
        val = tot / N;
        gcoef = -1.0 / (val * val) / N;
    } else {
        // mean over images of the unbiased variance over H*W (loss.py:14-16)
        if (tid == 0) s_var = 0.0;
        __syncthreads();
        for (int img = 0; img < nimg; ++img) {
            double a = 0.0, b = 0.0;
            for (int i = tid; i < tiles_per_img; i += 1024) {
                a += cpart[2 * ((size_t)img * tiles_per_img + i)];
                b += cpart[2 * ((size_t)img * tiles_per_img + i) + 1];
            }
            const double s1 = block_sum_d<1024>(a, s_red[0]);
            const double s2 = block_sum_d<1024>(b, s_red[1]);
            if (tid == 0) s_var += (s2 - s1 * s1 / (double)HW) / (double)(HW - 1);
        }
        __syncthreads();
        val = s_var / (double)nimg;
        gcoef = -1.0 / (val * val) * 2.0 / ((double)(HW - 1) * (double)nimg);
    }
    double smooth = 0.0;
    if (n_sblocks > 0) {
        const double sx = block_sum_d<1024>(sm_a, s_red[0]);
        const double sy = block_sum_d<1024>(sm_b, s_red[1]);
        smooth = (double)smooth_weight * ((sx / smooth_count + sy / smooth_count) / 2.0);
    }
    if (tid == 0) {
        const double focus = 1.0 / val;
        scal[MPC_SCAL_LOSS] = (float)(focus + smooth);
        scal[MPC_SCAL_FOCUS] = (float)focus;
        scal[MPC_SCAL_SMOOTH] = (float)smooth;
        scal[MPC_SCAL_VAL] = (float)val;
        scal[MPC_SCAL_GCOEF] = (float)gcoef;
        scal[5] = scal[6] = scal[7] = 0.f;
        if (scal_out != nullptr) { scal_out[0] = (float)(focus + smooth); scal_out[1] = (float)focus; scal_out[2] = (float)smooth; }
    }
}

__global__ void k_scale(const float *__restrict__ x, const float *__restrict__ a,
                        float *__restrict__ y, int64_t n) {
    const float s = a[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        y[i] = s * x[i];
}

// ------------------------------------------------------------------------------------------
// host entry points
// ------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------
// smoothness, MARCHING form (as k_contrast_march: lane = column, rows walked with rolling register windows, DPP lane
// shifts, no LDS, no barrier): one wavefront owns 60 cell columns (+ 2 halo each side) and MPC_SM_H rows (+ 2) of one
// channel pair.  Same sums, in the same association, as round 1's LDS-tiled kernel had (removed in round 4).
// grid (ceil(wq/60), ceil(hq/MPC_SM_H), nimg*C/2), 64 threads
// ------------------------------------------------------------------------------------------
// TH rows per band: MPC_SM_H (16), or half of it for small fields (smooth_band_rows below)
template <int TH>
__device__ __forceinline__ void lut_smooth_march_body(const float *__restrict__ field, float *__restrict__ gfield,
                                                      double *__restrict__ part, int hq, int wq, int C, float gscale,
                                                      unsigned bx, unsigned by, unsigned bz, unsigned gx, unsigned gy) {
    constexpr int TW = MPC_SM_W;
    const int c = threadIdx.x;
    const int C2 = C >> 1;
    const int img = bz / C2, cp = bz - img * C2;
    const int x0 = bx * TW, y0 = by * TH;
    const size_t base = (size_t)img * hq * wq * C2 + cp;        // in float2 units
    const float2 *f2 = reinterpret_cast<const float2 *>(field);
    float2 *g2 = reinterpret_cast<float2 *>(gfield);
    const float eps2 = 1e-3f * 1e-3f;   // charbonnier epsilon ** 2 (loss.py:46,55)
    const int x = x0 - 2 + c;
    const bool xin = x >= 0 && x < wq;
    const bool own_col = c >= 2 && c < 2 + TW && x < wq;
    float2 f1 = make_float2(0.f, 0.f), f2r = f1, hd1 = f1, hd2 = f1;          // f and hd at rows y-1, y-2
    float2 hx2 = f1, hx3 = f1, vy2 = f1, vy3 = f1;                              // hx and vy at rows y-2, y-3
    double a0 = 0.0, a1 = 0.0;
    // rows requested MPC_SM_PF iterations ahead of their use (rolling window in registers: the loop is fully unrolled)
    constexpr int PF = MPC_SM_PF;
    float2 f_next[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        const int y = y0 - 2 + k;
        f_next[k] = (k < TH + 4 && xin && y >= 0 && y < hq) ? f2[base + ((size_t)y * wq + x) * C2] : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int it = 0; it < TH + 4; ++it) {
        const int y = y0 - 2 + it;
        const float2 f0 = f_next[it % PF];
        {
            const int yn = y + PF;
            f_next[it % PF] = (it + PF < TH + 4 && xin && yn >= 0 && yn < hq) ? f2[base + ((size_t)yn * wq + x) * C2] : make_float2(0.f, 0.f);
        }
        const float2 hd0 = make_float2(lane_right(f0.x) - lane_left(f0.x), lane_right(f0.y) - lane_left(f0.y));
        // row y - 1: Sobel -> charbonnier terms and their derivatives
        const int ys = y - 1;
        float2 vx = make_float2(0.f, 0.f), vy1 = make_float2(0.f, 0.f);
        {
            const float2 vd = make_float2(f0.x - f2r.x, f0.y - f2r.y);
            const float dxx = hd2.x + 2.f * hd1.x + hd0.x, dxy = hd2.y + 2.f * hd1.y + hd0.y;
            const float dyx = lane_left(vd.x) + 2.f * vd.x + lane_right(vd.x), dyy = lane_left(vd.y) + 2.f * vd.y + lane_right(vd.y);
            if (xin && ys >= 0 && ys < hq) {
                // hardware sqrt and reciprocal (1 ulp each)
                const float sxx = __builtin_amdgcn_sqrtf(dxx * dxx + eps2), syx = __builtin_amdgcn_sqrtf(dyx * dyx + eps2);
                const float sxy = __builtin_amdgcn_sqrtf(dxy * dxy + eps2), syy = __builtin_amdgcn_sqrtf(dyy * dyy + eps2);
                vx.x = dxx * __builtin_amdgcn_rcpf(sxx); vy1.x = dyx * __builtin_amdgcn_rcpf(syx);
                vx.y = dxy * __builtin_amdgcn_rcpf(sxy); vy1.y = dyy * __builtin_amdgcn_rcpf(syy);
                if (own_col && ys >= y0 && ys < y0 + TH) {
                    a0 += (double)sxx; a1 += (double)syx;
                    a0 += (double)sxy; a1 += (double)syy;
                }
            }
        }
        const float2 hx1 = make_float2(lane_left(vx.x) - lane_right(vx.x), lane_left(vx.y) - lane_right(vx.y));
        // row y - 2: adjoint of the Sobel pair
        const int yo = y - 2;
        {
            const float2 vyd = make_float2(vy3.x - vy1.x, vy3.y - vy1.y);
            const float gyx = lane_right(vyd.x) + 2.f * vyd.x + lane_left(vyd.x), gyy = lane_right(vyd.y) + 2.f * vyd.y + lane_left(vyd.y);
            if (gfield != nullptr && own_col && yo >= y0 && yo < y0 + TH && yo < hq) {
                float2 o;
                o.x = gscale * ((hx1.x + 2.f * hx2.x + hx3.x) + gyx);
                o.y = gscale * ((hx1.y + 2.f * hx2.y + hx3.y) + gyy);
                g2[base + ((size_t)yo * wq + x) * C2] = o;
            }
        }
        f2r = f1; f1 = f0; hd2 = hd1; hd1 = hd0;
        hx3 = hx2; hx2 = hx1; vy3 = vy2; vy2 = vy1;
    }
    a0 = wave_sum_d(a0); a1 = wave_sum_d(a1);
    if (c == 0) {
        const size_t bid = ((size_t)bz * gy + by) * gx + bx;
        part[2 * bid] = a0;
        part[2 * bid + 1] = a1;
    }
}

template <int TH>
__global__ __launch_bounds__(64) void k_lut_smooth_march(const float *__restrict__ field, float *__restrict__ gfield,
                                                         double *__restrict__ part, int hq, int wq, int C, float gscale) {
    lut_smooth_march_body<TH>(field, gfield, part, hq, wq, C, gscale, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y);
}

// ------------------------------------------------------------------------------------------
// contrast + smoothness in ONE launch (mpc_focus_fwd): the two marching kernels above are independent of each other (the
// smoothness reads the finished LUT, the contrast the raw IWE), both are 64-thread workgroups without LDS or barrier, and each
// alone leaves wave slots empty and runs short of its issue and bandwidth limits.  A 1-D grid of n_c + n_s workgroups; a
// wave-uniform branch on the linear block id picks the body and the id is decomposed into the (x, y, z) the body had in its own
// launch -- same arithmetic, same partial-sum slots, so k_finalize adds the same numbers in the same order.
// Order of the two kinds of workgroup in the grid: MPC_CS_ORDER (tuning.h has the measurements).
//   0: the contrast workgroups first, 1: the smoothness workgroups first,
//   2: interleaved in proportion to their counts -- `ng` groups of `ra` contrast and `rb` smoothness workgroups, the rest (of
//      the larger kind, if the counts are not a multiple of each other) behind them, contrast first.
// ------------------------------------------------------------------------------------------
struct mpc_cs_grid {
    unsigned cgx, cgy, cgz, sgx, sgy;     // the grids the two kernels have in launches of their own (smoothness z: what is left)
    unsigned n_c, n_s;                    // workgroups of each kind
    unsigned ra, rb, ng;                  // interleaved order: group shape and count
};

template <bool L2N, int CTH, int STH>
__global__ __launch_bounds__(64) void k_contrast_smooth_march(const float *__restrict__ raw, float *__restrict__ blur,
                                                              float *__restrict__ gimg, double *__restrict__ cpart, int H, int W,
                                                              int nslots, const float *__restrict__ field, float *__restrict__ gfield,
                                                              double *__restrict__ spart, int hq, int wq, int C, float gscale,
                                                              const mpc_cs_grid g) {
    const unsigned b = blockIdx.x;
    bool smooth;
    unsigned i;
#if MPC_CS_ORDER == 0
    smooth = b >= g.n_c;
    i = smooth ? b - g.n_c : b;
#elif MPC_CS_ORDER == 1
    smooth = b < g.n_s;
    i = smooth ? b : b - g.n_s;
#else
    const unsigned per = g.ra + g.rb, head = g.ng * per;
    if (b < head) {
        const unsigned grp = b / per, k = b - grp * per;
        smooth = k >= g.ra;
        i = smooth ? grp * g.rb + (k - g.ra) : grp * g.ra + k;
    } else {
        const unsigned t = b - head, rem_c = g.n_c - g.ng * g.ra;
        smooth = t >= rem_c;
        i = smooth ? g.ng * g.rb + (t - rem_c) : g.ng * g.ra + t;
    }
#endif
    if (!smooth) {
        const unsigned zy = i / g.cgx, bx = i - zy * g.cgx;
        const unsigned bz = zy / g.cgy, by = zy - bz * g.cgy;
        contrast_march_body<L2N, CTH>(raw, blur, gimg, cpart, H, W, nslots, bx, by, bz, g.cgx, g.cgy, g.cgz);
    } else {
        const unsigned zy = i / g.sgx, bx = i - zy * g.sgx;
        const unsigned bz = zy / g.sgy, by = zy - bz * g.sgy;
        lut_smooth_march_body<STH>(field, gfield, spart, hq, wq, C, gscale, bx, by, bz, g.sgx, g.sgy);
    }
}

extern "C" int mpc_contrast_fwd(const mpc_shape *s, const float *iwe_raw, float *iwe_blur,
                                float *grad_iwe, void *ws, void *stream) {
    MPC_CHECK_ARG(s && iwe_raw && iwe_blur && ws, MPC_E_NULL, "null argument");
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    const mpc_ws_layout L = mpc_layout(s);
    hipStream_t st = (hipStream_t)stream;
    double *cpart = (double *)((char *)ws + L.off_cpart);
    const dim3 grid(mpc_cdiv(s->W, MPC_CT_W), mpc_cdiv(s->H, MPC_CT_H), L.nimg);
    const int variance = (s->flags & MPC_F_OBJ_VARIANCE) ? 1 : 0;
    const int l2 = (s->flags & MPC_F_NORM_L2) ? 1 : 0;
    if (grad_iwe && !variance) {
        const dim3 gridf(mpc_cdiv(s->W, MPC_CF_TW), mpc_cdiv(s->H, MPC_CT_H), L.nimg);
        if ((int64_t)gridf.x * gridf.y * gridf.z < 1536) {
            // few images: bands of 16 rows, twice the wavefronts (the partial-sum array is sized for them)
            const dim3 gridh(gridf.x, mpc_cdiv(s->H, MPC_CT_H / 2), L.nimg);
            if (l2) MPC_LAUNCH((k_contrast_march<true, MPC_CT_H / 2>), gridh, dim3(64), 0, st, iwe_raw, iwe_blur, grad_iwe, cpart, s->H, s->W, L.n_cblocks);
            else MPC_LAUNCH((k_contrast_march<false, MPC_CT_H / 2>), gridh, dim3(64), 0, st, iwe_raw, iwe_blur, grad_iwe, cpart, s->H, s->W, L.n_cblocks);
        } else if (l2) MPC_LAUNCH((k_contrast_march<true, MPC_CT_H>), gridf, dim3(64), 0, st, iwe_raw, iwe_blur, grad_iwe, cpart, s->H, s->W, L.n_cblocks);
        else MPC_LAUNCH((k_contrast_march<false, MPC_CT_H>), gridf, dim3(64), 0, st, iwe_raw, iwe_blur, grad_iwe, cpart, s->H, s->W, L.n_cblocks);
        MPC_CHECK_LAUNCH();
        return 0;
    }
    {   // the unfused tiling has fewer workgroups than the partial-sum array: clear the rest
        const int e = mpc_zero_async(cpart, (size_t)L.n_cblocks * 2 * sizeof(double), st);
        if (e) return e;
    }
    MPC_LAUNCH(k_contrast_fwd, grid, dim3(256), 0, st, iwe_raw, iwe_blur, cpart, s->H, s->W, l2, variance);
    MPC_CHECK_LAUNCH();
    if (grad_iwe) {      // variance objective: the adjoint needs the image means first
        {
            float *means = (float *)((char *)ws + L.off_counts) + 8;   // nimg floats after the counters
            MPC_LAUNCH(k_image_means, dim3(L.nimg), dim3(256), 0, st, cpart, means,
                               (int)(grid.x * grid.y), s->H * s->W);
            MPC_LAUNCH(k_contrast_bwd_var, grid, dim3(256), 0, st, iwe_blur, means, grad_iwe, s->H, s->W);
        }
        MPC_CHECK_LAUNCH();
    }
    return 0;
}

// rows per band of the marching smoothness kernel -- mpc_lut_smooth and mpc_finalize (which adds the partial sums of
// the bands) must agree on it: bands of 8 rows when 16 would leave the chip short of wavefronts (B = 1: 360 bands)
static int smooth_band_rows(const mpc_shape *s, int nimg, int C) {
    const int64_t bands = (int64_t)mpc_cdiv(s->wq, MPC_SM_W) * mpc_cdiv(s->hq, MPC_SM_H) * nimg * (C / 2);
    return bands < 1536 ? MPC_SM_H / 2 : MPC_SM_H;
}

extern "C" int mpc_lut_smooth(const mpc_shape *s, const float *field, int32_t nimg, int32_t C,
                              float smooth_weight, float *grad_field, void *ws, void *stream) {
    MPC_CHECK_ARG(s && field && ws, MPC_E_NULL, "null argument");
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    const mpc_ws_layout L = mpc_layout(s);
    MPC_CHECK_ARG(nimg > 0 && C > 0 && (C % 2) == 0, MPC_E_SHAPE, "field must have an even number of channels");
    const int band = smooth_band_rows(s, nimg, C);
    const dim3 grid(mpc_cdiv(s->wq, MPC_SM_W), mpc_cdiv(s->hq, band), nimg * (C / 2));
    const int64_t nblk = (int64_t)grid.x * grid.y * grid.z;
    MPC_CHECK_ARG(nblk <= L.n_sblocks_max, MPC_E_SHAPE, "field larger than the LUT of this shape");
    hipStream_t st = (hipStream_t)stream;
    double *spart = (double *)((char *)ws + L.off_spart);
    const double count = (double)nimg * C * s->hq * s->wq;
    const float gscale = (float)((double)smooth_weight / (2.0 * count));
    if (band == MPC_SM_H) MPC_LAUNCH(k_lut_smooth_march<MPC_SM_H>, grid, dim3(64), 0, st, field, grad_field, spart, s->hq, s->wq, C, gscale);
    else MPC_LAUNCH(k_lut_smooth_march<MPC_SM_H / 2>, grid, dim3(64), 0, st, field, grad_field, spart, s->hq, s->wq, C, gscale);
    MPC_CHECK_LAUNCH();
    return 0;
}

// mpc_focus_fwd: mpc_lut_smooth and the marching form of mpc_contrast_fwd as one launch (k_contrast_smooth_march).  The caller has
// checked that mpc_contrast_fwd would take the marching kernel (grad_iwe given, not the variance objective); band heights,
// grids and partial-sum slots are the ones the two entry points choose, so mpc_finalize reads what it reads after them.  Taken at every
// size: the one launch measured faster than the two at C3, C2 and C4 (tuning.h: MPC_CS_ORDER).
int mpc_contrast_smooth_fwd(const mpc_shape *s, const float *iwe_raw, float *iwe_blur, float *grad_iwe, const float *field,
                            int32_t nimg, int32_t C, float smooth_weight, float *grad_field, void *ws, void *stream) {
    MPC_CHECK_ARG(s && iwe_raw && iwe_blur && grad_iwe && field && ws, MPC_E_NULL, "null argument");
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    const mpc_ws_layout L = mpc_layout(s);
    MPC_CHECK_ARG(!(s->flags & MPC_F_OBJ_VARIANCE), MPC_E_SHAPE, "the variance objective has no marching kernel");
    MPC_CHECK_ARG(nimg > 0 && C > 0 && (C % 2) == 0, MPC_E_SHAPE, "field must have an even number of channels");
    hipStream_t st = (hipStream_t)stream;
    // contrast grid: as mpc_contrast_fwd
    dim3 cgrid(mpc_cdiv(s->W, MPC_CF_TW), mpc_cdiv(s->H, MPC_CT_H), L.nimg);
    const bool chalf = (int64_t)cgrid.x * cgrid.y * cgrid.z < 1536;
    if (chalf) cgrid.y = mpc_cdiv(s->H, MPC_CT_H / 2);
    // smoothness grid: as mpc_lut_smooth
    const int band = smooth_band_rows(s, nimg, C);
    const dim3 sgrid(mpc_cdiv(s->wq, MPC_SM_W), mpc_cdiv(s->hq, band), nimg * (C / 2));
    const int64_t n_c = (int64_t)cgrid.x * cgrid.y * cgrid.z, n_s = (int64_t)sgrid.x * sgrid.y * sgrid.z;
    MPC_CHECK_ARG(n_s <= L.n_sblocks_max, MPC_E_SHAPE, "field larger than the LUT of this shape");
    MPC_CHECK_ARG(n_c > 0 && n_c <= L.n_cblocks && n_c + n_s < ((int64_t)1 << 31), MPC_E_SHAPE, "grid out of range");
    mpc_cs_grid g;
    g.cgx = cgrid.x; g.cgy = cgrid.y; g.cgz = cgrid.z; g.sgx = sgrid.x; g.sgy = sgrid.y;
    g.n_c = (unsigned)n_c; g.n_s = (unsigned)n_s;
    if (n_c >= n_s) { g.rb = 1; g.ra = (unsigned)(n_c / n_s); }
    else { g.ra = 1; g.rb = (unsigned)(n_s / n_c); }
    g.ng = (unsigned)(n_c / g.ra < n_s / g.rb ? n_c / g.ra : n_s / g.rb);
    double *cpart = (double *)((char *)ws + L.off_cpart), *spart = (double *)((char *)ws + L.off_spart);
    const double count = (double)nimg * C * s->hq * s->wq;
    const float gscale = (float)((double)smooth_weight / (2.0 * count));
    const dim3 grid((unsigned)(n_c + n_s));
    const bool l2 = (s->flags & MPC_F_NORM_L2) != 0, shalf = band != MPC_SM_H;
#define MPC_CS_GO(L2N, CTH, STH)                                                                                                   \
    MPC_LAUNCH((k_contrast_smooth_march<L2N, CTH, STH>), grid, dim3(64), 0, st, iwe_raw, iwe_blur, grad_iwe, cpart, s->H, s->W,  \
               L.n_cblocks, field, grad_field, spart, s->hq, s->wq, C, gscale, g)
#define MPC_CS_GO_S(L2N, CTH)                                                                                                     \
    do { if (shalf) MPC_CS_GO(L2N, CTH, MPC_SM_H / 2); else MPC_CS_GO(L2N, CTH, MPC_SM_H); } while (0)
    if (l2) { if (chalf) MPC_CS_GO_S(true, MPC_CT_H / 2); else MPC_CS_GO_S(true, MPC_CT_H); }
    else { if (chalf) MPC_CS_GO_S(false, MPC_CT_H / 2); else MPC_CS_GO_S(false, MPC_CT_H); }
#undef MPC_CS_GO_S
#undef MPC_CS_GO
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_finalize(const mpc_shape *s, int32_t smooth_nimg, int32_t smooth_C,
                            float smooth_weight, float *scal, void *ws, void *stream) {
    return mpc_finalize_ex(s, smooth_nimg, smooth_C, smooth_weight, scal, nullptr, ws, stream);
}

// scal_out: loss, focus, smooth once more (mpc_focus_fwd: the copy the caller hands out), or null
int mpc_finalize_ex(const mpc_shape *s, int32_t smooth_nimg, int32_t smooth_C, float smooth_weight, float *scal, float *scal_out,
                    void *ws, void *stream) {
    MPC_CHECK_ARG(s && scal && ws, MPC_E_NULL, "null argument");
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    const mpc_ws_layout L = mpc_layout(s);
    const int tiles = mpc_cdiv(s->W, MPC_CT_W) * mpc_cdiv(s->H, MPC_CT_H);
    int64_t nsblk = 0;
    double count = 1.0;
    if (smooth_nimg > 0) {
        const int band = smooth_band_rows(s, smooth_nimg, smooth_C);
        nsblk = (int64_t)mpc_cdiv(s->wq, MPC_SM_W) * mpc_cdiv(s->hq, band) * smooth_nimg * (smooth_C / 2);
        MPC_CHECK_ARG(nsblk <= L.n_sblocks_max, MPC_E_SHAPE, "field larger than the LUT of this shape");
        count = (double)smooth_nimg * smooth_C * s->hq * s->wq;
    }
    MPC_LAUNCH(k_finalize, dim3(1), dim3(1024), 0, (hipStream_t)stream,
                       (const double *)((char *)ws + L.off_cpart), L.n_cblocks, tiles, L.nimg,
                       s->H * s->W, (const double *)((char *)ws + L.off_spart), (int)nsblk, count,
                       smooth_weight, (s->flags & MPC_F_OBJ_VARIANCE) ? 1 : 0, scal, scal_out);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_scale(const float *x, const float *a, float *y, int64_t count, void *stream) {
    MPC_CHECK_ARG(x && a && y, MPC_E_NULL, "null argument");
    if (count <= 0) return 0;
    const int grid = (int)((count + 255) / 256 < 2048 ? (count + 255) / 256 : 2048);
    MPC_LAUNCH(k_scale, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, a, y, count);
    MPC_CHECK_LAUNCH();
    return 0;
}


// ---- UNPINNED EXTENSION (default off): IWE pyramid (BASELINE.json configs[2] names one; the reference has none, SURVEY.md
// Appendix C).  Level l + 1 = 2x2 average of level l; the objective of every level is the reference's
// calculate_focus_loss on that level (src/utils/loss.py:4-27), the focus term their sum.  Two helpers: the pooling and its
// adjoint, which carries the coarser level's adjoint image (in units of ITS 1 / val^2 coefficient) into the finer one's.
__global__ __launch_bounds__(256) void k_pool2_fwd(const float *__restrict__ in, float *__restrict__ out, int nimg, int H, int W) {
    const int H2 = H >> 1, W2 = W >> 1;
    const size_t n = (size_t)nimg * H2 * W2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % W2), y = (int)((i / W2) % H2);
        const size_t img = i / ((size_t)W2 * H2);
        const float *p = in + (img * H + 2 * y) * W + 2 * x;
        out[i] = 0.25f * ((p[0] + p[1]) + (p[W] + p[W + 1]));
    }
}
// big[y][x] += (coef_small / coef_big) * 0.25 * small[y / 2][x / 2]     (coefficients: device scalars)
__global__ __launch_bounds__(256) void k_pool2_bwd_add(const float *__restrict__ small, const float *__restrict__ coef_small,
                                                       float *__restrict__ big, const float *__restrict__ coef_big, int nimg, int H, int W) {
    const int H2 = H >> 1, W2 = W >> 1;
    // (a level whose objective is flat -- an empty or constant image -- has coefficient 0 or inf: it passes nothing on, and
    // a finer level without a coefficient of its own receives nothing: no inf / NaN into the gradient)
    const float cs_ = coef_small[0], cb_ = coef_big[0];
    const float ratio = cs_ / cb_;
    const float r = (cb_ != 0.f && ratio == ratio && fabsf(ratio) < INFINITY) ? 0.25f * ratio : 0.f;
    const size_t n = (size_t)nimg * H * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const size_t img = i / ((size_t)W * H);
        if ((y >> 1) < H2 && (x >> 1) < W2) big[i] += r * small[(img * H2 + (y >> 1)) * W2 + (x >> 1)];
    }
}

extern "C" int mpc_pool2_fwd(const float *in, float *out, int32_t nimg, int32_t H, int32_t W, void *stream) {
    MPC_CHECK_ARG(in && out, MPC_E_NULL, "null argument");
    MPC_CHECK_ARG(nimg >= 0 && H >= 2 && W >= 2, MPC_E_SHAPE, "image smaller than a pooling window");
    const int64_t n = (int64_t)nimg * (H / 2) * (W / 2);
    if (n == 0) return 0;
    MPC_LAUNCH(k_pool2_fwd, dim3((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), dim3(256), 0, (hipStream_t)stream, in, out, nimg, H, W);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_pool2_bwd_add(const float *small, const float *coef_small, float *big, const float *coef_big, int32_t nimg,
                                 int32_t H, int32_t W, void *stream) {
    MPC_CHECK_ARG(small && coef_small && big && coef_big, MPC_E_NULL, "null argument");
    MPC_CHECK_ARG(nimg >= 0 && H >= 2 && W >= 2, MPC_E_SHAPE, "image smaller than a pooling window");
    const int64_t n = (int64_t)nimg * H * W;
    if (n == 0) return 0;
    MPC_LAUNCH(k_pool2_bwd_add, dim3((unsigned)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192)), dim3(256), 0, (hipStream_t)stream,
               small, coef_small, big, coef_big, nimg, H, W);
    MPC_CHECK_LAUNCH();
    return 0;
}

MPC_BOUNDS_UNIT("contrast.hip")
