// IWE pyramid as ONE pass behind any forward of the library (UNPINNED extension: BASELINE.json's configs[2] names a multi-scale
// IWE pyramid, the reference has none -- SURVEY.md Appendix C; the definition is that of ops.PyramidFocusFn and is unchanged).
// Every route ends its forward in the raw IWE, the unscaled adjoint image grad_iwe and `scal` with d focus / d raw =
// scal[MPC_SCAL_GCOEF] * grad_iwe.  This pass reads the raw IWE, adds the coarse levels' focus terms to `scal` and folds their
// adjoint images into grad_iwe in units of level 0's coefficient: the backward kernels of every route run unchanged.
//   k_iwe_pyramid_levels : all coarse levels of all images in one launch.  One wavefront marches one band of one level through
//                          contrast_march_body (contrast_march.h); a level-l raw value is formed in registers from the level-0
//                          image by l chained 2x2 averages in the association of k_pool2_fwd, so its bits are those of the
//                          mpc_pool2_fwd chain and no coarse raw image is ever stored.  -> per-level unscaled adjoint images,
//                          per-band partial sums.
//   k_iwe_pyramid_reduce : one workgroup.  Per level the band sums in a fixed order -> val, 1 / val, GCOEF and the fold ratio
//                          r_l; the level table; scal (and scal_out) += the coarse levels' focus terms.
//   k_iwe_pyramid_fold   : (gradient wanted) grad_iwe[y][x] += sum_{l >= 1} r_l * g_l[y >> l][x >> l], one pass over level 0.
// Plain launches on one stream: no memset / memcpy node, no atomics, no host synchronisation, no workgroup waits on another;
// every sum has a fixed order (bitwise reproducible).
#include "common.h"
#include "bounds.h"
#include "contrast_march.h"
#include <string.h>

#define PYR_MAX_LEVELS 6          // levels of the pyramid, level 0 included
#define PYR_TH 16                 // rows per band of a coarse level (the coarse levels are small: thin bands, more wavefronts)

// level LV of the pyramid at (y, x), formed from the level-0 image `p` (row stride W0; 16-byte aligned, W0 a multiple of 2^LV):
// 0.25f * ((a + b) + (c + d)) per step, a b / c d the 2x2 window of the finer level -- k_pool2_fwd's expression, so its bits
template <int LV>
struct pyr_pool {
    // (LV >= 3: 4^LV loads per value -- a loop over the four finer values in a function of its own, or the unrolled marching
    // loop would hold 40 x 4^LV loads; such levels are 1 / 64 of the image and smaller)
    static __device__ __noinline__ float at(const float *__restrict__ p, int W0, int y, int x) {
        float pair = 0.f, first = 0.f, v = 0.f;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const float f = pyr_pool<LV - 1>::at(p, W0, 2 * y + (j >> 1), 2 * x + (j & 1));
            if (j & 1) {
                const float s = first + f;
                if (j == 1) pair = s;
                else v = 0.25f * (pair + s);
            } else first = f;
        }
        return v;
    }
};
template <>
struct pyr_pool<1> {
    static __device__ __forceinline__ float at(const float *__restrict__ p, int W0, int y, int x) {
        const float2 t = *reinterpret_cast<const float2 *>(p + (size_t)(2 * y) * W0 + 2 * x);
        const float2 b = *reinterpret_cast<const float2 *>(p + (size_t)(2 * y + 1) * W0 + 2 * x);
        return 0.25f * ((t.x + t.y) + (b.x + b.y));
    }
};
template <>
struct pyr_pool<2> {
    static __device__ __forceinline__ float at(const float *__restrict__ p, int W0, int y, int x) {
        const float *q = p + (size_t)(4 * y) * W0 + 4 * x;
        const float4 r0 = *reinterpret_cast<const float4 *>(q), r1 = *reinterpret_cast<const float4 *>(q + W0);
        const float4 r2 = *reinterpret_cast<const float4 *>(q + 2 * (size_t)W0), r3 = *reinterpret_cast<const float4 *>(q + 3 * (size_t)W0);
        const float a = 0.25f * ((r0.x + r0.y) + (r1.x + r1.y)), b = 0.25f * ((r0.z + r0.w) + (r1.z + r1.w));
        const float c = 0.25f * ((r2.x + r2.y) + (r3.x + r3.y)), d = 0.25f * ((r2.z + r2.w) + (r3.z + r3.w));
        return 0.25f * ((a + b) + (c + d));
    }
};

// the row source of contrast_march_body for level LV: H, W are the LEVEL's size, the image behind it is (H << LV) x (W << LV)
template <int LV>
struct pyr_rows {
    static constexpr bool kBlur = false;          // coarse blurred images are not an output
    const float *p;
    int W0;
    __device__ __forceinline__ pyr_rows(const float *__restrict__ raw, unsigned bz, int H, int W)
        : p(raw + (size_t)bz * ((size_t)H << LV) * ((size_t)W << LV)), W0(W << LV) {}
    __device__ __forceinline__ float operator()(int y, int x) const { return pyr_pool<LV>::at(p, W0, y, x); }
};

// what the three kernels need to know of the pyramid (by value): level l - 1 of the arrays is pyramid level l
struct pyr_plan {
    int32_t levels, nimg, H0, W0;
    uint32_t gx[PYR_MAX_LEVELS - 1], gy[PYR_MAX_LEVELS - 1];       // bands of a level: gx x gy x nimg
    uint32_t first[PYR_MAX_LEVELS];                                // first workgroup of a level in the 1-D grid; [levels - 1]: the total
    int64_t goff[PYR_MAX_LEVELS - 1];                              // the level's adjoint image [nimg][H_l][W_l]: floats from the workspace's start
    int64_t poff[PYR_MAX_LEVELS - 1];                              // the level's band sums [bands][2]: doubles from the start of the sums
};

template <bool L2N>
__global__ __launch_bounds__(64) void k_iwe_pyramid_levels(const float *__restrict__ raw, float *__restrict__ gbase /* or null */,
                                                           double *__restrict__ pbase, const pyr_plan g) {
    const unsigned b = blockIdx.x;
    int l = 1;
    while (l < g.levels - 1 && b >= g.first[l]) ++l;                 // (uniform: at most four steps)
    const unsigned i = b - g.first[l - 1];
    const unsigned gx = g.gx[l - 1], gy = g.gy[l - 1];
    const unsigned zy = i / gx, bx = i - zy * gx;
    const unsigned bz = zy / gy, by = zy - bz * gy;
    const int H = g.H0 >> l, W = g.W0 >> l;
    float *gimg = gbase ? gbase + g.goff[l - 1] : nullptr;
    double *part = pbase + g.poff[l - 1];
    const int nb = (int)(gx * gy * (unsigned)g.nimg);                // every slot of the level's sums has its band
#define PYR_GO(LV) contrast_march_body<L2N, PYR_TH, pyr_rows<LV>>(raw, nullptr, gimg, part, H, W, nb, bx, by, bz, gx, gy, (unsigned)g.nimg)
    switch (l) {
    case 1: PYR_GO(1); break;
    case 2: PYR_GO(2); break;
    case 3: PYR_GO(3); break;
    case 4: PYR_GO(4); break;
    default: PYR_GO(5); break;
    }
#undef PYR_GO
}

// level_scal [levels][MPC_SCAL_COUNT]: row l = what mpc_finalize writes for level l alone (LOSS = FOCUS = 1 / val_l, SMOOTH 0, VAL,
// GCOEF) and, in [MPC_SCAL_PYR_RATIO], the fold ratio r_l; row 0 = `scal` as the pass found it (r_0 = 1).
// r_l = 4^-l GCOEF_l / GCOEF_0, or 0 where a coefficient of level 0 .. l is 0, inf or NaN (k_pool2_bwd_add's rule: a flat level
// passes nothing on, neither its own adjoint image nor what the coarser levels handed it).
__global__ __launch_bounds__(1024) void k_iwe_pyramid_reduce(const double *__restrict__ pbase, float *__restrict__ scal,
                                                            float *__restrict__ scal_out, float *__restrict__ level_scal, const pyr_plan g) {
    __shared__ double s_red[16];
    const int tid = threadIdx.x;
    float focus = 0.f, c0 = 0.f;
    bool alive = false;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < MPC_SCAL_COUNT; ++k) level_scal[k] = scal[k];
        level_scal[MPC_SCAL_PYR_RATIO] = 1.f;
        focus = scal[MPC_SCAL_FOCUS];
        c0 = scal[MPC_SCAL_GCOEF];
        alive = c0 != 0.f && fabsf(c0) < INFINITY;                  // (NaN compares false)
    }
    double quarter = 1.0;
    for (int l = 1; l < g.levels; ++l) {
        const double *part = pbase + g.poff[l - 1];
        const int nb = (int)(g.gx[l - 1] * g.gy[l - 1] * (unsigned)g.nimg);
        double a = 0.0;
        for (int i = tid; i < nb; i += 1024) a += part[2 * (size_t)i];
        const double tot = block_sum_d<1024>(a, s_red);
        quarter *= 0.25;
        if (tid == 0) {
            const double N = (double)g.nimg * (double)(g.H0 >> l) * (double)(g.W0 >> l);
            const double val = tot / N;
            const float fl = (float)(1.0 / val), cl = (float)(-1.0 / (val * val) / N);
            alive = alive && cl != 0.f && fabsf(cl) < INFINITY;
            const float r = (float)(quarter * (double)cl / (double)c0);
            float *row = level_scal + (size_t)l * MPC_SCAL_COUNT;
            row[MPC_SCAL_LOSS] = fl; row[MPC_SCAL_FOCUS] = fl; row[MPC_SCAL_SMOOTH] = 0.f;
            row[MPC_SCAL_VAL] = (float)val; row[MPC_SCAL_GCOEF] = cl;
            row[MPC_SCAL_PYR_RATIO] = (alive && fabsf(r) < INFINITY) ? r : 0.f;
            row[6] = row[7] = 0.f;
            focus += fl;                                              // fp32, level by level: the sum ops.PyramidFocusFn forms
        }
    }
    if (tid == 0) {
        const float loss = focus + scal[MPC_SCAL_SMOOTH];
        scal[MPC_SCAL_FOCUS] = focus;
        scal[MPC_SCAL_LOSS] = loss;
        if (scal_out != nullptr) { scal_out[MPC_SCAL_LOSS] = loss; scal_out[MPC_SCAL_FOCUS] = focus; }
    }
}

// one thread per pair of level-0 pixels (W0 is even: both lie under the same pixel of every coarse level); a fused multiply-add
// per level, finest first: levels - 1 roundings beside the one of each r_l
__global__ __launch_bounds__(256) void k_iwe_pyramid_fold(float *__restrict__ grad_iwe, const float *__restrict__ gbase,
                                                          const float *__restrict__ level_scal, const pyr_plan g) {
    float r[PYR_MAX_LEVELS - 1];
#pragma unroll
    for (int l = 1; l < PYR_MAX_LEVELS; ++l) r[l - 1] = l < g.levels ? level_scal[(size_t)l * MPC_SCAL_COUNT + MPC_SCAL_PYR_RATIO] : 0.f;
    const int W2 = g.W0 >> 1;
    const size_t n = (size_t)g.nimg * g.H0 * W2;
    float2 *out = reinterpret_cast<float2 *>(grad_iwe);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int x2 = (int)(i % W2), y = (int)((i / W2) % g.H0);
        const size_t img = i / ((size_t)W2 * g.H0);
        float2 v = out[i];
#pragma unroll
        for (int l = 1; l < PYR_MAX_LEVELS; ++l) {
            if (l < g.levels) {
                const int Hl = g.H0 >> l, Wl = g.W0 >> l;
                const size_t j = (img * Hl + (y >> l)) * Wl + (x2 >> (l - 1));
                const float t = r[l - 1] != 0.f ? gbase[g.goff[l - 1] + MPC_IDX(j, (size_t)g.nimg * Hl * Wl)] : 0.f;      // (a flat level: 0, not 0 * inf)
                v.x = __fmaf_rn(r[l - 1], t, v.x);
                v.y = __fmaf_rn(r[l - 1], t, v.y);
            }
        }
        out[i] = v;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// no device is touched here: mpc_iwe_pyramid_supported and the workspace query answer on a machine without one
static int pyr_check(const char *who, const mpc_shape *s, int32_t levels) {
    MPC_CHECK_ARG_WHO(who, s != nullptr, MPC_E_NULL, "null shape");
    const int rc = mpc_validate_shape(s);
    if (rc) return rc;
    MPC_CHECK_ARG_WHO(who, levels >= 2 && levels <= PYR_MAX_LEVELS, MPC_E_UNSUPPORTED, "pyramid levels outside [2, 6]");
    MPC_CHECK_ARG_WHO(who, !(s->flags & MPC_F_OBJ_VARIANCE), MPC_E_UNSUPPORTED, "the IWE pyramid needs the gradient-magnitude objective (not variance)");
    MPC_CHECK_ARG_WHO(who, s->T == 1, MPC_E_UNSUPPORTED, "the IWE pyramid needs num_tref == 1");
    const int m = (1 << (levels - 1)) - 1;
    MPC_CHECK_ARG_WHO(who, !(s->H & m) && !(s->W & m) && (s->H >> (levels - 1)) >= 3 && (s->W >> (levels - 1)) >= 3, MPC_E_SHAPE,
                      "H and W must be divisible by 2^(levels - 1) and the coarsest level at least 3x3");
    return 0;
}

struct pyr_layout {
    pyr_plan g;
    int64_t off_part;       // bytes: the band sums behind the adjoint images
    int64_t total;          // bytes
};

static pyr_layout pyr_lay(const mpc_shape *s, int32_t levels, bool want_grad) {
    pyr_layout L;
    memset(&L, 0, sizeof(L));
    pyr_plan &g = L.g;
    g.levels = levels;
    g.nimg = s->B * s->T * ((s->flags & MPC_F_POLARITY_SPLIT) ? 2 : 1);
    g.H0 = s->H; g.W0 = s->W;
    int64_t gf = 0, pd = 0;
    uint32_t first = 0;
    for (int l = 1; l < levels; ++l) {
        const int H = s->H >> l, W = s->W >> l;
        g.gx[l - 1] = (uint32_t)mpc_cdiv(W, MPC_CF_TW);
        g.gy[l - 1] = (uint32_t)mpc_cdiv(H, PYR_TH);
        g.first[l - 1] = first;
        first += g.gx[l - 1] * g.gy[l - 1] * (uint32_t)g.nimg;
        g.goff[l - 1] = gf;
        if (want_grad) gf += mpc_align((int64_t)g.nimg * H * W, 64);          // 256-byte aligned images
        g.poff[l - 1] = pd;
        pd += 2 * (int64_t)g.gx[l - 1] * g.gy[l - 1] * g.nimg;
    }
    g.first[levels - 1] = first;
    L.off_part = mpc_align(gf * (int64_t)sizeof(float));
    L.total = L.off_part + mpc_align(pd * (int64_t)sizeof(double));
    return L;
}

extern "C" int mpc_iwe_pyramid_supported(const mpc_shape *s, int32_t levels) { return pyr_check("mpc_iwe_pyramid_supported", s, levels); }

extern "C" int64_t mpc_iwe_pyramid_workspace_bytes(const mpc_shape *s, int32_t levels, int32_t want_grad) {
    const int rc = pyr_check("mpc_iwe_pyramid_workspace_bytes", s, levels);
    if (rc) return rc;
    return pyr_lay(s, levels, want_grad != 0).total;
}

extern "C" int mpc_iwe_pyramid_fwd(const mpc_shape *s, int32_t levels, const float *iwe_raw, float *grad_iwe, float *scal, float *scal_out,
                                   float *level_scal, void *pws, void *stream) {
    int rc = pyr_check("mpc_iwe_pyramid_fwd", s, levels);
    if (rc) return rc;
    MPC_CHECK_ARG(iwe_raw && scal && level_scal && pws, MPC_E_NULL, "null argument");
    // (the coarse levels are read from the level-0 image with 8- and 16-byte loads, the fold works on pixel pairs)
    MPC_CHECK_ARG(!(reinterpret_cast<uintptr_t>(iwe_raw) & 15) && !(reinterpret_cast<uintptr_t>(grad_iwe) & 7) && !(reinterpret_cast<uintptr_t>(pws) & 15),
                  MPC_E_SHAPE, "iwe_raw and pws must be 16-byte aligned, grad_iwe 8-byte aligned");
    const pyr_layout L = pyr_lay(s, levels, grad_iwe != nullptr);
    const pyr_plan &g = L.g;
    if (g.nimg <= 0) return 0;
    MPC_CHECK_ARG((int64_t)g.nimg * s->H * s->W < ((int64_t)1 << 40) && g.first[levels - 1] > 0 && g.first[levels - 1] < (1u << 31), MPC_E_UNSUPPORTED, "images too large");
    hipStream_t st = (hipStream_t)stream;
    float *gbase = grad_iwe ? (float *)pws : nullptr;
    double *pbase = (double *)((char *)pws + L.off_part);
    const dim3 grid(g.first[levels - 1]);
    if (s->flags & MPC_F_NORM_L2) MPC_LAUNCH(k_iwe_pyramid_levels<true>, grid, dim3(64), 0, st, iwe_raw, gbase, pbase, g);
    else MPC_LAUNCH(k_iwe_pyramid_levels<false>, grid, dim3(64), 0, st, iwe_raw, gbase, pbase, g);
    MPC_LAUNCH(k_iwe_pyramid_reduce, dim3(1), dim3(1024), 0, st, (const double *)pbase, scal, scal_out, level_scal, g);
    if (grad_iwe) {
        const int64_t n = (int64_t)g.nimg * s->H * (s->W >> 1);
        const int64_t blocks = (n + 255) / 256;
        MPC_LAUNCH(k_iwe_pyramid_fold, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, grad_iwe, (const float *)gbase, (const float *)level_scal, g);
    }
    MPC_CHECK_LAUNCH();
    return 0;
}

MPC_BOUNDS_UNIT("iwe_pyramid.hip")
