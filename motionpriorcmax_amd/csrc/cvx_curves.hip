// RAFT-spline output head -> `trajectories` / dense flows: the convex upsampling of the 1/8-grid control points fused with the
// curve product of curves.hip (BASELINE.json configs[3], EVIMO2 / MultiFlow).
//   reference: src/models/raft_spline/curves/base.py:35-38 (create_upsampled), src/models/raft_spline/utils.py:30-45 (cvx_upsample),
//   base.py:95-123 + bezier.py:92-113 (get_flow_from_reference), src/modules/raft_spline.py:122-154 (what validation evaluates).
// For the full-resolution pixel (y, x), cy = y / 8, sy = y % 8, cx = x / 8, sx = x % 8:
//   w_k   = softmax over k = 0..8 of mask[b][k * 64 + sy * 8 + sx][cy][cx]
//   up[c] = sum_k w_k * (8 * P0[b][c][cy + k / 3 - 1][cx + k % 3 - 1])          P0: params zero-padded by one cell (F.unfold's order)
//   flow_t = scale * sum_j basis[t][j] * up[j]                                    dim 1 of params is (x, y), trajectories are (y, x)
// In plain torch this is a softmax, an unfold, a broadcast product [B, 2d, 9, 8, 8, h, w] (1.3 GB at 480 x 640, B = 6, d = 10), a sum,
// a permute and a reshape, of which the loss reads the tile centres only.  Here the forward is one kernel with one thread per
// (sample, tile centre) -- it reads the 9 * (8 / tile)^2 mask channels the centres touch and nothing else --, the dense forward one
// thread per pixel, and the backward two launches in gather form without float atomics (bitwise reproducible):
//   k_cvx_bwd_centres   workgroups [0, nA): per tile centre dflow[2d] = scale * sum_t basis[t][j] * grad_traj[t] (t in index order),
//                       the softmax weights again, both to the workspace, and grad_mask at the centre's nine channels
//                       w_k * (g_k - sum_j w_j g_j), g_k = sum_c (8 * P0[c][nbr_k]) * dflow[c];
//                       workgroups [nA, ..): every OTHER element of the dense grad_mask = 0 (the two roles write disjoint elements
//                       that together are the whole tensor: no memset, no ordering between them)
//   k_cvx_bwd_params    per (sample, channel, cell): 8 * sum over the centres in the 3 x 3 neighbour cells of
//                       w_{k(cell seen from the centre)} * dflow[c], neighbours in k order, centres of a cell in row-major order.
// dflow goes through the workspace ((2d + 9) floats per centre): a cell gathers from up to 9 * (8 / tile)^2 centres, and recomputing
// each centre's T-term sum there would read grad_traj that many times over.
// Sums run in index order with one rounding per multiply and per add (-ffp-contract=off).
#include "common.h"
#include "cvx_device.h"        // cvx_softmax9, cvx_up (shared with val_metrics.hip)

#define CVX_FILL_ELEMS 1024    // elements of one mask plane a zero-fill workgroup covers (256 threads x 4)

template <int D, typename M>
__global__ __launch_bounds__(256) void k_cvx_traj_fwd(const float *__restrict__ params, const M *__restrict__ mask,
                                                      const float *__restrict__ basis, float scale, float *__restrict__ traj,
                                                      int B, int d, int T, int h, int w, int tile, int ntx, int n) {
    extern __shared__ float s_basis[];          // [T][d]
    for (int i = threadIdx.x; i < T * d; i += 256) s_basis[i] = basis[i];
    __syncthreads();
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (long long)B * n) return;
    const int b = (int)(gi / n), i = (int)(gi - (long long)b * n);
    const int iy = i / ntx, ix = i - iy * ntx;
    const int y = (tile >> 1) + iy * tile, x = (tile >> 1) + ix * tile;
    const size_t plane = (size_t)h * w;
    float ux[D], uy[D];
    cvx_up<D>(params + (size_t)b * 2 * d * plane, mask + (size_t)b * 576 * plane, d, h, w, y, x, ux, uy);
    const float py = (float)y, px = (float)x;
    float2 *out = reinterpret_cast<float2 *>(traj) + (size_t)b * T * n + i;
    for (int t = 0; t < T; ++t) {
        float fy = 0.f, fx = 0.f;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (k < d) { const float bw = s_basis[t * d + k]; fy = fy + bw * uy[k]; fx = fx + bw * ux[k]; }
        }
        out[(size_t)t * n] = make_float2(py + fy * scale, px + fx * scale);
    }
}

// flows [T][B][2][8h][8w], (x, y) order: one thread per pixel, every store coalesced over x
template <int D, typename M>
__global__ __launch_bounds__(256) void k_cvx_flow_fwd(const float *__restrict__ params, const M *__restrict__ mask,
                                                      const float *__restrict__ basis, float scale, float *__restrict__ flows,
                                                      int B, int d, int T, int h, int w) {
    extern __shared__ float s_basis[];
    for (int i = threadIdx.x; i < T * d; i += 256) s_basis[i] = basis[i];
    __syncthreads();
    const int W = 8 * w;
    const size_t HW = (size_t)64 * h * w, plane = (size_t)h * w;
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (long long)B * (long long)HW) return;
    const int b = (int)(gi / (long long)HW);
    const size_t pix = (size_t)(gi - (long long)b * (long long)HW);
    const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
    float ux[D], uy[D];
    cvx_up<D>(params + (size_t)b * 2 * d * plane, mask + (size_t)b * 576 * plane, d, h, w, y, x, ux, uy);
    for (int t = 0; t < T; ++t) {
        float fy = 0.f, fx = 0.f;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (k < d) { const float bw = s_basis[t * d + k]; fy = fy + bw * uy[k]; fx = fx + bw * ux[k]; }
        }
        float *o = flows + ((size_t)t * B + b) * 2 * HW + pix;
        o[0] = fx * scale;
        o[HW] = fy * scale;
    }
}

// is the full-resolution coordinate v a tile centre (tile / 2 + i * tile)?
__device__ __forceinline__ bool cvx_is_centre(int v, int tile) {
    const int s = tile >> 1;
    return v >= s && (v - s) % tile == 0;
}

template <int D, typename M>
__global__ __launch_bounds__(256) void k_cvx_bwd_centres(const float *__restrict__ grad_traj, const float *__restrict__ params,
                                                         const M *__restrict__ mask, const float *__restrict__ basis, float scale,
                                                         M *__restrict__ grad_mask, float *__restrict__ ws_dflow,
                                                         float *__restrict__ ws_w, int B, int d, int T, int h, int w, int tile,
                                                         int ntx, int n, int nA, int fill_chunks) {
    extern __shared__ float s_basis[];
    const size_t plane = (size_t)h * w;
    if ((int)blockIdx.x >= nA) {
        // ---- zero fill of every grad_mask element that is no tile centre's
        const int fb = (int)blockIdx.x - nA;
        const int pl = fb / fill_chunks, chunk = fb - pl * fill_chunks;           // pl = b * 576 + channel
        const int ch = pl % 576, sy = (ch >> 3) & 7, sx = ch & 7;
        const bool uni = (8 % tile) == 0;         // then every cell of a plane holds a centre at (sy, sx), or none does
        const bool plane_centre = cvx_is_centre(sy, tile) && cvx_is_centre(sx, tile);
        if (uni && plane_centre) return;
        M *gp = grad_mask + (size_t)pl * plane;
        // a thread covers V elements = one 16-byte store: 4 fp32 (256 threads a chunk) or 8 fp16 / bf16 (the first 128 threads)
        constexpr int V = MPC_VEC(M);
        if ((int)threadIdx.x * V >= CVX_FILL_ELEMS) return;
        const size_t e0 = (size_t)chunk * CVX_FILL_ELEMS + threadIdx.x * V;
        bool z[V], all = e0 + (V - 1) < plane;
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const size_t e = e0 + q;
            z[q] = false;
            if (e < plane) {
                bool c = false;
                if (!uni) { const int cy = (int)(e / w), cx = (int)(e - (size_t)cy * w); c = cvx_is_centre(8 * cy + sy, tile) && cvx_is_centre(8 * cx + sx, tile); }
                z[q] = !c;
            }
            all = all && z[q];
        }
        // (the test is on the ADDRESS: the planes of an odd h * w start at every multiple of 4 bytes, or of 2 with a 16-bit mask)
        if (all && (((uintptr_t)(gp + e0)) & 15) == 0) {
            float zero[V];
#pragma unroll
            for (int q = 0; q < V; ++q) zero[q] = 0.f;
            mpc_store_vec(gp + e0, zero);
        } else {
#pragma unroll
            for (int q = 0; q < V; ++q) if (z[q]) mpc_st(gp + e0 + q, 0.f);
        }
        return;
    }
    // ---- one thread per (sample, tile centre)
    for (int i = threadIdx.x; i < T * d; i += 256) s_basis[i] = basis[i];
    __syncthreads();
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (long long)B * n) return;
    const int b = (int)(gi / n), i = (int)(gi - (long long)b * n);
    const int iy = i / ntx, ix = i - iy * ntx;
    const int y = (tile >> 1) + iy * tile, x = (tile >> 1) + ix * tile;
    float gx[D], gy[D];
#pragma unroll
    for (int k = 0; k < D; ++k) gx[k] = gy[k] = 0.f;
    const float2 *g = reinterpret_cast<const float2 *>(grad_traj) + (size_t)b * T * n + i;
    for (int t = 0; t < T; ++t) {
        const float2 gt = g[(size_t)t * n];                               // (d/dy, d/dx)
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (k < d) { const float bw = s_basis[t * d + k]; gy[k] = gy[k] + bw * gt.x; gx[k] = gx[k] + bw * gt.y; }
        }
    }
#pragma unroll
    for (int k = 0; k < D; ++k) { gx[k] = gx[k] * scale; gy[k] = gy[k] * scale; }
    float wk[9];
    cvx_softmax9(mask + (size_t)b * 576 * plane, h, w, y, x, wk);
    if (ws_dflow) {
        float *wd = ws_dflow + (size_t)b * 2 * d * n + i;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (k < d) { wd[(size_t)k * n] = gx[k]; wd[(size_t)(d + k) * n] = gy[k]; }
        }
        float *ww = ws_w + (size_t)b * 9 * n + i;
#pragma unroll
        for (int k = 0; k < 9; ++k) ww[(size_t)k * n] = wk[k];
    }
    if (!grad_mask) return;
    const int cy = y >> 3, sy = y & 7, cx = x >> 3, sx = x & 7;
    const float *pb = params + (size_t)b * 2 * d * plane;
    float g9[9], dot = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int ny = cy + k / 3 - 1, nx = cx + k % 3 - 1;
        float a = 0.f;
        if (ny >= 0 && ny < h && nx >= 0 && nx < w) {
            const float *pn = pb + (size_t)ny * w + nx;
#pragma unroll
            for (int j = 0; j < D; ++j) if (j < d) a = a + (8.f * pn[(size_t)j * plane]) * gx[j];
#pragma unroll
            for (int j = 0; j < D; ++j) if (j < d) a = a + (8.f * pn[(size_t)(d + j) * plane]) * gy[j];
        }
        g9[k] = a;
        dot = dot + wk[k] * a;
    }
    M *gm = grad_mask + ((size_t)b * 576 + sy * 8 + sx) * plane + (size_t)cy * w + cx;
#pragma unroll
    for (int k = 0; k < 9; ++k) mpc_st(gm + (size_t)k * 64 * plane, wk[k] * (g9[k] - dot));      // (one rounding to the mask's type)
}

// grad_params: one thread per (cell, channel, sample) = (x chunk of 256 cells, blockIdx.y, blockIdx.z)
__global__ __launch_bounds__(256) void k_cvx_bwd_params(const float *__restrict__ ws_dflow, const float *__restrict__ ws_w,
                                                        float *__restrict__ grad_params, int d, int h, int w, int tile, int nty,
                                                        int ntx, int n) {
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= h * w) return;
    const int c = blockIdx.y, b = blockIdx.z, s = tile >> 1;
    const int cy = cell / w, cx = cell - cy * w;
    const float *df = ws_dflow + ((size_t)b * 2 * d + c) * n;
    const float *wb = ws_w + (size_t)b * 9 * n;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int qy = cy - (k / 3 - 1), qx = cx - (k % 3 - 1);          // the cell whose centres see this one as neighbour k
        if (qy < 0 || qy >= h || qx < 0 || qx >= w) continue;
        const int y0 = 8 * qy, x0 = 8 * qx;
        if (y0 + 7 < s || x0 + 7 < s) continue;
        const int iy_lo = y0 > s ? (y0 - s + tile - 1) / tile : 0, iy_hi = min((y0 + 7 - s) / tile, nty - 1);
        const int ix_lo = x0 > s ? (x0 - s + tile - 1) / tile : 0, ix_hi = min((x0 + 7 - s) / tile, ntx - 1);
        const float *wkp = wb + (size_t)k * n;
        for (int iy = iy_lo; iy <= iy_hi; ++iy)
            for (int ix = ix_lo; ix <= ix_hi; ++ix) {
                const int i = iy * ntx + ix;
                acc = acc + wkp[i] * df[i];
            }
    }
    grad_params[((size_t)b * 2 * d + c) * ((size_t)h * w) + cell] = 8.f * acc;
}

static int cvx_tiles(int v8, int tile) { const int s = tile >> 1; return v8 > s ? (v8 - s + tile - 1) / tile : 0; }

static int cvx_check(const char *who, int B, int d, int T, int h, int w, int tile) {
    if (B < 0 || h < 0 || w < 0 || d < 1 || T < 1 || tile < 1) { mpc_set_error("%s: bad B / d / T / h / w / tile", who); return MPC_E_SHAPE; }
    if (d > CVX_DMAX || (size_t)T * d * sizeof(float) > 48 * 1024) { mpc_set_error("%s: more than %d control points per axis (or a basis matrix beyond 48 KB)", who, CVX_DMAX); return MPC_E_UNSUPPORTED; }
    if ((long long)h * w > (1ll << 24) || (long long)B * 576 * h * w > (1ll << 40) || (long long)B * 576 > (1ll << 21)) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    return 0;
}

#define CVX_DISPATCH(kern, M, grid, lds, st, ...)                                                           \
    do {                                                                                                    \
        if (d <= 4) MPC_LAUNCH((kern<4, M>), grid, dim3(256), lds, st, __VA_ARGS__);                        \
        else if (d <= 10) MPC_LAUNCH((kern<10, M>), grid, dim3(256), lds, st, __VA_ARGS__);                 \
        else MPC_LAUNCH((kern<CVX_DMAX, M>), grid, dim3(256), lds, st, __VA_ARGS__);                        \
    } while (0)

// the ONE copy of the host code of the three entry points; M: the element type of mask / grad_mask (dt_device.h)
template <typename M>
static int cvx_traj_fwd_run(const char *who, const float *params, const void *mask, const float *basis, float scale, float *traj,
                            int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, int32_t tile, void *stream) {
    if (!params || !mask || !basis || !traj) { mpc_set_error("%s: null argument", who); return MPC_E_NULL; }
    int rc = cvx_check(who, B, d, T, h, w, tile);
    if (rc) return rc;
    const int nty = cvx_tiles(8 * h, tile), ntx = cvx_tiles(8 * w, tile), n = nty * ntx;
    const long long work = (long long)B * n;
    if (work == 0) return 0;
    if (work > (1ll << 38)) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    const dim3 grid((unsigned)((work + 255) / 256));
    const size_t lds = (size_t)T * d * sizeof(float);
    CVX_DISPATCH(k_cvx_traj_fwd, M, grid, lds, (hipStream_t)stream, params, (const M *)mask, basis, scale, traj, B, d, T, h, w, tile, ntx, n);
    MPC_CHECK_LAUNCH_WHO(who);
    return 0;
}

template <typename M>
static int cvx_flow_fwd_run(const char *who, const float *params, const void *mask, const float *basis, float scale, float *flows,
                            int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, void *stream) {
    if (!params || !mask || !basis || !flows) { mpc_set_error("%s: null argument", who); return MPC_E_NULL; }
    int rc = cvx_check(who, B, d, T, h, w, 1);
    if (rc) return rc;
    const long long work = (long long)B * 64 * h * w;
    if (work == 0) return 0;
    if (work > (1ll << 38)) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    const dim3 grid((unsigned)((work + 255) / 256));
    const size_t lds = (size_t)T * d * sizeof(float);
    CVX_DISPATCH(k_cvx_flow_fwd, M, grid, lds, (hipStream_t)stream, params, (const M *)mask, basis, scale, flows, B, d, T, h, w);
    MPC_CHECK_LAUNCH_WHO(who);
    return 0;
}

extern "C" int64_t mpc_cvx_traj_bwd_workspace_bytes(int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, int32_t tile) {
    int rc = cvx_check(__func__, B, d, T, h, w, tile);
    if (rc) return rc;
    const int64_t n = (int64_t)cvx_tiles(8 * h, tile) * cvx_tiles(8 * w, tile);
    return mpc_align((int64_t)B * n * (2 * d + 9) * (int64_t)sizeof(float));
}

template <typename M>
static int cvx_traj_bwd_run(const char *who, const float *grad_traj, const float *params, const void *mask, const float *basis, float scale,
                            float *grad_params, void *grad_mask, int32_t B, int32_t d, int32_t T, int32_t h, int32_t w,
                            int32_t tile, void *ws, void *stream) {
    if (!grad_traj || !params || !mask || !basis) { mpc_set_error("%s: null argument", who); return MPC_E_NULL; }
    int rc = cvx_check(who, B, d, T, h, w, tile);
    if (rc) return rc;
    if (grad_params && !ws) { mpc_set_error("%s: grad_params needs the workspace", who); return MPC_E_NULL; }
    if (!grad_params && !grad_mask) return 0;
    const long long plane = (long long)h * w;
    if ((long long)B * plane == 0) return 0;
    const int nty = cvx_tiles(8 * h, tile), ntx = cvx_tiles(8 * w, tile), n = nty * ntx;
    const long long work = (long long)B * n;
    if (work > (1ll << 38)) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    const int nA = (int)((work + 255) / 256);
    const int chunks = (int)((plane + CVX_FILL_ELEMS - 1) / CVX_FILL_ELEMS);
    const long long nfill = grad_mask ? (long long)B * 576 * chunks : 0;
    if (nA + nfill > 0x7fffffffll) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    float *ws_dflow = grad_params ? (float *)ws : nullptr;
    float *ws_w = grad_params ? ws_dflow + (size_t)B * 2 * d * n : nullptr;
    const size_t lds = (size_t)T * d * sizeof(float);
    if (nA + nfill > 0) {
        const dim3 grid((unsigned)(nA + nfill));
        CVX_DISPATCH(k_cvx_bwd_centres, M, grid, lds, (hipStream_t)stream, grad_traj, params, (const M *)mask, basis, scale, (M *)grad_mask, ws_dflow, ws_w,
                     B, d, T, h, w, tile, ntx, n, nA, chunks);
        MPC_CHECK_LAUNCH_WHO(who);
    }
    if (grad_params) {
        const dim3 grid((unsigned)((plane + 255) / 256), (unsigned)(2 * d), (unsigned)B);
        MPC_LAUNCH(k_cvx_bwd_params, grid, dim3(256), 0, (hipStream_t)stream, ws_dflow, ws_w, grad_params, d, h, w, tile, nty, ntx, n);
        MPC_CHECK_LAUNCH_WHO(who);
    }
    return 0;
}

extern "C" int mpc_cvx_traj_fwd_dt(const float *params, const void *mask, int32_t dtype, const float *basis, float scale, float *traj,
                                   int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, int32_t tile, void *stream) {
    MPC_DT_RETURN(dtype, cvx_traj_fwd_run, params, mask, basis, scale, traj, B, d, T, h, w, tile, stream);
}

extern "C" int mpc_cvx_flow_fwd_dt(const float *params, const void *mask, int32_t dtype, const float *basis, float scale, float *flows,
                                   int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, void *stream) {
    MPC_DT_RETURN(dtype, cvx_flow_fwd_run, params, mask, basis, scale, flows, B, d, T, h, w, stream);
}

extern "C" int mpc_cvx_traj_bwd_dt(const float *grad_traj, const float *params, const void *mask, int32_t dtype, const float *basis, float scale,
                                   float *grad_params, void *grad_mask, int32_t B, int32_t d, int32_t T, int32_t h, int32_t w,
                                   int32_t tile, void *ws, void *stream) {
    MPC_DT_RETURN(dtype, cvx_traj_bwd_run, grad_traj, params, mask, basis, scale, grad_params, grad_mask, B, d, T, h, w, tile, ws, stream);
}

extern "C" int mpc_cvx_traj_fwd(const float *params, const float *mask, const float *basis, float scale, float *traj,
                                int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, int32_t tile, void *stream) {
    return mpc_cvx_traj_fwd_dt(params, mask, MPC_DT_F32, basis, scale, traj, B, d, T, h, w, tile, stream);
}

extern "C" int mpc_cvx_flow_fwd(const float *params, const float *mask, const float *basis, float scale, float *flows,
                                int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, void *stream) {
    return mpc_cvx_flow_fwd_dt(params, mask, MPC_DT_F32, basis, scale, flows, B, d, T, h, w, stream);
}

extern "C" int mpc_cvx_traj_bwd(const float *grad_traj, const float *params, const float *mask, const float *basis, float scale,
                                float *grad_params, float *grad_mask, int32_t B, int32_t d, int32_t T, int32_t h, int32_t w,
                                int32_t tile, void *ws, void *stream) {
    return mpc_cvx_traj_bwd_dt(grad_traj, params, mask, MPC_DT_F32, basis, scale, grad_params, grad_mask, B, d, T, h, w, tile, ws, stream);
}
