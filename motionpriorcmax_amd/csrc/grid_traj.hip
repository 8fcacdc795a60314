// The network's coefficient grid -> `trajectories` for FocusLoss.calc, and its adjoint back to the grid: row A3 of SURVEY.md 8(a), the
// glue in front of the loss of every training step of the poly / dct / learned bases.
//   reference: src/modules/trajectory_net.py:57-119 (compute_basis, calculate_coords, calculate_trajectories_at_t), 142-161 (step),
//   src/utils/trajectories.py:3-52 (tile mask, coeffs_grid_to_list), src/utils/basis.py:4-46.
// In plain torch this is a boolean-mask gather (a `nonzero`, i.e. a host synchronisation, every step), two basis evaluations, a dozen
// broadcast / sum / stack nodes, and in the backward their adjoints ending in a zero fill + index_put of the dense [B,S,2k,H,W]
// gradient: ~25 launches each way.  Here one kernel forward and one backward (two with a learned basis).
//   tile centres      (y, x) = (iy * tile + tile / 2, ix * tile + tile / 2), iy < hq = ceil((H - tile / 2) / tile), ix < wq likewise:
//                     the count of mask[s::tile, s::tile]; tile i = iy * wq + ix (the order of torch.nonzero)
//   dphi[t][j]        = phi_j(times[t]) - phi_j(anchor), j = 1..k: t^j (polynomial) or sqrt(2) cos(pi/2 (2t + 1) j) (dct), evaluated
//                     per workgroup from the device `times` (drawn on the device every step: nothing cached, nothing read by the host);
//                     or the caller's [n_t][k] matrix (learned: net(times) - net(anchor), differentiated by torch)
//   k_grid_traj_fwd   traj[b][t][i] = (sum_j dphi[t][j] cy[b][i][j], sum_j dphi[t][j] cx[b][i][j]) (+ (y, x)), c = sum over the S scales
//                     of grid[b][s][c][y][x] (channels 0..k-1: y, k..2k-1: x); optionally those rows [B*n][2k]
//   k_grid_traj_bwd   ggrid[b][s][c][y][x] = sum_t g[b][t][i][d] dphi[t][j] at a tile centre, 0 elsewhere -- EVERY element written (the
//                     zero fill IS the kernel); the centre values are computed once per tile and stored to all S scales.  With a learned
//                     basis each centre-row workgroup also writes its partial sums of grad_dphi[t][j] = sum_(b,i) g.y cy[j] + g.x cx[j]
//   k_grid_dphi_sum   grad_dphi = sum of those partials in a fixed order (no float atomics: bitwise reproducible)
// Sums run in index order (over s, j, t), one rounding per multiply and per add (-ffp-contract=off).
#include "common.h"
#include "bounds.h"
#include "dt_device.h"         // the element types of grid / grad_grid (mpc_ld, mpc_store_vec)
#include "partials_device.h"   // the finishing pass of grad_dphi, shared with curve_basis.hip

#define GT_KMAX 16             // basis orders per axis
#define GT_TC 256              // tile columns of a backward workgroup (one thread each)
#define GT_PHI_BYTES (16 * 1024)   // LDS slice of the [n_t][k] basis difference (utils/grid_traj.py: GRID_PHI_FLOATS)

__device__ __forceinline__ float gt_phi(int basis, float t, int j) {
    if (basis == MPC_BASIS_POLY) return powf(t, (float)j);                              // times ** k_idx (basis.py:30-31)
    return 1.41421356237309515f * cosf(1.57079632679489656f * ((2.f * t + 1.f) * (float)j));   // sqrt(2) cos(pi/2 (2t + 1) k) (:20-24)
}

// s_phi[t][j] = dphi[t][j] for the whole workgroup
__device__ __forceinline__ void gt_load_dphi(float *s_phi, const float *times, const float *dphi, int basis, float anchor, int n_t, int k) {
    for (int e = threadIdx.x; e < n_t * k; e += blockDim.x) {
        const int t = e / k, j = e - t * k + 1;
        s_phi[MPC_IDX(e, n_t * k)] = basis == MPC_BASIS_MATRIX ? dphi[e] : gt_phi(basis, times[t], j) - gt_phi(basis, anchor, j);
    }
}

template <int K, typename T>
__global__ __launch_bounds__(256) void k_grid_traj_fwd(const T *__restrict__ grid, const float *__restrict__ times,
                                                       const float *__restrict__ dphi, int basis, float anchor, int add_offsets,
                                                       float *__restrict__ traj, float *__restrict__ rows, int B, int S, int k, int H,
                                                       int W, int tile, int n_t, int hq, int wq) {
    extern __shared__ float s_phi[];            // [n_t][k]
    gt_load_dphi(s_phi, times, dphi, basis, anchor, n_t, k);
    __syncthreads();
    const int n = hq * wq;
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;          // (b, tile)
    if (gi >= (long long)B * n) return;
    const int b = (int)(gi / n), i = (int)(gi - (long long)b * n);
    const int iy = i / wq, ix = i - iy * wq;
    const int y = iy * tile + tile / 2, x = ix * tile + tile / 2;
    MPC_EXPECT(y < H && x < W);
    const size_t plane = (size_t)H * W;
    const T *src = grid + (size_t)b * S * 2 * k * plane + (size_t)y * W + x;
    float cy[K], cx[K];
#pragma unroll
    for (int j = 0; j < K; ++j) cy[j] = cx[j] = 0.f;
    for (int s = 0; s < S; ++s) {               // neighbouring lanes: neighbouring tiles of one row of a channel plane
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < k) { cy[j] += mpc_ld(src + ((size_t)s * 2 * k + j) * plane); cx[j] += mpc_ld(src + ((size_t)s * 2 * k + k + j) * plane); }
    }
    if (rows != nullptr) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < k) { rows[(size_t)gi * 2 * k + j] = cy[j]; rows[(size_t)gi * 2 * k + k + j] = cx[j]; }
    }
    const float py = add_offsets ? (float)y : 0.f, px = add_offsets ? (float)x : 0.f;
    float2 *out = reinterpret_cast<float2 *>(traj) + (size_t)b * n_t * n + i;
    for (int t = 0; t < n_t; ++t) {
        float fy = 0.f, fx = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < k) { const float w = s_phi[MPC_IDX(t * k + j, n_t * k)]; fy = fy + w * cy[j]; fx = fx + w * cx[j]; }
        out[(size_t)t * n] = add_offsets ? make_float2(fy + py, fx + px) : make_float2(fy, fx);
    }
}

// one workgroup per (b, pixel row y, chunk of GT_TC tile columns); `part` (learned basis only): [B*hq*nch][n_t][k]
template <int K, typename T>
__global__ __launch_bounds__(256) void k_grid_traj_bwd(const float *__restrict__ g, const float *__restrict__ times,
                                                       const float *__restrict__ dphi, int basis, float anchor,
                                                       const float *__restrict__ rows, T *__restrict__ ggrid,
                                                       float *__restrict__ part, int B, int S, int k, int H, int W, int tile, int n_t,
                                                       int hq, int wq, int nch, int vec) {
    extern __shared__ float s_phi[];            // [n_t][k]
    __shared__ float s_g[2 * K * GT_TC];        // [2k][GT_TC] the centre values of this row chunk
    __shared__ float s_red[4][K];
    const int ch = (int)(blockIdx.x % nch);
    const long long r = blockIdx.x / nch;
    const int y = (int)(r % H), b = (int)(r / H);
    const int c2 = 2 * k, s0 = tile / 2, iy = y / tile, tx0 = ch * GT_TC;
    const bool centre = y - iy * tile == s0 && iy < hq;                       // (uniform over the workgroup)
    if (centre) {
        gt_load_dphi(s_phi, times, dphi, basis, anchor, n_t, k);
        __syncthreads();
        const int n = hq * wq, ix = tx0 + (int)threadIdx.x;
        const bool act = ix < wq;
        const int i = iy * wq + (act ? ix : 0);
        float gy[K], gx[K], ry[K], rx[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { gy[j] = gx[j] = 0.f; ry[j] = rx[j] = 0.f; }
        if (part != nullptr && act) {
            const float *rw = rows + ((size_t)b * n + i) * c2;
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j < k) { ry[j] = rw[j]; rx[j] = rw[k + j]; }
        }
        const float2 *gp = reinterpret_cast<const float2 *>(g) + (size_t)b * n_t * n + i;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (part == nullptr) {                  // (no barrier in the loop: four gradient loads in flight instead of one)
#pragma unroll 4
            for (int t = 0; t < n_t; ++t) {
                const float2 gt = act ? gp[(size_t)t * n] : make_float2(0.f, 0.f);     // (d/dy, d/dx)
#pragma unroll
                for (int j = 0; j < K; ++j)
                    if (j < k) { const float w = s_phi[MPC_IDX(t * k + j, n_t * k)]; gy[j] = gy[j] + gt.x * w; gx[j] = gx[j] + gt.y * w; }
            }
        }
        for (int t = 0; part != nullptr && t < n_t; ++t) {
            const float2 gt = act ? gp[(size_t)t * n] : make_float2(0.f, 0.f);     // (d/dy, d/dx)
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j < k) { const float w = s_phi[MPC_IDX(t * k + j, n_t * k)]; gy[j] = gy[j] + gt.x * w; gx[j] = gx[j] + gt.y * w; }
            {              // this workgroup's share of grad_dphi[t][:], summed in a fixed order (butterfly, waves 0..3)
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if (j < k) {
                        float v = gt.x * ry[j] + gt.y * rx[j];
                        for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
                        if (lane == 0) s_red[wv][j] = v;
                    }
                }
                __syncthreads();
                if ((int)threadIdx.x < k) {
                    const int j = threadIdx.x;
                    const long long pb = ((long long)b * hq + iy) * nch + ch;
                    part[(pb * n_t + t) * k + j] = ((s_red[0][j] + s_red[1][j]) + s_red[2][j]) + s_red[3][j];
                }
                __syncthreads();
            }
        }
        if (act) {
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j < k) { s_g[MPC_IDX(j * GT_TC + threadIdx.x, 2 * K * GT_TC)] = gy[j]; s_g[MPC_IDX((k + j) * GT_TC + threadIdx.x, 2 * K * GT_TC)] = gx[j]; }
        }
        __syncthreads();
    }
    // the row chunk [x0, x0 + xw) of all S * 2k planes: zeros, and the centre values at the centres
    const int x0 = tx0 * tile;
    const int xw = min(W - x0, GT_TC * tile);
    const size_t plane = (size_t)H * W;
    T *row = ggrid + ((size_t)b * S * c2 * H + y) * W + x0;                   // + (s * c2 + c) * plane
    constexpr int V = MPC_VEC(T);               // elements of a 16-byte store: 4 fp32, 8 fp16 / bf16
    if (vec) {                                  // W % V == 0 and a 16-byte aligned tensor: 16-byte stores (x0 is a multiple of 8)
        const int nxv = xw / V;
        for (int it = threadIdx.x; it < c2 * nxv; it += 256) {
            const int c = it / nxv, q = it - c * nxv;
            float v[V];
#pragma unroll
            for (int u = 0; u < V; ++u) v[u] = 0.f;
            if (centre) {
#pragma unroll
                for (int u = 0; u < V; ++u) {
                    const int x = x0 + V * q + u, ix = x / tile;
                    if (x - ix * tile == s0 && ix < wq) v[u] = s_g[MPC_IDX(c * GT_TC + ix - tx0, 2 * K * GT_TC)];
                }
            }
            for (int s = 0; s < S; ++s) mpc_store_vec(row + (size_t)(s * c2 + c) * plane + V * q, v);
        }
    } else {
        for (int it = threadIdx.x; it < c2 * xw; it += 256) {
            const int c = it / xw, xx = it - c * xw;
            const int x = x0 + xx, ix = x / tile;
            float v = 0.f;
            if (centre && x - ix * tile == s0 && ix < wq) v = s_g[MPC_IDX(c * GT_TC + ix - tx0, 2 * K * GT_TC)];
            for (int s = 0; s < S; ++s) mpc_st(row + (size_t)(s * c2 + c) * plane + xx, v);
        }
    }
}

// grad_dphi[e] = sum over the P workgroup partials part[p][e], e = (t, j): one workgroup per element, a fixed order (partials_device.h)
__global__ __launch_bounds__(256) void k_grid_dphi_sum(const float *__restrict__ part, float *__restrict__ grad_dphi, long long P, int ne) {
    __shared__ float s[256];
    const float v = mpc_partials_sum(part, P, ne, (int)blockIdx.x, s);
    if (threadIdx.x == 0) grad_dphi[blockIdx.x] = v;
}

static void gt_tiles(int H, int W, int tile, int *hq, int *wq) {
    const int s = tile / 2;
    *hq = H > s ? (H - s + tile - 1) / tile : 0;
    *wq = W > s ? (W - s + tile - 1) / tile : 0;
}

static int gt_check(int basis, const float *times, const float *dphi, int B, int S, int k, int H, int W, int tile, int n_t, const char *who) {
    if (basis != MPC_BASIS_POLY && basis != MPC_BASIS_DCT && basis != MPC_BASIS_MATRIX) { mpc_set_error("%s: unknown basis %d", who, basis); return MPC_E_UNSUPPORTED; }
    if (basis == MPC_BASIS_MATRIX ? dphi == nullptr : times == nullptr) { mpc_set_error("%s: null argument (times, or dphi for MPC_BASIS_MATRIX)", who); return MPC_E_NULL; }
    if (B < 0 || S < 1 || k < 1 || H < 1 || W < 1 || tile < 1 || n_t < 1) { mpc_set_error("%s: bad B / S / k / H / W / tile / n_t", who); return MPC_E_SHAPE; }
    if (k > GT_KMAX || (size_t)n_t * k * sizeof(float) > GT_PHI_BYTES) {
        mpc_set_error("%s: more than %d basis orders per axis (or an n_t x k basis beyond %d bytes)", who, GT_KMAX, GT_PHI_BYTES);
        return MPC_E_UNSUPPORTED;
    }
    if ((long long)B * H > (1ll << 24)) { mpc_set_error("%s: B * H too large", who); return MPC_E_UNSUPPORTED; }
    return 0;
}

extern "C" int64_t mpc_grid_traj_scratch_floats(int32_t B, int32_t k, int32_t H, int32_t W, int32_t tile, int32_t n_t) {
    if (B < 0 || k < 1 || H < 1 || W < 1 || tile < 1 || n_t < 1) { mpc_set_error("%s: bad shape", __func__); return MPC_E_SHAPE; }
    int hq, wq;
    gt_tiles(H, W, tile, &hq, &wq);
    const long long nch = ((long long)W + (long long)GT_TC * tile - 1) / ((long long)GT_TC * tile);
    return (int64_t)B * hq * nch * n_t * k;
}

// the ONE copy of the host code of the two entry points; T: the element type of grid / grad_grid (dt_device.h)
template <typename T>
static int gt_fwd(const char *who, const void *grid_, const float *times, const float *dphi, int32_t basis, float anchor_time, int32_t add_offsets,
                  float *traj, float *rows, int32_t B, int32_t S, int32_t k, int32_t H, int32_t W, int32_t tile, int32_t n_t, void *stream) {
    const T *grid = (const T *)grid_;
    int rc = gt_check(basis, times, dphi, B, S, k, H, W, tile, n_t, who);
    if (rc) return rc;
    int hq, wq;
    gt_tiles(H, W, tile, &hq, &wq);
    const long long total = (long long)B * hq * wq;
    if (total == 0) return 0;                   // (empty tensors may come as NULL)
    MPC_CHECK_ARG_WHO(who, grid && traj, MPC_E_NULL, "null argument");
    const dim3 grd((unsigned)((total + 255) / 256));
    const size_t lds = (size_t)n_t * k * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
#define GT_FWD(KK) MPC_LAUNCH((k_grid_traj_fwd<KK, T>), grd, dim3(256), lds, st, grid, times, dphi, basis, anchor_time, add_offsets, traj, rows, B, S, k, H, W, tile, n_t, hq, wq)
    if (k <= 4) GT_FWD(4);
    else if (k <= 8) GT_FWD(8);
    else GT_FWD(GT_KMAX);
#undef GT_FWD
    MPC_CHECK_LAUNCH_WHO(who);
    return 0;
}

template <typename T>
static int gt_bwd(const char *who, const float *grad_traj, const float *times, const float *dphi, int32_t basis, float anchor_time, const float *rows,
                  void *grad_grid_, float *grad_dphi, float *scratch, int32_t B, int32_t S, int32_t k, int32_t H, int32_t W, int32_t tile,
                  int32_t n_t, void *stream) {
    T *grad_grid = (T *)grad_grid_;
    int rc = gt_check(basis, times, dphi, B, S, k, H, W, tile, n_t, who);
    if (rc) return rc;
    if (grad_dphi != nullptr) MPC_CHECK_ARG_WHO(who, basis == MPC_BASIS_MATRIX, MPC_E_UNSUPPORTED, "grad_dphi is only defined for MPC_BASIS_MATRIX");
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {                               // no gradient element; grad_dphi is still an output: zeros (a sum over no partials)
        if (grad_dphi != nullptr) {
            MPC_LAUNCH(k_grid_dphi_sum, dim3((unsigned)(n_t * k)), dim3(256), 0, st, scratch, grad_dphi, 0ll, n_t * k);
            MPC_CHECK_LAUNCH_WHO(who);
        }
        return 0;
    }
    int hq, wq;
    gt_tiles(H, W, tile, &hq, &wq);
    const bool tiles = (long long)hq * wq > 0;  // (without tiles grad_traj and rows are empty: they may come as NULL, and are not read)
    MPC_CHECK_ARG_WHO(who, grad_grid && (grad_traj || !tiles), MPC_E_NULL, "null argument");
    if (grad_dphi != nullptr) MPC_CHECK_ARG_WHO(who, scratch && (rows || !tiles), MPC_E_NULL, "grad_dphi needs rows and scratch");
    const int nch = (int)(((long long)W + (long long)GT_TC * tile - 1) / ((long long)GT_TC * tile));
    const long long blocks = (long long)B * H * nch;
    if (blocks > 0x7fffffffll) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    // (every row start and every chunk start x0 = ch * GT_TC * tile is then a multiple of MPC_VEC elements from the 16-byte aligned base)
    const int vec = W % MPC_VEC(T) == 0 && ((uintptr_t)grad_grid & 15) == 0;
    const size_t lds = (size_t)n_t * k * sizeof(float);
    float *part = grad_dphi != nullptr ? scratch : nullptr;
#define GT_BWD(KK) MPC_LAUNCH((k_grid_traj_bwd<KK, T>), dim3((unsigned)blocks), dim3(256), lds, st, grad_traj, times, dphi, basis, anchor_time, rows, grad_grid, part, B, S, k, H, W, tile, n_t, hq, wq, nch, vec)
    if (k <= 4) GT_BWD(4);
    else if (k <= 8) GT_BWD(8);
    else GT_BWD(GT_KMAX);
#undef GT_BWD
    MPC_CHECK_LAUNCH_WHO(who);
    if (grad_dphi != nullptr) {
        const long long P = (long long)B * hq * nch;
        MPC_LAUNCH(k_grid_dphi_sum, dim3((unsigned)(n_t * k)), dim3(256), 0, st, scratch, grad_dphi, P, n_t * k);
        MPC_CHECK_LAUNCH_WHO(who);
    }
    return 0;
}

extern "C" int mpc_grid_traj_fwd_dt(const void *grid, int32_t dtype, const float *times, const float *dphi, int32_t basis, float anchor_time,
                                    int32_t add_offsets, float *traj, float *rows, int32_t B, int32_t S, int32_t k, int32_t H, int32_t W,
                                    int32_t tile, int32_t n_t, void *stream) {
    MPC_DT_RETURN(dtype, gt_fwd, grid, times, dphi, basis, anchor_time, add_offsets, traj, rows, B, S, k, H, W, tile, n_t, stream);
}

extern "C" int mpc_grid_traj_bwd_dt(const float *grad_traj, const float *times, const float *dphi, int32_t basis, float anchor_time,
                                    const float *rows, void *grad_grid, int32_t dtype, float *grad_dphi, float *scratch, int32_t B, int32_t S,
                                    int32_t k, int32_t H, int32_t W, int32_t tile, int32_t n_t, void *stream) {
    MPC_DT_RETURN(dtype, gt_bwd, grad_traj, times, dphi, basis, anchor_time, rows, grad_grid, grad_dphi, scratch, B, S, k, H, W, tile, n_t, stream);
}

extern "C" int mpc_grid_traj_fwd(const float *grid, const float *times, const float *dphi, int32_t basis, float anchor_time,
                                 int32_t add_offsets, float *traj, float *rows, int32_t B, int32_t S, int32_t k, int32_t H, int32_t W,
                                 int32_t tile, int32_t n_t, void *stream) {
    return mpc_grid_traj_fwd_dt(grid, MPC_DT_F32, times, dphi, basis, anchor_time, add_offsets, traj, rows, B, S, k, H, W, tile, n_t, stream);
}

extern "C" int mpc_grid_traj_bwd(const float *grad_traj, const float *times, const float *dphi, int32_t basis, float anchor_time,
                                 const float *rows, float *grad_grid, float *grad_dphi, float *scratch, int32_t B, int32_t S, int32_t k,
                                 int32_t H, int32_t W, int32_t tile, int32_t n_t, void *stream) {
    return mpc_grid_traj_bwd_dt(grad_traj, times, dphi, basis, anchor_time, rows, grad_grid, MPC_DT_F32, grad_dphi, scratch, B, S, k, H, W, tile, n_t, stream);
}

MPC_BOUNDS_UNIT("grid_traj.hip")
