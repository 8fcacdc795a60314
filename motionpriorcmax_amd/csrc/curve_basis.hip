// The gradient of the [T][d] basis matrix of the RAFT-spline nodes -- the plain head (curves.hip), the convex-upsampling head
// (cvx_curves.hip) and the correlation lookup (corr_lookup.hip) -- for the reference's curve_type LEARNED while its basis network
// trains (src/models/raft_spline/curves/learned.py:76-77: the matrix is the network's output).  The curve is linear in the matrix,
// so the three nodes share one form: with R[b][i][c][j] the control points that site i of sample b evaluates (c: x, y) and
// G[t][b][i][c] the cotangent of the displacement there,
//   grad_basis[t][j] = scale * sum over (b, i) of (G[t][b][i].x * R[b][i].x[j] + G[t][b][i].y * R[b][i].y[j])
// A reduction of its own behind the nodes' unchanged backward kernels, in the scheme of grid_traj.hip's grad_dphi:
//   k_curve_basis_part  workgroup p takes the 256 consecutive (sample, site) pairs [256 p, 256 p + 256), one per thread, the 2 d
//                       control values in registers; per t a butterfly over the wavefront, then the four waves in order:
//                       part[p][t][j].  Which pairs a workgroup sums is fixed by its index alone.
//   k_curve_basis_sum   grad_basis[t][j] = scale * (the partials summed in a fixed order: partials_device.h, the body of
//                       k_grid_dphi_sum)
// No float atomics, no host synchronisation, nothing allocated: bitwise reproducible and independent of the launch's scheduling.
// One rounding per multiply and per add (-ffp-contract=off).  Both operands are read once; neighbouring lanes read neighbouring
// sites: 4-byte (the planes of params and grad_coords) or 8-byte neighbours (grad_traj), or the consecutive rows of mpc_pec_head_rows
// (a wavefront reads 64 * 2 d consecutive floats over its j loop).
#include "common.h"
#include "bounds.h"
#include "partials_device.h"

#define CBG_DMAX 16            // control points per axis held in registers (the nodes' limit)

// element offsets, in floats: R(b, i, c, j) = R[r_off + b * r_b + i * r_i + c * r_c + j * r_j] with c = 0: x, 1: y;
// G(t, b, i, c) = G[g_off + t * g_t + b * g_b + i * g_i + c * g_c].  (r_c and g_c are negative where the tensor holds y first.)
struct cbg_layout {
    long long r_off, r_b, r_i, r_c, r_j, g_off, g_t, g_b, g_i, g_c;
};

template <int D>
__global__ __launch_bounds__(256) void k_curve_basis_part(const float *__restrict__ G, const float *__restrict__ R, const cbg_layout L,
                                                          float *__restrict__ part, int B, int d, int T, int sites, long long P) {
    __shared__ float s_red[2][4 * D];           // the four waves' sums of one t; two buffers: one barrier per t
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool act = q < (long long)B * sites;
    const int b = act ? (int)(q / sites) : 0, i = act ? (int)(q - (long long)b * sites) : 0;
    const float *r = R + L.r_off + b * L.r_b + i * L.r_i;
    const float *g = G + L.g_off + b * L.g_b + i * L.g_i;
    float rx[D], ry[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        rx[j] = (act && j < d) ? r[j * L.r_j] : 0.f;
        ry[j] = (act && j < d) ? r[L.r_c + j * L.r_j] : 0.f;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int t = 0; t < T; ++t) {
        const float gx = act ? g[t * L.g_t] : 0.f, gy = act ? g[t * L.g_t + L.g_c] : 0.f;
        float *sr = s_red[t & 1];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (j < d) {                        // (uniform over the workgroup: every lane takes part in the butterfly)
                float v = gx * rx[j] + gy * ry[j];
                for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
                if (lane == 0) sr[MPC_IDX(wv * D + j, 4 * D)] = v;
            }
        }
        __syncthreads();                        // (the writes of t + 2 into this buffer lie behind the barrier of t + 1)
        if ((int)threadIdx.x < d) {
            const int j = threadIdx.x;
            part[MPC_IDX(((long long)blockIdx.x * T + t) * d + j, P * T * d)] =
                ((sr[MPC_IDX(j, 4 * D)] + sr[MPC_IDX(D + j, 4 * D)]) + sr[MPC_IDX(2 * D + j, 4 * D)]) + sr[MPC_IDX(3 * D + j, 4 * D)];
        }
    }
}

// grad_basis[e] = scale * sum over the P partials part[p][e], e = (t, j): one workgroup per element
__global__ __launch_bounds__(256) void k_curve_basis_sum(const float *__restrict__ part, float *__restrict__ grad_basis, long long P, int ne,
                                                         float scale) {
    __shared__ float s[256];
    const float v = mpc_partials_sum(part, P, ne, (int)blockIdx.x, s);
    if (threadIdx.x == 0) grad_basis[blockIdx.x] = v * scale;
}

static int cbg_check(const char *who, int layout, int B, int d, int T, int sites) {
    if (B < 0 || sites < 0 || d < 1 || T < 1) { mpc_set_error("%s: bad B / d / T / sites", who); return MPC_E_SHAPE; }
    if (layout != MPC_CBG_PLAIN && layout != MPC_CBG_ROWS && layout != MPC_CBG_LOOKUP) { mpc_set_error("%s: unknown layout %d", who, layout); return MPC_E_UNSUPPORTED; }
    if (d > CBG_DMAX || (size_t)T * d * sizeof(float) > 48 * 1024) {
        mpc_set_error("%s: more than %d control points per axis (or a basis matrix beyond 48 KB)", who, CBG_DMAX);
        return MPC_E_UNSUPPORTED;
    }
    if (((long long)B * sites + 255) / 256 > 0x7fffffffll) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    return 0;
}

extern "C" int64_t mpc_curve_basis_grad_scratch_floats(int32_t B, int32_t d, int32_t T, int32_t sites) {
    int rc = cbg_check(__func__, MPC_CBG_PLAIN, B, d, T, sites);
    if (rc) return rc;
    return (((int64_t)B * sites + 255) / 256) * T * d;
}

extern "C" int mpc_curve_basis_grad(const float *G, const float *R, int32_t layout, float scale, float *grad_basis, float *scratch,
                                    int32_t B, int32_t d, int32_t T, int32_t sites, void *stream) {
    int rc = cbg_check(__func__, layout, B, d, T, sites);
    if (rc) return rc;
    MPC_CHECK_ARG(grad_basis, MPC_E_NULL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)B * sites, P = (total + 255) / 256;
    if (total > 0) {                            // (without a site G, R and scratch are empty: they may come as NULL and are not read)
        MPC_CHECK_ARG(G && R && scratch, MPC_E_NULL, "null argument");
        const long long n = sites;
        cbg_layout L;
        if (layout == MPC_CBG_ROWS) {           // R = rows [B * sites][2][d], y first
            L.r_off = d; L.r_b = n * 2 * d; L.r_i = 2 * d; L.r_c = -d; L.r_j = 1;
        } else {                                // R = params [B][2][d][sites], x first
            L.r_off = 0; L.r_b = 2 * d * n; L.r_i = 1; L.r_c = d * n; L.r_j = n;
        }
        if (layout == MPC_CBG_LOOKUP) {         // G = grad_coords [T][B][2][sites], x first
            L.g_off = 0; L.g_t = (long long)B * 2 * n; L.g_b = 2 * n; L.g_i = 1; L.g_c = n;
        } else {                                // G = grad_traj [B][T][sites][2], y first
            L.g_off = 1; L.g_t = 2 * n; L.g_b = (long long)T * 2 * n; L.g_i = 2; L.g_c = -1;
        }
        const dim3 grid((unsigned)P);
        if (d <= 4) MPC_LAUNCH(k_curve_basis_part<4>, grid, dim3(256), 0, st, G, R, L, scratch, B, d, T, sites, P);
        else if (d <= 10) MPC_LAUNCH(k_curve_basis_part<10>, grid, dim3(256), 0, st, G, R, L, scratch, B, d, T, sites, P);
        else MPC_LAUNCH(k_curve_basis_part<CBG_DMAX>, grid, dim3(256), 0, st, G, R, L, scratch, B, d, T, sites, P);
        MPC_CHECK_LAUNCH();
    }
    // (B = 0 or no site: a sum over no partials, zeros)
    MPC_LAUNCH(k_curve_basis_sum, dim3((unsigned)(T * d)), dim3(256), 0, st, scratch, grad_basis, P, T * d, scale);
    MPC_CHECK_LAUNCH();
    return 0;
}

MPC_BOUNDS_UNIT("curve_basis.hip")
