// UNPINNED EXTENSION (FocusLoss.calc_per_event_curves; BASELINE.json's north_star and configs[3]): the per-event continuous-time warp
// along RAFT-spline curves.  The RAFT-spline head produces control points 1..d (P0 = 0) on the 1/8 grid plus the convex-upsampling
// mask (reference src/models/raft_spline/curves/base.py:35-38, utils.py:30-45, curves/polynomial.py:60-61: x channels first); every
// event is moved along the curve of its LUT cell evaluated at ITS OWN timestamp -- no time bins, no KNN look-up table, no [B, M, d]
// basis tensor: the basis is evaluated in registers.
//   k_pec_head_rows    rows[(b, cell)][0][j] = scale * up_y[j], rows[(b, cell)][1][j] = scale * up_x[j] at the tile centres
//                      (iy * tile + tile / 2, ix * tile + tile / 2) of the 8h x 8w image (cvx_device.h: cvx_up), or of params themselves
//                      (no mask: h x w is the tile grid).  The tile centre is never added: (centre + v) - centre is not v in fp32.
//   k_pec_warp         rows_out = (y + fy, x + fx, t, p, cell bits, valid) (pe_device.h: pe_own_cell, pe_write_row -- mpc_pe_warp's);
//                      fy = fx = 0; for j ascending: fy += c[0][j] * phi[j], fx += c[1][j] * phi[j]; phi[j] = E_j(t_ref) - E_j(t)
//   k_pec_accum        grad_rows[(b, cell)][a][j] = coef * sum over the cell's rows of phi[j] * gpos[row][a] for bucket-ordered rows:
//                      one workgroup per (sample, LUT strip, pass over a chunk of orders), Q33.30 sums in LDS (ds_add_u64, pe_to_fixed;
//                      strip and ranges as in k_pe_accum -- pe_device.h: bitwise reproducible), every element written once
//   k_pec_grad_atomic  the same with global float atomics (any row order; slow -- ~20 G atomics/s -- and not reproducible)
//   k_pec_*_bsp        the three kernels above for the cubic B-spline (the same bodies, instantiated without the other kinds: those
//                      run exactly the code they ran before the B-spline existed)
//   mpc_pec_field      k_basis_field<16> (pe_device.h)
//   k_pec_field_adj    grad_rows[(b, cell)][a][j] += grad_out * sum_t grad_field[(b, t)][cell][a] * phim[t][j]
//   k_pec_rows_to_*    the transposes between grad_rows and what the head's adjoint takes
//   k_pec_table_grad   d loss / d table through the events (a table that trains): pe_table_grad_body<., 16> (pe_device.h), one streaming
//                      pass, Q33.30 sums in LDS, bitwise reproducible in either layout; k_pec_table_finish: the t_ref knots and the scale
//   mpc_pec_field_basis_grad  k_field_basis_grad_part / _sum <16> (pe_device.h): the adjoint of the field w.r.t. phim, fp64 in a fixed order
// The adjoint of "centre + v" is the adjoint of v: the head's backward with a mask IS mpc_cvx_traj_bwd (cvx_curves.hip) with the identity
// as its basis matrix and grad_rows transposed to [B][d][G][2].
//
// E, the basis at a time t, in fp32 with one rounding per line (-ffp-contract=off; utils.curve_event_basis spells the same lines in
// torch and agrees bit for bit):
//   BEZIER      u = 1 - t;  tp_1 = t, tp_i = tp_{i-1} * t;  up_0 = 1, up_1 = u, up_i = up_{i-1} * u;  E_i = (C(d, i) * tp_i) * up_{d-i}
//               (t = 0: every E_i is exactly 0; t = 1: E_d is exactly 1, the others exactly 0 -- the shortcut rows of curves/base.py:102-106)
//   POLYNOMIAL  E_1 = t, E_i = E_{i-1} * t                                (the lines of pe_phi, pe_basis.hip)
//   TABLE       pe_tab_locate / pe_tab_lerp (pe_device.h, with the definition)
//   BSPLINE     the clamped (open-uniform) cubic B-spline of d + 1 control points (P0 = 0), L = d - 2 spans, d >= 3 (pec_bspline):
//                 tc = min(max(t, 0), 1);  x = tc * (float)L;  s = min((int)floorf(x), L - 1)
//                 u(k) = (float)min(max(s + k, 0), L)          scaled knots, exact small integers, k = -2..3
//                 N_0 = 1
//                 for j = 1..3:  saved = 0
//                     for r = 0..j-1:
//                         right = u(r+1) - x;   left = x - u(1-j+r);   den = u(r+1) - u(1-j+r)      (den is 1, 2 or 3, never 0)
//                         temp = N_r / den;     N_r = saved + right * temp;     saved = left * temp
//                     N_j = saved
//                 E_{s-1+q} = N_q, q = 0..3   (index -1 is P0 and is dropped);   every other E_j = +0
//               (the division is the correctly rounded one: hipcc's default for fp32.  t = 0: every E_j is exactly 0 -- left = 0 in
//               every `saved`; t = 1: right = 0 everywhere, E_d is exactly 1, the others exactly 0.)  At most 4 of the d are non-zero,
//               so phi_j is exactly +0 outside the windows of t_ref and t: k_pec_warp reads the coefficient pairs of the others only
//               (c * 0 added to a sum that starts at +0 never changes it for finite c: the same bits as the dense sum), the two
//               gradient kernels add nothing for them (a zero in the integer sums; +-0 in the float atomics).
#include "ev_device.h"         // load_event
#include "pe_device.h"
#include "cvx_device.h"

#define PEC_NT 1024            // threads of k_pec_accum
#define PEC_NIF 4              // rows in flight per thread of k_pec_accum

struct PecBasis {
    int kind, d, S;
    const float *table;        // [S + 1][d] (MPC_PEC_TABLE)
    float binom[PEC_DMAX];     // C(d, j + 1), exact in fp32 (d <= 16: at most 12870)
};

// the four non-zero functions s .. s + 3 (of the d + 1; function 0 belongs to P0) of the cubic B-spline at t; returns the span s
__device__ __forceinline__ int pec_bspline(int d, float t, float N[4]) {
    const int L = d - 2;
    const float tc = fminf(fmaxf(t, 0.f), 1.f);
    const float x = tc * (float)L;
    const int s = min((int)floorf(x), L - 1);
    float u[6];                                          // u[k + 2] = u(k)
#pragma unroll
    for (int k = -2; k <= 3; ++k) u[k + 2] = (float)min(max(s + k, 0), L);
    N[0] = 1.f;
#pragma unroll
    for (int j = 1; j <= 3; ++j) {
        float saved = 0.f;
#pragma unroll
        for (int r = 0; r < j; ++r) {
            const float right = u[r + 3] - x, left = x - u[3 - j + r], den = u[r + 3] - u[3 - j + r];
            const float temp = N[r] / den;
            N[r] = saved + right * temp;
            saved = left * temp;
        }
        N[j] = saved;
    }
    return s;
}

// BSP: the B-spline has kernels of its own (k_pec_*_bsp), so that the three other kinds run the code they ran before it existed
template <bool BSP>
__device__ __forceinline__ void pec_basis(const PecBasis &pb, float t, float E[PEC_DMAX]) {
    const int d = pb.d;
    if constexpr (BSP) {
        float N[4];
        const int s = pec_bspline(d, t, N);
#pragma unroll
        for (int j = 0; j < PEC_DMAX; ++j) {
            const int q = j + 1 - s;                     // (s + 3 <= d: every j >= d gets 0)
            E[j] = q == 0 ? N[0] : q == 1 ? N[1] : q == 2 ? N[2] : q == 3 ? N[3] : 0.f;
        }
    } else if (pb.kind == MPC_PEC_BEZIER) {
        const float u = 1.f - t;
        float tp = t;
#pragma unroll
        for (int j = 0; j < PEC_DMAX; ++j) {
            if (j < d) { E[j] = pb.binom[j] * tp; tp = tp * t; }
        }
        float w = 1.f;                                   // up_0, up_1 = 1 * u = u exactly
#pragma unroll
        for (int j = PEC_DMAX - 1; j >= 0; --j) {
            if (j < d) { E[j] = E[j] * w; w = w * u; }
        }
    } else if (pb.kind == MPC_PEC_POLYNOMIAL) {
        float c = t;
#pragma unroll
        for (int j = 0; j < PEC_DMAX; ++j) {
            if (j < d) { E[j] = c; c = c * t; }
        }
    } else {
        int i; float f;
        pe_tab_locate(t, pb.S, i, f);
        const float *r0 = pb.table + (size_t)i * d, *r1 = r0 + d;
#pragma unroll
        for (int j = 0; j < PEC_DMAX; ++j) {
            if (j < d) E[j] = pe_tab_lerp(r0[j], r1[j], f);
        }
    }
}

// ---- head rows ------------------------------------------------------------------------------------------------------------------
template <typename M>
__global__ __launch_bounds__(256) void k_pec_head_rows(const float *__restrict__ params, const M *__restrict__ mask, float scale, int tile,
                                                       float *__restrict__ rows, int B, int d, int h, int w, int nty, int ntx) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    const int n = nty * ntx;
    if (gi >= (long long)B * n) return;
    const int b = (int)(gi / n), i = (int)(gi - (long long)b * n);
    const int iy = i / ntx, ix = i - iy * ntx;
    const size_t plane = (size_t)h * w;
    const float *pb = params + (size_t)b * 2 * d * plane;
    float ux[PEC_DMAX], uy[PEC_DMAX];
    if (mask != nullptr) {
        cvx_up<PEC_DMAX>(pb, mask + (size_t)b * 576 * plane, d, h, w, (tile >> 1) + iy * tile, (tile >> 1) + ix * tile, ux, uy);
    } else {
#pragma unroll
        for (int j = 0; j < PEC_DMAX; ++j) {
            ux[j] = j < d ? pb[(size_t)j * plane + i] : 0.f;
            uy[j] = j < d ? pb[(size_t)(d + j) * plane + i] : 0.f;
        }
    }
    float *o = rows + (size_t)gi * 2 * d;
#pragma unroll
    for (int j = 0; j < PEC_DMAX; ++j) {
        if (j < d) { o[j] = scale * uy[j]; o[d + j] = scale * ux[j]; }
    }
}

// grad_rows [B*n][2][d] -> grad_traj [B][d][n][2] (what mpc_cvx_traj_bwd takes with T = d), and the identity matrix [d][d] behind it
__global__ __launch_bounds__(256) void k_pec_rows_to_traj(const float *__restrict__ grows, float *__restrict__ gtraj, float *__restrict__ ident,
                                                          int B, int d, int n) {
    const long long total = (long long)B * d * n;
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi < (long long)d * d) ident[gi] = (gi / d == gi % d) ? 1.f : 0.f;
    if (gi >= total) return;
    const int i = (int)(gi % n);
    const long long r = gi / n;
    const int j = (int)(r % d), b = (int)(r / d);
    const float *g = grows + ((size_t)b * n + i) * 2 * d;
    reinterpret_cast<float2 *>(gtraj)[gi] = make_float2(g[j], g[d + j]);
}

// no mask: grad_params [B][2d][n], channel c < d (x) = scale * grad_rows[.][1][c], channel d + j (y) = scale * grad_rows[.][0][j]
__global__ __launch_bounds__(256) void k_pec_rows_to_params(const float *__restrict__ grows, float scale, float *__restrict__ gparams,
                                                            int B, int d, int n) {
    const long long total = (long long)B * 2 * d * n;
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= total) return;
    const int i = (int)(gi % n);
    const long long r = gi / n;
    const int c = (int)(r % (2 * d)), b = (int)(r / (2 * d));
    const float *g = grows + ((size_t)b * n + i) * 2 * d;
    gparams[gi] = scale * (c < d ? g[d + c] : g[c - d]);
}

// ---- warp -----------------------------------------------------------------------------------------------------------------------
// the flow of one event, j ascending.  SPARSE (the B-spline): an order whose phi_j is exactly 0 is not read -- at most 8 of d remain
template <bool SPARSE>
__device__ __forceinline__ void pec_flow(const float *__restrict__ c, int d, const float Er[PEC_DMAX], const float E[PEC_DMAX], float &fy, float &fx) {
    fy = 0.f; fx = 0.f;
#pragma unroll
    for (int j = 0; j < PEC_DMAX; ++j) {
        if (j < d) {
            const float ph = Er[j] - E[j];
            if (!SPARSE || ph != 0.f) { fy += c[j] * ph; fx += c[d + j] * ph; }
        }
    }
}

template <bool BSP>
__device__ __forceinline__ void pec_warp_body(const mpc_shape &s, const float *__restrict__ events, const float *__restrict__ coef,
                                              const PecBasis &pb, const float *__restrict__ t_ref, float *__restrict__ rows_out) {
    const int d = pb.d;
    float Er[PEC_DMAX];
    pec_basis<BSP>(pb, t_ref[0], Er);
    const size_t total = (size_t)s.B * s.M;
    for (size_t row = (size_t)blockIdx.x * 256 + threadIdx.x; row < total; row += (size_t)gridDim.x * 256) {
        const int b = (int)(row / s.M);
        float e[6];
        load_event(events, row, e);
        const int cell = pe_own_cell(b, e[0], e[1], s.sp, s.hq, s.wq);
        const float *c = coef + (size_t)cell * 2 * d;
        float E[PEC_DMAX];
        pec_basis<BSP>(pb, e[2], E);
        float fy, fx;
        pec_flow<BSP>(c, d, Er, E, fy, fx);
        pe_write_row(rows_out, row, e, fy, fx, cell);
    }
}
__global__ __launch_bounds__(256) void k_pec_warp(const mpc_shape s, const float *__restrict__ events, const float *__restrict__ coef,
                                                  const PecBasis pb, const float *__restrict__ t_ref, float *__restrict__ rows_out) {
    pec_warp_body<false>(s, events, coef, pb, t_ref, rows_out);
}
__global__ __launch_bounds__(256) void k_pec_warp_bsp(const mpc_shape s, const float *__restrict__ events, const float *__restrict__ coef,
                                                      const PecBasis pb, const float *__restrict__ t_ref, float *__restrict__ rows_out) {
    pec_warp_body<true>(s, events, coef, pb, t_ref, rows_out);
}

// ---- row gradient ---------------------------------------------------------------------------------------------------------------
// coef = scal[MPC_SCAL_GCOEF] (or 1) * grad_out[0] (or 1): gpos holds UNSCALED position gradients where the caller hands both over, so
// that the fixed-point products are O(event weight x adjoint-image differences) as in k_pe_accum, whatever the loss scale
__device__ __forceinline__ float pec_coef(const float *__restrict__ scal, const float *__restrict__ grad_out) {
    return (scal ? scal[MPC_SCAL_GCOEF] : 1.f) * (grad_out ? grad_out[0] : 1.f);
}

// one row's adds of the orders j0 .. j0 + kc - 1 into its cell's sums a [2][kc].  SPARSE (the B-spline): an order whose phi_j is exactly
// 0 -- decided from the row's own time, never from its bin -- would add the integer 0 (+-0 in k_pec_grad_atomic): skipped, the same bits
template <bool SPARSE>
__device__ __forceinline__ void pec_accum_row(unsigned long long *a, int j0, int kc, const float Er[PEC_DMAX], const float E[PEC_DMAX], float2 g) {
#pragma unroll
    for (int j = 0; j < PEC_DMAX; ++j) {
        if (j >= j0 && j < j0 + kc) {
            const float ph = Er[j] - E[j];
            if (SPARSE && ph == 0.f) continue;
            atomicAdd(a + MPC_IDX(j - j0, kc), (unsigned long long)pe_to_fixed(ph * g.x));
            atomicAdd(a + MPC_IDX(kc + j - j0, 2 * kc), (unsigned long long)pe_to_fixed(ph * g.y));
        }
    }
}

template <bool SPARSE>
__device__ __forceinline__ void pec_atomic_row(float *o, int d, const float Er[PEC_DMAX], const float E[PEC_DMAX], float2 g) {
#pragma unroll
    for (int j = 0; j < PEC_DMAX; ++j) {
        if (j < d) {
            const float ph = Er[j] - E[j];
            if (SPARSE && ph == 0.f) continue;
            atomicAdd(o + j, ph * g.x); atomicAdd(o + d + j, ph * g.y);
        }
    }
}

template <bool BSP>
__device__ __forceinline__ void pec_accum_body(const mpc_shape &s, int CSR, int NCS, int KC, int NPASS, const int *__restrict__ offsets,
                                               const float *__restrict__ rows, const float2 *__restrict__ gpos, const PecBasis &pb,
                                               const float *__restrict__ t_ref, const float *__restrict__ scal,
                                               const float *__restrict__ grad_out, float *__restrict__ grows) {
    extern __shared__ unsigned long long s_acc[];                // [ncell][2][kc]
    __shared__ int s_r0[2 * 64 + 1], s_pre[2 * 64 + 1], s_cnt[2 * 64];          // first row / running count / length of the 2 * nb ranges (nb <= 64)
    const int tid = threadIdx.x, d = pb.d;
    const int pass = blockIdx.x % NPASS, bs = blockIdx.x / NPASS;
    const int b = bs / NCS, cst = bs - b * NCS;
    const int j0 = pass * KC, kc = min(KC, d - j0);
    const PeStrip strip = pe_strip(b, cst, CSR, s.hq, s.wq);
    const int ncell = strip.ncell, cell0 = strip.cell0;
    const int NK = s.nb * NCS, nrange = 2 * s.nb;
    const int nacc = ncell * 2 * kc;
    for (int i = tid; i < nacc; i += PEC_NT) s_acc[MPC_IDX(i, nacc)] = 0ull;
    // (one lane per range reads its two offsets, then one thread forms the running counts from LDS: read by one thread in turn,
    // the 2 * nb loads cost a memory latency each -- 160 -> 147 us at 41 bins)
    for (int j = tid; j < nrange; j += PEC_NT) {
        const int pol = j / s.nb, it = j - pol * s.nb;
        const int *o = offsets + (size_t)(b * 2 + pol) * (NK + 1) + it * NCS + cst;
        // (a table that does not belong to the tensor: clamp into the sample, never read outside it)
        const int r0 = min(max(o[0], 0), s.M), r1 = min(max(o[1], r0), s.M);
        s_r0[j] = r0; s_cnt[j] = r1 - r0;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int j = 0; j < nrange; ++j) { s_pre[j] = run; run += s_cnt[j]; }
        s_pre[nrange] = run;
    }
    __syncthreads();
    const int n = s_pre[nrange];
    float Er[PEC_DMAX];
    pec_basis<BSP>(pb, t_ref[0], Er);
    // (PEC_NIF rows per thread and iteration, their loads issued together: with one row in flight the pass waits out a memory
    // latency per 1024 rows)
    for (int q0 = tid; q0 < n; q0 += PEC_NIF * PEC_NT) {
        float2 g[PEC_NIF];
        float tt[PEC_NIF];
        int lc[PEC_NIF];
#pragma unroll
        for (int u = 0; u < PEC_NIF; ++u) {
            const int q = q0 + u * PEC_NT;
            const bool on = q < n;
            int lo = 0;
            if (on) lo = pe_range_of(s_pre, nrange, q);
            // (n > 0 here, so the sample has a row 0: a lane past the end loads it and drops it)
            const size_t row = (size_t)b * s.M + (on ? s_r0[lo] + (q - s_pre[lo]) : 0);
            g[u] = gpos[row];
            tt[u] = rows[row * 6 + 2];
            lc[u] = on ? __float_as_int(rows[row * 6 + 4]) - cell0 : -1;
        }
#pragma unroll
        for (int u = 0; u < PEC_NIF; ++u) {
            if (q0 + u * PEC_NT >= n || (g[u].x == 0.f && g[u].y == 0.f)) continue;
            MPC_EXPECT(lc[u] >= 0 && lc[u] < ncell);            // (a row outside its strip: the offsets table is not this tensor's)
            if (lc[u] < 0 || lc[u] >= ncell) continue;
            float E[PEC_DMAX];
            pec_basis<BSP>(pb, tt[u], E);
            unsigned long long *a = s_acc + (size_t)lc[u] * 2 * kc;
            pec_accum_row<BSP>(a, j0, kc, Er, E, g[u]);
        }
    }
    __syncthreads();
    const float coef = pec_coef(scal, grad_out);
    for (int i = tid; i < nacc; i += PEC_NT) {
        const int lc = i / (2 * kc), r = i - lc * 2 * kc, a = r / kc, jj = r - a * kc;
        grows[((size_t)(cell0 + lc) * 2 + a) * d + j0 + jj] = coef * mpc_from_fixed((long long)s_acc[MPC_IDX(i, nacc)]);
    }
}
__global__ __launch_bounds__(PEC_NT) void k_pec_accum(const mpc_shape s, int CSR, int NCS, int KC, int NPASS, const int *__restrict__ offsets,
                                                      const float *__restrict__ rows, const float2 *__restrict__ gpos, const PecBasis pb,
                                                      const float *__restrict__ t_ref, const float *__restrict__ scal,
                                                      const float *__restrict__ grad_out, float *__restrict__ grows) {
    pec_accum_body<false>(s, CSR, NCS, KC, NPASS, offsets, rows, gpos, pb, t_ref, scal, grad_out, grows);
}
__global__ __launch_bounds__(PEC_NT) void k_pec_accum_bsp(const mpc_shape s, int CSR, int NCS, int KC, int NPASS, const int *__restrict__ offsets,
                                                          const float *__restrict__ rows, const float2 *__restrict__ gpos, const PecBasis pb,
                                                          const float *__restrict__ t_ref, const float *__restrict__ scal,
                                                          const float *__restrict__ grad_out, float *__restrict__ grows) {
    pec_accum_body<true>(s, CSR, NCS, KC, NPASS, offsets, rows, gpos, pb, t_ref, scal, grad_out, grows);
}

template <bool BSP>
__device__ __forceinline__ void pec_grad_atomic_body(const mpc_shape &s, const float *__restrict__ rows, const float2 *__restrict__ gpos,
                                                     const PecBasis &pb, const float *__restrict__ t_ref, const float *__restrict__ scal,
                                                     const float *__restrict__ grad_out, float *__restrict__ grows) {
    const int d = pb.d;
    const float coef = pec_coef(scal, grad_out);
    const int ncell = s.B * s.hq * s.wq;
    float Er[PEC_DMAX];
    pec_basis<BSP>(pb, t_ref[0], Er);
    const size_t total = (size_t)s.B * s.M;
    for (size_t row = (size_t)blockIdx.x * 256 + threadIdx.x; row < total; row += (size_t)gridDim.x * 256) {
        float2 g = gpos[row];
        g.x *= coef; g.y *= coef;
        if (g.x == 0.f && g.y == 0.f) continue;
        const float2 tp = reinterpret_cast<const float2 *>(rows + row * 6)[1];
        const int cell = __float_as_int(rows[row * 6 + 4]);
        MPC_EXPECT(cell >= 0 && cell < ncell);
        if (cell < 0 || cell >= ncell) continue;                // (rows that mpc_pec_warp did not write)
        float E[PEC_DMAX];
        pec_basis<BSP>(pb, tp.x, E);
        float *o = grows + (size_t)cell * 2 * d;
        pec_atomic_row<BSP>(o, d, Er, E, g);
    }
}
__global__ __launch_bounds__(256) void k_pec_grad_atomic(const mpc_shape s, const float *__restrict__ rows, const float2 *__restrict__ gpos,
                                                         const PecBasis pb, const float *__restrict__ t_ref, const float *__restrict__ scal,
                                                         const float *__restrict__ grad_out, float *__restrict__ grows) {
    pec_grad_atomic_body<false>(s, rows, gpos, pb, t_ref, scal, grad_out, grows);
}
__global__ __launch_bounds__(256) void k_pec_grad_atomic_bsp(const mpc_shape s, const float *__restrict__ rows, const float2 *__restrict__ gpos,
                                                             const PecBasis pb, const float *__restrict__ t_ref, const float *__restrict__ scal,
                                                             const float *__restrict__ grad_out, float *__restrict__ grows) {
    pec_grad_atomic_body<true>(s, rows, gpos, pb, t_ref, scal, grad_out, grows);
}

// ---- smoothness field and its adjoint -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pec_field_adj(const float *__restrict__ gfield, const float *__restrict__ phim,
                                                       const float *__restrict__ gout, float *__restrict__ grows, int B, int G, int d, int nbm) {
    __shared__ float s_phi[64 * PEC_DMAX];
    for (int i = threadIdx.x; i < nbm * d; i += 256) s_phi[i] = phim[i];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // (b, cell)
    if (i >= (long long)B * G) return;
    const int b = (int)(i / G), cell = (int)(i - (long long)b * G);
    float gy[PEC_DMAX], gx[PEC_DMAX];
#pragma unroll
    for (int j = 0; j < PEC_DMAX; ++j) gy[j] = gx[j] = 0.f;
    for (int t = 0; t < nbm; ++t) {
        const float2 g = reinterpret_cast<const float2 *>(gfield)[((size_t)b * nbm + t) * G + cell];
#pragma unroll
        for (int j = 0; j < PEC_DMAX; ++j)
            if (j < d) { gy[j] += g.x * s_phi[t * d + j]; gx[j] += g.y * s_phi[t * d + j]; }
    }
    const float go = gout ? gout[0] : 1.f;
    float *o = grows + (size_t)i * 2 * d;
#pragma unroll
    for (int j = 0; j < PEC_DMAX; ++j)
        if (j < d) { o[j] += go * gy[j]; o[d + j] += go * gx[j]; }
}

// ---- the gradient w.r.t. a tabulated basis (a table that trains: FocusLoss.calc_per_event_curves with basis_table.requires_grad) ----
// Through the events: pe_table_grad_body / pe_table_finish_one (pe_device.h -- the ONE implementation, pe_basis.hip's k_pe_table_grad is
// its <KB, 8> instantiation; the comment on the fixed-point bounds and on time-sorted batches is there) with 16 orders: `coef` are the
// tile rows of k_pec_head_rows, the records those of k_pec_warp.  <10>: the shipped curve degree, its loops unrolled; <0>: any other d.
template <int KB>
__global__ __launch_bounds__(PE_TAB_NT) void k_pec_table_grad(const mpc_shape s, const float *__restrict__ rows, const float2 *__restrict__ gpos,
                                                              const float *__restrict__ coef, int S, int d, unsigned long long *__restrict__ acc) {
    pe_table_grad_body<KB, PEC_DMAX>((size_t)s.B * s.M, s.B * s.hq * s.wq, rows, gpos, coef, S, d, acc);
}
__global__ __launch_bounds__(256) void k_pec_table_finish(const unsigned long long *__restrict__ acc, int S, int d, const float *__restrict__ t_ref,
                                                          const float *__restrict__ scal, const float *__restrict__ grad_out,
                                                          float *__restrict__ gtable) {
    pe_table_finish_one(blockIdx.x * 256 + threadIdx.x, acc, S, d, t_ref, scal, grad_out, gtable);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------
static int pec_tile_ok(int tile) { return tile == 2 || tile == 4 || tile == 8 || tile == 16; }

// the tile grid of the head: with a mask the centres of the 8h x 8w image, without one the grid of params itself
static int pec_head_grid(const char *who, int B, int d, int h, int w, int tile, int has_mask, int *nty, int *ntx) {
    if (B < 0 || h < 0 || w < 0 || d < 1) { mpc_set_error("%s: bad B / d / h / w", who); return MPC_E_SHAPE; }
    if (d > PEC_DMAX) { mpc_set_error("%s: more than %d control points per axis", who, PEC_DMAX); return MPC_E_UNSUPPORTED; }
    if (has_mask) {
        if (!pec_tile_ok(tile) || (8 * h) % tile || (8 * w) % tile) { mpc_set_error("%s: tile must be 2, 4, 8 or 16 and divide 8h and 8w", who); return MPC_E_SHAPE; }
        *nty = 8 * h / tile; *ntx = 8 * w / tile;
    } else {
        *nty = h; *ntx = w;
    }
    if ((long long)B * *nty * *ntx * 2 * d > (1ll << 31) || (long long)h * w > (1ll << 24)) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    return 0;
}

static int pec_make_basis(const char *who, int basis, int d, const float *table, int S, PecBasis *pb) {
    if (d < 1 || basis < MPC_PEC_BEZIER || basis > MPC_PEC_BSPLINE) { mpc_set_error("%s: bad degree or basis kind", who); return MPC_E_SHAPE; }
    if (d > PEC_DMAX) { mpc_set_error("%s: more than %d control points per axis", who, PEC_DMAX); return MPC_E_UNSUPPORTED; }
    if (basis == MPC_PEC_BSPLINE && d < 3) { mpc_set_error("%s: the cubic B-spline needs degree >= 3 (d + 1 >= 4 control points)", who); return MPC_E_SHAPE; }
    pb->kind = basis; pb->d = d; pb->S = 0; pb->table = nullptr;
    long long c = 1;
    for (int j = 0; j < PEC_DMAX; ++j) {
        if (j < d) c = c * (d - j) / (j + 1);              // C(d, j + 1), exact
        pb->binom[j] = j < d ? (float)c : 0.f;
    }
    if (basis == MPC_PEC_TABLE) {
        if (!table) { mpc_set_error("%s: the table is null", who); return MPC_E_NULL; }
        if (S < 1) { mpc_set_error("%s: a table needs samples >= 1", who); return MPC_E_SHAPE; }
        if ((int64_t)(S + 1) * d > mpc_pe_table_limit()) { mpc_set_error("%s: (samples + 1) * degree exceeds mpc_pe_table_limit()", who); return MPC_E_UNSUPPORTED; }
        pb->S = S; pb->table = table;
    }
    return 0;
}

// orders per pass of k_pec_accum that fit the LDS beside a strip's cells (0: not even one)
static int pec_orders_per_pass(const mpc_shape *s, const mpc_ws_layout &L, int d) {
    if (L.n_cstrips <= 0 || L.cstrip_rows <= 0) return 0;
    const int64_t per_order = (int64_t)L.cstrip_rows * s->wq * 2 * 8;
    const int64_t kc = PE_LDS_MAX / per_order;
    return (int)(kc < d ? kc : d);
}

// The library's choice of orders per pass (orders_per_pass = 0).  Every pass is a workgroup of its own, so FEWER orders per pass
// spread a strip's adds over more CUs at the price of streaming its rows once more per pass: the smallest count whose workgroups
// still fit the device in one round (all choices write the same bits: integer sums per element).  Measured at the C4 shape
// (1 x 500 k events, 7 strips, d = 10): 3 orders per pass (28 workgroups) 179 us, 1 order per pass (70 workgroups) 160 us.
static int pec_choose_orders(const mpc_shape *s, const mpc_ws_layout &L, int d, int kmax) {
    const int64_t groups = (int64_t)s->B * L.n_cstrips, ncu = mpc_cu_count();
    for (int kc = 1; kc < kmax; ++kc)
        if (groups * ((d + kc - 1) / kc) <= ncu) return kc;
    return kmax;
}

extern "C" int32_t mpc_pec_supported(const mpc_shape *s, int32_t d, int32_t basis, int32_t S) {
    if (!s || mpc_validate_shape(s)) return 0;
    if (!(s->flags & MPC_F_NO_WARP) || s->T != 1 || d < 1 || d > PEC_DMAX || s->nb < 1 || s->nb > 64 || s->B < 0) return 0;
    if (basis < MPC_PEC_BEZIER || basis > MPC_PEC_BSPLINE || (basis == MPC_PEC_BSPLINE && d < 3)) return 0;
    if (basis == MPC_PEC_TABLE && (S < 1 || (int64_t)(S + 1) * d > mpc_pe_table_limit())) return 0;
    int32_t r = 1;
    if (s->B > 0) {
        const mpc_ws_layout L = mpc_layout(s);
        if (pec_orders_per_pass(s, L, d) >= 1) r |= 2;
    }
    return r;
}

// the ONE copy of the host code of the two entry points; M: the element type of mask / grad_mask (dt_device.h)
template <typename M>
static int pec_head_rows_run(const char *who, const float *params, const void *mask, float scale, int32_t tile, float *rows,
                             int32_t B, int32_t d, int32_t h, int32_t w, void *stream) {
    MPC_CHECK_ARG_WHO(who, params && rows, MPC_E_NULL, "null argument");
    int nty = 0, ntx = 0;
    int rc = pec_head_grid(who, B, d, h, w, tile, mask != nullptr, &nty, &ntx);
    if (rc) return rc;
    const long long work = (long long)B * nty * ntx;
    if (work == 0) return 0;
    MPC_LAUNCH(k_pec_head_rows<M>, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params, (const M *)mask, scale, tile, rows, B, d, h, w, nty, ntx);
    MPC_CHECK_LAUNCH_WHO(who);
    return 0;
}

extern "C" int mpc_pec_head_rows_dt(const float *params, const void *mask, int32_t dtype, float scale, int32_t tile, float *rows,
                                    int32_t B, int32_t d, int32_t h, int32_t w, void *stream) {
    MPC_DT_RETURN(dtype, pec_head_rows_run, params, mask, scale, tile, rows, B, d, h, w, stream);
}

extern "C" int mpc_pec_head_rows(const float *params, const float *mask, float scale, int32_t tile, float *rows,
                                 int32_t B, int32_t d, int32_t h, int32_t w, void *stream) {
    return mpc_pec_head_rows_dt(params, mask, MPC_DT_F32, scale, tile, rows, B, d, h, w, stream);
}

extern "C" int64_t mpc_pec_head_rows_bwd_workspace_bytes(int32_t B, int32_t d, int32_t h, int32_t w, int32_t tile) {
    int nty = 0, ntx = 0;
    int rc = pec_head_grid(__func__, B, d, h, w, tile, 1, &nty, &ntx);
    if (rc) return rc;
    const int64_t cvx = mpc_cvx_traj_bwd_workspace_bytes(B, d, d, h, w, tile);
    if (cvx < 0) return cvx;
    return mpc_align((int64_t)B * d * nty * ntx * 2 * 4) + mpc_align((int64_t)d * d * 4) + cvx;
}

extern "C" int mpc_pec_head_rows_bwd_dt(const float *grad_rows, const float *params, const void *mask, int32_t dtype, float scale, int32_t tile,
                                        float *grad_params, void *grad_mask, int32_t B, int32_t d, int32_t h, int32_t w, void *ws, void *stream) {
    MPC_CHECK_ARG(dtype == MPC_DT_F32 || dtype == MPC_DT_F16 || dtype == MPC_DT_BF16, MPC_E_UNSUPPORTED,
                  "unknown dtype code (MPC_DT_F32, MPC_DT_F16 or MPC_DT_BF16)");
    MPC_CHECK_ARG(grad_rows && params && grad_params && (!mask || (grad_mask && ws)), MPC_E_NULL, "null argument");
    int nty = 0, ntx = 0;
    int rc = pec_head_grid(__func__, B, d, h, w, tile, mask != nullptr, &nty, &ntx);
    if (rc) return rc;
    const int n = nty * ntx;
    hipStream_t st = (hipStream_t)stream;
    if ((long long)B * h * w == 0) return 0;
    if (mask == nullptr) {
        const long long total = (long long)B * 2 * d * n;
        MPC_LAUNCH(k_pec_rows_to_params, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, grad_rows, scale, grad_params, B, d, n);
        MPC_CHECK_LAUNCH();
        return 0;
    }
    float *gtraj = (float *)ws;
    float *ident = (float *)((char *)ws + mpc_align((int64_t)B * d * n * 2 * 4));
    void *cvx_ws = (char *)ident + mpc_align((int64_t)d * d * 4);
    long long total = (long long)B * d * n;
    if (total < (long long)d * d) total = (long long)d * d;
    MPC_LAUNCH(k_pec_rows_to_traj, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, grad_rows, gtraj, ident, B, d, n);
    MPC_CHECK_LAUNCH();
    return mpc_cvx_traj_bwd_dt(gtraj, params, mask, dtype, ident, scale, grad_params, grad_mask, B, d, d, h, w, tile, cvx_ws, stream);
}

extern "C" int mpc_pec_head_rows_bwd(const float *grad_rows, const float *params, const float *mask, float scale, int32_t tile,
                                     float *grad_params, float *grad_mask, int32_t B, int32_t d, int32_t h, int32_t w, void *ws, void *stream) {
    return mpc_pec_head_rows_bwd_dt(grad_rows, params, mask, MPC_DT_F32, scale, tile, grad_params, grad_mask, B, d, h, w, ws, stream);
}

#define PEC_SHAPE_CHECKS()                                                                                                                   \
    MPC_CHECK_ARG((s->flags & MPC_F_NO_WARP) && s->T == 1, MPC_E_UNSUPPORTED, "takes MPC_F_NO_WARP shapes with num_tref == 1");                \
    { int rc__ = mpc_validate_shape(s); if (rc__) return rc__; }

extern "C" int mpc_pec_warp(const mpc_shape *s, const float *events, const float *rows, int32_t basis, int32_t d, const float *table, int32_t S,
                            const float *t_ref, float *rows_out, void *stream) {
    MPC_CHECK_ARG(s && rows && t_ref && rows_out && (events || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    PEC_SHAPE_CHECKS();
    PecBasis pb;
    int rc = pec_make_basis(__func__, basis, d, table, S, &pb);
    if (rc) return rc;
    const int64_t total = (int64_t)s->B * s->M;
    if (total == 0) return 0;
    const int grid = pe_row_grid(total);
    if (basis == MPC_PEC_BSPLINE) MPC_LAUNCH(k_pec_warp_bsp, dim3(grid), dim3(256), 0, (hipStream_t)stream, *s, events, rows, pb, t_ref, rows_out);
    else MPC_LAUNCH(k_pec_warp, dim3(grid), dim3(256), 0, (hipStream_t)stream, *s, events, rows, pb, t_ref, rows_out);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_pec_rows_grad(const mpc_shape *s, const float *rows_warped, const int32_t *offsets, const float *grad_pos, int32_t basis,
                                 int32_t d, const float *table, int32_t S, const float *t_ref, const float *scal, const float *grad_out,
                                 int32_t orders_per_pass, float *grad_rows, void *stream) {
    MPC_CHECK_ARG(s && t_ref && grad_rows && ((rows_warped && grad_pos) || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    PEC_SHAPE_CHECKS();
    PecBasis pb;
    int rc = pec_make_basis(__func__, basis, d, table, S, &pb);
    if (rc) return rc;
    MPC_CHECK_ARG(orders_per_pass >= 0, MPC_E_SHAPE, "orders_per_pass < 0");
    if (s->B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t out_bytes = (size_t)s->B * s->hq * s->wq * 2 * d * sizeof(float);
    if (offsets == nullptr) {
        const int e0 = mpc_zero_async(grad_rows, out_bytes, st);
        if (e0) return e0;
        const int64_t total = (int64_t)s->B * s->M;
        if (total == 0) return 0;
        const int grid = pe_row_grid(total);
        if (basis == MPC_PEC_BSPLINE)
            MPC_LAUNCH(k_pec_grad_atomic_bsp, dim3(grid), dim3(256), 0, st, *s, rows_warped, reinterpret_cast<const float2 *>(grad_pos), pb, t_ref, scal,
                       grad_out, grad_rows);
        else
            MPC_LAUNCH(k_pec_grad_atomic, dim3(grid), dim3(256), 0, st, *s, rows_warped, reinterpret_cast<const float2 *>(grad_pos), pb, t_ref, scal,
                       grad_out, grad_rows);
        MPC_CHECK_LAUNCH();
        return 0;
    }
    MPC_CHECK_ARG(s->nb <= 64, MPC_E_UNSUPPORTED, "num_bins > 64");
    const mpc_ws_layout L = mpc_layout(s);
    const int kmax = pec_orders_per_pass(s, L, d);
    MPC_CHECK_ARG(kmax >= 1, MPC_E_UNSUPPORTED, "a LUT strip's accumulators of one order do not fit the LDS (pass no offsets)");
    const int kc = orders_per_pass == 0 ? pec_choose_orders(s, L, d, kmax) : (orders_per_pass < d ? orders_per_pass : d);
    MPC_CHECK_ARG(kc <= kmax, MPC_E_UNSUPPORTED, "orders_per_pass beyond what the LDS holds");
    const int npass = (d + kc - 1) / kc;
    const size_t lds = (size_t)L.cstrip_rows * s->wq * 2 * kc * 8;
    static mpc_device_once attr_once;
    // (the kernel has 1 KB of static LDS of its own)
    if ((rc = mpc_raise_lds_cap(attr_once, __func__, PE_LDS_MAX + 2048, {(const void *)k_pec_accum, (const void *)k_pec_accum_bsp}))) return rc;
    if (basis == MPC_PEC_BSPLINE)
        MPC_LAUNCH(k_pec_accum_bsp, dim3(s->B * L.n_cstrips * npass), dim3(PEC_NT), lds, st, *s, L.cstrip_rows, L.n_cstrips, kc, npass, offsets,
                   rows_warped, reinterpret_cast<const float2 *>(grad_pos), pb, t_ref, scal, grad_out, grad_rows);
    else
        MPC_LAUNCH(k_pec_accum, dim3(s->B * L.n_cstrips * npass), dim3(PEC_NT), lds, st, *s, L.cstrip_rows, L.n_cstrips, kc, npass, offsets, rows_warped,
                   reinterpret_cast<const float2 *>(grad_pos), pb, t_ref, scal, grad_out, grad_rows);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t mpc_pec_rows_grad_passes(const mpc_shape *s, int32_t d, int32_t orders_per_pass) {
    if (!s || mpc_validate_shape(s) || d < 1 || d > PEC_DMAX || s->B <= 0) return 0;
    const mpc_ws_layout L = mpc_layout(s);
    const int kmax = pec_orders_per_pass(s, L, d);
    if (kmax < 1) return 0;
    const int kc = orders_per_pass <= 0 ? pec_choose_orders(s, L, d, kmax) : (orders_per_pass < d ? orders_per_pass : d);
    return kc <= kmax ? (d + kc - 1) / kc : 0;
}

extern "C" int mpc_pec_field(const float *rows, const float *phim, float *field, int32_t B, int32_t G, int32_t d, int32_t nbm, void *stream) {
    return pe_field_run<PEC_DMAX>(__func__, "more than 16 orders or 64 field times", rows, phim, field, B, G, d, nbm, stream);
}

extern "C" int mpc_pec_field_adjoint(const float *grad_field, const float *phim, const float *grad_out, float *grad_rows,
                                     int32_t B, int32_t G, int32_t d, int32_t nbm, void *stream) {
    MPC_CHECK_ARG(grad_field && phim && grad_rows, MPC_E_NULL, "null argument");
    MPC_CHECK_ARG(B >= 0 && G >= 0 && d >= 1 && nbm >= 1, MPC_E_SHAPE, "bad shape");
    MPC_CHECK_ARG(d <= PEC_DMAX && nbm <= 64, MPC_E_UNSUPPORTED, "more than 16 orders or 64 field times");
    if ((long long)B * G == 0) return 0;
    MPC_LAUNCH(k_pec_field_adj, dim3((unsigned)(((long long)B * G + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_field, phim, grad_out,
               grad_rows, B, G, d, nbm);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_pec_table_basis_grad(const mpc_shape *s, const float *rows_warped, const float *grad_pos, const float *rows, int32_t d, int32_t S,
                                        const float *t_ref, const float *scal, const float *grad_out, int64_t *acc, float *grad_table, void *stream) {
    MPC_CHECK_ARG(s && rows && t_ref && scal && acc && grad_table && ((rows_warped && grad_pos) || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    PEC_SHAPE_CHECKS();
    MPC_CHECK_ARG(d >= 1 && S >= 1, MPC_E_SHAPE, "degree >= 1, samples >= 1");
    MPC_CHECK_ARG(d <= PEC_DMAX, MPC_E_UNSUPPORTED, "more than 16 control points per axis");
    MPC_CHECK_ARG((int64_t)(S + 1) * d <= mpc_pe_table_limit(), MPC_E_UNSUPPORTED, "(samples + 1) * degree exceeds mpc_pe_table_limit()");
    hipStream_t st = (hipStream_t)stream;
    static mpc_device_once attr_once;
    const float2 *gpos = reinterpret_cast<const float2 *>(grad_pos);
    return pe_table_basis_grad_run<PEC_DMAX>(
        __func__, s, S, d, acc, st, attr_once, {(const void *)k_pec_table_grad<10>, (const void *)k_pec_table_grad<0>},
        [&](int grid, size_t lds, unsigned long long *a) {
            if (d == 10) MPC_LAUNCH(k_pec_table_grad<10>, dim3(grid), dim3(PE_TAB_NT), lds, st, *s, rows_warped, gpos, rows, S, d, a);
            else MPC_LAUNCH(k_pec_table_grad<0>, dim3(grid), dim3(PE_TAB_NT), lds, st, *s, rows_warped, gpos, rows, S, d, a);
        },
        [&](int nent) {
            MPC_LAUNCH(k_pec_table_finish, dim3((nent + 255) / 256), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(acc), S, d, t_ref, scal,
                       grad_out, grad_table);
        });
}

extern "C" int mpc_pec_field_basis_grad(const float *grad_field, const float *rows, const float *grad_out, double *part, float *grad_phim,
                                        int32_t B, int32_t G, int32_t d, int32_t nbm, void *stream) {
    return pe_field_basis_grad_run<PEC_DMAX>(__func__, "more than 16 orders or 64 field times", grad_field, rows, grad_out, part, grad_phim,
                                             B, G, d, nbm, stream);
}

MPC_BOUNDS_UNIT("pe_curves.hip")
