// The per-event continuous-time warp, the code its three families share (pe_basis.hip: the basis tensor / built-in polynomial and the
// tabulated basis; pe_curves.hip: RAFT-spline curves; tiles.hip: the smoothness field of both).  The tests that hold the families
// to each other bit for bit hold because every line below exists once; the event row they all read is ev_device.h.
#pragma once
#include "ev_device.h"
#include "bounds.h"

#define PE_KMAX 8              // basis orders the basis families hold in registers (beyond: k_pe_*<0> read phi per use)
#define PEC_DMAX 16            // control points per axis of a curve
#define PE_LDS_MAX (150 * 1024)  // dynamic LDS of the ordered accumulate kernels (they have 1 KB of static LDS of their own)

// the grid of the kernels that stride over the B * M rows with 256 threads
static inline int pe_row_grid(int64_t total) { return (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384); }

// field[(b, t)][cell] = (sum_j rows[(b, cell)][0][j] phim[t][j], sum_j rows[(b, cell)][1][j] phim[t][j]), k <= KMAX, nb <= 64 (the
// layout mpc_lut_smooth takes): mpc_pe_basis_field is <8>, mpc_pec_field <16>
template <int KMAX>
__global__ __launch_bounds__(256) void k_basis_field(const float *__restrict__ rows, const float *__restrict__ phim, float *__restrict__ field,
                                                     int B, int G, int k, int nb) {
    __shared__ float s_phi[64 * KMAX];
    for (int i = threadIdx.x; i < nb * k; i += 256) s_phi[i] = phim[i];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // (b, cell)
    if (i >= (long long)B * G) return;
    const int b = (int)(i / G), cell = (int)(i - (long long)b * G);
    float cy[KMAX], cx[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        cy[j] = j < k ? rows[(size_t)i * 2 * k + j] : 0.f;
        cx[j] = j < k ? rows[(size_t)i * 2 * k + k + j] : 0.f;
    }
    for (int t = 0; t < nb; ++t) {
        float fy = 0.f, fx = 0.f;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) { fy += cy[j] * s_phi[t * k + j]; fx += cx[j] * s_phi[t * k + j]; }
        reinterpret_cast<float2 *>(field)[((size_t)b * nb + t) * G + cell] = make_float2(fy, fx);
    }
}

template <int KMAX>
static int pe_field_run(const char *who, const char *beyond, const float *rows, const float *phim, float *field, int B, int G, int k, int nb,
                        void *stream) {
    if (!(rows && phim && field)) { mpc_set_error("%s: null argument", who); return MPC_E_NULL; }
    if (!(B >= 0 && G >= 0 && k >= 1 && nb >= 1)) { mpc_set_error("%s: bad shape", who); return MPC_E_SHAPE; }
    if (!(k <= KMAX && nb <= 64)) { mpc_set_error("%s: %s", who, beyond); return MPC_E_UNSUPPORTED; }
    if ((long long)B * G == 0) return 0;
    MPC_LAUNCH(k_basis_field<KMAX>, dim3((unsigned)(((long long)B * G + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, phim, field, B, G, k, nb);
    MPC_CHECK_LAUNCH();
    return 0;
}

// Q33.30 of one phi * gradient product, rounded to NEAREST: at most 2^-31 per row added, and no bias (with small event weights a
// product is a few units of 2^-30, and a conversion that truncates towards zero shrinks every sum by half a unit per row)
__device__ __forceinline__ long long pe_to_fixed(float v) {         // |v| < 2^31
    const float hi = truncf(v);
    return ((long long)(int)hi << MPC_FIX_SHIFT) + (long long)__float2int_rn((v - hi) * (float)(1 << MPC_FIX_SHIFT));
}

// The tabulated basis: a table T [S + 1][k] of samples of the basis at the knots i / S, interpolated linearly.  The DEFINITION is
// these five fp32 operations, one per line, nothing fused (utils.table_basis_values spells the same lines in torch and must agree
// bit for bit):
//   tc = min(max(t, 0), 1);  x = tc * (float)S;  i = min((int)floorf(x), S - 1);  f = x - (float)i;  B_j = T[i][j] + f * (T[i+1][j] - T[i][j])
// (t == 1 lands in the last interval with f == 1).
__device__ __forceinline__ void pe_tab_locate(float t, int S, int &i, float &f) {
    const float tc = fminf(fmaxf(t, 0.f), 1.f);
    const float x = tc * (float)S;
    i = min((int)floorf(x), S - 1);
    f = x - (float)i;
}
// one order: a = T[i][j], a1 = T[i+1][j] (the difference in a float of its own: every operation rounds once)
__device__ __forceinline__ float pe_tab_lerp(float a, float a1, float f) {
    const float d = a1 - a;
    return a + f * d;
}

// ---- the gradient w.r.t. a tabulated basis through the events (pe_basis.hip: mpc_pe_table_basis_grad, k <= 8; pe_curves.hip:
// mpc_pec_table_basis_grad, d <= 16 -- ONE body, instantiated on the largest order count KMAX) ----
//   pe_table_grad_body : ONE streaming pass over the rows' (t, cell), the stored unscaled (gy, gx) and the tile rows (cache-resident,
//               cell-coherent in the ordered layout).  G_j = gy c[cell][0][j] + gx c[cell][1][j];  acc[i][j] += (1 - f) G_j,
//               acc[i + 1][j] += f G_j, sum[j] += G_j, with (i, f) of the row's time (pe_tab_locate).  The accumulators
//               [(S + 1) k knot entries + k sums] live in LDS as Q33.30 (pe_to_fixed: round to nearest; ds_add_u64), every workgroup
//               adds its non-zero entries to the global 64-bit accumulators at the end: integer sums, so the result is bitwise
//               the same for any order of the rows, any grid and either event layout.
//               BOUNDS: pe_to_fixed takes |G_j| < 2^31 -- G is (event weight) x (a difference of adjoint-image values, O(1) in the
//               unscaled units of MPC_SCAL_GCOEF) x (a tile coefficient: a displacement in pixels); a knot's sum over the WHOLE batch
//               must stay below 2^33 in magnitude (S = 1 puts every event on two knots: 2.8 M events x a mean |G| of 3000).
//               A time-sorted batch (the DSEC loader's) puts the 64 lanes of a wavefront on one or two neighbouring intervals,
//               i.e. 64 adds to the same two or three LDS words.  Every live lane adds by itself all the same: summing the knots'
//               integers across the lanes with shuffles first (lane 0 adding once) was measured and is no faster -- 75 against
//               68 us on a time-sorted C3 batch, 46 against 47 us on a bucket-ordered one -- the pass is
//               bound by its gathers of tile rows, not by the LDS.  The sums over ALL events stay in registers and are added once
//               per wavefront (every lane of every wavefront would hit the same k words).
//   pe_table_finish_one : grad_table[i][j] = scal[GCOEF] grad_out (-acc[i][j] + [i == ir] (1 - fr) sum[j] + [i == ir + 1] fr sum[j]),
//               (ir, fr) of t_ref: phi_j = B_j(t_ref) - B_j(t_event), products unscaled until here
#define PE_TAB_NT 1024
#define PE_TABLE_MAX_ENTRIES 16384          // (S + 1) * k: 128 KB of 64-bit accumulators (+ k sums) in the CU's 160 KB
__device__ __forceinline__ long long pe_wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// KB > 0: exactly KB orders, the loops unrolled; KB == 0: min(k, KMAX) orders.  coef [ncell][2][k]; total = B * M rows.
template <int KB, int KMAX>
__device__ __forceinline__ void pe_table_grad_body(size_t total, int ncell, const float *__restrict__ rows, const float2 *__restrict__ gpos,
                                                   const float *__restrict__ coef, int S, int k, unsigned long long *__restrict__ acc) {
    extern __shared__ unsigned long long s_tacc[];          // [(S + 1) * kk] knots, then [kk] sums
    const int tid = threadIdx.x, kk = KB > 0 ? KB : min(k, KMAX);
    const int nent = (S + 1) * kk, nall = nent + kk;
    for (int i = tid; i < nall; i += PE_TAB_NT) s_tacc[MPC_IDX(i, nall)] = 0ull;
    __syncthreads();
    long long sg[KB > 0 ? KB : KMAX];
    for (int j = 0; j < kk; ++j) sg[j] = 0;
    for (size_t base = (size_t)blockIdx.x * PE_TAB_NT; base < total; base += (size_t)gridDim.x * PE_TAB_NT) {
        const size_t row = base + tid;
        float2 g = make_float2(0.f, 0.f);
        if (row < total) g = gpos[row];
        if (g.x == 0.f && g.y == 0.f) continue;                 // (a row of weight 0, or past the end: contributes nothing)
        const float2 tp = *reinterpret_cast<const float2 *>(rows + row * 6 + 2);         // (t, p)
        const int cell = min(max(__float_as_int(rows[row * 6 + 4]), 0), ncell - 1);     // (rows of the family's warp; never outside coef)
        int i; float f;
        pe_tab_locate(tp.x, S, i, f);
        const float one_f = 1.f - f;
        const float *c = coef + (size_t)cell * 2 * k;
        for (int j = 0; j < kk; ++j) {
            const float py = g.x * c[j], px = g.y * c[k + j];
            const float G = py + px;
            // (0 <= i <= S - 1: both knots lie inside the [S + 1] rows)
            atomicAdd(&s_tacc[MPC_IDX((size_t)i * kk + j, nent)], (unsigned long long)pe_to_fixed(one_f * G));
            atomicAdd(&s_tacc[MPC_IDX((size_t)(i + 1) * kk + j, nent)], (unsigned long long)pe_to_fixed(f * G));
            sg[j] += pe_to_fixed(G);
        }
    }
    for (int j = 0; j < kk; ++j) {
        const long long v = pe_wave_sum_ll(sg[j]);
        if ((tid & 63) == 0 && v != 0) atomicAdd(&s_tacc[MPC_IDX(nent + j, nall)], (unsigned long long)v);
    }
    __syncthreads();
    for (int i = tid; i < nall; i += PE_TAB_NT) {
        const unsigned long long v = s_tacc[MPC_IDX(i, nall)];
        if (v != 0ull) atomicAdd(acc + i, v);
    }
}

// entry idx of grad_table [S + 1][k] from acc [(S + 1) * k knots, then k sums]
__device__ __forceinline__ void pe_table_finish_one(int idx, const unsigned long long *__restrict__ acc, int S, int k, const float *__restrict__ t_ref,
                                                    const float *__restrict__ scal, const float *__restrict__ grad_out, float *__restrict__ gtable) {
    const int nent = (S + 1) * k;
    if (idx >= nent) return;
    const int i = idx / k, j = idx - i * k;
    const float coef = scal[MPC_SCAL_GCOEF] * (grad_out ? grad_out[0] : 1.f);
    int ir; float fr;
    pe_tab_locate(t_ref[0], S, ir, fr);
    const double unit = 1.0 / (double)(1 << MPC_FIX_SHIFT);
    const double sum = (double)(long long)acc[nent + j] * unit;
    double v = -((double)(long long)acc[idx] * unit);
    if (i == ir) v += (double)(1.f - fr) * sum;
    if (i == ir + 1) v += (double)fr * sum;
    gtable[idx] = v == 0.0 ? 0.f : coef * (float)v;            // (no contribution stays 0 where the objective's scale is not finite: no events)
}

// The host side of both table-gradient entry points, after their own argument checks: zero `acc` [(S + 2) * k], raise the dynamic
// LDS of the family's instantiations `fns` once per device (`once`: the caller's static), launch_grad(grid, lds bytes, acc) where
// there are rows, launch_finish(entries).  The launches stay with the caller: MPC_LAUNCH names a kernel by its spelling.
template <int KMAX, class LaunchGrad, class LaunchFinish>
static int pe_table_basis_grad_run(const char *who, const mpc_shape *s, int S, int k, int64_t *acc, hipStream_t st, mpc_device_once &once,
                                   std::initializer_list<const void *> fns, LaunchGrad launch_grad, LaunchFinish launch_finish) {
    const int nent = (S + 1) * k, nall = nent + k;
    const int e0 = mpc_zero_async(acc, (size_t)nall * 8, st);
    if (e0) return e0;
    const int64_t total = (int64_t)s->B * s->M;
    if (total > 0) {
        const int rc = mpc_raise_lds_cap(once, who, (PE_TABLE_MAX_ENTRIES + KMAX) * 8, fns);          // (the knots and the KMAX sums)
        if (rc) return rc;
        // (one workgroup per CU and 1024 rows per trip; a batch of more than 256 Ki rows makes further trips)
        const int grid = (int)((total + PE_TAB_NT - 1) / PE_TAB_NT < 256 ? (total + PE_TAB_NT - 1) / PE_TAB_NT : 256);
        launch_grad(grid, (size_t)nall * 8, reinterpret_cast<unsigned long long *>(acc));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { mpc_set_error("%s: %s", who, hipGetErrorString(e)); return (int)e; }
    }
    launch_finish(nent);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { mpc_set_error("%s: %s", who, hipGetErrorString(e)); return (int)e; }
    return 0;
}

// The adjoint of k_basis_field with respect to phim (a basis that is differentiable: the table routes):
//   gphim[t][j] = gout * sum_{b, cell, d} gfield[(b, t)][cell][d] * rows[(b, cell)][d][j]
// Workgroup (part, t) sums every FB_PARTS-th block of 256 cells in fp64 -- per thread, then block_sum_d: a fixed order -- into
// part[t][part][j]; k_field_basis_grad_sum adds the parts in order.  Bitwise reproducible.  mpc_pe_field_basis_grad is <8>,
// mpc_pec_field_basis_grad <16>.
#define FB_PARTS 64
template <int KMAX>
__global__ __launch_bounds__(256) void k_field_basis_grad_part(const float *__restrict__ gfield, const float *__restrict__ rows,
                                                               double *__restrict__ part, int B, int G, int k, int nb, int P) {
    __shared__ double s_red[256 / 64];
    const int pt = blockIdx.x, t = blockIdx.y;
    const long long n = (long long)B * G;
    double a[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) a[j] = 0.0;
    for (long long i = (long long)pt * 256 + threadIdx.x; i < n; i += (long long)P * 256) {
        const int b = (int)(i / G), cell = (int)(i - (long long)b * G);
        const float2 g = reinterpret_cast<const float2 *>(gfield)[((size_t)b * nb + t) * G + cell];
        const float *c = rows + (size_t)i * 2 * k;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) a[j] += (double)g.x * (double)c[j] + (double)g.y * (double)c[k + j];
    }
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        if (j < k) {                                               // (k is uniform: every thread takes the same branches)
            const double v = block_sum_d<256>(a[j], s_red);
            if (threadIdx.x == 0) part[((size_t)t * P + pt) * k + j] = v;
        }
    }
}

template <int KMAX>          // (KMAX is not used: a template only so that this header may define a __global__ in several translation units)
__global__ __launch_bounds__(256) void k_field_basis_grad_sum(const double *__restrict__ part, const float *__restrict__ gout,
                                                              float *__restrict__ gphim, int k, int nb, int P) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nb * k) return;
    const int t = idx / k, j = idx - t * k;
    double v = 0.0;
    for (int q = 0; q < P; ++q) v += part[((size_t)t * P + q) * k + j];
    gphim[idx] = (float)((double)(gout ? gout[0] : 1.f) * v);
}

template <int KMAX>
static int pe_field_basis_grad_run(const char *who, const char *beyond, const float *grad_field, const float *rows, const float *grad_out,
                                   double *part, float *grad_phim, int B, int G, int k, int nb, void *stream) {
    if (!(grad_field && rows && part && grad_phim)) { mpc_set_error("%s: null argument", who); return MPC_E_NULL; }
    if (!(B >= 0 && G >= 0 && k >= 1 && nb >= 1)) { mpc_set_error("%s: bad shape", who); return MPC_E_SHAPE; }
    if (!(k <= KMAX && nb <= 64)) { mpc_set_error("%s: %s", who, beyond); return MPC_E_UNSUPPORTED; }
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)B * G;
    const int P = (int)((n + 255) / 256 < FB_PARTS ? (n + 255) / 256 : FB_PARTS);
    if (P > 0) {
        MPC_LAUNCH(k_field_basis_grad_part<KMAX>, dim3(P, nb), dim3(256), 0, st, grad_field, rows, part, B, G, k, nb, P);
        MPC_CHECK_LAUNCH();
    }
    MPC_LAUNCH(k_field_basis_grad_sum<KMAX>, dim3((nb * k + 255) / 256), dim3(256), 0, st, part, grad_out, grad_phim, k, nb, P);
    MPC_CHECK_LAUNCH();
    return 0;
}

// the LUT cell of an event's own position (y, x) in sample b (focus.py:186-187)
__device__ __forceinline__ int pe_own_cell(int b, float y, float x, int sp, int hq, int wq) {
    const int iy = ev_cell(y, sp, hq), ix = ev_cell(x, sp, wq);
    return (b * hq + iy) * wq + ix;
}

// the warped row (y + fy, x + fx, t, p, cell bits, valid): the cell goes to column 4 for the backward -- with MPC_F_NO_WARP
// nothing else reads that column
__device__ __forceinline__ void pe_write_row(float *__restrict__ rows_out, size_t row, const float e[6], float fy, float fx, int cell) {
    float2 *o = reinterpret_cast<float2 *>(rows_out + row * 6);
    o[0] = make_float2(e[0] + fy, e[1] + fx);
    o[1] = make_float2(e[2], e[3]);
    o[2] = make_float2(__int_as_float(cell), e[5]);
}

// The ordered accumulate kernels: one workgroup serves the LUT strip cst (CSR cell rows) of sample b and walks the strip's 2 * nb
// row ranges as one sequence q = 0 .. s_pre[nrange] - 1.
struct PeStrip { int crow0, crow1, ncell, cell0; };         // cell rows [crow0, crow1), ncell cells from cell0 on
__device__ __forceinline__ PeStrip pe_strip(int b, int cst, int CSR, int hq, int wq) {
    PeStrip st;
    st.crow0 = cst * CSR; st.crow1 = min(st.crow0 + CSR, hq);
    st.ncell = max(st.crow1 - st.crow0, 0) * wq;
    st.cell0 = (b * hq + st.crow0) * wq;
    return st;
}
// the range that holds q: the last j with s_pre[j] <= q (s_pre[0 .. nrange]: the running counts of the ranges' lengths)
__device__ __forceinline__ int pe_range_of(const int *s_pre, int nrange, int q) {
    int lo = 0, hi = nrange;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_pre[mid] <= q) lo = mid; else hi = mid; }
    return lo;
}
