// The per-event continuous-time warp, the code its three families share (events.hip: the basis tensor / built-in polynomial and the
// tabulated basis; pe_curves.hip: RAFT-spline curves; tiles.hip: the smoothness field of both).  The tests that hold the families
// to each other bit for bit hold because every line below exists once.
#pragma once
#include "common.h"
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

// the LUT cell of an event's own position (y, x) in sample b (focus.py:186-187)
__device__ __forceinline__ int pe_own_cell(int b, float y, float x, int sp, int hq, int wq) {
    const int iy = min(max((int)floorf(mpc_div_sp(y, sp)), 0), hq - 1), ix = min(max((int)floorf(mpc_div_sp(x, sp)), 0), wq - 1);
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
