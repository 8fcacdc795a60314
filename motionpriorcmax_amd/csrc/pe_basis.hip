// The per-event continuous-time basis warp (FocusLoss.calc_per_event_basis): basis tensor, built-in polynomial and tabulated basis.
// Shared with the RAFT-spline curves of pe_curves.hip: pe_device.h.  Compiled with -ffp-contract=off like events.hip.
#include "pe_device.h"

// ---- UNPINNED EXTENSION, fused form (FocusLoss.calc_per_event_basis): the per-event continuous-time basis warp itself and the
// chain from the position gradient back to the tile coefficients, one pass over the events each.
//   k_pe_warp : rows_out[b][i] = (y + sum_k c[cell][0][k] phi[b][i][k], x + sum_k c[cell][1][k] phi[b][i][k], t, p, cell, valid)
//               cell = LUT cell of the event's own position (pe_device.h: pe_own_cell, pe_write_row; the RAFT-spline curves of
//               pe_curves.hip write the same record); coef [B*hq*wq][2][k], phi [B][M][k] (basis_k(t_ref) - basis_k(t))
//   k_pe_grad : grad_coef[cell][d][k] += phi[b][i][k] * d objective / d warped position_d  (float atomics: the gradient of this
//               extension is not bitwise reproducible; the forward is)
// phi[j] = basis_j(t_ref) - basis_j(t), j < k, from the tensor, or -- phi == nullptr: the polynomial basis t^(j+1) (basis.py:26-27) --
// worked out here (one multiply per order instead of 4 k bytes of traffic per event and kernel)
// A third source (TAB; FocusLoss.calc_per_event_basis(basis_type='table')): a table T [S + 1][k] of samples of the basis at the knots
// i / S, interpolated linearly (pe_device.h: pe_tab_locate / pe_tab_lerp, with the definition).  The table is read THROUGH THE
// CACHE in all three kernels: a time-sorted batch puts the 64 lanes of a wavefront on one or two knots (a broadcast load), a
// bucket-ordered one on the knots of one time bin, and an LDS copy of up to 64 KB per workgroup would cost k_pe_warp / k_pe_grad
// their occupancy and does not fit beside k_pe_accum's strip accumulators (up to 150 KB).
template <int KB>
__device__ __forceinline__ void pe_tab_basis(const float *__restrict__ table, int S, int k, float t, float *out /* [KB or min(k, 8)] */) {
    const int kk = KB > 0 ? KB : min(k, PE_KMAX);
    int i; float f;
    pe_tab_locate(t, S, i, f);
    const float *r0 = table + (size_t)i * k, *r1 = r0 + k;
    for (int j = 0; j < kk; ++j) out[j] = pe_tab_lerp(r0[j], r1[j], f);
}
// the table the TAB instantiations read (appended to the kernels' arguments: the other instantiations never load them); bref =
// B(t_ref), formed once per thread before its loop over the rows
struct PeTab { const float *table; int S; };
template <int KB, bool TAB>
__device__ __forceinline__ void pe_tab_ref(const PeTab tb, int k, float tref, float *bref /* [KB or min(k, 8)] */) {
    if (TAB) pe_tab_basis<KB>(tb.table, tb.S, k, tref, bref);
}
template <int KB, bool TAB = false>
__device__ __forceinline__ void pe_phi(const float *__restrict__ phi, size_t row, int k, float t, float tref, float *out /* [KB or min(k, 8)] */,
                                       const PeTab tb = PeTab{nullptr, 0}, const float *bref = nullptr) {
    const int kk = KB > 0 ? KB : min(k, PE_KMAX);       // (k: the row stride of phi; the first PE_KMAX orders go to registers)
    if (TAB) {
        float bt[KB > 0 ? KB : PE_KMAX];
        pe_tab_basis<KB>(tb.table, tb.S, k, t, bt);
        for (int j = 0; j < kk; ++j) out[j] = bref[j] - bt[j];
        return;
    }
    if (phi != nullptr) { for (int j = 0; j < kk; ++j) out[j] = phi[row * k + j]; return; }
    float a = tref, c = t;
    for (int j = 0; j < kk; ++j) { out[j] = a - c; a *= tref; c *= t; }
}

template <int KB, bool TAB = false>
__global__ __launch_bounds__(256) void k_pe_warp(const mpc_shape s, const float *__restrict__ events, const float *__restrict__ coef,
                                                 const float *__restrict__ phi, int k, const float *__restrict__ t_ref,
                                                 float *__restrict__ rows_out, const PeTab tb) {
    const EvParams p = make_params(s);
    const float tref = t_ref ? t_ref[0] : 0.f;
    float bref[KB > 0 ? KB : PE_KMAX];
    pe_tab_ref<KB, TAB>(tb, k, tref, bref);
    const size_t total = (size_t)p.B * p.M;
    for (size_t row = (size_t)blockIdx.x * 256 + threadIdx.x; row < total; row += (size_t)gridDim.x * 256) {
        const int b = (int)(row / p.M);
        float e[6];
        load_event(events, row, e);
        const int cell = pe_own_cell(b, e[0], e[1], p.sp, p.hq, p.wq);
        const float *c = coef + (size_t)cell * 2 * k;
        float fy = 0.f, fx = 0.f;
        float ph[KB > 0 ? KB : PE_KMAX];
        pe_phi<KB, TAB>(phi, row, k, e[2], tref, ph, tb, bref);
        if (KB > 0) {
#pragma unroll
            for (int j = 0; j < KB; ++j) { fy += c[j] * ph[j]; fx += c[KB + j] * ph[j]; }
        } else {
            for (int j = 0; j < k; ++j) { const float f = j < PE_KMAX ? ph[j] : phi[row * k + j]; fy += c[j] * f; fx += c[k + j] * f; }
        }
        pe_write_row(rows_out, row, e, fy, fx, cell);
    }
}

// (TAB with gpos: every row's UNSCALED position gradient (gy, gx) is stored as well -- zeros for the rows of weight 0 --, 8 bytes per
// event, for k_pe_table_grad: the adjoint image's taps are gathered once)
template <int KB, bool TAB = false>
__global__ __launch_bounds__(256) void k_pe_grad(const mpc_shape s, const float *__restrict__ rows, const float *__restrict__ phi, int k,
                                                 const float *__restrict__ t_ref, const float *__restrict__ gimg,
                                                 const float *__restrict__ scal, const float *__restrict__ grad_out,
                                                 float *__restrict__ gcoef, const PeTab tb, float2 *__restrict__ gpos) {
    const EvParams p = make_params(s);
    const float coef = scal[MPC_SCAL_GCOEF] * (grad_out ? grad_out[0] : 1.f);
    const float tref = t_ref[0];
    float bref[KB > 0 ? KB : PE_KMAX];
    pe_tab_ref<KB, TAB>(tb, k, tref, bref);
    const size_t total = (size_t)p.B * p.M;
    for (size_t row = (size_t)blockIdx.x * 256 + threadIdx.x; row < total; row += (size_t)gridDim.x * 256) {
        const int b = (int)(row / p.M), i = (int)(row - (size_t)b * p.M);
        float e[6];
        load_event(rows, row, e);
        const int pol = (p.P == 2 && i >= p.Mp) ? 1 : 0;
        Warped o;
        if (!warp_event_with(p, e, make_float2(0.f, 0.f), tref, o)) {
            if (TAB && gpos != nullptr) gpos[row] = make_float2(0.f, 0.f);
            continue;
        }
        float gy, gx;
        event_pos_grad(p, o, gimg + ((size_t)b * p.P + pol) * p.H * p.W, gy, gx);
        if (TAB && gpos != nullptr) gpos[row] = make_float2(gy, gx);
        gy *= coef; gx *= coef;
        if (gy == 0.f && gx == 0.f) continue;
        const int cell = __float_as_int(e[4]);
        float *g = gcoef + (size_t)cell * 2 * k;
        const int kk = KB > 0 ? KB : k;
        float ph[KB > 0 ? KB : PE_KMAX];
        pe_phi<KB, TAB>(phi, row, k, e[2], tref, ph, tb, bref);
        for (int j = 0; j < kk; ++j) { const float f = (TAB || j < PE_KMAX) ? ph[j] : phi[row * k + j]; atomicAdd(g + j, f * gy); atomicAdd(g + kk + j, f * gx); }
    }
}

//   k_pe_accum: the same gradient WITHOUT global atomics, for bucket-ordered events (mpc_event_bucket_order / ingest: the rows of a
//               (sample, polarity, bin, LUT strip) are contiguous, `offsets`): one workgroup per (sample, LUT strip) walks the
//               2 * nb row ranges of its strip, gathers the adjoint-image taps of every row and adds phi * gradient to the strip's
//               [cell][2][k] accumulators in LDS -- 64-bit fixed point like k_lut_accum: integer sums, bitwise reproducible -- and
//               writes every cell of the strip once (global float atomics ran at ~20 G/s on this chip: 0.83 ms for the 17 M of a C3 step)
//               (pe_device.h: pe_to_fixed, pe_strip, pe_range_of -- shared with k_pec_accum of pe_curves.hip)
#define PE_NT 1024
#define PE_NIF 4
// (TAB with gpos: the unscaled (gy, gx) of every row that contributes is stored for k_pe_table_grad; the caller zeroes gpos first --
// rows outside every range of the offsets table, and rows this kernel skips, then read as zeros)
template <int KB, bool TAB = false>
__global__ __launch_bounds__(PE_NT) void k_pe_accum(const mpc_shape s, int CSR, int NCS, int SPLIT, const int *__restrict__ offsets,
                                                    const float *__restrict__ rows, const float *__restrict__ phi, int k,
                                                    const float *__restrict__ t_ref, const float *__restrict__ gimg,
                                                    const float *__restrict__ scal, const float *__restrict__ grad_out,
                                                    float *__restrict__ gcoef, const PeTab tb, float2 *__restrict__ gpos) {
    extern __shared__ unsigned long long s_pacc[];
    __shared__ int s_r0[2 * 64 + 1], s_pre[2 * 64 + 1];          // first row / running count of the 2 * nb ranges (nb <= 64)
    const EvParams p = make_params(s);
    const int tid = threadIdx.x, kk = KB > 0 ? KB : k;
    // (SPLIT workgroups per (sample, strip), each with every SPLIT-th of the strip's row ranges and a partial output of its own:
    // B * NCS workgroups -- 98 at the DSEC batch -- left most of the CUs idle)
    const int part = blockIdx.x % SPLIT, bs = blockIdx.x / SPLIT;
    const int b = bs / NCS, cst = bs - b * NCS;
    const PeStrip strip = pe_strip(b, cst, CSR, p.hq, p.wq);
    const int ncell = strip.ncell, cell0 = strip.cell0;
    const int NK = p.nb * NCS, nrange = 2 * p.nb;
    for (int i = tid; i < ncell * 2 * kk; i += PE_NT) s_pacc[i] = 0ull;
    if (tid == 0) {
        int run = 0;
        for (int j = 0; j < nrange; ++j) {
            const int pol = j / p.nb, it = j - pol * p.nb;
            const int *o = offsets + (size_t)(b * 2 + pol) * (NK + 1) + it * NCS + cst;
            // (a table that does not belong to the tensor: clamp into the sample, never read outside it)
            const int r0 = min(max(o[0], 0), p.M), r1 = (j % SPLIT == part) ? min(max(o[1], r0), p.M) : r0;
            s_r0[j] = r0; s_pre[j] = run; run += r1 - r0;
        }
        s_pre[nrange] = run;
    }
    __syncthreads();
    const int n = s_pre[nrange];
    const float tref = t_ref[0];
    float bref[KB > 0 ? KB : PE_KMAX];
    pe_tab_ref<KB, TAB>(tb, k, tref, bref);
    for (int q0 = tid; q0 < n; q0 += PE_NIF * PE_NT) {
        float e[PE_NIF][6];
        size_t grow[PE_NIF];
        bool on[PE_NIF];
        int pol[PE_NIF];
#pragma unroll
        for (int u = 0; u < PE_NIF; ++u) {
            const int q = q0 + u * PE_NT;
            on[u] = q < n;
            int j = 0;
            if (on[u]) j = pe_range_of(s_pre, nrange, q);
            const int row = on[u] ? s_r0[j] + (q - s_pre[j]) : 0;
            pol[u] = (p.P == 2) ? (row >= p.Mp ? 1 : 0) : 0;
            grow[u] = (size_t)b * p.M + row;
            load_event(rows, grow[u], e[u]);
        }
        float gy[PE_NIF], gx[PE_NIF];
#pragma unroll
        for (int u = 0; u < PE_NIF; ++u) {
            Warped o;
            gy[u] = gx[u] = 0.f;
            if (on[u] && warp_event_with(p, e[u], make_float2(0.f, 0.f), tref, o))
                event_pos_grad(p, o, gimg + ((size_t)b * p.P + pol[u]) * p.H * p.W, gy[u], gx[u]);
        }
#pragma unroll
        for (int u = 0; u < PE_NIF; ++u) {
            const int lc = __float_as_int(e[u][4]) - cell0;
            MPC_EXPECT(!on[u] || (gy[u] == 0.f && gx[u] == 0.f) || (lc >= 0 && lc < ncell));      // (a row outside its strip: the offsets table is not this tensor's)
            if (!on[u] || lc < 0 || lc >= ncell || (gy[u] == 0.f && gx[u] == 0.f)) continue;
            if (TAB && gpos != nullptr) gpos[grow[u]] = make_float2(gy[u], gx[u]);
            float ph[KB > 0 ? KB : PE_KMAX];
            pe_phi<KB, TAB>(phi, grow[u], k, e[u][2], tref, ph, tb, bref);
            unsigned long long *a = s_pacc + (size_t)lc * 2 * kk;
            for (int j = 0; j < kk; ++j) {
                const float f = (TAB || j < PE_KMAX) ? ph[j] : phi[grow[u] * k + j];
                atomicAdd(a + j, (unsigned long long)pe_to_fixed(f * gy[u]));
                atomicAdd(a + kk + j, (unsigned long long)pe_to_fixed(f * gx[u]));
            }
        }
    }
    __syncthreads();
    const float coef = scal[MPC_SCAL_GCOEF] * (grad_out ? grad_out[0] : 1.f);
    float *dst = gcoef + ((size_t)part * p.B * p.hq * p.wq + cell0) * 2 * kk;
    for (int i = tid; i < ncell * 2 * kk; i += PE_NT) dst[i] = coef * mpc_from_fixed((long long)s_pacc[i]);
}

// ---- entry points.  Every operation has ONE implementation that takes (phi, PeTab, gpos) and launches the TAB instantiation where
// there is a table; the public functions of the two families keep what differs between them -- their own pointers and the limits
// on k and S -- in the order they always had, and hand over.
#define PE_DISPATCH(kern, TAB, grid, block, lds, st, ...)                                        \
    do {                                                                                         \
        if (k == 1) MPC_LAUNCH((kern<1, TAB>), grid, block, lds, st, __VA_ARGS__);               \
        else if (k == 3) MPC_LAUNCH((kern<3, TAB>), grid, block, lds, st, __VA_ARGS__);          \
        else MPC_LAUNCH((kern<0, TAB>), grid, block, lds, st, __VA_ARGS__);                      \
    } while (0)
#define PE_DISPATCH_TB(kern, grid, block, lds, st, ...)                                          \
    do {                                                                                         \
        if (tb.table) PE_DISPATCH(kern, true, grid, block, lds, st, __VA_ARGS__);                \
        else PE_DISPATCH(kern, false, grid, block, lds, st, __VA_ARGS__);                        \
    } while (0)
static const PeTab PE_NO_TAB{nullptr, 0};

static int pe_warp_impl(const mpc_shape *s, const float *events, const float *coef_rows, const float *phi, int k, const PeTab tb,
                        const float *t_ref, float *rows_out, void *stream) {
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    const int64_t total = (int64_t)s->B * s->M;
    if (total == 0) return 0;
    PE_DISPATCH_TB(k_pe_warp, dim3(pe_row_grid(total)), dim3(256), 0, (hipStream_t)stream, *s, events, coef_rows, phi, k, t_ref, rows_out, tb);
    MPC_CHECK_LAUNCH();
    return 0;
}

static int pe_grad_impl(const mpc_shape *s, const float *rows, const float *phi, int k, const PeTab tb, const float *t_ref,
                        const float *grad_iwe, const float *scal, const float *grad_out, float *grad_coef_rows, float2 *gpos, void *stream) {
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int e0 = mpc_zero_async(grad_coef_rows, (size_t)s->B * s->hq * s->wq * 2 * k * sizeof(float), st);
    if (e0) return e0;
    const int64_t total = (int64_t)s->B * s->M;
    if (total == 0) return 0;
    PE_DISPATCH_TB(k_pe_grad, dim3(pe_row_grid(total)), dim3(256), 0, st, *s, rows, phi, k, t_ref, grad_iwe, scal, grad_out, grad_coef_rows, tb, gpos);
    MPC_CHECK_LAUNCH();
    return 0;
}

// 1 where mpc_pe_grad_ordered serves (shape, k) -- a LUT strip's [cell][2][k] accumulators fit the LDS, num_bins <= 64 --, 0 where
// the caller has to take mpc_pe_grad (the one copy of the rule: the Python side asks instead of restating it)
extern "C" int32_t mpc_pe_grad_ordered_supported(const mpc_shape *s, int32_t k) {
    if (!s || mpc_validate_shape(s)) return 0;
    if (!(s->flags & MPC_F_NO_WARP) || s->T != 1 || k < 1 || k > 64 || s->nb > 64 || s->B <= 0) return 0;
    const mpc_ws_layout L = mpc_layout(s);
    if (L.n_cstrips <= 0) return 0;
    return (size_t)L.cstrip_rows * s->wq * 2 * k * 8 <= PE_LDS_MAX ? 1 : 0;
}

// (gpos: zeroed here first -- rows outside every range of the offsets table, and rows the kernel skips, carry no gradient)
static int pe_grad_ordered_impl(const mpc_shape *s, const float *rows, const int32_t *offsets, const float *phi, int k, const PeTab tb,
                                const float *t_ref, const float *grad_iwe, const float *scal, const float *grad_out, float *grad_coef_rows,
                                int split, float2 *gpos, void *stream) {
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    if (s->B == 0) return 0;
    const mpc_ws_layout L = mpc_layout(s);
    MPC_CHECK_ARG(L.n_cstrips > 0, MPC_E_UNSUPPORTED, "no bucketed event layout for this shape");
    const size_t lds = (size_t)L.cstrip_rows * s->wq * 2 * k * 8;
    MPC_CHECK_ARG(lds <= PE_LDS_MAX, MPC_E_UNSUPPORTED, "a LUT strip's accumulators do not fit the LDS (use the atomic gradient)");
    MPC_CHECK_ARG(split >= 1 && split <= 16, MPC_E_SHAPE, "1 <= split <= 16");
    hipStream_t st = (hipStream_t)stream;
    static mpc_device_once attr_once;
    // (these kernels have 1 KB of static LDS of their own: the 160 KB - 512 of events.hip would pass the CU's 160 KB)
    if ((rc = mpc_raise_lds_cap(attr_once, __func__, PE_LDS_MAX + 2048,
                                {(const void *)k_pe_accum<1, false>, (const void *)k_pe_accum<3, false>, (const void *)k_pe_accum<0, false>,
                                 (const void *)k_pe_accum<1, true>, (const void *)k_pe_accum<3, true>, (const void *)k_pe_accum<0, true>})))
        return rc;
    if (gpos != nullptr && (int64_t)s->B * s->M > 0) {
        const int e0 = mpc_zero_async(gpos, (size_t)s->B * s->M * 2 * sizeof(float), st);
        if (e0) return e0;
    }
    PE_DISPATCH_TB(k_pe_accum, dim3(s->B * L.n_cstrips * split), dim3(PE_NT), lds, st, *s, L.cstrip_rows, L.n_cstrips, split, offsets, rows, phi, k,
                   t_ref, grad_iwe, scal, grad_out, grad_coef_rows, tb, gpos);
    MPC_CHECK_LAUNCH();
    return 0;
}

#define PE_PHI_K_MSG "1 <= num_basis <= 64 (<= 8 for the built-in polynomial basis)"
#define PE_ROWS_CHECK() MPC_CHECK_ARG((s->flags & MPC_F_NO_WARP) && s->T == 1, MPC_E_UNSUPPORTED, "takes the rows of the per-event warp (MPC_F_NO_WARP), num_tref == 1")

extern "C" int mpc_pe_warp(const mpc_shape *s, const float *events, const float *coef_rows, const float *phi, int32_t k,
                           const float *t_ref, float *rows_out, void *stream) {
    MPC_CHECK_ARG(s && coef_rows && (phi || t_ref) && rows_out && (events || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    MPC_CHECK_ARG(k >= 1 && k <= 64 && (phi || k <= PE_KMAX), MPC_E_SHAPE, PE_PHI_K_MSG);
    return pe_warp_impl(s, events, coef_rows, phi, k, PE_NO_TAB, t_ref, rows_out, stream);
}

extern "C" int mpc_pe_grad(const mpc_shape *s, const float *rows, const float *phi, int32_t k, const float *t_ref, const float *grad_iwe,
                           const float *scal, const float *grad_out, float *grad_coef_rows, void *stream) {
    MPC_CHECK_ARG(s && (phi || t_ref) && grad_iwe && scal && grad_coef_rows && (rows || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    PE_ROWS_CHECK();
    MPC_CHECK_ARG(t_ref, MPC_E_NULL, "t_ref is null");
    MPC_CHECK_ARG(k >= 1 && k <= 64 && (phi || k <= PE_KMAX), MPC_E_SHAPE, PE_PHI_K_MSG);
    return pe_grad_impl(s, rows, phi, k, PE_NO_TAB, t_ref, grad_iwe, scal, grad_out, grad_coef_rows, nullptr, stream);
}

extern "C" int mpc_pe_grad_ordered(const mpc_shape *s, const float *rows, const int32_t *offsets, const float *phi, int32_t k,
                                   const float *t_ref, const float *grad_iwe, const float *scal, const float *grad_out,
                                   float *grad_coef_rows, int32_t split, void *stream) {
    MPC_CHECK_ARG(s && offsets && (phi || t_ref) && grad_iwe && scal && grad_coef_rows && (rows || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    PE_ROWS_CHECK();
    MPC_CHECK_ARG(t_ref, MPC_E_NULL, "t_ref is null");
    MPC_CHECK_ARG(k >= 1 && k <= 64 && (phi || k <= PE_KMAX) && s->nb <= 64, MPC_E_SHAPE, PE_PHI_K_MSG ", num_bins <= 64");
    return pe_grad_ordered_impl(s, rows, offsets, phi, k, PE_NO_TAB, t_ref, grad_iwe, scal, grad_out, grad_coef_rows, split, nullptr, stream);
}

// ---- the table basis (basis_type='table'): the three kernels above as TAB instantiations, and the gradient w.r.t. the table ----
//   k_pe_table_grad / k_pe_table_finish : pe_table_grad_body<KB, PE_KMAX> / pe_table_finish_one (pe_device.h, with the comment on
//               bounds and on time-sorted batches): the body is shared with the curves' k_pec_table_grad, which holds 16 orders
#define PT_NT PE_TAB_NT
template <int KB, bool TAB = true>          // (TAB: the name PE_DISPATCH gives an instantiation; there is no other)
__global__ __launch_bounds__(PT_NT) void k_pe_table_grad(const mpc_shape s, const float *__restrict__ rows, const float2 *__restrict__ gpos,
                                                         const float *__restrict__ coef, int S, int k,
                                                         unsigned long long *__restrict__ acc) {
    const EvParams p = make_params(s);
    pe_table_grad_body<KB, PE_KMAX>((size_t)p.B * p.M, p.B * p.hq * p.wq, rows, gpos, coef, S, k, acc);
}

__global__ __launch_bounds__(256) void k_pe_table_finish(const unsigned long long *__restrict__ acc, int S, int k, const float *__restrict__ t_ref,
                                                         const float *__restrict__ scal, const float *__restrict__ grad_out,
                                                         float *__restrict__ gtable) {
    pe_table_finish_one(blockIdx.x * 256 + threadIdx.x, acc, S, k, t_ref, scal, grad_out, gtable);
}

static bool pe_table_ok(const mpc_shape *s, int32_t k, int32_t S) {
    return (s->flags & MPC_F_NO_WARP) && s->T == 1 && k >= 1 && k <= PE_KMAX && S >= 1 && s->nb <= 64 &&
           (int64_t)(S + 1) * k <= PE_TABLE_MAX_ENTRIES;
}

// 1 where the table kernels serve (shape, k, S) -- k <= 8, num_bins <= 64, (S + 1) * k accumulators within the LDS --, 0 where the
// caller takes its plain-torch route (the one copy of the rule: the Python side asks and never restates it)
extern "C" int32_t mpc_pe_table_supported(const mpc_shape *s, int32_t k, int32_t S) {
    if (!s || mpc_validate_shape(s)) return 0;
    return pe_table_ok(s, k, S) ? 1 : 0;
}

// the largest (S + 1) * k the table kernels take
extern "C" int32_t mpc_pe_table_limit(void) { return PE_TABLE_MAX_ENTRIES; }

#define PE_TABLE_CHECKS(who)                                                                                                              \
    MPC_CHECK_ARG((s->flags & MPC_F_NO_WARP) && s->T == 1, MPC_E_UNSUPPORTED, who " takes MPC_F_NO_WARP shapes, num_tref == 1");            \
    MPC_CHECK_ARG(k >= 1 && k <= PE_KMAX && S >= 1 && s->nb <= 64, MPC_E_SHAPE, "1 <= num_basis <= 8, samples >= 1, num_bins <= 64");       \
    MPC_CHECK_ARG((int64_t)(S + 1) * k <= PE_TABLE_MAX_ENTRIES, MPC_E_UNSUPPORTED, "(samples + 1) * num_basis exceeds mpc_pe_table_limit()")

extern "C" int mpc_pe_table_warp(const mpc_shape *s, const float *events, const float *coef_rows, const float *table, int32_t S, int32_t k,
                                 const float *t_ref, float *rows_out, void *stream) {
    MPC_CHECK_ARG(s && coef_rows && table && t_ref && rows_out && (events || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    PE_TABLE_CHECKS("mpc_pe_table_warp");
    return pe_warp_impl(s, events, coef_rows, nullptr, k, PeTab{table, S}, t_ref, rows_out, stream);
}

extern "C" int mpc_pe_table_grad(const mpc_shape *s, const float *rows, const float *table, int32_t S, int32_t k, const float *t_ref,
                                 const float *grad_iwe, const float *scal, const float *grad_out, float *grad_coef_rows, float *grad_pos,
                                 void *stream) {
    MPC_CHECK_ARG(s && table && t_ref && grad_iwe && scal && grad_coef_rows && (rows || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    PE_TABLE_CHECKS("mpc_pe_table_grad");
    return pe_grad_impl(s, rows, nullptr, k, PeTab{table, S}, t_ref, grad_iwe, scal, grad_out, grad_coef_rows, reinterpret_cast<float2 *>(grad_pos),
                        stream);
}

extern "C" int mpc_pe_table_grad_ordered(const mpc_shape *s, const float *rows, const int32_t *offsets, const float *table, int32_t S, int32_t k,
                                         const float *t_ref, const float *grad_iwe, const float *scal, const float *grad_out,
                                         float *grad_coef_rows, int32_t split, float *grad_pos, void *stream) {
    MPC_CHECK_ARG(s && offsets && table && t_ref && grad_iwe && scal && grad_coef_rows && (rows || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    PE_TABLE_CHECKS("mpc_pe_table_grad_ordered");
    return pe_grad_ordered_impl(s, rows, offsets, nullptr, k, PeTab{table, S}, t_ref, grad_iwe, scal, grad_out, grad_coef_rows, split,
                                reinterpret_cast<float2 *>(grad_pos), stream);
}

extern "C" int mpc_pe_table_basis_grad(const mpc_shape *s, const float *rows, const float *grad_pos, const float *coef_rows, int32_t S, int32_t k,
                                       const float *t_ref, const float *scal, const float *grad_out, int64_t *acc, float *grad_table,
                                       void *stream) {
    MPC_CHECK_ARG(s && coef_rows && t_ref && scal && acc && grad_table && ((rows && grad_pos) || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    PE_TABLE_CHECKS("mpc_pe_table_basis_grad");
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    static mpc_device_once attr_once;
    const float2 *gpos = reinterpret_cast<const float2 *>(grad_pos);
    return pe_table_basis_grad_run<PE_KMAX>(
        __func__, s, S, k, acc, st, attr_once,
        {(const void *)k_pe_table_grad<1>, (const void *)k_pe_table_grad<3>, (const void *)k_pe_table_grad<0>},
        [&](int grid, size_t lds, unsigned long long *a) { PE_DISPATCH(k_pe_table_grad, true, dim3(grid), dim3(PT_NT), lds, st, *s, rows, gpos, coef_rows, S, k, a); },
        [&](int nent) {
            MPC_LAUNCH(k_pe_table_finish, dim3((nent + 255) / 256), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(acc), S, k, t_ref, scal,
                       grad_out, grad_table);
        });
}

MPC_BOUNDS_UNIT("pe_basis.hip")
