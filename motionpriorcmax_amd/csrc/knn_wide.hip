// KNN flow look-up table for MORE trajectories per sample than the 16-bit tables of knn.hip / knn_strip.hip hold (n >= 65536;
// reference focus.py:129-178 has no such limit).  The exact search stays where it is: the caller runs mpc_knn_lut_fwd on contiguous
// index chunks of at most 65535 points and keeps each chunk's sorted neighbour list (idx_out).  The K nearest of all n points are
// the K smallest, by (distance, index), of the union of the chunks' K nearest; chunks are contiguous index ranges, so the tie rule
// of the search (the lowest trajectory index wins) is the tie rule of the merge.  This file holds what comes after the search:
//   k_knn_merge        C sorted lists per query -> the merged list of global indices, the LUT ('mean' / 'iwd') and flow_to_next
//   k_knn_idx_bwd      dL/dtraj from dL/dLUT (and dL/dflow_next) over a saved index list, in 64-bit fixed point: integer sums,
//                      any order, bitwise reproducible (the scheme of k_knn_bwd_far, knn.hip)
// The merge ranks by distances recomputed with pair_dist at the query centre of knn_one_query (knn_device.h), in the same fp32
// expression (-ffp-contract=off): a near-tie must not rank a point K + 1 in its chunk and K in the merge.
// Kernels only, on the caller's stream; no allocation, no synchronisation.
#include "common.h"
#include "bounds.h"
#include "knn_device.h"
#include <limits.h>
#include <string.h>

#define KW_MAX_CHUNKS 64          // one lane per chunk of a query: a wavefront at most
#define KW_MAX_N (1 << 22)
#define KW_LDS_BYTES (64 * 1024)
#define KW_NONE INT_MAX           // an exhausted (or invalid) list entry: sorts behind every point

struct WideParams {
    int B, nb, T, n, hq, wq, sp, K, G, NQ;      // G = hq * wq cells, NQ = B * nb * G queries
    int C, LPQ, QW;                               // chunks; lanes per query (power of two >= C); queries per wavefront
    int l1, iwd, want_next;
    float off;                                    // sp/2 - 0.5 : centre of cell 0 (focus.py:117)
    int start[KW_MAX_CHUNKS + 1];                 // chunk c holds the points [start[c], start[c + 1])
};

struct WideQuery {
    int b, t, cell;
    float qy, qx;
};
__device__ __forceinline__ WideQuery wide_query(const WideParams &p, int q) {
    WideQuery r;
    const int bt = q / p.G;
    r.cell = q - bt * p.G;
    r.b = bt / p.nb; r.t = bt - r.b * p.nb;
    const int cy = r.cell / p.wq, cx = r.cell - cy * p.wq;
    r.qy = (float)(cy * p.sp) + p.off; r.qx = (float)(cx * p.sp) + p.off;      // as knn_one_query forms it
    return r;
}

// The interpolation itself runs in fp64 on the fp32 inputs and is rounded once: flows of a hundred pixels have an ulp of 7.6e-6, and a
// sum of K of them in fp32 -- in whatever order -- is off by several; the LUT is held to 1e-5 ABSOLUTE.  Only the ranking needs the
// search kernels' fp32 distance.  The 'iwd' weight of a member, before normalisation (focus.py:158-160):
__device__ __forceinline__ double wide_iwd_weight(float qy, float qx, float2 pj, int l1) {
    const double dy = (double)qy - (double)pj.x, dx = (double)qx - (double)pj.y;
    return 1.0 / ((l1 ? fabs(dy) + fabs(dx) : dy * dy + dx * dx) + 1e-9);
}

// ------------------------------------------------------------------------------------------
// merge: one wavefront per workgroup serves QW consecutive queries with LPQ lanes each (lane c of a query owns chunk c).
//   0. the wavefront's candidate words, chunk by chunk, coalesced (consecutive queries are consecutive in [Q][K]); every word
//      becomes (global index, distance) in LDS -- the trajectory gathers are independent of each other and come from L2
//   1. K steps of: smallest head of the query's lists by (distance, index) -- a butterfly over the LPQ lanes --, the owner advances
//   2. the merged lists leave LDS as one contiguous, coalesced store
//   3. the flows of the merged list, summed in list order: a fixed function of the input.  Tasks (reference time or
//      flow_to_next) are dealt to the lanes of the query.
// LDS: s_g int [QW*LPQ*K], s_d float [QW*LPQ*K], s_m int [QW*K]
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_knn_merge(const WideParams p, const float2 *__restrict__ traj, const int *__restrict__ cand,
                                                  int *__restrict__ idx_out, float2 *__restrict__ flow_lut, float2 *__restrict__ flow_next) {
    extern __shared__ int s_mem[];
    const int lane = threadIdx.x;
    const int NL = p.QW * p.LPQ * p.K;
    [[maybe_unused]] const int NM = p.QW * p.K;                 // (extents of the checked accessors: unused in the product build)
    int *s_g = s_mem;
    float *s_d = reinterpret_cast<float *>(s_mem + NL);
    int *s_m = s_mem + 2 * NL;
    const int q0 = (int)blockIdx.x * p.QW;
    const int nq = min(p.QW, p.NQ - q0);
    const size_t rows = (size_t)(p.T + p.nb);
    [[maybe_unused]] const size_t ntraj = (size_t)p.B * rows * p.n;
    // ---- 0 ----
    for (int c = 0; c < p.C; ++c) {
        const int *cc = cand + ((size_t)c * p.NQ + q0) * p.K;
        const int lo = p.start[c], len = p.start[c + 1] - lo;
        for (int w = lane; w < nq * p.K; w += 64) {
            const int qi = w / p.K, k = w - qi * p.K;
            const int li = cc[MPC_IDX(w, (size_t)(p.NQ - q0) * p.K)];
            const WideQuery Q = wide_query(p, q0 + qi);
            const bool ok = li >= 0 && li < len;
            const int g = lo + (ok ? li : 0);
            const float2 pj = traj[MPC_IDX(((size_t)Q.b * rows + p.T + Q.t) * p.n + g, ntraj)];
            const float d = pair_dist(Q.qy, Q.qx, pj.x, pj.y, p.l1);
            const int slot = (qi * p.LPQ + c) * p.K + k;
            s_g[MPC_IDX(slot, NL)] = ok ? g : KW_NONE;
            s_d[MPC_IDX(slot, NL)] = ok ? d : INFINITY;
        }
    }
    __syncthreads();
    // ---- 1 ----
    const int grp = lane / p.LPQ, c = lane - grp * p.LPQ;
    const bool owner = grp < nq && c < p.C;
    const int base = (grp * p.LPQ + c) * p.K;
    int h = 0, cg = KW_NONE;
    float cd = INFINITY;
    if (owner) { cd = s_d[MPC_IDX(base, NL)]; cg = s_g[MPC_IDX(base, NL)]; }
    for (int k = 0; k < p.K; ++k) {
        float bd = cd; int bg = cg;
        for (int o = p.LPQ >> 1; o > 0; o >>= 1) {
            const float od = __shfl_xor(bd, o, 64);
            const int og = __shfl_xor(bg, o, 64);
            if (od < bd || (od == bd && og < bg)) { bd = od; bg = og; }
        }
        bg = __shfl(bg, lane - c, 64);           // one answer per query, whatever the comparisons made of a NaN
        if (c == 0 && grp < nq) s_m[MPC_IDX(grp * p.K + k, NM)] = bg;
        if (owner && cg == bg && bg != KW_NONE) {            // (global indices are unique: one owner)
            ++h;
            if (h < p.K) { cd = s_d[MPC_IDX(base + h, NL)]; cg = s_g[MPC_IDX(base + h, NL)]; }
            else { cd = INFINITY; cg = KW_NONE; }
        }
    }
    __syncthreads();
    // ---- 2 ----
    for (int w = lane; w < nq * p.K; w += 64) idx_out[MPC_IDX((size_t)q0 * p.K + w, (size_t)p.NQ * p.K)] = s_m[MPC_IDX(w, NM)];
    // ---- 3 ----
    if (grp >= nq) return;
    const int q = q0 + grp;
    const WideQuery Q = wide_query(p, q);
    const bool has_next = p.want_next && Q.t < p.nb - 1;
    const int ntask = p.T + (has_next ? 1 : 0);
    const float2 *tb = traj + (size_t)Q.b * rows * p.n;
    const float2 *mid = tb + (size_t)(p.T + Q.t) * p.n;
    const int *ml = s_m + grp * p.K;
    for (int v = c; v < ntask; v += p.LPQ) {
        const bool nxt = v >= p.T;
        const float2 *tgt = tb + (size_t)(nxt ? p.T + Q.t + 1 : v) * p.n;      // traj(t_ref[v]), or traj(t_mid[t + 1])
        const bool iwd = p.iwd && !nxt;                                         // focus.py:175: flow_to_next is always the mean
        double sw = 0.0;
        if (iwd) {
            for (int k = 0; k < p.K; ++k) {
                const int g = ml[MPC_IDX(k, p.K)];
                if (g >= p.n) continue;
                sw += wide_iwd_weight(Q.qy, Q.qx, mid[MPC_IDX(g, p.n)], p.l1);
            }
        }
        double sy = 0.0, sx = 0.0;
        for (int k = 0; k < p.K; ++k) {
            const int g = ml[MPC_IDX(k, p.K)];
            if (g >= p.n) continue;
            const float2 pj = mid[MPC_IDX(g, p.n)], a = tgt[MPC_IDX(g, p.n)];
            const double fy = (double)a.x - (double)pj.x, fx = (double)a.y - (double)pj.y;
            if (iwd) {
                // focus.py:158-163: 1 / (d + 1e-9), divided by the sum of the K weights, times the flow
                const double wk = wide_iwd_weight(Q.qy, Q.qx, pj, p.l1) / sw;
                sy += wk * fy; sx += wk * fx;
            } else { sy += fy; sx += fx; }
        }
        const float2 ov = iwd ? make_float2((float)sy, (float)sx) : make_float2((float)(sy / (double)p.K), (float)(sx / (double)p.K));
        if (nxt) flow_next[MPC_IDX((size_t)(Q.b * (p.nb - 1) + Q.t) * p.G + Q.cell, (size_t)p.B * (p.nb - 1) * p.G)] = ov;
        else flow_lut[MPC_IDX((size_t)q * p.T + v, (size_t)p.NQ * p.T)] = ov;
    }
}

// ------------------------------------------------------------------------------------------
// backward over an index list: for every query that has point i among its neighbours, with weight w
// ('mean': 1 / K; 'iwd': the constant weight of the forward, recomputed from traj)
//     dtraj(t_ref[tr])[i] += w g[tr]      dtraj(t_mid[t])[i] -= sum_tr w g[tr]
//     dtraj(t_mid[t + 1])[i] += gn / K    dtraj(t_mid[t])[i] -= gn / K                 (flow_to_next)
// summed as 64-bit integers: every addend is scaled by 2^(shift - ex), 2^ex the power of two above the largest |gradient| (one
// reduction launch finds it), so |addend| < 2^shift and `shift` leaves room for every addend an element can receive.
// ws: [0] the largest |gradient| as float bits (+ padding to 256 B), then int64 acc [B][T + nb][n][2]
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_knn_wide_gmax(const float *__restrict__ glut, size_t n_lut, const float *__restrict__ gnext,
                                                       size_t n_next, unsigned *__restrict__ gmax) {
    // (on the bits: a NaN is larger than every number, fmaxf would drop it)
    unsigned m = 0u;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_lut; i += stride) m = max(m, __float_as_uint(glut[MPC_IDX(i, n_lut)]) & 0x7fffffffu);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_next; i += stride) m = max(m, __float_as_uint(gnext[MPC_IDX(i, n_next)]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    __shared__ unsigned s_wm[4];
    if ((threadIdx.x & 63) == 0) s_wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {                                  // one atomic per workgroup: they all go to one address
        m = max(max(s_wm[0], s_wm[1]), max(s_wm[2], s_wm[3]));
        if (m != 0u) atomicMax(gmax, m);
    }
}

// scale of the fixed-point sums from the largest |gradient| gm (finite, > 0): gm = f * 2^ex, f in [0.5, 1)
__device__ __forceinline__ double wide_fix_scale(float gm, int shift) {
    int ex = 0;
    (void)frexpf(gm, &ex);
    return ldexp(1.0, shift - ex);
}

__global__ __launch_bounds__(256) void k_knn_idx_bwd(const WideParams p, const float2 *__restrict__ traj, const int *__restrict__ idx,
                                                     const float2 *__restrict__ glut, const float2 *__restrict__ gnext,
                                                     const unsigned *__restrict__ gmax, int shift, unsigned long long *__restrict__ acc) {
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (q >= p.NQ) return;
    const float gm = __uint_as_float(*gmax);
    if (!(gm > 0.f) || !(gm < INFINITY)) return;          // nothing to add / not a number: k_knn_wide_finish writes the answer
    const double scale = wide_fix_scale(gm, shift);
    const WideQuery Q = wide_query(p, q);
    const size_t rows = (size_t)(p.T + p.nb);
    [[maybe_unused]] const size_t nacc = (size_t)p.B * rows * p.n * 2;
    const float2 *mid = traj + ((size_t)Q.b * rows + p.T + Q.t) * p.n;
    const int *il = idx + (size_t)q * p.K;
    double sw = 0.0;
    if (p.iwd) {
        for (int k = 0; k < p.K; ++k) {
            const int i = il[MPC_IDX(k, p.K)];
            if ((unsigned)i >= (unsigned)p.n) continue;
            sw += wide_iwd_weight(Q.qy, Q.qx, mid[MPC_IDX(i, p.n)], p.l1);
        }
    }
    const bool has_next = p.want_next && gnext != nullptr && Q.t < p.nb - 1;
    long long ny = 0, nx = 0;                              // flow_to_next: the same addend for every member
    if (has_next) {
        const float2 gn = gnext[MPC_IDX((size_t)(Q.b * (p.nb - 1) + Q.t) * p.G + Q.cell, (size_t)p.B * (p.nb - 1) * p.G)];
        ny = __double2ll_rn((double)gn.x / (double)p.K * scale); nx = __double2ll_rn((double)gn.y / (double)p.K * scale);
    }
    unsigned long long *ab = acc + (size_t)Q.b * rows * p.n * 2;
    for (int k = 0; k < p.K; ++k) {
        const int i = il[MPC_IDX(k, p.K)];
        if ((unsigned)i >= (unsigned)p.n) continue;
        // the member's weight as the forward formed it
        const double wk = p.iwd ? wide_iwd_weight(Q.qy, Q.qx, mid[MPC_IDX(i, p.n)], p.l1) / sw : 1.0 / (double)p.K;
        long long my = -ny, mx = -nx;
        for (int tr = 0; tr < p.T; ++tr) {
            const float2 g = glut[MPC_IDX((size_t)q * p.T + tr, (size_t)p.NQ * p.T)];
            const long long vy = __double2ll_rn(wk * (double)g.x * scale), vx = __double2ll_rn(wk * (double)g.y * scale);
            const size_t e = ((size_t)tr * p.n + i) * 2;
            atomicAdd(&ab[MPC_IDX(e, nacc)], (unsigned long long)vy);
            atomicAdd(&ab[MPC_IDX(e + 1, nacc)], (unsigned long long)vx);
            my -= vy; mx -= vx;
        }
        const size_t e = ((size_t)(p.T + Q.t) * p.n + i) * 2;
        atomicAdd(&ab[MPC_IDX(e, nacc)], (unsigned long long)my);
        atomicAdd(&ab[MPC_IDX(e + 1, nacc)], (unsigned long long)mx);
        if (has_next) {
            atomicAdd(&ab[MPC_IDX(e + (size_t)p.n * 2, nacc)], (unsigned long long)ny);
            atomicAdd(&ab[MPC_IDX(e + (size_t)p.n * 2 + 1, nacc)], (unsigned long long)nx);
        }
    }
}

__global__ __launch_bounds__(256) void k_knn_wide_finish(const long long *__restrict__ acc, const unsigned *__restrict__ gmax, int shift,
                                                         float *__restrict__ grad_traj, size_t count) {
    const float gm = __uint_as_float(*gmax);
    const bool bad = !(gm < INFINITY);                     // an infinite or NaN gradient came in: so does it go out
    const double inv = (gm > 0.f && !bad) ? 1.0 / wide_fix_scale(gm, shift) : 0.0;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride)
        grad_traj[MPC_IDX(i, count)] = bad ? NAN : (float)((double)acc[MPC_IDX(i, count)] * inv);
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
static int wide_check(const char *who, const mpc_shape *s) {
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    if (!(s->n >= s->K && s->K >= 1)) { mpc_set_error("%s: need 1 <= K <= n", who); return MPC_E_SHAPE; }
    if (s->n > KW_MAX_N) { mpc_set_error("%s: more than %d trajectories per sample", who, KW_MAX_N); return MPC_E_UNSUPPORTED; }
    return 0;
}

static WideParams wide_params(const mpc_shape *s) {
    WideParams p;
    memset(&p, 0, sizeof(p));
    p.B = s->B; p.nb = s->nb; p.T = s->T; p.n = s->n; p.hq = s->hq; p.wq = s->wq; p.sp = s->sp; p.K = s->K;
    p.G = s->hq * s->wq; p.NQ = s->B * s->nb * p.G;
    p.l1 = (s->flags & MPC_F_DIST_L1) ? 1 : 0;
    p.iwd = ((s->flags & MPC_F_SCHEME_IWD) && s->K > 1) ? 1 : 0;      // focus.py:145-147: K == 1 is a plain gather
    p.want_next = (s->flags & MPC_F_WANT_NEXT) ? 1 : 0;
    p.off = (float)s->sp / 2.f - 0.5f;
    return p;
}

// bits the sum of every addend of one element of grad_traj may need above one addend's: a reference row takes one addend per
// (bin, query), a mid-time row one of up to T + 1 addends' size per query and one from the bin before it
static int wide_fix_shift(const mpc_shape *s) {
    const int64_t adds = (int64_t)s->nb * s->hq * s->wq * (s->T + 2);
    int bits = 0;
    while (((int64_t)1 << bits) < adds) ++bits;
    return 62 - bits < 40 ? 62 - bits : 40;
}

extern "C" int64_t mpc_knn_wide_workspace_bytes(const mpc_shape *s) {
    MPC_CHECK_ARG(s, MPC_E_NULL, "null argument");
    const int rc = wide_check(__func__, s);
    if (rc) return rc;
    return 256 + mpc_align((int64_t)(s->B > 0 ? s->B : 1) * (s->T + s->nb) * s->n * 2 * (int64_t)sizeof(long long));
}

extern "C" int mpc_knn_merge_fwd(const mpc_shape *s, const float *traj, const int32_t *cand, const int32_t *chunk_start, int32_t num_chunks,
                                 int32_t *idx_out, float *flow_lut, float *flow_next, void *stream) {
    MPC_CHECK_ARG(s && traj && cand && chunk_start && idx_out && flow_lut, MPC_E_NULL, "null argument");
    MPC_CHECK_ARG(!(s->flags & MPC_F_WANT_NEXT) || flow_next, MPC_E_NULL, "flow_next is null");
    int rc = wide_check(__func__, s);
    if (rc) return rc;
    MPC_CHECK_ARG(num_chunks >= 1, MPC_E_SHAPE, "need at least one chunk");
    MPC_CHECK_ARG(num_chunks <= KW_MAX_CHUNKS, MPC_E_UNSUPPORTED, "more than 64 chunks");
    WideParams p = wide_params(s);
    p.C = num_chunks;
    for (int c = 0; c <= num_chunks; ++c) p.start[c] = chunk_start[c];
    MPC_CHECK_ARG(p.start[0] == 0 && p.start[num_chunks] == s->n, MPC_E_SHAPE, "the chunks must cover [0, n)");
    for (int c = 0; c < num_chunks; ++c)
        MPC_CHECK_ARG(p.start[c + 1] - p.start[c] >= s->K && p.start[c + 1] - p.start[c] < 65536, MPC_E_SHAPE, "every chunk must hold K .. 65535 points");
    p.LPQ = 1;
    while (p.LPQ < p.C) p.LPQ <<= 1;
    // as many queries per wavefront as the candidates' (index, distance) pairs and the merged lists leave room for in LDS
    p.QW = 64 / p.LPQ;
    const auto lds_bytes = [&](int qw) { return (size_t)qw * (2 * p.LPQ + 1) * p.K * sizeof(int); };
    while (p.QW > 1 && lds_bytes(p.QW) > KW_LDS_BYTES) p.QW >>= 1;
    MPC_CHECK_ARG(lds_bytes(p.QW) <= KW_LDS_BYTES, MPC_E_UNSUPPORTED, "chunks x K beyond the merge kernel's LDS");
    if (s->B == 0) return 0;
    MPC_LAUNCH(k_knn_merge, dim3(mpc_cdiv(p.NQ, p.QW)), dim3(64), lds_bytes(p.QW), (hipStream_t)stream, p, reinterpret_cast<const float2 *>(traj),
               cand, idx_out, reinterpret_cast<float2 *>(flow_lut), reinterpret_cast<float2 *>(flow_next));
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_knn_idx_bwd(const mpc_shape *s, const float *traj, const int32_t *idx, const float *grad_flow_lut,
                               const float *grad_flow_next, float *grad_traj, void *ws, void *stream) {
    MPC_CHECK_ARG(s && traj && idx && grad_flow_lut && grad_traj && ws, MPC_E_NULL, "null argument");
    int rc = wide_check(__func__, s);
    if (rc) return rc;
    if (s->B == 0) return 0;
    const WideParams p = wide_params(s);
    hipStream_t st = (hipStream_t)stream;
    unsigned *gmax = (unsigned *)ws;
    long long *acc = (long long *)((char *)ws + 256);
    const size_t count = (size_t)s->B * (s->T + s->nb) * s->n * 2;
    if ((rc = mpc_zero_async(ws, 256 + count * sizeof(long long), st))) return rc;
    const bool next = p.want_next && grad_flow_next != nullptr && s->nb > 1;
    const size_t n_lut = (size_t)p.NQ * p.T * 2, n_next = next ? (size_t)s->B * (s->nb - 1) * p.G * 2 : 0;
    const int shift = wide_fix_shift(s);
    const auto blocks = [](size_t items, size_t cap) { const size_t b = (items + 255) / 256; return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b)); };
    MPC_LAUNCH(k_knn_wide_gmax, dim3(blocks(n_lut + n_next, 512)), dim3(256), 0, st, grad_flow_lut, n_lut, grad_flow_next, n_next, gmax);
    MPC_LAUNCH(k_knn_idx_bwd, dim3(mpc_cdiv(p.NQ, 256)), dim3(256), 0, st, p, reinterpret_cast<const float2 *>(traj), idx,
               reinterpret_cast<const float2 *>(grad_flow_lut), reinterpret_cast<const float2 *>(next ? grad_flow_next : nullptr), gmax, shift,
               reinterpret_cast<unsigned long long *>(acc));
    MPC_LAUNCH(k_knn_wide_finish, dim3(blocks(count, 4096)), dim3(256), 0, st, acc, gmax, shift, grad_traj, count);
    MPC_CHECK_LAUNCH();
    return 0;
}

MPC_BOUNDS_UNIT("knn_wide.hip")
