// Per-event part of the CMax loss: LUT warp, event weight, bilinear vote into the Image of
// Warped Events, and its hand-derived backward into the flow look-up table.
//   forward : reference src/losses/focus.py:182-230 + src/utils/event_image_converter.py:333-391
//   backward: SURVEY.md 8a row A11
// Arithmetic follows SURVEY.md Appendix A op for op (fp32, no FMA contraction: this file is
// compiled with -ffp-contract=off).
// Holds the loss path: the atomic cross-check kernels, the LDS-tiled k_ev_bin / k_iwe_accum / k_lut_accum with the stand-alone
// counting pass, and k_event_pos_grad (the vote's adjoint for rows that are warped already).  The event helpers are ev_device.h;
// the per-event basis warp is pe_basis.hip, the (time bin, LUT strip) counting sort ev_order.hip.
#include "pe_device.h"          // (ev_device.h; pe_row_grid)
#include "ev_count_device.h"
#include "knn_device.h"
#include "diag/stamps.h"

// ------------------------------------------------------------------------------------------
// v0: one thread per event, global float atomics (debug / cross-check path, MPC_F_ATOMIC_PATH)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_splat_fwd_atomic(const mpc_shape s,
                                                          const float *__restrict__ events,
                                                          const float *__restrict__ lut,
                                                          const float *__restrict__ t_ref,
                                                          float *__restrict__ iwe) {
    const EvParams p = make_params(s);
    const size_t total = (size_t)p.B * p.M;
    for (size_t row = (size_t)blockIdx.x * 256 + threadIdx.x; row < total; row += (size_t)gridDim.x * 256) {
        const int b = (int)(row / p.M), i = (int)(row - (size_t)b * p.M);
        float e[6];
        load_event(events, row, e);
        const int pol = (p.P == 2 && i >= p.Mp) ? 1 : 0;
        for (int tr = 0; tr < p.T; ++tr) {
            Warped o;
            const float tref = (p.flags & MPC_F_SCALE_BY_DT) ? t_ref[tr] : 0.f;
            if (!warp_event(p, e, b, tr, lut, tref, o)) continue;
            float *img = iwe + ((size_t)(b * p.T + tr) * p.P + pol) * p.H * p.W;
            const float w00 = (1.f - o.fy) * (1.f - o.fx) * o.w;
            const float w10 = o.fy * (1.f - o.fx) * o.w;
            const float w01 = (1.f - o.fy) * o.fx * o.w;
            const float w11 = o.fy * o.fx * o.w;
            const bool yin0 = o.y0 >= 0 && o.y0 < p.H, yin1 = o.y0 + 1 >= 0 && o.y0 + 1 < p.H;
            const bool xin0 = o.x0 >= 0 && o.x0 < p.W, xin1 = o.x0 + 1 >= 0 && o.x0 + 1 < p.W;
            if (yin0 && xin0) atomicAdd(img + (size_t)o.y0 * p.W + o.x0, w00);
            if (yin1 && xin0) atomicAdd(img + (size_t)(o.y0 + 1) * p.W + o.x0, w10);
            if (yin0 && xin1) atomicAdd(img + (size_t)o.y0 * p.W + o.x0 + 1, w01);
            if (yin1 && xin1) atomicAdd(img + (size_t)(o.y0 + 1) * p.W + o.x0 + 1, w11);
        }
    }
}

__global__ __launch_bounds__(256) void k_splat_bwd_atomic(const mpc_shape s,
                                                          const float *__restrict__ events,
                                                          const float *__restrict__ lut,
                                                          const float *__restrict__ t_ref,
                                                          const float *__restrict__ gimg,
                                                          const float *__restrict__ scal,
                                                          const float *__restrict__ grad_out,
                                                          float *__restrict__ glut) {
    const EvParams p = make_params(s);
    const float coef = scal[MPC_SCAL_GCOEF] * (grad_out ? grad_out[0] : 1.f);
    const size_t total = (size_t)p.B * p.M;
    for (size_t row = (size_t)blockIdx.x * 256 + threadIdx.x; row < total; row += (size_t)gridDim.x * 256) {
        const int b = (int)(row / p.M), i = (int)(row - (size_t)b * p.M);
        float e[6];
        load_event(events, row, e);
        const int pol = (p.P == 2 && i >= p.Mp) ? 1 : 0;
        for (int tr = 0; tr < p.T; ++tr) {
            Warped o;
            const float tref = (p.flags & MPC_F_SCALE_BY_DT) ? t_ref[tr] : 0.f;
            if (!warp_event(p, e, b, tr, lut, tref, o)) continue;
            const float *img = gimg + ((size_t)(b * p.T + tr) * p.P + pol) * p.H * p.W;
            float gy, gx;
            event_pos_grad(p, o, img, gy, gx);
            atomicAdd(glut + 2 * (size_t)o.lut, coef * gy);
            atomicAdd(glut + 2 * (size_t)o.lut + 1, coef * gx);
        }
    }
}

// ------------------------------------------------------------------------------------------
// UNPINNED EXTENSION (default off, `FocusLoss.calc_per_event_basis`): gradient of the objective with respect to the WARPED
// POSITION of every event -- what autograd computes for `warped = differences + events[..., :2]` (focus.py:191) through
// create_iwe (event_image_converter.py:333-391).  The rows carry positions that are warped already (MPC_F_NO_WARP): a per-event
// continuous-time warp (the motion basis evaluated at the event's own timestamp, no flow LUT and no KNN -- BASELINE.json's
// north_star; the reference has none, focus.py:182-195 gathers a binned LUT) is formed by the caller in plain torch, whose
// autograd carries grad_pos on to the coefficient grid.  One thread per event row, no atomics.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_event_pos_grad(const mpc_shape s, const float *__restrict__ events,
                                                        const float *__restrict__ t_ref, const float *__restrict__ gimg,
                                                        const float *__restrict__ scal, const float *__restrict__ grad_out,
                                                        float2 *__restrict__ gpos) {
    const EvParams p = make_params(s);
    const float coef = scal[MPC_SCAL_GCOEF] * (grad_out ? grad_out[0] : 1.f);
    const float tref = (p.flags & MPC_F_SCALE_BY_DT) ? t_ref[0] : 0.f;
    const size_t total = (size_t)p.B * p.M;
    for (size_t row = (size_t)blockIdx.x * 256 + threadIdx.x; row < total; row += (size_t)gridDim.x * 256) {
        const int b = (int)(row / p.M), i = (int)(row - (size_t)b * p.M);
        float e[6];
        load_event(events, row, e);
        const int pol = (p.P == 2 && i >= p.Mp) ? 1 : 0;
        Warped o;
        float2 g = make_float2(0.f, 0.f);
        if (warp_event_with(p, e, make_float2(0.f, 0.f), tref, o)) {
            float gy, gx;
            event_pos_grad(p, o, gimg + ((size_t)b * p.P + pol) * p.H * p.W, gy, gx);
            g = make_float2(coef * gy, coef * gx);
        }
        gpos[row] = g;
    }
}

extern "C" int mpc_event_pos_grad(const mpc_shape *s, const float *events, const float *t_ref, const float *grad_iwe,
                                  const float *scal, const float *grad_out, float *grad_pos, void *stream) {
    MPC_CHECK_ARG(s && grad_iwe && scal && grad_pos && (events || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    MPC_CHECK_ARG((s->flags & MPC_F_NO_WARP) && s->T == 1, MPC_E_UNSUPPORTED, "mpc_event_pos_grad takes rows with warped positions (MPC_F_NO_WARP), num_tref == 1");
    MPC_CHECK_ARG(!(s->flags & MPC_F_SCALE_BY_DT) || t_ref, MPC_E_NULL, "t_ref is null");
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    const int64_t total = (int64_t)s->B * s->M;
    if (total == 0) return 0;
    const int grid = pe_row_grid(total);
    MPC_LAUNCH(k_event_pos_grad, dim3(grid), dim3(256), 0, (hipStream_t)stream, *s, events, t_ref, grad_iwe, scal, grad_out,
               reinterpret_cast<float2 *>(grad_pos));
    MPC_CHECK_LAUNCH();
    return 0;
}

// ==========================================================================================
// v1: LDS-tiled path (num_tref == 1)
//
//   forward   k_ev_bin     one pass over the events: warp, weight, and append a 16-byte record to
//                          (a) the bucket of the destination strip(s) of the image it votes into
//                          and (b) the bucket of its (time bin, source LUT strip) for the backward
//             k_iwe_accum  one workgroup per (image, strip): the strip lives in LDS as 64-bit
//                          fixed point (Q33.30), records are voted with ds_add_u64 -- the global
//                          scatter becomes an on-chip accumulate -- and the strip is written once
//                          with plain coalesced stores (no zero-fill, no global atomics)
//   backward  k_lut_accum  one workgroup per (sample, bin, LUT strip): gathers the 4 taps of the
//                          adjoint image per record and accumulates d/dLUT in LDS (Q33.30)
//   capacity  a bucket holds every record that can reach it (all events of a polarity block can vote into one
//             strip; all events of a sample can sit in one (bin, LUT strip)): address space, not traffic -- only the
//             filled part is ever touched -- so no spill path exists and the sums are bitwise reproducible for any
//             event distribution; a concentrated distribution costs a long tail of the busiest workgroup instead
//
// Why fixed point: on gfx950 ds_add_f32 serialises the wave (~193 cycles per instruction) while
// ds_add_u64 takes ~8-12 (profiles/r01_ubench_lds_atomics.txt).  Q33.30 resolves 9.3e-10, finer
// than fp32 accumulation of the same taps, and integer sums are order independent, so the
// image is bitwise reproducible from run to run.
// ==========================================================================================
#define EV_MARKER 0x6d706331   // 'mpc1': backward records of this workspace are valid

struct BinLayout {
    int SR, NS, CSR, NCS, NF, NBk, fcap, bcap, P, exact;
    int *gcount;            // [NF + NBk + 8]
    int *bcapcnt;           // [NBk] rows of the sample in each backward bucket (ev_count_device.h): its capacity; then [NBk] first records
    float4 *frec, *brec;    // bucket storage: frec [NF][fcap] of 12-byte records {y, x, w} (the image is implied by the bucket); brec: 16-byte records
};

struct __attribute__((packed, aligned(4))) rec3 { float y, x, w; };       // forward record (one 12-byte store / load)

__device__ __forceinline__ long long ev_to_fixed_small(float v) {   // |v| < 2; otherwise mpc_to_fixed (common.h)
    return (long long)(int)(v * (float)(1 << MPC_FIX_SHIFT));
}

// Workgroups are dealt round-robin over the 8 XCDs (each with its own L2).  Map physical block p to
// logical block l so that every XCD works on ONE contiguous range of logical blocks: neighbours in
// that range touch the same LUT slices / adjoint-image rows, which then stay in that XCD's L2
// instead of being fetched by all eight (speed only; correct for any placement).
__device__ __forceinline__ int xcd_swizzle(int p, int n) {
    const int per = (n + 7) >> 3;
    return (p & 7) * per + (p >> 3);
}


// one record into slot `slot` of local bucket `lb` (forward buckets first, then backward ones)
__device__ __forceinline__ void ev_emit(const EvParams &p, const BinLayout &L, int b, int nf_loc, int lb, int slot,
                                        float4 rec) {
    if (lb < nf_loc) {
        const int g = (b * p.P + lb / L.NS) * L.NS + (lb % L.NS);
        MPC_EXPECT(g >= 0 && g < L.NF);
        reinterpret_cast<rec3 *>(L.frec)[(size_t)g * L.fcap + MPC_IDX(slot, L.fcap)] = rec3{rec.x, rec.y, rec.z};
    } else {
        // (exact buckets: `slot` counts from the sample's first record -- the bucket starts behind the rows of the buckets
        // before it; else every bucket has room for all the rows of its sample)
        const size_t base = L.exact ? (size_t)b : (size_t)(b * p.nb * L.NCS + (lb - nf_loc));
        MPC_EXPECT((long long)base < (L.exact ? (long long)p.B : (long long)L.NBk));
        L.brec[base * L.bcap + MPC_IDX(slot, L.bcap)] = rec;
    }
}

// grid (ceil(ceil(M / (256*EV_PER_THREAD)) * B / 8) * 8), 256 threads, dynamic LDS = (P*NS + nb*NCS) * 2 ints
__global__ __launch_bounds__(256) void k_ev_bin(const mpc_shape s, const BinLayout L,
                                                const float *__restrict__ events,
                                                const float *__restrict__ lut,
                                                const float *__restrict__ t_ref, int want_bwd,
                                                const int *__restrict__ offsets) {
    extern __shared__ __align__(16) int s_cnt[];          // [nloc] local counts, [nloc] global bases, [nloc+1] local offsets, ids, records
    __shared__ int s_wsum[4];
    const EvParams p = make_params(s);
    const int chunks = (p.M + 256 * EV_PER_THREAD - 1) / (256 * EV_PER_THREAD);
    const int lblk = xcd_swizzle(blockIdx.x, chunks * p.B);
    if (lblk >= chunks * p.B) return;
    const int tid = threadIdx.x, b = lblk / chunks, chunk = lblk - b * chunks;
    // bucket-ordered events (offsets table of ingest / mpc_event_bucket_order): the last entry of a polarity block's table is its
    // first PADDING row -- rows from there to the end of the block are zero rows that vote for nothing: not even read
    int pad0 = p.M, pad1 = p.M, blk1 = p.M;                // [pad0, blk1) and [pad1, M) are padding
    if (offsets != nullptr) {
        const int nk1 = p.nb * L.NCS + 1;
        const int *ob = offsets + (size_t)b * 2 * nk1;
        blk1 = p.Mp;                                        // the two blocks are [0, Mp) and [Mp, M) whatever P is
        pad0 = min(max(ob[nk1 - 1], 0), blk1);
        pad1 = min(max(ob[2 * nk1 - 1], blk1), p.M);
        const int c0 = chunk * EV_PER_THREAD * 256, c1 = min(c0 + EV_PER_THREAD * 256, p.M);
        const bool all_pad = (c0 >= pad0 && c1 <= blk1) || c0 >= pad1;
        if (all_pad) return;                                  // (the marker of the backward records is not this workgroup's to write: ordered events have none)
    }
    const int nf_loc = p.P * L.NS, nb_loc = want_bwd ? p.nb * L.NCS : 0, nloc = nf_loc + nb_loc;
    int *s_base = s_cnt + nloc;
    const int stage_off = ((3 * nloc + 1 + EV_STAGE / 2) + 3) & ~3;     // in ints; 16-byte aligned record area
    for (int i = tid; i < nloc; i += 256) s_cnt[i] = 0;
    __syncthreads();
    const float tref = (p.flags & MPC_F_SCALE_BY_DT) ? t_ref[0] : 0.f;
    const float inv_SR = 1.f / (float)L.SR, inv_CSR = ev_strip_inv(L.CSR);

    float ry[EV_PER_THREAD], rx[EV_PER_THREAD], rw[EV_PER_THREAD];
    int f0[EV_PER_THREAD], f1[EV_PER_THREAD], bk[EV_PER_THREAD];     // local bucket ids (-1: none)
    int r0[EV_PER_THREAD], r1[EV_PER_THREAD], rb[EV_PER_THREAD];     // ranks inside the block
    unsigned aux[EV_PER_THREAD];
    // the rows of a thread are requested together, then their LUT gathers, and only then does the bucket logic
    // (with its branches and LDS atomics) run: two dependent memory round trips per workgroup instead of four
    float ev[EV_PER_THREAD][6];
    Warped wo[EV_PER_THREAD];
    bool live[EV_PER_THREAD];
#pragma unroll
    for (int k = 0; k < EV_PER_THREAD; ++k) {
        const int i = (chunk * EV_PER_THREAD + k) * 256 + tid;
        load_event(events, (size_t)b * p.M + min(i, p.M - 1), ev[k]);
    }
#pragma unroll
    for (int k = 0; k < EV_PER_THREAD; ++k) {
        const int i = (chunk * EV_PER_THREAD + k) * 256 + tid;
        live[k] = warp_event(p, ev[k], b, 0, lut, tref, wo[k]) && (i < p.M) && !((i >= pad0 && i < blk1) || i >= pad1);
    }
#pragma unroll
    for (int k = 0; k < EV_PER_THREAD; ++k) {
        const int i = (chunk * EV_PER_THREAD + k) * 256 + tid;
        f0[k] = f1[k] = bk[k] = -1;
        r0[k] = r1[k] = rb[k] = 0;
        ry[k] = rx[k] = rw[k] = 0.f; aux[k] = 0u;
        if (!live[k]) continue;
        const Warped &o = wo[k];
        const bool xin = (o.x0 + 1 >= 0) && (o.x0 < p.W);
        const bool yin0 = o.y0 >= 0 && o.y0 < p.H, yin1 = o.y0 + 1 >= 0 && o.y0 + 1 < p.H;
        if (!xin || !(yin0 || yin1)) continue;            // no tap inside the image
        const int pol = (p.P == 2 && i >= p.Mp) ? 1 : 0;
        ry[k] = o.y; rx[k] = o.x; rw[k] = o.w;
        // strip = row / SR without an integer division: (row + 0.5) / SR is at least 0.5 / SR away from an
        // integer, far more than the rounding of the float product, so the truncation is exact
        const int s0 = yin0 ? (int)(((float)o.y0 + 0.5f) * inv_SR) : -1, s1 = yin1 ? (int)(((float)o.y0 + 1.5f) * inv_SR) : -1;
        if (s0 >= 0) { f0[k] = pol * L.NS + s0; r0[k] = atomicAdd(&s_cnt[MPC_IDX(f0[k], nf_loc)], 1); }
        if (s1 >= 0 && s1 != s0) { f1[k] = pol * L.NS + s1; r1[k] = atomicAdd(&s_cnt[MPC_IDX(f1[k], nf_loc)], 1); }
        if (want_bwd && o.lut >= 0) {
            const int cst = ev_strip(o.iy, inv_CSR);
            bk[k] = nf_loc + o.it * L.NCS + cst;
            rb[k] = atomicAdd(&s_cnt[MPC_IDX(bk[k], nloc)], 1);
            aux[k] = ((unsigned)pol << 31) | (unsigned)((o.iy - cst * L.CSR) * p.wq + o.ix);
        }
    }
    __syncthreads();
    // reserve the block's slots in the global buckets
    for (int i = tid; i < nloc; i += 256) {
        const int c = s_cnt[i];
        int g;
        int first = 0;            // backward bucket: its first record among the sample's (ev_prefix_block, before this kernel)
        if (i < nf_loc) g = (b * p.P + i / L.NS) * L.NS + (i % L.NS);
        else { g = L.NF + b * p.nb * L.NCS + (i - nf_loc); if (L.exact) first = L.bcapcnt[L.NBk + b * p.nb * L.NCS + (i - nf_loc)]; }
        s_base[i] = (c > 0 ? atomicAdd(&L.gcount[MPC_IDX(g, L.NF + L.NBk)], c) : 0) + first;
    }
    // Local exclusive prefix of the counts: the records are first laid out in LDS bucket by bucket and then
    // written out in that order, so that neighbouring lanes store to neighbouring slots of the same bucket
    // (a 64-lane store touches a few runs of 16-byte records instead of 64 separate cache lines; the kernel
    // was bound by the issue of scattered stores: SQ_WAIT_INST_ANY 46 % of the wave cycles).
    int *s_loc = s_base + nloc;                              // [nloc + 1]
    unsigned short *s_bid = reinterpret_cast<unsigned short *>(s_loc + nloc + 1);     // [EV_STAGE]
    float4 *s_rec = reinterpret_cast<float4 *>(s_cnt + stage_off);                     // [EV_STAGE]
    {   // block_prefix_excl (common.h) written out: through the helper the compiler orders two instructions of this kernel
        // differently, and this kernel's code is held as measured
        const int per = (nloc + 255) >> 8;
        const int i0 = min(tid * per, nloc), i1 = min(i0 + per, nloc);
        int local = 0;
        for (int i = i0; i < i1; ++i) local += s_cnt[i];
        const int incl = wave_scan_incl(local);
        if ((tid & 63) == 63) s_wsum[tid >> 6] = incl;
        __syncthreads();
        int run = incl - local;
        for (int w = 0; w < (tid >> 6); ++w) run += s_wsum[w];
        for (int i = i0; i < i1; ++i) { s_loc[i] = run; run += s_cnt[i]; }
        if (tid == 255) s_loc[nloc] = run;
    }
    __syncthreads();
    const int total = s_loc[nloc];
#pragma unroll
    for (int k = 0; k < EV_PER_THREAD; ++k) {
        if (f0[k] >= 0 || f1[k] >= 0) {
            const int polf = (f0[k] >= 0 ? f0[k] : f1[k]) / L.NS;
            const float4 rec = make_float4(ry[k], rx[k], rw[k], __int_as_float(b * p.P + polf));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int lb = h ? f1[k] : f0[k];
                if (lb < 0) continue;
                const int at = s_loc[lb] + (h ? r1[k] : r0[k]);
                if (at < EV_STAGE) { s_rec[MPC_IDX(at, EV_STAGE)] = rec; s_bid[MPC_IDX(at, EV_STAGE)] = (unsigned short)lb; }
                else ev_emit(p, L, b, nf_loc, lb, s_base[lb] + (h ? r1[k] : r0[k]), rec);
            }
        }
        if (bk[k] >= 0) {
            const float4 rec = make_float4(ry[k], rx[k], rw[k], __uint_as_float(aux[k]));
            const int at = s_loc[bk[k]] + rb[k];
            if (at < EV_STAGE) { s_rec[MPC_IDX(at, EV_STAGE)] = rec; s_bid[MPC_IDX(at, EV_STAGE)] = (unsigned short)bk[k]; }
            else ev_emit(p, L, b, nf_loc, bk[k], s_base[bk[k]] + rb[k], rec);
        }
    }
    __syncthreads();
    for (int r = tid; r < min(total, EV_STAGE); r += 256) {
        const int lb = s_bid[r];
        ev_emit(p, L, b, nf_loc, lb, s_base[MPC_IDX(lb, nloc)] + (r - s_loc[lb]), s_rec[r]);
    }
    if (want_bwd && lblk == 0 && tid == 0) L.gcount[L.NF + L.NBk + 2] = EV_MARKER;
}

// taps of one record restricted to rows [row0, row1): calls f(yy, xx, value)
template <typename F>
__device__ __forceinline__ void record_taps(float y, float x, float w, int H, int W, int row0, int row1, F f) {
    const float y0f = floorf(y + 1e-6f), x0f = floorf(x + 1e-6f);
    const float fy = y - y0f, fx = x - x0f;
    const int y0 = (int)fminf(fmaxf(y0f, -4.f), (float)H + 4.f), x0 = (int)fminf(fmaxf(x0f, -4.f), (float)W + 4.f);
    const bool r0 = y0 >= row0 && y0 < row1, r1 = y0 + 1 >= row0 && y0 + 1 < row1;
    const bool c0 = x0 >= 0 && x0 < W, c1 = x0 + 1 >= 0 && x0 + 1 < W;
    if (r0 && c0) f(y0, x0, (1.f - fy) * (1.f - fx) * w);
    if (r1 && c0) f(y0 + 1, x0, fy * (1.f - fx) * w);
    if (r0 && c1) f(y0, x0 + 1, (1.f - fy) * fx * w);
    if (r1 && c1) f(y0 + 1, x0 + 1, fy * fx * w);
}

// grid NF, 1024 threads, dynamic LDS = SR * W * 8 bytes.  FIXED: the accumulators themselves (Q33.30, int64) are the
// output -- partial images of event shards add up exactly, in any order (mpc_event_splat_fwd_fixed)
template <bool FIXED>
__global__ __launch_bounds__(1024) void k_iwe_accum(const BinLayout L, float *__restrict__ iwe, int H, int W) {
    extern __shared__ unsigned long long s_acc[];
    const int tid = threadIdx.x;
    const int g = blockIdx.x, img = g / L.NS, strip = g - img * L.NS;
    const int row0 = strip * L.SR, row1 = min(row0 + L.SR, H);
    const int npix = (row1 - row0) * W;
    // the count and, without waiting for it, the first four records of every thread are requested ahead of the zeroing and its
    // barrier: one round trip where there were two.  The index is clamped to the bucket's CAPACITY, so the load stays in the
    // bucket's own records; what comes back from beyond the count is uninitialised and is never looked at
    const int n = L.gcount[g];
    const rec3 *rec = reinterpret_cast<const rec3 *>(L.frec) + (size_t)g * L.fcap;
    rec3 e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = rec[MPC_IDX(min(tid + u * 1024, L.fcap - 1), L.fcap)];
    for (int i = tid; i < npix; i += 1024) s_acc[i] = 0ull;
    __syncthreads();
    for (int r0 = tid; r0 < n; r0 += 4 * 1024) {           // four record loads in flight per thread
        if (r0 != tid) {
#pragma unroll
            for (int u = 0; u < 4; ++u) e[u] = rec[min(r0 + u * 1024, n - 1)];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r0 + u * 1024 >= n) continue;
            // |tap| <= (1 + 1e-6)^2 |w|: the one-conversion form is exact below 2, any other weight (create_iwe(weight=
            // tensor), a weighted `valid` column; event_image_converter.py:45-74 accepts any) takes the hi/lo split
            if (fabsf(e[u].w) <= 1.5f)
                record_taps(e[u].y, e[u].x, e[u].w, H, W, row0, row1, [&](int yy, int xx, float v) {
                    atomicAdd(&s_acc[MPC_IDX((yy - row0) * W + xx, npix)], (unsigned long long)ev_to_fixed_small(v));
                });
            else
                record_taps(e[u].y, e[u].x, e[u].w, H, W, row0, row1, [&](int yy, int xx, float v) {
                    atomicAdd(&s_acc[MPC_IDX((yy - row0) * W + xx, npix)], (unsigned long long)mpc_to_fixed(v));
                });
        }
    }
    __syncthreads();
    if (FIXED) {
        long long *dst = reinterpret_cast<long long *>(iwe) + ((size_t)img * H + row0) * W;
        for (int i = tid; i < npix; i += 1024) dst[i] = (long long)s_acc[i];
    } else {
        float *dst = iwe + ((size_t)img * H + row0) * W;
        for (int i = tid; i < npix; i += 1024) dst[i] = mpc_from_fixed((long long)s_acc[i]);
    }
}

__global__ __launch_bounds__(256) void k_iwe_from_fixed(const long long *__restrict__ src, float *__restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = mpc_from_fixed(src[i]);
}

struct __attribute__((packed, aligned(4))) pair4 { float x, y; };

// gradient of one record w.r.t. its warped position from the adjoint image (unscaled)
__device__ __forceinline__ void record_grad(float y, float x, float w, const float *__restrict__ g, int H, int W,
                                            float &gy, float &gx) {
    const float y0f = floorf(y + 1e-6f), x0f = floorf(x + 1e-6f);
    const float fy = y - y0f, fx = x - x0f;
    const int y0 = (int)fminf(fmaxf(y0f, -4.f), (float)H + 4.f), x0 = (int)fminf(fmaxf(x0f, -4.f), (float)W + 4.f);
    const bool r0 = y0 >= 0 && y0 < H, r1 = y0 + 1 >= 0 && y0 + 1 < H;
    const bool c0 = x0 >= 0 && x0 < W, c1 = x0 + 1 >= 0 && x0 + 1 < W;
    // Branch-free: two unconditional 8-byte (4-byte aligned) gathers at clamped coordinates, the taps picked
    // and masked afterwards.  With branches around the loads the compiler could not start the gathers of the
    // four records a thread has in flight together: four dependent L2 round trips instead of one (measured:
    // 13.7 us of the 16.5 us a workgroup of k_lut_accum lives).
    const int xa = min(max(x0, 0), W - 2);
    const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
    const pair4 a = *reinterpret_cast<const pair4 *>(g + MPC_IDX((size_t)ya * W + xa, (long long)H * W - 1));
    const pair4 b = *reinterpret_cast<const pair4 *>(g + MPC_IDX((size_t)yb * W + xa, (long long)H * W - 1));
    const bool lo = (xa == x0);                 // column x0 is the first element of the pair
    const float g00 = (r0 && c0) ? (lo ? a.x : a.y) : 0.f;
    const float g01 = (r0 && c1) ? (lo ? a.y : a.x) : 0.f;
    const float g10 = (r1 && c0) ? (lo ? b.x : b.y) : 0.f;
    const float g11 = (r1 && c1) ? (lo ? b.y : b.x) : 0.f;
    gy = w * ((1.f - fx) * (g10 - g00) + fx * (g11 - g01));
    gx = w * ((1.f - fy) * (g01 - g00) + fy * (g11 - g10));
}

// grid NBk, 512 threads, dynamic LDS = CSR * wq * 2 * 8 bytes.
// glut = grad_out * (GCOEF * sum + add_term): the smoothness gradient is folded in here.
// ORDERED: the events were ordered by mpc_event_bucket_order -- the rows of bucket (bin, LUT strip) of each polarity
// block are contiguous (offsets table) -- so the kernel reads the event rows themselves and redoes the warp instead of
// reading records that the forward would have had to write (section 7 of DESIGN.md).
template <bool ORDERED>
__global__ __launch_bounds__(ORDERED ? EV_LUT_THREADS_ORD : EV_LUT_THREADS, ORDERED ? 1 : EV_LUT_MINWAVES) void k_lut_accum(const mpc_shape s, const BinLayout L,
                                                    const float *__restrict__ gimg,
                                                    const float *__restrict__ scal,
                                                    const float *__restrict__ grad_out,
                                                    float *__restrict__ glut,
                                                    const float *__restrict__ add_term,
                                                    const float *__restrict__ events, const float *__restrict__ lut,
                                                    const float *__restrict__ t_ref, const int *__restrict__ offsets,
                                                    const KnnReachJob job) {
    extern __shared__ unsigned long long s_acc[];
    LA_STAMP_DECL
    constexpr int NT = ORDERED ? EV_LUT_THREADS_ORD : EV_LUT_THREADS, NIF = ORDERED ? EV_LUT_INFLIGHT_ORD : EV_LUT_INFLIGHT;
    constexpr int APF = ORDERED ? 0 : EV_LUT_ADD_PF;      // cells of add_term requested at the top
    const EvParams p = make_params(s);
    const int tid = threadIdx.x;
    // logical order (sample, LUT strip, bin): the bins of one strip read the same adjoint-image rows
    const int lg = xcd_swizzle(blockIdx.x, L.NBk);
    if (lg >= L.NBk) return;
    const int b = lg / (L.NCS * p.nb), rem = lg - b * (L.NCS * p.nb);
    const int cst = rem / p.nb, it = rem - cst * p.nb;
    const int bt = b * p.nb + it;
    const int g = bt * L.NCS + cst;                   // bucket id: (b*nb + it)*NCS + cstrip
    const int crow0 = cst * L.CSR, crow1 = min(crow0 + L.CSR, p.hq);
    const int ncell = (crow1 - crow0) * p.wq;
    const int NK = p.nb * L.NCS, key = it * L.NCS + cst;
    // Record variant: everything the workgroup reads that does not hang on a record is requested HERE -- the marker, the count, the
    // two scalars, this thread's first APF cells of add_term and, without waiting for the count, the first NIF records of every
    // thread -- so that one dependent pair of round trips is left (records -> adjoint taps) where there were four (marker + count
    // -> records -> taps -> scalars + add_term); the reach side job, the zeroing of the strip and its barrier run while these are
    // in flight.  The speculative record index is clamped to the CAPACITY (the count is not here yet): fixed-capacity buckets to
    // the bucket's own bcap records, exact-size ones to the end of the sample's region, so no load leaves the records of the
    // workspace whatever M and the counters hold; what comes back from beyond the count is uninitialised and is replaced by a
    // zero record (polarity 0, cell 0, weight 0) before anything is derived from it.  (The ordered variant keeps its loads where
    // they are used: the same treatment measured no gain there, profiles/event_chains_runs.md.)
    float4 e[NIF];
    float2 addv[APF > 0 ? APF : 1];
    int mark = 0, n = 0;
    float gcoef = 0.f, gout = 1.f;
    const float4 *rec = L.brec;
    int rcap = L.bcap;                                // records from `rec` to the end of the region it points into
    const float2 *add = add_term ? reinterpret_cast<const float2 *>(add_term) + ((size_t)bt * p.hq + crow0) * p.wq : nullptr;
    // (a layout without backward records -- MPC_F_NO_BWD_RECORDS -- has no region to read ahead from)
    const bool spec = !ORDERED && !(p.flags & MPC_F_NO_BWD_RECORDS);
    if (!ORDERED) {
        mark = L.gcount[L.NF + L.NBk + 2];
        n = L.gcount[L.NF + g];
        // the bucket's records: behind those of the sample's buckets before it (first records: ev_prefix_block)
        int first = 0;
        if (L.exact) first = min(max(L.bcapcnt[L.NBk + (size_t)b * NK + key], 0), L.bcap - 1);
        rec = L.brec + (size_t)(L.exact ? b : g) * L.bcap + first;
        rcap = L.bcap - first;
        // (unconditional, so that nothing waits for them here: without a region the four loads read the first counters instead)
        const float4 *src = spec ? rec : reinterpret_cast<const float4 *>(L.gcount);
        const int last = spec ? rcap - 1 : 0;
#pragma unroll
        for (int u = 0; u < NIF; ++u) e[u] = src[MPC_IDX(min(tid + u * NT, last), last + 1)];
        gcoef = scal[MPC_SCAL_GCOEF];
        if (grad_out) gout = grad_out[0];
        if (add && ncell > 0) {
#pragma unroll
            for (int k = 0; k < APF; ++k) addv[k] = add[MPC_IDX(min(tid + k * NT, ncell - 1), ncell)];
        }
    }
    // mpc_focus_bwd: the KNN backward follows on the stream and needs the reach of every 16x16 tile of every (sample, bin); the
    // first workgroup of each (sample, bin) here works it out on the side (knn_device.h) -- this kernel leaves the vector pipes
    // almost idle, and the gather that follows loses two dependent round trips per workgroup (132 -> 117 us at C3)
    if (job.on && cst == 0) {
        if (job.p.l1) knn_reach_slice<true>(job.p, job.tile_dkmax, job.reach, bt, job.gx, job.gy, job.bd, reinterpret_cast<float *>(s_acc));
        else knn_reach_slice<false>(job.p, job.tile_dkmax, job.reach, bt, job.gx, job.gy, job.bd, reinterpret_cast<float *>(s_acc));
        __syncthreads();
    }
    for (int i = tid; i < 2 * ncell; i += NT) s_acc[i] = 0ull;
    // ORDERED: the bucket's strip of the table goes to LDS (coalesced, while the event rows are on their way), so the
    // warp costs no dependent round trip of its own
    float2 *s_lut = reinterpret_cast<float2 *>(s_acc + 2 * ncell);
    if (ORDERED) {
        const float2 *src = reinterpret_cast<const float2 *>(lut) + ((size_t)(b * p.nb + it) * p.hq + crow0) * p.wq;
        for (int i = tid; i < ncell; i += NT) s_lut[i] = src[i];
    }
    __syncthreads();
    LA_STAMP(1);
    const bool valid = ORDERED || mark == EV_MARKER;
    int n_pos = 0, o_pos = 0, o_neg = 0;
    if (ORDERED) {
        const int *ob = offsets + (size_t)b * 2 * (NK + 1);
        // (clamped: a table that does not belong to this tensor must not make the kernel read outside it)
        o_pos = min(max(ob[key], 0), p.M); n_pos = min(max(ob[key + 1] - o_pos, 0), p.M - o_pos);
        o_neg = min(max(ob[NK + 1 + key], 0), p.M);
        n = n_pos + min(max(ob[NK + 1 + key + 1] - o_neg, 0), p.M - o_neg);
    } else if (!valid) n = 0;
    LA_STAMP(2);
    const float tref = (ORDERED && (p.flags & MPC_F_SCALE_BY_DT)) ? t_ref[0] : 0.f;
    // record r of this bucket: from the forward's list, or rebuilt from event row r of the ordered tensor
    auto fetch = [&](int r) -> float4 {
        if (!ORDERED) return rec[MPC_IDX(r, rcap)];
        const int pol = r >= n_pos ? 1 : 0;
        const int row = pol ? o_neg + (r - n_pos) : o_pos + r;
        float e[6];
        load_event(events, (size_t)b * p.M + row, e);
        Warped o;
        warp_cell(p, e, b, 0, o);
        // (an ordered tensor puts every row into the bucket of its own cell; a row that does not belong here -- a
        // foreign tensor passed with offsets -- contributes nothing)
        const bool here = o.it == it && o.iy >= crow0 && o.iy < crow1;
        const int cell = here ? (o.iy - crow0) * p.wq + o.ix : 0;
        const bool mine = warp_event_with(p, e, s_lut[MPC_IDX(cell, ncell)], tref, o) && here;
        const unsigned aux = ((unsigned)((p.P == 2) ? pol : 0) << 31) | (unsigned)cell;
        return make_float4(o.y, o.x, mine ? o.w : 0.f, __uint_as_float(aux));
    };
    // four records per thread in flight: their adjoint-image gathers (the latency of this kernel) overlap
    for (int r0 = tid; r0 < n; r0 += NIF * NT) {
        if (spec && r0 == tid) {                      // first trip: requested at the top; beyond the count: the zero record
#pragma unroll
            for (int u = 0; u < NIF; ++u) if (r0 + u * NT >= n) e[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
#pragma unroll
            for (int u = 0; u < NIF; ++u) e[u] = fetch(min(r0 + u * NT, n - 1));
        }
        LA_STAMP(3);
        float gy[NIF], gx[NIF];
#pragma unroll
        for (int u = 0; u < NIF; ++u) {
            const int pol = (int)(__float_as_uint(e[u].w) >> 31);
            record_grad(e[u].x, e[u].y, e[u].z, gimg + (size_t)(b * p.P + pol) * p.H * p.W, p.H, p.W, gy[u], gx[u]);
        }
        LA_STAMP(4);
#pragma unroll
        for (int u = 0; u < NIF; ++u) {
            if (r0 + u * NT < n && (!ORDERED || e[u].z != 0.f)) {
                const int cell = (int)(__float_as_uint(e[u].w) & 0x7fffffffu);
                atomicAdd(&s_acc[MPC_IDX(2 * cell, 2 * ncell)], (unsigned long long)mpc_to_fixed(gy[u]));
                atomicAdd(&s_acc[MPC_IDX(2 * cell + 1, 2 * ncell)], (unsigned long long)mpc_to_fixed(gx[u]));
            }
        }
    }
    __syncthreads();
    LA_STAMP(5);
    if (ORDERED) { gout = grad_out ? grad_out[0] : 1.f; gcoef = scal[MPC_SCAL_GCOEF]; }
    const float coef = valid ? gcoef * gout : __int_as_float(0x7fc00000);
    float2 *dst = reinterpret_cast<float2 *>(glut) + ((size_t)bt * p.hq + crow0) * p.wq;
    auto put = [&](int i, bool have, float2 o) {
        float2 v = make_float2(coef * mpc_from_fixed((long long)s_acc[2 * i]), coef * mpc_from_fixed((long long)s_acc[2 * i + 1]));
        if (add) { if (!have) o = add[i]; v.x += gout * o.x; v.y += gout * o.y; }
        dst[i] = v;
    };
#pragma unroll
    for (int k = 0; k < APF; ++k) if (tid + k * NT < ncell) put(tid + k * NT, true, addv[k]);
    for (int i = tid + APF * NT; i < ncell; i += NT) put(i, false, make_float2(0.f, 0.f));      // (strips beyond the cells held in registers)
    LA_STAMP_WRITE(tid, dst, n);
}

// the counting pass of ev_count_device.h as a launch of its own (stage entry points; the fused forward lets spare
// workgroups of the KNN strip kernel do it).  grid ev_count_blocks(a), 256 threads, dynamic LDS nb * NCS ints
__global__ __launch_bounds__(256) void k_ev_count(const EvCountArgs a) {
    extern __shared__ int s_ec[];
    ev_count_block(a, blockIdx.x, s_ec);
}
// grid B, 256 threads
__global__ __launch_bounds__(256) void k_ev_prefix(const EvCountArgs a) {
    __shared__ int s_tmp[4];
    ev_prefix_block(a, blockIdx.x, s_tmp);
}

static BinLayout bin_layout(const mpc_shape *s, const mpc_ws_layout &L, void *ws) {
    BinLayout B;
    B.SR = L.strip_rows; B.NS = L.n_strips; B.CSR = L.cstrip_rows; B.NCS = L.n_cstrips;
    B.NF = L.nfb; B.NBk = L.nbb; B.fcap = L.fcap; B.bcap = L.bcap; B.P = L.P; B.exact = L.b_exact;
    B.gcount = (int *)((char *)ws + L.off_fcount);
    B.bcapcnt = B.gcount + L.nfb + L.nbb + 8;
    B.frec = (float4 *)((char *)ws + L.off_frec);
    B.brec = (float4 *)((char *)ws + L.off_brec);
    return B;
}

// what the counting pass needs (null events: nothing to count -- no tiled path, no backward records wanted)
EvCountArgs mpc_event_count_args(const mpc_shape *s, const float *events, void *ws) {
    EvCountArgs a{};
    const mpc_ws_layout L = mpc_layout(s);
    const bool tiled = !(s->flags & MPC_F_ATOMIC_PATH) && s->T == 1 && L.strip_rows > 0 && L.cstrip_rows > 0;
    if (!tiled || !L.b_exact || (s->flags & (MPC_F_NO_WARP | MPC_F_NO_BWD_RECORDS)) || s->B <= 0 || s->M <= 0 || !events) return a;
    a.events = events;
    a.cap = (int *)((char *)ws + L.off_fcount) + L.nfb + L.nbb + 8;
    a.B = s->B; a.M = s->M; a.nb = s->nb; a.sp = s->sp; a.hq = s->hq; a.CSR = L.cstrip_rows; a.NCS = L.n_cstrips;
    return a;
}

static bool use_tiled(const mpc_shape *s, const mpc_ws_layout &L) { return !(s->flags & MPC_F_ATOMIC_PATH) && s->T == 1 && L.strip_rows > 0 && L.cstrip_rows > 0; }

// ------------------------------------------------------------------------------------------
// host entry points
// ------------------------------------------------------------------------------------------
extern "C" int mpc_event_splat_fwd(const mpc_shape *s, const float *events, const float *flow_lut,
                                   const float *t_ref, float *iwe_raw, void *ws, void *stream) {
    return mpc_event_splat_fwd_ex(s, events, flow_lut, t_ref, iwe_raw, ws, stream, 0, nullptr);
}

static int splat_fwd_impl(const mpc_shape *s, const float *events, const float *flow_lut, const float *t_ref,
                          float *iwe_raw, void *ws, void *stream, int counters_zeroed, bool fixed, const int32_t *offsets = nullptr);

// Event-axis sharding ("optional finer split" for batches smaller than the number of ranks): the raw IWE of
// THIS rank's events as the Q33.30 accumulators themselves; integer partial images sum exactly, so an all-reduce(SUM) of
// them followed by mpc_iwe_from_fixed gives, bit for bit, the image a single rank computes from all the events.
extern "C" int mpc_event_splat_fwd_fixed(const mpc_shape *s, const float *events, const float *flow_lut, const float *t_ref,
                                         int64_t *iwe_fixed, void *ws, void *stream) {
    MPC_CHECK_ARG(s && iwe_fixed && ws, MPC_E_NULL, "null argument");
    MPC_CHECK_ARG(!(s->flags & MPC_F_ATOMIC_PATH) && s->T == 1, MPC_E_UNSUPPORTED, "fixed-point images come from the LDS-tiled path (num_tref == 1)");
    return splat_fwd_impl(s, events, flow_lut, t_ref, reinterpret_cast<float *>(iwe_fixed), ws, stream, 0, true);
}

extern "C" int mpc_iwe_from_fixed(const int64_t *iwe_fixed, float *iwe_raw, int64_t count, void *stream) {
    MPC_CHECK_ARG((iwe_fixed && iwe_raw) || count == 0, MPC_E_NULL, "null argument");
    if (count <= 0) return 0;
    const int64_t blocks = (count + 255) / 256 < 8192 ? (count + 255) / 256 : 8192;
    MPC_LAUNCH(k_iwe_from_fixed, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const long long *>(iwe_fixed), iwe_raw, (size_t)count);
    MPC_CHECK_LAUNCH();
    return 0;
}

int mpc_event_splat_fwd_ex(const mpc_shape *s, const float *events, const float *flow_lut, const float *t_ref,
                           float *iwe_raw, void *ws, void *stream, int counters_zeroed, const int32_t *offsets) {
    return splat_fwd_impl(s, events, flow_lut, t_ref, iwe_raw, ws, stream, counters_zeroed, false, offsets);
}

static int splat_fwd_impl(const mpc_shape *s, const float *events, const float *flow_lut, const float *t_ref,
                          float *iwe_raw, void *ws, void *stream, int counters_zeroed, bool fixed, const int32_t *offsets) {
    MPC_CHECK_ARG(s && iwe_raw && ws && (events || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    MPC_CHECK_ARG((s->flags & MPC_F_NO_WARP) || flow_lut, MPC_E_NULL, "flow_lut is null");
    MPC_CHECK_ARG(!(s->flags & MPC_F_SCALE_BY_DT) || t_ref, MPC_E_NULL, "t_ref is null");
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    const mpc_ws_layout L = mpc_layout(s);
    hipStream_t st = (hipStream_t)stream;
    if (use_tiled(s, L)) {
        static mpc_device_once attr_once;   // raising the dynamic-LDS cap: idempotent, once per device
        if ((rc = mpc_raise_lds_cap(attr_once, __func__, 160 * 1024 - 512, {(const void *)k_iwe_accum<false>, (const void *)k_iwe_accum<true>,
                                                                            (const void *)k_lut_accum<false>, (const void *)k_lut_accum<true>})))
            return rc;
        const BinLayout BL = bin_layout(s, L, ws);
        const int want_bwd = (s->flags & (MPC_F_NO_WARP | MPC_F_NO_BWD_RECORDS)) ? 0 : 1;
        // counters_zeroed: bit 0 = the counters were zeroed, bit 1 = the backward capacities were counted (mpc_focus_fwd: by the
        // KNN forward's kernels)
        if (!(counters_zeroed & 1) && (rc = mpc_zero_async(BL.gcount, (size_t)(L.nfb + 2 * L.nbb + 8) * sizeof(int), st))) return rc;
        if (s->B > 0 && s->M > 0) {
            const int nblk = mpc_cdiv(s->M, 256 * EV_PER_THREAD) * s->B;
            const dim3 grid(((nblk + 7) / 8) * 8);
            if (want_bwd && L.b_exact && !(counters_zeroed & 2)) {
                const EvCountArgs ca = mpc_event_count_args(s, events, ws);
                MPC_LAUNCH(k_ev_count, dim3(ev_count_blocks(ca)), dim3(256), (size_t)s->nb * L.n_cstrips * sizeof(int), st, ca);
                MPC_LAUNCH(k_ev_prefix, dim3(s->B), dim3(256), 0, st, ca);
                MPC_CHECK_LAUNCH();
            }
            const int nloc = L.P * L.n_strips + s->nb * L.n_cstrips;
            const size_t lds = (size_t)(((3 * nloc + 1 + EV_STAGE / 2) + 3) & ~3) * sizeof(int) + (size_t)EV_STAGE * 16;
            MPC_LAUNCH(k_ev_bin, grid, dim3(256), lds, st, *s, BL, events, flow_lut, t_ref, want_bwd, want_bwd ? nullptr : offsets);
            MPC_CHECK_LAUNCH();
        }
        if (L.nfb > 0) {
            if (fixed) MPC_LAUNCH(k_iwe_accum<true>, dim3(L.nfb), dim3(1024), (size_t)L.strip_rows * s->W * 8, st, BL, iwe_raw, s->H, s->W);
            else MPC_LAUNCH(k_iwe_accum<false>, dim3(L.nfb), dim3(1024), (size_t)L.strip_rows * s->W * 8, st, BL, iwe_raw, s->H, s->W);
            MPC_CHECK_LAUNCH();
        }
        return 0;
    }
    MPC_CHECK_ARG(!fixed, MPC_E_UNSUPPORTED, "fixed-point images need the LDS-tiled path");
    const size_t img_bytes = (size_t)L.nimg * s->H * s->W * sizeof(float);
    const int e = mpc_zero_async(iwe_raw, img_bytes, st);
    if (e) return e;
    const int64_t total = (int64_t)s->B * s->M;
    if (total == 0) return 0;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    MPC_LAUNCH(k_splat_fwd_atomic, dim3(grid), dim3(256), 0, st, *s, events, flow_lut, t_ref, iwe_raw);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_event_splat_bwd(const mpc_shape *s, const float *events, const float *flow_lut,
                                   const float *t_ref, const float *grad_iwe, const float *scal,
                                   const float *grad_out, float *grad_flow_lut, const float *add_term,
                                   void *ws, void *stream) {
    return mpc_event_splat_bwd_ordered(s, events, nullptr, flow_lut, t_ref, grad_iwe, scal, grad_out, grad_flow_lut, add_term, ws, stream);
}

extern "C" int mpc_event_splat_bwd_ordered(const mpc_shape *s, const float *events, const int32_t *offsets, const float *flow_lut,
                                           const float *t_ref, const float *grad_iwe, const float *scal,
                                           const float *grad_out, float *grad_flow_lut, const float *add_term,
                                           void *ws, void *stream) {
    return mpc_event_splat_bwd_job(s, events, offsets, flow_lut, t_ref, grad_iwe, scal, grad_out, grad_flow_lut, add_term, ws, stream, nullptr, nullptr);
}

// knn_state != nullptr (mpc_focus_bwd): k_lut_accum also computes the tile reaches of the KNN backward that follows; *reach_done
// tells the caller whether it did
int mpc_event_splat_bwd_job(const mpc_shape *s, const float *events, const int32_t *offsets, const float *flow_lut,
                            const float *t_ref, const float *grad_iwe, const float *scal,
                            const float *grad_out, float *grad_flow_lut, const float *add_term,
                            void *ws, void *stream, const float *knn_state, int *reach_done) {
    if (reach_done) *reach_done = 0;
    MPC_CHECK_ARG(s && flow_lut && grad_iwe && scal && grad_flow_lut && ws && (events || s->M == 0 || s->B == 0), MPC_E_NULL, "null argument");
    MPC_CHECK_ARG(!(s->flags & MPC_F_NO_WARP), MPC_E_UNSUPPORTED, "no LUT to differentiate with MPC_F_NO_WARP");
    MPC_CHECK_ARG(!(s->flags & MPC_F_SCALE_BY_DT) || t_ref, MPC_E_NULL, "t_ref is null");
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const mpc_ws_layout L = mpc_layout(s);
    if (use_tiled(s, L)) {
        const BinLayout BL = bin_layout(s, L, ws);
        // the records must come from mpc_event_splat_fwd on this same workspace: the kernel checks
        // the marker that call left behind and poisons the output with NaN if it is missing
        if (L.nbb > 0) {
            MPC_CHECK_ARG(!offsets || (size_t)L.cstrip_rows * s->wq * 24 <= 160 * 1024 - 512, MPC_E_UNSUPPORTED,
                          "LUT too wide for the ordered backward (use mpc_event_splat_bwd)");
            KnnReachJob job{};
            const size_t lds_acc = (size_t)L.cstrip_rows * s->wq * (offsets ? 24 : 16);
            if (knn_state && mpc_knn_reach_job(s, knn_state, ws, &job) &&
                ((size_t)job.gx * job.gy * (KNN_NCLS + 1) + 16) * sizeof(float) > lds_acc) job.on = 0;      // (does not fit this kernel's LDS)
            if (offsets)
                MPC_LAUNCH(k_lut_accum<true>, dim3(((L.nbb + 7) / 8) * 8), dim3(EV_LUT_THREADS_ORD), lds_acc, st, *s, BL,
                                   grad_iwe, scal, grad_out, grad_flow_lut, add_term, events, flow_lut, t_ref, offsets, job);
            else
                MPC_LAUNCH(k_lut_accum<false>, dim3(((L.nbb + 7) / 8) * 8), dim3(EV_LUT_THREADS), lds_acc, st, *s, BL,
                                   grad_iwe, scal, grad_out, grad_flow_lut, add_term, events, flow_lut, t_ref, offsets, job);
            MPC_CHECK_LAUNCH();
            if (reach_done) *reach_done = job.on;
        }
        return 0;
    }
    {
        const int64_t cnt = (int64_t)s->B * s->nb * s->hq * s->wq * s->T * 2;
        if (add_term) {
            rc = grad_out ? mpc_scale(add_term, grad_out, grad_flow_lut, cnt, stream) : (int)hipMemcpyAsync(grad_flow_lut, add_term, cnt * sizeof(float), hipMemcpyDeviceToDevice, st);
            if (rc) return rc;
        } else {
            const int e = mpc_zero_async(grad_flow_lut, cnt * sizeof(float), st);
            if (e) return e;
        }
    }
    const int64_t total = (int64_t)s->B * s->M;
    if (total == 0) return 0;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    MPC_LAUNCH(k_splat_bwd_atomic, dim3(grid), dim3(256), 0, st, *s, events, flow_lut, t_ref,
                       grad_iwe, scal, grad_out, grad_flow_lut);
    MPC_CHECK_LAUNCH();
    return 0;
}


MPC_BOUNDS_UNIT("events.hip")
