// The bucket key of an event -- (time bin, LUT strip) of its OWN LUT cell (focus.py:184-191: it = int(bin), iy = int(y // sp),
// ix = int(x // sp)) -- and the workspace of the counting sort that orders the rows by it.  The key is the contract between the
// forward and the backward of the event path: the forward's backward records (k_ev_bin), the exact-size bucket capacities
// (ev_count_device.h), the `offsets` table of bucket-ordered events (mpc_event_bucket_order, ingest) and the ordered accumulate
// kernels all file an event under it, and they agree bit for bit because this is the only place that computes it.
#pragma once
#include "common.h"

// constants of the key: NCS strips of CSR cell rows each, NK = nb * NCS keys (key NK itself: the padding rows), sp, hq of the loss
struct EvKey { int NCS, CSR, NK, sp, hq; };

// Cell rows below this bound are filed under the strip that integer division gives them (ev_strip, below).  The library accepts
// taller LUTs (mpc_validate_shape bounds B * nb * hq * wq * T by 2^30, so hq can reach 2^30 - 1 with wq = 1), and for those
// the buckets of the rows beyond the bound are still consistent between every user -- they all call ev_strip -- but a row may
// sit one strip beside row / CSR, which the ordered accumulate kernels (strip = rows [cst * CSR, (cst + 1) * CSR)) do not expect.
#define EV_KEY_EXACT_ROWS (1 << 22)

// ---- the ordering sort's workspace -------------------------------------------------------------------------------------
// counts [b][pol][key][chunk] (key 0 .. NK; the counting kernels fill it, the scans turn it in place into the chunk's first row
// inside the key), then totals [b][pol][key]
struct EvoWs { int nk1, chunks; int *counts, *totals; int64_t bytes; };          // nk1: keys with the padding key
static inline EvoWs evo_ws(int B, int NK, int chunks, void *ws) {
    const int64_t n = (int64_t)2 * (B > 0 ? B : 1) * (NK + 1);
    return EvoWs{NK + 1, chunks, (int *)ws, ws ? (int *)ws + n * chunks : nullptr, mpc_align(n * (chunks + 1) * 4)};          // (ws null: the size alone)
}
__host__ __device__ static inline size_t evo_count_at(const EvKey &k, int chunks, int b, int pol, int key, int chunk) {
    return ((size_t)(b * 2 + pol) * (k.NK + 1) + key) * chunks + chunk;
}
// the two scans of the counting sort over a filled counts array -> offsets [B][2][NK + 1] (ev_order.hip)
int mpc_evo_scans(const mpc_shape *s, const EvKey &k, const EvoWs &w, int32_t *offsets, hipStream_t st);

#ifdef __HIPCC__
// torch indexing would raise on out-of-range indices; clamp instead of faulting: the time bin among nb, a cell row among hq ...
__device__ __forceinline__ int ev_clamp(int i, int n) { return min(max(i, 0), n - 1); }
// cell row (column) of the position v = y (x), before and after the clamp to n = hq (wq).  (The hot kernels convert all the
// indices of a row first and clamp them afterwards: the order their instruction schedules were measured with.)
__device__ __forceinline__ int ev_cell_raw(float v, int sp) { return (int)floorf(mpc_div_sp(v, sp)); }
__device__ __forceinline__ int ev_cell(float v, int sp, int n) { return ev_clamp(ev_cell_raw(v, sp), n); }

// Strip of cell row iy = iy / CSR without an integer division: inv_CSR = ev_strip_inv(CSR), hoisted by the caller.
// Exact for 0 <= iy < EV_KEY_EXACT_ROWS and ANY CSR >= 1 (CSR < 2^24: exact as a float): iy + 0.5 is exact below 2^23; the
// reciprocal and the product are each correctly rounded (relative error <= u = 2^-24), so the result is (iy + 0.5) / CSR *
// (1 + d) with |d| <= 2u + u^2.  The true quotient lies at least 0.5 / CSR from an integer, and the error (iy + 0.5) / CSR *
// |d| stays below that as long as (iy + 0.5) * (2^-23 + 2^-48) < 0.5, i.e. iy <= 2^22 - 1: the truncation cannot cross.
// The bound is tight to 0.2 %: among CSR 1 .. 4096 the first row filed one strip too high is 4 201 469 at CSR 4095
// (tests/test_event_key_host.py walks every row below the bound for every CSR 1 .. 4096, and that row).
__device__ __forceinline__ float ev_strip_inv(int CSR) { return 1.f / (float)CSR; }
__device__ __forceinline__ int ev_strip(int iy, float inv_CSR) { return (int)(((float)iy + 0.5f) * inv_CSR); }

// key of a row with time bin `it` (unclamped) at height y
__device__ __forceinline__ int ev_key(const EvKey &k, int nb, int it, float y) {
    return ev_clamp(it, nb) * k.NCS + ev_strip(ev_cell(y, k.sp, k.hq), ev_strip_inv(k.CSR));
}
#endif
