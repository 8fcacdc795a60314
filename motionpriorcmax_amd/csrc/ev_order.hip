// The (time bin, LUT strip) counting sort of the event rows, and its two scans for the ingest kernels that count while they write.
#include "ev_device.h"
#include "bounds.h"

// ==========================================================================================
// f-1, layout half (reference loader.py:360-415 builds the padded tensor in time order): order the rows of
// every polarity block by (time bin, LUT strip) -- the key of the BACKWARD buckets, which does not depend on the flow.
// Permuting rows inside a polarity block does not change the loss (bit for bit: the accumulators are integers), so the
// ordered tensor is a valid `events` for the reference too; with its offsets table the forward need not write, and the
// backward not read back, a 16-byte record per event.  Padding rows (valid == 0) keep their place at the end of their block.
//   offsets [B][2][nb*NCS + 1]: first row of every (bin, LUT strip) inside the block; [nb*NCS] = first padding row
// Counting sort: per-chunk counts -> scan over the chunks of every key -> scan over the keys -> scatter (the order inside a
// bucket is not defined and need not be).
// ==========================================================================================
#define EVO_ROWS 2048          // rows of one chunk (256 threads x 8)

__device__ __forceinline__ int evo_key(const EvParams &p, const EvKey &k, const float e[6]) {
    if (e[5] == 0.f && !(p.flags & MPC_F_UNIT_WEIGHT)) return k.NK;   // padding row (weight 0: it votes for nothing)
    return ev_key(k, p.nb, (int)e[4], e[0]);
}

// grid (chunks, 2 * B): counts[b][pol][key][chunk] (ev_key_device.h)
__global__ __launch_bounds__(256) void k_evo_count(const mpc_shape s, const EvKey k, const float *__restrict__ events,
                                                   int *__restrict__ counts, int chunks) {
    extern __shared__ int s_c[];
    const EvParams p = make_params(s);
    const int b = blockIdx.y >> 1, pol = blockIdx.y & 1, chunk = blockIdx.x;
    const int r0 = pol ? p.Mp : 0, r1 = pol ? p.M : p.Mp;
    for (int i = threadIdx.x; i <= k.NK; i += 256) s_c[i] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < EVO_ROWS; j += 256) {
        const int row = r0 + chunk * EVO_ROWS + j;
        if (row >= r1) break;
        float e[6];
        load_event(events, (size_t)b * p.M + row, e);
        atomicAdd(&s_c[evo_key(p, k, e)], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= k.NK; i += 256) counts[evo_count_at(k, chunks, b, pol, i, chunk)] = s_c[i];
}

// Step 1, grid (ceil((NK + 1) / 4), 2 * B), 256 threads: one wavefront per key scans its chunks (lanes = chunks; in place ->
// the chunk's first row inside the key) and leaves the key's total.
__global__ __launch_bounds__(256) void k_evo_scan_chunks(const EvKey k, int *__restrict__ counts, int *__restrict__ totals, int chunks) {
    const int lane = threadIdx.x & 63, key = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (key > k.NK) return;
    int *ci = counts + evo_count_at(k, chunks, blockIdx.y >> 1, blockIdx.y & 1, key, 0);
    int run = 0;
    for (int c0 = 0; c0 < chunks; c0 += 64) {
        const int ch = c0 + lane;
        const int v = ch < chunks ? ci[ch] : 0;
        const int incl = wave_scan_incl(v);
        if (ch < chunks) ci[ch] = run + incl - v;
        run += __shfl(incl, 63);
    }
    if (lane == 0) totals[(size_t)blockIdx.y * (k.NK + 1) + key] = run;
}

// Step 2, grid 2 * B, 256 threads: exclusive scan of the NK + 1 key totals of a polarity block -> offsets
__global__ __launch_bounds__(256) void k_evo_scan_keys(const mpc_shape s, const EvKey k, const int *__restrict__ totals,
                                                       int *__restrict__ offsets) {
    __shared__ int s_wsum[4];
    const size_t o = (size_t)blockIdx.x * (k.NK + 1);
    block_prefix_excl(totals + o, offsets + o, k.NK + 1, s_wsum, (blockIdx.x & 1) ? s.Mp : 0);
}

// grid (chunks, 2 * B)
__global__ __launch_bounds__(256) void k_evo_scatter(const mpc_shape s, const EvKey k, const float *__restrict__ events,
                                                     const int *__restrict__ counts, const int *__restrict__ offsets,
                                                     float *__restrict__ out, int chunks) {
    extern __shared__ int s_c[];
    const EvParams p = make_params(s);
    const int b = blockIdx.y >> 1, pol = blockIdx.y & 1, chunk = blockIdx.x;
    const int r0 = pol ? p.Mp : 0, r1 = pol ? p.M : p.Mp;
    const int *ob = offsets + (size_t)(b * 2 + pol) * (k.NK + 1);
    for (int i = threadIdx.x; i <= k.NK; i += 256) s_c[i] = ob[i] + counts[evo_count_at(k, chunks, b, pol, i, chunk)];   // first destination row of the chunk's share
    __syncthreads();
    for (int j = threadIdx.x; j < EVO_ROWS; j += 256) {
        const int row = r0 + chunk * EVO_ROWS + j;
        if (row >= r1) break;
        float e[6];
        load_event(events, (size_t)b * p.M + row, e);
        const int dst = atomicAdd(&s_c[evo_key(p, k, e)], 1);
        float2 *d = reinterpret_cast<float2 *>(out + ((size_t)b * p.M + dst) * 6);
        d[0] = make_float2(e[0], e[1]); d[1] = make_float2(e[2], e[3]); d[2] = make_float2(e[4], e[5]);
    }
}

// the two scans of the counting sort, for a counts array someone filled (mpc_event_bucket_order below, ingest.hip)
int mpc_evo_scans(const mpc_shape *s, const EvKey &k, const EvoWs &w, int32_t *offsets, hipStream_t st) {
    MPC_LAUNCH(k_evo_scan_chunks, dim3(mpc_cdiv(w.nk1, 4), 2 * s->B), dim3(256), 0, st, k, w.counts, w.totals, w.chunks);
    MPC_LAUNCH(k_evo_scan_keys, dim3(2 * s->B), dim3(256), 0, st, *s, k, w.totals, (int *)offsets);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t mpc_event_lut_strips(const mpc_shape *s) {
    if (!s || mpc_validate_shape(s)) return MPC_E_SHAPE;
    return mpc_layout(s).n_cstrips;
}

extern "C" int64_t mpc_event_order_workspace_bytes(const mpc_shape *s) {
    if (!s || mpc_validate_shape(s)) return MPC_E_SHAPE;
    return evo_ws(s->B, s->nb * mpc_layout(s).n_cstrips, mpc_cdiv(s->M > 0 ? s->M : 1, EVO_ROWS), nullptr).bytes;
}

extern "C" int mpc_event_bucket_order(const mpc_shape *s, const float *events_in, float *events_out, int32_t *offsets,
                                      void *ws, void *stream) {
    MPC_CHECK_ARG(s && ws && ((events_in && events_out) || s->M == 0 || s->B == 0) && (offsets || s->B == 0), MPC_E_NULL, "null argument");
    int rc = mpc_validate_shape(s);
    if (rc) return rc;
    const mpc_ws_layout L = mpc_layout(s);
    MPC_CHECK_ARG(L.n_cstrips > 0, MPC_E_UNSUPPORTED, "no LDS-tiled event path for this shape (num_tref > 1 or the atomic debugging path)");
    if (s->B == 0) return 0;
    const EvKey k{L.n_cstrips, L.cstrip_rows, s->nb * L.n_cstrips, s->sp, s->hq};
    // no rows: every bucket is empty and starts at row 0
    if (s->M == 0) return mpc_zero_async(offsets, (size_t)s->B * 2 * (k.NK + 1) * sizeof(int32_t), (hipStream_t)stream);
    MPC_CHECK_ARG(events_in != events_out, MPC_E_SHAPE, "in-place ordering is not supported");
    const EvoWs w = evo_ws(s->B, k.NK, mpc_cdiv(s->M, EVO_ROWS), ws);       // chunks of the longer block at most; chunks beyond a block's rows are empty
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)w.nk1 * 4;
    MPC_LAUNCH(k_evo_count, dim3(w.chunks, 2 * s->B), dim3(256), lds, st, *s, k, events_in, w.counts, w.chunks);
    if ((rc = mpc_evo_scans(s, k, w, offsets, st))) return rc;
    MPC_LAUNCH(k_evo_scatter, dim3(w.chunks, 2 * s->B), dim3(256), lds, st, *s, k, events_in, w.counts, (const int *)offsets,
                       events_out, w.chunks);
    MPC_CHECK_LAUNCH();
    return 0;
}

MPC_BOUNDS_UNIT("ev_order.hip")
