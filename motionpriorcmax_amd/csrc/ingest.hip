// Event ingest: raw window (x, y, t_us, p per event, ragged batch) -> the padded
// [B][M][6] event tensor the loss consumes, built on the GPU.
//   per-sample half : reference src/loader/dsec/loader.py:152-167 (time normalisation by min/max in
//                     float64, bin = clip(searchsorted(linspace(0,1,nb+1), t) - 1, 0), in-image filter,
//                     positive / negative split, cast to float32)
//   collate half    : loader.py:360-415 (pad_events + sequence_collate_fn: zero rows with valid = 0,
//                     positive block padded to the batch maximum, then the negative block)
// Three passes: per-chunk counts and time extrema -> per-sample scan (chunk offsets, totals, batch
// maxima) -> stable scatter (order inside each block is the input order, as boolean masking gives).
// The caller reads the two batch maxima to size the output (the only host round trip of ingest).
#include "ev_key_device.h"
#include "bounds.h"
#include <type_traits>

#define ING_CHUNK 1024          // events per workgroup (256 threads x 4 consecutive events)

struct IngLayout {
    int nchunks;
    int *chunk_cnt;             // [B][nchunks][2]  valid positives / negatives per chunk
    long long *chunk_t;         // [B][nchunks][2]  min / max timestamp per chunk
    int *chunk_off;             // [B][nchunks][2]  exclusive offsets
    long long *tminmax;         // [B][2]
    int *totals;                // [B][2]
};

__device__ __forceinline__ int classify(float x, float y, float p, int H, int W) {
    // 1: positive row, 2: negative row, 0: dropped   (loader.py:160-165; comparisons on the float32 values)
    const bool in = (0.f <= y) && (y < (float)H) && (0.f <= x) && (x < (float)W);
    if (!in) return 0;
    return p == 1.f ? 1 : (p == 0.f ? 2 : 0);
}

// four consecutive values of one array: 16-byte loads (one for a 4-byte type, two for an 8-byte one) where the sample's first
// event is 16-byte aligned (vec: N a multiple of 4 and an aligned base pointer) and all four exist, else element by element
__device__ __forceinline__ void ing_vec4(const float *a, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4 *>(a);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void ing_vec4(const int *a, int (&v)[4]) {
    const int4 q = *reinterpret_cast<const int4 *>(a);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ __forceinline__ void ing_vec4(const long long *a, long long (&v)[4]) {
    const longlong2 q0 = *reinterpret_cast<const longlong2 *>(a), q1 = *reinterpret_cast<const longlong2 *>(a + 2);
    v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y;
}
template <typename T>
__device__ __forceinline__ void ing_quad(const T *__restrict__ a, size_t base, int i0, int n, int vec, T fill, T (&v)[4]) {
    if (vec && i0 + 3 < n) {
        ing_vec4(a + base + i0, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? a[base + i0 + k] : fill;
    }
}

// the four consecutive events of a thread (XY: float or int coordinates, PT: float or long long polarity)
template <typename XY, typename PT> struct IngQuadT { XY x[4], y[4]; PT p[4]; long long t[4]; };
typedef IngQuadT<float, float> IngQuad;
template <typename XY, typename PT>
__device__ __forceinline__ IngQuadT<XY, PT> ing_load4(const XY *__restrict__ x, const XY *__restrict__ y, const long long *__restrict__ t,
                                                      const PT *__restrict__ p, size_t base, int i0, int n, int vec) {
    IngQuadT<XY, PT> q;
    if (vec && i0 + 3 < n) {
        ing_vec4(x + base + i0, q.x); ing_vec4(y + base + i0, q.y); ing_vec4(p + base + i0, q.p); ing_vec4(t + base + i0, q.t);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool on = i0 + k < n;
            q.x[k] = on ? x[base + i0 + k] : (XY)-1; q.y[k] = on ? y[base + i0 + k] : (XY)-1; q.p[k] = on ? p[base + i0 + k] : (PT)-1;
            q.t[k] = on ? t[base + i0 + k] : 0;
        }
    }
    return q;
}

// Where the coordinates of an event come from.  IngXY: the float32 values themselves (rectified by the caller).  IngRect: raw sensor
// pixel indices looked up in the DSEC rectification map [Hs][Ws] of (x_rect, y_rect) pairs -- rectify_ev_map[y, x] of reference
// src/loader/dsec/loader.py:153,187-189 -- as part of the coordinate load: one 8-byte load per event after a bounds test on the raw
// index, no [B][N] float arrays in between.  An index outside the map (the reference raises or wraps: unpinned) gives (-2, -2): it
// fails the in-image filter and both taps of the voxel builder fall outside every grid.  Everything behind the load is shared.
struct IngXY { const float *x, *y; };
struct IngRect { const int *x, *y; const float2 *map; int Hs, Ws; };
__device__ __forceinline__ IngQuad ing_load4(const IngXY &c, const long long *__restrict__ t, const float *__restrict__ p, size_t base,
                                             int i0, int n, int vec) {
    return ing_load4(c.x, c.y, t, p, base, i0, n, vec);
}
__device__ __forceinline__ IngQuad ing_load4(const IngRect &c, const long long *__restrict__ t, const float *__restrict__ p, size_t base,
                                             int i0, int n, int vec) {
    const IngQuadT<int, float> r = ing_load4(c.x, c.y, t, p, base, i0, n, vec);
    IngQuad q;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float2 m = make_float2(-2.f, -2.f);
        if (i0 + k < n && (unsigned)r.x[k] < (unsigned)c.Ws && (unsigned)r.y[k] < (unsigned)c.Hs)
            m = c.map[(size_t)r.y[k] * c.Ws + r.x[k]];
        q.x[k] = m.x; q.y[k] = m.y; q.p[k] = r.p[k]; q.t[k] = r.t[k];
    }
    return q;
}

// the counts and time extrema of a workgroup's threads -> slot `o` of the per-chunk tables
__device__ __forceinline__ void ing_chunk_reduce(int cp, int cn, long long tmin, long long tmax, const IngLayout &L, size_t o,
                                                 int (&s_c)[2][4], long long (&s_t)[2][4]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) {
        cp += __shfl_down(cp, o2, 64); cn += __shfl_down(cn, o2, 64);
        const long long a = __shfl_down(tmin, o2, 64), c2 = __shfl_down(tmax, o2, 64);
        tmin = a < tmin ? a : tmin; tmax = c2 > tmax ? c2 : tmax;
    }
    if ((tid & 63) == 0) { s_c[0][tid >> 6] = cp; s_c[1][tid >> 6] = cn; s_t[0][tid >> 6] = tmin; s_t[1][tid >> 6] = tmax; }
    __syncthreads();
    if (tid == 0) {
        L.chunk_cnt[o] = s_c[0][0] + s_c[0][1] + s_c[0][2] + s_c[0][3];
        L.chunk_cnt[o + 1] = s_c[1][0] + s_c[1][1] + s_c[1][2] + s_c[1][3];
        long long a = s_t[0][0], c2 = s_t[1][0];
        for (int w = 1; w < 4; ++w) { a = s_t[0][w] < a ? s_t[0][w] : a; c2 = s_t[1][w] > c2 ? s_t[1][w] : c2; }
        L.chunk_t[o] = a; L.chunk_t[o + 1] = c2;
    }
}

// grid (nchunks, B), 256 threads
template <typename SRC>
__device__ __forceinline__ void ing_count_body(const mpc_ingest_shape s, const IngLayout L,
                                               const SRC c,
                                               const long long *__restrict__ t, const float *__restrict__ p,
                                               const int *__restrict__ counts, int *__restrict__ out_max, int vec) {
    __shared__ int s_c[2][4];
    __shared__ long long s_t[2][4];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    // (the batch maxima that k_ingest_scan raises with atomicMax start at 0: set here, a launch earlier, instead of by a memset)
    if (b == 0 && chunk == 0 && tid < 2) out_max[tid] = 0;
    const int n = min(counts[b], s.N);
    const size_t base = (size_t)b * s.N;
    int cp = 0, cn = 0;
    long long tmin = 0x7fffffffffffffffLL, tmax = -0x7fffffffffffffffLL - 1;
    const int i0 = chunk * ING_CHUNK + tid * 4;
    if (i0 < n) {
        const IngQuad q = ing_load4(c, t, p, base, i0, n, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < n) {
                const int c = classify(q.x[k], q.y[k], q.p[k], s.H, s.W);
                cp += c == 1; cn += c == 2;
                const long long tv = q.t[k];            // extrema over ALL events of the window (loader.py:152)
                tmin = tv < tmin ? tv : tmin; tmax = tv > tmax ? tv : tmax;
            }
        }
    }
    ing_chunk_reduce(cp, cn, tmin, tmax, L, ((size_t)b * L.nchunks + chunk) * 2, s_c, s_t);
}

// the two kernels of this body: float coordinates (the signature it always had) / raw indices + the rectification map
__global__ __launch_bounds__(256) void k_ingest_count(const mpc_ingest_shape s, const IngLayout L, const float *__restrict__ x, const float *__restrict__ y,
    const long long *__restrict__ t, const float *__restrict__ p,
    const int *__restrict__ counts, int *__restrict__ out_max, int vec) {
    ing_count_body(s, L, IngXY{x, y}, t, p, counts, out_max, vec);
}
__global__ __launch_bounds__(256) void k_ingest_rect_count(const mpc_ingest_shape s, const IngLayout L, const int *__restrict__ x, const int *__restrict__ y,
    const float2 *__restrict__ map, int Hs, int Ws, const long long *__restrict__ t, const float *__restrict__ p,
    const int *__restrict__ counts, int *__restrict__ out_max, int vec) {
    ing_count_body(s, L, IngRect{x, y, map, Hs, Ws}, t, p, counts, out_max, vec);
}

// grid B, 256 threads: exclusive scan over the chunks of one sample
__global__ __launch_bounds__(256) void k_ingest_scan(const IngLayout L, int *__restrict__ out_max) {
    __shared__ int s_run[2];
    __shared__ int s_part[2][256];
    __shared__ long long s_t[2][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { s_run[0] = 0; s_run[1] = 0; }
    long long tmin = 0x7fffffffffffffffLL, tmax = -0x7fffffffffffffffLL - 1;
    __syncthreads();
    for (int c0 = 0; c0 < L.nchunks; c0 += 256) {
        const int c = c0 + tid;
        int vp = 0, vn = 0;
        if (c < L.nchunks) {
            const size_t o = ((size_t)b * L.nchunks + c) * 2;
            vp = L.chunk_cnt[o]; vn = L.chunk_cnt[o + 1];
            const long long a = L.chunk_t[o], c2 = L.chunk_t[o + 1];
            tmin = a < tmin ? a : tmin; tmax = c2 > tmax ? c2 : tmax;
        }
        s_part[0][tid] = vp; s_part[1][tid] = vn;
        __syncthreads();
        if (tid < 2) {                      // serial scan of <= 256 values per polarity: tiny
            int run = s_run[tid];
            for (int k = 0; k < 256; ++k) { const int v = s_part[tid][k]; s_part[tid][k] = run; run += v; }
            s_run[tid] = run;
        }
        __syncthreads();
        if (c < L.nchunks) {
            const size_t o = ((size_t)b * L.nchunks + c) * 2;
            L.chunk_off[o] = s_part[0][tid]; L.chunk_off[o + 1] = s_part[1][tid];
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long a = __shfl_down(tmin, o, 64), c2 = __shfl_down(tmax, o, 64);
        tmin = a < tmin ? a : tmin; tmax = c2 > tmax ? c2 : tmax;
    }
    if ((tid & 63) == 0) { s_t[0][tid >> 6] = tmin; s_t[1][tid >> 6] = tmax; }
    __syncthreads();
    if (tid == 0) {
        long long a = s_t[0][0], c2 = s_t[1][0];
        for (int w = 1; w < 4; ++w) { a = s_t[0][w] < a ? s_t[0][w] : a; c2 = s_t[1][w] > c2 ? s_t[1][w] : c2; }
        L.tminmax[b * 2] = a; L.tminmax[b * 2 + 1] = c2;
        L.totals[b * 2] = s_run[0]; L.totals[b * 2 + 1] = s_run[1];
        atomicMax(&out_max[0], s_run[0]);
        atomicMax(&out_max[1], s_run[1]);
    }
}

__device__ __forceinline__ int bin_index(double tn, int nb) {
    // np.searchsorted(np.linspace(0, 1, nb + 1), tn, side='left') - 1, clipped at 0.
    // linspace: e_i = i * (1.0 / nb) in float64, e_nb = 1.0 exactly.
    if (tn != tn) return nb;      // a window of one event: 0/0 time; numpy sorts NaN last (searchsorted -> nb + 1)
    const double step = 1.0 / (double)nb;
    int i = (int)ceil(tn * (double)nb);
    i = i < 0 ? 0 : (i > nb ? nb : i);
    auto edge = [&](int k) { return k >= nb ? 1.0 : (double)k * step; };
    while (i > 0 && edge(i - 1) >= tn) --i;
    while (i < nb && edge(i) < tn) ++i;
    if (i == nb && edge(nb) < tn) i = nb + 1;          // tn > 1 cannot happen after min/max normalisation
    return i - 1 < 0 ? 0 : i - 1;
}

// exclusive scan of (lp, ln), the positive / negative rows of every thread, over the workgroup: rp / rn = the LDS rows of this
// thread's first positive / negative (positives from the front, the negatives behind them), np_wg / nn_wg = the totals
__device__ __forceinline__ void ing_block_rank(int lp, int ln, int (&s_w)[2][4], int &rp, int &rn, int &np_wg, int &nn_wg) {
    const int tid = threadIdx.x;
    const int ip = wave_scan_incl(lp), in_ = wave_scan_incl(ln);
    if ((tid & 63) == 63) { s_w[0][tid >> 6] = ip; s_w[1][tid >> 6] = in_; }
    __syncthreads();
    int wp = 0, wn = 0;
    np_wg = 0; nn_wg = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < (tid >> 6)) { wp += s_w[0][w]; wn += s_w[1][w]; }
        np_wg += s_w[0][w]; nn_wg += s_w[1][w];
    }
    rp = wp + ip - lp; rn = np_wg + wn + in_ - ln;
}

// Workgroup `chunk` of the gridDim.x of sample b zeroes its share of the sample's padding rows (loader.py:360-364: zero rows,
// valid = 0; they stay last in their polarity block [0, Mp) / [Mp, M)) -- not a memset of the whole tensor in front of the kernel
__device__ __forceinline__ void ing_zero_padding(const IngLayout &L, int b, int chunk, int Mp, int M, float *__restrict__ events) {
    const int tp = L.totals[b * 2], tn_ = L.totals[b * 2 + 1];
    const int pad_p = 3 * (Mp - tp), pad_n = 3 * (M - Mp - tn_), pad = pad_p + pad_n;
    if (pad > 0) {
        const int per = (pad + (int)gridDim.x - 1) / (int)gridDim.x;
        float2 *zp = reinterpret_cast<float2 *>(events + ((size_t)b * M + tp) * 6);
        float2 *zn = reinterpret_cast<float2 *>(events + ((size_t)b * M + Mp + tn_) * 6);
        const int j1 = min((chunk + 1) * per, pad);
        for (int j = chunk * per + (int)threadIdx.x; j < j1; j += 256) {
            if (j < pad_p) zp[j] = make_float2(0.f, 0.f); else zn[j - pad_p] = make_float2(0.f, 0.f);
        }
    }
}

// The rows a workgroup put together in LDS -> its two runs of the output (slot `chunk` of the offset table), and its share of
// the sample's padding rows (loader.py:360-364: zero rows, valid = 0)
__device__ __forceinline__ void ing_flush(const float2 *s_rows, const IngLayout &L, int b, int chunk, int np_wg, int nn_wg,
                                          int max_pos, int max_neg, float *__restrict__ events) {
    const int tid = threadIdx.x, M = max_pos + max_neg;
    const size_t co = ((size_t)b * L.nchunks + chunk) * 2;
    float2 *dstp = reinterpret_cast<float2 *>(events + ((size_t)b * M + L.chunk_off[co]) * 6);
    float2 *dstn = reinterpret_cast<float2 *>(events + ((size_t)b * M + max_pos + L.chunk_off[co + 1]) * 6);
    for (int j = tid; j < 3 * np_wg; j += 256) dstp[j] = s_rows[j];
    for (int j = tid; j < 3 * nn_wg; j += 256) dstn[j] = s_rows[3 * np_wg + j];
    ing_zero_padding(L, b, chunk, max_pos, M, events);
}

// grid (nchunks, B), 256 threads.  Thread t owns 4 consecutive events, so ranks follow the input order.  The rows of a
// workgroup are two contiguous runs of the output (its positives, its negatives): they are put together in LDS and written as
// runs of 8-byte words (a lane writing its own 24-byte row was six scattered 4-byte stores per event).  The padding rows of
// the sample (loader.py:360-364: zero rows, valid = 0) are zeroed here too, a share per workgroup -- not by a memset of the
// whole tensor in front of the kernel.
template <typename SRC>
__device__ __forceinline__ void ing_scatter_body(const mpc_ingest_shape s, const IngLayout L,
                                                 const SRC c,
                                                 const long long *__restrict__ t, const float *__restrict__ p,
                                                 const int *__restrict__ counts, int max_pos, int max_neg,
                                                 float *__restrict__ events, float *__restrict__ xytp, int vec) {
    __shared__ int s_w[2][4];
    __shared__ float2 s_rows[ING_CHUNK * 3];          // positives from the front, the negatives behind them
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int n = min(counts[b], s.N);
    const size_t base = (size_t)b * s.N;
    const long long tmin = L.tminmax[b * 2], tmax = L.tminmax[b * 2 + 1];
    const double span = (double)(tmax - tmin);
    const int i0 = chunk * ING_CHUNK + tid * 4;
    IngQuad q;
    int cls[4], lp = 0, ln = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cls[k] = 0;
    if (i0 < n) {
        q = ing_load4(c, t, p, base, i0, n, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cls[k] = (i0 + k < n) ? classify(q.x[k], q.y[k], q.p[k], s.H, s.W) : 0;
            lp += cls[k] == 1; ln += cls[k] == 2;
        }
    }
    int rp, rn, np_wg, nn_wg;
    ing_block_rank(lp, ln, s_w, rp, rn, np_wg, nn_wg);
    if (i0 < n) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k >= n) continue;
            const long long tv = q.t[k];
            if (xytp != nullptr) {
                // loader.py:135-138: t = (t - t[0]).astype(float32); t = t / t[-1]   (t increasing)
                const float tf = (float)(tv - tmin) / (float)(tmax - tmin);
                reinterpret_cast<float4 *>(xytp)[base + i0 + k] = make_float4(q.x[k], q.y[k], tf, q.p[k]);
            }
            if (cls[k] == 0) continue;
            const double tn = (double)(tv - tmin) / span;                       // loader.py:152 (float64)
            const int row = cls[k] == 1 ? rp++ : rn++;
            s_rows[MPC_IDX(3 * row + 0, ING_CHUNK * 3)] = make_float2(q.y[k], q.x[k]);
            s_rows[MPC_IDX(3 * row + 1, ING_CHUNK * 3)] = make_float2((float)tn, q.p[k]);
            s_rows[MPC_IDX(3 * row + 2, ING_CHUNK * 3)] = make_float2((float)bin_index(tn, s.nb), 1.f);
        }
    }
    __syncthreads();
    ing_flush(s_rows, L, b, chunk, np_wg, nn_wg, max_pos, max_neg, events);
}

// the two kernels of this body: float coordinates (the signature it always had) / raw indices + the rectification map
__global__ __launch_bounds__(256) void k_ingest_scatter(const mpc_ingest_shape s, const IngLayout L, const float *__restrict__ x, const float *__restrict__ y,
    const long long *__restrict__ t, const float *__restrict__ p,
    const int *__restrict__ counts, int max_pos, int max_neg, float *__restrict__ events, float *__restrict__ xytp, int vec) {
    ing_scatter_body(s, L, IngXY{x, y}, t, p, counts, max_pos, max_neg, events, xytp, vec);
}
__global__ __launch_bounds__(256) void k_ingest_rect_scatter(const mpc_ingest_shape s, const IngLayout L, const int *__restrict__ x, const int *__restrict__ y,
    const float2 *__restrict__ map, int Hs, int Ws, const long long *__restrict__ t, const float *__restrict__ p,
    const int *__restrict__ counts, int max_pos, int max_neg, float *__restrict__ events, float *__restrict__ xytp, int vec) {
    ing_scatter_body(s, L, IngRect{x, y, map, Hs, Ws}, t, p, counts, max_pos, max_neg, events, xytp, vec);
}

// ---- ingest straight into the bucket-ordered layout (both halves in one) -----------------------------
// The rows of each polarity block ordered by (time bin, LUT strip) -- the key of the loss's backward buckets
// (ev_order.hip: mpc_event_bucket_order) -- as ingest WRITES them: the key of an event is known the moment its row is
// built, so ordering costs no pass over the event tensor of its own (ingest + mpc_event_bucket_order read and wrote the
// tensor once more: 175 + 50 us at 14 x 200k events).  Counting sort: per-chunk counts of (polarity, key) -> the scans of
// the bucket-order kernels (ev_order.hip) -> scatter.  Order inside a bucket is not defined and need not be.
__device__ __forceinline__ int ing_key(const mpc_ingest_shape &s, const EvKey &k, float yv, double tn) {
    return ev_key(k, s.nb, bin_index(tn, s.nb), yv);          // (the row's bin column holds (float)bin_index: the same int)
}

// grid (nchunks, B), 256 threads, dynamic LDS 2 * (NK + 1) ints: counts[b][pol][key][chunk]
template <typename SRC>
__device__ __forceinline__ void ing_keycount_body(const mpc_ingest_shape s, const IngLayout L, const EvKey k,
                                                  const SRC c,
                                                  const long long *__restrict__ t, const float *__restrict__ p,
                                                  const int *__restrict__ counts, int *__restrict__ kcounts, int vec) {
    extern __shared__ int s_k[];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int n = min(counts[b], s.N);
    const size_t base = (size_t)b * s.N;
    const long long tmin = L.tminmax[b * 2], tmax = L.tminmax[b * 2 + 1];
    const double span = (double)(tmax - tmin);
    for (int i = tid; i < 2 * (k.NK + 1); i += 256) s_k[i] = 0;
    __syncthreads();
    const int i0 = chunk * ING_CHUNK + tid * 4;
    if (i0 < n) {
        const IngQuad q = ing_load4(c, t, p, base, i0, n, vec);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u >= n) continue;
            const int c = classify(q.x[u], q.y[u], q.p[u], s.H, s.W);
            if (c == 0) continue;
            const double tn = (double)(q.t[u] - tmin) / span;
            atomicAdd(&s_k[MPC_IDX((c - 1) * (k.NK + 1) + ing_key(s, k, q.y[u], tn), 2 * (k.NK + 1))], 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * (k.NK + 1); i += 256) {
        const int pol = i / (k.NK + 1), key = i - pol * (k.NK + 1);
        kcounts[evo_count_at(k, L.nchunks, b, pol, key, chunk)] = s_k[i];
    }
}

// the two kernels of this body: float coordinates (the signature it always had) / raw indices + the rectification map
__global__ __launch_bounds__(256) void k_ingest_keycount(const mpc_ingest_shape s, const IngLayout L, const EvKey k, const float *__restrict__ x, const float *__restrict__ y,
    const long long *__restrict__ t, const float *__restrict__ p,
    const int *__restrict__ counts, int *__restrict__ kcounts, int vec) {
    ing_keycount_body(s, L, k, IngXY{x, y}, t, p, counts, kcounts, vec);
}
__global__ __launch_bounds__(256) void k_ingest_rect_keycount(const mpc_ingest_shape s, const IngLayout L, const EvKey k, const int *__restrict__ x, const int *__restrict__ y,
    const float2 *__restrict__ map, int Hs, int Ws, const long long *__restrict__ t, const float *__restrict__ p,
    const int *__restrict__ counts, int *__restrict__ kcounts, int vec) {
    ing_keycount_body(s, L, k, IngRect{x, y, map, Hs, Ws}, t, p, counts, kcounts, vec);
}

// grid (nchunks, B), 256 threads, dynamic LDS 2 * (NK + 1) ints.  kcounts (scanned in place) = first row of this chunk's
// share inside every (polarity, key); offsets [B][2][NK + 1] = first row of every key
template <typename SRC>
__device__ __forceinline__ void ing_scatter_ordered_body(const mpc_ingest_shape s, const IngLayout L, const EvKey k,
                                                         const SRC c,
                                                         const long long *__restrict__ t, const float *__restrict__ p,
                                                         const int *__restrict__ counts, int M,
                                                         const int *__restrict__ kcounts, const int *__restrict__ offsets,
                                                         float *__restrict__ events, float *__restrict__ xytp, int vec) {
    extern __shared__ int s_k[];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int n = min(counts[b], s.N);
    const size_t base = (size_t)b * s.N;
    const long long tmin = L.tminmax[b * 2], tmax = L.tminmax[b * 2 + 1];
    const double span = (double)(tmax - tmin);
    for (int i = tid; i < 2 * (k.NK + 1); i += 256) {
        const int pol = i / (k.NK + 1), key = i - pol * (k.NK + 1);
        s_k[i] = offsets[(size_t)(b * 2 + pol) * (k.NK + 1) + key] + kcounts[evo_count_at(k, L.nchunks, b, pol, key, chunk)];
    }
    __syncthreads();
    const int i0 = chunk * ING_CHUNK + tid * 4;
    if (i0 < n) {
        const IngQuad q = ing_load4(c, t, p, base, i0, n, vec);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u;
            if (i >= n) continue;
            const long long tv = q.t[u];
            if (xytp != nullptr) {
                const float tf = (float)(tv - tmin) / (float)(tmax - tmin);
                reinterpret_cast<float4 *>(xytp)[base + i] = make_float4(q.x[u], q.y[u], tf, q.p[u]);
            }
            const int c = classify(q.x[u], q.y[u], q.p[u], s.H, s.W);
            if (c == 0) continue;
            const double tn = (double)(tv - tmin) / span;
            const int row = atomicAdd(&s_k[MPC_IDX((c - 1) * (k.NK + 1) + ing_key(s, k, q.y[u], tn), 2 * (k.NK + 1))], 1);
            float2 *e = reinterpret_cast<float2 *>(events + ((size_t)b * M + row) * 6);      // (24-byte rows: 8-byte aligned)
            e[0] = make_float2(q.y[u], q.x[u]); e[1] = make_float2((float)tn, q.p[u]);
            e[2] = make_float2((float)bin_index(tn, s.nb), 1.f);
        }
    }
    const int Mp = offsets[(size_t)(b * 2 + 1) * (k.NK + 1)];          // first row of the negative block = max_pos
    ing_zero_padding(L, b, chunk, Mp, M, events);
}

// the two kernels of this body: float coordinates (the signature it always had) / raw indices + the rectification map
__global__ __launch_bounds__(256) void k_ingest_scatter_ordered(const mpc_ingest_shape s, const IngLayout L, const EvKey k, const float *__restrict__ x, const float *__restrict__ y,
    const long long *__restrict__ t, const float *__restrict__ p,
    const int *__restrict__ counts, int M, const int *__restrict__ kcounts, const int *__restrict__ offsets,
    float *__restrict__ events, float *__restrict__ xytp, int vec) {
    ing_scatter_ordered_body(s, L, k, IngXY{x, y}, t, p, counts, M, kcounts, offsets, events, xytp, vec);
}
__global__ __launch_bounds__(256) void k_ingest_rect_scatter_ordered(const mpc_ingest_shape s, const IngLayout L, const EvKey k, const int *__restrict__ x, const int *__restrict__ y,
    const float2 *__restrict__ map, int Hs, int Ws, const long long *__restrict__ t, const float *__restrict__ p,
    const int *__restrict__ counts, int M, const int *__restrict__ kcounts, const int *__restrict__ offsets,
    float *__restrict__ events, float *__restrict__ xytp, int vec) {
    ing_scatter_ordered_body(s, L, k, IngRect{x, y, map, Hs, Ws}, t, p, counts, M, kcounts, offsets, events, xytp, vec);
}

// ------------------------------------------------------------------------------------------
static int ing_validate(const mpc_ingest_shape *s) {
    MPC_CHECK_ARG(s->B >= 0 && s->N >= 0 && s->H >= 1 && s->W >= 1 && s->nb >= 1, MPC_E_SHAPE, "bad ingest shape");
    MPC_CHECK_ARG((int64_t)s->B * s->N < (1LL << 31), MPC_E_UNSUPPORTED, "too many events");
    return 0;
}

// 16-byte loads of four consecutive events: every sample's first event aligned
static int ing_vec(const mpc_ingest_shape *s, const void *x, const void *y, const void *t, const void *p) {
    return (s->N % 4 == 0) && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)t | (uintptr_t)p) & 15) == 0 ? 1 : 0;
}

struct IngHost { IngLayout L; int64_t total; };

static IngHost ing_layout(const mpc_ingest_shape *s, void *ws) {
    IngHost h;
    const int B = s->B > 0 ? s->B : 1;
    h.L.nchunks = mpc_cdiv(s->N > 0 ? s->N : 1, ING_CHUNK);
    const int64_t nc = (int64_t)B * h.L.nchunks;
    int64_t off = 0;
    char *w = (char *)ws;
    h.L.chunk_t = (long long *)(w + off);  off += mpc_align(nc * 2 * 8);
    h.L.tminmax = (long long *)(w + off);  off += mpc_align((int64_t)B * 2 * 8);
    h.L.chunk_cnt = (int *)(w + off);      off += mpc_align(nc * 2 * 4);
    h.L.chunk_off = (int *)(w + off);      off += mpc_align(nc * 2 * 4);
    h.L.totals = (int *)(w + off);         off += mpc_align((int64_t)B * 2 * 4);
    h.total = off;
    return h;
}

extern "C" int64_t mpc_ingest_workspace_bytes(const mpc_ingest_shape *s) {
    if (!s) { mpc_set_error("mpc_ingest_workspace_bytes: null shape"); return MPC_E_NULL; }
    int rc = ing_validate(s);
    if (rc) return rc;
    return ing_layout(s, nullptr).total;
}

// The entry points below exist twice: with the float coordinates (IngXY) and with raw indices + the rectification map (IngRect).
// One host body per entry point, a template over the source as the kernels are.
static int ing_rect_validate(int32_t Hs, int32_t Ws, const float *map) {
    MPC_CHECK_ARG(Hs >= 1 && Ws >= 1 && (int64_t)Hs * Ws < (1LL << 31), MPC_E_SHAPE, "bad rectification map shape");
    MPC_CHECK_ARG(map != nullptr, MPC_E_NULL, "rectify_map is null");
    MPC_CHECK_ARG(((uintptr_t)map & 7) == 0, MPC_E_UNSUPPORTED, "rectify_map must be 8-byte aligned (one load per (x, y) pair)");
    return 0;
}

template <typename SRC>
static int ing_count(const char *fn, const mpc_ingest_shape *s, const SRC &c, const int64_t *t_us, const float *p, const int32_t *counts,
                     int32_t *out_max, void *ws, void *stream) {
    if (!(s && counts && out_max && ws && ((c.x && c.y && t_us && p) || s->N == 0 || s->B == 0))) { mpc_set_error("%s: null argument", fn); return MPC_E_NULL; }
    int rc = ing_validate(s);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (s->B == 0) return mpc_zero_async(out_max, 2 * sizeof(int32_t), st);
    const IngLayout L = ing_layout(s, ws).L;
    const long long *t = reinterpret_cast<const long long *>(t_us);
    const int vec = ing_vec(s, c.x, c.y, t_us, p);
    if constexpr (std::is_same<SRC, IngXY>::value) MPC_LAUNCH(k_ingest_count, dim3(L.nchunks, s->B), dim3(256), 0, st, *s, L, c.x, c.y, t, p, counts, out_max, vec);
    else MPC_LAUNCH(k_ingest_rect_count, dim3(L.nchunks, s->B), dim3(256), 0, st, *s, L, c.x, c.y, c.map, c.Hs, c.Ws, t, p, counts, out_max, vec);
    MPC_LAUNCH(k_ingest_scan, dim3(s->B), dim3(256), 0, st, L, out_max);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_ingest_count(const mpc_ingest_shape *s, const float *x, const float *y, const int64_t *t_us,
                                const float *p, const int32_t *counts, int32_t *out_max, void *ws, void *stream) {
    return ing_count(__func__, s, IngXY{x, y}, t_us, p, counts, out_max, ws, stream);
}

extern "C" int mpc_ingest_rect_count(const mpc_ingest_shape *s, int32_t Hs, int32_t Ws, const float *rectify_map, const int32_t *x,
                                     const int32_t *y, const int64_t *t_us, const float *p, const int32_t *counts, int32_t *out_max,
                                     void *ws, void *stream) {
    int rc = ing_rect_validate(Hs, Ws, rectify_map);
    if (rc) return rc;
    return ing_count(__func__, s, IngRect{x, y, reinterpret_cast<const float2 *>(rectify_map), Hs, Ws}, t_us, p, counts, out_max, ws, stream);
}

template <typename SRC>
static int ing_scatter(const char *fn, const mpc_ingest_shape *s, const SRC &c, const int64_t *t_us, const float *p, const int32_t *counts,
                       int32_t max_pos, int32_t max_neg, float *events, float *xytp, void *ws, void *stream) {
    if (!(s && counts && ws && ((c.x && c.y && t_us && p) || s->N == 0 || s->B == 0))) { mpc_set_error("%s: null argument", fn); return MPC_E_NULL; }
    if (!(max_pos >= 0 && max_neg >= 0 && (events || max_pos + max_neg == 0 || s->B == 0))) { mpc_set_error("%s: events is null", fn); return MPC_E_NULL; }
    int rc = ing_validate(s);
    if (rc) return rc;
    if (s->B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = (int64_t)max_pos + max_neg;
    if (s->N == 0) return M > 0 ? mpc_zero_async(events, (size_t)s->B * M * 6 * sizeof(float), st) : 0;     // padding rows only
    const IngLayout L = ing_layout(s, ws).L;
    const long long *t = reinterpret_cast<const long long *>(t_us);
    const int vec = ing_vec(s, c.x, c.y, t_us, p);
    if constexpr (std::is_same<SRC, IngXY>::value) MPC_LAUNCH(k_ingest_scatter, dim3(L.nchunks, s->B), dim3(256), 0, st, *s, L, c.x, c.y, t, p, counts, max_pos, max_neg, events, xytp, vec);
    else MPC_LAUNCH(k_ingest_rect_scatter, dim3(L.nchunks, s->B), dim3(256), 0, st, *s, L, c.x, c.y, c.map, c.Hs, c.Ws, t, p, counts, max_pos, max_neg, events, xytp, vec);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_ingest_scatter(const mpc_ingest_shape *s, const float *x, const float *y, const int64_t *t_us,
                                  const float *p, const int32_t *counts, int32_t max_pos, int32_t max_neg,
                                  float *events, float *xytp, void *ws, void *stream) {
    return ing_scatter(__func__, s, IngXY{x, y}, t_us, p, counts, max_pos, max_neg, events, xytp, ws, stream);
}

extern "C" int mpc_ingest_rect_scatter(const mpc_ingest_shape *s, int32_t Hs, int32_t Ws, const float *rectify_map, const int32_t *x,
                                       const int32_t *y, const int64_t *t_us, const float *p, const int32_t *counts, int32_t max_pos,
                                       int32_t max_neg, float *events, float *xytp, void *ws, void *stream) {
    int rc = ing_rect_validate(Hs, Ws, rectify_map);
    if (rc) return rc;
    return ing_scatter(__func__, s, IngRect{x, y, reinterpret_cast<const float2 *>(rectify_map), Hs, Ws}, t_us, p, counts, max_pos, max_neg,
                       events, xytp, ws, stream);
}


extern "C" int64_t mpc_ingest_ordered_workspace_bytes(const mpc_ingest_shape *s, const mpc_shape *loss) {
    if (!s || !loss) { mpc_set_error("mpc_ingest_ordered_workspace_bytes: null shape"); return MPC_E_NULL; }
    int rc = ing_validate(s);
    if (rc) return rc;
    const int32_t ncs = mpc_event_lut_strips(loss);
    if (ncs <= 0) { mpc_set_error("mpc_ingest_ordered_workspace_bytes: no bucketed event layout for this loss shape"); return MPC_E_UNSUPPORTED; }
    return evo_ws(s->B, loss->nb * ncs, mpc_cdiv(s->N > 0 ? s->N : 1, ING_CHUNK), nullptr).bytes;
}

// Same outputs as mpc_ingest_scatter followed by mpc_event_bucket_order for the loss shape `loss` (B, nb, H, W, sp, hq, wq,
// flags of the FocusLoss; M = max_pos + max_neg, Mp = max_pos): `events` with the rows of every polarity block grouped by
// (time bin, LUT strip) and the table `offsets` [B][2][nb * strips + 1].  `ws` = the workspace of mpc_ingest_count
// (unchanged since that call), `ws_order` = mpc_ingest_ordered_workspace_bytes.
template <typename SRC>
static int ing_scatter_ordered(const char *fn, const mpc_ingest_shape *s, const mpc_shape *loss, const SRC &c, const int64_t *t_us,
                               const float *p, const int32_t *counts, int32_t max_pos, int32_t max_neg, float *events, int32_t *offsets,
                               float *xytp, void *ws, void *ws_order, void *stream) {
    if (!(s && loss && counts && ws && ws_order && offsets && ((c.x && c.y && t_us && p) || s->N == 0 || s->B == 0))) { mpc_set_error("%s: null argument", fn); return MPC_E_NULL; }
    if (!(max_pos >= 0 && max_neg >= 0 && (events || max_pos + max_neg == 0 || s->B == 0))) { mpc_set_error("%s: events is null", fn); return MPC_E_NULL; }
    int rc = ing_validate(s);
    if (rc) return rc;
    if ((rc = mpc_validate_shape(loss))) return rc;
    MPC_CHECK_ARG(loss->B == s->B && loss->nb == s->nb && loss->H == s->H && loss->W == s->W && loss->M == max_pos + max_neg && loss->Mp == max_pos,
                  MPC_E_SHAPE, "loss shape does not match the ingest shape / the block sizes");
    const mpc_ws_layout LL = mpc_layout(loss);
    MPC_CHECK_ARG(LL.n_cstrips > 0, MPC_E_UNSUPPORTED, "no bucketed event layout for this loss shape");
    if (s->B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = (int64_t)max_pos + max_neg;
    const EvKey k{LL.n_cstrips, LL.cstrip_rows, loss->nb * LL.n_cstrips, loss->sp, loss->hq};
    if (M > 0 && s->N == 0) {
        const int e = mpc_zero_async(events, (size_t)s->B * M * 6 * sizeof(float), st);     // padding rows only (else: the scatter kernel zeroes them)
        if (e) return e;
    }
    const IngLayout L = ing_layout(s, ws).L;
    const EvoWs w = evo_ws(s->B, k.NK, L.nchunks, ws_order);
    int *kcounts = w.counts;
    const size_t lds = (size_t)2 * (k.NK + 1) * sizeof(int);
    if (s->N == 0) return mpc_zero_async(offsets, (size_t)s->B * 2 * (k.NK + 1) * sizeof(int32_t), st);
    const long long *t = reinterpret_cast<const long long *>(t_us);
    const int vec = ing_vec(s, c.x, c.y, t_us, p);
    if constexpr (std::is_same<SRC, IngXY>::value) MPC_LAUNCH(k_ingest_keycount, dim3(L.nchunks, s->B), dim3(256), lds, st, *s, L, k, c.x, c.y, t, p, counts, kcounts, vec);
    else MPC_LAUNCH(k_ingest_rect_keycount, dim3(L.nchunks, s->B), dim3(256), lds, st, *s, L, k, c.x, c.y, c.map, c.Hs, c.Ws, t, p, counts, kcounts, vec);
    MPC_CHECK_LAUNCH();
    if ((rc = mpc_evo_scans(loss, k, w, offsets, st))) return rc;
    if constexpr (std::is_same<SRC, IngXY>::value) MPC_LAUNCH(k_ingest_scatter_ordered, dim3(L.nchunks, s->B), dim3(256), lds, st, *s, L, k, c.x, c.y, t, p,
                                                              counts, (int)M, kcounts, (const int *)offsets, events, xytp, vec);
    else MPC_LAUNCH(k_ingest_rect_scatter_ordered, dim3(L.nchunks, s->B), dim3(256), lds, st, *s, L, k, c.x, c.y, c.map, c.Hs, c.Ws, t, p,
                    counts, (int)M, kcounts, (const int *)offsets, events, xytp, vec);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_ingest_scatter_ordered(const mpc_ingest_shape *s, const mpc_shape *loss, const float *x, const float *y,
                                          const int64_t *t_us, const float *p, const int32_t *counts, int32_t max_pos,
                                          int32_t max_neg, float *events, int32_t *offsets, float *xytp, void *ws, void *ws_order,
                                          void *stream) {
    return ing_scatter_ordered(__func__, s, loss, IngXY{x, y}, t_us, p, counts, max_pos, max_neg, events, offsets, xytp, ws, ws_order, stream);
}

extern "C" int mpc_ingest_rect_scatter_ordered(const mpc_ingest_shape *s, const mpc_shape *loss, int32_t Hs, int32_t Ws,
                                               const float *rectify_map, const int32_t *x, const int32_t *y, const int64_t *t_us,
                                               const float *p, const int32_t *counts, int32_t max_pos, int32_t max_neg, float *events,
                                               int32_t *offsets, float *xytp, void *ws, void *ws_order, void *stream) {
    int rc = ing_rect_validate(Hs, Ws, rectify_map);
    if (rc) return rc;
    return ing_scatter_ordered(__func__, s, loss, IngRect{x, y, reinterpret_cast<const float2 *>(rectify_map), Hs, Ws}, t_us, p, counts,
                               max_pos, max_neg, events, offsets, xytp, ws, ws_order, stream);
}

// ---- raw windows of the EVIMO2 / MultiFlow configurations -> the same [B][M][6] tensor --------------------------------
//   MPC_WINDOW_TIME_FP32_SUFFIX (EVIMO2): reference src/loader/evimo2/datasubset.py:206-228.  The cut, the normalisation and
//       the bins run in FLOAT32 there (ts[-1] - flow_duration * 1e3 promotes an int64 0-dim tensor to fp32), and that is what
//       the kernels restate operation by operation: ts_start = f32(t_last) - f32(duration), keep f32(t) > ts_start,
//       (f32(t) - ts_start) / (f32(t_last) - ts_start) with a correctly rounded quotient, torch.searchsorted over the fp32 edges
//       of torch.linspace (computed by the caller on the CPU, read here from LDS).  Conversion to fp32 is monotone, so with
//       non-decreasing timestamps the kept events are a SUFFIX of the window: its first index is found by a 64-way search, and
//       counting and scattering start at the 1024-event chunk that holds it -- the 0.4 s of context in front is never loaded.
//   MPC_WINDOW_TIME_MINMAX64 (MultiFlow): src/loader/multiflow/sample.py:224-236, the float64 arithmetic of the DSEC loader
//       above (bin_index, the extrema of k_ingest_scan) without the in-image filter.
//   Collate: src/modules/data_loading.py:14-47 (pad_events / event_collate_fn) -- the layout of the DSEC collate (ing_flush);
//       without the polarity split every kept event counts as "positive" and the negative block is empty.
// Passes: k_window_first (first kept index per sample) -> k_window_count -> k_ingest_scan -> k_window_scatter.  Workgroup
// `blockIdx.x` of sample b works on chunk blockIdx.x + first[b] / ING_CHUNK, so the chunk grid keeps the 16-byte alignment of
// ing_quad; workgroups past the end of the sample only write their (zero) counts and their share of the padding.
__device__ __forceinline__ float win_ts_start(long long t_last, float duration_us) { return (float)t_last - duration_us; }

// grid B, 64 threads
__global__ __launch_bounds__(64) void k_window_first(const mpc_window_shape s, const long long *__restrict__ t,
                                                     const int *__restrict__ counts, int *__restrict__ first,
                                                     int *__restrict__ out_max) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b == 0 && lane < 2) out_max[lane] = 0;          // (raised by k_ingest_scan with atomicMax, two launches later)
    const int n = max(min(counts[b], s.N), 0);
    const size_t base = (size_t)b * s.N;
    int lo = 0, hi = 0;          // every event in front of lo is dropped, every event from hi on is kept
    if (s.time_mode == MPC_WINDOW_TIME_FP32_SUFFIX && n > 0) {
        const float ts_start = win_ts_start(t[base + n - 1], s.duration_us);
        hi = n;
        while (hi > lo) {
            const int step = (hi - lo + 63) / 64;
            const int idx = lo + (lane + 1) * step - 1;          // 64 probes, step apart; the last one is at or past hi - 1
            const bool kept = idx < hi ? (float)t[base + MPC_IDX(idx, n)] > ts_start : true;
            const unsigned long long m = __ballot(kept);
            if (m == 0ull) { lo = hi; break; }
            const int l = __ffsll((long long)m) - 1;          // first kept probe: the answer lies behind the probe before it
            hi = min(lo + (l + 1) * step - 1, hi);
            lo = lo + l * step;
        }
    }
    if (lane == 0) first[b] = lo;
}

template <typename PT>
__device__ __forceinline__ int win_classify(PT p, int split) {
    // 1: positive block, 2: negative block, 0: in neither (datasubset.py:219-220: boolean masks p == 1 and p == 0)
    return split ? (p == (PT)1 ? 1 : (p == (PT)0 ? 2 : 0)) : 1;
}

// grid (nchunks, B), 256 threads.  The suffix mode reads the polarity alone (nothing at all without the split).
template <int TM, typename PT>
__global__ __launch_bounds__(256) void k_window_count(const mpc_window_shape s, const IngLayout L, const int *__restrict__ first,
                                                      const long long *__restrict__ t, const PT *__restrict__ p,
                                                      const int *__restrict__ counts, int vec) {
    __shared__ int s_c[2][4];
    __shared__ long long s_t[2][4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = max(min(counts[b], s.N), 0), f = first[b];
    const int chunk = (int)blockIdx.x + f / ING_CHUNK;
    const size_t base = (size_t)b * s.N;
    int cp = 0, cn = 0;
    long long tmin = 0x7fffffffffffffffLL, tmax = -0x7fffffffffffffffLL - 1;
    const int i0 = chunk < L.nchunks ? chunk * ING_CHUNK + tid * 4 : n;
    if (i0 < n) {
        if (s.split) {
            PT pv[4];
            ing_quad(p, base, i0, n, vec, (PT)-1, pv);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = (i0 + k < n && i0 + k >= f) ? win_classify(pv[k], 1) : 0;
                cp += c == 1; cn += c == 2;
            }
        } else {
            cp = min(i0 + 4, n) - max(i0, f);
            cp = cp < 0 ? 0 : cp;
        }
        if (TM == MPC_WINDOW_TIME_MINMAX64) {          // extrema over all events of the window (sample.py:230)
            long long tv[4];
            ing_quad(t, base, i0, n, vec, 0LL, tv);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i0 + k < n) { tmin = tv[k] < tmin ? tv[k] : tmin; tmax = tv[k] > tmax ? tv[k] : tmax; }
            }
        }
    }
    ing_chunk_reduce(cp, cn, tmin, tmax, L, ((size_t)b * L.nchunks + blockIdx.x) * 2, s_c, s_t);
}

__device__ __forceinline__ int win_bin(const float *e, float tn, int nb) {
    // torch.searchsorted(edges, tn) - 1 (side = 'left': the number of edges below tn), -1 -> 0   (datasubset.py:213-214)
    int i = (int)ceilf(tn * (float)nb);          // a guess; the two loops settle it on the edges themselves
    i = i > 0 ? (i > nb ? nb : i) : 0;
    while (i > 0 && e[MPC_IDX(i - 1, nb + 1)] >= tn) --i;
    while (i <= nb && e[MPC_IDX(i, nb + 1)] < tn) ++i;
    return i - 1 < 0 ? 0 : i - 1;
}

// grid (nchunks, B), 256 threads, dynamic LDS (nb + 1) floats in the suffix mode (the bin edges)
template <int TM, typename XY, typename PT>
__global__ __launch_bounds__(256) void k_window_scatter(const mpc_window_shape s, const IngLayout L, const int *__restrict__ first,
                                                        const XY *__restrict__ x, const XY *__restrict__ y,
                                                        const long long *__restrict__ t, const PT *__restrict__ p,
                                                        const int *__restrict__ counts, const float *__restrict__ edges,
                                                        int max_pos, int max_neg, float *__restrict__ events, int vec) {
    extern __shared__ float s_edge[];
    __shared__ int s_w[2][4];
    __shared__ float2 s_rows[ING_CHUNK * 3];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = max(min(counts[b], s.N), 0), f = first[b];
    const int chunk = (int)blockIdx.x + f / ING_CHUNK;
    const size_t base = (size_t)b * s.N;
    if (TM == MPC_WINDOW_TIME_FP32_SUFFIX) {
        for (int i = tid; i <= s.nb; i += 256) s_edge[i] = edges[i];          // (visible after the barrier of ing_block_rank)
    }
    const int i0 = chunk < L.nchunks ? chunk * ING_CHUNK + tid * 4 : n;
    IngQuadT<XY, PT> q;
    int cls[4], lp = 0, ln = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cls[k] = 0;
    if (i0 < n && i0 + 3 >= f) {
        q = ing_load4(x, y, t, p, base, i0, n, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cls[k] = (i0 + k < n && i0 + k >= f) ? win_classify(q.p[k], s.split) : 0;
            lp += cls[k] == 1; ln += cls[k] == 2;
        }
    }
    int rp, rn, np_wg, nn_wg;
    ing_block_rank(lp, ln, s_w, rp, rn, np_wg, nn_wg);
    if (lp + ln > 0) {
        float ts_start = 0.f, den = 1.f;
        long long tmin = 0;
        double span = 1.0;
        if (TM == MPC_WINDOW_TIME_FP32_SUFFIX) {
            const long long t_last = t[base + MPC_IDX(n - 1, s.N)];
            ts_start = win_ts_start(t_last, s.duration_us);          // datasubset.py:208
            den = (float)t_last - ts_start;                          // :211, ts_end - ts_start
        } else {
            tmin = L.tminmax[b * 2];
            span = (double)(L.tminmax[b * 2 + 1] - tmin);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (cls[k] == 0) continue;
            float tn, bin;
            if (TM == MPC_WINDOW_TIME_FP32_SUFFIX) {
                tn = ((float)q.t[k] - ts_start) / den;          // IEEE quotient (hipcc rounds fp32 division correctly by default; no fast-math here)
                bin = (float)win_bin(s_edge, tn, s.nb);
            } else {
                const double tn64 = (double)(q.t[k] - tmin) / span;          // sample.py:231 (float64)
                tn = (float)tn64;
                bin = (float)bin_index(tn64, s.nb);
            }
            const int row = cls[k] == 1 ? rp++ : rn++;
            s_rows[MPC_IDX(3 * row + 0, ING_CHUNK * 3)] = make_float2((float)q.y[k] * s.y_scale, (float)q.x[k] * s.x_scale);
            s_rows[MPC_IDX(3 * row + 1, ING_CHUNK * 3)] = make_float2(tn, (float)q.p[k]);
            s_rows[MPC_IDX(3 * row + 2, ING_CHUNK * 3)] = make_float2(bin, 1.f);
        }
    }
    __syncthreads();
    ing_flush(s_rows, L, b, blockIdx.x, np_wg, nn_wg, max_pos, max_neg, events);
}

#define WIN_MAX_EDGES 4096          // (nb + 1) floats of dynamic LDS beside the 24 KB of row staging

static int win_validate(const mpc_window_shape *s) {
    MPC_CHECK_ARG(s->B >= 0 && s->N >= 0 && s->nb >= 1, MPC_E_SHAPE, "bad window shape");
    MPC_CHECK_ARG(s->time_mode == MPC_WINDOW_TIME_FP32_SUFFIX || s->time_mode == MPC_WINDOW_TIME_MINMAX64, MPC_E_SHAPE, "unknown time mode");
    MPC_CHECK_ARG((s->xy_int | 1) == 1 && (s->p_int64 | 1) == 1 && (s->split | 1) == 1, MPC_E_SHAPE, "xy_int, p_int64 and split are 0 or 1");
    MPC_CHECK_ARG((int64_t)s->B * s->N < (1LL << 31) && s->N <= 0x7fffffff - 2 * ING_CHUNK, MPC_E_UNSUPPORTED, "too many events");
    if (s->time_mode == MPC_WINDOW_TIME_FP32_SUFFIX) {
        MPC_CHECK_ARG(s->duration_us >= 0.f && s->duration_us < 3e38f, MPC_E_SHAPE, "duration_us must be finite and not negative");
        MPC_CHECK_ARG(s->nb + 1 <= WIN_MAX_EDGES, MPC_E_UNSUPPORTED, "more bin edges than the LDS table holds");
    }
    return 0;
}

struct WinHost { IngLayout L; int *first; int64_t total; };

static WinHost win_layout(const mpc_window_shape *s, void *ws) {
    const mpc_ingest_shape is{s->B, s->N, 1, 1, s->nb};
    const IngHost h = ing_layout(&is, ws);
    WinHost w;
    w.L = h.L;
    w.first = (int *)((char *)ws + h.total);
    w.total = h.total + mpc_align((int64_t)(s->B > 0 ? s->B : 1) * 4);
    return w;
}

static int win_vec(const mpc_window_shape *s, const void *a) { return (s->N % 4 == 0) && ((uintptr_t)a & 15) == 0; }

extern "C" int64_t mpc_ingest_window_workspace_bytes(const mpc_window_shape *s) {
    if (!s) { mpc_set_error("mpc_ingest_window_workspace_bytes: null shape"); return MPC_E_NULL; }
    int rc = win_validate(s);
    if (rc) return rc;
    return win_layout(s, nullptr).total;
}

extern "C" int mpc_ingest_window_count(const mpc_window_shape *s, const int64_t *t_us, const void *p, const int32_t *counts,
                                       int32_t *out_max, void *ws, void *stream) {
    MPC_CHECK_ARG(s && counts && out_max && ws && ((t_us && p) || s->N == 0 || s->B == 0), MPC_E_NULL, "null argument");
    int rc = win_validate(s);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (s->B == 0) return mpc_zero_async(out_max, 2 * sizeof(int32_t), st);
    const WinHost w = win_layout(s, ws);
    const long long *t = reinterpret_cast<const long long *>(t_us);
    const int vec = win_vec(s, t_us) && win_vec(s, p);
    const dim3 grid(w.L.nchunks, s->B);
    MPC_LAUNCH(k_window_first, dim3(s->B), dim3(64), 0, st, *s, t, counts, w.first, out_max);
#define WIN_COUNT(TM, PT) MPC_LAUNCH((k_window_count<TM, PT>), grid, dim3(256), 0, st, *s, w.L, w.first, t, (const PT *)p, counts, vec)
    if (s->time_mode == MPC_WINDOW_TIME_FP32_SUFFIX) { if (s->p_int64) WIN_COUNT(MPC_WINDOW_TIME_FP32_SUFFIX, long long); else WIN_COUNT(MPC_WINDOW_TIME_FP32_SUFFIX, float); }
    else { if (s->p_int64) WIN_COUNT(MPC_WINDOW_TIME_MINMAX64, long long); else WIN_COUNT(MPC_WINDOW_TIME_MINMAX64, float); }
#undef WIN_COUNT
    MPC_LAUNCH(k_ingest_scan, dim3(s->B), dim3(256), 0, st, w.L, out_max);
    MPC_CHECK_LAUNCH();
    return 0;
}

template <int TM, typename XY>
static void win_scatter_launch(const mpc_window_shape *s, const WinHost &w, const void *x, const void *y, const long long *t,
                               const void *p, const int32_t *counts, const float *edges, int max_pos, int max_neg, float *events,
                               int vec, hipStream_t st) {
    const dim3 grid(w.L.nchunks, s->B);
    const size_t lds = TM == MPC_WINDOW_TIME_FP32_SUFFIX ? (size_t)(s->nb + 1) * sizeof(float) : 0;
    if (s->p_int64)
        MPC_LAUNCH((k_window_scatter<TM, XY, long long>), grid, dim3(256), lds, st, *s, w.L, w.first, (const XY *)x, (const XY *)y, t,
                   (const long long *)p, counts, edges, max_pos, max_neg, events, vec);
    else
        MPC_LAUNCH((k_window_scatter<TM, XY, float>), grid, dim3(256), lds, st, *s, w.L, w.first, (const XY *)x, (const XY *)y, t,
                   (const float *)p, counts, edges, max_pos, max_neg, events, vec);
}

extern "C" int mpc_ingest_window_scatter(const mpc_window_shape *s, const void *x, const void *y, const int64_t *t_us, const void *p,
                                         const int32_t *counts, const float *edges, int32_t max_pos, int32_t max_neg, float *events,
                                         void *ws, void *stream) {
    MPC_CHECK_ARG(s && counts && ws && ((x && y && t_us && p) || s->N == 0 || s->B == 0), MPC_E_NULL, "null argument");
    MPC_CHECK_ARG(max_pos >= 0 && max_neg >= 0 && (events || max_pos + max_neg == 0 || s->B == 0), MPC_E_NULL, "events is null");
    int rc = win_validate(s);
    if (rc) return rc;
    MPC_CHECK_ARG(edges || s->time_mode != MPC_WINDOW_TIME_FP32_SUFFIX || s->N == 0 || s->B == 0, MPC_E_NULL, "edges is null");
    MPC_CHECK_ARG(s->split || max_neg == 0, MPC_E_SHAPE, "one block per sample has no negative block");
    if (s->B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t M = (int64_t)max_pos + max_neg;
    if (s->N == 0) return M > 0 ? mpc_zero_async(events, (size_t)s->B * M * 6 * sizeof(float), st) : 0;     // padding rows only
    const WinHost w = win_layout(s, ws);
    const long long *t = reinterpret_cast<const long long *>(t_us);
    const int vec = win_vec(s, x) && win_vec(s, y) && win_vec(s, t_us) && win_vec(s, p);
    if (s->time_mode == MPC_WINDOW_TIME_FP32_SUFFIX) {
        if (s->xy_int) win_scatter_launch<MPC_WINDOW_TIME_FP32_SUFFIX, int>(s, w, x, y, t, p, counts, edges, max_pos, max_neg, events, vec, st);
        else win_scatter_launch<MPC_WINDOW_TIME_FP32_SUFFIX, float>(s, w, x, y, t, p, counts, edges, max_pos, max_neg, events, vec, st);
    } else {
        if (s->xy_int) win_scatter_launch<MPC_WINDOW_TIME_MINMAX64, int>(s, w, x, y, t, p, counts, edges, max_pos, max_neg, events, vec, st);
        else win_scatter_launch<MPC_WINDOW_TIME_MINMAX64, float>(s, w, x, y, t, p, counts, edges, max_pos, max_neg, events, vec, st);
    }
    MPC_CHECK_LAUNCH();
    return 0;
}

MPC_BOUNDS_UNIT("ingest.hip")
