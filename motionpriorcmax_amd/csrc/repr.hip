// Centred voxel grid: the network input of the EVIMO2 and MultiFlow configurations, which the reference's
// DataLoader workers build on the CPU (src/loader/utils/representation.py:26-111 VoxelGrid.convert, :9-18 norm_voxel_grid;
// called from src/loader/evimo2/datasubset.py:146-189 and src/loader/multiflow/sample.py:172-200), with the resize of
// datasubset.py:189 (F.interpolate, bilinear, align_corners=False) fused into the write pass.
//
// Same machinery as voxel.hip: one binning pass appends 16-byte records to per-(sample, channel, row-strip) buckets
// (strip_buckets.h, shared with it), one workgroup per bucket accumulates its strip in LDS as Q33.30 fixed
// point (ds_add_u64: integer sums, any order, bitwise reproducible) and writes it with plain stores; with a normalisation the
// strips are accumulated twice (statistics, then the write) so that the grid is written once and never read back.
//
// What differs from voxel.hip (each changes values):
//   * int64 timestamps and per-sample centres on the device: t_norm = float(t - c0) / float(c1 - c0) * float(C - 1), the two
//     differences in integers (absolute microseconds exceed 2^24), representation.py:58; default centres = first / last valid row;
//   * floor, not truncation, for all three indices (representation.py:82,96-97); events outside [c0, c1] still vote;
//   * integer coordinates: two taps (representation.py:85-94).  The reference has no spatial bounds check there; an event
//     outside the sensor is dropped here;
//   * a strip is a range of OUTPUT rows.  Its LDS holds the input rows [lo, hi) those rows interpolate from; consecutive strips
//     share the rows [lo(s + 1), hi(s)) (one when the grid shrinks, up to two when it grows), and a vote into a shared row is
//     recorded for both strips.  The statistics count every input row once, in the strip that owns it: rows [lo(s), lo(s + 1)).
//     The write pass normalises the four source values as it reads them and stores Ho x Wo rows; the H x W grid never exists in
//     HBM.  Without a resize the same code runs with lo / hi = the strip's own rows.
#include "strip_buckets.h"
#include "resize_src.h"

#define REPR_PER_THREAD 2
#define REPR_SLOTS 6          // buckets one event can vote into: 2 channels x up to 3 strips (rows y0, y0 + 1 across a shared row)
#define REPR_NORM_BLOCKS 256
#define REPR_STAT 6            // doubles per partial statistic

struct ReprGeom {
    int H, W, Ho, Wo;     // Ho x Wo = H x W without a resize
    int SRo, NS;          // output rows per strip, strips
    int resize;
    float sh, sw;         // float(H) / Ho, float(W) / Wo   (area_pixel_compute_scale)
};

struct ReprLayout : StripBuckets {
    double *spart;        // [NBk][REPR_STAT]  partial statistics of the strips: count, sum, sum of squares, smallest, largest non-zero entry
    float *stat;          // [B][4]      mean, std (0: subtract only)
};

// repr_src (source index and weight of output index j along an axis): resize_src.h, shared with flow_targets.hip

// input rows of strip s: held in LDS [lo, hi), owned (statistics) [lo, own_hi); own_hi = lo of the next strip
__host__ __device__ __forceinline__ void repr_strip_rows(const ReprGeom &g, int s, int &lo, int &hi, int &own_hi) {
    int a, b;
    float l;
    lo = 0;
    if (s > 0) { repr_src(g.sh, s * g.SRo, g.H, g.resize, lo, b, l); }
    if (s >= g.NS - 1) { hi = own_hi = g.H; return; }
    repr_src(g.sh, (s + 1) * g.SRo, g.H, g.resize, own_hi, b, l);
    repr_src(g.sh, (s + 1) * g.SRo - 1, g.H, g.resize, a, b, l);
    hi = b + 1 > own_hi ? b + 1 : own_hi;
}

// representation.py:14-17 for one non-zero entry: (v - mean) / std if std > 0 else v - mean
__device__ __forceinline__ float repr_norm(float v, float mean, float sd) {
    const float d = v - mean;
    return sd > 0.f ? d / sd : d;
}

// grid (chunks * B rounded up to 8), 256 threads, dynamic LDS = (3 C NS + 2 NS + 1) ints
__global__ __launch_bounds__(256) void k_repr_bin(const mpc_repr_shape s, const ReprGeom G, const ReprLayout L,
                                                  const float *__restrict__ xs, const float *__restrict__ ys,
                                                  const long long *__restrict__ ts, const float *__restrict__ ps,
                                                  const int *__restrict__ counts, const long long *__restrict__ centres) {
    extern __shared__ int s_cnt[];
    const int chunks = (s.N + 256 * REPR_PER_THREAD - 1) / (256 * REPR_PER_THREAD);
    const int lblk = sb_bin_block(chunks * s.B);
    if (lblk >= chunks * s.B) return;
    const int tid = threadIdx.x, b = lblk / chunks, chunk = lblk - b * chunks;
    const int NS = G.NS, nloc = s.C * NS;
    int *s_base = s_cnt + nloc, *s_spill = s_base + nloc;
    int *s_lo = s_spill + nloc;           // [NS + 1]  first input row of every strip, then H
    int *s_hi = s_lo + NS + 1;            // [NS]      one past the last input row a strip holds
    for (int i = tid; i < nloc; i += 256) s_cnt[i] = 0;
    for (int i = tid; i < NS; i += 256) {
        int lo, hi, own;
        repr_strip_rows(G, i, lo, hi, own);
        s_lo[MPC_IDX(i, NS + 1)] = lo;
        s_hi[MPC_IDX(i, NS)] = hi;
    }
    if (tid == 0) s_lo[NS] = G.H;
    __syncthreads();
    const int n = min(counts[b], s.N);
    const size_t row = (size_t)b * s.N;
    long long c0 = 0, c1 = 1;
    if (centres) { c0 = centres[2 * b]; c1 = centres[2 * b + 1]; }
    else if (n > 0) { c0 = ts[row]; c1 = ts[row + n - 1]; }              // representation.py:78-79
    const float span = (float)(c1 - c0), cm1 = (float)(s.C - 1);
    const float inv_own = (float)NS / (float)G.H;
    float ry[REPR_PER_THREAD], rx[REPR_PER_THREAD], rw[REPR_PER_THREAD][2];
    int bk[REPR_PER_THREAD][REPR_SLOTS], rk[REPR_PER_THREAD][REPR_SLOTS];
#pragma unroll
    for (int k = 0; k < REPR_PER_THREAD; ++k) {
#pragma unroll
        for (int u = 0; u < REPR_SLOTS; ++u) { bk[k][u] = -1; rk[k][u] = 0; }
        ry[k] = rx[k] = rw[k][0] = rw[k][1] = 0.f;
        const int i = (chunk * REPR_PER_THREAD + k) * 256 + tid;
        if (i >= n) continue;
        const float x = xs[row + i], y = ys[row + i], p = ps[row + i];
        const long long t = ts[row + i];
        const float tn = (float)(t - c0) / span * cm1;                    // representation.py:58
        if (!(fabsf(tn) <= 3.0e38f)) continue;                           // c1 == c0: no time axis (the reference asserts c1 > c0 for given centres)
        const int t0 = (int)fminf(fmaxf(floorf(tn), -2.f), (float)s.C + 1.f);      // representation.py:82
        const float val = 2.f * p - 1.f;
        // rows [ya, yb] and columns this event votes into
        int ya, yb;
        if (s.int_xy) {
            const int xi = (int)fminf(fmaxf(x, -8.f), (float)G.W + 8.f);
            ya = yb = (int)fminf(fmaxf(y, -8.f), (float)G.H + 8.f);
            if (xi < 0 || xi >= G.W || ya < 0 || ya >= G.H) continue;      // outside the sensor: dropped
            if ((float)xi != x || (float)ya != y) continue;              // not an integer (NaN included): not this path's input
        } else {
            const int x0 = (int)floorf(fminf(fmaxf(x, -8.f), (float)G.W + 8.f));      // representation.py:96-97
            if (x0 + 1 < 0 || x0 >= G.W) continue;                       // no column inside the sensor
            ya = (int)floorf(fminf(fmaxf(y, -8.f), (float)G.H + 8.f));
            yb = min(ya + 1, G.H - 1);
            ya = max(ya, 0);
            if (ya > yb) continue;
        }
        ry[k] = y; rx[k] = x;
        // owner strip of row ya (s_lo[sa] <= ya < s_lo[sa + 1]); the strips that hold ya or yb are consecutive
        int sa = min((int)(((float)ya + 0.5f) * inv_own), NS - 1);
        while (sa > 0 && ya < s_lo[MPC_IDX(sa, NS + 1)]) --sa;
        while (sa < NS - 1 && ya >= s_lo[MPC_IDX(sa + 1, NS + 1)]) ++sa;
        const int s_first = (sa > 0 && ya < s_hi[MPC_IDX(sa - 1, NS)]) ? sa - 1 : sa;
        const int s_last = (sa < NS - 1 && yb >= s_lo[MPC_IDX(sa + 1, NS + 1)]) ? sa + 1 : sa;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            const int tl = t0 + dt;
            if (tl < 0 || tl >= s.C) continue;
            rw[k][dt] = val * (1.f - fabsf((float)tl - tn));
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int st = s_first + u;
                if (st > s_last) continue;
                const int lb = tl * NS + st;
                bk[k][dt * 3 + u] = lb;
                rk[k][dt * 3 + u] = atomicAdd(&s_cnt[MPC_IDX(lb, nloc)], 1);
            }
        }
    }
    __syncthreads();
    sb_reserve(L, b, nloc, s_cnt, s_base, s_spill);
#pragma unroll
    for (int k = 0; k < REPR_PER_THREAD; ++k)
#pragma unroll
        for (int u = 0; u < REPR_SLOTS; ++u)
            if (bk[k][u] >= 0) sb_store(L, b, nloc, bk[k][u], rk[k][u], ry[k], rx[k], rw[k][u / 3], s_base, s_spill);
}

// the taps of one record that fall into the rows [lo, hi) of a strip, added to its LDS accumulators
__device__ __forceinline__ void repr_vote(unsigned long long *s_acc, const float4 e, int int_xy, int H, int W, int lo, int hi, int npix) {
    if (int_xy) {
        const int yy = (int)e.x, xx = (int)e.y;
        if (yy < lo || yy >= hi || xx < 0 || xx >= W) return;
        atomicAdd(&s_acc[MPC_IDX((yy - lo) * W + xx, npix)], (unsigned long long)mpc_to_fixed(e.z));
        return;
    }
    const int y0 = (int)floorf(fminf(fmaxf(e.x, -8.f), (float)H + 8.f)), x0 = (int)floorf(fminf(fmaxf(e.y, -8.f), (float)W + 8.f));
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
        const int xx = x0 + dx;
        if (xx < 0 || xx >= W) continue;
        const float wx = 1.f - fabsf((float)xx - e.y);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int yy = y0 + dy;
            if (yy < lo || yy >= hi) continue;
            const float wy = 1.f - fabsf((float)yy - e.x);
            // value * wx * wy * wt left to right (representation.py:103); value = +-1 commutes exactly
            atomicAdd(&s_acc[MPC_IDX((yy - lo) * W + xx, npix)], (unsigned long long)mpc_to_fixed((wx * wy) * e.z));
        }
    }
}

// grid NBk, 1024 threads, dynamic LDS = (rows of the largest strip) * W * 8.  One strip of one channel image.
//   MODE 0: written as it is (resized if asked)     MODE 1: nothing written, the statistics of the rows the strip owns -> spart[g]
//   MODE 2: written normalised with the sample's (mean, 1 / std) from k_repr_finalize (resized if asked)
template <int MODE>
__global__ __launch_bounds__(1024) void k_repr_accum(const ReprGeom G, const ReprLayout L, float *__restrict__ grid, int C, int int_xy, int lds_pix) {
    extern __shared__ unsigned long long s_acc[];
    __shared__ double s_red[3][16];
    const int tid = threadIdx.x;
    const int g = blockIdx.x, img = g / G.NS, strip = g - img * G.NS;
    const int H = G.H, W = G.W;
    int lo, hi, own_hi;
    repr_strip_rows(G, strip, lo, hi, own_hi);
    const int npix = (hi - lo) * W;
    MPC_EXPECT(npix <= lds_pix);
    // The host sized the dynamic LDS with the SAME repr_strip_rows (one function, __host__ __device__, IEEE single, no contraction:
    // -ffp-contract=off in build.py), so this cannot differ; if a compile flag ever made host and device round repr_src differently,
    // the strip would not fit and is written as NaN rather than left unwritten or overrun (the header promises every element written)
    if (npix > lds_pix) {
        if (MODE != 1) {
            const int o0 = strip * G.SRo, o1 = min(o0 + G.SRo, G.Ho);
            float *dst = grid + ((size_t)img * G.Ho + o0) * G.Wo;
            for (int i = tid; i < (o1 - o0) * G.Wo; i += 1024) dst[i] = NAN;
        }
        return;
    }
    for (int i = tid; i < npix; i += 1024) s_acc[i] = 0ull;
    __syncthreads();
    sb_drain(L, g, C * G.NS, [&](const float4 e) { repr_vote(s_acc, e, int_xy, H, W, lo, hi, npix); });
    __syncthreads();
    if (MODE == 1) {
        // per-thread partials in fp32 (a thread sees ~10 entries), everything above them in fp64
        const int nown = (own_hi - lo) * W;
        int cnt = 0;
        float sum = 0.f, sq = 0.f, mn = INFINITY, mx = -INFINITY;
        for (int i = tid; i < nown; i += 1024) {
            const float v = mpc_from_fixed((long long)s_acc[MPC_IDX(i, npix)]);
            if (v != 0.f) { ++cnt; sum += v; sq = fmaf(v, v, sq); mn = fminf(mn, v); mx = fmaxf(mx, v); }
        }
        const double r0 = block_sum_d<1024>((double)cnt, s_red[0]);
        const double r1 = block_sum_d<1024>((double)sum, s_red[1]);
        const double r2 = block_sum_d<1024>((double)sq, s_red[2]);
        const double r3 = block_min_d<1024>((double)mn, s_red[0]);
        const double r4 = block_max_d<1024>((double)mx, s_red[1]);
        if (tid == 0) {
            double *p = L.spart + (size_t)MPC_IDX(g, L.NBk) * REPR_STAT;
            p[0] = r0; p[1] = r1; p[2] = r2; p[3] = r3; p[4] = r4; p[5] = 0.0;
        }
        return;
    }
    float sub = 0.f, sd = 0.f;                               // the sample's mean and std (0: subtract only)
    if (MODE == 2) { const int b = img / C; sub = L.stat[b * 4 + 0]; sd = L.stat[b * 4 + 1]; }
    auto value = [&](int yy, int xx) -> float {              // entry (yy, xx) of the (normalised) full-size grid (representation.py:14-17)
        float v = mpc_from_fixed((long long)s_acc[MPC_IDX((yy - lo) * W + xx, npix)]);
        if (MODE == 2 && v != 0.f) v = repr_norm(v, sub, sd);
        return v;
    };
    if (!G.resize) {
        float *dst = grid + ((size_t)img * H + lo) * W;
        const int nown = (own_hi - lo) * W;
        for (int i = tid; i < nown; i += 1024) {
            float v = mpc_from_fixed((long long)s_acc[MPC_IDX(i, npix)]);
            if (MODE == 2 && v != 0.f) v = repr_norm(v, sub, sd);
            dst[i] = v;
        }
        return;
    }
    const int Wo = G.Wo, o0 = strip * G.SRo, o1 = min(o0 + G.SRo, G.Ho);
    auto pixel = [&](int j, int i) -> float {                // output (j, i): upsample_bilinear2d, rows combined last
        int y0, y1, x0, x1;
        float ly, lx;
        repr_src(G.sh, j, H, 1, y0, y1, ly);
        repr_src(G.sw, i, W, 1, x0, x1, lx);
        MPC_EXPECT(y0 >= lo && y1 < hi);
        const float top = (1.f - lx) * value(y0, x0) + lx * value(y0, x1);
        const float bot = (1.f - lx) * value(y1, x0) + lx * value(y1, x1);
        return (1.f - ly) * top + ly * bot;
    };
    float *dst = grid + ((size_t)img * G.Ho + o0) * Wo;
    const int nout = (o1 - o0) * Wo;
    if ((Wo & 3) == 0 && (reinterpret_cast<uintptr_t>(grid) & 15) == 0) {          // 16-byte stores
        for (int q = tid; q < (nout >> 2); q += 1024) {
            const int j = (q << 2) / Wo, i = (q << 2) - j * Wo;
            float4 o;
            o.x = pixel(o0 + j, i); o.y = pixel(o0 + j, i + 1); o.z = pixel(o0 + j, i + 2); o.w = pixel(o0 + j, i + 3);
            reinterpret_cast<float4 *>(dst)[q] = o;
        }
    } else {
        for (int q = tid; q < nout; q += 1024) { const int j = q / Wo; dst[q] = pixel(o0 + j, q - j * Wo); }
    }
}

// one workgroup per sample: mean and std of the non-zero entries (unbiased, torch.std) from nblk partials.  std == 0 is decided
// exactly: all non-zero entries are equal iff the smallest equals the largest (the cancellation s2 - n mean^2 of rounded sums can
// leave a tiny positive variance there, and a division by it would blow the grid up where the reference subtracts only)
__global__ __launch_bounds__(256) void k_repr_finalize(const double *__restrict__ part, float *__restrict__ stat, int nblk) {
    __shared__ double s_red[3][4];
    const int b = blockIdx.x;
    double cnt = 0.0, sum = 0.0, sq = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < nblk; i += 256) {
        const double *p = part + ((size_t)b * nblk + i) * REPR_STAT;
        cnt += p[0]; sum += p[1]; sq += p[2]; mn = fmin(mn, p[3]); mx = fmax(mx, p[4]);
    }
    const double n = block_sum_d<256>(cnt, s_red[0]);
    const double s1 = block_sum_d<256>(sum, s_red[1]);
    const double s2 = block_sum_d<256>(sq, s_red[2]);
    const double lo = block_min_d<256>(mn, s_red[0]);
    const double hi = block_max_d<256>(mx, s_red[1]);
    if (threadIdx.x == 0) {
        float sub = 0.f, sd = 0.f;
        if (n > 0.0) {                                        // representation.py:11-17
            const double mean = s1 / n;
            const double var = (n > 1.0 && hi > lo) ? (s2 - n * mean * mean) / (n - 1.0) : 0.0;
            sub = (float)mean;
            sd = var > 0.0 ? (float)sqrt(var) : 0.f;          // std == 0, or NaN for a single entry: only subtract (:16-17)
        }
        stat[b * 4 + 0] = sub;
        stat[b * 4 + 1] = sd;
    }
}

// norm_voxel_grid of a grid that already lies in memory: grid (REPR_NORM_BLOCKS, B), 256 threads
__global__ __launch_bounds__(256) void k_repr_gstats(const float *__restrict__ grid, double *__restrict__ part, int64_t per_sample) {
    __shared__ double s_red[3][4];
    const float *g = grid + (size_t)blockIdx.y * per_sample;
    double cnt = 0.0, sum = 0.0, sq = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_sample; i += (int64_t)gridDim.x * 256) {
        const float v = g[i];
        if (v != 0.f) { cnt += 1.0; sum += (double)v; sq += (double)v * (double)v; mn = fmin(mn, (double)v); mx = fmax(mx, (double)v); }
    }
    const double r0 = block_sum_d<256>(cnt, s_red[0]);
    const double r1 = block_sum_d<256>(sum, s_red[1]);
    const double r2 = block_sum_d<256>(sq, s_red[2]);
    const double r3 = block_min_d<256>(mn, s_red[0]);
    const double r4 = block_max_d<256>(mx, s_red[1]);
    if (threadIdx.x == 0) {
        double *p = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * REPR_STAT;
        p[0] = r0; p[1] = r1; p[2] = r2; p[3] = r3; p[4] = r4; p[5] = 0.0;
    }
}

__global__ __launch_bounds__(256) void k_repr_gnorm(float *__restrict__ grid, const float *__restrict__ stat, int64_t per_sample) {
    const int b = blockIdx.y;
    const float sub = stat[b * 4 + 0], sd = stat[b * 4 + 1];
    float *g = grid + (size_t)b * per_sample;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_sample; i += (int64_t)gridDim.x * 256) {
        const float v = g[i];
        if (v != 0.f) g[i] = repr_norm(v, sub, sd);
    }
}

// ------------------------------------------------------------------------------------------
struct ReprHostLayout { ReprGeom G; ReprLayout L; int lds_rows; int64_t total; };

static int repr_max_rows(const ReprGeom &G) {
    int m = 0;
    for (int s = 0; s < G.NS; ++s) {
        int lo, hi, own;
        repr_strip_rows(G, s, lo, hi, own);
        if (hi - lo > m) m = hi - lo;
    }
    return m;
}

// strips of output rows whose input rows fit `budget` bytes of LDS; false if not even one output row does
static bool repr_geometry(const mpc_repr_shape *s, int64_t budget, ReprGeom &G, int &rows) {
    G.H = s->H; G.W = s->W;
    G.resize = (s->Ho > 0);
    G.Ho = G.resize ? s->Ho : s->H;
    G.Wo = G.resize ? s->Wo : s->W;
    G.sh = (float)G.H / (float)G.Ho;
    G.sw = (float)G.W / (float)G.Wo;
    const int64_t fit = budget / ((int64_t)s->W * 8);               // input rows the budget holds
    if (fit < 1) return false;
    int64_t sro = G.resize ? (fit * G.Ho) / G.H : fit;
    if (sro > G.Ho) sro = G.Ho;
    if (sro < 1) sro = 1;
    for (; sro >= 1; --sro) {
        G.NS = mpc_cdiv(G.Ho, sro);
        G.SRo = mpc_cdiv(G.Ho, G.NS);
        rows = repr_max_rows(G);
        if (rows <= fit) return true;
    }
    return false;
}

static int repr_validate(const mpc_repr_shape *s, ReprGeom *Gout, int *rows_out) {
    MPC_CHECK_ARG(s->B >= 0 && s->N >= 0 && s->C >= 1 && s->H >= 1 && s->W >= 1 && s->Ho >= 0 && s->Wo >= 0, MPC_E_SHAPE, "bad shape");
    MPC_CHECK_ARG((s->Ho == 0) == (s->Wo == 0), MPC_E_SHAPE, "Ho and Wo must both be 0 (no resize) or both be positive");
    MPC_CHECK_ARG((s->int_xy == 0 || s->int_xy == 1) && (s->norm == 0 || s->norm == 1), MPC_E_SHAPE, "int_xy and norm must be 0 or 1");
    MPC_CHECK_ARG(s->C >= 2 && s->H >= 2 && s->W >= 2, MPC_E_UNSUPPORTED, "channels, height and width must exceed 1 (representation.py:28-30)");
    MPC_CHECK_ARG((int64_t)s->B * s->N < (1LL << 31), MPC_E_UNSUPPORTED, "too many events");
    MPC_CHECK_ARG((int64_t)s->B * s->C * (s->Ho > 0 ? s->Ho : s->H) * (s->Ho > 0 ? s->Wo : s->W) < (1LL << 31) && (int64_t)s->H * s->W < (1LL << 28),
                  MPC_E_UNSUPPORTED, "voxel grid too large");
    ReprGeom G;
    int rows = 0;
    bool ok = repr_geometry(s, (int64_t)REPR_STRIP_KB * 1024, G, rows);
    if (!ok) ok = repr_geometry(s, 150 * 1024, G, rows);
    MPC_CHECK_ARG(ok, MPC_E_UNSUPPORTED, "the input rows of one output row do not fit the LDS (sensor too wide, or shrunk too far)");
    // what the binning pass relies on: every strip owns a row, and a row is held by at most two strips
    for (int st = 0; st < G.NS; ++st) {
        int lo, hi, own, lo2 = G.H, hi2, own2;
        repr_strip_rows(G, st, lo, hi, own);
        if (st + 2 < G.NS) repr_strip_rows(G, st + 2, lo2, hi2, own2);
        MPC_CHECK_ARG(own > lo && hi <= lo2 && hi <= G.H, MPC_E_UNSUPPORTED, "resize factor too large for the strip layout");
    }
    MPC_CHECK_ARG(((int64_t)s->C * G.NS * 3 + 2 * G.NS + 1) * 4 <= 60 * 1024 && (int64_t)s->B * s->C * G.NS < (1LL << 30), MPC_E_UNSUPPORTED,
                  "too many (channel, strip) buckets for the binning pass");
    if (Gout) *Gout = G;
    if (rows_out) *rows_out = rows;
    return 0;
}

static ReprHostLayout repr_layout(const mpc_repr_shape *s, const ReprGeom &G, int rows, void *ws) {
    ReprHostLayout h;
    h.G = G;
    h.lds_rows = rows;
    ReprLayout &L = h.L;
    // an event votes into two channels x up to three strips; an integer pixel has one row, in at most two strips
    int64_t off = sb_layout(L, s->B, s->N, (int64_t)s->C * G.NS, s->int_xy ? 4 : REPR_SLOTS, 256 * REPR_PER_THREAD, ws);
    L.spart = sb_take<double>(ws, off, (int64_t)(L.NBk > 0 ? L.NBk : 1) * REPR_STAT * 8);
    L.stat = sb_take<float>(ws, off, (int64_t)(s->B > 0 ? s->B : 1) * 4 * 4);
    h.total = off;
    return h;
}

extern "C" int64_t mpc_repr_workspace_bytes(const mpc_repr_shape *s) {
    if (!s) { mpc_set_error("mpc_repr_workspace_bytes: null shape"); return MPC_E_NULL; }
    ReprGeom G;
    int rows;
    int rc = repr_validate(s, &G, &rows);
    if (rc) return rc;
    MPC_CHECK_ARG((int64_t)s->N * REPR_SLOTS < (1LL << 31), MPC_E_UNSUPPORTED, "too many events per sample");
    return repr_layout(s, G, rows, nullptr).total;
}

extern "C" int mpc_repr_grid(const mpc_repr_shape *s, const float *x, const float *y, const int64_t *time, const float *pol,
                             const int32_t *counts, const int64_t *centres, float *grid, void *ws, void *stream) {
    MPC_CHECK_ARG(s && counts && grid && ws && ((x && y && time && pol) || s->N == 0 || s->B == 0), MPC_E_NULL, "null argument");
    ReprGeom G;
    int rows;
    int rc = repr_validate(s, &G, &rows);
    if (rc) return rc;
    MPC_CHECK_ARG((int64_t)s->N * REPR_SLOTS < (1LL << 31), MPC_E_UNSUPPORTED, "too many events per sample");
    if (s->B == 0) return 0;
    const ReprHostLayout h = repr_layout(s, G, rows, ws);
    const ReprLayout &L = h.L;
    hipStream_t st = (hipStream_t)stream;
    static mpc_device_once attr_once;
    rc = mpc_raise_lds_cap(attr_once, __func__, SB_LDS_CAP, {(const void *)k_repr_accum<0>, (const void *)k_repr_accum<1>, (const void *)k_repr_accum<2>});
    if (!rc) rc = sb_zero_counters(L, s->B, st);
    if (rc) return rc;
    if (s->N > 0) {
        const int nblk = mpc_cdiv(s->N, 256 * REPR_PER_THREAD) * s->B;
        const size_t bin_lds = ((size_t)s->C * G.NS * 3 + 2 * G.NS + 1) * sizeof(int);
        MPC_LAUNCH(k_repr_bin, dim3(((nblk + 7) / 8) * 8), dim3(256), bin_lds, st, *s, G, L, x, y,
                   reinterpret_cast<const long long *>(time), pol, counts, reinterpret_cast<const long long *>(centres));
        MPC_CHECK_LAUNCH();
    }
    const int lds_pix = rows * s->W;
    const size_t strip_lds = (size_t)lds_pix * 8;
    if (s->norm) {
        MPC_LAUNCH(k_repr_accum<1>, dim3(L.NBk), dim3(1024), strip_lds, st, G, L, grid, s->C, s->int_xy, lds_pix);
        MPC_LAUNCH(k_repr_finalize, dim3(s->B), dim3(256), 0, st, L.spart, L.stat, s->C * G.NS);
        MPC_LAUNCH(k_repr_accum<2>, dim3(L.NBk), dim3(1024), strip_lds, st, G, L, grid, s->C, s->int_xy, lds_pix);
    } else {
        MPC_LAUNCH(k_repr_accum<0>, dim3(L.NBk), dim3(1024), strip_lds, st, G, L, grid, s->C, s->int_xy, lds_pix);
    }
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t mpc_repr_norm_workspace_bytes(int32_t B) {
    if (B < 0) { mpc_set_error("mpc_repr_norm_workspace_bytes: negative batch"); return MPC_E_SHAPE; }
    return mpc_align((int64_t)(B > 0 ? B : 1) * REPR_NORM_BLOCKS * REPR_STAT * 8) + mpc_align((int64_t)(B > 0 ? B : 1) * 4 * 4);
}

extern "C" int mpc_repr_norm(float *grid, int32_t B, int64_t per_sample, void *ws, void *stream) {
    MPC_CHECK_ARG(B >= 0 && per_sample >= 0, MPC_E_SHAPE, "bad shape");
    if (B == 0 || per_sample == 0) return 0;
    MPC_CHECK_ARG(grid && ws, MPC_E_NULL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)ws;
    float *stat = (float *)((char *)ws + mpc_align((int64_t)B * REPR_NORM_BLOCKS * REPR_STAT * 8));
    MPC_LAUNCH(k_repr_gstats, dim3(REPR_NORM_BLOCKS, B), dim3(256), 0, st, grid, part, per_sample);
    MPC_LAUNCH(k_repr_finalize, dim3(B), dim3(256), 0, st, part, stat, REPR_NORM_BLOCKS);
    MPC_LAUNCH(k_repr_gnorm, dim3(REPR_NORM_BLOCKS, B), dim3(256), 0, st, grid, stat, per_sample);
    MPC_CHECK_LAUNCH();
    return 0;
}

MPC_BOUNDS_UNIT("repr.hip")
