// RAFT-spline correlation lookup: the one gather inside the network's update loop (12 times per forward).
//   reference: src/models/raft_spline/corr.py:304-348 (CorrBlockParallelMultiTarget.__call__), raft_spline/utils.py:4-20
//   (bilinear_sampler), raft.py:165-189 (flows = bezier.get_flow_from_reference(times); coords1 = coords0 + flows; corr_block(coords1)).
// For the query q = (b, y, x), the entry e = (level l, slot k) with target t = level_target[l][k], K = 2R + 1:
//   (cx, cy) = coords[t][b][:, y, x]   or, coords == NULL,   (x, y) + sum_j basis[t][j] * params[b][(j, d + j)][y][x]
//   sx = cx / 2^l, sy = cy / 2^l, x0 = floor(sx), fx = sx - x0 (exact in fp32 but for -0.5 < sx < 0: rounded there, by <= 2^-25, up to 1.0f), y0, fy likewise
//   out[b][e * K * K + i * K + j][y][x] = w00 V[i][j] + w01 V[i][j + 1] + w10 V[i + 1][j] + w11 V[i + 1][j + 1]
//   V[a][c] = level[l][k][q][y0 - R + a][x0 - R + c] (0 outside the slice), w00 = (1 - fx)(1 - fy), w01 = fx (1 - fy), w10 = (1 - fx) fy, w11 = fx fy
// In plain torch this is a [n * B * h * w, K, K, 2] coordinate tensor built by half a dozen elementwise operators, its normalisation to
// [-1, 1], a grid_sample with four loads per sample, and cat / permute / reshape.  The offsets are integers, so the K * K samples of a
// (query, entry) share ONE pair of fractions and read ONE (K + 1)^2 window of the query's own slice; the sample coordinate is formed
// directly, without the round trip through [-1, 1].
//   k_corr_lookup_fwd<R>        a workgroup takes 64 consecutive queries of one (sample, entry).  A wave first loads the windows of its 16
//                               queries, lanes over the (K + 1)^2 cells (row pieces of K + 1 floats; 2 loads per lane and query, all 32
//                               in flight), then forms the K * K outputs of each from the shared fractions through a per-wave LDS
//                               window; the [K * K][64] tile leaves through LDS (row pitch 65: 21 KB at R = 4), so that every store
//                               is coalesced along w.
//   k_corr_lookup_fwd_lane<R>   MPC_CORR_F_LANE_PER_QUERY: one thread per (query, entry), the window streams through two register rows
//                               (scattered 4-byte loads, no LDS).  The mapping that lost the A/B of tools/corr_lookup_probe.py (figures
//                               in DESIGN.md section 7); kept for that probe, the same expression per output and so the same bits.
//   k_corr_lookup_bwd<R>        workgroups [0, nA): 64 consecutive queries of a sample, the E entries dealt to the four waves: the window
//                               again (lane per query), 2^-l * sum over (i, j) in index order of g * d(bilinear)/d(fraction) per entry
//                               into LDS; then grad centre[t] = the sum over the entries of t, levels ascending; coords mode writes
//                               grad_coords, the Bezier mode the same workgroup's grad_params[c] = sum_t basis[t][j] * grad centre[t]
//                               (t in index order).  Workgroups [nA, ..): a wave per (level that wants a gradient, slot, query) writes
//                               the WHOLE slice of grad_level: a window cell gathers its up to four cotangents, every other element is
//                               0 (no memset, no atomics: another query never touches this slice); 16-byte stores where w_l % 4 == 0.
//   k_corr_lookup_bwd<R, 1>     MPC_CORR_F_GRAD_ACCUM: the centre role as above; workgroups [nA, ..) ADD into grad_level instead of writing
//                               it (the 12 lookups of a forward share one gradient buffer: ops.CorrLookupSharedFn).  The forward's mapping
//                               run backwards: a workgroup takes 64 consecutive queries of one (level that wants a gradient, slot, sample);
//                               their [K * K][64] cotangent tile enters LDS through coalesced loads, a wave forms the (K + 1)^2 cell
//                               gradients of its 16 queries in registers (lanes over the cells, the fill's four-term sum), THEN loads the
//                               in-slice window cells of all 16 (row pieces of K + 1 floats, all loads in flight), adds once and stores:
//                               work and traffic follow the windows, every other element of the slice is left as it is.
// Sums run in index order with one rounding per multiply and per add (-ffp-contract=off): bitwise reproducible.
#include <algorithm>
#include "common.h"
#include "bounds.h"

#define CORR_COORD_LIMIT 1048576.f        // |sample coordinate| is clamped here before the conversion to int (NaN -> -limit): such a window lies outside

struct corr_frac { int x0, y0; float fx, fy; };
typedef float corr_v4f __attribute__((ext_vector_type(4)));

// entry e -> (level, slot): entries are level-major
__device__ __forceinline__ void corr_entry(const mpc_corr_desc &D, int e, int &l, int &k) {
    l = 0; k = e;
    while (l < D.num_levels - 1 && k >= D.level_n[l]) { k -= D.level_n[l]; ++l; }
}

// centre of target t at pixel pix = y * w + x of sample b; brow: row t of the basis (Bezier mode)
__device__ __forceinline__ float2 corr_centre(const mpc_corr_desc &D, const float *__restrict__ coords, const float *__restrict__ params,
                                              const float *brow, int t, int b, int pix, size_t hw) {
    if (coords) {
        const float *c = coords + ((size_t)t * D.B + b) * 2 * hw + pix;
        return make_float2(c[0], c[hw]);
    }
    const int y = pix / D.w, x = pix - y * D.w;
    const float *p = params + (size_t)b * 2 * D.d * hw + pix;
    float fx = 0.f, fy = 0.f;
    for (int j = 0; j < D.d; ++j) {
        const float bw = brow[j];
        fx = fx + bw * p[(size_t)j * hw];
        fy = fy + bw * p[(size_t)(D.d + j) * hw];
    }
    return make_float2((float)x + fx, (float)y + fy);
}

__device__ __forceinline__ corr_frac corr_split(float2 c, float inv) {
    corr_frac f;
    const float sx = fminf(fmaxf(c.x * inv, -CORR_COORD_LIMIT), CORR_COORD_LIMIT);        // (c * 2^-l is exact)
    const float sy = fminf(fmaxf(c.y * inv, -CORR_COORD_LIMIT), CORR_COORD_LIMIT);
    const float flx = floorf(sx), fly = floorf(sy);
    f.x0 = (int)flx; f.y0 = (int)fly;
    f.fx = sx - flx; f.fy = sy - fly;
    return f;
}

template <int R>
__global__ __launch_bounds__(256) void k_corr_lookup_fwd_lane(const mpc_corr_desc D, const float *__restrict__ coords,
                                                         const float *__restrict__ params, const float *__restrict__ basis,
                                                         float *__restrict__ out, int chunks, int E) {
    extern __shared__ float s_brow[];          // [d]: the basis row of this workgroup's target (Bezier mode)
    constexpr int K = 2 * R + 1, WN = 2 * R + 2;
    const size_t hw = (size_t)D.h * D.w;
    int bid = blockIdx.x;
    const int chunk = bid % chunks; bid /= chunks;
    const int e = bid % E, b = bid / E;
    int l, k;
    corr_entry(D, e, l, k);
    const int t = D.level_target[l][k];
    const int hl = D.level_h[l], wl = D.level_w[l];
    if (!coords) {
        for (int i = threadIdx.x; i < D.d; i += 256) s_brow[MPC_IDX(i, D.d)] = basis[t * D.d + i];
        __syncthreads();
    }
    const size_t pix = (size_t)chunk * 256 + threadIdx.x;
    if (pix >= hw) return;
    const corr_frac f = corr_split(corr_centre(D, coords, params, s_brow, t, b, (int)pix, hw), 1.f / (float)(1 << l));
    const float w00 = (1.f - f.fx) * (1.f - f.fy), w01 = f.fx * (1.f - f.fy), w10 = (1.f - f.fx) * f.fy, w11 = f.fx * f.fy;
    const size_t nq = (size_t)D.B * hw, q = (size_t)b * hw + pix, sl = (size_t)hl * wl;
    const float *slice = D.level[l] + ((size_t)k * nq + q) * sl;
    float *o = out + ((size_t)b * E + e) * (K * K) * hw + pix;
    float prev[WN], cur[WN];
#pragma unroll
    for (int i = 0; i < WN; ++i) {
        const int yy = f.y0 - R + i;
        const bool rowin = yy >= 0 && yy < hl;
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int xx = f.x0 - R + j;
            cur[j] = (rowin && xx >= 0 && xx < wl) ? slice[MPC_IDX((size_t)yy * wl + xx, sl)] : 0.f;
        }
        if (i > 0) {
#pragma unroll
            for (int j = 0; j < K; ++j)
                o[(size_t)((i - 1) * K + j) * hw] = ((prev[j] * w00 + prev[j + 1] * w01) + cur[j] * w10) + cur[j + 1] * w11;
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) prev[j] = cur[j];
    }
}

#define CORR_TILE_LD 65        // row pitch of the [K * K][64] output tile in LDS: consecutive channels fall into consecutive banks

template <int R>
__global__ __launch_bounds__(256) void k_corr_lookup_fwd(const mpc_corr_desc D, const float *__restrict__ coords,
                                                              const float *__restrict__ params, const float *__restrict__ basis,
                                                              float *__restrict__ out, int chunks, int E) {
    extern __shared__ float s_mem[];           // [K * K][65] tile | [4][WN * WN] windows | [64] x0 | [64] y0 | [64] fx | [64] fy | [d] basis row
    constexpr int K = 2 * R + 1, WN = 2 * R + 2, NT = K * K * CORR_TILE_LD, NW = WN * WN;
    float *s_tile = s_mem, *s_win = s_mem + NT, *s_fx = s_win + 4 * NW + 128, *s_fy = s_fx + 64, *s_brow = s_fy + 64;
    int *s_x0 = reinterpret_cast<int *>(s_win + 4 * NW), *s_y0 = s_x0 + 64;
    const size_t hw = (size_t)D.h * D.w;
    int bid = blockIdx.x;
    const int chunk = bid % chunks; bid /= chunks;
    const int e = bid % E, b = bid / E;
    int l, k;
    corr_entry(D, e, l, k);
    const int t = D.level_target[l][k];
    const int hl = D.level_h[l], wl = D.level_w[l];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!coords) {
        for (int i = threadIdx.x; i < D.d; i += 256) s_brow[MPC_IDX(i, D.d)] = basis[t * D.d + i];
        __syncthreads();
    }
    const size_t pix0 = (size_t)chunk * 64;
    if (threadIdx.x < 64) {
        corr_frac f = {0, 0, 0.f, 0.f};
        if (pix0 + lane < hw) f = corr_split(corr_centre(D, coords, params, s_brow, t, b, (int)(pix0 + lane), hw), 1.f / (float)(1 << l));
        s_x0[MPC_IDX(lane, 64)] = f.x0; s_y0[MPC_IDX(lane, 64)] = f.y0; s_fx[MPC_IDX(lane, 64)] = f.fx; s_fy[MPC_IDX(lane, 64)] = f.fy;
    }
    __syncthreads();
    const size_t nq = (size_t)D.B * hw, sl = (size_t)hl * wl;
    const float *lvl = D.level[l] + ((size_t)k * nq + (size_t)b * hw + pix0) * sl;
    // every window of this wave's 16 queries into registers first: 32 loads in flight per lane
    float v[16][2];
#pragma unroll
    for (int qi = 0; qi < 16; ++qi) {
        const int ql = wv * 16 + qi;
        const int x0 = s_x0[MPC_IDX(ql, 64)], y0 = s_y0[MPC_IDX(ql, 64)];
        const bool live = pix0 + ql < hw;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int c = lane + 64 * p, ci = c / WN, cj = c - ci * WN;
            const int yy = y0 - R + ci, xx = x0 - R + cj;
            v[qi][p] = (live && c < NW && yy >= 0 && yy < hl && xx >= 0 && xx < wl) ? lvl[(size_t)ql * sl + MPC_IDX((size_t)yy * wl + xx, sl)] : 0.f;
        }
    }
    float *win = s_win + wv * NW;
#pragma unroll
    for (int qi = 0; qi < 16; ++qi) {
        const int ql = wv * 16 + qi;
        const float fx = s_fx[MPC_IDX(ql, 64)], fy = s_fy[MPC_IDX(ql, 64)];
        const float w00 = (1.f - fx) * (1.f - fy), w01 = fx * (1.f - fy), w10 = (1.f - fx) * fy, w11 = fx * fy;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int c = lane + 64 * p;
            if (c < NW) win[MPC_IDX(c, NW)] = v[qi][p];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int c = lane + 64 * p;
            if (c < K * K) {
                const int i = c / K, j = c - i * K;
                const float *a = win + MPC_IDX(i * WN + j, NW - WN - 1);
                s_tile[MPC_IDX(c * CORR_TILE_LD + ql, NT)] = ((a[0] * w00 + a[1] * w01) + a[WN] * w10) + a[WN + 1] * w11;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
    if (pix0 + lane >= hw) return;
    float *o = out + ((size_t)b * E + e) * (K * K) * hw + pix0 + lane;
    for (int c = wv; c < K * K; c += 4) o[(size_t)c * hw] = s_tile[MPC_IDX(c * CORR_TILE_LD + lane, NT)];
}

// the cotangent a window cell (ci, cj) gathers: output (i, j) reads the cells (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1) with
// w00, w01, w10, w11 -- so the cell is read by the outputs (ci, cj), (ci, cj - 1), (ci - 1, cj), (ci - 1, cj - 1), added in this order
template <int R>
__device__ __forceinline__ float corr_cell_grad(const float *__restrict__ g, size_t hw, int ci, int cj, float w00, float w01, float w10, float w11) {
    constexpr int K = 2 * R + 1, WN = 2 * R + 2;
    float v = 0.f;
    if (ci >= 0 && ci < WN && cj >= 0 && cj < WN) {
        if (ci < K && cj < K) v = v + g[(size_t)(ci * K + cj) * hw] * w00;
        if (ci < K && cj >= 1) v = v + g[(size_t)(ci * K + cj - 1) * hw] * w01;
        if (ci >= 1 && cj < K) v = v + g[(size_t)((ci - 1) * K + cj) * hw] * w10;
        if (ci >= 1 && cj >= 1) v = v + g[(size_t)((ci - 1) * K + cj - 1) * hw] * w11;
    }
    return v;
}

// MPC_CORR_F_GRAD_ACCUM, workgroups [nA, ..): fb-th workgroup of the role -> 64 consecutive queries of one (level that wants a gradient,
// slot, sample).  No load of the read-modify-write stream waits behind a store: the cell gradients are in registers before its first
// load, and every load of a wave is issued before its first store (loads and stores share one in-order counter).
template <int R>
__device__ __forceinline__ void corr_bwd_accum(const mpc_corr_desc &D, const float *__restrict__ coords, const float *__restrict__ params,
                                               const float *__restrict__ basis, const float *__restrict__ grad_out, float *s_mem,
                                               long long fb, int chunks, int E) {
    // [K * K][65] cotangent tile | [64] x0 | [64] y0 | [64] fx | [64] fy | [d] basis row
    constexpr int K = 2 * R + 1, WN = 2 * R + 2, KK = K * K, NT = KK * CORR_TILE_LD, NW = WN * WN, NP = (NW + 63) / 64;
    float *s_tile = s_mem, *s_fx = s_mem + NT + 128, *s_fy = s_fx + 64, *s_brow = s_fy + 64;
    int *s_x0 = reinterpret_cast<int *>(s_mem + NT), *s_y0 = s_x0 + 64;
    const size_t hw = (size_t)D.h * D.w, nq = (size_t)D.B * hw;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long per = (long long)D.B * chunks;
    int l = 0, ebase = 0;
    for (; l < D.num_levels; ++l) {
        if (D.grad_level[l]) {
            const long long cnt = (long long)D.level_n[l] * per;
            if (fb < cnt) break;
            fb -= cnt;
        }
        ebase += D.level_n[l];
    }
    MPC_EXPECT(l < D.num_levels);
    if (l >= D.num_levels) return;
    const int k = (int)(fb / per);
    const int rem = (int)(fb - (long long)k * per), b = rem / chunks, chunk = rem - b * chunks;
    const int t = D.level_target[l][k];
    const int hl = D.level_h[l], wl = D.level_w[l], sl = hl * wl;
    if (!coords) {
        for (int i = threadIdx.x; i < D.d; i += 256) s_brow[MPC_IDX(i, D.d)] = basis[t * D.d + i];
        __syncthreads();
    }
    const size_t pix0 = (size_t)chunk * 64;
    const int nlive = hw - pix0 < 64 ? (int)(hw - pix0) : 64;                         // (pix0 < hw: the first query of a chunk exists)
    if (threadIdx.x < 64) {
        corr_frac f = {0, 0, 0.f, 0.f};
        if (lane < nlive) f = corr_split(corr_centre(D, coords, params, s_brow, t, b, (int)(pix0 + lane), hw), 1.f / (float)(1 << l));
        s_x0[MPC_IDX(lane, 64)] = f.x0; s_y0[MPC_IDX(lane, 64)] = f.y0; s_fx[MPC_IDX(lane, 64)] = f.fx; s_fy[MPC_IDX(lane, 64)] = f.fy;
    }
    // the cotangent tile, coalesced along w; a lane past the grid reads the chunk's first query (never used)
    const float *g = grad_out + ((size_t)b * E + ebase + k) * KK * hw + pix0 + (lane < nlive ? lane : 0);
    for (int c = wv; c < KK; c += 4) s_tile[MPC_IDX(c * CORR_TILE_LD + lane, NT)] = g[(size_t)c * hw];
    __syncthreads();
    // the cell gradients of this wave's 16 queries: lanes over the (K + 1)^2 cells; off < 0: outside the slice or past the grid
    float v[16][NP];
    int off[16][NP];
#pragma unroll
    for (int qi = 0; qi < 16; ++qi) {
        const int ql = wv * 16 + qi;
        const int x0 = s_x0[MPC_IDX(ql, 64)], y0 = s_y0[MPC_IDX(ql, 64)];
        const float fx = s_fx[MPC_IDX(ql, 64)], fy = s_fy[MPC_IDX(ql, 64)];
        const float w00 = (1.f - fx) * (1.f - fy), w01 = fx * (1.f - fy), w10 = (1.f - fx) * fy, w11 = fx * fy;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int c = lane + 64 * p, ci = c / WN, cj = c - ci * WN;
            const int yy = y0 - R + ci, xx = x0 - R + cj;
            const bool ok = ql < nlive && c < NW && yy >= 0 && yy < hl && xx >= 0 && xx < wl;
            // the fill's sum (corr_cell_grad), its cotangents read from the tile: the same terms in the same order
            float a = 0.f;
            if (ok) {
                if (ci < K && cj < K) a = a + s_tile[MPC_IDX((ci * K + cj) * CORR_TILE_LD + ql, NT)] * w00;
                if (ci < K && cj >= 1) a = a + s_tile[MPC_IDX((ci * K + cj - 1) * CORR_TILE_LD + ql, NT)] * w01;
                if (ci >= 1 && cj < K) a = a + s_tile[MPC_IDX(((ci - 1) * K + cj) * CORR_TILE_LD + ql, NT)] * w10;
                if (ci >= 1 && cj >= 1) a = a + s_tile[MPC_IDX(((ci - 1) * K + cj - 1) * CORR_TILE_LD + ql, NT)] * w11;
            }
            v[qi][p] = a;
            off[qi][p] = ok ? ql * sl + yy * wl + xx : -1;
        }
    }
    // read, add once, store: every load first (a cell outside reads the chunk's first element, which exists, and stores nothing)
    float *gs = D.grad_level[l] + ((size_t)k * nq + (size_t)b * hw + pix0) * (size_t)sl;
    float o[16][NP];
#pragma unroll
    for (int qi = 0; qi < 16; ++qi)
#pragma unroll
        for (int p = 0; p < NP; ++p) o[qi][p] = gs[MPC_IDX(off[qi][p] < 0 ? 0 : off[qi][p], (long long)nlive * sl)];
#pragma unroll
    for (int qi = 0; qi < 16; ++qi)
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (off[qi][p] >= 0) gs[MPC_IDX(off[qi][p], (long long)nlive * sl)] = o[qi][p] + v[qi][p];
}

// GC (Bezier mode only): the coordinate gradient of every target, which the centre role forms before it contracts it with the basis
// matrix, is ALSO written to grad_coords [T][B][2][h][w] (what the basis matrix' own gradient is summed from: curve_basis.hip), and
// grad_params may be NULL.  A variant of its own: with GC = 0 the kernel is the code it was.
template <int R, int ACC = 0, int GC = 0>
__global__ __launch_bounds__(256) void k_corr_lookup_bwd(const mpc_corr_desc D, const float *__restrict__ coords,
                                                         const float *__restrict__ params, const float *__restrict__ basis,
                                                         const float *__restrict__ grad_out, float *__restrict__ grad_coords,
                                                         float *__restrict__ grad_params, int chunks, int nA, int E, int groups) {
    extern __shared__ float s_mem[];           // [T][d] basis (Bezier mode) | [E][2][64] per-entry centre gradients | [T][2][64] per-target sums;
                                               // the slice-fill workgroups: [4][(K + 1)^2] window gradients; ACC: corr_bwd_accum's carve-up
    constexpr int K = 2 * R + 1, WN = 2 * R + 2;
    const int T = D.T, d = D.d, nbas = coords ? 0 : T * d;
    float *s_basis = s_mem, *s_ge = s_mem + nbas, *s_gc = s_ge + E * 128;
    const size_t hw = (size_t)D.h * D.w, nq = (size_t)D.B * hw;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if ((int)blockIdx.x < nA) {
        // ---- the centres' gradient: 64 consecutive queries of a sample, the entries dealt to the four waves
        const int b = (int)blockIdx.x / chunks, chunk = (int)blockIdx.x - b * chunks;
        if (!coords) {
            for (int i = threadIdx.x; i < nbas; i += 256) s_basis[MPC_IDX(i, nbas)] = basis[i];
            __syncthreads();
        }
        const size_t pix = (size_t)chunk * 64 + lane;
        const bool live = pix < hw;
        for (int e = wv; e < E; e += 4) {
            int l, k;
            corr_entry(D, e, l, k);
            float gx = 0.f, gy = 0.f;
            if (live) {
                const int t = D.level_target[l][k];
                const float inv = 1.f / (float)(1 << l);
                const corr_frac f = corr_split(corr_centre(D, coords, params, s_basis + t * d, t, b, (int)pix, hw), inv);
                const int hl = D.level_h[l], wl = D.level_w[l];
                const size_t sl = (size_t)hl * wl;
                const float *slice = D.level[l] + ((size_t)k * nq + (size_t)b * hw + pix) * sl;
                const float *g = grad_out + ((size_t)b * E + e) * (K * K) * hw + pix;
                const float ofx = 1.f - f.fx, ofy = 1.f - f.fy;
                float ax = 0.f, ay = 0.f, prev[WN], cur[WN];
#pragma unroll
                for (int j = 0; j < WN; ++j) prev[j] = 0.f;
#pragma unroll 1          // (a rolled row loop: unrolled, the 100 window and 81 cotangent loads are all hoisted and the kernel spills)
                for (int i = 0; i < WN; ++i) {
                    const int yy = f.y0 - R + i;
                    const bool rowin = yy >= 0 && yy < hl;
#pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        const int xx = f.x0 - R + j;
                        cur[j] = (rowin && xx >= 0 && xx < wl) ? slice[MPC_IDX((size_t)yy * wl + xx, sl)] : 0.f;
                    }
                    if (i > 0) {
#pragma unroll
                        for (int j = 0; j < K; ++j) {
                            const float go = g[(size_t)((i - 1) * K + j) * hw];
                            ax = ax + go * ((prev[j + 1] - prev[j]) * ofy + (cur[j + 1] - cur[j]) * f.fy);
                            ay = ay + go * ((cur[j] - prev[j]) * ofx + (cur[j + 1] - prev[j + 1]) * f.fx);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < WN; ++j) prev[j] = cur[j];
                }
                gx = inv * ax;
                gy = inv * ay;
            }
            s_ge[MPC_IDX((e * 2 + 0) * 64 + lane, E * 128)] = gx;
            s_ge[MPC_IDX((e * 2 + 1) * 64 + lane, E * 128)] = gy;
        }
        __syncthreads();
        // per target: the sum over its entries, levels ascending
        for (int t = wv; t < T; t += 4) {
            float gx = 0.f, gy = 0.f;
            int ebase = 0;
            for (int l = 0; l < D.num_levels; ++l) {
                for (int s = 0; s < D.level_n[l]; ++s)
                    if (D.level_target[l][s] == t) {
                        gx = gx + s_ge[MPC_IDX(((ebase + s) * 2 + 0) * 64 + lane, E * 128)];
                        gy = gy + s_ge[MPC_IDX(((ebase + s) * 2 + 1) * 64 + lane, E * 128)];
                    }
                ebase += D.level_n[l];
            }
            if (coords) {
                if (live) {
                    float *gc = grad_coords + ((size_t)t * D.B + b) * 2 * hw + pix;
                    gc[0] = gx; gc[hw] = gy;
                }
            } else {
                s_gc[MPC_IDX((t * 2 + 0) * 64 + lane, T * 128)] = gx;
                s_gc[MPC_IDX((t * 2 + 1) * 64 + lane, T * 128)] = gy;
                if constexpr (GC != 0) {
                    if (live) {
                        float *gc = grad_coords + ((size_t)t * D.B + b) * 2 * hw + pix;
                        gc[0] = gx; gc[hw] = gy;
                    }
                }
            }
        }
        if (coords) return;
        if constexpr (GC != 0) {
            if (!grad_params) return;           // (uniform: params detached, the coordinate gradient alone)
        }
        __syncthreads();
        for (int c = wv; c < 2 * d; c += 4) {
            const int axis = c / d, j = c - axis * d;
            float acc = 0.f;
            for (int t = 0; t < T; ++t) acc = acc + s_basis[MPC_IDX(t * d + j, nbas)] * s_gc[MPC_IDX((t * 2 + axis) * 64 + lane, T * 128)];
            if (live) grad_params[((size_t)b * 2 * d + c) * hw + pix] = acc;
        }
        return;
    }
    if constexpr (ACC != 0) {
        // ---- grad_level, MPC_CORR_F_GRAD_ACCUM: the window cells are added into it, nothing else is touched (groups is unused)
        corr_bwd_accum<R>(D, coords, params, basis, grad_out, s_mem, (long long)blockIdx.x - nA, chunks, E);
        return;
    }
    // ---- grad_level: a wave per (level that wants a gradient, slot, query) writes the whole slice
    long long fb = (long long)blockIdx.x - nA;
    int l = 0, ebase = 0;
    for (; l < D.num_levels; ++l) {
        if (D.grad_level[l]) {
            const long long cnt = (long long)D.level_n[l] * groups;
            if (fb < cnt) break;
            fb -= cnt;
        }
        ebase += D.level_n[l];
    }
    MPC_EXPECT(l < D.num_levels);
    if (l >= D.num_levels) return;
    const int k = (int)(fb / groups);
    const size_t q = (size_t)(fb - (long long)k * groups) * 4 + wv;
    if (q >= nq) return;
    const int b = (int)(q / hw), t = D.level_target[l][k];
    const size_t pix = q - (size_t)b * hw;
    const corr_frac f = corr_split(corr_centre(D, coords, params, coords ? nullptr : basis + t * d, t, b, (int)pix, hw), 1.f / (float)(1 << l));
    const float w00 = (1.f - f.fx) * (1.f - f.fy), w01 = f.fx * (1.f - f.fy), w10 = (1.f - f.fx) * f.fy, w11 = f.fx * f.fy;
    const int hl = D.level_h[l], wl = D.level_w[l], sl = hl * wl;
    const int wy = f.y0 - R, wx = f.x0 - R;                              // the window's first row and column
    const float *g = grad_out + ((size_t)b * E + ebase + k) * (K * K) * hw + pix;
    float *gs = D.grad_level[l] + ((size_t)k * nq + q) * (size_t)sl;
    // the window's (K + 1)^2 cell gradients first, into this wave's LDS window: the streaming loop below then issues no global load,
    // so no store of it ever waits for a load behind the earlier stores (loads and stores share one in-order counter)
    constexpr int NW = WN * WN;
    float *win = s_mem + wv * NW;
#pragma unroll
    for (int p = 0; p < (NW + 63) / 64; ++p) {
        const int c = lane + 64 * p, ci = c / WN, cj = c - ci * WN;
        if (c < NW) win[MPC_IDX(c, NW)] = corr_cell_grad<R>(g, hw, ci, cj, w00, w01, w10, w11);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if ((wl & 3) == 0 && (((uintptr_t)gs) & 15) == 0) {
        // four elements of one row per lane (w_l is a multiple of 4: a group never crosses a row), 16-byte stores
        const int dq = 256 / wl, dr = 256 - dq * wl;
        int yy = (lane * 4) / wl, xx = lane * 4 - yy * wl;
        for (int el = lane * 4; el < sl; el += 256) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            const int ci = yy - wy;
            if (ci >= 0 && ci < WN && xx + 3 >= wx && xx < wx + WN) {                 // (nearly every group lies outside the window)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int cj = xx + u - wx;
                    if (cj >= 0 && cj < WN) v[u] = win[MPC_IDX(ci * WN + cj, NW)];
                }
            }
            MPC_EXPECT(el + 3 < sl);
            const corr_v4f v4 = {v[0], v[1], v[2], v[3]};
            __builtin_nontemporal_store(v4, reinterpret_cast<corr_v4f *>(gs + MPC_IDX(el, sl)));      // written once, read by a later kernel
            yy += dq; xx += dr;
            if (xx >= wl) { xx -= wl; ++yy; }
        }
        return;
    }
    const int dq = 64 / wl, dr = 64 - dq * wl;
    int yy = lane / wl, xx = lane - yy * wl;
    for (int el = lane; el < sl; el += 64) {
        const int ci = yy - wy, cj = xx - wx;
        gs[MPC_IDX(el, sl)] = (ci >= 0 && ci < WN && cj >= 0 && cj < WN) ? win[MPC_IDX(ci * WN + cj, NW)] : 0.f;
        yy += dq; xx += dr;
        if (xx >= wl) { xx -= wl; ++yy; }
    }
}

static int corr_check(const char *who, const mpc_corr_desc *D) {
    if (!D) { mpc_set_error("%s: null descriptor", who); return MPC_E_NULL; }
    if (D->B < 0 || D->h < 1 || D->w < 1 || D->T < 1 || D->d < 0 || D->radius < 1 || D->num_levels < 1) {
        mpc_set_error("%s: bad B / h / w / T / d / radius / num_levels", who); return MPC_E_SHAPE;
    }
    if (D->radius > MPC_CORR_MAX_RADIUS || D->d > 16 || D->T > MPC_CORR_MAX_TARGETS || D->num_levels > MPC_CORR_MAX_LEVELS) {
        mpc_set_error("%s: radius %d > %d, d %d > 16, T %d > %d or %d levels > %d", who, D->radius, MPC_CORR_MAX_RADIUS, D->d, D->T,
                      MPC_CORR_MAX_TARGETS, D->num_levels, MPC_CORR_MAX_LEVELS);
        return MPC_E_UNSUPPORTED;
    }
    long long E = 0;
    for (int l = 0; l < D->num_levels; ++l) {
        const int hl = D->level_h[l], wl = D->level_w[l], n = D->level_n[l];
        if (hl != (D->h >> l) || wl != (D->w >> l)) { mpc_set_error("%s: level %d is %d x %d, expected %d x %d", who, l, hl, wl, D->h >> l, D->w >> l); return MPC_E_SHAPE; }
        if (hl < 2 || wl < 2) { mpc_set_error("%s: level %d is %d x %d: a level below 2 x 2 cannot be sampled (align_corners divides by size - 1)", who, l, hl, wl); return MPC_E_SHAPE; }
        if (n < 1 || n > D->T || (l == 0 && n != D->T)) { mpc_set_error("%s: level %d holds %d targets of %d", who, l, n, D->T); return MPC_E_SHAPE; }
        for (int s = 0; s < n; ++s) {
            const int t = D->level_target[l][s];
            bool ok = t < D->T && (s == 0 || t > D->level_target[l][s - 1]);
            if (ok && l > 0) {
                ok = false;
                for (int u = 0; u < D->level_n[l - 1]; ++u) ok = ok || D->level_target[l - 1][u] == t;
            }
            if (!ok) { mpc_set_error("%s: the targets of level %d are not ascending / not among those of level %d", who, l, l - 1); return MPC_E_SHAPE; }
        }
        E += n;
    }
    const long long hw = (long long)D->h * D->w, K2 = (2 * D->radius + 1) * (2 * D->radius + 1);
    if (hw > (1ll << 24) || (long long)D->B * hw > (1ll << 30) || (long long)D->B * E * K2 * hw > (1ll << 40) ||
        (long long)D->B * hw * D->T * hw > (1ll << 42)) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    return 0;
}

static int corr_entries(const mpc_corr_desc *D) {
    int E = 0;
    for (int l = 0; l < D->num_levels; ++l) E += D->level_n[l];
    return E;
}

static int corr_check_call(const char *who, const mpc_corr_desc *D, const float *coords, const float *params, const float *basis) {
    int rc = corr_check(who, D);
    if (rc) return rc;
    if ((coords != nullptr) == (params != nullptr)) { mpc_set_error("%s: exactly one of coords and params", who); return MPC_E_NULL; }
    if (params && !basis) { mpc_set_error("%s: params without a basis", who); return MPC_E_NULL; }
    if (params && D->d < 1) { mpc_set_error("%s: params with d = 0", who); return MPC_E_SHAPE; }
    if (D->B > 0) for (int l = 0; l < D->num_levels; ++l) if (!D->level[l]) { mpc_set_error("%s: level %d is null", who, l); return MPC_E_NULL; }
    return 0;
}

extern "C" int mpc_corr_lookup_supported(const mpc_corr_desc *desc) { return corr_check(__func__, desc); }

#define CORR_DISPATCH(kern, grid, lds, st, ...)                                                             \
    do {                                                                                                    \
        switch (desc->radius) {                                                                             \
        case 1: MPC_LAUNCH(kern<1>, grid, dim3(256), lds, st, __VA_ARGS__); break;                          \
        case 2: MPC_LAUNCH(kern<2>, grid, dim3(256), lds, st, __VA_ARGS__); break;                          \
        case 3: MPC_LAUNCH(kern<3>, grid, dim3(256), lds, st, __VA_ARGS__); break;                          \
        default: MPC_LAUNCH(kern<4>, grid, dim3(256), lds, st, __VA_ARGS__); break;                         \
        }                                                                                                   \
    } while (0)

extern "C" int mpc_corr_lookup_fwd(const mpc_corr_desc *desc, const float *coords, const float *params, const float *basis, float *out,
                                   void *stream) {
    int rc = corr_check_call(__func__, desc, coords, params, basis);
    if (rc) return rc;
    const long long hw = (long long)desc->h * desc->w;
    if (desc->B == 0) return 0;
    if (!out) { mpc_set_error("%s: null argument", __func__); return MPC_E_NULL; }
    const int E = corr_entries(desc), K = 2 * desc->radius + 1;
    const size_t brow = coords ? 0 : (size_t)desc->d * sizeof(float);
    if (!(desc->flags & MPC_CORR_F_LANE_PER_QUERY)) {
        const int chunks = (int)((hw + 63) / 64);
        const long long nb = (long long)desc->B * E * chunks;
        if (nb > 0x7fffffffll) { mpc_set_error("%s: grid too large", __func__); return MPC_E_UNSUPPORTED; }
        const size_t lds = ((size_t)K * K * CORR_TILE_LD + 4 * (K + 1) * (K + 1) + 256) * sizeof(float) + brow;
        const dim3 grid((unsigned)nb);
        CORR_DISPATCH(k_corr_lookup_fwd, grid, lds, (hipStream_t)stream, *desc, coords, params, basis, out, chunks, E);
    } else {
        const int chunks = (int)((hw + 255) / 256);
        const long long nb = (long long)desc->B * E * chunks;
        if (nb > 0x7fffffffll) { mpc_set_error("%s: grid too large", __func__); return MPC_E_UNSUPPORTED; }
        const dim3 grid((unsigned)nb);
        CORR_DISPATCH(k_corr_lookup_fwd_lane, grid, brow, (hipStream_t)stream, *desc, coords, params, basis, out, chunks, E);
    }
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_corr_lookup_bwd(const mpc_corr_desc *desc, const float *coords, const float *params, const float *basis,
                                   const float *grad_out, float *grad_coords, float *grad_params, void *stream) {
    int rc = corr_check_call(__func__, desc, coords, params, basis);
    if (rc) return rc;
    if (desc->B == 0) return 0;
    if (!grad_out) { mpc_set_error("%s: null argument", __func__); return MPC_E_NULL; }
    // (grad_coords in the Bezier mode: the targets' coordinate gradient beside grad_params, or alone -- the GC variant of the kernel)
    if (grad_params && !params) { mpc_set_error("%s: a gradient for an input that was not given", __func__); return MPC_E_NULL; }
    const bool gc = params && grad_coords;
    const long long hw = (long long)desc->h * desc->w, nq = (long long)desc->B * hw;
    const int E = corr_entries(desc);
    const int chunks = (int)((hw + 63) / 64), groups = (int)((nq + 3) / 4);
    const long long nA = (grad_coords || grad_params) ? (long long)desc->B * chunks : 0;
    const bool accum = (desc->flags & MPC_CORR_F_GRAD_ACCUM) != 0;        // (with every grad_level NULL the flag changes nothing)
    long long nfill = 0;
    for (int l = 0; l < desc->num_levels; ++l)
        if (desc->grad_level[l]) nfill += (long long)desc->level_n[l] * (accum ? (long long)desc->B * chunks : (long long)groups);
    if (nA + nfill == 0) return 0;
    if (nA + nfill > 0x7fffffffll) { mpc_set_error("%s: grid too large", __func__); return MPC_E_UNSUPPORTED; }
    const size_t WN = 2 * (size_t)desc->radius + 2;
    const size_t lds = std::max(((coords ? 0 : (size_t)desc->T * desc->d) + ((size_t)E + desc->T) * 128) * sizeof(float),
                                4 * WN * WN * sizeof(float));                       // (the slice-fill workgroups' window gradients)
    const dim3 grid((unsigned)(nA + nfill));
#define CORR_BWD_VARIANT(RR, AA, GG, bytes)                                                                                   \
    MPC_LAUNCH((k_corr_lookup_bwd<RR, AA, GG>), grid, dim3(256), bytes, (hipStream_t)stream, *desc, coords, params, basis, grad_out, \
               grad_coords, grad_params, chunks, (int)nA, E, groups)
    if (gc) {                                   // every other call takes the launches below, as it did
        const size_t K = 2 * (size_t)desc->radius + 1;
        const bool acc = accum && nfill > 0;
        const size_t bytes = acc ? std::max(lds, (K * K * CORR_TILE_LD + 256 + (size_t)desc->d) * sizeof(float)) : lds;
        switch (desc->radius) {
        case 1: if (acc) CORR_BWD_VARIANT(1, 1, 1, bytes); else CORR_BWD_VARIANT(1, 0, 1, bytes); break;
        case 2: if (acc) CORR_BWD_VARIANT(2, 1, 1, bytes); else CORR_BWD_VARIANT(2, 0, 1, bytes); break;
        case 3: if (acc) CORR_BWD_VARIANT(3, 1, 1, bytes); else CORR_BWD_VARIANT(3, 0, 1, bytes); break;
        default: if (acc) CORR_BWD_VARIANT(4, 1, 1, bytes); else CORR_BWD_VARIANT(4, 0, 1, bytes); break;
        }
        MPC_CHECK_LAUNCH();
        return 0;
    }
#undef CORR_BWD_VARIANT
    if (accum && nfill > 0) {
        const size_t K = 2 * (size_t)desc->radius + 1;
        const size_t lds_acc = std::max(lds, (K * K * CORR_TILE_LD + 256 + (coords ? 0 : (size_t)desc->d)) * sizeof(float));
        switch (desc->radius) {
        case 1: MPC_LAUNCH((k_corr_lookup_bwd<1, 1>), grid, dim3(256), lds_acc, (hipStream_t)stream, *desc, coords, params, basis, grad_out, grad_coords, grad_params, chunks, (int)nA, E, groups); break;
        case 2: MPC_LAUNCH((k_corr_lookup_bwd<2, 1>), grid, dim3(256), lds_acc, (hipStream_t)stream, *desc, coords, params, basis, grad_out, grad_coords, grad_params, chunks, (int)nA, E, groups); break;
        case 3: MPC_LAUNCH((k_corr_lookup_bwd<3, 1>), grid, dim3(256), lds_acc, (hipStream_t)stream, *desc, coords, params, basis, grad_out, grad_coords, grad_params, chunks, (int)nA, E, groups); break;
        default: MPC_LAUNCH((k_corr_lookup_bwd<4, 1>), grid, dim3(256), lds_acc, (hipStream_t)stream, *desc, coords, params, basis, grad_out, grad_coords, grad_params, chunks, (int)nA, E, groups); break;
        }
        MPC_CHECK_LAUNCH();
        return 0;
    }
    CORR_DISPATCH(k_corr_lookup_bwd, grid, lds, (hipStream_t)stream, *desc, coords, params, basis, grad_out, grad_coords, grad_params,
                  chunks, (int)nA, E, groups);
    MPC_CHECK_LAUNCH();
    return 0;
}

MPC_BOUNDS_UNIT("corr_lookup.hip")
