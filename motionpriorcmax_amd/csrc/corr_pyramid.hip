// RAFT-spline correlation pyramid: the all-pairs volume of the reference frame against every target, and its average-pooled levels.
//   reference: src/models/raft_spline/corr.py:235-270 (CorrComputation._corr_dot_prod_1_to_N, get_correlation_volume: the batched
//   matmul and the division by sqrt(D)), corr.py:106-123 (CorrData.get_downsampled: avg_pool2d 2 x 2, stride 2, per level),
//   corr.py:296-302 (which targets a level holds), raft.py:126 (fp32).
// Pooling is linear, so level l of target t is a GEMM of its own against the l-times pooled feature map P_l of that target:
//   level_l[slot][b * hw + i][j] = (sum_c fmap1[b][c][i] * P_l(fmap2[t][b])[c][j]) / sqrt(D)
// -- every level is written once, level 0 is never read back (plain torch writes it, rewrites it for the division and reads it
// again to pool), and the backward needs no volume-sized temporary:
//   grad_fmap1[b][c][i] = (sum over (level, slot, j) of G_l[slot][b * hw + i][j] * P_l[t][b][c][j]) / sqrt(D)
//   gP_l[slot][b][c][j] = (sum_i fmap1[b][c][i] * G_l[slot][b * hw + i][j]) / sqrt(D)
//   grad_fmap2[t][b][c][y][x] = sum_l 4^-l gP_l[slot_l(t)][b][c][y >> l][x >> l]   (levels ascending; only (y >> l) < h_l, (x >> l) < w_l)
//   k_corr_pyr_pool     P_l from P_(l-1) (P_0 = fmap2), one launch per level >= 1, into the workspace: rows [c] of pitch
//                       round_up(h_l * w_l, 4), the pad written 0.  ((a00 + a01) + a10) + a11, then * 0.25.
//   k_corr_pyr_gemm<M>  the one GEMM core: 128 x 128 x 32 workgroup tile, four waves of 2 x 2 tiles of 32 x 32 on
//                       v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fma chain per element), operands through LDS, the next k
//                       block's global loads in flight during the MFMAs; ragged edges in m, n and k by predication.
//                       M = 0 forward: one launch over every (level, slot, sample, tile).
//                       M = 1 gP: one launch over every (split, level with a cotangent, slot, sample, tile); k = i.
//                       M = 2 grad_fmap1: k = the concatenation over (level, slot, j).
//                       Both backward products have few tiles at batch 1 (244 and 48 at the shipped shape): k is split into S1 / S
//                       contiguous ranges of k blocks (from the sizes alone); the ranges write partials.
//   k_corr_pyr_reduce   grad_fmap1 = (partial_0 + partial_1 + ... in index order) / sqrt(D)   (S > 1 only)
//   k_corr_pyr_gather   grad_fmap2 from the gP_l (their partials in index order, levels ascending); writes every element (0 where
//                       no level reaches); four x per thread and 16-byte accesses where w % 4 == 0.
// No atomics, every sum in one fixed order: bitwise reproducible.  Volume offsets are 64-bit.
// Element types (the `_dt` entry points; dt_device.h): every kernel and cp_ref / cp_operand / cp_load are templates over the type T of
// the feature maps and their gradients -- float, mpc_f16 or mpc_bf16; levels, cotangents, P_l (l >= 1), gP_l and the split-k partials
// are fp32 whatever T is.  The float instantiations are the kernels as they were before (same device code).  With a 16-bit T:
//   k_corr_pyr_gemm16   level 0 of the forward -- both operands feature maps as they lie -- on v_mfma_f32_32x32x16_f16 / _bf16: the
//                       products are exact in fp32 and the accumulation is fp32, so the element is the sum of the fp32 kernel on the
//                       upcast maps in another order (equal bits where every partial sum is exact; else bounded by gamma(D) with
//                       u = 2^-23: the rounding of the instruction's adder is not specified).  fp16 subnormal inputs are multiplied as
//                       the values they are (measured: the instruction does not flush them).  A launch of its own before gemm<0>,
//                       which then serves the levels >= 1 alone.
//   everything else     the fp32 kernels with the 16-bit element converted at the load (cp_ldv / mpc_ld: exact; one 8-byte load of 4
//                       elements where the fp32 kernel loads 16 bytes): the pool at l = 1, fmap1 in gemm<0> / gemm<1>, P_0 = fmap2 in
//                       gemm<2> -- the fp32 kernels' arithmetic on the upcast maps bit for bit, same tiling, splits and order.
//   gradients           rounded once to T (mpc_st / mpc_store_vec): cp_write where S == 1, k_corr_pyr_reduce, k_corr_pyr_gather (8 x
//                       per thread and one 16-byte store where w % 8 == 0 and the tensors are 16-byte aligned, else per element).
// Several references (corr.py:221-225, 246-260: CorrComputation.__add__ / _corr_dot_prod_M_to_N, events then frames): the flat target
// list is the concatenation of the references' targets, the problem is block-diagonal, and the same launches serve it -- a slot
// reads the fmap1 / fmap2 of its target's reference where they lie and writes its gradient into that reference's tensors.  Every
// reference keeps the split (S1, S, kblocks) of the single-reference problem of that reference alone and gemm<2> runs over (reference,
// split, sample, tile) with k = that reference's (level, slot, j): the call equals the single-reference calls bit for bit.  The
// single-reference entry points are the same code with one reference.
#include <algorithm>
#include <math.h>
#include "common.h"
#include "bounds.h"
#include "dt_device.h"
#include <type_traits>

#define CP_MAX_D 512
#define CP_BM 128
#define CP_BK 32
#define CP_LDK 33                          // row pitch of a k-contiguous operand tile [128][32] in LDS: (x + k) % 32 banks, conflict free
#define CP_TILE (CP_BM * CP_LDK)           // floats of LDS per operand ([32][128] for an operand that is contiguous along m / n)
#define CP_MAX_SPLIT 16

typedef float cp_f32x16 __attribute__((ext_vector_type(16)));

// sub-buffers of the workspace, in floats: P_l (l >= 1) of all slots, then per reference gP_l (backward) and its split-k partials
struct cp_plan {
    long long p_off[MPC_CORR_MAX_LEVELS], total;
    int pitch[MPC_CORR_MAX_LEVELS];
    int D;
    float sq;                              // sqrt(D) in fp32, as torch.sqrt(torch.tensor(D).float()) gives it
};

// one reference: its tensors, its flat targets [t0, t0 + level_n[0]), its slots [slot0[l], slot0[l] + level_n[l]) of level l
// (contiguous: the targets of a level ascend), and the split of its two backward products
template <typename T>
struct cp_ref {
    const T *fmap1, *fmap2;
    T *grad_fmap1, *grad_fmap2;
    long long gp_off[MPC_CORR_MAX_LEVELS], part_off;
    int t0, num_levels;
    int slot0[MPC_CORR_MAX_LEVELS], level_n[MPC_CORR_MAX_LEVELS];
    int S, kblocks;                        // grad_fmap1: S ranges of the kblocks k blocks of the concatenation
    int S1;                                // gP: S1 ranges of the k blocks of i; gP_l is [S1][level_n[l]][B][D][pitch_l]
};

template <typename T>
struct cp_refs {
    int R;
    unsigned char ref_of[MPC_CORR_MAX_TARGETS];        // flat target -> reference
    cp_ref<T> r[MPC_CORR_MAX_REFS];
};

// an operand of element type T (float: the workspace, a cotangent, an fp32 feature map; mpc_f16 / mpc_bf16: a feature map as it lies)
template <typename T>
struct cp_operand {
    const T *p;                            // at the tile's origin in m / n and the range's origin in k
    long long ld;
    int rem;                               // valid m / n from the origin
    bool vec;                              // loads of 4 elements allowed (pointer and pitch are multiples of 4 elements: 16 bytes of
                                           // fp32, 8 bytes of a 16-bit type)
};

// 4 consecutive elements as fp32 (mpc_ld: exact), one load
__device__ __forceinline__ float4 cp_ldv(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 cp_ldv(const mpc_f16 *p) {
    const uint2 q = *reinterpret_cast<const uint2 *>(p);
    return make_float4((float)__builtin_bit_cast(_Float16, (uint16_t)q.x), (float)__builtin_bit_cast(_Float16, (uint16_t)(q.x >> 16)),
                       (float)__builtin_bit_cast(_Float16, (uint16_t)q.y), (float)__builtin_bit_cast(_Float16, (uint16_t)(q.y >> 16)));
}
__device__ __forceinline__ float4 cp_ldv(const mpc_bf16 *p) {
    const uint2 q = *reinterpret_cast<const uint2 *>(p);
    return make_float4(__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u), __uint_as_float(q.y << 16),
                       __uint_as_float(q.y & 0xffff0000u));
}

template <typename T>
__device__ __forceinline__ float4 cp_ld4(const T *p, int n, bool vec) {
    if (vec && n >= 4) return cp_ldv(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0) v.x = mpc_ld(p);
    if (n > 1) v.y = mpc_ld(p + 1);
    if (n > 2) v.z = mpc_ld(p + 2);
    if (n > 3) v.w = mpc_ld(p + 3);
    return v;
}

// KC = false: element (k, x) at p[k * ld + x] (contiguous along m / n); KC = true: at p[x * ld + k] (contiguous along k)
template <bool KC, typename T>
__device__ __forceinline__ void cp_load(float4 (&r)[4], const cp_operand<T> &o, int kb, int k1) {
    const int t = threadIdx.x;
    if (o.vec && o.rem >= CP_BM && kb + CP_BK <= k1) {
        // an interior tile (uniform branch): four 16-byte loads back to back, no predicate between them
        const T *p = KC ? o.p + (long long)(t >> 3) * o.ld + kb + (t & 7) * 4 : o.p + (long long)(kb + (t >> 5)) * o.ld + (t & 31) * 4;
        const long long step = (KC ? 32 : 8) * o.ld;
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = cp_ldv(p + q * step);
        return;
    }
    if (!KC) {
        const int x4 = (t & 31) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = kb + (t >> 5) + 8 * q;
            r[q] = k < k1 ? cp_ld4(o.p + (long long)k * o.ld + x4, o.rem - x4, o.vec) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        const int k4 = kb + (t & 7) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x = (t >> 3) + 32 * q;
            r[q] = x < o.rem ? cp_ld4(o.p + (long long)x * o.ld + k4, k1 - k4, o.vec) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

template <bool KC>
__device__ __forceinline__ void cp_store(float *s, const float4 (&r)[4]) {
    const int t = threadIdx.x;
    if (!KC) {
        const int x4 = (t & 31) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = (t >> 5) + 8 * q;
            *reinterpret_cast<float4 *>(s + MPC_IDX(k * CP_BM + x4, CP_TILE - 3)) = r[q];
        }
    } else {
        const int k4 = (t & 7) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float *d = s + MPC_IDX(((t >> 3) + 32 * q) * CP_LDK + k4, CP_TILE - 3);
            d[0] = r[q].x; d[1] = r[q].y; d[2] = r[q].z; d[3] = r[q].w;
        }
    }
}

template <bool KC>
__device__ __forceinline__ float cp_frag(const float *s, int x, int k) {
    return KC ? s[MPC_IDX(x * CP_LDK + k, CP_TILE)] : s[MPC_IDX(k * CP_BM + x, CP_TILE)];
}

// acc += A^T B over k in [k0, k1) of the operands' own k axis (k0 a multiple of 4 where the operand is vectorised along k)
template <bool AK, bool BK, typename TA, typename TB>
__device__ __forceinline__ void cp_gemm_range(cp_f32x16 (&acc)[2][2], const cp_operand<TA> &A, const cp_operand<TB> &B, int k0, int k1,
                                              float *sA, float *sB) {
    if (k0 >= k1) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int xa = (wv >> 1) * 64 + (lane & 31), xb = (wv & 1) * 64 + (lane & 31), kh = lane >> 5;
    float4 ra[4], rb[4];
    cp_load<AK>(ra, A, k0, k1);
    cp_load<BK>(rb, B, k0, k1);
    for (int kb = k0; kb < k1; kb += CP_BK) {
        __syncthreads();                                   // the previous block's fragments are read
        cp_store<AK>(sA, ra);
        cp_store<BK>(sB, rb);
        __syncthreads();
        if (kb + CP_BK < k1) {
            cp_load<AK>(ra, A, kb + CP_BK, k1);
            cp_load<BK>(rb, B, kb + CP_BK, k1);
        }
#pragma unroll 4
        for (int kk = 0; kk < CP_BK; kk += 2) {
            const float a0 = cp_frag<AK>(sA, xa, kk + kh), a1 = cp_frag<AK>(sA, xa + 32, kk + kh);
            const float b0 = cp_frag<BK>(sB, xb, kk + kh), b1 = cp_frag<BK>(sB, xb + 32, kk + kh);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}

// C[m][n] = acc (/ sq) for the tile's valid part, rounded once to C's type; `ext`: elements of C's buffer from c on (bounds build)
template <typename TC>
__device__ __forceinline__ void cp_write(const cp_f32x16 (&acc)[2][2], TC *c, long long ldc, int mrem, int nrem, bool div, float sq,
                                         long long ext) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // v / sq as the division gives it, without the division sequence, where sq is a power of two (D = 4, 16, 64, 256: the
    // reciprocal is exact and the product is the same scaling of the exponent); uniform branch
    const bool pow2 = (__float_as_uint(sq) & 0x007fffffu) == 0;
    const float inv = 1.f / sq;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int col = (wv & 1) * 64 + b * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (wv >> 1) * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < mrem && col < nrem) {
                    const float v = acc[a][b][r];
                    const float o = !div ? v : pow2 ? v * inv : v / sq;
                    mpc_st(&c[MPC_IDX((long long)row * ldc + col, ext)], o);
                }
            }
        }
}

__device__ __forceinline__ bool cp_al16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
// aligned for cp_ldv
template <typename T> __device__ __forceinline__ bool cp_alv(const T *p) { return (((uintptr_t)p) & (4 * sizeof(T) - 1)) == 0; }

// the operand P_0 of (slot k, sample b): the fmap2 of the slot's reference itself, pitch h * w
template <typename T>
__device__ __forceinline__ const T *cp_level0(const mpc_corr_desc &D, const cp_plan &P, const cp_refs<T> &M, int k, int b) {
    const int t = D.level_target[0][k];
    const cp_ref<T> &R = M.r[MPC_IDX(M.ref_of[MPC_IDX(t, D.T)], M.R)];
    return R.fmap2 + ((long long)MPC_IDX(t - R.t0, R.level_n[0]) * D.B + b) * P.D * ((long long)D.h * D.w);
}

// the fp32 operand P_l of (level l, slot k, sample b): the workspace above level 0; at level 0 the fp32 fmap2 (T = float only)
template <typename T>
__device__ __forceinline__ const float *cp_pooled(const mpc_corr_desc &D, const cp_plan &P, const cp_refs<T> &M, const float *ws, int l,
                                                  int k, int b, long long &ld) {
    const long long hw = (long long)D.h * D.w;
    if (std::is_same<T, float>::value && l == 0) {
        const int t = D.level_target[0][k];
        const cp_ref<T> &R = M.r[MPC_IDX(M.ref_of[MPC_IDX(t, D.T)], M.R)];
        ld = hw;
        return reinterpret_cast<const float *>(R.fmap2) + ((long long)MPC_IDX(t - R.t0, R.level_n[0]) * D.B + b) * P.D * hw;
    }
    ld = P.pitch[l];
    return ws + P.p_off[l] + ((long long)k * D.B + b) * P.D * ld;
}

// T: the element type of the feature maps and their gradients.  T = float: every product on the fp32 MFMA, as before the 16-bit types
// existed.  A 16-bit T: the same kernel with the feature maps converted at the load (cp_ldv / mpc_ld: exact), so every sum is the fp32
// kernel's on the upcast tensor; MODE 0 then serves the levels >= 1 only (level 0: k_corr_pyr_gemm16 below).
template <int MODE, typename T>
__global__ __launch_bounds__(256) void k_corr_pyr_gemm(const mpc_corr_desc D, const cp_plan P, const cp_refs<T> M, float *__restrict__ ws) {
    constexpr bool F32 = std::is_same<T, float>::value;
    extern __shared__ __attribute__((aligned(16))) float s_cp[];          // [CP_TILE] A | [CP_TILE] B
    float *sA = s_cp, *sB = s_cp + CP_TILE;
    const long long hw = (long long)D.h * D.w;
    const int Dm = P.D;
    cp_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    long long bid = blockIdx.x;
    if (MODE == 0) {
        // (level, slot, sample, tile m, tile n), n fastest: m = i, n = j, k = c
        const int tm = (int)((hw + CP_BM - 1) / CP_BM);
        int l = F32 ? 0 : 1, tn = 1;
        for (; l < D.num_levels; ++l) {
            tn = (D.level_h[l] * D.level_w[l] + CP_BM - 1) / CP_BM;
            const long long cnt = (long long)D.level_n[l] * D.B * tm * tn;
            if (bid < cnt) break;
            bid -= cnt;
        }
        MPC_EXPECT(l < D.num_levels);
        if (l >= D.num_levels) return;
        const int in = (int)(bid % tn); bid /= tn;
        const int im = (int)(bid % tm); bid /= tm;
        const int b = (int)(bid % D.B), k = (int)(bid / D.B);
        const int N = D.level_h[l] * D.level_w[l], m0 = im * CP_BM, n0 = in * CP_BM;
        const T *fmap1 = M.r[MPC_IDX(M.ref_of[MPC_IDX(D.level_target[l][MPC_IDX(k, D.level_n[l])], D.T)], M.R)].fmap1;
        long long ldb;
        const float *pb = cp_pooled(D, P, M, ws, l, k, b, ldb);
        const cp_operand<T> A = {fmap1 + (long long)b * Dm * hw + m0, hw, (int)(hw - m0), (hw & 3) == 0 && cp_alv(fmap1)};
        const cp_operand<float> B = {pb + n0, ldb, N - n0, (ldb & 3) == 0 && cp_al16(pb)};
        cp_gemm_range<false, false>(acc, A, B, 0, Dm, sA, sB);
        const long long row0 = (long long)k * D.B * hw + (long long)b * hw + m0;
        const long long ext = ((long long)D.level_n[l] * D.B * hw - row0) * N - n0;
        cp_write(acc, const_cast<float *>(D.level[l]) + row0 * N + n0, N, (int)(hw - m0), N - n0, true, P.sq, ext);
    } else if (MODE == 1) {
        // (level with a cotangent, reference that wants grad_fmap2, split, slot of the reference, sample, tile m, tile n), n fastest:
        // m = c, n = j, k = i in the reference's own S1 ranges
        const int tm = (Dm + CP_BM - 1) / CP_BM;
        int l = 0, tn = 1, s = 0, ri = 0;
        bool found = false;
        for (; l < D.num_levels; ++l) {
            if (!D.grad_level[l]) continue;
            tn = (D.level_h[l] * D.level_w[l] + CP_BM - 1) / CP_BM;
            for (ri = 0; ri < M.R; ++ri) {
                if (!M.r[ri].grad_fmap2 || l >= M.r[ri].num_levels) continue;
                const long long per = (long long)M.r[ri].level_n[l] * D.B * tm * tn, cnt = per * M.r[ri].S1;
                if (bid < cnt) { s = (int)(bid / per); bid -= s * per; found = true; break; }
                bid -= cnt;
            }
            if (found) break;
        }
        MPC_EXPECT(found);
        if (!found) return;
        const cp_ref<T> &R = M.r[MPC_IDX(ri, M.R)];
        const int in = (int)(bid % tn); bid /= tn;
        const int im = (int)(bid % tm); bid /= tm;
        const int b = (int)(bid % D.B), kr = (int)(bid / D.B), k = R.slot0[l] + MPC_IDX(kr, R.level_n[l]);
        const int N = D.level_h[l] * D.level_w[l], m0 = im * CP_BM, n0 = in * CP_BM;
        const float *g = D.grad_level[l] + ((long long)MPC_IDX(k, D.level_n[l]) * D.B + b) * hw * N;
        const cp_operand<T> A = {R.fmap1 + ((long long)b * Dm + m0) * hw, hw, Dm - m0, (hw & 3) == 0 && cp_alv(R.fmap1)};
        const cp_operand<float> B = {g + n0, N, N - n0, (N & 3) == 0 && cp_al16(g)};
        const int nkb = (int)((hw + CP_BK - 1) / CP_BK);
        const int kb0 = (int)((long long)s * nkb / R.S1), kb1 = (int)((long long)(s + 1) * nkb / R.S1);
        cp_gemm_range<true, false>(acc, A, B, kb0 * CP_BK, min((long long)kb1 * CP_BK, hw), sA, sB);
        const long long ld = P.pitch[l], row0 = (((long long)s * R.level_n[l] + kr) * D.B + b) * Dm + m0;
        const long long ext = ((long long)R.S1 * R.level_n[l] * D.B * Dm - row0) * ld - n0;
        cp_write(acc, ws + R.gp_off[l] + row0 * ld + n0, ld, Dm - m0, N - n0, true, P.sq, ext);
    } else {
        // (reference that wants grad_fmap1, split, sample, tile m, tile n), n fastest: m = c, n = i, k = (level, slot of the reference, j)
        // in k blocks [kb0, kb1) of the reference's concatenation
        const int tm = (Dm + CP_BM - 1) / CP_BM, tn = (int)((hw + CP_BM - 1) / CP_BM);
        int ri = 0;
        for (; ri < M.R; ++ri) {
            if (!M.r[ri].grad_fmap1) continue;
            const long long cnt = (long long)M.r[ri].S * D.B * tm * tn;
            if (bid < cnt) break;
            bid -= cnt;
        }
        MPC_EXPECT(ri < M.R);
        if (ri >= M.R) return;
        const cp_ref<T> &R = M.r[ri];
        const int in = (int)(bid % tn); bid /= tn;
        const int im = (int)(bid % tm); bid /= tm;
        const int b = (int)(bid % D.B), s = (int)(bid / D.B);
        const int m0 = im * CP_BM, n0 = in * CP_BM;
        const int kb0 = (int)((long long)s * R.kblocks / R.S), kb1 = (int)((long long)(s + 1) * R.kblocks / R.S);
        int first = 0;
        for (int l = 0; l < R.num_levels; ++l) {
            if (!D.grad_level[l]) continue;
            const int N = D.level_h[l] * D.level_w[l], nkb = (N + CP_BK - 1) / CP_BK;
            for (int kr = 0; kr < R.level_n[l]; ++kr, first += nkb) {
                const int lo = max(kb0, first) - first, hi = min(kb1, first + nkb) - first;
                if (lo >= hi) continue;
                const int k = R.slot0[l] + kr;
                if constexpr (!F32) if (l == 0) {
                    // P_0 is the 16-bit fmap2 as it lies
                    const T *pa = cp_level0(D, P, M, k, b);
                    const float *g = D.grad_level[l] + (((long long)MPC_IDX(k, D.level_n[l]) * D.B + b) * hw + n0) * N;
                    const cp_operand<T> A = {pa + (long long)m0 * hw, hw, Dm - m0, (hw & 3) == 0 && cp_alv(pa)};
                    const cp_operand<float> B = {g, N, (int)(hw - n0), (N & 3) == 0 && cp_al16(D.grad_level[l])};
                    cp_gemm_range<true, true>(acc, A, B, lo * CP_BK, min(hi * CP_BK, N), sA, sB);
                    continue;
                }
                long long lda;
                const float *pa = cp_pooled(D, P, M, ws, l, k, b, lda);
                const float *g = D.grad_level[l] + (((long long)MPC_IDX(k, D.level_n[l]) * D.B + b) * hw + n0) * N;
                const cp_operand<float> A = {pa + (long long)m0 * lda, lda, Dm - m0, (lda & 3) == 0 && cp_al16(pa)};
                const cp_operand<float> B = {g, N, (int)(hw - n0), (N & 3) == 0 && cp_al16(D.grad_level[l])};
                cp_gemm_range<true, true>(acc, A, B, lo * CP_BK, min(hi * CP_BK, N), sA, sB);
            }
        }
        const long long row0 = (long long)b * Dm + m0;
        if (R.S == 1) {
            cp_write(acc, R.grad_fmap1 + row0 * hw + n0, hw, Dm - m0, (int)(hw - n0), true, P.sq, ((long long)D.B * Dm - row0) * hw - n0);
        } else {
            const long long prow0 = (long long)s * D.B * Dm + row0;
            cp_write(acc, ws + R.part_off + prow0 * hw + n0, hw, Dm - m0, (int)(hw - n0), false, 1.f,
                     ((long long)R.S * D.B * Dm - prow0) * hw - n0);
        }
    }
}

// ---- level 0 of the forward from 16-bit feature maps, on the 16-bit matrix cores
// Both operands are feature maps as they lie, [c][i] and [c][j]: a product of two fp16 (two bf16) values is exact in fp32 and
// v_mfma_f32_32x32x16_f16 / _bf16 accumulates in fp32, so the element is the sum the fp32 kernel forms on the upcast tensors, in
// another order (16 channels per instruction).  Same 128 x 128 workgroup tile of 2 x 2 wave tiles of 32 x 32 and the same cp_write;
// a k block is CP_HK = 32 channels = two MFMA steps per wave tile.  The instruction wants 8 consecutive k per lane (lane l: row /
// column l & 31, k = 8 (l >> 5) + j), the maps are contiguous along m / n: the tile is transposed on its way into LDS.  Threads
// 0-127 stage A, 128-255 stage B: a thread loads rows kb + 4q .. 4q + 3 (q = t & 7) of 8 consecutive m / n (x8 = 8 (t >> 3)), packs
// the four k of each m / n into 8 bytes and stores them at [x][4q] of the k-contiguous image [128][CP_HLD].  Row pitch 80 bytes:
// the 16-byte fragment reads of a 16-lane group fall on 16 different bank quads; the 8-byte stores of a 16-lane group are 2-way.
// Loader branches (a tile's, uniform per wave): `interior` -- 16-byte loads allowed (base 16-byte aligned, h * w a multiple of 8),
// 128 valid m / n, 32 valid k: four loads back to back; else per row: k beyond D -> zeros (`k remainder`), a chunk of 8 inside the
// valid m / n with 16-byte loads allowed -> one load, a chunk past the valid m / n -> zeros (`ragged m` / `ragged n`), and where
// 16-byte loads are not allowed -> 8 predicated element loads (`narrow`: odd h * w, a view 1, 2 or 4 elements into its storage).
#define CP_HK 32
#define CP_HLD 40                          // row pitch of the k-contiguous 16-bit tile [128][32], in elements
#define CP_HTILE (CP_BM * CP_HLD)

typedef __bf16 cp_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 cp_f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ cp_f32x16 cp_mfma16(const mpc_bf16 *, uint4 a, uint4 b, cp_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cp_bf16x8, a), __builtin_bit_cast(cp_bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ cp_f32x16 cp_mfma16(const mpc_f16 *, uint4 a, uint4 b, cp_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cp_f16x8, a), __builtin_bit_cast(cp_f16x8, b), c, 0, 0, 0);
}

// r[i]: the 8 elements x8 .. x8 + 7 of row kb + 4q + i, zeros beyond k1 and beyond o.rem; o.vec: 16-byte loads allowed
template <typename T>
__device__ __forceinline__ void cp_h_load(uint4 (&r)[4], const cp_operand<T> &o, int kb, int k1) {
    const int tl = threadIdx.x & 127, q = tl & 7, x8 = (tl >> 3) * 8;
    const uint16_t *p = reinterpret_cast<const uint16_t *>(o.p) + (long long)(kb + 4 * q) * o.ld + x8;
    if (o.vec && o.rem >= CP_BM && kb + CP_HK <= k1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = *reinterpret_cast<const uint4 *>(p + i * o.ld);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[i] = make_uint4(0u, 0u, 0u, 0u);
        if (kb + 4 * q + i >= k1 || x8 >= o.rem) continue;
        const uint16_t *e = p + i * o.ld;
        if (o.vec && x8 + 8 <= o.rem) { r[i] = *reinterpret_cast<const uint4 *>(e); continue; }
        const int n = o.rem - x8;
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = j < n ? (uint32_t)e[j] : 0u;
        r[i] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
    }
}

// the thread's 4 k x 8 m / n block into the image s [128][CP_HLD]: 8 bytes (k = 4q .. 4q + 3) per m / n
__device__ __forceinline__ void cp_h_store(uint16_t *s, const uint4 (&r)[4]) {
    const int tl = threadIdx.x & 127, q = tl & 7, x8 = (tl >> 3) * 8;
    const uint32_t w[4][4] = {{r[0].x, r[0].y, r[0].z, r[0].w}, {r[1].x, r[1].y, r[1].z, r[1].w}, {r[2].x, r[2].y, r[2].z, r[2].w},
                              {r[3].x, r[3].y, r[3].z, r[3].w}};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int d = j >> 1;
        const uint32_t lo = (j & 1) ? (w[0][d] >> 16) | (w[1][d] & 0xffff0000u) : (w[0][d] & 0xffffu) | (w[1][d] << 16);
        const uint32_t hi = (j & 1) ? (w[2][d] >> 16) | (w[3][d] & 0xffff0000u) : (w[2][d] & 0xffffu) | (w[3][d] << 16);
        *reinterpret_cast<uint2 *>(s + MPC_IDX((x8 + j) * CP_HLD + 4 * q, CP_HTILE - 3)) = make_uint2(lo, hi);
    }
}

// (slot, sample, tile m, tile n) of level 0, n fastest: m = i, n = j, k = c
template <typename T>
__global__ __launch_bounds__(256) void k_corr_pyr_gemm16(const mpc_corr_desc D, const cp_plan P, const cp_refs<T> M) {
    __shared__ __attribute__((aligned(16))) uint16_t s_h[2 * CP_HTILE];          // A | B
    const long long hw = (long long)D.h * D.w;
    const int Dm = P.D;
    cp_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    long long bid = blockIdx.x;
    const int tm = (int)((hw + CP_BM - 1) / CP_BM);
    const int in = (int)(bid % tm); bid /= tm;
    const int im = (int)(bid % tm); bid /= tm;
    const int b = (int)(bid % D.B), k = (int)(bid / D.B);
    MPC_EXPECT(k < D.level_n[0]);
    if (k >= D.level_n[0]) return;
    const int m0 = im * CP_BM, n0 = in * CP_BM;
    const T *fmap1 = M.r[MPC_IDX(M.ref_of[MPC_IDX(D.level_target[0][k], D.T)], M.R)].fmap1;
    const T *fmap2 = cp_level0(D, P, M, k, b);
    const cp_operand<T> A = {fmap1 + (long long)b * Dm * hw + m0, hw, (int)(hw - m0), (hw & 7) == 0 && cp_al16(fmap1)};
    const cp_operand<T> B = {fmap2 + n0, hw, (int)(hw - n0), (hw & 7) == 0 && cp_al16(fmap2)};
    // the operand this wave stages (waves 0, 1: A; 2, 3: B) -- uniform
    const bool stage_b = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 7)) != 0;
    const cp_operand<T> O = stage_b ? B : A;
    uint16_t *so = s_h + (stage_b ? CP_HTILE : 0);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // the fragments of lane (r = lane & 31, h = lane >> 5) in step ks: 8 k at [x + r][16 ks + 8 h]
    const uint16_t *fa = s_h + ((wv >> 1) * 64 + (lane & 31)) * CP_HLD + 8 * (lane >> 5);
    const uint16_t *fb = s_h + CP_HTILE + ((wv & 1) * 64 + (lane & 31)) * CP_HLD + 8 * (lane >> 5);
    uint4 r[4];
    cp_h_load(r, O, 0, Dm);
    for (int kb = 0; kb < Dm; kb += CP_HK) {
        __syncthreads();                                   // the previous block's fragments are read
        cp_h_store(so, r);
        __syncthreads();
        if (kb + CP_HK < Dm) cp_h_load(r, O, kb + CP_HK, Dm);
#pragma unroll
        for (int ks = 0; ks < CP_HK / 16; ++ks) {
            const uint4 a0 = *reinterpret_cast<const uint4 *>(fa + 16 * ks), a1 = *reinterpret_cast<const uint4 *>(fa + 32 * CP_HLD + 16 * ks);
            const uint4 b0 = *reinterpret_cast<const uint4 *>(fb + 16 * ks), b1 = *reinterpret_cast<const uint4 *>(fb + 32 * CP_HLD + 16 * ks);
            acc[0][0] = cp_mfma16(fmap1, a0, b0, acc[0][0]);
            acc[0][1] = cp_mfma16(fmap1, a0, b1, acc[0][1]);
            acc[1][0] = cp_mfma16(fmap1, a1, b0, acc[1][0]);
            acc[1][1] = cp_mfma16(fmap1, a1, b1, acc[1][1]);
        }
    }
    const int N = (int)hw;
    const long long row0 = (long long)k * D.B * hw + (long long)b * hw + m0;
    const long long ext = ((long long)D.level_n[0] * D.B * hw - row0) * N - n0;
    cp_write(acc, const_cast<float *>(D.level[0]) + row0 * N + n0, N, (int)(hw - m0), N - n0, true, P.sq, ext);
}

// P_l [n_l][B][D][pitch_l] from P_(l-1) (the fmap2 [n_r][B][D][hw] of the slot's reference at l = 1, of element type T): a thread per
// element, the pad of a row included
template <typename T>
__global__ __launch_bounds__(256) void k_corr_pyr_pool(const mpc_corr_desc D, const cp_plan P, const cp_refs<T> M, float *__restrict__ ws,
                                                       int l) {
    const int pitch = P.pitch[l], wl = D.level_w[l], N = D.level_h[l] * wl;
    const long long rows = (long long)D.level_n[l] * D.B * P.D, total = rows * pitch;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long row = e / pitch;
    const int j = (int)(e - row * pitch);
    float v = 0.f;
    if (j < N) {
        const int c = (int)(row % P.D);
        const long long kb = row / P.D;
        const int b = (int)(kb % D.B), k = (int)(kb / D.B), t = D.level_target[l][k];
        int u = 0;
        while (u < D.level_n[l - 1] - 1 && D.level_target[l - 1][u] != t) ++u;
        const int ws_ = D.level_w[l - 1];
        const T *src1 = nullptr;
        const float *src = nullptr;
        if (l == 1) {
            // the reference of target t by selects over the table (uniform reads): a per-thread index into it would cost loads
            const T *f2 = M.r[0].fmap2;
            [[maybe_unused]] int nr = M.r[0].level_n[0];           // (the extent of the checked index)
            int t0 = 0;
            for (int ri = 1; ri < M.R; ++ri)
                if (t >= M.r[ri].t0) { f2 = M.r[ri].fmap2; t0 = M.r[ri].t0; nr = M.r[ri].level_n[0]; }
            src1 = f2 + (((long long)MPC_IDX(t - t0, nr) * D.B + b) * P.D + c) * ((long long)D.h * D.w);
        } else {
            src = ws + P.p_off[l - 1] + MPC_IDX(((long long)u * D.B + b) * P.D + c, (long long)D.level_n[l - 1] * D.B * P.D) * P.pitch[l - 1];
        }
        const int y = j / wl, x = j - y * wl;
        if constexpr (std::is_same<T, float>::value) {
            const float *q = (l == 1 ? src1 : src) + (long long)(2 * y) * ws_ + 2 * x;
            v = (((q[0] + q[1]) + q[ws_]) + q[ws_ + 1]) * 0.25f;
        } else if (l == 1) {
            // the 16-bit map itself: converted at the load, then the same sums
            const T *q = src1 + (long long)(2 * y) * ws_ + 2 * x;
            v = (((mpc_ld(q) + mpc_ld(q + 1)) + mpc_ld(q + ws_)) + mpc_ld(q + ws_ + 1)) * 0.25f;
        } else {
            const float *q = src + (long long)(2 * y) * ws_ + 2 * x;
            v = (((q[0] + q[1]) + q[ws_]) + q[ws_ + 1]) * 0.25f;
        }
    }
    ws[P.p_off[l] + MPC_IDX(e, total)] = v;
}

// grad_fmap1 of every reference whose S > 1 (and that wants it), n = B * D * hw elements and ceil(n / 256) workgroups each (the
// reference is the workgroup's: its table entry is read once, uniformly): partial_0 + partial_1 + ... / sqrt(D)
template <typename T>
__global__ __launch_bounds__(256) void k_corr_pyr_reduce(const cp_plan P, const cp_refs<T> M, const float *__restrict__ ws, long long n) {
    const long long per = (n + 255) / 256;
    long long bid = blockIdx.x;
    int ri = 0;
    for (; ri < M.R; ++ri) {
        if (!M.r[ri].grad_fmap1 || M.r[ri].S <= 1) continue;
        if (bid < per) break;
        bid -= per;
    }
    MPC_EXPECT(ri < M.R);
    if (ri >= M.R) return;
    const cp_ref<T> &R = M.r[ri];
    const long long e = bid * 256 + threadIdx.x;
    if (e >= n) return;
    const float *part = ws + R.part_off;
    float v = part[MPC_IDX(e, n * R.S)];
    for (int s = 1; s < R.S; ++s) v = v + part[MPC_IDX((long long)s * n + e, n * R.S)];
    const float o = v / P.sq;
    mpc_st(&R.grad_fmap1[e], o);                        // (rounded once to T)
}

// a thread per element (V of them: 1, or MPC_VEC(T) = one 16-byte store) of the grad_fmap2 of every reference that wants it, whole
// workgroups per reference (its table entry is read uniformly); the fp32 sum is rounded once to T
template <int V, typename T>
__global__ __launch_bounds__(256) void k_corr_pyr_gather(const mpc_corr_desc D, const cp_plan P, const cp_refs<T> M, const float *__restrict__ ws) {
    const long long hw = (long long)D.h * D.w;
    long long bid = blockIdx.x;
    int ri = 0;
    for (; ri < M.R; ++ri) {
        if (!M.r[ri].grad_fmap2) continue;
        const long long cnt = ((long long)M.r[ri].level_n[0] * D.B * P.D * hw / V + 255) / 256;
        if (bid < cnt) break;
        bid -= cnt;
    }
    MPC_EXPECT(ri < M.R);
    if (ri >= M.R) return;
    const cp_ref<T> &R = M.r[ri];
    const long long total = (long long)R.level_n[0] * D.B * P.D * hw;
    const long long e = (bid * 256 + threadIdx.x) * V;                            // V > 1: w % V == 0, the V elements share a row
    if (e >= total) return;
    const long long row = e / hw;                      // (k * B + b) * D + c, k the reference's own target
    const int pix = (int)(e - row * hw), y = pix / D.w, x = pix - y * D.w;
    const long long tb = row / P.D;
    const int c = (int)(row - tb * P.D), b = (int)(tb % D.B), t = R.t0 + (int)(tb / D.B);
    float v[V];
#pragma unroll
    for (int u = 0; u < V; ++u) v[u] = 0.f;
    float wgt = 1.f;
    for (int l = 0; l < R.num_levels; ++l, wgt *= 0.25f) {
        if (!D.grad_level[l]) continue;
        int k = -1;
        for (int u = 0; u < R.level_n[l]; ++u) if (D.level_target[l][MPC_IDX(R.slot0[l] + u, D.level_n[l])] == t) k = u;
        const int yl = y >> l, wl = D.level_w[l];
        if (k < 0 || yl >= D.level_h[l]) continue;
        const long long rows = (long long)R.level_n[l] * D.B * P.D;
        for (int s = 0; s < R.S1; ++s) {
            const float *gp = ws + R.gp_off[l] + MPC_IDX(s * rows + ((long long)k * D.B + b) * P.D + c, rows * R.S1) * P.pitch[l] + yl * wl;
            if (V == 4 && l == 0) {
                const float4 q = *reinterpret_cast<const float4 *>(gp + MPC_IDX(x, wl - 3));
                v[0] = v[0] + q.x; v[1 % V] = v[1 % V] + q.y; v[2 % V] = v[2 % V] + q.z; v[3 % V] = v[3 % V] + q.w;
            } else if (V == 8 && l == 0) {
                const float4 q = *reinterpret_cast<const float4 *>(gp + MPC_IDX(x, wl - 7));
                const float4 p = *reinterpret_cast<const float4 *>(gp + MPC_IDX(x + 4, wl - 3));
                v[0] = v[0] + q.x; v[1 % V] = v[1 % V] + q.y; v[2 % V] = v[2 % V] + q.z; v[3 % V] = v[3 % V] + q.w;
                v[4 % V] = v[4 % V] + p.x; v[5 % V] = v[5 % V] + p.y; v[6 % V] = v[6 % V] + p.z; v[7 % V] = v[7 % V] + p.w;
            } else {
#pragma unroll
                for (int u = 0; u < V; ++u) {
                    const int xl = (x + u) >> l;
                    if (xl < wl) v[u] = v[u] + wgt * gp[MPC_IDX(xl, wl)];
                }
            }
        }
    }
    T *out = R.grad_fmap2 + MPC_IDX(e, total - (V - 1));
    if constexpr (V > 1) mpc_store_vec(out, v);
    else mpc_st(out, v[0]);
}

// ---- host

static int cp_check(const char *who, const mpc_corr_desc *D, int Dm) {
    if (!D) { mpc_set_error("%s: null descriptor", who); return MPC_E_NULL; }
    if (D->B < 0 || D->h < 1 || D->w < 1 || D->T < 1 || D->num_levels < 1 || Dm < 1) {
        mpc_set_error("%s: bad B / h / w / T / num_levels / D", who); return MPC_E_SHAPE;
    }
    if (Dm < 4 || Dm > CP_MAX_D || (Dm & 3) || D->T > MPC_CORR_MAX_TARGETS || D->num_levels > MPC_CORR_MAX_LEVELS) {
        mpc_set_error("%s: D %d is not a multiple of 4 in [4, %d], T %d > %d or %d levels > %d", who, Dm, CP_MAX_D, D->T,
                      MPC_CORR_MAX_TARGETS, D->num_levels, MPC_CORR_MAX_LEVELS);
        return MPC_E_UNSUPPORTED;
    }
    for (int l = 0; l < D->num_levels; ++l) {
        const int hl = D->level_h[l], wl = D->level_w[l], n = D->level_n[l];
        if (hl != (D->h >> l) || wl != (D->w >> l)) { mpc_set_error("%s: level %d is %d x %d, expected %d x %d", who, l, hl, wl, D->h >> l, D->w >> l); return MPC_E_SHAPE; }
        if (hl < 1 || wl < 1) { mpc_set_error("%s: level %d is empty (%d x %d)", who, l, hl, wl); return MPC_E_SHAPE; }
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
    }
    const long long hw = (long long)D->h * D->w;
    if (hw > (1ll << 24) || (long long)D->B * hw > (1ll << 30) || (long long)D->B * hw * D->T * hw > (1ll << 42) ||
        (long long)D->T * D->B * Dm * hw > (1ll << 38)) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    return 0;
}

static int cp_check_refs(const char *who, const mpc_corr_desc *D, const mpc_corr_refs *refs) {
    if (!refs) { mpc_set_error("%s: null references", who); return MPC_E_NULL; }
    if (refs->R < 1 || refs->R > MPC_CORR_MAX_REFS) {
        mpc_set_error("%s: %d references, 1 to %d are served", who, refs->R, MPC_CORR_MAX_REFS); return MPC_E_UNSUPPORTED;
    }
    bool ok = refs->first_target[0] == 0 && refs->first_target[refs->R] == D->T;
    for (int r = 0; r < refs->R; ++r) ok = ok && refs->first_target[r] < refs->first_target[r + 1];
    if (!ok) {
        mpc_set_error("%s: first_target does not cover the %d targets: it must rise from 0 to T, a target or more per reference", who, D->T);
        return MPC_E_SHAPE;
    }
    return 0;
}

// The workspace layout and every reference's split.  A reference's split is that of the single-reference problem of the reference
// alone, from its sizes only (S1: as if every level had a cotangent), so that equal calls -- and the single-reference call of the
// same reference -- sum in equal order.  `all_levels`: size for a cotangent at every level (the workspace query); else by
// desc->grad_level.  Pointers are not set here.
template <typename T>
static cp_plan cp_make_plan(const mpc_corr_desc *D, int Dm, const mpc_corr_refs *refs, int backward, bool all_levels, cp_refs<T> &M) {
    cp_plan P = {};
    M = {};
    const long long hw = (long long)D->h * D->w;
    P.D = Dm;
    P.sq = sqrtf((float)Dm);
    long long off = 0;
    for (int l = 0; l < D->num_levels; ++l) {
        P.pitch[l] = (D->level_h[l] * D->level_w[l] + 3) / 4 * 4;
        if (l >= 1) { P.p_off[l] = off; off += (long long)D->level_n[l] * D->B * Dm * P.pitch[l]; }
    }
    M.R = refs->R;
    for (int r = 0; r < refs->R; ++r) {
        cp_ref<T> &R = M.r[r];
        const int t0 = refs->first_target[r], t1 = refs->first_target[r + 1];
        R.t0 = t0; R.S = 1; R.S1 = 1;
        for (int t = t0; t < t1; ++t) M.ref_of[t] = (unsigned char)r;
        for (int l = 0; l < D->num_levels; ++l) {
            int first = -1, n = 0;
            for (int s = 0; s < D->level_n[l]; ++s) {
                const int t = D->level_target[l][s];
                if (t >= t0 && t < t1) { if (first < 0) first = s; ++n; }
            }
            R.slot0[l] = std::max(first, 0); R.level_n[l] = n;
            if (n > 0) R.num_levels = l + 1;
        }
        if (!backward) continue;
        // the two backward products have few tiles at batch 1: split k until about three workgroups per CU, at least four k
        // blocks each
        long long tiles1 = 0;
        for (int l = 0; l < R.num_levels; ++l)
            tiles1 += (long long)R.level_n[l] * std::max(D->B, 1) * ((Dm + CP_BM - 1) / CP_BM) * ((D->level_h[l] * D->level_w[l] + CP_BM - 1) / CP_BM);
        R.S1 = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(CP_MAX_SPLIT, (768 + tiles1 - 1) / tiles1), (hw + CP_BK - 1) / CP_BK / 4));
        for (int l = 0; l < R.num_levels; ++l) {
            R.gp_off[l] = off; off += (long long)R.S1 * R.level_n[l] * D->B * Dm * P.pitch[l];
            if (all_levels || D->grad_level[l]) R.kblocks += R.level_n[l] * ((D->level_h[l] * D->level_w[l] + CP_BK - 1) / CP_BK);
        }
        const long long tiles = (long long)std::max(D->B, 1) * ((Dm + CP_BM - 1) / CP_BM) * ((hw + CP_BM - 1) / CP_BM);
        long long S = std::min<long long>(CP_MAX_SPLIT, (768 + tiles - 1) / tiles);
        S = std::max<long long>(1, std::min<long long>(S, R.kblocks / 4));
        R.S = (int)S;
        R.part_off = off;
        if (R.S > 1) off += (long long)R.S * D->B * Dm * hw;
    }
    P.total = off;
    return P;
}

// (the pointers of mpc_corr_refs are typed float for the fp32 calls; a `_dt` call reads them as its element type)
static mpc_corr_refs cp_one_ref(const mpc_corr_desc *D, const void *fmap1, const void *fmap2, void *grad_fmap1, void *grad_fmap2) {
    mpc_corr_refs refs = {};
    refs.R = 1;
    refs.first_target[1] = D ? D->T : 0;
    refs.fmap1[0] = (const float *)fmap1; refs.fmap2[0] = (const float *)fmap2;
    refs.grad_fmap1[0] = (float *)grad_fmap1; refs.grad_fmap2[0] = (float *)grad_fmap2;
    return refs;
}

// the descriptor of reference r alone: what the single-reference entry points take for it
static mpc_corr_desc cp_ref_desc(const mpc_corr_desc *D, const cp_refs<float> &M, int r) {
    mpc_corr_desc d = *D;
    const cp_ref<float> &R = M.r[r];
    d.T = R.level_n[0]; d.num_levels = R.num_levels;
    for (int l = 0; l < MPC_CORR_MAX_LEVELS; ++l) {
        d.level_n[l] = l < R.num_levels ? R.level_n[l] : 0;
        for (int s = 0; s < MPC_CORR_MAX_TARGETS; ++s)
            d.level_target[l][s] = l < R.num_levels && s < R.level_n[l] ? (uint8_t)(D->level_target[l][R.slot0[l] + s] - R.t0) : 0;
    }
    return d;
}

static long long cp_workspace_bytes(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, int backward) {
    cp_refs<float> M;                                    // (the layout does not depend on the element type)
    return std::max<long long>(16, cp_make_plan(desc, D, refs, backward, true, M).total * (long long)sizeof(float));
}

extern "C" int mpc_corr_pyramid_supported(const mpc_corr_desc *desc, int D) { return cp_check(__func__, desc, D); }

extern "C" long long mpc_corr_pyramid_workspace_bytes(const mpc_corr_desc *desc, int D, int backward) {
    const int rc = cp_check(__func__, desc, D);
    if (rc) return rc;
    const mpc_corr_refs one = cp_one_ref(desc, nullptr, nullptr, nullptr, nullptr);
    return cp_workspace_bytes(desc, D, &one, backward);
}

extern "C" int mpc_corr_pyramid_multi_supported(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs) {
    const int rc = cp_check(__func__, desc, D);
    return rc ? rc : cp_check_refs(__func__, desc, refs);
}

// the sum of what the single-reference query gives for every reference alone (each at least 16 bytes); the layout needs no more
extern "C" long long mpc_corr_pyramid_multi_workspace_bytes(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, int backward) {
    int rc = cp_check(__func__, desc, D);
    if (!rc) rc = cp_check_refs(__func__, desc, refs);
    if (rc) return rc;
    cp_refs<float> M;
    cp_make_plan(desc, D, refs, 0, true, M);
    long long bytes = 0;
    for (int r = 0; r < refs->R; ++r) {
        const mpc_corr_desc d = cp_ref_desc(desc, M, r);
        const mpc_corr_refs one = cp_one_ref(&d, nullptr, nullptr, nullptr, nullptr);
        bytes += cp_workspace_bytes(&d, D, &one, backward);
    }
    return bytes;
}

template <typename T>
static int cp_pool_levels(const mpc_corr_desc *desc, const cp_plan &P, const cp_refs<T> &M, float *ws, hipStream_t st) {
    for (int l = 1; l < desc->num_levels; ++l) {
        const long long total = (long long)desc->level_n[l] * desc->B * P.D * P.pitch[l];
        MPC_LAUNCH(k_corr_pyr_pool<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, *desc, P, M, ws, l);
    }
    return 0;
}

#define CP_LDS (2 * CP_TILE * sizeof(float))

// `multi`: the list form (its references are checked too); the checks come first, whatever the element type
template <typename T>
static int cp_fwd(const char *who, const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, bool multi, void *ws, void *stream) {
    constexpr bool F32 = std::is_same<T, float>::value;
    int rc = cp_check(who, desc, D);
    if (!rc && multi) rc = cp_check_refs(who, desc, refs);
    if (rc) return rc;
    if (desc->B == 0) return 0;
    bool null = !ws || (((uintptr_t)ws) & 15);
    for (int r = 0; r < refs->R; ++r) null = null || !refs->fmap1[r] || !refs->fmap2[r];
    if (null) { mpc_set_error("%s: null argument (or a workspace that is not 16-byte aligned)", who); return MPC_E_NULL; }
    for (int l = 0; l < desc->num_levels; ++l) if (!desc->level[l]) { mpc_set_error("%s: level %d is null", who, l); return MPC_E_NULL; }
    cp_refs<T> M;
    const cp_plan P = cp_make_plan(desc, D, refs, 0, true, M);
    for (int r = 0; r < refs->R; ++r) { M.r[r].fmap1 = (const T *)refs->fmap1[r]; M.r[r].fmap2 = (const T *)refs->fmap2[r]; }
    const hipStream_t st = (hipStream_t)stream;
    cp_pool_levels(desc, P, M, (float *)ws, st);
    const long long hw = (long long)desc->h * desc->w, tm = (hw + CP_BM - 1) / CP_BM;
    // 16-bit maps: level 0 on the 16-bit matrix cores in a launch of its own, the levels above in the fp32 kernel
    const long long nb0 = F32 ? 0 : (long long)desc->level_n[0] * desc->B * tm * tm;
    long long nb = 0;
    for (int l = F32 ? 0 : 1; l < desc->num_levels; ++l)
        nb += (long long)desc->level_n[l] * desc->B * tm * ((desc->level_h[l] * desc->level_w[l] + CP_BM - 1) / CP_BM);
    if (nb > 0x7fffffffll || nb0 > 0x7fffffffll) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
    if constexpr (!F32) MPC_LAUNCH(k_corr_pyr_gemm16<T>, dim3((unsigned)nb0), dim3(256), 0, st, *desc, P, M);
    if (nb > 0) MPC_LAUNCH((k_corr_pyr_gemm<0, T>), dim3((unsigned)nb), dim3(256), CP_LDS, st, *desc, P, M, (float *)ws);
    MPC_CHECK_LAUNCH();
    return 0;
}

template <typename T>
static int cp_bwd(const char *who, const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, bool multi, void *ws, void *stream) {
    int rc = cp_check(who, desc, D);
    if (!rc && multi) rc = cp_check_refs(who, desc, refs);
    if (rc) return rc;
    bool want1 = false, want2 = false;
    for (int r = 0; r < refs->R; ++r) { want1 = want1 || refs->grad_fmap1[r]; want2 = want2 || refs->grad_fmap2[r]; }
    if (desc->B == 0 || (!want1 && !want2)) return 0;
    bool null = !ws || (((uintptr_t)ws) & 15);
    for (int r = 0; r < refs->R; ++r) null = null || !refs->fmap1[r] || !refs->fmap2[r];
    if (null) { mpc_set_error("%s: null argument (or a workspace that is not 16-byte aligned)", who); return MPC_E_NULL; }
    cp_refs<T> M;
    const cp_plan P = cp_make_plan(desc, D, refs, 1, false, M);
    for (int r = 0; r < refs->R; ++r) {
        M.r[r].fmap1 = (const T *)refs->fmap1[r]; M.r[r].fmap2 = (const T *)refs->fmap2[r];
        M.r[r].grad_fmap1 = (T *)refs->grad_fmap1[r]; M.r[r].grad_fmap2 = (T *)refs->grad_fmap2[r];
    }
    const hipStream_t st = (hipStream_t)stream;
    const long long hw = (long long)desc->h * desc->w, tm = (D + CP_BM - 1) / CP_BM;
    if (want1) {
        // the pooled feature maps, where a slot of a reference that wants grad_fmap1 reads one
        bool pooled = false;
        for (int r = 0; r < refs->R; ++r)
            for (int l = 1; l < M.r[r].num_levels; ++l) pooled = pooled || (refs->grad_fmap1[r] && desc->grad_level[l]);
        if (pooled) cp_pool_levels(desc, P, M, (float *)ws, st);
        long long nb = 0, reduced = 0;
        for (int r = 0; r < refs->R; ++r)
            if (refs->grad_fmap1[r]) { nb += (long long)M.r[r].S * desc->B * tm * ((hw + CP_BM - 1) / CP_BM); reduced += M.r[r].S > 1; }
        if (nb > 0x7fffffffll) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
        MPC_LAUNCH((k_corr_pyr_gemm<2, T>), dim3((unsigned)nb), dim3(256), CP_LDS, st, *desc, P, M, (float *)ws);
        if (reduced) {
            const long long n = (long long)desc->B * D * hw;
            MPC_LAUNCH(k_corr_pyr_reduce<T>, dim3((unsigned)(reduced * ((n + 255) / 256))), dim3(256), 0, st, P, M, (const float *)ws, n);
        }
    }
    if (want2) {
        long long nb = 0;
        bool al16 = true;
        for (int r = 0; r < refs->R; ++r) {
            if (!refs->grad_fmap2[r]) continue;
            al16 = al16 && (((uintptr_t)refs->grad_fmap2[r]) & 15) == 0;
            for (int l = 0; l < M.r[r].num_levels; ++l)
                if (desc->grad_level[l])
                    nb += (long long)M.r[r].S1 * M.r[r].level_n[l] * desc->B * tm * ((desc->level_h[l] * desc->level_w[l] + CP_BM - 1) / CP_BM);
        }
        if (nb > 0x7fffffffll) { mpc_set_error("%s: grid too large", who); return MPC_E_UNSUPPORTED; }
        if (nb > 0) MPC_LAUNCH((k_corr_pyr_gemm<1, T>), dim3((unsigned)nb), dim3(256), CP_LDS, st, *desc, P, M, (float *)ws);
        // one 16-byte store of MPC_VEC(T) elements (4 fp32, 8 of a 16-bit type) where a row is whole stores and the tensors are aligned
        const int V = desc->w % MPC_VEC(T) == 0 && al16 ? MPC_VEC(T) : 1;
        long long gb = 0;                                       // whole workgroups per reference that wants grad_fmap2
        for (int r = 0; r < refs->R; ++r)
            if (refs->grad_fmap2[r]) gb += ((long long)M.r[r].level_n[0] * desc->B * D * hw / V + 255) / 256;
        if (V > 1) MPC_LAUNCH((k_corr_pyr_gather<MPC_VEC(T), T>), dim3((unsigned)gb), dim3(256), 0, st, *desc, P, M, (const float *)ws);
        else MPC_LAUNCH((k_corr_pyr_gather<1, T>), dim3((unsigned)gb), dim3(256), 0, st, *desc, P, M, (const float *)ws);
    }
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_corr_pyramid_fwd_dt(const mpc_corr_desc *desc, int D, const void *fmap1, const void *fmap2, int32_t dtype, void *ws,
                                       void *stream) {
    const mpc_corr_refs one = cp_one_ref(desc, fmap1, fmap2, nullptr, nullptr);
    MPC_DT_RETURN(dtype, cp_fwd, desc, D, &one, false, ws, stream);
}

extern "C" int mpc_corr_pyramid_bwd_dt(const mpc_corr_desc *desc, int D, const void *fmap1, const void *fmap2, void *grad_fmap1,
                                       void *grad_fmap2, int32_t dtype, void *ws, void *stream) {
    const mpc_corr_refs one = cp_one_ref(desc, fmap1, fmap2, grad_fmap1, grad_fmap2);
    MPC_DT_RETURN(dtype, cp_bwd, desc, D, &one, false, ws, stream);
}

extern "C" int mpc_corr_pyramid_multi_fwd_dt(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, int32_t dtype, void *ws,
                                             void *stream) {
    MPC_DT_RETURN(dtype, cp_fwd, desc, D, refs, true, ws, stream);
}

extern "C" int mpc_corr_pyramid_multi_bwd_dt(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, int32_t dtype, void *ws,
                                             void *stream) {
    MPC_DT_RETURN(dtype, cp_bwd, desc, D, refs, true, ws, stream);
}

extern "C" int mpc_corr_pyramid_fwd(const mpc_corr_desc *desc, int D, const float *fmap1, const float *fmap2, void *ws, void *stream) {
    return mpc_corr_pyramid_fwd_dt(desc, D, fmap1, fmap2, MPC_DT_F32, ws, stream);
}

extern "C" int mpc_corr_pyramid_bwd(const mpc_corr_desc *desc, int D, const float *fmap1, const float *fmap2, float *grad_fmap1,
                                    float *grad_fmap2, void *ws, void *stream) {
    return mpc_corr_pyramid_bwd_dt(desc, D, fmap1, fmap2, grad_fmap1, grad_fmap2, MPC_DT_F32, ws, stream);
}

extern "C" int mpc_corr_pyramid_multi_fwd(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, void *ws, void *stream) {
    return mpc_corr_pyramid_multi_fwd_dt(desc, D, refs, MPC_DT_F32, ws, stream);
}

extern "C" int mpc_corr_pyramid_multi_bwd(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, void *ws, void *stream) {
    return mpc_corr_pyramid_multi_bwd_dt(desc, D, refs, MPC_DT_F32, ws, stream);
}

MPC_BOUNDS_UNIT("corr_pyramid.hip")
