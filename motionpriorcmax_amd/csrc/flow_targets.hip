// Ground-truth flow targets of the EVIMO2 and MultiFlow configurations: what the reference's DataLoader workers
// make of the raw multi-step flow before validation_step compares predictions with it --
//   mode 0 (EVIMO2, src/loader/evimo2/datasubset.py:171-188): validity = neither channel NaN, NaN -> 0 element by element,
//     F.interpolate(bilinear, align_corners=False) to Ho x Wo, channel 0 * fp32(Wo / W), channel 1 * fp32(Ho / H); the validity and
//     the object-id mask by F.interpolate(nearest);
//   mode 1 (MultiFlow, src/loader/multiflow/sample.py:108-139, downsample=True): channels-last input (the np.moveaxis folded into
//     the read), F.interpolate(bilinear, align_corners=True), then / 2 (a multiply by 0.5: exact); no NaN treatment, no mask --
// as ONE launch that reads the raw flow once and writes every output element once (nothing to pre-zero, no workspace).
//
// A thread owns four consecutive elements of the flat [B][S][Ho][Wo] pixel index: both channels of each pixel and its validity
// come from the same four taps per channel (the nearest tap is read again only where it is none of them; at the shipped ratio
// 1.25 it always is the bilinear i0), the four validity bytes leave as one 32-bit store, and with Wo % 4 == 0 and 16-byte
// aligned outputs the four pixels lie in one row and each channel leaves as one float4 (VEC); otherwise every pixel is decoded
// on its own and the flow is stored by the element.  The object-id mask is further work items of the same launch.  The taps are
// plain loads served by L1 / L2: neighbouring lanes read neighbouring columns of the same two rows, and every input line is
// fetched from HBM once (profiles/flow_targets.json has the achieved rate).
#include "common.h"
#include "resize_src.h"

struct TgtGeom {
    int H, W, Ho, Wo;
    float sh, sw;         // mode 0: float(H) / Ho, float(W) / Wo;  mode 1: float(H - 1) / (Ho - 1), float(W - 1) / (Wo - 1)
    float mx, my;         // what channel 0 / channel 1 is multiplied by after the blend
};

// F.interpolate(mode='nearest'): min(floor(j * scale), size - 1)
__host__ __device__ __forceinline__ int tgt_nearest(float scale, int j, int size) {
    const int i = (int)floorf((float)j * scale);
    return i < size - 1 ? i : size - 1;
}

// F.interpolate(mode='bilinear', align_corners=True): scale * j, the neighbour clamped to the last entry
__host__ __device__ __forceinline__ void tgt_src_aligned(float scale, int j, int size, int &i0, int &i1, float &lam) {
    const float r = scale * (float)j;
    i0 = (int)r;
    if (i0 > size - 1) i0 = size - 1;
    i1 = i0 < size - 1 ? i0 + 1 : i0;
    lam = fminf(fmaxf(r - (float)i0, 0.f), 1.f);
}

__device__ __forceinline__ float tgt_zero_nan(float v) { return v != v ? 0.f : v; }

// upsample_bilinear2d: columns blended first, rows last
__device__ __forceinline__ float tgt_blend(float v00, float v01, float v10, float v11, float lx, float ly) {
    const float top = (1.f - lx) * v00 + lx * v01;
    const float bot = (1.f - lx) * v10 + lx * v11;
    return (1.f - ly) * top + ly * bot;
}

// output pixel (j, i) of one (sample, step) image `img`: both channels, and (mode 0) its validity as 0 / 1
template <int MODE>
__device__ __forceinline__ void tgt_pixel(const TgtGeom &G, const float *__restrict__ img, int j, int i, float &ox, float &oy, unsigned &valid) {
    const int W = G.W;
    int y0, y1, x0, x1;
    float ly, lx;
    if (MODE == 0) {
        repr_src(G.sh, j, G.H, 1, y0, y1, ly);
        repr_src(G.sw, i, W, 1, x0, x1, lx);
        const float *__restrict__ c0 = img, *__restrict__ c1 = img + (size_t)G.H * W;
        const size_t r0 = (size_t)y0 * W, r1 = (size_t)y1 * W;
        float a00 = c0[r0 + x0], a01 = c0[r0 + x1], a10 = c0[r1 + x0], a11 = c0[r1 + x1];
        float b00 = c1[r0 + x0], b01 = c1[r0 + x1], b10 = c1[r1 + x0], b11 = c1[r1 + x1];
        // the nearest tap: one of the four just read, or (a ratio at which it is none of them) two more loads
        const int ny = tgt_nearest(G.sh, j, G.H), nx = tgt_nearest(G.sw, i, W);
        float va, vb;
        if ((ny == y0 || ny == y1) && (nx == x0 || nx == x1)) {
            va = ny == y0 ? (nx == x0 ? a00 : a01) : (nx == x0 ? a10 : a11);
            vb = ny == y0 ? (nx == x0 ? b00 : b01) : (nx == x0 ? b10 : b11);
        } else {
            va = c0[(size_t)ny * W + nx];
            vb = c1[(size_t)ny * W + nx];
        }
        valid = (va != va || vb != vb) ? 0u : 1u;                    // datasubset.py:171
        a00 = tgt_zero_nan(a00); a01 = tgt_zero_nan(a01); a10 = tgt_zero_nan(a10); a11 = tgt_zero_nan(a11);          // :173
        b00 = tgt_zero_nan(b00); b01 = tgt_zero_nan(b01); b10 = tgt_zero_nan(b10); b11 = tgt_zero_nan(b11);
        ox = tgt_blend(a00, a01, a10, a11, lx, ly) * G.mx;           // :187-188, one fp32 multiply after the blend
        oy = tgt_blend(b00, b01, b10, b11, lx, ly) * G.my;
    } else {
        tgt_src_aligned(G.sh, j, G.H, y0, y1, ly);
        tgt_src_aligned(G.sw, i, W, x0, x1, lx);
        const size_t p00 = ((size_t)y0 * W + x0) * 2, p01 = ((size_t)y0 * W + x1) * 2, p10 = ((size_t)y1 * W + x0) * 2, p11 = ((size_t)y1 * W + x1) * 2;
        ox = tgt_blend(img[p00], img[p01], img[p10], img[p11], lx, ly) * G.mx;              // sample.py:137
        oy = tgt_blend(img[p00 + 1], img[p01 + 1], img[p10 + 1], img[p11 + 1], lx, ly) * G.my;
        valid = 1u;
    }
}

// grid ceil((nq_flow + nq_id) / blockDim), 64 or 256 threads.  Work items [0, nq_flow): four pixels of flow (+ validity) each;
// [nq_flow, nq_flow + nq_id): four elements of the resized object-id mask each.
template <int MODE, bool VEC>
__device__ __forceinline__ void tgt_items(const TgtGeom &G, const float *__restrict__ raw, const float *__restrict__ id_mask,
                                          float *__restrict__ flow, uint8_t *__restrict__ valid, float *__restrict__ id_out,
                                          long long n_flow, long long nq_flow, long long n_id, long long nq_id) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Wo = G.Wo;
    const long long HoWo = (long long)G.Ho * Wo, HW = (long long)G.H * G.W;
    if (t < nq_flow) {
        const long long e0 = t * 4;
        if (VEC) {                                                   // Wo % 4 == 0: one row, one image; 16-byte stores
            const long long bs = e0 / HoWo;
            const int rem = (int)(e0 - bs * HoWo), j = rem / Wo, i = rem - j * Wo;
            const float *img = raw + (size_t)bs * 2 * HW;
            float4 fx, fy;
            unsigned v0, v1, v2, v3;
            tgt_pixel<MODE>(G, img, j, i, fx.x, fy.x, v0);
            tgt_pixel<MODE>(G, img, j, i + 1, fx.y, fy.y, v1);
            tgt_pixel<MODE>(G, img, j, i + 2, fx.z, fy.z, v2);
            tgt_pixel<MODE>(G, img, j, i + 3, fx.w, fy.w, v3);
            float *dst = flow + (size_t)bs * 2 * HoWo + rem;
            *reinterpret_cast<float4 *>(dst) = fx;
            *reinterpret_cast<float4 *>(dst + HoWo) = fy;
            if (MODE == 0) *reinterpret_cast<uint32_t *>(valid + e0) = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
        } else {
            unsigned packed = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long e = e0 + k;
                if (e >= n_flow) break;
                const long long bs = e / HoWo;
                const int rem = (int)(e - bs * HoWo), j = rem / Wo, i = rem - j * Wo;
                float ox, oy;
                unsigned v;
                tgt_pixel<MODE>(G, raw + (size_t)bs * 2 * HW, j, i, ox, oy, v);
                float *dst = flow + (size_t)bs * 2 * HoWo + rem;
                dst[0] = ox;
                dst[HoWo] = oy;
                packed |= v << (8 * k);
            }
            if (MODE == 0) {
                if (e0 + 4 <= n_flow) *reinterpret_cast<uint32_t *>(valid + e0) = packed;       // (valid is 4-byte aligned: checked on the host)
                else for (long long e = e0; e < n_flow; ++e) valid[e] = (uint8_t)((packed >> (8 * (int)(e - e0))) & 0xffu);       // the last 1..3 bytes of the array
            }
        }
        return;
    }
    const long long q = t - nq_flow;
    if (q >= nq_id) return;
    const long long e0 = q * 4;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long e = e0 + k;
        if (e >= n_id) break;
        const long long b = e / HoWo;
        const int rem = (int)(e - b * HoWo), j = rem / Wo, i = rem - j * Wo;
        o[k] = id_mask[(size_t)b * HW + (size_t)tgt_nearest(G.sh, j, G.H) * G.W + tgt_nearest(G.sw, i, G.W)];          // datasubset.py:182
    }
    if (VEC) {
        *reinterpret_cast<float4 *>(id_out + e0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (e0 + k < n_id) id_out[e0 + k] = o[k];
    }
}

// the two store paths under names of their own (the kernel timer and the tests tell them apart)
template <int MODE>
__global__ __launch_bounds__(256) void k_flow_targets_vec(const TgtGeom G, const float *__restrict__ raw, const float *__restrict__ id_mask,
                                                          float *__restrict__ flow, uint8_t *__restrict__ valid, float *__restrict__ id_out,
                                                          long long n_flow, long long nq_flow, long long n_id, long long nq_id) {
    tgt_items<MODE, true>(G, raw, id_mask, flow, valid, id_out, n_flow, nq_flow, n_id, nq_id);
}
template <int MODE>
__global__ __launch_bounds__(256) void k_flow_targets_elem(const TgtGeom G, const float *__restrict__ raw, const float *__restrict__ id_mask,
                                                           float *__restrict__ flow, uint8_t *__restrict__ valid, float *__restrict__ id_out,
                                                           long long n_flow, long long nq_flow, long long n_id, long long nq_id) {
    tgt_items<MODE, false>(G, raw, id_mask, flow, valid, id_out, n_flow, nq_flow, n_id, nq_id);
}

// ------------------------------------------------------------------------------------------
static int targets_check(const char *who, const mpc_targets_shape *s) {
    if (!s) { mpc_set_error("%s: null shape", who); return MPC_E_NULL; }
    if (s->B < 1 || s->S < 1 || s->H < 1 || s->W < 1 || s->Ho < 1 || s->Wo < 1) {
        mpc_set_error("%s: B, S, H, W, Ho, Wo must be at least 1 (got %d %d %d %d %d %d)", who, s->B, s->S, s->H, s->W, s->Ho, s->Wo); return MPC_E_SHAPE;
    }
    if ((s->mode != 0 && s->mode != 1) || (s->has_id != 0 && s->has_id != 1)) { mpc_set_error("%s: mode and has_id must be 0 or 1", who); return MPC_E_SHAPE; }
    if (s->mode == 1 && (s->Ho < 2 || s->Wo < 2)) {
        mpc_set_error("%s: mode 1 (align_corners=True) divides by Ho - 1 and Wo - 1: both must be at least 2 (got %d x %d)", who, s->Ho, s->Wo); return MPC_E_SHAPE;
    }
    if (s->mode == 1 && s->has_id) { mpc_set_error("%s: mode 1 (MultiFlow) has no object-id mask", who); return MPC_E_SHAPE; }
    const long long in = (long long)s->B * s->S * 2 * s->H * s->W, out = (long long)s->B * s->S * 2 * s->Ho * s->Wo;
    if ((long long)s->H * s->W >= (1ll << 30) || (long long)s->Ho * s->Wo >= (1ll << 30) || in >= (1ll << 40) || out >= (1ll << 40)) {
        mpc_set_error("%s: flow block too large", who); return MPC_E_UNSUPPORTED;
    }
    return 0;
}

extern "C" int mpc_flow_targets_supported(const mpc_targets_shape *s) { return targets_check(__func__, s); }

extern "C" int mpc_flow_targets(const mpc_targets_shape *s, const float *raw_flow, const float *id_mask, float *flow, uint8_t *flow_valid,
                                float *id_out, void *stream) {
    const int rc = targets_check(__func__, s);
    if (rc) return rc;
    MPC_CHECK_ARG(raw_flow && flow && (s->mode == 1 || flow_valid) && (!s->has_id || (id_mask && id_out)), MPC_E_NULL, "null argument");
    MPC_CHECK_ARG((reinterpret_cast<uintptr_t>(flow) & 3) == 0 && (s->mode == 1 || (reinterpret_cast<uintptr_t>(flow_valid) & 3) == 0), MPC_E_UNSUPPORTED,
                  "flow and flow_valid must be 4-byte aligned (the validity bytes are stored four at a time)");
    TgtGeom G;
    G.H = s->H; G.W = s->W; G.Ho = s->Ho; G.Wo = s->Wo;
    if (s->mode == 0) {
        G.sh = (float)s->H / (float)s->Ho;                            // area_pixel_compute_scale
        G.sw = (float)s->W / (float)s->Wo;
        G.mx = (float)((double)s->Wo / (double)s->W);                 // datasubset.py:185-188: a Python float, rounded to fp32 by the multiply
        G.my = (float)((double)s->Ho / (double)s->H);
    } else {
        G.sh = (float)(s->H - 1) / (float)(s->Ho - 1);
        G.sw = (float)(s->W - 1) / (float)(s->Wo - 1);
        G.mx = G.my = 0.5f;                                           // sample.py:137
    }
    const long long n_flow = (long long)s->B * s->S * s->Ho * s->Wo, nq_flow = (n_flow + 3) / 4;
    const long long n_id = s->has_id ? (long long)s->B * s->Ho * s->Wo : 0, nq_id = (n_id + 3) / 4;
    const bool vec = (s->Wo & 3) == 0 && (reinterpret_cast<uintptr_t>(flow) & 15) == 0 && (!s->has_id || (reinterpret_cast<uintptr_t>(id_out) & 15) == 0);
    // a few workgroups per CU at one 384 x 512 image (49152 work items): single-wave workgroups until there are enough of 256
    const long long items = nq_flow + nq_id;
    const int block = items >= 256ll * 1024 ? 256 : 64;
    const long long nblk = (items + block - 1) / block;
    MPC_CHECK_ARG(nblk <= 0x7fffffffll, MPC_E_UNSUPPORTED, "grid too large");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk), blk(block);
    if (s->mode == 0) {
        if (vec) MPC_LAUNCH(k_flow_targets_vec<0>, grid, blk, 0, st, G, raw_flow, id_mask, flow, flow_valid, id_out, n_flow, nq_flow, n_id, nq_id);
        else MPC_LAUNCH(k_flow_targets_elem<0>, grid, blk, 0, st, G, raw_flow, id_mask, flow, flow_valid, id_out, n_flow, nq_flow, n_id, nq_id);
    } else {
        if (vec) MPC_LAUNCH(k_flow_targets_vec<1>, grid, blk, 0, st, G, raw_flow, id_mask, flow, flow_valid, id_out, n_flow, nq_flow, n_id, nq_id);
        else MPC_LAUNCH(k_flow_targets_elem<1>, grid, blk, 0, st, G, raw_flow, id_mask, flow, flow_valid, id_out, n_flow, nq_flow, n_id, nq_id);
    }
    MPC_CHECK_LAUNCH();
    return 0;
}
