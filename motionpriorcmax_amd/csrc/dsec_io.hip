// The DSEC flow files on the device: the 16-bit PNG payload [B][H][W][3] (uint16; channel 0 = x, 1 = y, 2 = valid) as imageio
// returns it and as the benchmark's submission takes it.
//
//  k_dsec_decode       reference src/loader/dsec/loader.py:174-180   payload -> forward_flow [B][2][H][W] (y, x) + flow_valid
//  k_dsec_err_partial  the same decode in the load of the flow error metrics (src/utils/flow.py:18-70, src/utils/metrics.py:50-56):
//                      no fp32 target and no mask in memory; the per-pixel body, the pixels of a thread and the order of the sums
//                      are those of k_flow_err_partial (flow_err_device.h), so both give the same bits
//  k_dsec_encode       scripts/dsec_inference.py:33-49 (scale_optical_flow + save_flow): dense flow -> payload
//
// All three stream: 6 B of payload per pixel against 8 B (+ 1 B) of planes.  A pixel is three 16-bit words, so neither a pixel nor
// a pair of pixels is a naturally aligned store; FOUR pixels are 24 B = three aligned 8-byte words, and that is the unit of a
// thread on the fast path (16-byte plane accesses, 8-byte payload accesses: the widest the 24-byte period allows with an 8-byte
// aligned base).  H * W not a multiple of 4, or a misaligned pointer: one pixel per thread, 2-byte accesses.
#include "common.h"
#include "flow_err_device.h"

struct DsecPx4 { unsigned short c[4][3]; };

// four consecutive pixels, 24 B from an 8-byte aligned address
__device__ __forceinline__ DsecPx4 dsec_load4(const unsigned short *__restrict__ png, long long i4) {
    const uint2 *q = reinterpret_cast<const uint2 *>(png) + i4 * 3;
    const uint2 a = q[0], b = q[1], c = q[2];
    const unsigned w[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
    DsecPx4 r;
#pragma unroll
    for (int k = 0; k < 12; ++k) r.c[k / 3][k % 3] = (unsigned short)((k & 1) ? (w[k >> 1] >> 16) : (w[k >> 1] & 0xffffu));
    return r;
}

// loader.py:176-177: (float32(v) - 2**15) / 128.  Exact in fp32: every uint16 is representable, the difference is an integer of at
// most 16 bits and 128 is a power of two.
__device__ __forceinline__ float dsec_flow(unsigned short v) { return ((float)v - 32768.f) * 0.0078125f; }

// grid ceil(pixels / 256) or ceil(quads / 256), 256 threads; HW = H * W, total = B * HW
template <bool VEC>
__global__ __launch_bounds__(256) void k_dsec_decode(const unsigned short *__restrict__ png, float *__restrict__ flow,
                                                     unsigned char *__restrict__ valid, long long HW, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        if (i * 4 >= total) return;
        const long long b = (i * 4) / HW, r = i * 4 - b * HW;          // (HW % 4 == 0: the four pixels lie in one sample)
        const DsecPx4 q = dsec_load4(png, i);
        float *f0 = flow + b * 2 * HW + r;
        *reinterpret_cast<float4 *>(f0) = make_float4(dsec_flow(q.c[0][1]), dsec_flow(q.c[1][1]), dsec_flow(q.c[2][1]), dsec_flow(q.c[3][1]));
        *reinterpret_cast<float4 *>(f0 + HW) = make_float4(dsec_flow(q.c[0][0]), dsec_flow(q.c[1][0]), dsec_flow(q.c[2][0]), dsec_flow(q.c[3][0]));
        *reinterpret_cast<uchar4 *>(valid + i * 4) = make_uchar4(q.c[0][2] != 0, q.c[1][2] != 0, q.c[2][2] != 0, q.c[3][2] != 0);   // :178 astype(bool)
    } else {
        if (i >= total) return;
        const long long b = i / HW, r = i - b * HW;
        const unsigned short *px = png + i * 3;
        flow[b * 2 * HW + r] = dsec_flow(px[1]);
        flow[b * 2 * HW + HW + r] = dsec_flow(px[0]);
        valid[i] = px[2] != 0;
    }
}

// grid (FE_BLOCKS, B), 256 threads: k_flow_err_partial (flow.hip) with the ground truth and the mask read from the payload
template <bool VEC>
__global__ __launch_bounds__(256) void k_dsec_err_partial(const mpc_err_shape s, const unsigned short *__restrict__ png,
                                                          const float *__restrict__ pred, const float *__restrict__ time_scale,
                                                          double *__restrict__ part) {
    __shared__ double s_red[4];
    const int b = blockIdx.y;
    const long long HW = (long long)s.H * s.W;
    const unsigned short *g = png + (long long)b * HW * 3;
    const float *p0 = pred + (long long)b * 2 * HW, *p1 = p0 + HW;
    const bool has_ts = time_scale != nullptr;
    const float ts = has_ts ? time_scale[b] : 1.f;
    FeAcc a;
#pragma unroll
    for (int k = 0; k < FE_NACC; ++k) a.v[k] = 0.0;
    if (VEC) {
        const long long n4 = HW >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)FE_BLOCKS * 256) {
            const DsecPx4 q = dsec_load4(g, i);
            const float4 b0 = reinterpret_cast<const float4 *>(p0)[i], b1 = reinterpret_cast<const float4 *>(p1)[i];
            fe_pixel(dsec_flow(q.c[0][1]), dsec_flow(q.c[0][0]), b0.x, b1.x, q.c[0][2] != 0, ts, has_ts, a);
            fe_pixel(dsec_flow(q.c[1][1]), dsec_flow(q.c[1][0]), b0.y, b1.y, q.c[1][2] != 0, ts, has_ts, a);
            fe_pixel(dsec_flow(q.c[2][1]), dsec_flow(q.c[2][0]), b0.z, b1.z, q.c[2][2] != 0, ts, has_ts, a);
            fe_pixel(dsec_flow(q.c[3][1]), dsec_flow(q.c[3][0]), b0.w, b1.w, q.c[3][2] != 0, ts, has_ts, a);
        }
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)FE_BLOCKS * 256)
            fe_pixel(dsec_flow(g[i * 3 + 1]), dsec_flow(g[i * 3]), p0[i], p1[i], g[i * 3 + 2] != 0, ts, has_ts, a);
    }
#pragma unroll
    for (int k = 0; k < FE_NACC; ++k) {
        const double r = block_sum_d<256>(a.v[k], s_red);
        if (threadIdx.x == 0) part[((long long)b * FE_BLOCKS + blockIdx.x) * FE_NACC + k] = r;
    }
}

// scripts/dsec_inference.py:33-49 for one pixel, operation by operation in fp32 (the build has -ffp-contract=off; sqrtf and / are
// the correctly rounded ones: no fast-math anywhere in this library).  u = flow[0] (y), v = flow[1] (x).
//   :35  magnitude = sqrt(u**2 + v**2)            two products, one sum
//   :36  exceed = magnitude > max                 strict
//   :38-39  u = (u / magnitude) * max, likewise v both with the magnitude of :35
//   :47-48  (flow * 128 + 2**15).astype(uint16)   truncation
// UNPINNED (numpy's cast of such values is undefined): a pixel with a NaN or infinite component gets payload 0 in both channels;
// a finite q below 0 / above 65535 (only with max_magnitude >= 256) saturates.
__device__ __forceinline__ void dsec_quant(float u, float v, float maxm, unsigned short &qx, unsigned short &qy) {
    const bool finite = fabsf(u) < INFINITY && fabsf(v) < INFINITY;          // (false for NaN)
    const float mag = sqrtf(u * u + v * v);
    if (mag > maxm) { u = (u / mag) * maxm; v = (v / mag) * maxm; }
    const float a = u * 128.f + 32768.f, b = v * 128.f + 32768.f;
    qy = finite && a == a ? (unsigned short)(int)fminf(fmaxf(a, 0.f), 65535.f) : (unsigned short)0;
    qx = finite && b == b ? (unsigned short)(int)fminf(fmaxf(b, 0.f), 65535.f) : (unsigned short)0;
}

// grid ceil(pixels / 256) or ceil(quads / 256), 256 threads
template <bool VEC>
__global__ __launch_bounds__(256) void k_dsec_encode(const float *__restrict__ flow, float maxm, unsigned short *__restrict__ png,
                                                     long long HW, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        if (i * 4 >= total) return;
        const long long b = (i * 4) / HW, r = i * 4 - b * HW;
        const float *f0 = flow + b * 2 * HW + r;
        const float4 u = *reinterpret_cast<const float4 *>(f0), v = *reinterpret_cast<const float4 *>(f0 + HW);
        unsigned short x[4], y[4];
        dsec_quant(u.x, v.x, maxm, x[0], y[0]); dsec_quant(u.y, v.y, maxm, x[1], y[1]);
        dsec_quant(u.z, v.z, maxm, x[2], y[2]); dsec_quant(u.w, v.w, maxm, x[3], y[3]);
        // 12 words (x0 y0 0 | x1 y1 0 | x2 y2 0 | x3 y3 0) as three 8-byte stores
        uint2 *o = reinterpret_cast<uint2 *>(png) + i * 3;
        o[0] = make_uint2((unsigned)x[0] | ((unsigned)y[0] << 16), (unsigned)x[1] << 16);
        o[1] = make_uint2((unsigned)y[1], (unsigned)x[2] | ((unsigned)y[2] << 16));
        o[2] = make_uint2((unsigned)x[3] << 16, (unsigned)y[3]);
    } else {
        if (i >= total) return;
        const long long b = i / HW, r = i - b * HW;
        unsigned short x, y;
        dsec_quant(flow[b * 2 * HW + r], flow[b * 2 * HW + HW + r], maxm, x, y);
        png[i * 3] = x; png[i * 3 + 1] = y; png[i * 3 + 2] = 0;
    }
}

// ------------------------------------------------------------------------------------------------------
static int dsec_validate(int32_t B, int32_t H, int32_t W) {
    MPC_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, MPC_E_SHAPE, "bad shape");
    MPC_CHECK_ARG((int64_t)B * H * W < (1LL << 31), MPC_E_UNSUPPORTED, "too many pixels");          // (one thread per pixel on the slow path)
    return 0;
}

extern "C" int mpc_dsec_flow_decode(const uint16_t *png16, float *flow, uint8_t *valid, int32_t B, int32_t H, int32_t W, void *stream) {
    MPC_CHECK_ARG(png16 && flow && valid, MPC_E_NULL, "null argument");
    int rc = dsec_validate(B, H, W);
    if (rc) return rc;
    MPC_CHECK_ARG(((uintptr_t)png16 & 1) == 0 && ((uintptr_t)flow & 3) == 0, MPC_E_UNSUPPORTED, "misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long HW = (long long)H * W, total = HW * B;
    const bool vec = (HW & 3) == 0 && ((uintptr_t)png16 & 7) == 0 && ((uintptr_t)flow & 15) == 0 && ((uintptr_t)valid & 3) == 0;
    if (vec)
        MPC_LAUNCH(k_dsec_decode<true>, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, st, png16, flow, valid, HW, total);
    else
        MPC_LAUNCH(k_dsec_decode<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, png16, flow, valid, HW, total);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t mpc_dsec_flow_error_workspace_bytes(const mpc_err_shape *s) { return mpc_flow_error_workspace_bytes(s); }

extern "C" int mpc_dsec_flow_error(const mpc_err_shape *s, const uint16_t *png16, const float *flow_pred, const float *time_scale,
                                   float *out, void *ws, void *stream) {
    MPC_CHECK_ARG(s && png16 && flow_pred && out && ws, MPC_E_NULL, "null argument");
    MPC_CHECK_ARG(s->B >= 1 && s->B <= 65535 && s->H >= 1 && s->W >= 1, MPC_E_SHAPE, "bad shape");
    MPC_CHECK_ARG(((uintptr_t)png16 & 1) == 0 && ((uintptr_t)flow_pred & 3) == 0, MPC_E_UNSUPPORTED, "misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long HW = (long long)s->H * s->W;
    const bool vec = (HW & 3) == 0 && ((uintptr_t)flow_pred & 15) == 0 && ((uintptr_t)png16 & 7) == 0;
    if (vec)
        MPC_LAUNCH(k_dsec_err_partial<true>, dim3(FE_BLOCKS, s->B), dim3(256), 0, st, *s, png16, flow_pred, time_scale, (double *)ws);
    else
        MPC_LAUNCH(k_dsec_err_partial<false>, dim3(FE_BLOCKS, s->B), dim3(256), 0, st, *s, png16, flow_pred, time_scale, (double *)ws);
    mpc_flow_err_final(s, (const double *)ws, out, st);
    MPC_CHECK_LAUNCH();
    return 0;
}

extern "C" int mpc_dsec_flow_encode(const float *flow, float max_magnitude, uint16_t *png16, int32_t B, int32_t H, int32_t W, void *stream) {
    MPC_CHECK_ARG(flow && png16, MPC_E_NULL, "null argument");
    int rc = dsec_validate(B, H, W);
    if (rc) return rc;
    MPC_CHECK_ARG(((uintptr_t)png16 & 1) == 0 && ((uintptr_t)flow & 3) == 0, MPC_E_UNSUPPORTED, "misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long HW = (long long)H * W, total = HW * B;
    const bool vec = (HW & 3) == 0 && ((uintptr_t)png16 & 7) == 0 && ((uintptr_t)flow & 15) == 0;
    if (vec)
        MPC_LAUNCH(k_dsec_encode<true>, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, st, flow, max_magnitude, png16, HW, total);
    else
        MPC_LAUNCH(k_dsec_encode<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, flow, max_magnitude, png16, HW, total);
    MPC_CHECK_LAUNCH();
    return 0;
}
