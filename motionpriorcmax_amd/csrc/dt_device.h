// The element types of the network tensors the head kernels read in place (MPC_DT_F32 / _F16 / _BF16 of include/mpcmax.h): the coefficient
// grid of grid_traj.hip and tiles.hip, the convex-upsampling mask of cvx_device.h / cvx_curves.hip / pe_curves.hip, and their gradients.
//   load    mpc_ld: the element as fp32 -- fp16 by the hardware convert (v_cvt_f32_f16), bf16 as bits << 16: both exact, so everything
//           behind the load is the arithmetic of the fp32 kernel on the upcast tensor, bit for bit
//   store   mpc_bits<T>: the fp32 value rounded ONCE to the tensor's type, round to nearest even -- fp16 by the hardware convert (overflow
//           to +-inf, subnormals kept: the library is built with 16-bit denormals on), bf16 by the formula below, which is bit for bit
//           what torch.Tensor.to(torch.bfloat16) does:  NaN -> 0x7FC0;  otherwise u += 0x7FFF + ((u >> 16) & 1), u >>= 16
//   mpc_store_vec<T>: MPC_VEC<T> consecutive elements (4 fp32, 8 of a 16-bit type) as one 16-byte store; the address must be 16-byte aligned
// The `float` instantiations are the kernels as they were before the 16-bit types existed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct mpc_f16 { uint16_t u; };
struct mpc_bf16 { uint16_t u; };

__device__ __forceinline__ float mpc_ld(const float *p) { return *p; }
__device__ __forceinline__ float mpc_ld(const mpc_f16 *p) { return (float)*reinterpret_cast<const _Float16 *>(p); }
__device__ __forceinline__ float mpc_ld(const mpc_bf16 *p) { return __uint_as_float((uint32_t)p->u << 16); }

__device__ __forceinline__ uint16_t mpc_bf16_bits(float v) {
    uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ uint16_t mpc_f16_bits(float v) {
    // (an opaque value: left to itself the compiler folds a product in front of the conversion into v_fma_mixlo_f16 a, b, 0 -- ONE
    // rounding of the exact product instead of the fp32 rounding and then this one, and -0 + 0 = +0: not the fp32 kernel's element)
    asm("" : "+v"(v));
    const _Float16 h = (_Float16)v;
    return __builtin_bit_cast(uint16_t, h);
}

template <typename T> struct mpc_dt;
template <> struct mpc_dt<float> { static constexpr int VEC = 4; };
template <> struct mpc_dt<mpc_f16> { static constexpr int VEC = 8; };
template <> struct mpc_dt<mpc_bf16> { static constexpr int VEC = 8; };
#define MPC_VEC(T) (mpc_dt<T>::VEC)

__device__ __forceinline__ void mpc_st(float *p, float v) { *p = v; }
__device__ __forceinline__ void mpc_st(mpc_f16 *p, float v) { p->u = mpc_f16_bits(v); }
__device__ __forceinline__ void mpc_st(mpc_bf16 *p, float v) { p->u = mpc_bf16_bits(v); }

__device__ __forceinline__ void mpc_store_vec(float *p, const float v[4]) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void mpc_store_vec(mpc_f16 *p, const float v[8]) {
    uint4 q;
    q.x = mpc_f16_bits(v[0]) | ((uint32_t)mpc_f16_bits(v[1]) << 16); q.y = mpc_f16_bits(v[2]) | ((uint32_t)mpc_f16_bits(v[3]) << 16);
    q.z = mpc_f16_bits(v[4]) | ((uint32_t)mpc_f16_bits(v[5]) << 16); q.w = mpc_f16_bits(v[6]) | ((uint32_t)mpc_f16_bits(v[7]) << 16);
    *reinterpret_cast<uint4 *>(p) = q;
}
__device__ __forceinline__ void mpc_store_vec(mpc_bf16 *p, const float v[8]) {
    uint4 q;
    q.x = mpc_bf16_bits(v[0]) | ((uint32_t)mpc_bf16_bits(v[1]) << 16); q.y = mpc_bf16_bits(v[2]) | ((uint32_t)mpc_bf16_bits(v[3]) << 16);
    q.z = mpc_bf16_bits(v[4]) | ((uint32_t)mpc_bf16_bits(v[5]) << 16); q.w = mpc_bf16_bits(v[6]) | ((uint32_t)mpc_bf16_bits(v[7]) << 16);
    *reinterpret_cast<uint4 *>(p) = q;
}

// Host side: return fn<element type of `dtype`>(args) -- the ONE copy of an entry point's host code, which takes the typed tensors as
// void pointers --; an unknown code: MPC_E_UNSUPPORTED with an error string, nothing runs.
#define MPC_DT_RETURN(dtype, fn, ...)                                                                        \
    do {                                                                                                     \
        if ((dtype) == MPC_DT_F32) return fn<float>(__func__, __VA_ARGS__);                                  \
        if ((dtype) == MPC_DT_F16) return fn<mpc_f16>(__func__, __VA_ARGS__);                                \
        if ((dtype) == MPC_DT_BF16) return fn<mpc_bf16>(__func__, __VA_ARGS__);                              \
        mpc_set_error("%s: unknown dtype code %d (MPC_DT_F32, MPC_DT_F16 or MPC_DT_BF16)", __func__, (int)(dtype)); \
        return MPC_E_UNSUPPORTED;                                                                            \
    } while (0)
