// The output side shared by the kernels that hand something to a device consumer as tensors (vp8_side.hip, vp8_residual.hip, vp8_coef.hip, the
// vp8_trace*.hip through vp8_trace_read.hip.h and, for the walk and the planar store, vp8_rgb.hip): the element of a dtype,
// value x scale as the element's bits, the map between an output grid and the samples it is laid over in both directions, the share
// of a row range among workgroups, the store of four neighbouring elements and a lane's walk over a row range in groups of four.
#pragma once
#include <hip/hip_fp16.h>
#include "vp8_common.hip.h"

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

// an element as the unsigned integer of its size: by bytes, and by TENSOR_* dtype
template <int ES> struct TensorUint;
template <> struct TensorUint<1> { typedef unsigned char T; };
template <> struct TensorUint<2> { typedef unsigned short T; };
template <> struct TensorUint<4> { typedef unsigned int T; };
template <int DTYPE> struct TensorElem : TensorUint<DTYPE == TENSOR_F32 ? 4 : DTYPE == TENSOR_U8 ? 1 : 2> {};

// v (an int16; TENSOR_U8: a byte) as the bits of an element: itself, or v x scale as a float / a half
template <int DTYPE>
__device__ __forceinline__ unsigned tensor_value(int v, float scale)
{
    if constexpr (DTYPE == TENSOR_I16) return (unsigned)v & 0xffffu;
    else if constexpr (DTYPE == TENSOR_U8) return (unsigned)v & 0xffu;
    else {
        // (float)((double)v * (double)scale): the product of an int16 and a float is exact in double, so this is that product
        // rounded once -- which is what the single-precision multiply gives (denormal results kept: the kernels' float mode)
        const float f = __fmul_rn((float)v, scale);
        if constexpr (DTYPE == TENSOR_F32) return __float_as_uint(f);
        else return (unsigned)__half_as_ushort(__float2half_rn(f));
    }
}

// v[0..3] (int16 each) x one scale as the bits of four elements: tensor_value four times -- but the halves are made two at a time, by
// the packed conversion.  Asked for one at a time, the compiler may fuse the multiply and the conversion of a half into one
// v_fma_mixlo_f16, which rounds the exact product once (the definition rounds twice: to a float, then to a half) and gives +0 for -0.
template <int DTYPE>
__device__ __forceinline__ void tensor_values4(const int (&v)[4], float scale, unsigned (&e)[4])
{
    if constexpr (DTYPE != TENSOR_F16) {
#pragma unroll
        for (int i = 0; i < 4; i++) e[i] = tensor_value<DTYPE>(v[i], scale);
    } else {
        typedef float f32x2_t __attribute__((ext_vector_type(2)));
        typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
            const f32x2_t f = {__fmul_rn((float)v[i], scale), __fmul_rn((float)v[i + 1], scale)};
            const unsigned u = __builtin_bit_cast(unsigned, __builtin_convertvector(f, f16x2_t));
            e[i] = u & 0xffffu;
            e[i + 1] = u >> 16;
        }
    }
}

// the centre map: the sample output i of a grid of g takes, the grid laid over d samples
__device__ __forceinline__ int tensor_src(int i, int g, int d)
{
    return (int)(((unsigned)(2 * i + 1) * (unsigned)d) / (unsigned)(2 * g));
}

// its inverse: the first output whose sample is T or beyond (g where none is): ((2i + 1) * d) / (2g) >= T  <=>  (2i + 1) * d >= 2 * g * T
__device__ __forceinline__ int tensor_first(int T, int g, int d)
{
    const int num = 2 * g * T - d;               // (T <= 16384, g <= 16383: below 2^30)
    return num <= 0 ? 0 : min((num + 2 * d - 1) / (2 * d), g);
}

// rows a .. b - 1 shared by S workgroups: the share of number `part`
__device__ __forceinline__ void tensor_share(int a, int b, int S, int part, int &y0, int &y1)
{
    const int per = (b - a + S - 1) / S;
    y0 = a + part * per;
    y1 = min(b, y0 + per);
}

// The elements e[0..3] of ES bytes for four neighbouring columns of a row as one piece at o, which is aligned to it: a dword of bytes,
// 8 bytes of int16 / halves, 16 of floats.  For a group whose four all belong to the caller, where the tensor takes whole pieces
// (width a multiple of 4; destination and stride aligned to the piece).  Every other group goes element by element at the call
// site -- each element exactly once, none outside the caller's range: as a function that loop compiles to more registers.
template <int ES>
__device__ __forceinline__ void tensor_store4(uint8_t *o, const unsigned (&e)[4])
{
    if constexpr (ES == 1) *(g_u32p)o = e[0] | e[1] << 8 | e[2] << 16 | e[3] << 24;
    else if constexpr (ES == 2) *(GLOBAL_AS u32x2_t *)o = u32x2_t{e[0] | e[1] << 16, e[2] | e[3] << 16};
    else *(GLOBAL_AS u32x4_t *)o = u32x4_t{e[0], e[1], e[2], e[3]};
}

// A lane's walk over rows of nq groups of four, the workgroup's 256 lanes on neighbouring groups: from group threadIdx.x in steps
// of 256 groups, as (row, col).  for (TensorWalk t(nq); t.row < nrows; t.next())
struct TensorWalk {
    int nq, adv_rows, adv_cols, row, col;
    __device__ __forceinline__ TensorWalk(int nq_)
        : nq(nq_), adv_rows(256 / nq_), adv_cols(256 - adv_rows * nq_), row((int)threadIdx.x / nq_), col((int)threadIdx.x - row * nq_) {}
    __device__ __forceinline__ void next()
    {
        col += adv_cols;
        row += adv_rows;
        if (col >= nq) { col -= nq; row++; }
    }
};
