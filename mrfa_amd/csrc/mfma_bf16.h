// The arithmetic shared by the kernels on the bf16 matrix pipe (conv_split / conv_halo / conv_lean / wgrad_split / wgrad_halo / wgrad_lean):
// fp32 operands split EXACTLY into three bf16 pieces (or rounded to one), the order of the six products, the transposing LDS fragment read
// and the statistics reduction of the transposed epilogues.  conv_split.hip's file head explains the split.
#pragma once
#include "common.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((__vector_size__(4 * sizeof(__bf16)))) __bf16 bf16x4_t;

__device__ __forceinline__ unsigned pack_hi16(float a, float b) {      // (bf16 chop of b) << 16 | (bf16 chop of a)
    return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
__device__ __forceinline__ float chop_rest(float x) { return x - __uint_as_float(__float_as_uint(x) & 0xffff0000u); }
// plain bf16 operands (NP = 1): round-to-nearest-even of the fp32 value, one product -- the arithmetic of a bf16 autocast
__device__ __forceinline__ unsigned rne16(float x) {
    const unsigned u = __float_as_uint(x);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// N consecutive k of one row -> bf16 pairs packed into dwords.  NP = number of products kept: 6 / 3: the three exact pieces p1 + p2 + p3 = x (bf16x3
// launches ignore p3); 1: p1 = the values rounded to nearest even, p2 / p3 untouched.
template <int NP, int N, typename V>
__device__ __forceinline__ void bf16_pieces(const float (&x)[N], V& p1, V& p2, V& p3) {
#pragma unroll
    for (int h = 0; h < N / 2; ++h) {
        if constexpr (NP == 1) {
            p1[h] = rne16(x[2 * h]) | (rne16(x[2 * h + 1]) << 16);
        } else {
            const float a = x[2 * h], b = x[2 * h + 1];
            p1[h] = pack_hi16(a, b);
            const float ar = chop_rest(a), br = chop_rest(b);
            p2[h] = pack_hi16(ar, br);
            p3[h] = pack_hi16(chop_rest(ar), chop_rest(br));
        }
    }
}
// 4 consecutive k -> bf16x4 pieces (2 dwords each); 8 consecutive k (wgrad_split.hip) go through the array form above
template <int NP>
__device__ __forceinline__ void bf16_pieces(const f32x4 v, u32x2& p1, u32x2& p2, u32x2& p3) {
    if constexpr (NP == 1) {
        p1[0] = rne16(v.x) | (rne16(v.y) << 16);
        p1[1] = rne16(v.z) | (rne16(v.w) << 16);
    } else {
        const float x[4] = {v.x, v.y, v.z, v.w};
        bf16_pieces<NP>(x, p1, p2, p3);
    }
}

// transposing fragment read: rows (pixels) k0 .. k0+7 of this lane's channel column of a pixel-major [pixel][64 B] LDS image as one MFMA operand
// (two ds_read_b64_tr_b16; wgrad_halo.hip's file head describes the lane mapping)
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* p) {
    typedef __attribute__((address_space(3))) bf16x4_t* lds4;
    const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)(p));
    const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)(p + 4 * 64));
    bf16x8 r;
    __builtin_memcpy(&r, &lo, 8);
    __builtin_memcpy(reinterpret_cast<char*>(&r) + 8, &hi, 8);
    return r;
}

// the six products a[PA[t]] * b[PB[t]] (piece indices, 0 = leading), smallest first; bf16x3 runs t = 3..5, plain bf16 t = 5
inline constexpr int PA[6] = {2, 0, 1, 1, 0, 0};
inline constexpr int PB[6] = {0, 2, 1, 0, 1, 0};

// Statistics of the transposed (D = W X^T) epilogues: a lane holds 16 per-channel partial sums (4 quads x 4 channels) of its pixel; the sums over the
// 32 pixel lanes of a half are formed by a butterfly reduce-scatter (16 shuffles for the 16 values).  Afterwards v[0] of lane L is the total of value
// index kk = 8 b4 + 4 b3 + 2 b2 + b1 (bN = bit N of L); lanes L and L ^ 1 hold the same total.
template <int W>
__device__ __forceinline__ void reduce_scatter_stage(float (&v)[16], int lane) {      // lanes L / L ^ 2W: the low one keeps v[0..W), the high one v[W..2W)
    const bool hi = (lane & (2 * W)) != 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const float send = hi ? v[k] : v[k + W];
        const float keep = hi ? v[k + W] : v[k];
        v[k] = keep + __shfl_xor(send, 2 * W, 64);
    }
}
__device__ __forceinline__ void reduce_scatter16(float (&v)[16], int lane) {
    reduce_scatter_stage<8>(v, lane);
    reduce_scatter_stage<4>(v, lane);
    reduce_scatter_stage<2>(v, lane);
    reduce_scatter_stage<1>(v, lane);
    v[0] += __shfl_xor(v[0], 1, 64);
}
// the lane -> channel decode: value kk is channel (kk & 3) of quad kk >> 2, quads 8 channels apart; cb = the lane's first channel
__device__ __forceinline__ int reduce_scatter16_index(int lane) {
    return ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
}
__device__ __forceinline__ int reduce_scatter16_channel(int cb, int lane) {
    const int kk = ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
    return cb + 8 * (kk >> 2) + (kk & 3);
}
