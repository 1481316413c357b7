// pair augmentation: a batch of uint8 frame pairs (B,2,H,W,Cin), as the image reader returns them, -> the flipped, colour-jittered fp32 `source` / `driving`
// batches (B,3,H,W) of the training step (augmentation.py:325-355 with the flip_param / jitter_param of both training configs).  Entry and rules:
// include/mrfa_data_hip.h (that comment is the specification); the per-pixel arithmetic: augment_math.h, shared with the host tests.
//
// Like frames.hip: NT = 256, grid-stride, no atomics, every output has one writer.  blockIdx.y is the FRAME (2 b + t); the descriptors of all pairs are a
// launch argument, so a workgroup's ops, factors and flips are uniform (scalar registers) and nothing on the device needs keeping alive.
//
// luma_sum_kernel<CIN, QUAD> -- launched only when some pair has contrast; workgroups of the other pairs leave at once.  gridDim.x = MRFA_AUG_PARTS: workgroup
//   p strides over its frame's items, takes each pixel through the ops that PRECEDE contrast, and writes one 32-bit sum of the lumas to partials[frame][p]
//   (255 H W / 64 < 2^32 by MRFA_AUG_MAX_PIXELS).  Integer adds: any order gives the same bits.  Every slot the apply pass reads is written: no zeroing.
// apply_kernel<CIN, QUAD> -- thread 0 adds the frame's 64 partials in index order into 64 bits and forms m; then every item goes through the whole chain, the
//   flips and byte * fl32(1 / 255).
// QUAD (W % 4 == 0): an item is four consecutive pixels of a row -- Cin dwords in where src is 4-byte aligned (`vload`; frame offsets are multiples of 4 then),
//   single bytes otherwise; one float4 per plane out where source / driving are 16-byte aligned (`vstore`), four scalars otherwise.  With hflip the lane that
//   owns output quad q of a row reads input quad W / 4 - 1 - q and reverses it.  Otherwise an item is one pixel: byte loads, scalar stores.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "mrfa_data_hip.h"
#include "augment_math.h"

void mrfa_data_set_error(const char* fmt, ...);

#define MRFA_DATA_CHECK_ARG(cond, ...)            \
    do {                                          \
        if (!(cond)) {                            \
            mrfa_data_set_error(__VA_ARGS__);     \
            return 1;                             \
        }                                         \
    } while (0)

static_assert(MRFA_AUG_NONE == AUG_NONE && MRFA_AUG_BRIGHTNESS == AUG_BRIGHTNESS && MRFA_AUG_CONTRAST == AUG_CONTRAST &&
              MRFA_AUG_SATURATION == AUG_SATURATION && MRFA_AUG_HUE == AUG_HUE, "augment_math.h and mrfa_data_hip.h number the ops alike");
static_assert(sizeof(mrfa_pair_aug) == 20, "mrfa_pair_aug is 20 bytes (mrfa_amd/data_hip.py mirrors it)");

namespace {

constexpr int NT = 256;
constexpr float INV255 = (float)(1.0 / 255.0);        // fl32(1 / 255)

struct AugSet { mrfa_pair_aug p[MRFA_AUG_MAX_PAIRS]; };

// the uniform part of a workgroup: its pair's descriptor in registers
struct Chain {
    unsigned char op[4];
    float factor[3];
    unsigned hue_shift;
    bool contrast;
};

__device__ __forceinline__ Chain chain_of(const mrfa_pair_aug& a) {
    Chain c;
    c.contrast = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c.op[k] = a.op[k];
        c.contrast |= a.op[k] == MRFA_AUG_CONTRAST;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) c.factor[k] = a.factor[k];
    c.hue_shift = a.hue_shift;
    return c;
}

template <int CIN>
__device__ __forceinline__ AugRgb pixel_at(const unsigned char* s) {
    AugRgb c;
    c.r = s[0];
    c.g = CIN == 1 ? c.r : s[1];
    c.b = CIN == 1 ? c.r : s[2];
    return c;
}

// the four pixels that start at byte `s` (4 CIN bytes): CIN dwords, or bytes
template <int CIN>
__device__ __forceinline__ void quad_at(const unsigned char* s, bool vload, AugRgb px[4]) {
    if (vload) {
        unsigned w[CIN];
#pragma unroll
        for (int k = 0; k < CIN; ++k) w[k] = reinterpret_cast<const unsigned*>(s)[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int byte = CIN == 1 ? j : j * CIN + c;             // grey: the one value in all three channels; CIN 4: byte 3 of a pixel is never used
                v[c] = (w[byte >> 2] >> (8 * (byte & 3))) & 0xffu;
            }
            px[j].r = v[0], px[j].g = v[1], px[j].b = v[2];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j] = pixel_at<CIN>(s + j * CIN);
    }
}

template <int CIN, bool QUAD>
__global__ __launch_bounds__(NT) void luma_sum_kernel(const AugSet set, const unsigned char* __restrict__ src, long long HW, int vload,
                                                      unsigned* __restrict__ partials) {
    const int fr = blockIdx.y;
    const Chain ch = chain_of(set.p[fr >> 1]);
    if (!ch.contrast) return;
    const unsigned char* frame = src + (size_t)fr * HW * CIN;
    const long long items = QUAD ? HW / 4 : HW, stride = (long long)MRFA_AUG_PARTS * NT;
    unsigned acc = 0;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < items; i += stride) {
        if (QUAD) {
            AugRgb px[4];
            quad_at<CIN>(frame + (size_t)i * 4 * CIN, vload != 0, px);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const AugRgb c = aug_chain(px[j], ch.op, ch.factor, ch.hue_shift, 0u, true);
                acc += aug_luma(c.r, c.g, c.b);
            }
        } else {
            const AugRgb c = aug_chain(pixel_at<CIN>(frame + (size_t)i * CIN), ch.op, ch.factor, ch.hue_shift, 0u, true);
            acc += aug_luma(c.r, c.g, c.b);
        }
    }
    __shared__ unsigned s_acc[NT];
    s_acc[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_acc[threadIdx.x] += s_acc[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[(size_t)fr * MRFA_AUG_PARTS + blockIdx.x] = s_acc[0];
}

__device__ __forceinline__ float unit_of_byte(unsigned v) { return __fmul_rn((float)v, INV255); }

template <int CIN, bool QUAD>
__global__ __launch_bounds__(NT) void apply_kernel(const AugSet set, const unsigned char* __restrict__ src, int H, int W, int vload, int vstore,
                                                   const unsigned* __restrict__ partials, float* __restrict__ source, float* __restrict__ driving) {
    const int fr = blockIdx.y, b = fr >> 1;
    const mrfa_pair_aug& a = set.p[b];
    const Chain ch = chain_of(a);
    const bool hflip = a.hflip != 0;
    const long long HW = (long long)H * W;
    __shared__ unsigned s_part[MRFA_AUG_PARTS];
    __shared__ unsigned s_mean;
    unsigned mean = 0;
    if (ch.contrast) {                                                      // (uniform over the workgroup)
        if (threadIdx.x < MRFA_AUG_PARTS) s_part[threadIdx.x] = partials[(size_t)fr * MRFA_AUG_PARTS + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long S = 0;
            for (int k = 0; k < MRFA_AUG_PARTS; ++k) S += s_part[k];
            s_mean = aug_contrast_mean(S, (unsigned long long)HW);
        }
        __syncthreads();
        mean = s_mean;
    }
    const unsigned char* frame = src + (size_t)fr * HW * CIN;
    const bool second = ((fr & 1) != 0) != (a.time_flip != 0);              // this frame is the pair's `driving`
    float* dst = (second ? driving : source) + (size_t)b * 3 * HW;
    const long long stride = (long long)gridDim.x * NT;
    if (QUAD) {
        const int QW = W >> 2;
        const long long items = (long long)H * QW;
        for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < items; i += stride) {
            const long long r = i / QW;
            const int q = (int)(i - r * QW), qin = hflip ? QW - 1 - q : q;
            AugRgb px[4];
            quad_at<CIN>(frame + ((size_t)r * W + (size_t)qin * 4) * CIN, vload != 0, px);
            float v[3][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const AugRgb c = aug_chain(px[j], ch.op, ch.factor, ch.hue_shift, mean, false);
                const int jo = hflip ? 3 - j : j;
                v[0][jo] = unit_of_byte(c.r), v[1][jo] = unit_of_byte(c.g), v[2][jo] = unit_of_byte(c.b);
            }
            float* d = dst + (size_t)r * W + (size_t)q * 4;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (vstore) {
                    f32x4 o;
                    o[0] = v[c][0], o[1] = v[c][1], o[2] = v[c][2], o[3] = v[c][3];
                    *reinterpret_cast<f32x4*>(d + (size_t)c * HW) = o;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) d[(size_t)c * HW + j] = v[c][j];
                }
            }
        }
    } else {
        for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < HW; i += stride) {
            const long long r = i / W;
            const int x = (int)(i - r * W), xin = hflip ? W - 1 - x : x;
            const AugRgb c = aug_chain(pixel_at<CIN>(frame + ((size_t)r * W + xin) * CIN), ch.op, ch.factor, ch.hue_shift, mean, false);
            dst[i] = unit_of_byte(c.r);
            dst[HW + i] = unit_of_byte(c.g);
            dst[2 * HW + i] = unit_of_byte(c.b);
        }
    }
}

template <int CIN, bool QUAD>
void launch(hipStream_t st, const AugSet& set, bool contrast, const unsigned char* src, int B, int H, int W, bool vload, bool vstore, unsigned* partials,
            float* source, float* driving) {
    const long long HW = (long long)H * W, items = QUAD ? HW / 4 : HW;
    if (contrast)
        hipLaunchKernelGGL((luma_sum_kernel<CIN, QUAD>), dim3(MRFA_AUG_PARTS, 2 * B), dim3(NT), 0, st, set, src, HW, (int)vload, partials);
    hipLaunchKernelGGL((apply_kernel<CIN, QUAD>), dim3((unsigned)stream_grid(items, NT), 2 * B), dim3(NT), 0, st, set, src, H, W, (int)vload, (int)vstore,
                       partials, source, driving);
}

template <int CIN>
void launch_cin(hipStream_t st, const AugSet& set, bool contrast, const unsigned char* src, int B, int H, int W, unsigned* partials, float* source,
                float* driving) {
    if (W % 4 == 0)
        launch<CIN, true>(st, set, contrast, src, B, H, W, (reinterpret_cast<uintptr_t>(src) & 3u) == 0, aligned16(source) && aligned16(driving), partials,
                          source, driving);
    else
        launch<CIN, false>(st, set, contrast, src, B, H, W, false, false, partials, source, driving);
}

bool dims_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && (long long)H * W <= MRFA_AUG_MAX_PIXELS; }

}  // namespace

extern "C" long long mrfa_pair_augment_workspace(int B, int H, int W) {
    if (!dims_ok(B, H, W) || B > MRFA_AUG_MAX_PAIRS) return -1;
    return 2LL * B * MRFA_AUG_PARTS * (long long)sizeof(unsigned);
}

extern "C" int mrfa_pair_augment(void* stream, const unsigned char* src, int B, int H, int W, int Cin, const mrfa_pair_aug* params, void* workspace,
                                 long long workspace_bytes, float* source, float* driving) {
    MRFA_DATA_CHECK_ARG(src && params && workspace && source && driving, "pair_augment: null pointer (src %p, params %p, workspace %p, source %p, driving %p)",
                        (const void*)src, (const void*)params, workspace, (void*)source, (void*)driving);
    MRFA_DATA_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "pair_augment: B, H and W must be >= 1 (B %d, H %d, W %d)", B, H, W);
    MRFA_DATA_CHECK_ARG((long long)H * W <= MRFA_AUG_MAX_PIXELS, "pair_augment: H W must be <= %lld (H %d, W %d)", (long long)MRFA_AUG_MAX_PIXELS, H, W);
    MRFA_DATA_CHECK_ARG(B <= MRFA_AUG_MAX_PAIRS, "pair_augment: B must be <= %d pairs per call (B %d)", MRFA_AUG_MAX_PAIRS, B);
    MRFA_DATA_CHECK_ARG(Cin == 1 || Cin == 3 || Cin == 4, "pair_augment: Cin must be 1 (grey), 3 or 4 (alpha is dropped), not %d", Cin);
    AugSet set;
    memset(&set, 0, sizeof set);
    bool contrast = false;
    for (int b = 0; b < B; ++b) {
        const mrfa_pair_aug& a = params[b];
        unsigned seen = 0;
        for (int k = 0; k < 4; ++k) {
            const int o = a.op[k];
            MRFA_DATA_CHECK_ARG(o <= MRFA_AUG_HUE, "pair_augment: pair %d: op[%d] is %d, not one of 0 (none) .. %d", b, k, o, MRFA_AUG_HUE);
            MRFA_DATA_CHECK_ARG(o == MRFA_AUG_NONE || !(seen >> o & 1u), "pair_augment: pair %d: op %d appears twice", b, o);
            seen |= 1u << o;
        }
        for (int k = 0; k < 3; ++k)
            MRFA_DATA_CHECK_ARG(isfinite(a.factor[k]) && a.factor[k] >= 0.f, "pair_augment: pair %d: factor[%d] must be finite and >= 0 (%g)", b, k,
                                (double)a.factor[k]);
        contrast |= (seen >> MRFA_AUG_CONTRAST & 1u) != 0;
        set.p[b] = a;
    }
    const long long need = mrfa_pair_augment_workspace(B, H, W);
    MRFA_DATA_CHECK_ARG(workspace_bytes >= need, "pair_augment: the workspace has %lld bytes, mrfa_pair_augment_workspace(%d, %d, %d) asks for %lld",
                        workspace_bytes, B, H, W, need);
    MRFA_DATA_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "pair_augment: workspace %p must be 8-byte aligned", workspace);
    MRFA_DATA_CHECK_ARG(((reinterpret_cast<uintptr_t>(source) | reinterpret_cast<uintptr_t>(driving)) & 3u) == 0,
                        "pair_augment: source %p and driving %p must be 4-byte aligned (fp32 stores)", (void*)source, (void*)driving);
    const hipStream_t st = (hipStream_t)stream;
    unsigned* partials = static_cast<unsigned*>(workspace);
    if (Cin == 1)
        launch_cin<1>(st, set, contrast, src, B, H, W, partials, source, driving);
    else if (Cin == 3)
        launch_cin<3>(st, set, contrast, src, B, H, W, partials, source, driving);
    else
        launch_cin<4>(st, set, contrast, src, B, H, W, partials, source, driving);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        mrfa_data_set_error("mrfa_pair_augment: launch failed: %s", hipGetErrorString(e));
        return 2;
    }
    return 0;
}
