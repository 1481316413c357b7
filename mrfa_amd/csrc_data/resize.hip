// frame resize: uint8 frames (N,Hi,Wi,Cin), cropped to a box and resized to (Ho,Wo) with Pillow's bytes, -> fp32 (N,3,Ho,Wo) and / or uint8 (N,Ho,Wo,3).
// Entries and rules: include/mrfa_resize_hip.h (that comment is the specification); the coefficient tables: resize_coeffs.h, shared with the host test.
//
// resize_kernel<CIN, STAGE>: NT = 256, one workgroup per TH x TW = 8 x 32 tile of output pixels of one frame (blockIdx.z).  CH = 1 channel for grey, 3 otherwise.
//   1. STAGE (both ksize <= MRFA_RESIZE_LDS_TAPS, every reduction below 21x Lanczos): the tile's rows of both tables go to LDS (kk_h: TW rows of ksize_h
//      ints, kk_v: TH rows of ksize_v; ksize is odd, so lanes that read the same tap of consecutive columns hit different banks).  Longer rows, up to
//      MRFA_RESIZE_MAX_TAPS, are read where they lie (the second instantiation, whose LDS goes to a footprint of twice the rows instead).
//   2. rounds (one, unless the vertical footprint of the tile exceeds FOOT rows): for the output rows [ya, yb) whose source rows [f0, f1) fit,
//      horizontal pass: item (row r, column x, channel c), c fastest -> the byte s_rows[r][x CH + c], read straight from global memory (a lane walks cnt
//      bytes Cin apart; neighbouring lanes are scale Cin bytes apart, so a wave's loads share cache lines);
//      vertical pass: item (y, x, c) sums s_rows[ymin - f0 + k][x CH + c] * kk_v[y][k] -- a wave reads consecutive bytes of one row -- and writes the three
//      bytes of the pixel (grey: one value three times) to s_out[y][3 x + c].
//   3. s_out -> global: one float4 per (plane, row, four columns) and one dword per four bytes of a row where `vec` allows, scalars otherwise.
// Every output has one writer, nothing is accumulated across workgroups: no atomics, nothing to zero, every run bit-identical.
#include <stdint.h>
#include <vector>

#include "common.h"
#include "mrfa_resize_hip.h"
#include "resize_coeffs.h"

void mrfa_data_set_error(const char* fmt, ...);

#define MRFA_RESIZE_CHECK(cond, rc, ...)          \
    do {                                          \
        if (!(cond)) {                            \
            mrfa_data_set_error(__VA_ARGS__);     \
            return rc;                            \
        }                                         \
    } while (0)

static_assert(MRFA_RESIZE_BOX == mrfa_resize::FILTER_BOX && MRFA_RESIZE_BILINEAR == mrfa_resize::FILTER_BILINEAR &&
              MRFA_RESIZE_HAMMING == mrfa_resize::FILTER_HAMMING && MRFA_RESIZE_BICUBIC == mrfa_resize::FILTER_BICUBIC &&
              MRFA_RESIZE_LANCZOS == mrfa_resize::FILTER_LANCZOS, "resize_coeffs.h and mrfa_resize_hip.h number the filters alike");

namespace {

constexpr int NT = 256, TH = 8, TW = 32;
constexpr int LDS_TAPS = MRFA_RESIZE_LDS_TAPS, FOOT_STAGED = MRFA_RESIZE_FOOT_ROWS, FOOT_LONG = 2 * MRFA_RESIZE_FOOT_ROWS;
constexpr int ROUND = 1 << (mrfa_resize::PRECISION_BITS - 1);
constexpr float INV255 = (float)(1.0 / 255.0);        // fl32(1 / 255)
static_assert(FOOT_STAGED >= LDS_TAPS && FOOT_LONG >= MRFA_RESIZE_MAX_TAPS, "one output row's taps always fit a round");
static_assert(TW * LDS_TAPS * 4 + TH * LDS_TAPS * 4 + FOOT_STAGED * TW * 3 + TH * TW * 3 + (TW + TH) * 8 <= 64 * 1024 &&
              FOOT_LONG * TW * 3 + TH * TW * 3 + (TW + TH) * 8 + 64 <= 64 * 1024, "static LDS of a workgroup");

__device__ __forceinline__ int byte_of(int acc) {
    const int v = acc >> mrfa_resize::PRECISION_BITS;
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

template <int CIN, bool STAGE>
__global__ __launch_bounds__(NT) void resize_kernel(const unsigned char* __restrict__ src, int Hi, int Wi, const int* __restrict__ bounds_h,
                                                    const int* __restrict__ kk_h, int ksh, const int* __restrict__ bounds_v,
                                                    const int* __restrict__ kk_v, int ksv, int Ho, int Wo, float* __restrict__ out_f32,
                                                    unsigned char* __restrict__ out_u8, int vecf, int vecb) {
    constexpr int CH = CIN == 1 ? 1 : 3, FOOT = STAGE ? FOOT_STAGED : FOOT_LONG;
    __shared__ int s_kh[STAGE ? TW * LDS_TAPS : 1];
    __shared__ int s_kv[STAGE ? TH * LDS_TAPS : 1];
    __shared__ int s_bh[TW * 2];
    __shared__ int s_bv[TH * 2];
    __shared__ unsigned char s_rows[FOOT * TW * CH];
    __shared__ __attribute__((aligned(16))) unsigned char s_out[TH * TW * 3];

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, n = blockIdx.z;
    const int tw = min(TW, Wo - x0), th = min(TH, Ho - y0);
    kk_h += (size_t)x0 * ksh, kk_v += (size_t)y0 * ksv;          // the tile's rows
    if (STAGE) {
        for (int i = tid; i < tw * ksh; i += NT) s_kh[i] = kk_h[i];
        for (int i = tid; i < th * ksv; i += NT) s_kv[i] = kk_v[i];
    }
    if (tid < 2 * tw) s_bh[tid] = bounds_h[2 * x0 + tid];
    if (tid < 2 * th) s_bv[tid] = bounds_v[2 * y0 + tid];
    __syncthreads();

    const unsigned char* frame = src + (size_t)n * Hi * Wi * CIN;
    const int rowlen = tw * CH;                                  // bytes of a resampled row that this tile uses; rows of s_rows are rowlen apart
    for (int ya = 0; ya < th;) {                                 // (everything that steers this loop is uniform over the workgroup)
        int f0 = s_bv[2 * ya], f1 = f0 + s_bv[2 * ya + 1], yb = ya + 1;
        while (yb < th) {
            const int g0 = min(f0, s_bv[2 * yb]), g1 = max(f1, s_bv[2 * yb] + s_bv[2 * yb + 1]);
            if (g1 - g0 > FOOT) break;
            f0 = g0, f1 = g1, ++yb;
        }
        const int hitems = (f1 - f0) * rowlen;
        for (int i = tid; i < hitems; i += NT) {
            const int r = i / rowlen, j = i - r * rowlen;
            const int x = CH == 1 ? j : j / 3, c = j - x * CH;
            const int xmin = s_bh[2 * x], cnt = s_bh[2 * x + 1];
            const unsigned char* p = frame + ((size_t)(f0 + r) * Wi + xmin) * CIN + c;
            const int* k = (STAGE ? s_kh : kk_h) + x * ksh;
            int acc = ROUND;
            for (int t = 0; t < cnt; ++t) acc += (int)p[(size_t)t * CIN] * k[t];
            s_rows[i] = (unsigned char)byte_of(acc);             // (i == r * rowlen + j)
        }
        __syncthreads();
        const int vitems = (yb - ya) * rowlen;
        for (int i = tid; i < vitems; i += NT) {
            const int yy = i / rowlen, j = i - yy * rowlen, y = ya + yy;
            const int x = CH == 1 ? j : j / 3, c = j - x * CH;
            const int ymin = s_bv[2 * y], cnt = s_bv[2 * y + 1];
            const unsigned char* p = s_rows + (ymin - f0) * rowlen + j;
            const int* k = (STAGE ? s_kv : kk_v) + y * ksv;
            int acc = ROUND;
            for (int t = 0; t < cnt; ++t) acc += (int)p[t * rowlen] * k[t];
            const unsigned char b = (unsigned char)byte_of(acc);
            unsigned char* o = s_out + (y * TW + x) * 3;
            if (CH == 1)
                o[0] = o[1] = o[2] = b;
            else
                o[c] = b;
        }
        __syncthreads();
        ya = yb;
    }

    const size_t HWo = (size_t)Ho * Wo;
    if (out_f32) {
        float* dst = out_f32 + (size_t)n * 3 * HWo;
        if (vecf) {                                              // Wo % 4 == 0: tw is a multiple of 4 and every quad starts 16-byte aligned
            const int qw = tw >> 2, items = 3 * th * qw;
            for (int i = tid; i < items; i += NT) {
                const int c = i / (th * qw), rem = i - c * th * qw, y = rem / qw, q = rem - y * qw;
                const unsigned char* o = s_out + (y * TW + 4 * q) * 3 + c;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = __fmul_rn((float)o[3 * e], INV255);
                *reinterpret_cast<f32x4*>(dst + (size_t)c * HWo + (size_t)(y0 + y) * Wo + x0 + 4 * q) = v;
            }
        } else {
            const int items = 3 * th * tw;
            for (int i = tid; i < items; i += NT) {
                const int c = i / (th * tw), rem = i - c * th * tw, y = rem / tw, x = rem - y * tw;
                dst[(size_t)c * HWo + (size_t)(y0 + y) * Wo + x0 + x] = __fmul_rn((float)s_out[(y * TW + x) * 3 + c], INV255);
            }
        }
    }
    if (out_u8) {
        unsigned char* dst = out_u8 + ((size_t)n * HWo + (size_t)y0 * Wo + x0) * 3;
        if (vecb) {                                              // Wo % 4 == 0 and out_u8 4-byte aligned: a tile row is 3 tw / 4 whole, aligned dwords
            const int dw = (3 * tw) >> 2, items = th * dw;
            for (int i = tid; i < items; i += NT) {
                const int y = i / dw, d = i - y * dw;
                reinterpret_cast<unsigned*>(dst + (size_t)y * Wo * 3)[d] = reinterpret_cast<const unsigned*>(s_out + y * TW * 3)[d];
            }
        } else {
            const int rb = 3 * tw, items = th * rb;
            for (int i = tid; i < items; i += NT) {
                const int y = i / rb, j = i - y * rb;
                dst[(size_t)y * Wo * 3 + j] = s_out[y * TW * 3 + j];
            }
        }
    }
}

// what mrfa_resize_ksize and mrfa_resize_coeffs refuse alike; returns the taps, or -1 with the message set
int checked_ksize(const char* who, int in_size, float in0, float in1, int out_size, int filter) {
    MRFA_RESIZE_CHECK(in_size >= 1 && out_size >= 1, -1, "%s: in_size and out_size must be >= 1 (in_size %d, out_size %d)", who, in_size, out_size);
    MRFA_RESIZE_CHECK(mrfa_resize::filter_known(filter), -1, "%s: unknown filter %d (0 box, 1 bilinear, 2 hamming, 3 bicubic, 4 lanczos)", who, filter);
    MRFA_RESIZE_CHECK(mrfa_resize::box_ok(in_size, in0, in1), -1, "%s: the box [%.9g, %.9g] must lie in [0, %d] with in1 - in0 > 0", who, (double)in0,
                      (double)in1, in_size);
    const double ksize = mrfa_resize::axis_of(in0, in1, out_size, filter).ksize;
    MRFA_RESIZE_CHECK(ksize <= (double)MRFA_RESIZE_MAX_TAPS, -1, "%s: %.0f taps per output sample (in_size %d, box [%.9g, %.9g], out_size %d, filter %d), at most %d",
                      who, ksize, in_size, (double)in0, (double)in1, out_size, filter, MRFA_RESIZE_MAX_TAPS);
    return (int)ksize;
}

}  // namespace

extern "C" int mrfa_resize_version(void) { return MRFA_RESIZE_ABI_VERSION; }

extern "C" int mrfa_resize_ksize(int in_size, float in0, float in1, int out_size, int filter) {
    return checked_ksize("resize_ksize", in_size, in0, in1, out_size, filter);
}

extern "C" int mrfa_resize_coeffs(int in_size, float in0, float in1, int out_size, int filter, int* bounds, int* kk) {
    MRFA_RESIZE_CHECK(bounds && kk, 1, "resize_coeffs: null table (bounds %p, kk %p)", (void*)bounds, (void*)kk);
    const int ksize = checked_ksize("resize_coeffs", in_size, in0, in1, out_size, filter);
    if (ksize < 0) return 1;
    std::vector<double> w((size_t)ksize);
    mrfa_resize::coeffs(in_size, in0, in1, out_size, filter, ksize, bounds, kk, w.data());
    return 0;
}

extern "C" int mrfa_frames_resize_u8(void* stream, const unsigned char* src, int N, int Hi, int Wi, int Cin, const int* bounds_h, const int* kk_h, int ksize_h,
                                     const int* bounds_v, const int* kk_v, int ksize_v, int Ho, int Wo, float* out_f32, unsigned char* out_u8) {
    MRFA_RESIZE_CHECK(src && bounds_h && kk_h && bounds_v && kk_v, 1, "frames_resize_u8: null pointer (src %p, bounds_h %p, kk_h %p, bounds_v %p, kk_v %p)",
                      (const void*)src, (const void*)bounds_h, (const void*)kk_h, (const void*)bounds_v, (const void*)kk_v);
    MRFA_RESIZE_CHECK(out_f32 || out_u8, 1, "frames_resize_u8: out_f32 and out_u8 are both null");
    MRFA_RESIZE_CHECK(N >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1, 1, "frames_resize_u8: N, Hi, Wi, Ho and Wo must be >= 1 (N %d, Hi %d, Wi %d, Ho %d, Wo %d)",
                      N, Hi, Wi, Ho, Wo);
    const long long tiles_x = ((long long)Wo + TW - 1) / TW, tiles_y = ((long long)Ho + TH - 1) / TH;
    MRFA_RESIZE_CHECK(N <= 65535 && tiles_y <= 65535 && tiles_x <= 65535, 1, "frames_resize_u8: at most 65535 frames and 65535 tiles of %d x %d each way (N %d, Ho %d, Wo %d)",
                      TH, TW, N, Ho, Wo);
    MRFA_RESIZE_CHECK(Cin == 1 || Cin == 3 || Cin == 4, 1, "frames_resize_u8: Cin must be 1 (grey), 3 or 4 (the fourth byte is dropped), not %d", Cin);
    MRFA_RESIZE_CHECK(ksize_h >= 1 && ksize_h <= MRFA_RESIZE_MAX_TAPS && ksize_v >= 1 && ksize_v <= MRFA_RESIZE_MAX_TAPS, 1,
                      "frames_resize_u8: ksize_h %d and ksize_v %d must lie in [1, %d]", ksize_h, ksize_v, MRFA_RESIZE_MAX_TAPS);
    MRFA_RESIZE_CHECK((reinterpret_cast<uintptr_t>(out_f32) & 3u) == 0, 1, "frames_resize_u8: out_f32 %p must be 4-byte aligned (fp32 stores)", (void*)out_f32);
    const int vecf = out_f32 && Wo % 4 == 0 && aligned16(out_f32), vecb = out_u8 && Wo % 4 == 0 && (reinterpret_cast<uintptr_t>(out_u8) & 3u) == 0;
    const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)N);
    const hipStream_t st = (hipStream_t)stream;
    const bool stage = ksize_h <= LDS_TAPS && ksize_v <= LDS_TAPS;
#define MRFA_RESIZE_LAUNCH(CIN, STAGE)                                                                                                                    \
    hipLaunchKernelGGL((resize_kernel<CIN, STAGE>), grid, dim3(NT), 0, st, src, Hi, Wi, bounds_h, kk_h, ksize_h, bounds_v, kk_v, ksize_v, Ho, Wo, out_f32, \
                       out_u8, vecf, vecb)
    if (Cin == 1) {
        if (stage) MRFA_RESIZE_LAUNCH(1, true); else MRFA_RESIZE_LAUNCH(1, false);
    } else if (Cin == 3) {
        if (stage) MRFA_RESIZE_LAUNCH(3, true); else MRFA_RESIZE_LAUNCH(3, false);
    } else {
        if (stage) MRFA_RESIZE_LAUNCH(4, true); else MRFA_RESIZE_LAUNCH(4, false);
    }
#undef MRFA_RESIZE_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        mrfa_data_set_error("mrfa_frames_resize_u8: launch failed: %s", hipGetErrorString(e));
        return 2;
    }
    return 0;
}
