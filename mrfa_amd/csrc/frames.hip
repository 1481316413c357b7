// frames: the two ends of an inference loop as the reference's callers hold them -- uint8 H x W x C frames in (frames_dataset.py:29-65) and uint8
// H x W x 3 frames or a composed grid out (demo.py:72,160; reconstruction.py:63-76; logger.py:91-152) -- against the planar fp32 (N,3,H,W) in [0,1] that
// every entry of infer.py takes and returns.  Entries and their rules: include/mrfa_hip.h (that comment is the specification).  Inference only.
//
// Both kernels are pure data movement: one thread owns FOUR consecutive pixels of one row, which are 16 bytes in each fp32 plane and 4 Cin / 12 bytes on the
// byte side.  No LDS (nothing is read twice), no atomics, no scratch; every output byte has one writer: two runs are bit-identical.
//
// frames_from_u8_kernel<CIN, VEC>.  VEC (W % 4 == 0, src 4-byte and dst 16-byte aligned): quad q holds pixels 4q .. 4q + 3 of the flattened N H W pixels --
// never across a row, since W % 4 == 0 -- CIN dwords in (byte offset 4 q CIN), one float4 per plane out (plane offsets are multiples of 4 H W bytes).
// Otherwise one thread per pixel, byte loads and scalar stores: odd W, a single column, a source at an odd address.
//
// frames_to_u8_kernel.  blockIdx.y is the tile, whose descriptor is a launch argument (nothing on the device to keep alive: a captured launch replays);
// blockIdx.x strides over the tile's N x H x ceil(W / 4) quads.  Loads: a float4 per plane where the tile's W % 4 == 0 and its src is 16-byte aligned (a
// flag of the tile, uniform over the workgroup), four guarded scalars otherwise.  Stores: the quad's 12 bytes go out as three dwords where the quad is whole
// and its first byte, 3 ((n Hd + y0 + r) Wd + x0 + c), is 4-byte aligned -- with 3 Wd % 4 != 0 that changes from row to row, so it is decided per quad --
// and as single bytes otherwise (odd W, odd x0, the tail after whole quads).
//
// The per-element conversions are ONE fp32 multiply (__fmul_rn: never contracted, never turned into a division) and ONE convert / round.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "mrfa_hip.h"

namespace {

constexpr int NT = 256;
constexpr float INV255 = (float)(1.0 / 255.0);        // fl32(1 / 255): the reciprocal rounded once, in the compiler

__device__ __forceinline__ float unit_of_byte(unsigned v) { return __fmul_rn((float)v, INV255); }

template <int CIN>
struct QuadBytes { unsigned w[CIN]; };               // the 4 CIN bytes of four pixels

template <int CIN, bool VEC>
__global__ __launch_bounds__(NT) void frames_from_u8_kernel(const unsigned char* __restrict__ src, long long items, long long HW, float* __restrict__ dst) {
    const long long stride = (long long)gridDim.x * NT;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < items; i += stride) {
        if (VEC) {
            const QuadBytes<CIN> b = *reinterpret_cast<const QuadBytes<CIN>*>(src + (size_t)i * 4 * CIN);
            const long long p = i * 4, n = p / HW, o = p - n * HW;
            float* d = dst + (size_t)n * 3 * HW + o;
            f32x4 plane[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int byte = CIN == 1 ? j : j * CIN + c;           // grey: the one value in all three planes; CIN 4: byte 3 of a pixel is never used
                    plane[c][j] = unit_of_byte((b.w[byte >> 2] >> (8 * (byte & 3))) & 0xffu);
                }
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(d + (size_t)c * HW) = plane[c];
        } else {
            const long long n = i / HW, o = i - n * HW;
            const unsigned char* s = src + (size_t)i * CIN;
            float* d = dst + (size_t)n * 3 * HW + o;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[(size_t)c * HW] = unit_of_byte(s[CIN == 1 ? 0 : c]);
        }
    }
}

struct TileSet { mrfa_u8_tile t[MRFA_U8_MAX_TILES]; unsigned vec; };      // vec: bit t = tile t loads float4

// NaN -> 0, -inf and everything below 0 -> 0 (-0 included), +inf and everything above 255 -> 255
template <int ROUNDING>
__device__ __forceinline__ unsigned byte_of_unit(float s) {
    const float p = __fmul_rn(s, 255.0f);
    const float r = ROUNDING == 0 ? rintf(p) : truncf(p);                  // v_rndne_f32 (ties to even) / v_trunc_f32
    return r > 0.f ? (unsigned)(int)(r < 255.f ? r : 255.f) : 0u;
}

template <int ROUNDING>
__global__ __launch_bounds__(NT) void frames_to_u8_kernel(const TileSet ts, int N, int Hd, int Wd, unsigned char* __restrict__ dst) {
    const mrfa_u8_tile& t = ts.t[blockIdx.y];
    const bool vec = (ts.vec >> blockIdx.y) & 1u;
    const int H = t.H, W = t.W, QW = (W + 3) >> 2;
    const size_t HW = (size_t)H * W;
    const long long quads = (long long)N * H * QW, stride = (long long)gridDim.x * NT;
    const float r2 = __fmul_rn(t.radius, t.radius);
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < quads; i += stride) {
        const int q = (int)(i % QW);
        const long long row = i / QW;
        const int r = (int)(row % H), n = (int)(row / H);
        const int c0 = q * 4, cnt = W - c0 < 4 ? W - c0 : 4;
        const float* s = t.src + (size_t)n * 3 * HW + (size_t)r * W + c0;
        float v[3][4];
        if (vec) {                                                         // (W % 4 == 0: every quad is whole)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(s + c * HW);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[c][j] = x[j];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[c][j] = j < cnt ? s[c * HW + j] : 0.f;
        }
        unsigned b[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) b[j][c] = byte_of_unit<ROUNDING>(v[c][j]);
        if (t.kp) {                                                        // discs: the largest k that covers a pixel wins
            const float* kp = t.kp + (size_t)n * t.K * 2;
            int hit[4] = {-1, -1, -1, -1};
            for (int k = 0; k < t.K; ++k) {
                const float kx = kp[2 * k], ky = kp[2 * k + 1];
                if (!(isfinite(kx) && isfinite(ky))) continue;             // a non-finite keypoint draws nothing
                const float cx = __fmul_rn(__fmul_rn((float)W, __fadd_rn(kx, 1.f)), 0.5f), cy = __fmul_rn(__fmul_rn((float)H, __fadd_rn(ky, 1.f)), 0.5f);
                const float dy = __fsub_rn((float)r, cy), dy2 = __fmul_rn(dy, dy);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float dx = __fsub_rn((float)(c0 + j), cx);
                    if (__fadd_rn(dy2, __fmul_rn(dx, dx)) < r2) hit[j] = k;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (hit[j] >= 0) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) b[j][c] = byte_of_unit<ROUNDING>(t.colors[hit[j] * 3 + c]);
                }
        }
        if (t.border) {                                                    // after the discs: columns 0 and W - 1, no rows
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j == 0 || c0 + j == W - 1) b[j][0] = b[j][1] = b[j][2] = 255u;
        }
        unsigned char* d = dst + (((size_t)n * Hd + t.y0 + r) * Wd + t.x0 + c0) * 3;
        if (cnt == 4 && (reinterpret_cast<uintptr_t>(d) & 3u) == 0) {
            unsigned* d4 = reinterpret_cast<unsigned*>(d);
            d4[0] = b[0][0] | b[0][1] << 8 | b[0][2] << 16 | b[1][0] << 24;
            d4[1] = b[1][1] | b[1][2] << 8 | b[2][0] << 16 | b[2][1] << 24;
            d4[2] = b[2][2] | b[3][0] << 8 | b[3][1] << 16 | b[3][2] << 24;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[j * 3 + c] = (unsigned char)b[j][c];
                }
        }
    }
}

template <int CIN>
void launch_from_u8(hipStream_t st, bool vec, const unsigned char* src, long long pixels, long long HW, float* dst) {
    const long long items = vec ? pixels / 4 : pixels;
    const dim3 grid((unsigned)stream_grid(items, NT));
    if (vec)
        hipLaunchKernelGGL((frames_from_u8_kernel<CIN, true>), grid, dim3(NT), 0, st, src, items, HW, dst);
    else
        hipLaunchKernelGGL((frames_from_u8_kernel<CIN, false>), grid, dim3(NT), 0, st, src, items, HW, dst);
}

}  // namespace

extern "C" int mrfa_frames_from_u8(void* stream, const unsigned char* src, int N, int H, int W, int Cin, float* dst) {
    MRFA_CHECK_ARG(src && dst, "frames_from_u8: null pointer (src %p, dst %p)", (const void*)src, (void*)dst);
    MRFA_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "frames_from_u8: N, H and W must be >= 1 (N %d, H %d, W %d)", N, H, W);
    MRFA_CHECK_ARG(Cin == 1 || Cin == 3 || Cin == 4, "frames_from_u8: Cin must be 1 (grey), 3 or 4 (alpha is dropped), not %d", Cin);
    MRFA_CHECK_ARG((reinterpret_cast<uintptr_t>(dst) & 3u) == 0, "frames_from_u8: dst %p must be 4-byte aligned (fp32 stores)", (void*)dst);
    const long long HW = (long long)H * W, pixels = (long long)N * HW;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 3u) == 0 && aligned16(dst);
    const hipStream_t st = (hipStream_t)stream;
    if (Cin == 1)
        launch_from_u8<1>(st, vec, src, pixels, HW, dst);
    else if (Cin == 3)
        launch_from_u8<3>(st, vec, src, pixels, HW, dst);
    else
        launch_from_u8<4>(st, vec, src, pixels, HW, dst);
    MRFA_CHECK_LAUNCH("mrfa_frames_from_u8");
    return 0;
}

extern "C" int mrfa_frames_to_u8(void* stream, const mrfa_u8_tile* tiles, int n_tiles, int N, unsigned char* dst, int Hd, int Wd, int rounding) {
    MRFA_CHECK_ARG(tiles && dst, "frames_to_u8: null pointer (tiles %p, dst %p)", (const void*)tiles, (void*)dst);
    MRFA_CHECK_ARG(n_tiles >= 1 && n_tiles <= MRFA_U8_MAX_TILES, "frames_to_u8: 1 <= n_tiles <= %d (n_tiles %d)", MRFA_U8_MAX_TILES, n_tiles);
    MRFA_CHECK_ARG(N >= 1 && Hd >= 1 && Wd >= 1, "frames_to_u8: N, Hd and Wd must be >= 1 (N %d, Hd %d, Wd %d)", N, Hd, Wd);
    MRFA_CHECK_ARG(rounding == 0 || rounding == 1, "frames_to_u8: rounding must be 0 (nearest, ties to even) or 1 (floor), not %d", rounding);
    TileSet ts;
    memset(&ts, 0, sizeof ts);
    long long most = 0;
    for (int i = 0; i < n_tiles; ++i) {
        const mrfa_u8_tile& t = tiles[i];
        MRFA_CHECK_ARG(t.src, "frames_to_u8: tile %d has a null src", i);
        MRFA_CHECK_ARG((reinterpret_cast<uintptr_t>(t.src) & 3u) == 0, "frames_to_u8: tile %d: src %p must be 4-byte aligned", i, (const void*)t.src);
        MRFA_CHECK_ARG(t.H >= 1 && t.W >= 1, "frames_to_u8: tile %d: H and W must be >= 1 (H %d, W %d)", i, t.H, t.W);
        MRFA_CHECK_ARG(t.y0 >= 0 && t.x0 >= 0 && (long long)t.y0 + t.H <= Hd && (long long)t.x0 + t.W <= Wd,
                       "frames_to_u8: tile %d (%d x %d at y0 %d, x0 %d) lies outside dst (%d x %d)", i, t.H, t.W, t.y0, t.x0, Hd, Wd);
        if (t.kp) {
            MRFA_CHECK_ARG(t.colors, "frames_to_u8: tile %d has keypoints and colors == NULL", i);
            MRFA_CHECK_ARG(t.K >= 1 && t.K <= MRFA_U8_MAX_KP, "frames_to_u8: tile %d: 1 <= K <= %d (K %d)", i, MRFA_U8_MAX_KP, t.K);
            MRFA_CHECK_ARG(isfinite(t.radius) && t.radius > 0.f, "frames_to_u8: tile %d: the radius must be finite and > 0 (radius %g)", i, (double)t.radius);
            MRFA_CHECK_ARG(((reinterpret_cast<uintptr_t>(t.kp) | reinterpret_cast<uintptr_t>(t.colors)) & 3u) == 0,
                           "frames_to_u8: tile %d: kp %p and colors %p must be 4-byte aligned", i, (const void*)t.kp, (const void*)t.colors);
        }
        for (int j = 0; j < i; ++j) {
            const mrfa_u8_tile& u = tiles[j];
            MRFA_CHECK_ARG(t.y0 >= u.y0 + u.H || u.y0 >= t.y0 + t.H || t.x0 >= u.x0 + u.W || u.x0 >= t.x0 + t.W,
                           "frames_to_u8: tiles %d (%d x %d at y0 %d, x0 %d) and %d (%d x %d at y0 %d, x0 %d) overlap", j, u.H, u.W, u.y0, u.x0, i, t.H, t.W,
                           t.y0, t.x0);
        }
        ts.t[i] = t;
        if (t.W % 4 == 0 && aligned16(t.src)) ts.vec |= 1u << i;
        const long long quads = (long long)N * t.H * ((t.W + 3) / 4);
        most = quads > most ? quads : most;
    }
    const dim3 grid((unsigned)stream_grid(most, NT), (unsigned)n_tiles);
    if (rounding == 0)
        hipLaunchKernelGGL(frames_to_u8_kernel<0>, grid, dim3(NT), 0, (hipStream_t)stream, ts, N, Hd, Wd, dst);
    else
        hipLaunchKernelGGL(frames_to_u8_kernel<1>, grid, dim3(NT), 0, (hipStream_t)stream, ts, N, Hd, Wd, dst);
    MRFA_CHECK_LAUNCH("mrfa_frames_to_u8");
    return 0;
}
