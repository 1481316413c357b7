// frame_metrics: the full-reference metrics of a clip -- mean |p - t|, mean (p - t)^2 and SSIM of frame n of `pred` against frame n of `target` -- in one
// entry per group of frames, the rows kept on the device (reconstruction.py:52-70 prints L1 and PSNR per frame and declares an SSIM list it never fills).
// Entry: include/mrfa_hip.h.  Inference only.
//
// SSIM (Wang et al. 2004, data range 1): an 11-tap separable Gaussian window (sigma 1.5; the eleven fp32 numbers below ARE the definition), "valid"
// (no padding: (H - 10) x (W - 10) windows per channel), the five moments mu_x, mu_y, E[x^2], E[y^2], E[xy], no clamping of the variances,
//   S = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2)),  C1 = 0.01^2, C2 = 0.03^2,  ssim = mean of S over channels and windows.
// The second moments are taken on a = x - 0.5, b = y - 0.5 (the variances do not move with the shift, the means get the 0.5 back): images live in [0, 1],
// and E[a^2] - E[a]^2 cancels far fewer leading bits than E[x^2] - E[x]^2 does on a bright flat patch.
//
// frame_metrics_tile_kernel: one workgroup of 256 threads per (tile, channel, frame), tiles of TH x TW = 32 x 32 stepping over H x W.  A tile owns its
// TH x TW pixels (|d| and d^2, d = p - t on the numbers as loaded) and the windows whose top-left corner lies in it and is valid (y <= H - 11, x <= W - 11).
//   1. stage the (TH + 10) x (TW + 10) patch of a and b in LDS, guarded: a position outside the frame is never read and holds 0 (it only feeds windows
//      that are not valid and not summed);
//   2. horizontal pass: the five moments of every patch row at the TW window columns, into LDS;
//   3. vertical pass: a thread takes one column and four consecutive rows (fourteen LDS rows per moment instead of forty-four), forms S and sums the valid ones.
// LDS: 2 x 42 x 42 + 5 x 42 x 32 floats = 40 992 bytes (+ 48 for the reduction).  Lanes walk along a row in every pass: consecutive LDS words, no conflicts.
// Sums: a thread adds at most 7 staged pixels (4 values of S) in fp32, six shuffle steps add the lanes of a wave, one thread adds the four waves: no chain
// of fp32 additions is longer than 16.  The three partial sums of a workgroup go to the workspace as doubles.
// frame_metrics_finish_kernel, on the same stream, one wave per frame: adds the frame's partials in float64 in a fixed order (lane l takes partials l,
// l + 64, ...; then six shuffle steps), divides by the counts, rounds ONCE to fp32 and writes the row.  The kernel boundary is what publishes the partials:
// no ticket, no last-workgroup hand-off, no atomics.  Two runs on the same input are bit-identical.
#include <limits.h>

#include "common.h"
#include "mrfa_hip.h"

namespace {

constexpr int TH = MRFA_METRICS_TILE_H, TW = MRFA_METRICS_TILE_W;
constexpr int TAPS = 11, HALO = TAPS - 1;
constexpr int PH = TH + HALO, PW = TW + HALO;          // the staged patch
constexpr int NT = 256;
constexpr int ROWS_PER_THREAD = TH * TW / NT;          // vertical pass: 4 consecutive window rows of one column
static_assert(TW == 32 && TH * TW == NT * ROWS_PER_THREAD && TH % ROWS_PER_THREAD == 0, "the vertical pass maps a thread to (column tid % 32, rows 4 (tid / 32) ..)");

// g_i = exp(-(i - 5)^2 / 4.5) / sum, computed in float64 and rounded to fp32 (tests/test_clip_metrics_cpu.py compares these literals with the formula)
__device__ constexpr float GAUSS[TAPS] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
                                          0x1.b43c4p-3f,   0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
constexpr float SSIM_C1 = 1e-4f, SSIM_C2 = 9e-4f;         // 0.01^2 and 0.03^2, each rounded once

struct MetricsLds {
    float a[PH * PW], b[PH * PW];
    float h[5][PH * TW];                               // horizontal moments: a, b, a^2, b^2, a b
};

long long tiles_of(int H, int W) { return (long long)cdiv(H, TH) * cdiv(W, TW); }

// sums v over the workgroup in a fixed order; the total is valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <bool SSIM>
__global__ __launch_bounds__(NT) void frame_metrics_tile_kernel(const float* __restrict__ pred, const float* __restrict__ target, int C, int H, int W,
                                                                int tiles_x, int tiles, double* __restrict__ partial) {
    __shared__ MetricsLds L;
    __shared__ float red[3][4];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % tiles;
    const size_t plane = blockIdx.x / tiles;                               // n C + c
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const float* __restrict__ p = pred + plane * (size_t)H * W;
    const float* __restrict__ t = target + plane * (size_t)H * W;

    float s_abs = 0.f, s_sq = 0.f, s_ssim = 0.f;
    constexpr int SH = SSIM ? PH : TH, SW = SSIM ? PW : TW;                // without SSIM only the tile's own pixels are read
    for (int i = tid; i < SH * SW; i += NT) {
        const int py = i / SW, px = i % SW;
        const int y = y0 + py, x = x0 + px;
        float u = 0.5f, v = 0.5f;
        if (y < H && x < W) {                                              // (y0, x0 >= 0: nothing above or left of the frame)
            u = p[(size_t)y * W + x];
            v = t[(size_t)y * W + x];
            if (py < TH && px < TW) {
                const float d = u - v;
                s_abs += fabsf(d);
                s_sq += d * d;
            }
        }
        if (SSIM) {
            L.a[i] = u - 0.5f;
            L.b[i] = v - 0.5f;
        }
    }
    if (SSIM) {
        __syncthreads();
        for (int i = tid; i < PH * TW; i += NT) {
            const int r = i / TW, c = i % TW;
            float ma = 0.f, mb = 0.f, maa = 0.f, mbb = 0.f, mab = 0.f;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                const float av = L.a[r * PW + c + k], bv = L.b[r * PW + c + k];
                const float wa = GAUSS[k] * av, wb = GAUSS[k] * bv;
                ma += wa;
                mb += wb;
                maa += wa * av;
                mbb += wb * bv;
                mab += wa * bv;
            }
            L.h[0][i] = ma;
            L.h[1][i] = mb;
            L.h[2][i] = maa;
            L.h[3][i] = mbb;
            L.h[4][i] = mab;
        }
        __syncthreads();
        const int c = tid % TW, r0 = (tid / TW) * ROWS_PER_THREAD;
        float m[ROWS_PER_THREAD][5];
#pragma unroll
        for (int o = 0; o < ROWS_PER_THREAD; ++o)
#pragma unroll
            for (int q = 0; q < 5; ++q) m[o][q] = 0.f;
#pragma unroll
        for (int r = 0; r < ROWS_PER_THREAD + HALO; ++r) {
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const float hv = L.h[q][(r0 + r) * TW + c];
#pragma unroll
                for (int o = 0; o < ROWS_PER_THREAD; ++o)
                    if (r - o >= 0 && r - o < TAPS) m[o][q] += GAUSS[r - o] * hv;          // (resolved at compile time: every loop is unrolled)
            }
        }
        const bool col_ok = x0 + c <= W - TAPS;
#pragma unroll
        for (int o = 0; o < ROWS_PER_THREAD; ++o) {
            const float ma = m[o][0], mb = m[o][1];
            const float mux = ma + 0.5f, muy = mb + 0.5f;
            const float sxx = m[o][2] - ma * ma, syy = m[o][3] - mb * mb, sxy = m[o][4] - ma * mb;
            const float num = (2.f * mux * muy + SSIM_C1) * (2.f * sxy + SSIM_C2);
            const float den = (mux * mux + muy * muy + SSIM_C1) * (sxx + syy + SSIM_C2);
            const float S = num / den;
            if (col_ok && y0 + r0 + o <= H - TAPS) s_ssim += S;
        }
    }
    const float t_abs = block_sum(s_abs, red[0]), t_sq = block_sum(s_sq, red[1]), t_ssim = SSIM ? block_sum(s_ssim, red[2]) : 0.f;
    if (tid == 0) {
        double* out = partial + (size_t)blockIdx.x * 3;
        out[0] = (double)t_abs;
        out[1] = (double)t_sq;
        out[2] = (double)t_ssim;
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64) void frame_metrics_finish_kernel(const double* __restrict__ partial, int per_frame, double pixels, double windows,
                                                                  int want_ssim, float* __restrict__ out) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const double* f = partial + (size_t)n * per_frame * 3;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = lane; j < per_frame; j += 64) {
        s0 += f[(size_t)j * 3];
        s1 += f[(size_t)j * 3 + 1];
        s2 += f[(size_t)j * 3 + 2];
    }
    s0 = wave_sum_f64(s0);
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    if (lane == 0) {
        float* row = out + (size_t)n * 4;
        row[0] = (float)(s0 / pixels);
        row[1] = (float)(s1 / pixels);
        row[2] = want_ssim ? (float)(s2 / windows) : 0.f;
        row[3] = 0.f;
    }
}

}  // namespace

extern "C" long long mrfa_frame_metrics_workspace(int N, int C, int H, int W) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return -1;
    const long long wgs = (long long)N * C * tiles_of(H, W);
    if (wgs > INT_MAX) return -1;                                          // one workgroup each, a one-dimensional grid
    return wgs * 3 * (long long)sizeof(double);
}

extern "C" int mrfa_frame_metrics(void* stream, const float* pred, const float* target, int N, int C, int H, int W, int want_ssim, void* workspace,
                                  long long workspace_bytes, float* out) {
    MRFA_CHECK_ARG(pred && target && workspace && out, "frame_metrics: null pointer (pred %p, target %p, workspace %p, out %p)", (const void*)pred,
                   (const void*)target, workspace, (void*)out);
    MRFA_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "frame_metrics: N, C, H and W must be >= 1 (N %d, C %d, H %d, W %d)", N, C, H, W);
    const long long need = mrfa_frame_metrics_workspace(N, C, H, W);
    MRFA_CHECK_ARG(need > 0, "frame_metrics: N C tiles(H, W) = %lld x %lld workgroups exceed one grid (N %d, C %d, H %d, W %d)", (long long)N * C,
                   tiles_of(H, W), N, C, H, W);
    MRFA_CHECK_ARG(workspace_bytes >= need, "frame_metrics: the workspace holds %lld bytes, mrfa_frame_metrics_workspace(%d, %d, %d, %d) asks for %lld",
                   workspace_bytes, N, C, H, W, need);
    MRFA_CHECK_ARG(!want_ssim || (H >= TAPS && W >= TAPS), "frame_metrics: SSIM needs one %d x %d window, min(H, W) >= %d (H %d, W %d)", TAPS, TAPS, TAPS, H, W);
    const uintptr_t a4 = (uintptr_t)pred | (uintptr_t)target | (uintptr_t)out;
    MRFA_CHECK_ARG((a4 & 3u) == 0 && ((uintptr_t)workspace & 7u) == 0,
                   "frame_metrics: pred, target and out must be 4-byte aligned (scalar fp32 accesses), the workspace 8-byte aligned (doubles)");
    const int tiles_x = cdiv(W, TW), tiles = (int)tiles_of(H, W);
    const int per_frame = C * tiles;
    const dim3 grid((unsigned)((long long)N * per_frame));
    if (want_ssim)
        hipLaunchKernelGGL(frame_metrics_tile_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, pred, target, C, H, W, tiles_x, tiles, (double*)workspace);
    else
        hipLaunchKernelGGL(frame_metrics_tile_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, pred, target, C, H, W, tiles_x, tiles, (double*)workspace);
    MRFA_CHECK_LAUNCH("mrfa_frame_metrics (tiles)");
    const double pixels = (double)C * H * W, windows = want_ssim ? (double)C * (H - HALO) * (W - HALO) : 1.0;
    hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, per_frame, pixels, windows, want_ssim,
                       out);
    MRFA_CHECK_LAUNCH("mrfa_frame_metrics (finish)");
    return 0;
}
