// Batched weight (un)packing: every convolution's OIHW parameter -> all of its kernel layouts in ONE launch per <= 240
// convolutions (and the reverse for the weight gradients), instead of one small launch per (convolution, layout).
//
// The single-tensor kernels of layout.hip spend their time on 64-bit index divisions and 36-byte-strided reads
// (170 us for the 4.7 M-element 1024->512 3x3 weight = 0.2 TB/s) and cost 270 launches per training step.  Here a
// workgroup owns a (TCO output channels) x (32 input channels) x (all taps) tile of one convolution:
//   * OIHW side: each output channel's 32*T floats are contiguous: 16 bytes per lane where the segment length and the source
//     address allow it (4 bytes per lane otherwise),
//   * the tile is transposed through LDS (row stride odd: every store loop below reads it conflict free for odd T),
//   * kernel-layout side: a lane produces a whole 16-BYTE RUN along the layout's fastest axis and stores it at once:
//       - bf16 planes (modes 8 / 9 / 12 / 13 / 14 / 15): 8 consecutive K elements of one row = half of a chunk-major 32-byte run; the lane
//         splits them in registers (bf16_pieces) and writes one 16-byte store per piece.  Lanes are ordered (K half, row), so a wave
//         writes two contiguous 512-byte stretches of each piece (16 rows x 32 bytes of two K chunks),
//       - fp32 layouts (modes 0 - 3, 5, 7): 4 consecutive ci (modes 0, 1, 5) or co (2, 3, 7) as one float4 where the layout's
//         strides keep that aligned (always for 0 and 2, channel counts divisible by 4 for the others),
//     with a per-element tail path for the last channels of a tile and for destinations that are not 16-byte aligned.  The mode is
//     turned into axis roles and strides once per (descriptor, destination); the loops decode an item with shifts and masks only.
//     (The first version stored 4 bytes per lane -- 16 lanes = two 32-byte runs, the next 16 lanes in another tap's plane -- and
//     went through a switch and 64-bit multiplications per element.)
//   * phase layouts (modes 12 / 13): a lane reads the nine taps of its 8 (co, ci) pairs once and forms the phase-tap sums of one
//     phase row (8 of the 16) from registers, in the summation order of the first version (the sums are bit-identical).
// Padding elements of the destination layouts are never written: the host allocates those buffers zero-filled.
// The descriptor table travels BY VALUE in the kernel arguments (MRFA_PACK_MAX_DESCS = 240 descriptors: 16 KB -- gfx950 / ROCm 7 take kernel-argument
// segments of that size, also as hipGraph kernel nodes; through round 4 the table held 48 = 3 KB), so a launch is self-contained and can be recorded in a
// hipGraph without any host->device copy.
#include <stdint.h>
#include <type_traits>
#include "mfma_bf16.h"

namespace {

constexpr int TCI = 32;
constexpr int MAXD = MRFA_PACK_MAX_DESCS;
constexpr int LDS_FLOATS = 12832;              // 51.3 KB: 32 x (32*9 + 1), 16 x (32*25 + 1) or 8 x (32*49 + 1)

struct PackArgs {
    int n;
    int tile_prefix[MAXD + 1];                 // workgroup b handles desc d with tile_prefix[d] <= b < tile_prefix[d+1]
    mrfa_pack_desc d[MAXD];
};

__host__ __device__ inline int tco_for(int T) { return T <= 9 ? 32 : (T <= 25 ? 16 : 8); }           // a power of two
__host__ __device__ inline int rup(int a, int b) { return (a + b - 1) / b * b; }

// bf16 planes (modes 8 / 9 / 12 / 13 / 14 / 15) are K16-CHUNK-MAJOR: element (tap tt, row r, column f) of a [taps][rowsP][colsP] matrix sits at
// tt * rowsP * colsP + (f / 16) * (rowsP * 16) + r * 16 + f % 16: the 16-channel slab of a tap that a conv workgroup stages is ONE contiguous run
// of rows x 32 bytes (with row-major planes it was 32 bytes out of every row's Cin * 2: a quarter of each 128-byte line fetched from L2)
__device__ __forceinline__ long long chunk_major(int tt, int r, int f, int rowsP, int colsP) {
    return (long long)tt * rowsP * colsP + (long long)(f >> 4) * (rowsP * 16) + r * 16 + (f & 15);
}

__device__ __forceinline__ int find_desc(const int* prefix, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool aligned16p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// 8 consecutive elements along the fastest axis of one row (the first n of them inside the weight), idx % 8 == 0 -> the three pieces (RNE: the one
// rounded plane) as one 16-byte store each; element by element when the run is cut short by the weight's edge or the buffer is not 16-byte aligned
template <bool RNE>
__device__ __forceinline__ void store_run8(unsigned short* __restrict__ d16, long long piece, long long idx, const float (&v)[8], int n, bool vec) {
    constexpr int NPL = RNE ? 1 : 3;
    u32x4 p[3];
    bf16_pieces<RNE ? 1 : 6>(v, p[0], p[1], p[2]);
    if (vec && n >= 8) {
#pragma unroll
        for (int pc = 0; pc < NPL; ++pc) *reinterpret_cast<u32x4*>(d16 + pc * piece + idx) = p[pc];
    } else {
#pragma unroll
        for (int pc = 0; pc < NPL; ++pc)
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e < n) d16[pc * piece + idx + e] = (unsigned short)(p[pc][e >> 1] >> (16 * (e & 1)));
    }
}

// modes 8 / 9 / 14 / 15 of one tile.  CI_FAST: rows = co, K = ci (8, 14); else rows = ci, K = co, taps flipped (9, 15)
template <bool CI_FAST, bool RNE>
__device__ __forceinline__ void store_planes(const float* lds, unsigned short* __restrict__ d16, int T, int lt, int row, int co0, int ci0, int nco, int nci,
                                             int Cout, int Cin, bool vec) {
    const int rowsP = CI_FAST ? rup(Cout, 128) : rup(Cin, 128), colsP = CI_FAST ? rup(Cin, 32) : rup(Cout, 32);
    const long long piece = (long long)T * rowsP * colsP;
    if constexpr (CI_FAST) {
        // item = (g: 8-ci group, co_l, t), g fastest: a 32-lane half reads LDS banks 8 g (T odd) + co_l -- all different
        const int items = (4 << lt) * T;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int g = i & 3, co_l = (i >> 2) & ((1 << lt) - 1), t = i >> (2 + lt);
            const int n = nci - g * 8;
            if (co_l >= nco || n <= 0) continue;
            const float* wl = lds + co_l * row + g * 8 * T + t;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = wl[e * T];
            store_run8<RNE>(d16, piece, chunk_major(t, co0 + co_l, ci0 + g * 8, rowsP, colsP), v, n, vec);
        }
    } else {
        // item = (g: 8-co group, ci_l, t): banks 8 g + ci_l T
        const int lg = lt - 3;
        const int items = (32 << lg) * T;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int g = i & ((1 << lg) - 1), ci_l = (i >> lg) & 31, t = i >> (lg + 5);
            const int n = nco - g * 8;
            if (ci_l >= nci || n <= 0) continue;
            const float* wl = lds + g * 8 * row + ci_l * T + t;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = wl[e * row];
            store_run8<RNE>(d16, piece, chunk_major(T - 1 - t, ci0 + ci_l, co0 + g * 8, rowsP, colsP), v, n, vec);
        }
    }
}

// modes 12 / 13 (3x3 only: 32 x 32 tile, T = 9).  nearest-x2 upsample + 3x3 conv = four 2x2 "phase" convolutions on the low-resolution input
// (UpBlock2d, util.py:172-176): output pixel (2y + py, 2x + px) reads rows {y - 1 + py, y + py} x columns {x - 1 + px, x + px}; the weight of phase
// tap (a, b) is the sum of the 3x3 taps that land on that source pixel: rows R(py, a) = {0} {1,2} | {0,1} {2}, columns likewise.  Layout: three
// bf16 planes [piece][(py*2+px)*4 + a*2+b][CoutPad128][CinPad32] (mode 12: the split of mode 8 applied to the summed weights) or
// transposed [piece][..][CinPad128][CoutPad32] (mode 13: for the phase data gradient, the split of mode 9's role), each tap's matrix
// k16-chunk-major (chunk_major()).
// item = (g: 8-group along the fastest axis, slow index, py): the 256 threads take the tile's 256 items.  The tap rows of phase-tap row a are
// R(py, a) = rows r0, r0 + 1 (`two`) or r0 alone: a lane holds those <= 2 x 3 taps of its 8 (co, ci) pairs and forms the four (px, b) sums from them,
// rows outer, columns inner, as the element-by-element version did (a missing second row adds +0, which changes no sum)
template <bool TR>
__device__ __forceinline__ void store_phase(const float* lds, unsigned short* __restrict__ d16, int row, int co0, int ci0, int nco, int nci, int Cout, int Cin,
                                            bool vec) {
    const int rowsP = TR ? rup(Cin, 128) : rup(Cout, 128), colsP = TR ? rup(Cout, 32) : rup(Cin, 32);
    const long long piece = 16ll * rowsP * colsP;
    const int nfast = TR ? nco : nci, nslow = TR ? nci : nco;     // fastest destination axis: ci (12) / co (13)
    const int i = threadIdx.x;
    const int g = i & 3, sl = (i >> 2) & 31, py = i >> 7;
    const int n = nfast - g * 8;
    if (sl >= nslow || n <= 0) return;
    const float* wl = TR ? lds + g * 8 * row + sl * 9 : lds + sl * row + g * 8 * 9;
    const int estep = TR ? row : 9;
#pragma unroll
    for (int a_ = 0; a_ < 2; ++a_) {
        const int r0 = a_ ? 1 + py : 0;                           // R(0, .) = {0} {1, 2}; R(1, .) = {0, 1} {2}
        const bool two = (a_ == 0) == (py == 1);
        float wa[8][3], wb[8][3];
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int s_ = 0; s_ < 3; ++s_) {
                wa[e][s_] = wl[e * estep + r0 * 3 + s_];
                const float x = wl[e * estep + r0 * 3 + 3 + s_];  // (one row: the next pair's taps, inside the tile's LDS rows; not used)
                wb[e][s_] = two ? x : 0.f;
            }
#pragma unroll
        for (int px = 0; px < 2; ++px)
#pragma unroll
            for (int b_ = 0; b_ < 2; ++b_) {
                constexpr unsigned SM[4] = {0x1u, 0x6u, 0x3u, 0x4u};     // [px*2 + b] -> bit mask over s
                const unsigned sm = SM[px * 2 + b_];
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float s = 0.f;
#pragma unroll
                    for (int s_ = 0; s_ < 3; ++s_) if ((sm >> s_) & 1u) s += wa[e][s_];
#pragma unroll
                    for (int s_ = 0; s_ < 3; ++s_) if ((sm >> s_) & 1u) s += wb[e][s_];
                    v[e] = s;
                }
                const int pt = (py * 2 + px) * 4 + a_ * 2 + b_;
                const long long idx = TR ? chunk_major(pt, ci0 + sl, co0 + g * 8, rowsP, colsP) : chunk_major(pt, co0 + sl, ci0 + g * 8, rowsP, colsP);
                store_run8<false>(d16, piece, idx, v, n, vec);
            }
    }
}

// fp32 layouts: destination index of (co, ci, t) = base + co * sco + ci * sci + t * st (see mrfa_pack_conv_weight); the fastest axis has stride 1
struct F32Map { long long base, sco, sci, st; };
__device__ __forceinline__ F32Map f32_map(int mode, int Cout, int Cin, int T) {
    switch (mode) {
        case 0: return {0, rup(Cin, 32), 1, (long long)rup(Cout, 128) * rup(Cin, 32)};                                   // [t][CoP128][CiP32]
        case 1: return {0, rup(T * Cin, 32), 1, Cin};                                                                    // [CoP128][t * Cin + ci]
        case 2: { const long long m = (long long)rup(Cin, 128) * rup(Cout, 32); return {(T - 1) * m, 1, rup(Cout, 32), -m}; }   // [t'][CiP128][CoP32]
        case 3: return {(long long)(T - 1) * Cout, 1, rup(T * Cout, 32), -Cout};                                         // [CiP128][t' * Cout + co]
        case 5: return {0, (long long)T * Cin, 1, Cin};                                                                  // [co][t][ci]
        default: return {(long long)(T - 1) * Cout, 1, (long long)T * Cout, -Cout};                                      // 7: [ci][t'][co]
    }
}

template <bool CI_FAST>
__device__ __forceinline__ void store_f32(const float* lds, float* __restrict__ dst, const F32Map m, int T, int lt, int row, int co0, int ci0, int nco, int nci) {
    // float4 along the fastest axis when every other stride keeps the address 16-byte aligned (co0 and ci0 are multiples of 8)
    const bool vec = aligned16p(dst) && (((CI_FAST ? m.sco : m.sci) | m.st | m.base) & 3) == 0;
    if constexpr (CI_FAST) {
        // item = (g: 4-ci group, co_l, t): a 32-lane half reads banks 4 g T + co_l, all different for odd T
        const int items = (8 << lt) * T;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int g = i & 7, co_l = (i >> 3) & ((1 << lt) - 1), t = i >> (3 + lt);
            const int n = nci - g * 4;
            if (co_l >= nco || n <= 0) continue;
            const float* wl = lds + co_l * row + g * 4 * T + t;
            const f32x4 v = {wl[0], wl[T], wl[2 * T], wl[3 * T]};
            float* o = dst + m.base + (co0 + co_l) * m.sco + (ci0 + g * 4) + t * m.st;
            if (vec && n >= 4) *reinterpret_cast<f32x4*>(o) = v;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (e < n) o[e] = v[e];
            }
        }
    } else {
        // item = (g: 4-co group, ci_l, t): banks 4 g + ci_l T
        const int lg = lt - 2;
        const int items = (32 << lg) * T;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int g = i & ((1 << lg) - 1), ci_l = (i >> lg) & 31, t = i >> (lg + 5);
            const int n = nco - g * 4;
            if (ci_l >= nci || n <= 0) continue;
            const float* wl = lds + g * 4 * row + ci_l * T + t;
            const f32x4 v = {wl[0], wl[row], wl[2 * row], wl[3 * row]};
            float* o = dst + m.base + (co0 + g * 4) + (ci0 + ci_l) * m.sci + t * m.st;
            if (vec && n >= 4) *reinterpret_cast<f32x4*>(o) = v;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (e < n) o[e] = v[e];
            }
        }
    }
}

__global__ __launch_bounds__(256, 3) void pack_multi_kernel(const PackArgs a) {
    __shared__ float lds[LDS_FLOATS];
    const int di = find_desc(a.tile_prefix, a.n, blockIdx.x);
    const mrfa_pack_desc& d = a.d[di];
    const int T = d.R * d.S, Cout = d.Cout, Cin = d.Cin;
    const int TCO = tco_for(T), lt = TCO == 32 ? 5 : (TCO == 16 ? 4 : 3);
    const int tiles_ci = (Cin + TCI - 1) / TCI;
    const int tile = blockIdx.x - a.tile_prefix[di];
    const int co0 = (tile / tiles_ci) * TCO, ci0 = (tile % tiles_ci) * TCI;
    const int nco = min(TCO, Cout - co0), nci = min(TCI, Cin - ci0);
    const int row = TCI * T + 1;                                   // odd LDS row stride
    const int seg = nci * T;                                       // contiguous floats per output channel in OIHW
    // OIHW -> LDS [co_l][ci_l * T + t]; (co_l, position in the segment) walked incrementally
    const float* __restrict__ src = d.src;
    if ((seg & 3) == 0 && (((long long)Cin * T) & 3) == 0 && aligned16p(src)) {       // ci0 * T is a multiple of 32
        const int seg4 = seg >> 2;
        int co_l = threadIdx.x / seg4, r = threadIdx.x - co_l * seg4;
        while (co_l < nco) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + ((size_t)(co0 + co_l) * Cin + ci0) * T + 4 * r);
            float* l = lds + co_l * row + 4 * r;                   // (odd row stride: four 4-byte LDS stores)
            l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
            r += 256;
            while (r >= seg4) { r -= seg4; ++co_l; }
        }
    } else {
        int co_l = threadIdx.x / seg, r = threadIdx.x - co_l * seg;
        while (co_l < nco) {
            lds[co_l * row + r] = src[((size_t)(co0 + co_l) * Cin + ci0) * T + r];
            r += 256;
            while (r >= seg) { r -= seg; ++co_l; }
        }
    }
    __syncthreads();
    for (int k = 0; k < d.ndst; ++k) {
        const int mode = d.mode[k];
        float* __restrict__ dst = d.dst[k];
        unsigned short* __restrict__ d16 = reinterpret_cast<unsigned short*>(dst);
        const bool vec = aligned16p(dst);
        switch (mode) {                                            // once per (descriptor, destination)
            case 8: store_planes<true, false>(lds, d16, T, lt, row, co0, ci0, nco, nci, Cout, Cin, vec); break;
            case 9: store_planes<false, false>(lds, d16, T, lt, row, co0, ci0, nco, nci, Cout, Cin, vec); break;
            case 14: store_planes<true, true>(lds, d16, T, lt, row, co0, ci0, nco, nci, Cout, Cin, vec); break;    // ONE plane, round-to-nearest-even
            case 15: store_planes<false, true>(lds, d16, T, lt, row, co0, ci0, nco, nci, Cout, Cin, vec); break;
            case 12: store_phase<false>(lds, d16, row, co0, ci0, nco, nci, Cout, Cin, vec); break;
            case 13: store_phase<true>(lds, d16, row, co0, ci0, nco, nci, Cout, Cin, vec); break;
            case 0: case 1: case 5: store_f32<true>(lds, dst, f32_map(mode, Cout, Cin, T), T, lt, row, co0, ci0, nco, nci); break;
            default: store_f32<false>(lds, dst, f32_map(mode, Cout, Cin, T), T, lt, row, co0, ci0, nco, nci); break;   // 2, 3, 7
        }
    }
}

struct UnpackArgs {
    int n;
    int tile_prefix[MAXD + 1];
    mrfa_unpack_desc d[MAXD];
};

// dst (OIHW gradient) += src (accumulator in [tap][Cout][Cin], or [Cout][tap][Cin] when fewout)
__global__ __launch_bounds__(256) void unpack_multi_kernel(const UnpackArgs a) {
    __shared__ float lds[LDS_FLOATS];
    const int di = find_desc(a.tile_prefix, a.n, blockIdx.x);
    const mrfa_unpack_desc& d = a.d[di];
    const int T = d.T, Cout = d.Cout, Cin = d.Cin;
    const int TCO = tco_for(T), lt = TCO == 32 ? 5 : (TCO == 16 ? 4 : 3);
    const int tiles_ci = (Cin + TCI - 1) / TCI;
    const int tile = blockIdx.x - a.tile_prefix[di];
    const int co0 = (tile / tiles_ci) * TCO, ci0 = (tile % tiles_ci) * TCI;
    const int nco = min(TCO, Cout - co0), nci = min(TCI, Cin - ci0);
    const int row = TCI * T + 1;
    const int seg = nci * T;
    {   // ci fastest on the accumulator side: item = (g: 4-ci group, co_l, t) read as one float4 (Cin % 4 == 0: every row of the accumulator starts
        // 16-byte aligned), element by element otherwise; the LDS stores of a 32-lane half go to banks 4 g T + co_l: all different for odd T
        const float* __restrict__ src = d.src;
        const long long sco = d.fewout ? (long long)T * Cin : Cin, st = d.fewout ? Cin : (long long)Cout * Cin;
        const bool vec = (Cin & 3) == 0 && aligned16p(src);
        const int items = (8 << lt) * T;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int g = i & 7, co_l = (i >> 3) & ((1 << lt) - 1), t = i >> (3 + lt);
            const int n = nci - g * 4;
            if (co_l >= nco || n <= 0) continue;
            const float* s = src + (co0 + co_l) * sco + t * st + ci0 + g * 4;
            float* l = lds + co_l * row + g * 4 * T + t;
            if (vec && n >= 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(s);
                l[0] = v.x; l[T] = v.y; l[2 * T] = v.z; l[3 * T] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (e < n) l[e * T] = s[e];
            }
        }
    }
    __syncthreads();
    int co_l = threadIdx.x / seg, r = threadIdx.x - co_l * seg;
    while (co_l < nco) {
        // atomic: the two keypoint-encoder passes of a training step run their backward on two streams and accumulate into
        // the same weight.grad (mrfa_amd/train.py HotPath.encode_pair)
        atomicAdd(d.dst + ((size_t)(co0 + co_l) * Cin + ci0) * T + r, lds[co_l * row + r]);
        r += 256;
        while (r >= seg) { r -= seg; ++co_l; }
    }
}

template <typename Args, typename Desc, typename Kernel>
int launch_chunks(hipStream_t st, const Desc* descs, int n, Kernel kernel, const char* what) {
    for (int base = 0; base < n; base += MAXD) {
        Args a;
        a.n = min(MAXD, n - base);
        int tiles = 0;
        for (int i = 0; i < a.n; ++i) {
            const Desc& d = descs[base + i];
            a.d[i] = d;
            a.tile_prefix[i] = tiles;
            int T, Cout = d.Cout, Cin = d.Cin;
            if constexpr (std::is_same<Desc, mrfa_pack_desc>::value) T = d.R * d.S; else T = d.T;
            if (Cout <= 0 || Cin <= 0 || T <= 0 || tco_for(T) * (TCI * T + 1) > LDS_FLOATS) {
                mrfa_set_error("%s: desc %d: bad shape Cout=%d Cin=%d taps=%d", what, base + i, Cout, Cin, T);
                return 1;
            }
            tiles += cdiv(Cout, tco_for(T)) * cdiv(Cin, TCI);
        }
        a.tile_prefix[a.n] = tiles;
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(256), 0, st, a);
        MRFA_CHECK_LAUNCH(what);
    }
    return 0;
}

}  // namespace

extern "C" int mrfa_pack_conv_weights_multi(void* stream, const mrfa_pack_desc* descs, int n) {
    MRFA_CHECK_ARG(n >= 0 && (n == 0 || descs), "pack_conv_weights_multi: bad args");
    for (int i = 0; i < n; ++i) {
        MRFA_CHECK_ARG(descs[i].src && descs[i].ndst >= 1 && descs[i].ndst <= 3, "pack_conv_weights_multi: desc %d: null src or ndst %d", i,
                       descs[i].ndst);
        for (int k = 0; k < descs[i].ndst; ++k) {
            const int m = descs[i].mode[k];
            MRFA_CHECK_ARG(descs[i].dst[k] && (m == 0 || m == 1 || m == 2 || m == 3 || m == 5 || m == 7 || m == 8 || m == 9 || m == 14 || m == 15 || ((m == 12 || m == 13) && descs[i].R == 3 && descs[i].S == 3)),
                           "pack_conv_weights_multi: desc %d: null dst or mode %d", i, m);
        }
    }
    return launch_chunks<PackArgs>((hipStream_t)stream, descs, n, pack_multi_kernel, "pack_conv_weights_multi");
}

extern "C" int mrfa_unpack_wgrads_multi(void* stream, const mrfa_unpack_desc* descs, int n) {
    MRFA_CHECK_ARG(n >= 0 && (n == 0 || descs), "unpack_wgrads_multi: bad args");
    for (int i = 0; i < n; ++i) MRFA_CHECK_ARG(descs[i].src && descs[i].dst, "unpack_wgrads_multi: desc %d: null pointer", i);
    return launch_chunks<UnpackArgs>((hipStream_t)stream, descs, n, unpack_multi_kernel, "unpack_wgrads_multi");
}
