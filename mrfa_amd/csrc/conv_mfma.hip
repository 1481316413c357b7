// Implicit-GEMM convolution / batched NT GEMM on the CDNA4 fp32 matrix pipe (v_mfma_f32_32x32x2_f32).
//
//   out[p, co] = alpha * sum_{r,s,ci} in'[pix(p)+(r,s)-pad, ci] * W[co, r, s, ci]   (+bias, affine, ReLU, residual)
//
// GEMM view: M = N*Hout*Wout output pixels, N = Cout, K = R*S*Cin.  NHWC activations make K (channels) the
// contiguous axis of both operands, so both tiles are staged in LDS as [row][k] (k contiguous, row stride 36
// floats = conflict-free for ds_read_b128) and every lane fetches FOUR consecutive k of its MFMA row with one
// ds_read_b128: lane l (row i = l&31, half h = l>>5) reads k = 8q+4h..8q+4h+3 and feeds them to four successive
// 32x32x2 MFMAs; A and B use the same k permutation, so the sum over k is complete and exact fp32 FMA chains.
//
// 256 threads = 4 wave64 per workgroup; block tile BM x BN (128x128 default: each wave owns a 64x64 sub-tile =
// 2x2 MFMA tiles = 64 accumulator VGPRs), BK = 32, register-staged double-buffered LDS, one barrier per k-tile.
// fp32 MFMA issues once per 64 cycles per SIMD and needs only 2 operand floats per lane per issue, so this kernel
// is bounded by the matrix pipe (157.3 TF/s peak), not by LDS or L2: per k-tile a workgroup moves 32 KiB from L2
// and spends 64 MFMAs x 64 cycles = 4096 cycles per wave on it (8 B/cycle/CU).
//
// Reference call sites replaced: every F.conv2d on the hot path (see include/mrfa_hip.h) and the all-pairs
// correlation einsum (modules/raft.py:185).
#include "common.h"
#include <stdlib.h>

namespace {

constexpr int BK = 32;
constexpr int LDK = BK + 4;   // 36 floats = 144 B row stride: 16-B slots (9*i + h) mod 16 are distinct per lane group

template <int BM, int BN, int WAVES_M, int WAVES_N, bool FLAT>
__global__ __launch_bounds__(WAVES_M * WAVES_N * 64) void conv_mfma_kernel(const mrfa_conv_params p, const int KT, const int kt_per_split,
                                                       const long long M, const int tiles_n, const int total_tiles) {
    constexpr int TM = BM / WAVES_M / 32;
    constexpr int TN = BN / WAVES_N / 32;
    constexpr int NT = WAVES_M * WAVES_N * 64;       // threads per workgroup (256 or 512)
    constexpr int RSTEP = NT / 8;                    // rows covered by one pass of the loader (8 float4 per 32-wide row)
    constexpr int RA = BM / RSTEP;                   // float4 global loads per thread per k-tile (A)
    constexpr int RB = BN / RSTEP;                   // (B)
    static_assert(WAVES_M * WAVES_N == 4 || WAVES_M * WAVES_N == 8, "4 or 8 waves");
    static_assert(RA >= 1 && RB >= 1, "tile too small for the workgroup");
    static_assert(TM >= 1 && TN >= 1, "tile");

    __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * LDK];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WAVES_N;
    const int wn = wave % WAVES_N;
    const int lin = xcd_tile_index();
    if (lin >= total_tiles) return;
    const int tile_m = lin / tiles_n;
    const int tile_n = lin - tile_m * tiles_n;
    const long long m0 = (long long)tile_m * BM;
    const int n0 = tile_n * BN;
    const int bz = blockIdx.y;

    const float* __restrict__ x = p.x + (size_t)bz * p.x_bs;
    const float* __restrict__ w = p.w + (size_t)bz * p.w_bs;
    float* __restrict__ y = p.y + (size_t)bz * p.y_bs;

    const int lrow = tid >> 3;   // 0..31
    const int kq = tid & 7;      // which float4 of the 32-wide k-tile
    const int Hv = p.Hin << p.ups, Wv = p.Win << p.ups;
    const int HWo = p.Hout * p.Wout;
    const int KC = FLAT ? 1 : (p.Cin >> 5);

    int a_oy[RA], a_ox[RA], a_base[RA];
    bool a_ok[RA];
#pragma unroll
    for (int j = 0; j < RA; ++j) {
        const long long m = m0 + lrow + RSTEP * j;
        a_ok[j] = m < M;
        const long long mm = a_ok[j] ? m : 0;
        const int n_img = (int)(mm / HWo);
        const int rem = (int)(mm - (long long)n_img * HWo);
        a_oy[j] = rem / p.Wout;
        a_ox[j] = rem - a_oy[j] * p.Wout;
        if (FLAT && p.stride == 2) { a_oy[j] *= 2; a_ox[j] *= 2; }       // strided gather (flat-K launches only: HRNet's 3 -> 64 stem, hr_base.py:302)
        a_base[j] = n_img * p.Hin * p.Win;
    }
    bool b_ok[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) b_ok[j] = (n0 + lrow + RSTEP * j) < p.w_rows;

    f32x4 ra[RA], rb[RB];

    // (tap, channel-chunk) of the NEXT k-tile to load, advanced incrementally: no integer divisions in the k-loop
    int l_r = 0, l_s = 0, l_c = 0;           // tap row / col, chunk index
    const float* l_w = w;                    // packed-weight pointer of the current tap
    const int a_koff = kq * 4;

    auto load_tiles = [&](int kt) {
        if constexpr (!FLAT) {
            const int c0 = l_c * 32 + a_koff;
            f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
            if (p.in_scale) {
                sc = *reinterpret_cast<const f32x4*>(p.in_scale + c0);
                sh = *reinterpret_cast<const f32x4*>(p.in_shift + c0);
            }
            const int dr = l_r - p.pad, ds = l_s - p.pad;
#pragma unroll
            for (int j = 0; j < RA; ++j) {
                const int iy = a_oy[j] + dr;
                const int ix = a_ox[j] + ds;
                const bool inb = a_ok[j] && (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv;
                // branch-free: out-of-bounds rows read a valid address (pixel 0 of their image) and are zeroed afterwards
                const int pix = inb ? (a_base[j] + (iy >> p.ups) * p.Win + (ix >> p.ups)) : a_base[j];
                f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)pix * p.ldx + c0);
                if (p.in_scale) {
                    v = v * sc + sh;
                    if (p.in_relu) {
                        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                    }
                }
                ra[j] = inb ? v : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const float* wt = l_w + c0;
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int row = b_ok[j] ? (n0 + lrow + RSTEP * j) : 0;
                const f32x4 v = *reinterpret_cast<const f32x4*>(wt + (size_t)row * p.w_ld);
                rb[j] = b_ok[j] ? v : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            // advance (chunk, s, r)
            if (++l_c == KC) {
                l_c = 0;
                l_w += p.w_tap;
                if (++l_s == p.S) { l_s = 0; ++l_r; }
            }
        } else {
            const int k0 = kt * 32 + kq * 4;
            const int4 ent = *reinterpret_cast<const int4*>(p.ktab + k0);
            const int e[4] = {ent.x, ent.y, ent.z, ent.w};
#pragma unroll
            for (int j = 0; j < RA; ++j) {
                float vv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v = 0.f;
                    if (e[q] >= 0 && a_ok[j]) {
                        const int dy = (e[q] & 255) - 128, dx = ((e[q] >> 8) & 255) - 128, ci = e[q] >> 16;
                        const int iy = a_oy[j] + dy, ix = a_ox[j] + dx;
                        if ((unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv) {
                            const size_t pix = (size_t)(a_base[j] + (iy >> p.ups) * p.Win + (ix >> p.ups));
                            v = x[pix * p.ldx + ci];
                            if (p.in_scale) {
                                v = v * p.in_scale[ci] + p.in_shift[ci];
                                if (p.in_relu) v = fmaxf(v, 0.f);
                            }
                        }
                    }
                    vv[q] = v;
                }
                ra[j] = f32x4{vv[0], vv[1], vv[2], vv[3]};
            }
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (b_ok[j]) v = *reinterpret_cast<const f32x4*>(w + (size_t)(n0 + lrow + RSTEP * j) * p.w_ld + k0);
                rb[j] = v;
            }
        }
    };

    auto store_tiles = [&](int buf) {
        float* As = smem + buf * (BM + BN) * LDK;
        float* Bs = As + BM * LDK;
#pragma unroll
        for (int j = 0; j < RA; ++j) *reinterpret_cast<f32x4*>(As + (lrow + RSTEP * j) * LDK + kq * 4) = ra[j];
#pragma unroll
        for (int j = 0; j < RB; ++j) *reinterpret_cast<f32x4*>(Bs + (lrow + RSTEP * j) * LDK + kq * 4) = rb[j];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int kt_begin = blockIdx.z * kt_per_split;
    const int kt_end = min(KT, kt_begin + kt_per_split);

    if constexpr (!FLAT) {
        const int tap0 = kt_begin / KC;
        l_c = kt_begin - tap0 * KC;
        l_r = tap0 / p.S;
        l_s = tap0 - l_r * p.S;
        l_w = w + (size_t)tap0 * p.w_tap;
    }
    if (kt_begin < kt_end) {
        load_tiles(kt_begin);
        store_tiles(0);
    }
    __syncthreads();

    const int frag_row = lane & 31;
    const int frag_k = (lane >> 5) * 4;
    int cur = 0;
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const bool more = (kt + 1) < kt_end;
        if (more) load_tiles(kt + 1);
        const float* As = smem + cur * (BM + BN) * LDK + (wm * TM * 32 + frag_row) * LDK + frag_k;
        const float* Bs = smem + cur * (BM + BN) * LDK + BM * LDK + (wn * TN * 32 + frag_row) * LDK + frag_k;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const f32x4*>(As + i * 32 * LDK + q * 8);
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * LDK + q * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
        }
        if (more) store_tiles(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // ------------------------------------------------------------------ epilogue
    const int half = lane >> 5;
    const bool splitk = p.splitk > 1;
    if (splitk) {
        // partial tile: device-scope atomics into y (zeros, or the bias written by the init pass)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int c = n0 + (wn * TN + j) * 32 + (lane & 31);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (c < p.Cout && m < M) atomicAdd(y + (size_t)m * p.ldy + c, acc[i][j][r] * p.alpha);
                }
        }
        // v8: the workgroup that completes the tile applies the epilogue itself (otherwise splitk_epilogue_kernel does, in a pass of its own)
        if (!p.sk_ticket || !splitk_last_arriver(p.sk_ticket + (size_t)bz * total_tiles + lin, gridDim.z)) return;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int c = n0 + (wn * TN + j) * 32 + (lane & 31);
        const bool c_ok = c < p.Cout;
        float bias = 0.f, osc = 1.f, osh = 0.f;
        if (c_ok) {
            if (p.bias) bias = p.bias[c];
            if (p.out_scale) { osc = p.out_scale[c]; osh = p.out_shift[c]; }
        }
        float s1 = 0.f, s2 = 0.f;
        // Everything a 32-row block of this column tile READS first, all of it in flight together, from clamped (always valid) addresses.  With the loads inside the
        // per-element branch the compiler waited for each one before the next was issued: the last arriver of a K split read its 64 values per lane
        // back one memory-side round trip at a time -- ~30 us of a 65 us launch on the low-resolution levels (round 6, the ISA of this loop:
        // global_load_dword ... sc1 ; s_waitcnt vmcnt(0), 64 times; tools/sweep_splitk.py FUSED=1 before / after in profiles/r6_sweep_splitk_*)
        const int cq = c_ok ? c : 0;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            float yv[16], rv[16];
            auto row_of = [&](int r) {                     // (rows past M read the last row: a valid address, never stored)
                const long long m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                return m < M ? m : M - 1;
            };
            if (splitk) {
#pragma unroll
                for (int r = 0; r < 16; ++r) yv[r] = __hip_atomic_load(y + (size_t)row_of(r) * p.ldy + cq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (p.accumulate) {
#pragma unroll
                for (int r = 0; r < 16; ++r) yv[r] = y[(size_t)row_of(r) * p.ldy + cq];
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) yv[r] = 0.f;
            }
            if (p.res) {
#pragma unroll
                for (int r = 0; r < 16; ++r) rv[r] = p.res[(size_t)row_of(r) * p.ldr + cq];
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) rv[r] = 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (c_ok && m < M) {
                    float* dst = y + (size_t)m * p.ldy + c;
                    float v = splitk ? yv[r] : acc[i][j][r] * p.alpha;
                    v += bias;
                    v = v * osc + osh;
                    v += rv[r];
                    if (p.relu) v = fmaxf(v, 0.f);
                    if (!splitk) v += yv[r];                // (accumulate; zeros otherwise)
                    *dst = v;
                    s1 += v;
                    s2 += v * v;
                }
            }
        }
        if (p.stats) {
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (half == 0 && c_ok) {
                double* st = stat_slot(p, stat_group(p, m0, M), blockIdx.x);       // (statistic groups: the launcher keeps a tile inside one group)
                atomicAdd(st + c, (double)s1);
                atomicAdd(st + p.Cout + c, (double)s2);
            }
        }
    }
    if (p.fin_scale) fused_bn_finalize(p, (unsigned)total_tiles);      // (without a split: every workgroup with a tile; with one: the tile's last arriver)
}

// y = bias (or 0) broadcast: initialises the output of a split-K launch
__global__ void splitk_init_kernel(float* y, int ldy, long long rows, int C, const float* bias) {
    const long long total = rows * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / C;
        const int c = (int)(i - r * C);
        y[(size_t)r * ldy + c] = bias ? bias[c] : 0.f;
    }
}

// second pass of a split-K launch: affine / residual / ReLU / BN statistics on the summed output
__global__ void splitk_epilogue_kernel(float* y, int ldy, long long rows, int C, const float* osc, const float* osh,
                                       const float* res, int ldr, int relu, double* stats) {
    // one thread per channel-column chunk; rows strided over blockIdx.y so statistics reduce per thread first
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float sc = osc ? osc[c] : 1.f, sh = osh ? osh[c] : 0.f;
    float s1 = 0.f, s2 = 0.f;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        float v = y[(size_t)r * ldy + c] * sc + sh;
        if (res) v += res[(size_t)r * ldr + c];
        if (relu) v = fmaxf(v, 0.f);
        y[(size_t)r * ldy + c] = v;
        s1 += v;
        s2 += v * v;
    }
    if (stats) {
        double* st = stats + (size_t)(blockIdx.y % MRFA_STATS_SLOTS) * 2 * C;
        atomicAdd(st + c, (double)s1);
        atomicAdd(st + C + c, (double)s2);
    }
}

template <int BM, int BN, int WM_, int WN_>
int launch_cfg(hipStream_t st, const mrfa_conv_params& p, int KT, long long M, int splitk) {
    const int tiles_n = cdiv(p.Cout, BN);
    const long long tiles_m = (M + BM - 1) / BM;
    const int total_tiles = (int)(tiles_m * tiles_n);
    dim3 grid((unsigned)(cdiv(total_tiles, 8) * 8), (unsigned)(p.nbatch > 1 ? p.nbatch : 1), (unsigned)splitk);
    const int kps = cdiv(KT, splitk);
    mrfa_conv_params q = p;
    q.splitk = splitk;
    if (p.kflat > 0)
        hipLaunchKernelGGL((conv_mfma_kernel<BM, BN, WM_, WN_, true>), grid, dim3(WM_ * WN_ * 64), 0, st, q, KT, kps, M, tiles_n, total_tiles);
    else
        hipLaunchKernelGGL((conv_mfma_kernel<BM, BN, WM_, WN_, false>), grid, dim3(WM_ * WN_ * 64), 0, st, q, KT, kps, M, tiles_n, total_tiles);
    MRFA_CHECK_LAUNCH("mrfa_conv2d_nhwc");
    return 0;
}

}  // namespace

// 0: v_mfma_f32_32x32x2_f32 everywhere; 1: eligible launches (chunked K, 128-row tile) run the bf16x6 split-operand kernel;
// 2: the same kernels keeping the three leading products only (bf16x3: 2^-16-class product error instead of 2^-24);
// 3: plain bf16 operands (round-to-nearest-even), one product: the arithmetic of a bf16 autocast (BASELINE config 4)
static int g_mfma_mode = 0;
extern "C" int mrfa_set_mfma_mode(int mode) {
    if (mode < 0 || mode > 3) { mrfa_set_error("set_mfma_mode: unknown mode %d", mode); return 1; }
    g_mfma_mode = mode;
    return 0;
}
extern "C" int mrfa_get_mfma_mode(void) { return g_mfma_mode; }

static thread_local int g_last_tile = 0;
// (BM << 16) | (BN << 4) | (flat << 1) | (splitk > 1) of the most recent mrfa_conv2d_nhwc launch on this thread
extern "C" int mrfa_conv2d_last_config(void) { return g_last_tile; }

// the row-tiled kernels: the split-K init pass, the tile, the split-K epilogue pass
static int launch_rows(hipStream_t st, const mrfa_conv_params& p, const ConvPlan& c) {
    const bool flat = p.kflat > 0;
    const long long M = c.M;
    const int nb = p.nbatch > 1 ? p.nbatch : 1;
    const int splitk = c.splitk;
    mrfa_conv_params pk = p;                                 // what the kernels see
    if (splitk > 1) {
        // with y_zero the output already holds zeros (no init pass: the bias then comes with the fused epilogue)
        const bool init = !p.accumulate && !(p.y_zero && (c.fused || !p.bias));
        if (init) {
            const long long rows = M * nb;
            MRFA_CHECK_ARG(nb == 1 || p.y_bs == (long long)M * p.ldy, "conv2d: split-K batched output must be dense");
            hipLaunchKernelGGL(splitk_init_kernel, dim3(stream_grid(rows * p.Cout, 256)), dim3(256), 0, st, p.y, p.ldy, rows,
                               p.Cout, p.bias);
            MRFA_CHECK_LAUNCH("splitk_init");
            pk.bias = nullptr;                               // (written by the init pass)
        }
        if (!c.fused) pk.sk_ticket = nullptr;
    }
    if (!c.fin_in_launch) pk.fin_scale = nullptr;
    g_last_tile = c.last_config;
    const int BM = c.BM, BN = c.BN;
    int rc = 1;
#define CFG(bm, bn, wm, wn) if (BM == bm && BN == bn) rc = launch_cfg<bm, bn, wm, wn>(st, pk, c.KT, M, splitk)
    if (c.family == ConvFamily::rows_split) rc = mrfa_conv_split_launch(st, pk, c.KT, M, splitk, BN);
    else if (c.w8 && BM == 128 && BN == 128) rc = launch_cfg<128, 128, 2, 4>(st, pk, c.KT, M, splitk);
    else CFG(128, 128, 2, 2);
    else CFG(128, 96, 4, 1);
    else CFG(128, 64, 2, 2);
    else CFG(128, 32, 4, 1);
    else CFG(64, 128, 2, 2);
    else CFG(64, 64, 2, 2);
    else CFG(32, 128, 1, 4);
    else { mrfa_set_error("conv2d: no tile config %dx%d", BM, BN); return 1; }
#undef CFG
    if (rc) return rc;
    if (splitk > 1 && !c.fused && (p.relu || p.stats || p.out_scale || p.res)) {
        MRFA_CHECK_ARG(!p.accumulate, "conv2d: split-K with accumulate cannot apply an epilogue");
        const long long rows = M * nb;
        dim3 grid(cdiv(p.Cout, 64), (unsigned)(rows < 256 ? rows : 256));
        hipLaunchKernelGGL(splitk_epilogue_kernel, grid, dim3(64), 0, st, p.y, p.ldy, rows, p.Cout, p.out_scale, p.out_shift,
                           p.res, p.ldr, p.relu, p.stats);
        MRFA_CHECK_LAUNCH("splitk_epilogue");
    }
    return 0;
}

extern "C" int mrfa_conv2d_nhwc(void* stream, const mrfa_conv_params* pp) {
    MRFA_CHECK_ARG(pp, "conv2d: null parameter block");
    const mrfa_conv_params& p = *pp;
    hipStream_t st = (hipStream_t)stream;
    const ConvPlan c = plan_conv(p);
    MRFA_CHECK_ARG(c.groups_ok, "conv2d: groups = %d is not implemented for these parameters (N = %d, %d x %d outputs, splitk %d): ask "
                   "mrfa_conv2d_groups_supported() first", p.groups, p.N, p.Hout, p.Wout, p.splitk);
    if (p.fin_scale) {
        MRFA_CHECK_ARG(p.stats && p.fin_shift && p.fin_gamma && p.fin_beta && p.fin_counter && p.fin_count > 0,
                       "conv2d: fin_scale needs stats, fin_shift, fin_gamma, fin_beta, fin_counter and fin_count > 0");
        MRFA_CHECK_ARG((p.fin_rmean == nullptr) == (p.fin_rvar == nullptr), "conv2d: fin_rmean / fin_rvar come together");
    }
    if (p.bst_x) {
        MRFA_CHECK_ARG(p.stats && p.bst_scale && p.bst_shift && p.bst_mean && p.bst_invstd && !p.fin_scale,
                       "conv2d: bst_x needs stats, bst_scale / _shift / _mean / _invstd and no fin_*");
        MRFA_CHECK_ARG(c.bst_ok, "conv2d: bst_* is only implemented by the small-problem kernels: ask mrfa_conv2d_bwdstats_supported() first");
    }
    MRFA_CHECK_ARG(p.y, "conv2d: null pointer");
    if (c.family == ConvFamily::refused) { mrfa_set_error("%s", c.error); return 1; }
    int rc;
    switch (c.family) {
        case ConvFamily::lean: g_last_tile = c.last_config; rc = mrfa_conv_lean_launch(st, p, c.lean_geo); break;
        case ConvFamily::gemm_lean: g_last_tile = c.last_config; rc = mrfa_gemm_lean_launch(st, p, c.M, c.gemm_cfg); break;
        case ConvFamily::small: g_last_tile = c.last_config; rc = mrfa_conv_small_launch(st, p, c.M, c.small_tm, c.small_tn); break;
        case ConvFamily::halo:
        case ConvFamily::halo_dgrad: g_last_tile = c.last_config; rc = mrfa_conv_halo_launch(st, p, c.halo); break;
        default: rc = launch_rows(st, p, c); break;
    }
    if (rc || !p.fin_scale || c.fin_in_launch) return rc;
    // every kernel but the one-wave-per-tile one: the finalize launch behind the convolution, inside the call
    return mrfa_bn_finalize_groups(stream, p.stats, p.fin_count, p.fin_gamma, p.fin_beta, p.fin_rmean, p.fin_rvar, p.fin_momentum, p.fin_eps,
                                   p.Cout, p.groups > 1 ? p.groups : 1, p.fin_scale, p.fin_shift, p.fin_mean, p.fin_invstd);
}
