// Host side of the convolution dispatch: the tuning switches and the launch plans of mrfa_conv2d_nhwc / mrfa_conv2d_wgrad_nhwc.
//
// plan_conv / plan_wgrad decide, once per call, which kernel family runs a parameter block, with which geometry, and what the capability queries
// answer for it.  The dispatchers launch what the plan says and every query reads the same plan, so a query cannot drift from its launch.
#include "common.h"
#include <stdarg.h>

MrfaTuning g_tune = {
    /*conv_small*/ 1,
    /*conv_halo*/ 1, /*conv_halo_min_tiles*/ 128, /*conv_halo_pr*/ 0, /*conv_halo_phase*/ 1, /*conv_halo_bn256*/ 1,
    /*conv_halo_bn192*/ 1, /*conv_halo_bn64_fill*/ 1,
    /*conv_lean*/ 1, /*conv_lean_min_wgs*/ 128, /*conv_lean_geo*/ -1,
    /*gemm_lean*/ 1,      // 0 off, 1 where measured faster, 2 wherever it can run
    /*wgrad_halo*/ 1, /*wgrad_halo_min_wgs*/ 192, /*wgrad_halo_target_wgs*/ 256, /*wgrad_halo_phase*/ 1,
    /*wgrad_lean*/ 1,
    /*conv_fewout3*/ 1, /*attention_mfma*/ 1,
};

// how mrfa_set_tuning stores a value: on / off, as given, only when >= 0 (as given / as on-off / at most 2), only when > 0
enum TuneKind { T_ON, T_INT, T_NONNEG, T_NONNEG_ON, T_LEVEL, T_POS };
static const struct { const char* key; int* field; TuneKind kind; } TUNING_KEYS[] = {
    {"conv_small", &g_tune.conv_small, T_ON},
    {"conv_halo", &g_tune.conv_halo, T_ON},
    {"conv_halo_min_tiles", &g_tune.conv_halo_min_tiles, T_INT},
    {"conv_halo_pr", &g_tune.conv_halo_pr, T_INT},              // 0 = by workgroup count, 4 / 8 = forced patch height
    {"conv_halo_phase", &g_tune.conv_halo_phase, T_ON},
    {"conv_halo_bn256", &g_tune.conv_halo_bn256, T_ON},
    {"conv_halo_bn192", &g_tune.conv_halo_bn192, T_ON},
    {"conv_halo_bn64_fill", &g_tune.conv_halo_bn64_fill, T_ON},
    {"conv_lean", &g_tune.conv_lean, T_ON},
    {"conv_lean_min_wgs", &g_tune.conv_lean_min_wgs, T_NONNEG},
    {"conv_lean_geo", &g_tune.conv_lean_geo, T_INT},            // >= 0: only this geometry of conv_lean.hip (tests); -1: by workgroup count
    {"gemm_lean", &g_tune.gemm_lean, T_LEVEL},
    {"wgrad_halo", &g_tune.wgrad_halo, T_ON},
    {"wgrad_halo_min_wgs", &g_tune.wgrad_halo_min_wgs, T_NONNEG},
    {"wgrad_halo_target_wgs", &g_tune.wgrad_halo_target_wgs, T_POS},    // workgroups per round (one per CU)
    {"wgrad_halo_phase", &g_tune.wgrad_halo_phase, T_NONNEG_ON},        // weight gradient of fused-upsample layers in phase form
    {"wgrad_lean", &g_tune.wgrad_lean, T_ON},
    {"conv_fewout3", &g_tune.conv_fewout3, T_ON},
    {"attention_mfma", &g_tune.attention_mfma, T_ON},
};

extern "C" int mrfa_set_tuning(const char* key, int value) {
    if (!key) return -1;
    for (const auto& k : TUNING_KEYS) {
        if (strcmp(key, k.key)) continue;
        const int prev = *k.field;
        switch (k.kind) {
            case T_ON: *k.field = value != 0; break;
            case T_INT: *k.field = value; break;
            case T_NONNEG: if (value >= 0) *k.field = value; break;
            case T_NONNEG_ON: if (value >= 0) *k.field = value != 0; break;
            case T_LEVEL: if (value >= 0) *k.field = value > 2 ? 2 : value; break;
            case T_POS: if (value > 0) *k.field = value; break;
        }
        return prev;
    }
    return -1;
}

namespace {
constexpr int BK = 32;          // k-tile of the row-tiled kernels (conv_mfma.hip, conv_split.hip)

template <typename Plan>
Plan& refuse(Plan& c, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c.error, sizeof(c.error), fmt, ap);
    va_end(ap);
    c.family = decltype(c.family)::refused;
    return c;
}

// the row-tiled kernels (conv_mfma.hip fp32 tiles, conv_split.hip split-operand tile): tile, K split, variant
void plan_rows(ConvPlan& c, const mrfa_conv_params& p, int mode) {
    const bool flat = p.kflat > 0;
    const long long M = c.M;
    const int KT = c.KT;
    const int nb = p.nbatch > 1 ? p.nbatch : 1;
    // ---- tile selection: largest BN whose padding waste is small, then BM by how many workgroups result
    int BN = 128;
    {
        const int cands[4] = {128, 96, 64, 32};
        const double pen[4] = {1.0, 1.08, 1.16, 1.3};       // measured per-tile efficiency relative to 128x128
        double best = 1e18;
        for (int i = 0; i < 4; ++i) {
            if (cands[i] == 96 && flat) continue;
            const double cost = (double)cdiv(p.Cout, cands[i]) * cands[i] * pen[i];
            if (cost < best) { best = cost; BN = cands[i]; }
        }
    }
    // split-operand mode: the bf16x6 kernel only exists as a 128-wide tile and is ~1.5x faster than the fp32-MFMA tiles, which
    // outweighs the padding of 64 / 96 / 160 / 192-channel outputs to a multiple of 128
    if (mode >= 1 && !flat && p.Cout >= 32) BN = p.Cout <= 64 ? 64 : 128;
    auto ntiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * cdiv(p.Cout, bn) * nb; };
    // Few output tiles (low-resolution hourglass / generator levels): every M-tile re-reads the whole weight tensor, so
    // keep the tile tall and split K across workgroups first; shrink BM only when K is too short to split.
    int BM = 128;
    if (BN == 96 && ntiles(128, 96) < 384) BN = 128;     // few tiles: the 128-wide family has the 64/32-row variants
    if (BN == 128) { if (M <= 32) BM = 32; else if (M <= 64) BM = 64; }
    else if (BN == 64 && M <= 64) BM = 64;
    int splitk = 1;
    const bool auto_split = (p.splitk == 0);
    if (p.splitk > 1) splitk = p.splitk;
    {
        // Short K loop over many pixels (HRNet's 32..64-channel 3x3 convs at 64^2 / 32^2): a K split would add a zero-init and
        // a reduction/epilogue pass over the whole output (2 x 20 us measured) to a 20 us kernel -- keep one launch
        const bool short_k_big_m = KT < 32 && M > 4096;
        const bool grouped_stats = p.groups > 1 && p.stats && !(p.sk_ticket && !p.accumulate);       // (the split-K epilogue PASS does not keep statistic groups apart; the fused one does)
        const int max_split = (auto_split && !short_k_big_m && !grouped_stats) ? (KT / 2 > 0 ? KT / 2 : 1) : 1;
        long long t = ntiles(BM, BN);
        // (round 4, tools/sweep_splitk.py: with the split forced per launch the automatic choice is within 10 % of the best on six of eight low-resolution
        // shapes -- 128 -> 32 @64^2 fused upsample would prefer no split (74 -> 54 us), 256 -> 512 @8^2 a quarter of the slices (40 -> 30 us).  Lowering the
        // target here to catch those two moved OTHER layers onto the 64-row fp32 tiles through the BM loop below: +0.8 ms per step.  Left as it was.)
        if (t < 384 && !(short_k_big_m && t >= 128)) {
            // 512 workgroups -- or 256 for the deep-K launches that finish their split themselves (sk_ticket): their partial sums pass the memory-side atomic
            // units in one burst behind the k-loop (12 + 6 us of a 51 us launch, profiles/r6_splitk_launch_timeline.txt), and with the 128-row tile kept half the
            // slices are 5-6 us faster on 8 <= t <= 16 tiles (tools/sweep_splitk.py TILE128=1 COLD=1 FUSED=1: 1024 -> 1024 @4^2 52.3 -> 47.1, 512 -> 512 @8^2
            // 51.4 -> 46.7, 1024 -> 256 @8^2 up 53.0 -> 46.5, 256 -> 512 @8^2 42.8 -> 36.0)
            const bool half_target = auto_split && p.sk_ticket && !p.accumulate && KT >= 72 && KT <= 320 && BM == 128 && t >= 8 && t <= 16;      // (deeper K: 2048 -> 512 @8^2 up wants its 32 slices, 86 against 101 us)
            int want = (int)(((half_target ? 256 : 512) + t - 1) / t);
            if (auto_split) splitk = want <= max_split ? want : max_split;
            const int min_bm = (BN == 128) ? 32 : (BN == 64 ? 64 : 128);
            while (!half_target && ntiles(BM, BN) * splitk < 384 && BM > min_bm) {
                BM >>= 1;
                if (auto_split) {
                    t = ntiles(BM, BN);
                    want = (int)((512 + t - 1) / t);
                    splitk = want <= max_split ? want : max_split;
                }
            }
            if (splitk < 1) splitk = 1;
        }
    }
    bool w8 = false;                                         // 8-wave (512-thread) variant of the 128x128 tile
    if (p.tile) {
        BM = p.tile >> 16; BN = p.tile & 0x7fff; w8 = (p.tile & 0x8000) != 0;
        if (p.splitk >= 1) splitk = p.splitk;
    } else if (BM == 128 && BN == 128 && !flat) {
        w8 = true;                                           // 8 waves: 4 waves/SIMD hide the load/barrier phases (+4..13 %)
    }
    const bool split_operand = mode >= 1 && BM == 128 && (BN == 128 || BN == 64) && !flat;
    c.family = split_operand ? ConvFamily::rows_split : ConvFamily::rows_f32;
    c.BM = BM;
    c.BN = BN;
    c.w8 = w8;
    c.splitk = splitk;
    // v8: with sk_ticket the tile's last workgroup applies bias / affine / residual / ReLU / statistics (no epilogue pass)
    c.fused = splitk > 1 && p.sk_ticket && !p.accumulate;
    // the BatchNorm that follows (fin_*): finished by the launch's last workgroup, except behind a K split with an epilogue pass and in batched launches
    c.fin_in_launch = p.fin_scale && nb == 1 && (splitk == 1 || c.fused);
    // (the split-operand tile copies pre-split weight planes when it has them -- except in plain-bf16 mode, which rounds the fp32 layout itself)
    c.reads_w = !(split_operand && mode != 3 && p.w_split);
    c.last_config = (BM << 16) | (BN << 4) | ((flat ? 1 : 0) << 1) | (splitk > 1 ? 1 : 0) | (split_operand ? 4 : 0);     // bit 2: split-operand kernel
}
}  // namespace

ConvPlan plan_conv(const mrfa_conv_params& p) {
    ConvPlan c = {};
    const int mode = mrfa_get_mfma_mode();
    const bool flat = p.kflat > 0;
    c.M = (long long)p.N * p.Hout * p.Wout;
    c.KT = ((flat ? p.kflat : p.R * p.S * p.Cin) + BK - 1) / BK;
    c.splitk = 1;
    c.reads_w = true;
    c.fin_in_launch = p.fin_scale != nullptr;                // (the special kernels: finished by the launch's last workgroup)

    // which of the special kernels take the block, in the order the dispatch tries them
    c.lean_geo = flat ? -1 : mrfa_conv_lean_pick(p);
    c.gemm_cfg = (flat || c.lean_geo >= 0) ? -1 : mrfa_gemm_lean_pick(p, c.M);
    const bool lean = c.lean_geo >= 0, gemm = c.gemm_cfg >= 0;
    const bool small = !lean && !gemm && g_tune.conv_small && mrfa_conv_small_eligible(p, c.M);
    const bool halo = !flat && mrfa_conv_halo_eligible(p, &c.halo);

    // the capability queries (mrfa_hip.h)
    const long long rows = group_rows(p, c.M);
    // statistic groups: every kernel's output tile is at most 128 rows (and divides 128), the patch-tiled kernel's lies inside one image; a K split sums
    // its partial tiles in a pass whose workgroups stride over ALL rows, so grouped launches never split K (the automatic choice is switched off for them).
    // The lean kernels keep a patch inside one image / a workgroup's 64 rows inside one group, conv_small.hip its rows % 64; only conv_lean.hip has
    // prologue vectors per group.
    c.groups_ok = p.groups <= 1 || !(p.stats || p.fin_scale || p.bst_x || p.in_scale) ||
                  (p.nbatch <= 1 && p.splitk <= 1 && rows > 0 &&
                   (lean || gemm || (!p.in_scale && ((rows % 128) == 0 || small || (p.stride <= 1 && halo)))));
    c.bst_ok = p.stats && !p.fin_scale && p.stride >= 0 && !flat && (lean || gemm || small);
    c.stride2_ok = p.stride == 2 && p.Hout == (p.Hin + 2 * p.pad - p.R) / 2 + 1 && p.Wout == (p.Win + 2 * p.pad - p.S) / 2 + 1 &&
                   (flat ? (!p.ups && p.nbatch <= 1 && p.splitk <= 1 && p.ktab) : small);      // (flat K: the strided gather of the fp32 tile kernel)
    c.mask_ok = halo;
    c.phase_dgrad_ok = p.ups == 2 && halo;

    // the argument checks (null / misaligned views, sizes no kernel runs)
    if (!(p.x && p.w)) return refuse(c, "conv2d: null pointer");
    if (!(p.N > 0 && p.Cin > 0 && p.Cout > 0 && p.Hout > 0 && p.Wout > 0)) return refuse(c, "conv2d: bad sizes");
    if (!(p.R >= 1 && p.S >= 1 && p.R <= 15 && p.S <= 15)) return refuse(c, "conv2d: kernel size %dx%d unsupported", p.R, p.S);
    if (!((p.w_ld % 4) == 0 && aligned16(p.w))) return refuse(c, "conv2d: packed weight must be 16-B aligned, w_ld %% 4 == 0");
    if (!flat && (p.Cin % 32) != 0) return refuse(c, "conv2d: chunked mode needs Cin %% 32 == 0 (got %d); use flat mode", p.Cin);
    if (!flat && !((p.ldx % 4) == 0 && aligned16(p.x))) return refuse(c, "conv2d: chunked mode needs 16-B aligned x and ldx %% 4 == 0");
    if (!flat && p.in_scale && !(aligned16(p.in_scale) && aligned16(p.in_shift))) return refuse(c, "conv2d: in_scale/in_shift alignment");
    if (flat && !(p.ktab != nullptr && aligned16(p.ktab))) return refuse(c, "conv2d: flat mode needs a 16-B aligned ktab");
    // ---- the keypoint encoder's <= 128-channel 3x3 layers in a split-operand mode: four-wave patches on the bf16 pipe (conv_lean.hip)
    if (lean) {
        c.family = ConvFamily::lean;
        c.reads_w = false;
        c.last_config = (32 << 16) | (32 << 4) | 4 | (1 << 27);      // bit 27: conv_lean
        return c;
    }
    // ---- 1x1 convolutions / linears of the keypoint encoder in a split-operand mode: K-pipelined four-wave tiles on the bf16 pipe (conv_lean.hip)
    if (gemm) {
        c.family = ConvFamily::gemm_lean;
        c.reads_w = false;
        c.last_config = (64 << 16) | (64 << 4) | 4 | (1 << 26);      // bit 26: gemm_lean
        return c;
    }
    // ---- small problems (the MTIA prior's 0.1-0.6 GFLOP layers): one wave per output tile, no LDS / barrier / split-K (conv_small.hip)
    if (small) {
        c.family = ConvFamily::small;
        // wave tile: the largest of 32x32 / 16x32 / 16x16 that still yields >= ~2 000 waves (two per SIMD: measured best once the loads coalesce)
        const int ncols = (p.Cout + 15) / 16 * 16;
        auto waves = [&](int wm, int wn) { return ((c.M + wm - 1) / wm) * ((ncols + wn - 1) / wn); };
        int tm = 2, tn = 2;
        if (waves(32, 32) < 2048) { tm = 1; tn = 2; }
        if (tm == 1 && waves(16, 32) < 2048) { tn = 1; }
        if (ncols % 32 != 0 && tn == 2 && ncols < 32) tn = 1;
        if (p.groups > 1 && tm == 2 && (rows % 128) != 0) tm = 1;       // (eligibility guarantees % 64)
        c.small_tm = tm;
        c.small_tn = tn;
        c.last_config = (16 << 16) | (16 << 4) | 8;                    // bit 3: conv_small
        return c;
    }
    if (p.stride < 0 || p.stride > 2 || (p.stride == 2 && !(flat && !p.ups && p.nbatch <= 1)))
        return refuse(c, "conv2d: stride = %d is only implemented by the one-wave-per-tile kernel and by flat-K launches: ask mrfa_conv2d_stride_supported() first", p.stride);
    if (p.mask && !halo) return refuse(c, "conv2d: `mask` is only honoured by the patch-tiled kernel: ask mrfa_conv2d_mask_supported() first");
    if (p.ups == 2 && !halo)
        return refuse(c, "conv2d: ups = 2 (phase data gradient of a fused-upsample layer) is only implemented for the shapes mrfa_conv2d_phase_dgrad_supported() reports");
    // ---- 3x3 stride-1 layers with 32-aligned rows in split-operand mode: patch-tiled kernel, input halo split once per chunk (conv_halo.hip)
    if (halo) {
        c.family = p.ups == 2 ? ConvFamily::halo_dgrad : ConvFamily::halo;
        c.reads_w = false;
        c.last_config = (128 << 16) | ((p.Cout <= 64 ? 64 : 128) << 4) | 4 | (1 << 28);       // bit 28: conv_halo
        return c;
    }
    plan_rows(c, p, mode);
    return c;
}

WgradPlan plan_wgrad(const mrfa_wgrad_params& p) {
    WgradPlan c = {};
    const bool flat = p.kflat > 0;
    c.M = (long long)p.N * p.Hout * p.Wout;
    c.lean = mrfa_wgrad_lean_eligible(p);
    c.small = g_tune.conv_small && mrfa_wgrad_small_eligible(p, c.M);
    c.groups_ok = p.groups <= 1 || !p.in_scale || c.lean;
    c.stride2_ok = p.stride == 2 && p.Hout == (p.Hin + 2 * p.pad - p.R) / 2 + 1 && p.Wout == (p.Win + 2 * p.pad - p.S) / 2 + 1 && c.small;
    if (!(p.x && p.dy && p.dw)) return refuse(c, "wgrad: null pointer");
    if (!flat && !((p.ldx % 4) == 0 && aligned16(p.x))) return refuse(c, "wgrad: x must be a 16-B aligned view with ld %% 4 == 0");
    if (flat && !p.ktab) return refuse(c, "wgrad: flat mode needs ktab");
    if (!(c.M < (1ll << 31) - 64)) return refuse(c, "wgrad: too many pixels");
    // the keypoint encoder's <= 128-channel 3x3 layers WITH a prologue (a residual block's second convolution reading the raw output of its first): the
    // all-taps kernel of wgrad_lean.hip as a one-problem launch (without a prologue a lone problem stays on wgrad_small.hip: its 2 000 waves fill the chip)
    if (p.in_scale && c.lean) { c.family = WgradFamily::lean; return c; }
    if (!c.groups_ok) return refuse(c, "wgrad: groups = %d with a prologue is only implemented where mrfa_conv2d_wgrad_groups_supported() says so", p.groups);
    // small problems (the MTIA prior's layers): one wave per 32 x 32 weight block, no LDS staging, in-workgroup reduction (wgrad_small.hip)
    if (c.small) { c.family = WgradFamily::small; return c; }
    if (p.stride > 1) return refuse(c, "wgrad: stride = %d is only implemented by the small-problem kernel: ask mrfa_conv2d_wgrad_stride_supported() first", p.stride);
    // 3x3 stride-1 layers: all nine taps per staging (wgrad_halo.hip)
    c.family = !flat && mrfa_wgrad_halo_eligible(p) ? WgradFamily::halo : WgradFamily::tiled;
    return c;
}

// ---- the capability queries (mrfa_hip.h): each reads the plan of the block
extern "C" int mrfa_conv2d_split_k(const mrfa_conv_params* p) {
    if (!p) return 1;
    if (p->splitk > 1) return p->splitk;
    const ConvPlan c = plan_conv(*p);
    return c.family == ConvFamily::refused ? 1 : c.splitk;
}

// v9: does the kernel a call with these parameters would run read the fp32 weight layout `w` at all?  0: it reads the pre-split planes only (conv_halo.hip,
// conv_lean.hip, the row-tiled split-operand tile with w_split in the split modes) -- the caller may pass any non-NULL `w` and need not keep (or refresh, once
// per optimizer step) that layout: for the decoder's ~100 M parameters that is 8 of the 28 bytes per parameter the per-step re-packing moved.
extern "C" int mrfa_conv2d_reads_fp32_weights(const mrfa_conv_params* p) {
    if (!p) return 1;
    const ConvPlan c = plan_conv(*p);
    return c.family == ConvFamily::refused || c.reads_w ? 1 : 0;
}

extern "C" int mrfa_conv2d_groups_supported(const mrfa_conv_params* p) { return p && plan_conv(*p).groups_ok ? 1 : 0; }
extern "C" int mrfa_conv2d_bwdstats_supported(const mrfa_conv_params* p) { return p && plan_conv(*p).bst_ok ? 1 : 0; }
extern "C" int mrfa_conv2d_stride_supported(const mrfa_conv_params* p) { return p && plan_conv(*p).stride2_ok ? 1 : 0; }
extern "C" int mrfa_conv2d_mask_supported(const mrfa_conv_params* p) { return p && plan_conv(*p).mask_ok ? 1 : 0; }
extern "C" int mrfa_conv2d_phase_dgrad_supported(const mrfa_conv_params* p) { return p && plan_conv(*p).phase_dgrad_ok ? 1 : 0; }

extern "C" int mrfa_conv2d_wgrad_stride_supported(const mrfa_wgrad_params* p) { return p && plan_wgrad(*p).stride2_ok ? 1 : 0; }
extern "C" int mrfa_conv2d_wgrad_groups_supported(const mrfa_wgrad_params* p) { return p && plan_wgrad(*p).groups_ok ? 1 : 0; }
extern "C" int mrfa_conv2d_wgrad_lean_supported(const mrfa_wgrad_params* p) { return p && plan_wgrad(*p).lean ? 1 : 0; }
