"""Records the answers of the convolution capability queries of libmrfa_hip.so into tests/golden/conv_plan_table.npz.

Every row is one parameter block (mrfa_conv_params or mrfa_wgrad_params) under one matrix mode and one tuning switch, with the answers of
mrfa_conv2d_{split_k, reads_fp32_weights, groups_supported, bwdstats_supported, stride_supported, mask_supported, phase_dgrad_supported} or of
mrfa_conv2d_wgrad_{stride, groups, lean}_supported.  The queries never dereference the pointers of the block, so no GPU is needed: each pointer is
stored as its offset from a 4 KiB-aligned base (-1: NULL), and tests/test_conv_plan.py rebuilds the same blocks from the stored fields alone.

    python tools/conv_plan_table.py [--lib path/to/libmrfa_hip.so] [--out tests/golden/conv_plan_table.npz]"""
import argparse
import ctypes as C
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mrfa_amd.hip import ConvParams, WgradParams, tuned  # noqa: E402

# tuning switches of the table: (key, value) applied with mrfa_set_tuning on top of the defaults; None = defaults
TUNINGS = [None, ("conv_small", 0), ("conv_halo", 0), ("conv_lean", 0), ("wgrad_halo", 0), ("wgrad_lean", 0), ("gemm_lean", 2)]
CONV_QUERIES = ["split_k", "reads_fp32_weights", "groups_supported", "bwdstats_supported", "stride_supported", "mask_supported",
                "phase_dgrad_supported"]
WGRAD_QUERIES = ["wgrad_stride_supported", "wgrad_groups_supported", "wgrad_lean_supported"]
BASE = 1 << 32                     # pointer field i of a block sits at BASE + i * 4 KiB + its stored offset


def pointer_fields(struct):
    return [n for n, t in struct._fields_ if t is C.c_void_p]


def value_fields(struct):
    return [n for n, t in struct._fields_ if t is not C.c_void_p]


def make_block(struct, ptr_names, ptrs, val_names, vals):
    """the parameter block of one table row: pointers as offsets from their base (-1 = NULL), then the other fields"""
    p = struct()
    all_ptrs = pointer_fields(struct)
    for n, v in zip(ptr_names, ptrs):
        setattr(p, n, None if v < 0 else BASE + all_ptrs.index(n) * 4096 + int(v))
    for n, v in zip(val_names, vals):
        setattr(p, n, float(v) if n in ("alpha", "fin_momentum", "fin_eps") else int(v))
    return p


def open_lib(path):
    L = C.CDLL(path)
    for q in CONV_QUERIES:
        getattr(L, "mrfa_conv2d_" + q).argtypes = [C.POINTER(ConvParams)]
    for q in WGRAD_QUERIES:
        getattr(L, "mrfa_conv2d_" + q).argtypes = [C.POINTER(WgradParams)]
    L.mrfa_set_tuning.argtypes = [C.c_char_p, C.c_int]
    return L


def answer(L, mode, tuning, struct, queries, ptr_names, ptrs, val_names, vals):
    """the answers of `queries` for every row, under matrix mode `mode` and the tuning switch `tuning`"""
    assert L.mrfa_set_mfma_mode(mode) == 0
    with tuned(L, **dict([tuning] if tuning else [])):
        out = np.zeros((len(vals), len(queries)), np.int16)
        for i in range(len(vals)):
            p = make_block(struct, ptr_names, ptrs[i], val_names, vals[i])
            for j, q in enumerate(queries):
                out[i, j] = getattr(L, "mrfa_conv2d_" + q)(C.byref(p))
        return out


CH = [16, 32, 48, 64, 96, 128, 160, 192, 256, 320, 512, 576, 640, 1024]
SP = [4, 8, 16, 24, 32, 64, 128, 256]


def conv_block(rng):
    d = {}
    R = rng.choice([1, 3, 3, 3, 7])
    S = R if rng.random() < 0.9 else rng.choice([1, 3, 7])
    pad = R // 2 if rng.random() < 0.85 else rng.choice([0, 1])
    stride = rng.choice([0, 0, 1, 1, 2])
    ups = rng.choice([0, 0, 0, 1, 2]) if stride != 2 else rng.choice([0, 0, 0, 1])
    Cin, Cout = rng.choice(CH), rng.choice(CH if rng.random() < 0.95 else [1, 2, 3, 8])
    Ho = rng.choice(SP)
    Wo = Ho if rng.random() < 0.8 else rng.choice(SP + [33, 48])
    N = rng.choice([1, 2, 4, 8, 16])
    if ups == 1:
        Hi, Wi = max(Ho // 2, 1), max(Wo // 2, 1)
    elif ups == 2 or stride == 2:
        Hi, Wi = 2 * Ho, 2 * Wo
    else:
        Hi, Wi = Ho, Wo
    if rng.random() < 0.05:
        Hi += 1
    flat = rng.random() < 0.15
    T = R * S
    d.update(N=N, Cin=Cin, Cout=Cout, Hin=Hi, Win=Wi, Hout=Ho, Wout=Wo, R=R, S=S, pad=pad, stride=stride, ups=ups)
    d["ldx"] = Cin if rng.random() < 0.8 else Cin + rng.choice([2, 4, 32])
    d["ldy"] = Cout if rng.random() < 0.8 else Cout + rng.choice([1, 2, 4])
    cop = (Cout + 127) // 128 * 128
    d["w_ld"] = ((T * Cin + 31) // 32 * 32 if flat else Cin) + (2 if rng.random() < 0.05 else 0)
    d["w_tap"], d["w_rows"] = cop * Cin, cop
    d["alpha"] = 1
    d["nbatch"] = rng.choice([0] * 8 + [1, 2])
    if d["nbatch"] > 1:
        d["x_bs"], d["w_bs"], d["y_bs"] = Hi * Wi * d["ldx"], 0, N * Ho * Wo * d["ldy"] * rng.choice([1, 1, 2]) if N * Ho * Wo * d["ldy"] < 2 ** 29 else 1
    d["splitk"] = rng.choice([0] * 6 + [1, 2, 4])
    d["groups"] = rng.choice([0, 0, 1, 2, 2, 4])
    d["accumulate"] = int(rng.random() < 0.1)
    d["y_zero"] = int(rng.random() < 0.1)
    d["relu"] = int(rng.random() < 0.3)
    if flat:
        d["kflat"] = T * Cin
        d["ktab"] = 0 if rng.random() < 0.95 else -1
    if rng.random() < 0.1:
        d["tile"] = rng.choice([(128 << 16) | 128, (128 << 16) | 128 | 0x8000, (128 << 16) | 64, (64 << 16) | 64, (32 << 16) | 128,
                                (128 << 16) | 96])

    def al():                                      # pointer alignment offset: mostly 16-byte aligned
        return 0 if rng.random() < 0.93 else rng.choice([4, 8])
    d["x"], d["w"], d["y"] = al(), al(), al()
    if rng.random() < 0.02:
        d[rng.choice(["x", "w", "y"])] = -1
    if rng.random() < 0.6:
        d["w_split"], d["w_piece"] = al(), (0 if rng.random() < 0.1 else T * cop * Cin)
    if ups and rng.random() < 0.6:
        d["w_phase"], d["w_phase_piece"] = al(), (4 * cop * Cin if rng.random() < 0.97 else 1 << 30)
    if rng.random() < 0.3:
        d["bias"] = al()
    if rng.random() < 0.15:
        d["out_scale"], d["out_shift"] = al(), al()
    if rng.random() < 0.15:
        d["res"], d["ldr"] = al(), Cout + (0 if rng.random() < 0.9 else 2)
    if rng.random() < 0.2:
        d["in_scale"], d["in_shift"], d["in_relu"] = al(), al(), int(rng.random() < 0.8)
    if rng.random() < 0.1:
        d["mask"], d["ldm"] = al(), 1
    if rng.random() < 0.4:
        d["stats"] = al()
        if rng.random() < 0.4:
            for k in ("fin_gamma", "fin_beta", "fin_scale", "fin_shift", "fin_counter"):
                d[k] = al()
            d["fin_count"] = N * Ho * Wo
            if rng.random() < 0.5:
                d["fin_rmean"], d["fin_rvar"] = al(), al()
            if rng.random() < 0.5:
                d["fin_mean"], d["fin_invstd"] = al(), al()
        elif rng.random() < 0.4:
            for k in ("bst_x", "bst_scale", "bst_shift", "bst_mean", "bst_invstd"):
                d[k] = al()
            d["bst_ldx"], d["bst_relu"] = Cin + (0 if rng.random() < 0.9 else 2), int(rng.random() < 0.5)
    if rng.random() < 0.15:
        d["sk_ticket"] = 0
    if rng.random() < 0.5:
        clean(rng, d)
    return d


def clean(rng, d):
    """half of the conv blocks: the shapes the special kernels take -- dense aligned views, pre-split weights, no forced tile / split / batch"""
    kind = rng.choice(["lean", "gemm", "halo", "phase", "small"])
    for k in ("kflat", "tile", "splitk", "nbatch", "ktab", "mask", "x_bs", "y_bs", "w_bs"):
        d.pop(k, None)
    d.update(x=0, w=0, y=0, stride=rng.choice([0, 1]), ups=0, ldx=d["Cin"], ldy=d["Cout"])
    if d.get("res", -1) >= 0:
        d["res"], d["ldr"] = 0, d["Cout"]
    for k in ("in_scale", "in_shift", "bias", "out_scale", "out_shift", "bst_x", "bst_scale", "bst_shift", "bst_mean", "bst_invstd"):
        if d.get(k, -1) >= 0:
            d[k] = 0
    if d.get("bst_x", -1) >= 0:
        d["bst_ldx"] = d["Cin"]
    cop = (d["Cout"] + 127) // 128 * 128
    if kind in ("lean", "halo", "phase"):
        d.update(R=3, S=3, pad=1)
    if kind == "lean":
        d.update(Cin=rng.choice([32, 64, 128]), Cout=rng.choice([32, 64, 96, 128]), N=rng.choice([4, 8, 16]))
        d["Hout"] = d["Wout"] = rng.choice([16, 32, 64])
    elif kind == "gemm":
        d.update(R=1, S=1, pad=0, Cin=rng.choice([32, 64, 128, 192, 256, 576]), Cout=rng.choice([32, 64, 128, 192, 576]), N=rng.choice([1, 4, 16]))
        d["Hout"] = d["Wout"] = rng.choice([8, 16, 32, 64])
    elif kind == "halo":
        d.update(Cin=rng.choice([64, 128, 256, 512]), Cout=rng.choice([64, 128, 160, 192, 256, 512]), N=rng.choice([1, 2, 4, 8]))
        d["Hout"] = d["Wout"] = rng.choice([32, 64, 128, 256])
        if rng.random() < 0.3:
            d["ups"] = 1
            d["w_phase"], d["w_phase_piece"] = 0, 4 * cop * d["Cin"]
        if rng.random() < 0.15:
            d["mask"], d["ldm"] = 0, 1
    elif kind == "phase":
        d.update(ups=2, Cin=rng.choice([64, 128, 256]), Cout=rng.choice([32, 64, 128, 256]), N=rng.choice([1, 2, 4]))
        d["Hout"] = d["Wout"] = rng.choice([32, 64, 128])
        d["w_phase"], d["w_phase_piece"] = 0, 4 * cop * d["Cin"]
        d["in_scale"] = d["in_shift"] = -1
    else:
        d.update(Cin=rng.choice([16, 32, 64, 128, 256]), Cout=rng.choice([16, 32, 64, 128, 256]), N=rng.choice([1, 2]))
        d["Hout"] = d["Wout"] = rng.choice([8, 16, 32, 64])
        if rng.random() < 0.4:
            d["stride"] = 2
    d["ldx"], d["ldy"] = d["Cin"], d["Cout"]
    up = 2 if d.get("stride") == 2 else 1
    d["Hin"], d["Win"] = (d["Hout"] // 2, d["Wout"] // 2) if d["ups"] == 1 else ((2 * d["Hout"], 2 * d["Wout"]) if d["ups"] == 2 else (d["Hout"] * up, d["Wout"] * up))
    d["w_ld"], d["w_tap"], d["w_rows"] = d["Cin"], cop * d["Cin"], cop
    if kind != "small" or rng.random() < 0.5:
        d["w_split"], d["w_piece"] = 0, d["R"] * d["S"] * cop * d["Cin"]
    if d.get("stats", -1) >= 0 and d.get("fin_scale", -1) >= 0:
        d["fin_count"] = d["N"] * d["Hout"] * d["Wout"]


def wgrad_block(rng):
    d = {}
    R = rng.choice([1, 3, 3, 7])
    pad = R // 2 if rng.random() < 0.9 else 0
    stride = rng.choice([0, 0, 1, 1, 2])
    ups = rng.choice([0, 0, 0, 1]) if stride != 2 else 0
    Cin, Cout = rng.choice(CH), rng.choice(CH)
    Ho = rng.choice(SP)
    Wo = Ho if rng.random() < 0.8 else rng.choice(SP + [48])
    Hi, Wi = (max(Ho // 2, 1), max(Wo // 2, 1)) if ups else ((2 * Ho, 2 * Wo) if stride == 2 else (Ho, Wo))
    if rng.random() < 0.05:
        Wi += 1
    N = rng.choice([1, 2, 4, 8, 16])
    flat = rng.random() < 0.1
    d.update(N=N, Cin=Cin, Cout=Cout, Hin=Hi, Win=Wi, Hout=Ho, Wout=Wo, R=R, S=R, pad=pad, stride=stride, ups=ups, alpha=1)
    d["ldx"] = Cin if rng.random() < 0.85 else Cin + rng.choice([2, 4])
    d["ldy"] = Cout if rng.random() < 0.85 else Cout + rng.choice([2, 4])
    d["nbatch"] = rng.choice([0] * 8 + [2])
    d["ksplit"] = rng.choice([0] * 8 + [2])
    d["groups"] = rng.choice([0, 0, 1, 2, 3, 4])
    if flat:
        d["kflat"], d["ktab"] = R * R * Cin, 0

    def al():
        return 0 if rng.random() < 0.93 else rng.choice([4, 8])
    d["x"], d["dy"], d["dw"] = al(), al(), al()
    if rng.random() < 0.3:
        d["dbias"] = al()
    if rng.random() < 0.3:
        d["in_scale"], d["in_shift"], d["in_relu"] = al(), al(), int(rng.random() < 0.85)
    if rng.random() < 0.4:                          # the residual blocks' 3x3 layers (wgrad_lean.hip / wgrad_halo.hip)
        for k in ("kflat", "ktab", "nbatch", "ksplit", "dbias"):
            d.pop(k, None)
        C_ = rng.choice([32, 64, 128])
        d.update(R=3, S=3, pad=1, stride=rng.choice([0, 1]), ups=0, Cin=C_, Cout=rng.choice([C_, 64, 128]), x=0, dy=0, dw=0, N=rng.choice([4, 8, 16]))
        d["Hout"] = d["Wout"] = d["Hin"] = d["Win"] = rng.choice([16, 32, 64])
        d["ldx"], d["ldy"] = d["Cin"], d["Cout"]
        if d.get("in_scale", -1) >= 0:
            d["in_scale"] = d["in_shift"] = 0
    return d


def rows_of(struct, blocks):
    pn, vn = pointer_fields(struct), value_fields(struct)
    ptrs = np.array([[b.get(n, -1) for n in pn] for b in blocks], np.int8)
    vals = np.array([[b.get(n, 0) for n in vn] for b in blocks], np.int64)
    assert np.abs(vals).max() < 2 ** 31
    return ptrs, vals.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "mrfa_amd", "_lib", "libmrfa_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_plan_table.npz"))
    ap.add_argument("--conv", type=int, default=500, help="conv blocks per (mode, tuning)")
    ap.add_argument("--wgrad", type=int, default=250, help="wgrad blocks per (mode, tuning)")
    a = ap.parse_args()
    L = open_lib(a.lib)
    rng = random.Random(20261016)
    out = {}
    for kind, struct, queries, gen, n in (("conv", ConvParams, CONV_QUERIES, conv_block, a.conv),
                                          ("wgrad", WgradParams, WGRAD_QUERIES, wgrad_block, a.wgrad)):
        ptrs, vals, modes, tunings, answers = [], [], [], [], []
        for mode in range(4):
            for ti, tuning in enumerate(TUNINGS):
                pr, vr = rows_of(struct, [gen(rng) for _ in range(n)])
                answers.append(answer(L, mode, tuning, struct, queries, pointer_fields(struct), pr, value_fields(struct), vr))
                ptrs.append(pr)
                vals.append(vr)
                modes += [mode] * n
                tunings += [ti] * n
        out[f"{kind}_ptr_fields"] = np.array(pointer_fields(struct))
        out[f"{kind}_ptrs"] = np.concatenate(ptrs)
        out[f"{kind}_val_fields"] = np.array(value_fields(struct))
        out[f"{kind}_vals"] = np.concatenate(vals)
        out[f"{kind}_mode"] = np.array(modes, np.int8)
        out[f"{kind}_tuning"] = np.array(tunings, np.int8)
        out[f"{kind}_queries"] = np.array(queries)
        out[f"{kind}_answers"] = np.concatenate(answers)
    out["tunings"] = np.array(["" if t is None else f"{t[0]}={t[1]}" for t in TUNINGS])
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes;", {k: v.shape for k, v in out.items() if k.endswith("_vals")})


if __name__ == "__main__":
    main()
