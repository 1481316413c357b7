"""The token-transformer kernels (csrc/tokenpose.hip: LayerNorm, GELU, the VALU attention kernels; csrc/attention_mfma.hip) on every dispatch path against the
float64 reference of tests/ref_tokens.py (-m gpu), element by element.  tests/test_token_reference.py runs the same drivers, inputs and bounds on the fp32
specification (oracle/capi_emulator.py) and on deliberately wrong formulas, without a GPU: that is what shows the bounds can be met and that they discriminate.

THE BOUNDS.  Every assertion is |got - ref| <= bound per element; no bound is a fraction of a tensor's maximum.  u = 2^-24.  Each bound counts the fp32 roundings
of the ABI's formula against the reference's companion sums, to first order: a k-term dot product errs by at most k u sum|terms| and a k-term sum by (k - 1) u
sum|terms| IN ANY ORDER (lane-serial, shuffle tree, MFMA accumulation, atomics); a += adds u (|old| + |new|).

  transcendentals.  No document of the ROCm installation states the accuracy of v_exp_f32 / v_log_f32 / v_rsq_f32 or of the device library's erff, so the
  figures are the OpenCL full-profile limits the device library is written to (OpenCL C specification, "Relative error as ULPs"): exp2 3 ulp, log2 3 ulp,
  rsqrt 2 ulp, erf 16 ulp; one ulp is at most 2 u relative: E_EXP2 = E_LOG2 = 6 u, E_RSQ = 4 u, E_ERF = 32 u.  __expf(x) = exp2(x log2 e): the product and
  the constant each move the argument by u |x|: relative 2 u |x| + E_EXP2.  A result below 2^-126 may be flushed: TINY absolute.

  attention (A_ij = scale sum_c |q_ic k_jc|; x_ij = s_ij - lse_i; F the number of exponentials multiplied into one e_ij: 1 in the two-pass VALU forward,
  T + 1 in the online MFMA forward of T = ceil(n / 16) key tiles -- the bounds are per FORWARD family, and the backward's follow the lse they consume):
    score          q scale, d products, d - 1 additions:                                   ds_ij = (d + 2) u A_ij
    e_ij = exp(s_ij - m), any common m (it cancels between numerator and denominator): the score, the subtraction u |s - m|, __expf; in the online form
                   the factors exp(m_old - m_new) multiply it, at most T of them, their arguments summing to at most |s_ij - m_i|:
                                                                                            eps_ij = ds_ij + 3 u |s_ij - m_i| + F (E_EXP2 + u)
    out_ic         eps_i = max_j eps_ij in numerator and denominator; n-term dot product, (n - 1)-addition sum, 1 / l, the product:
                                                                                            (2 eps_i + (2 n + 1) u) sum_j p_ij |v_jc|
    lse_i          log sum exp of the computed scores moves by max_j ds_ij; l as above without ds; log l = log2(l) ln 2; the sum m + log l:
                   max_j ds_ij + max_j (eps_ij - ds_ij) + (n - 1) u + (E_LOG2 + 2 u) log l + 2 u (|m| + log l)
    backward       p_ij = exp(s_ij - lse_i) with the forward's lse:            epsb_ij = ds_ij + b_lse_i + 3 u |x_ij| + E_EXP2 + u
                   delta_i = dO_i . O_i on the forward's out:                  b_delta_i = sum_c |dO_ic| b_out_ic + d u sum_c |dO_ic O_ic|
                   dP_ij = dO_i . V_j:                                         d u sum_c |dO_ic v_jc|
                   dS_ij = p (dP - delta), w = |dP - delta|:                   E_ij = p_ij (epsb_ij w + b_dP_ij + b_delta_i + 2 u w)
                   dq_ic (+=)   scale sum_j E_ij |k_jc| + (n + 3) u (S_dq + |old|);   dk_jc likewise with |q_ic| over i;
                   dv_jc (+=)   sum_i p_ij epsb_ij |dO_ic| + (n + 2) u (S_dv + |old|)
    Where this count departs from the sketch the tests were specified with, and why.  (a) The sketch gives a probability the score error, 2 u |x| for
    __expf's argument product and the instruction's error; here 3 u |s - m|: the subtraction s - m is a rounding of its own, u |s - m|.  (b) The sketch has
    one exponential per probability; the online forward multiplies up to T rescale factors into each, every one an __expf and a product: F (E_EXP2 + u).  The
    two-pass VALU forward has none, and its bound (and that of the fp32 specification, two-pass as well) takes F = 1.  (c) The sketch's output element is
    (2 eps + (n + c) u) S_o; here (2 n + 1) u: the numerator's n-term dot product and the denominator's (n - 1)-addition sum are rounded independently, so
    their relative errors add, n + (n - 1), plus 1 / l and the last product.  All three only widen a bound by roundings the kernels really make; none was
    fitted, and the ratios below show that the narrower sketch would have passed too.
  LayerNorm (two passes; A1 = mean |x|, V the variance, r = rstd, d = x - mean):
    mean           C-term sum, the division:                                   dm = C u A1
    variance       sum_c (x_c - m')^2 = C V + C (m - m')^2 exactly; rounding d (2 u V), squares, sum, division:   dV = dm^2 + (C + 5) u V
    rstd           the addition of eps, rsqrtf:                                dr = r (0.5 (dV + u (V + eps)) / (V + eps) + E_RSQ + u)
    y_c            |gamma_c| (r dm + |d_c| (dr + 4 u r)) + u (|beta_c| + |y_c|)
    backward (on the forward's mean / rstd)   xhat_c: ex_c = r dm + |d_c| dr + 2 u |xhat_c|;   k1 = mean g: (C + 1) u mean |g|;
                   k2 = mean g xhat: mean (|g| ex) + (C + 2) u mean |g xhat|;   t_c = g_c - k1 - xhat_c k2:
                   dx_c (+=)   |t_c| dr + r (b_k1 + ex_c |k2| + |xhat_c| b_k2 + 4 u (|g_c| + |k1| + |xhat_c k2|)) + 2 u (|old| + r |t_c|)
                   dgamma_c (+=)   sum_r |dy_rc| ex_rc + (rows + 3) u (sum_r |dy xhat| + |old|);   dbeta_c (+=)   (rows + 1) u (sum_r |dy| + |old|)
  GELU (t = x / sqrt 2):  the argument moves erf by (2 / sqrt pi) e^{-t^2} 2 u |t|; erff E_ERF |erf|; the sum 1 + erf: u |1 + erf|:   b_E
                   y    0.5 |x| b_E + 2 u |y|
                   dx (+=)   cdf: 0.5 b_E;  pdf = c exp(-x^2 / 2): relative 4 u x^2 / 2 + E_EXP2 + 2 u (+ TINY);
                             |dy| (b_cdf + |x| b_pdf + u |x pdf| + 2 u |cdf + x pdf|) + u (|old| + |new|)

Every operand sits in a wider buffer (kernel_check.Buf): inputs NaN outside their [.., :C] slice, outputs a canary that must survive; every += output starts
from random values; after each call the inputs are bit-identical.  The attention path is predicted from the operands (att_family, a mirror of
mrfa_attention_mfma_ok and att_check) and asserted from the case's construction.

MEASURED on an MI355X, largest err / bound per family (each test prints its own through report()):
  attention, MFMA kernels   out 0.036  lse 0.082  delta 0.006  dq 0.013  dk 0.045  dv 0.289
  attention, VALU kernels   out 0.030  lse 0.066  delta 0.005  dq 0.010  dk 0.045  dv 0.289     (dv: the n = 1 sets, where dv = dO p is three roundings)
  LayerNorm                 y 0.200  mean 0.192  rstd 0.222  dx 0.177  dgamma 0.183  dbeta 0.543
  GELU                      y 0.602  dx 0.499
The worst-case counts are loose where n or C is large (the attention ratios at n ~ 1000 are below 0.02); that the bounds still discriminate is shown by the
mutants of tests/test_token_reference.py, not by these ratios.
"""
import contextlib
import functools
import types

import pytest
import torch

from mrfa_amd import hip
from tests import ref_tokens as R
from tests.kernel_check import CANARY, DEV, F64, NAN, U, Buf, check, note, report

pytestmark = pytest.mark.gpu

E_EXP2, E_LOG2, E_RSQ, E_ERF = 6 * U, 6 * U, 4 * U, 32 * U
TINY = 2.0 ** -126
LDS = 160 * 1024
CAP = 256 * 16                                            # stream_grid (csrc/common.h)
TAG = "tokens"


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def steps(work_threads):
    """trip count of the busiest thread's grid-stride loop in a stream_grid launch over `work_threads` threads' worth of work"""
    blocks = min(max((work_threads + 255) // 256, 1), CAP)
    return -(-work_threads // (blocks * 256))


class Library:
    """libmrfa_hip.so on the GPU"""
    dev, spec = DEV, False

    def call(self, name, *args):
        return getattr(hip.lib(), name)(hip.stream_ptr(), *args)

    def error(self):
        return hip.lib().mrfa_last_error().decode()

    def switch(self, value):
        return hip.tuned(attention_mfma=value)


class Spec:
    """the fp32 specification of the ABI on host memory (no GPU)"""
    dev, spec = "cpu", True

    def __init__(self):
        from oracle.capi_emulator import Emulator
        self.emu = Emulator()

    def call(self, name, *args):
        return getattr(self.emu, name)(0, *args)

    def error(self):
        return self.emu.mrfa_last_error().decode()

    def switch(self, value):
        return contextlib.nullcontext()


def unwritten(shape):
    """the initial content of an output's slice: NaN, so that an element the kernel leaves unwritten fails the comparison (CANARY is what surrounds the slice)"""
    return torch.full(shape, NAN)


# ================================================================================================================== attention
def att_lds(d, n, backward):
    """bytes of LDS of the largest launch: (VALU kernels, MFMA kernels)"""
    npad = -(-n // 16) * 16
    return (2 * n * (d + 4) + (2 * n if backward else 0)) * 4, (2 * npad * (d + 4) + 16 + (2 * npad if backward else 0)) * 4


def att_family(d, n, switch, operands, backward):
    """mirror of att_check + mrfa_attention_mfma_ok: which kernels take a call.  operands: (address, leading dimension) of qkv, out (, dout, dqkv)"""
    valu, mfma = att_lds(d, n, backward)
    if valu > LDS or d not in (16, 24, 32):
        return "refused"
    vec = all(p % 16 == 0 and ld % 4 == 0 for p, ld in operands)
    return "mfma" if switch and mfma <= LDS and vec else "valu"


def att_window(d, backward):
    """(largest n the MFMA kernels take, largest n the VALU kernels take)"""
    fits = lambda n, which: att_lds(d, n, backward)[which] <= LDS
    n_mfma = max(n for n in range(1, 1100) if fits(n, 1))
    n_valu = max(n for n in range(1, 1100) if fits(n, 0))
    return n_mfma, n_valu


REGIMES = ("mild", "peaked", "rows")
ATT_N = (1, 15, 16, 17, 31, 32, 33, 80, 81, 276)
ATT_D = (16, 24, 32)
REGIME_N = (17, 81, 276)


def att_bounds(r, old, n, d, scale, forward):
    """the bounds of the docstring, head layout, after a forward of the given family; r: ref_tokens.attention_grads_ref(full=True); old: |dq0|, |dk0|, |dv0|"""
    F = -(-n // 16) + 1 if forward == "mfma" else 1
    ds_ = (d + 2) * U * r["A"]
    rest = 3 * U * (r["s"] - r["m"][..., None]).abs() + F * (E_EXP2 + U)
    eps_f = (ds_ + rest).max(-1).values
    b_out = (2 * eps_f[..., None] + (2 * n + 1) * U) * r["S_o"] + TINY
    logl = torch.log(r["l"])
    b_lse = ds_.max(-1).values + rest.max(-1).values + (n - 1) * U + (E_LOG2 + 2 * U) * logl + 2 * U * (r["m"].abs() + logl)
    eps_b = ds_ + b_lse[..., None] + 3 * U * r["x"].abs() + E_EXP2 + U
    do = r["do"].abs()
    b_delta = (do * b_out).sum(-1) + d * U * r["S_delta"]
    w = (r["dp"] - r["delta"][..., None]).abs()
    E = r["p"] * (eps_b * w + d * U * r["S_dp"] + b_delta[..., None] + 2 * U * w) + TINY * (1 + w)
    PE = r["p"] * eps_b + TINY
    b_dq = scale * (E @ r["k"].abs()) + (n + 3) * U * (r["S_dq"] + old[0])
    b_dk = scale * (E.transpose(-1, -2) @ r["q"].abs()) + (n + 3) * U * (r["S_dk"] + old[1])
    b_dv = PE.transpose(-1, -2) @ do + (n + 2) * U * (r["S_dv"] + old[2])
    return dict(out=R.rows(b_out), lse=b_lse.reshape(1, -1), delta=b_delta.reshape(1, -1), dq=R.rows(b_dq), dk=R.rows(b_dk), dv=R.rows(b_dv))


@functools.lru_cache(maxsize=None)
def att_set(d, n, regime="mild", B=2, heads=3):
    """one input set with its float64 reference and bounds (computed once, shared, never modified)"""
    g = torch.Generator().manual_seed(100000 * d + 10 * n + REGIMES.index(regime) + 1000 * B)
    inner = heads * d
    qkv = torch.rand(B * n, 3 * inner, generator=g) * 4 - 2
    v5 = qkv.view(B, n, 3, heads, d)
    if regime == "peaked":
        v5[:, :, 0] *= 100.0                               # scores of +-500: a near one-hot softmax, every online rescale a large step
    if regime == "rows":
        v5[:, 0, 0] = 0.0                                  # row 0: q = 0, a uniform 1 / n
        v5[0, n - 1, 1] = 3.0 * v5[0, 1, 0]                # sample 0, row 1: the maximum is the last valid key n - 1 (the mask boundary)
        v5[1, 3, 1] = v5[1, n - 1, 1] = 2.5 * v5[1, 2, 0]  # sample 1, row 2: the maximum twice, in the first and in the last 16-key tile
    dout = torch.randn(B * n, inner, generator=g)
    dqkv0 = torch.randn(B * n, 3 * inner, generator=g)
    scale = f32(d ** -0.5)
    r = R.attention_grads_ref(qkv, dout, B, n, heads, d, scale, full=True)
    old = [t.abs() for t in R.split_qkv(dqkv0, B, n, heads, d)]
    S = types.SimpleNamespace(d=d, n=n, regime=regime, B=B, heads=heads, inner=inner, scale=scale, qkv=qkv, dout=dout, dqkv0=dqkv0)
    S.bounds = {fam: att_bounds(r, old, n, d, scale, fam) for fam in ("mfma", "valu")}      # by the family of the forward
    S.bound = S.bounds["mfma"]                             # the wider of the two: what a wrong formula has to break
    o0 = dqkv0.double()
    S.ref = dict(out=r["out"], lse=r["lse"].reshape(1, -1), delta=r["delta"].reshape(1, -1), dq=R.rows(r["dq"]) + o0[:, :inner],
                 dk=R.rows(r["dk"]) + o0[:, inner:2 * inner], dv=R.rows(r["dv"]) + o0[:, 2 * inner:])
    S.min_lse, S.min_range = r["lse"].min().item(), (r["s"].max(-1).values - r["s"].min(-1).values).min().item()
    if regime == "peaked":
        assert S.min_range > 120, S.min_range
    if regime == "rows":
        s = r["s"]
        assert torch.allclose(r["p"][:, :, 0], torch.full_like(r["p"][:, :, 0], 1.0 / n), rtol=1e-12, atol=0)
        assert (s[0, :, 1].argmax(-1) == n - 1).all()
        assert (s[1, :, 2, 3] == s[1, :, 2, n - 1]).all() and (s[1, :, 2].max(-1).values == s[1, :, 2, 3]).all() and (n - 1) // 16 > 0
    return S


PATHS = {                                                  # (switch at the forward, at the backward), misaligned out, misaligned dqkv -> the families
    "mfma": ((1, 1), False, False, ("mfma", "mfma")),
    "valu by switch": ((0, 0), False, False, ("valu", "valu")),
    "valu by operands": ((1, 1), True, True, ("valu", "valu")),
    "mfma fwd, valu bwd": ((1, 1), False, True, ("mfma", "valu")),
    "valu fwd, mfma bwd": ((0, 1), False, False, ("valu", "mfma")),
}


def run_att(be, S, test, path="mfma", expect=None, keep=None):
    """forward, then the backward on the forward's out and lse; returns the families that ran"""
    sw, mis_out, mis_dq, fams = PATHS[path]
    B, n, heads, d, inner, dev = S.B, S.n, S.heads, S.d, S.inner, be.dev
    N = B * heads * n
    bq = Buf(S.qkv, 1, 3 * inner + 4, NAN, lead=4, dev=dev)         # qkv and dout stay aligned: the VALU kernels stage them with float4
    bo = Buf(unwritten((B * n, inner)), 1, inner + (1 if mis_out else 4), CANARY, lead=1 if mis_out else 8, dev=dev)
    bl = Buf(unwritten((1, N)), 1, N + 3, CANARY, lead=2, dev=dev)
    bdo = Buf(S.dout, 1, inner + 8, NAN, lead=4, dev=dev)
    bdq = Buf(S.dqkv0, 1, 3 * inner + (1 if mis_dq else 8), CANARY, lead=3 if mis_dq else 4, dev=dev)
    bdl = Buf(unwritten((1, N)), 1, N + 1, CANARY, lead=1, dev=dev)
    fam_f = att_family(d, n, sw[0], [(bq.ptr, bq.ld), (bo.ptr, bo.ld)], False)
    fam_b = att_family(d, n, sw[1], [(bq.ptr, bq.ld), (bo.ptr, bo.ld), (bdo.ptr, bdo.ld), (bdq.ptr, bdq.ld)], True)
    if not be.spec:
        assert (fam_f, fam_b) == (expect or fams), (path, fam_f, fam_b, expect or fams)
        print(f"[{TAG}] attention d={d} n={n} B={B} heads={heads} {S.regime} [{path}]: forward {fam_f}<{d}>, backward {fam_b}<{d}>")
    bound = S.bounds["valu" if be.spec else fam_f]         # (the specification's forward is two-pass, as the VALU kernels')
    with be.switch(sw[0]):
        rc = be.call("mrfa_attention_fwd", bq.ptr, bq.ld, B, n, heads, d, S.scale, bo.ptr, bo.ld, bl.ptr)
        assert rc == 0, be.error()
        out, lse = bo.get(), bl.get()
        note(test, f"out[{fam_f}]", check(out, S.ref["out"], bound["out"], f"out [{fam_f}, {path}]"))
        note(test, f"lse[{fam_f}]", check(lse, S.ref["lse"], bound["lse"], f"lse [{fam_f}, {path}]"))
        out_bits, lse_bits = bo.bits(), bl.bits()
        with be.switch(sw[1]):
            rc = be.call("mrfa_attention_bwd", bq.ptr, bq.ld, bo.ptr, bo.ld, bdo.ptr, bdo.ld, bl.ptr, bdl.ptr, B, n, heads, d, S.scale, bdq.ptr, bdq.ld)
    if fam_b == "refused" and not be.spec:
        msg = be.error()
        assert rc != 0 and "attention_bwd" in msg and "LDS" in msg, (rc, msg)
        assert bdq.untouched() and bdl.untouched(), "a refused backward wrote"
    else:
        assert rc == 0, be.error()
        dqkv, fam = bdq.get(), fam_b if not be.spec else "spec"
        note(test, f"delta[{fam}]", check(bdl.get(), S.ref["delta"], bound["delta"], f"delta [{fam}, {path}]"))
        for i, k in enumerate(("dq", "dk", "dv")):
            note(test, f"{k}[{fam}]", check(dqkv[:, i * inner:(i + 1) * inner], S.ref[k], bound[k], f"{k} [{fam}, {path}]"))
    assert bq.untouched() and bdo.untouched(), "an input changed"
    assert torch.equal(bo.bits(), out_bits) and torch.equal(bl.bits(), lse_bits), "the backward changed out / lse"
    if keep is not None:
        keep.append((out_bits, lse_bits, bdq.bits(), bdl.bits()))
    return fam_f, fam_b


ATT_SETS = [(d, n, "mild", 2, 3) for d in ATT_D for n in ATT_N] + [(d, n, reg, 2, 3) for d in ATT_D for reg in ("peaked", "rows") for n in REGIME_N]


def att_lds_cases(d):
    """(n, forward family, backward family) around the two windows in which the unpadded LDS image fits 160 KB and the 16-row padded one does not"""
    f_mfma, f_valu = att_window(d, False)
    b_mfma, b_valu = att_window(d, True)
    assert b_mfma < b_valu < f_mfma < f_valu
    return [(b_mfma, "mfma", "mfma"), (b_valu, "mfma", "valu"), (f_mfma, "mfma", "refused"), (f_valu, "valu", "refused")]


ATT_LDS_SETS = [(d, n, "mild", 1, 2) for d in ATT_D for n, _, _ in att_lds_cases(d)]


@pytest.mark.parametrize("n", ATT_N)
@pytest.mark.parametrize("d", ATT_D)
def test_attention_every_path(d, n):
    """a single ragged tile, n = 1, multiples of 16 (no masked key), the workgroup boundaries of both families (80 / 81, 32 / 33) and the workload's 276 on the
    MFMA kernels, the VALU kernels (by the switch; by an `out` / `dqkv` of leading dimension width + 1 on a 4-byte aligned base) and both mixed orders, the
    lse of one family consumed by the other"""
    test = f"attention d{d} n{n}"
    S = att_set(d, n)
    for path in PATHS:
        run_att(Library(), S, test, path)
    report(test, TAG)


@pytest.mark.parametrize("n", REGIME_N)
@pytest.mark.parametrize("regime", ["peaked", "rows"])
@pytest.mark.parametrize("d", ATT_D)
def test_attention_score_regimes(d, regime, n):
    """peaked: q x 100, every row's score range > 120; rows: q = 0, the maximum at the last valid key, the maximum duplicated in two key tiles (att_set)"""
    test = f"attention {regime} d{d} n{n}"
    S = att_set(d, n, regime)
    for path in ("mfma", "valu by switch"):
        run_att(Library(), S, test, path)
    report(test, TAG)


@pytest.mark.parametrize("d", ATT_D)
def test_attention_lds_windows(d):
    """B = 1, heads = 2.  The largest n the MFMA backward takes; the largest n of the VALU backward (MFMA forward: its lse handed over; > 64 KB of dynamic LDS);
    the largest n of the MFMA forward and of the VALU forward: there the backward is refused with a message and leaves dqkv and delta untouched"""
    test = f"attention lds d{d}"
    for n, ff, fb in att_lds_cases(d):
        assert att_lds(d, n, False)[0] > 64 * 1024
        run_att(Library(), att_set(d, n, "mild", 1, 2), test, "mfma", expect=(ff, fb))
    report(test, TAG)


@pytest.mark.parametrize("d", ATT_D)
def test_attention_mfma_runs_are_bit_identical(d):
    """the MFMA kernels use no atomics: two runs of the forward and of the backward give the same bits"""
    for n in (81, 276):
        keep = []
        for _ in range(2):
            run_att(Library(), att_set(d, n), f"attention twice d{d}", "mfma", keep=keep)
        assert all(torch.equal(a, b) for a, b in zip(*keep)), (d, n)


# ================================================================================================================== LayerNorm
LN_EPS = f32(1e-5)
LN_C = (1, 4, 63, 64, 65, 192, 256, 257, 512, 1024)
LN_ROWS = (1, 2, 3, 37)
LN_THRESHOLD_ROWS = (2047, 2048, 2049, 4095, 4096, 4097)
LN_BIG = [(r, 8) for r in LN_THRESHOLD_ROWS] + [(4416, 192), (2049, 257), (4097, 257)]
LN_SETS = [(r, c) for c in LN_C for r in LN_ROWS] + LN_BIG


def ln_launch(rows, C, scratch):
    """(template, rows per wave, workgroups) of mrfa_layernorm_bwd"""
    rpw = (4 if rows >= 2048 else 2) if scratch else (8 if rows >= 4096 else 2)
    return ("<4, 4>" if C <= 256 else "<16, 1>"), rpw, -(-rows // (4 * rpw))


def ln_bounds(f, C, rows, old):
    eps = LN_EPS
    r, V, d, gam, xh = f["rstd"], f["var"], f["d"].abs(), f["gamma"].abs(), f["xh"].abs()
    dm = C * U * f["A1"]
    dV = dm * dm + (C + 5) * U * V
    dr = r * (0.5 * (dV + U * (V + eps)) / (V + eps) + E_RSQ + U)
    b_y = gam * (r * dm)[:, None] + gam * d * (dr + 4 * U * r)[:, None] + U * (f["beta"].abs() + f["y"].abs())
    ex = (r * dm)[:, None] + d * dr[:, None] + 2 * U * xh
    g, k1, k2, t = f["g"].abs(), f["k1"].abs(), f["k2"].abs(), f["t"].abs()
    b_k1 = (C + 1) * U * f["G1"]
    b_k2 = (g * ex).sum(1) / C + (C + 2) * U * f["S_k2"]
    b_dx = t * dr[:, None] + r[:, None] * (b_k1[:, None] + ex * k2[:, None] + xh * b_k2[:, None] + 4 * U * (g + k1[:, None] + xh * k2[:, None])) \
        + 2 * U * (old[0] + r[:, None] * t)
    b_dg = (f["dy"].abs() * ex).sum(0) + (rows + 3) * U * (f["S_dg"] + old[1])
    b_db = (rows + 1) * U * (f["S_db"] + old[2])
    return dict(y=b_y, mean=dm.view(1, -1), rstd=dr.view(1, -1), dx=b_dx, dgamma=b_dg.view(1, -1), dbeta=b_db.view(1, -1))


@functools.lru_cache(maxsize=None)
def ln_set(rows, C):
    """x ~ U(-2, 2); the last row constant (rows >= 2: variance 0, rstd = 1 / sqrt(eps)), the one before it 1000 + U(-1, 1) (rows >= 3)"""
    g = torch.Generator().manual_seed(1000 * rows + C)
    x = torch.rand(rows, C, generator=g) * 4 - 2
    if rows >= 2:
        x[rows - 1] = 3.25
    if rows >= 3:
        x[rows - 2] = 1000.0 + torch.rand(C, generator=g) * 2 - 1
    S = types.SimpleNamespace(rows=rows, C=C, x=x, gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g), dy=torch.randn(rows, C, generator=g),
                              dx0=torch.randn(rows, C, generator=g), dg0=torch.randn(C, generator=g), db0=torch.randn(C, generator=g))
    f = R.layernorm_grads_ref(x, S.dy, S.gamma, LN_EPS, full=True)
    f["beta"] = S.beta.double()
    f["y"] = f["y"] + f["beta"]
    S.bound = ln_bounds(f, C, rows, (S.dx0.double().abs(), S.dg0.double().abs(), S.db0.double().abs()))
    S.ref = dict(y=f["y"], mean=f["mean"].view(1, -1), rstd=f["rstd"].view(1, -1), dx=f["dx"] + S.dx0.double(), dgamma=(f["dgamma"] + S.dg0.double()).view(1, -1),
                 dbeta=(f["dbeta"] + S.db0.double()).view(1, -1))
    return S


def run_ln(be, S, test, scratch=False, null=()):
    """four distinct leading dimensions, no alignment anywhere"""
    rows, C, dev = S.rows, S.C, be.dev
    bx = Buf(S.x, 1, C + 1, NAN, lead=1, dev=dev)
    bg, bb = Buf(S.gamma.view(1, C), 1, C + 2, NAN, lead=1, dev=dev), Buf(S.beta.view(1, C), 1, C + 1, NAN, lead=3, dev=dev)
    by = Buf(unwritten((rows, C)), 1, C + 3, CANARY, lead=2, dev=dev)
    bm, br = Buf(unwritten((1, rows)), 1, rows + 2, CANARY, lead=1, dev=dev), Buf(unwritten((1, rows)), 1, rows + 1, CANARY, lead=3, dev=dev)
    rc = be.call("mrfa_layernorm_fwd", bx.ptr, bx.ld, rows, C, bg.ptr, bb.ptr, LN_EPS, by.ptr, by.ld, bm.ptr, br.ptr)
    assert rc == 0, be.error()
    for k, b in (("y", by), ("mean", bm), ("rstd", br)):
        note(test, k, check(b.get(), S.ref[k], S.bound[k], f"layernorm {k} {rows} x {C}"))
    bdy = Buf(S.dy, 1, C + 2, NAN, lead=3, dev=dev)
    bdx = Buf(S.dx0, 1, C + 5, CANARY, lead=1, dev=dev)
    bdg, bdb = Buf(S.dg0.view(1, C), 1, C + 1, CANARY, lead=2, dev=dev), Buf(S.db0.view(1, C), 1, C + 3, CANARY, lead=1, dev=dev)
    nsc = hip.LN_SLOTS * 2 * C + 1
    bsc = Buf(torch.zeros(1, nsc), 1, nsc + 4, CANARY, dev=dev) if scratch else None
    tmpl, rpw, wgs = ln_launch(rows, C, scratch)
    mean_bits, rstd_bits = bm.bits(), br.bits()
    rc = be.call("mrfa_layernorm_bwd", bx.ptr, bx.ld, bdy.ptr, bdy.ld, rows, C, bg.ptr, bm.ptr, br.ptr, bdx.ptr, bdx.ld,
                 None if "dgamma" in null else bdg.ptr, None if "dbeta" in null else bdb.ptr, bsc.ptr if scratch else None)
    assert rc == 0, be.error()
    var = f"{tmpl} rpw {rpw}" + (" slots" if scratch else "") + "".join(f" no {k}" for k in null)
    note(test, f"dx[{var}]", check(bdx.get(), S.ref["dx"], S.bound["dx"], f"layernorm dx {rows} x {C} [{var}]"))
    for k, b in (("dgamma", bdg), ("dbeta", bdb)):
        if k in null:
            assert b.untouched()
        else:                                              # (added to twice, or not at all, is far outside the bound: the old values are of order 1)
            note(test, f"{k}[{var}]", check(b.get(), S.ref[k], S.bound[k], f"layernorm {k} {rows} x {C} [{var}]"))
    if scratch and not be.spec:
        ticket = bsc.get().view(torch.int32)[0, -1].item()
        assert ticket == wgs, f"ticket word {ticket}, {wgs} workgroups"
    assert all(b.untouched() for b in (bx, bg, bdy)) and torch.equal(bm.bits(), mean_bits) and torch.equal(br.bits(), rstd_bits), "an input changed"
    return var


@pytest.mark.parametrize("C", LN_C)
def test_layernorm_small_rows_every_width(C):
    """rows 1 .. 3 and 37 (a ragged last wave and workgroup) at C = 1, around 64, at the template switch 256 / 257 and at all four rounds of the
    parameter-gradient loop (1024), with and without the slotted scratch"""
    test = f"layernorm C{C}"
    seen = set()
    for rows in LN_ROWS:
        for scratch in (False, True):
            seen.add(run_ln(Library(), ln_set(rows, C), test, scratch))
    print(f"[{TAG}] {test}: backward variants {sorted(seen)}")
    report(test, TAG)


@pytest.mark.parametrize("rows,C", LN_BIG)
def test_layernorm_rows_per_wave_thresholds(rows, C):
    """both sides of rows = 2048 (with scratch: 2 -> 4 rows per wave) and 4096 (without: 2 -> 8) at C = 8, the workload's 4416 x 192, and the <16, 1>
    template at both settings (C = 257)"""
    test = f"layernorm {rows}x{C}"
    seen = [run_ln(Library(), ln_set(rows, C), test, scratch) for scratch in (False, True)]
    print(f"[{TAG}] {test}: backward variants {seen}")
    report(test, TAG)


@pytest.mark.parametrize("rows,C", [(37, 192), (3, 257)])
def test_layernorm_null_parameter_gradients(rows, C):
    test = f"layernorm null {rows}x{C}"
    for null in (("dgamma",), ("dbeta",)):
        for scratch in (False, True):
            run_ln(Library(), ln_set(rows, C), test, scratch, null)
    report(test, TAG)


# ================================================================================================================== GELU
GELU_SPECIAL = [s * v for v in (0.0, 1e-30, 1e-4, 0.5, 1.0, 3.0, 5.0, 6.0, 10.0, 40.0) for s in (1.0, -1.0)]
GELU_SETS = [(5, 4), (37, 52), (300, 576), (1100, 4000)]      # the last: 1 100 000 float4, more than stream_grid's 4096 x 256 threads


def gelu_bounds(f, old):
    x, t, erf = f["x"].abs(), f["t"].abs(), f["erf"]
    b_E = 1.1283791670955126 * torch.exp(-t * t) * 2 * U * t + E_ERF * erf.abs() + U * (1 + erf).abs()
    b_y = 0.5 * x * b_E + 2 * U * f["y"].abs()
    pdf = f["pdf"]
    b_pdf = pdf * (4 * U * 0.5 * x * x + E_EXP2 + 2 * U) + TINY
    inner = (f["cdf"] + f["x"] * pdf).abs()
    b_dx = f["dy"].abs() * (0.5 * b_E + x * b_pdf + U * x * pdf + 2 * U * inner) + 2 * U * (old + f["dx"].abs())
    return dict(y=b_y, dx=b_dx)


@functools.lru_cache(maxsize=None)
def gelu_set(rows, C):
    g = torch.Generator().manual_seed(rows + C)
    x = torch.rand(rows * C, generator=g) * 8 - 4
    k = x[::7].numel()
    x[::7] = torch.tensor(GELU_SPECIAL).repeat(-(-k // len(GELU_SPECIAL)))[:k]
    S = types.SimpleNamespace(rows=rows, C=C, x=x.view(rows, C), dy=torch.randn(rows, C, generator=g), dx0=torch.randn(rows, C, generator=g))
    f = R.gelu_grads_ref(S.x, S.dy, full=True)
    S.bound = gelu_bounds(f, S.dx0.double().abs())
    S.ref = dict(y=f["y"], dx=f["dx"] + S.dx0.double())
    return S


def run_gelu(be, S, test):
    """padded, 16-byte aligned views with three different leading dimensions"""
    rows, C, dev = S.rows, S.C, be.dev
    bx = Buf(S.x, 1, C + 4, NAN, lead=4, dev=dev)
    by = Buf(unwritten((rows, C)), 1, C + 8, CANARY, lead=8, dev=dev)
    rc = be.call("mrfa_gelu_fwd", bx.ptr, bx.ld, rows, C, by.ptr, by.ld)
    assert rc == 0, be.error()
    note(test, "y", check(by.get(), S.ref["y"], S.bound["y"], f"gelu y {rows} x {C}"))
    del by
    bdy = Buf(S.dy, 1, C + 8, NAN, lead=4, dev=dev)
    bdx = Buf(S.dx0, 1, C + 12, CANARY, lead=4, dev=dev)
    rc = be.call("mrfa_gelu_bwd", bx.ptr, bx.ld, bdy.ptr, bdy.ld, rows, C, bdx.ptr, bdx.ld)
    assert rc == 0, be.error()
    note(test, "dx", check(bdx.get(), S.ref["dx"], S.bound["dx"], f"gelu dx {rows} x {C}"))
    assert bx.untouched() and bdy.untouched(), "an input changed"


@pytest.mark.parametrize("rows,C", GELU_SETS)
def test_gelu_tails_and_grid_stride(rows, C):
    """+-0, +-1e-30, +-1e-4 ... +-40 among U(-4, 4): the tails where erff saturates and __expf(-x^2 / 2) underflows; the largest launch grid-strides"""
    test = f"gelu {rows}x{C}"
    trips = steps(rows * C // 4)
    if (rows, C) == GELU_SETS[-1]:
        assert trips >= 2
    print(f"[{TAG}] {test}: grid-stride trip count {trips}")
    run_gelu(Library(), gelu_set(rows, C), test)
    report(test, TAG)


# ================================================================================================================== argument checks
def test_token_kernels_refuse_what_they_do_not_take():
    be = Library()
    bufs = [Buf(unwritten((4, 1100)), 1, 1100, CANARY) for _ in range(6)]
    zeros = Buf(torch.zeros(4, 1100), 1, 1100, 0.0)
    p = [b.ptr for b in bufs]
    z = zeros.ptr

    def refused(rc, name):
        msg = be.error()
        assert rc != 0 and len(msg) > 10 and name in msg, (rc, msg)
    for C in (1025, 0):
        refused(be.call("mrfa_layernorm_fwd", z, 1100, 4, C, z, z, LN_EPS, p[0], 1100, p[1], p[2]), "layernorm_fwd")
        refused(be.call("mrfa_layernorm_bwd", z, 1100, z, 1100, 4, C, z, z, z, p[3], 1100, p[4], p[5], None), "layernorm_bwd")
    for C in (6, 1, 1099):
        refused(be.call("mrfa_gelu_fwd", z, 1100, 4, C, p[0], 1100), "gelu_fwd")
        refused(be.call("mrfa_gelu_bwd", z, 1100, z, 1100, 4, C, p[3], 1100), "gelu_bwd")
    assert all(b.untouched() for b in bufs), "a refused call wrote"
