"""tests/ref_tokens.py (the float64 reference the kernel tests of csrc/tokenpose.hip and csrc/attention_mfma.hip compare against) held against ATen in double, and
the per-element bounds of tests/test_token_kernels_gpu.py held from both sides on every input set of that file: the fp32 specification of the ABI
(oracle/capi_emulator.py) meets them -- no bound is tighter than fp32 arithmetic allows -- and each of nine deliberately wrong float64 formulas breaks them.
No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import ref_tokens as R
from tests import test_token_kernels_gpu as K
from tests.kernel_check import report

F64 = torch.float64


def _rel(a, b, what, tol=1e-12):
    err = (a - b).abs().max().item()
    scale = max(b.abs().max().item(), 1e-300)
    assert err <= tol * scale, f"{what}: {err:.3e} vs scale {scale:.3e}"


# ------------------------------------------------------------------------------------------------------------------ the reference against ATen in double
@pytest.mark.parametrize("B,n,heads,d", [(2, 37, 3, 16), (1, 50, 2, 24), (2, 17, 1, 32)])
def test_attention_reference_equals_aten_in_double(B, n, heads, d):
    g = torch.Generator().manual_seed(n)
    inner, scale = heads * d, d ** -0.5
    qkv = torch.randn(B * n, 3 * inner, generator=g, dtype=F64)
    dout = torch.randn(B * n, inner, generator=g, dtype=F64)
    x = qkv.clone().requires_grad_(True)
    q, k, v = [x.view(B, n, 3, heads, d)[:, :, i].permute(0, 2, 1, 3) for i in range(3)]
    dots = torch.einsum("bhid,bhjd->bhij", q, k) * scale                        # tokenpose_base.py:77-91
    o = torch.einsum("bhij,bhjd->bhid", dots.softmax(dim=-1), v).permute(0, 2, 1, 3).reshape(B * n, inner)
    (gx,) = torch.autograd.grad(o, x, dout)
    out, lse = R.attention_ref(qkv, B, n, heads, d, scale)
    dq, dk, dv = R.attention_grads_ref(qkv, dout, B, n, heads, d, scale)
    _rel(out, o.detach(), "out")
    _rel(out, R.rows(F.scaled_dot_product_attention(q, k, v, scale=scale)).detach(), "out (sdpa)")
    _rel(lse, torch.logsumexp(dots, -1).reshape(-1).detach(), "lse")
    for i, (t, name) in enumerate(((dq, "dq"), (dk, "dk"), (dv, "dv"))):
        _rel(t, gx[:, i * inner:(i + 1) * inner], name)
    r = R.attention_grads_ref(qkv, dout, B, n, heads, d, scale, full=True)
    assert (r["s"].abs() <= r["A"] * (1 + 1e-12)).all() and (r["o"].abs() <= r["S_o"] * (1 + 1e-12)).all()
    assert (r["dq"].abs() <= r["S_dq"] * (1 + 1e-12)).all() and (r["dk"].abs() <= r["S_dk"] * (1 + 1e-12)).all() and (r["dv"].abs() <= r["S_dv"] * (1 + 1e-12)).all()
    _rel(r["x"].exp(), r["p"], "exp(s - lse) = p")


@pytest.mark.parametrize("rows,C", [(5, 1), (7, 63), (4, 257)])
def test_layernorm_reference_equals_aten_in_double(rows, C):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(rows, C, generator=g, dtype=F64) * 2 + 1
    gamma, beta, dy = [torch.randn(s, generator=g, dtype=F64) for s in ((C,), (C,), (rows, C))]
    xl, gl, bl = [t.clone().requires_grad_(True) for t in (x, gamma, beta)]
    y0 = F.layer_norm(xl, (C,), gl, bl, 1e-5)
    gx, gg, gb = torch.autograd.grad(y0, [xl, gl, bl], dy)
    y, mean, rstd = R.layernorm_ref(x, gamma, beta, 1e-5)
    dx, dgamma, dbeta = R.layernorm_grads_ref(x, dy, gamma, 1e-5)
    _rel(y, y0.detach(), "y")
    _rel(mean, x.mean(1), "mean")
    _rel(rstd, 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5), "rstd")
    if C > 1:
        _rel(dx, gx, "dx")
        _rel(dgamma, gg, "dgamma")
    else:                                                                        # (C = 1: xhat is identically 0, and with it dx and dgamma)
        assert not dx.any() and not dgamma.any()
        assert max(gx.abs().max().item(), gg.abs().max().item()) <= 1e-12 * dy.abs().max().item()
    _rel(dbeta, gb, "dbeta")


def test_gelu_reference_equals_aten_in_double():
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(500, generator=g, dtype=F64) * 3, torch.tensor(K.GELU_SPECIAL, dtype=F64)])
    dy = torch.randn(x.numel(), generator=g, dtype=F64)
    xl = x.clone().requires_grad_(True)
    y0 = F.gelu(xl)
    (gx,) = torch.autograd.grad(y0, xl, dy)
    assert torch.allclose(R.gelu_ref(x), y0.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(R.gelu_grads_ref(x, dy), gx, rtol=1e-12, atol=1e-300)


def test_attention_lds_window_mirror():
    """the windows derived from the two predicates (att_check of csrc/tokenpose.hip, mrfa_attention_mfma_ok): the VALU kernels alone take the forward at
    n = 1009..1024 / 721..731 / 561..568 and the backward at 961..975 / 705..706 / 545..553 (d = 16 / 24 / 32)"""
    assert [K.att_window(d, False) for d in K.ATT_D] == [(1008, 1024), (720, 731), (560, 568)]
    assert [K.att_window(d, True) for d in K.ATT_D] == [(960, 975), (704, 706), (544, 553)]
    for d in K.ATT_D:
        for n, ff, fb in K.att_lds_cases(d):
            aligned = [(64, 4 * d)] * 4
            assert K.att_family(d, n, 1, aligned[:2], False) == ff and K.att_family(d, n, 1, aligned, True) == fb
    assert K.att_family(24, 276, 0, [(64, 8)] * 2, False) == "valu" and K.att_family(24, 276, 1, [(64, 8), (68, 8)], False) == "valu"
    assert K.att_family(24, 276, 1, [(64, 8), (64, 9)], False) == "valu" and K.att_family(24, 276, 1, [(64, 8)] * 2, False) == "mfma"


# ------------------------------------------------------------------------------------------------------------------ the bounds can be met
ALL_ATT = K.ATT_SETS + K.ATT_LDS_SETS


@pytest.mark.parametrize("case", ALL_ATT, ids=lambda c: "d{}-n{}-{}-B{}h{}".format(*c))
def test_fp32_specification_meets_the_attention_bounds(case):
    test = "spec attention d{} n{} {}".format(*case[:3])
    K.run_att(K.Spec(), K.att_set(*case), test)
    report(test, K.TAG)


@pytest.mark.parametrize("rows,C", K.LN_SETS)
def test_fp32_specification_meets_the_layernorm_bounds(rows, C):
    test = f"spec layernorm {rows}x{C}"
    K.run_ln(K.Spec(), K.ln_set(rows, C), test, scratch=rows % 2 == 1)
    report(test, K.TAG)


@pytest.mark.parametrize("rows,C", K.GELU_SETS)
def test_fp32_specification_meets_the_gelu_bounds(rows, C):
    test = f"spec gelu {rows}x{C}"
    K.run_gelu(K.Spec(), K.gelu_set(rows, C), test)
    report(test, K.TAG)


# ------------------------------------------------------------------------------------------------------------------ the bounds discriminate
def breaks(S, key, mutant):
    """the mutant's output `key`, finite everywhere, leaves that output's bound at some element"""
    ref = S.ref[key]
    mutant = mutant.reshape(ref.shape)
    assert torch.isfinite(mutant).all(), key
    return bool(((mutant - ref).abs() > S.bound[key]).any())


@pytest.mark.parametrize("case", ALL_ATT, ids=lambda c: "d{}-n{}-{}-B{}h{}".format(*c))
def test_wrong_attention_formulas_break_the_bounds(case):
    """Each output a mutation reaches is asserted on its own, against the wider (MFMA-forward) bounds.  Exempt, because the mutation cannot show there:
    the padded-key mutant where n % 16 == 0 (the kernels pad nothing) and where every lse exceeds 17 (the extra key's weight exp(-lse) is below u: the
    peaked sets), and its `out` at the LDS sets (n >= 544: the weight exp(-lse) ~ 1e-3 times |o| ~ S_o / sqrt(n) is of the size of the (2 n + 1) u S_o
    that n roundings are allowed; its lse is asserted there); the last-key mutant at n = 1 (no key would be left); dk without scale and the wrong delta
    at n = 1 (p = 1 and l = 1: dS, dq and dk are identically 0 and the unnormalised output IS the output)."""
    d, n, regime, B, heads = case
    S = K.att_set(*case)
    inner, scale = S.inner, S.scale
    q, k, v = R.split_qkv(S.qkv, B, n, heads, d)
    old = S.dqkv0.double()
    if n > 1:
        m = R.attend(q, k[:, :, :-1], v[:, :, :-1], scale)
        assert breaks(S, "out", R.rows(m["o"])) and breaks(S, "lse", m["lse"]), "last key left out"
    if n % 16 != 0 and S.min_lse <= 17:
        zero = torch.zeros(B, heads, 1, d, dtype=F64)
        m = R.attend(q, torch.cat([k, zero], 2), torch.cat([v, zero], 2), scale)
        assert breaks(S, "lse", m["lse"]), "one all-zero key inside the softmax sum: lse"
        assert n >= 544 or breaks(S, "out", R.rows(m["o"])), "one all-zero key inside the softmax sum: out"
    else:
        assert n % 16 == 0 or regime == "peaked", (case, S.min_lse)
    if n > 1:
        assert breaks(S, "dk", old[:, inner:2 * inner] + (S.ref["dk"] - old[:, inner:2 * inner]) / scale), "dk without scale"
        r = R.attention_ref(S.qkv, B, n, heads, d, scale, full=True)
        do = R.heads_of(S.dout, B, n, heads, d)
        delta = (do * r["o"] * r["l"][..., None]).sum(-1)
        dq, dk, dv = R.attention_grads_ref(S.qkv, S.dout, B, n, heads, d, scale, delta=delta)
        assert breaks(S, "delta", delta), "delta from the unnormalised output: delta"
        assert breaks(S, "dq", dq + old[:, :inner]), "delta from the unnormalised output: dq"
        assert breaks(S, "dk", dk + old[:, inner:2 * inner]), "delta from the unnormalised output: dk"


@pytest.mark.parametrize("rows,C", K.LN_SETS)
def test_wrong_layernorm_formulas_break_the_bounds(rows, C):
    """Each output a mutation reaches is asserted on its own.  Exempt, because the mutation cannot show there: the unbiased variance and the dx mutant at
    C = 1 (C - 1 = 0 has no variance to give; xhat is 0); eps outside the square root at C = 1 in y (d = 0), in rstd where the set has no constant row and
    C > 65 (on rows of variance ~ 4 / 3 it moves rstd by 4.9e-6 relative, the bound on the variance's C-term sum allows (C / 2) u), and in y where C > 8
    (the constant row has d = 0; on the others 4.9e-6 |y| is several times the (C / 2 + 12) u |y| of the bound only while C is small)"""
    S = K.ln_set(rows, C)
    x, gamma, beta, dy, eps = S.x.double(), S.gamma.double(), S.beta.double(), S.dy.double(), K.LN_EPS
    mean = x.sum(1) / C
    d = x - mean[:, None]
    var = (d * d).sum(1) / C
    if C > 1:
        unb = 1 / torch.sqrt((d * d).sum(1) / (C - 1) + eps)
        assert breaks(S, "rstd", unb) and breaks(S, "y", d * unb[:, None] * gamma + beta), "unbiased variance"
    out = 1 / (torch.sqrt(var) + eps)
    if rows >= 2 or C <= 65:
        assert breaks(S, "rstd", out), "eps outside the square root: rstd"
    if 1 < C <= 8:
        assert breaks(S, "y", d * out[:, None] * gamma + beta), "eps outside the square root: y"
    if C > 1:
        rstd = 1 / torch.sqrt(var + eps)
        g = dy * gamma
        assert breaks(S, "dx", S.dx0.double() + rstd[:, None] * (g - g.sum(1, keepdim=True) / C)), "dx without the xhat mean(g xhat) term"


@pytest.mark.parametrize("rows,C", K.GELU_SETS)
def test_wrong_gelu_formulas_break_the_bounds(rows, C):
    S = K.gelu_set(rows, C)
    x, dy = S.x.double(), S.dy.double()
    tanh = 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    assert breaks(S, "y", tanh), "the tanh form"
    assert breaks(S, "dx", S.dx0.double() + dy * 0.5 * (1 + torch.erf(x * R.SQRT1_2))), "backward without the x pdf term"
