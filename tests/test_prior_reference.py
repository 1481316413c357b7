"""tests/ref_prior.py (the float64 reference the kernel tests of csrc/prior.hip compare against) held against ATen in double, and the per-element bounds of
tests/test_prior_kernels_gpu.py held from both sides on every input set of that file, through the same drivers: the fp32 specification of the ABI
(oracle/capi_emulator.py) meets them -- no bound is tighter than fp32 arithmetic allows -- and each of twelve deliberately wrong float64 formulas breaks one.
The kink share of every prior_motion set is within 0.1 % on the reference alone.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import ref_prior as R
from tests import test_prior_kernels_gpu as K
from tests.kernel_check import report

F64 = torch.float64


def _rel(a, b, what, tol=1e-12):
    err = (a - b).abs().max().item()
    scale = max(b.abs().max().item(), 1e-300)
    assert err <= tol * scale, f"{what}: {err:.3e} vs scale {scale:.3e}"


def rnd(g, *s, lo=-1.0, hi=1.0):
    return torch.rand(*s, generator=g, dtype=F64) * (hi - lo) + lo


def aten_grid(H, W):
    xs, ys = torch.linspace(-1, 1, W, dtype=F64), torch.linspace(-1, 1, H, dtype=F64)
    return torch.stack([xs.view(1, W).expand(H, W), ys.view(H, 1).expand(H, W)], -1)


# ------------------------------------------------------------------------------------------------------------------ the reference against ATen in double
@pytest.mark.parametrize("B,K,H,W", [(2, 3, 5, 7), (1, 1, 2, 3), (3, 4, 6, 4)])
def test_kp_gaussian_reference_equals_aten_in_double(B, K, H, W):
    g = torch.Generator().manual_seed(B + H)
    kp, pos, dout, var = rnd(g, B, K, 2), rnd(g, K, H, W), rnd(g, B, H, W, K), 0.07
    kl, pl = kp.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    d = aten_grid(H, W).view(1, 1, H, W, 2) - kl.view(B, K, 1, 1, 2)
    out = (torch.exp(-0.5 * (d * d).sum(-1) / var) + pl).permute(0, 2, 3, 1)
    gk, gp = torch.autograd.grad(out, (kl, pl), dout)
    _rel(R.kp_gaussian_fwd(kp, pos, H, W, var)["out"], out.detach(), "out")
    r = R.kp_gaussian_bwd(kp, dout, H, W, var)
    _rel(r["dkp"], gk, "dkp")
    _rel(r["dpos"], gp, "dpos")
    assert (r["dkp"].abs() <= r["S_dkp"] * (1 + 1e-12)).all() and (r["dpos"].abs() <= r["S_dpos"] * (1 + 1e-12)).all()


@pytest.mark.parametrize("B,K,H,W,C,jac,bg", [(2, 3, 5, 7, 3, True, True), (1, 1, 4, 3, 1, False, False), (2, 2, 6, 9, 2, True, False)])
def test_prior_motion_reference_equals_aten_in_double(B, K, H, W, C, jac, bg):
    """torch.linalg.inv, F.grid_sample(align_corners=False, padding_mode="zeros") and torch.autograd.grad; keypoint pairs that put samples into the border bands
    and outside"""
    g = torch.Generator().manual_seed(K + W)
    K1, inv_var = K + 1, 100.0
    kd, ks = rnd(g, B, K, 2, lo=-0.8, hi=0.8), rnd(g, B, K, 2, lo=-0.8, hi=0.8)
    ks[:, -1] = kd[:, -1] + 0.9
    eye = torch.tensor([1.0, 0, 0, 1.0], dtype=F64)
    jd, js = (eye + 0.2 * rnd(g, B, K, 4), eye + 0.2 * rnd(g, B, K, 4)) if jac else (None, None)
    bgm = torch.eye(3, dtype=F64).reshape(9) + 0.1 * rnd(g, B, 9) if bg else None
    src = rnd(g, B, H, W, C, lo=0.0)
    dheat, dwarp, dmot = rnd(g, B, K1, H, W), rnd(g, B, K1, C, H, W), rnd(g, B, K1, H, W, 2)
    leaves = [t.clone().requires_grad_(True) for t in (kd, ks, jd, js, bgm) if t is not None]
    it = iter(leaves)
    kdl, ksl = next(it), next(it)
    jdl, jsl = (next(it), next(it)) if jac else (None, None)
    bgl = next(it) if bg else None
    ident = aten_grid(H, W).view(1, 1, H, W, 2)
    gauss = lambda kp: torch.exp(-0.5 * ((ident - kp.view(B, K, 1, 1, 2)) ** 2).sum(-1) * inv_var)
    heat = torch.cat([torch.zeros(B, 1, H, W, dtype=F64), gauss(kdl) - gauss(ksl)], 1)
    z = ident - kdl.view(B, K, 1, 1, 2)
    if jac:
        J = jsl.view(B, K, 2, 2) @ torch.linalg.inv(jdl.view(B, K, 2, 2))
        z = torch.einsum("bkij,bkhwj->bkhwi", J, z)
    mo = z + ksl.view(B, K, 1, 1, 2)
    m0 = ident.expand(B, 1, H, W, 2)
    if bg:
        hom = torch.cat([m0, torch.ones_like(m0[..., :1])], -1)
        hom = (bgl.view(B, 1, 1, 1, 3, 3) @ hom.unsqueeze(-1)).squeeze(-1)
        m0 = hom[..., :2] / hom[..., 2:3]
    motions = torch.cat([m0, mo], 1)
    rep = src.permute(0, 3, 1, 2).unsqueeze(1).expand(B, K1, C, H, W).reshape(B * K1, C, H, W)
    wv = F.grid_sample(rep, motions.reshape(B * K1, H, W, 2), mode="bilinear", padding_mode="zeros", align_corners=False).view(B, K1, C, H, W)
    grads = torch.autograd.grad([heat, wv, motions], leaves, [dheat, dwarp, dmot])
    f = R.prior_fwd(kd, ks, jd, js, bgm, H, W, inv_var)
    _rel(f["motions"], motions.detach(), "motions")
    _rel(f["heat"], heat.detach(), "heat")
    wp = R.warp(src, motions.detach())
    _rel(wp["val"], wv.detach(), "warp")
    assert ((wp["ix"] < 0) & wp["inside"]).any() and (~wp["inside"]).any() and (wp["val"].abs() <= wp["tapabs"] * (1 + 1e-12)).all()
    r = R.prior_bwd(f, wp, dheat, dwarp, dmot)
    got = [r["dkd"], r["dks"]] + ([r["djd"], r["djs"]] if jac else []) + ([r["dbg"]] if bg else [])
    for a, b, what in zip(got, grads, ["dkd", "dks"] + (["djd", "djs"] if jac else []) + ["dbg"]):
        _rel(a, b.view_as(a), what)
    assert (r["acc"].abs() <= r["Sacc"] * (1 + 1e-12)).all()
    if jac:
        assert (r["djd"].abs() <= r["Cjd"] * (1 + 1e-12)).all() and (r["djs"].abs() <= r["Cjs"] * (1 + 1e-12)).all()
        _rel(torch.stack(f["A"]["J"], -1).view(B, K, 2, 2), J.detach(), "J")
    # the slope companion bounds the change of the value under a small shift of the position
    eps = 1e-3
    for dx, dy, key in ((eps, 0.0, "slope_h"), (0.0, eps, "slope_v")):
        m2 = motions.detach() + torch.tensor([dx * 2 / W, dy * 2 / H], dtype=F64)
        assert ((R.warp(src, m2)["val"] - wp["val"]).abs() <= wp[key] * eps * (1 + 1e-9) + 1e-15).all(), key


@pytest.mark.parametrize("B,H,W,K1", [(2, 3, 5, 4), (1, 2, 3, 1), (2, 4, 3, 7)])
def test_softmax_combine_reference_equals_aten_in_double(B, H, W, K1):
    g = torch.Generator().manual_seed(K1)
    l, mo = rnd(g, B, H, W, K1, lo=-3, hi=3), rnd(g, B, K1, H, W, 2)
    ddef, dmask, dn = rnd(g, B, H, W, 2), rnd(g, B, K1, H, W), rnd(g, B, K1, H, W)
    ll, ml = l.clone().requires_grad_(True), mo.clone().requires_grad_(True)
    mask = F.softmax(ll, -1)
    deform = (mask.unsqueeze(-1) * ml.permute(0, 2, 3, 1, 4)).sum(3)
    outs = [deform, mask.permute(0, 3, 1, 2), ll.permute(0, 3, 1, 2)]
    gl, gm = torch.autograd.grad(outs, (ll, ml), [ddef, dmask, dn])
    r = R.softmax_combine_fwd(l, mo)
    _rel(r["mask"], outs[1].detach(), "mask")
    _rel(r["deformation"], deform.detach(), "deformation")
    assert torch.equal(r["logit_nchw"], outs[2].detach())
    rb = R.softmax_combine_bwd(mo, r["mask"], ddef, dmask, dn)
    _rel(rb["dlogit"], gl, "dlogit")
    _rel(rb["dmotions"], gm, "dmotions")


@pytest.mark.parametrize("B,H,W,K,jac", [(2, 5, 7, 3, True), (1, 2, 3, 1, True), (2, 6, 4, 2, False)])
def test_kp_head_reference_equals_aten_in_double(B, H, W, K, jac):
    g = torch.Generator().manual_seed(H)
    T = 0.1
    lg, jm = rnd(g, B, H, W, K), rnd(g, B, H, W, 4) if jac else None
    dkp, djac = rnd(g, B, K, 2), rnd(g, B, K, 4)
    leaves = [lg.clone().requires_grad_(True)] + ([jm.clone().requires_grad_(True)] if jac else [])
    heat = F.softmax(leaves[0].reshape(B, H * W, K) / T, dim=1)
    kp = torch.einsum("bpk,pc->bkc", heat, aten_grid(H, W).reshape(H * W, 2))
    outs, gs = [kp], [dkp]
    if jac:
        outs.append(torch.einsum("bpk,bpj->bkj", heat, leaves[1].reshape(B, H * W, 4)))
        gs.append(djac)
    grads = torch.autograd.grad(outs, leaves, gs)
    r = R.kp_head_fwd(lg, jm, T)
    _rel(r["kp"], kp.detach(), "kp")
    _rel(r["heat"], heat.detach(), "heat")
    shifted = R.kp_head_fwd(lg, jm, T, mx=r["stat"][..., 0] + 0.25)
    _rel(shifted["kp"], kp.detach(), "kp for another common maximum")
    if jac:
        _rel(r["jac"], outs[1].detach(), "jac")
    rb = R.kp_head_bwd(lg, jm, T, r["kp"], r.get("jac"), shifted["stat"], dkp, djac if jac else None)
    _rel(rb["dlogits"], grads[0], "dlogits")
    if jac:
        _rel(rb["djm"], grads[1], "djm")


def test_grid_stride_sets_make_a_second_trip():
    assert K.CAP == 4096
    assert K.steps(5 * 10 * 160 * 144) == 2 and K.steps(2 * 11 * 224 * 216) == 2 and K.steps(1032 * 1032) == 2 and K.steps(1024 * 1024) == 1


# ------------------------------------------------------------------------------------------------------------------ the bounds can be met
@pytest.mark.parametrize("B,K_,H,W,ld", K.GAUSS_SETS)
def test_fp32_specification_meets_the_kp_gaussian_bounds(B, K_, H, W, ld):
    test = f"spec kp_gaussian {B}x{K_}x{H}x{W}"
    K.gauss_cases(K.Spec(), B, K_, H, W, ld, test)
    report(test, K.TAG)


@pytest.mark.parametrize("K1", K.SC_K1)
def test_fp32_specification_meets_the_softmax_combine_bounds(K1):
    test = f"spec softmax_combine K1={K1}"
    K.sc_cases(K.Spec(), K1, test)
    if K1 == 2:
        K.run_sc(K.Spec(), K.sc_set(*K.SC_BIG), test)
    report(test, K.TAG)


@pytest.mark.parametrize("B,H,W,K_", K.KH_SETS + [K.KH_BIG])
def test_fp32_specification_meets_the_kp_head_bounds(B, H, W, K_):
    test = f"spec kp_head {B}x{H}x{W}x{K_}"
    if (B, H, W, K_) == K.KH_BIG:
        K.run_kh(K.Spec(), K.kh_set(*K.KH_BIG), test, T=1.0, ldl=3, ldj=6)
    else:
        K.kh_cases(K.Spec(), B, H, W, K_, test)
    report(test, K.TAG)


@pytest.mark.parametrize("B,H,W,K_", [(2, 5, 9, 3), (1, 16, 17, 10)])
def test_fp32_specification_meets_the_kp_head_chain_bounds(B, H, W, K_):
    K.run_kh(K.Spec(), K.kh_set(B, H, W, K_, "peak"), "spec chain kp_head", T=0.1, ldl=K_ + 2, ldj=6, chain=True)


@pytest.mark.parametrize("shape", K.PM_SETS, ids=lambda s: "x".join(map(str, s)))
def test_fp32_specification_meets_the_prior_motion_bounds(shape):
    test = "spec prior_motion " + "x".join(map(str, shape))
    K.pm_cases(K.Spec(), shape, test)
    report(test, K.TAG)


def test_fp32_specification_meets_the_prior_motion_bounds_on_the_other_sets():
    test = "spec prior_motion others"
    K.pm_exact_case(K.Spec(), test)
    K.pm_big_case(K.Spec(), test)
    report(test, K.TAG)


@pytest.mark.parametrize("shape,variant", K.PM_CHAIN, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fp32_specification_meets_the_prior_motion_chain_bounds(shape, variant):
    K.run_chain_pm(K.Spec(), K.pm_set(*shape, **K.PM_VARIANTS[variant]), "spec chain prior_motion")


def stored(S):
    """the reference motions rounded to fp32: what an exact kernel would store"""
    return S.f["motions"].float()


def test_the_kink_holds_at_most_a_thousandth_of_any_set():
    """the reference alone: pixels whose coordinate lies within its counted error of an integer, on every prior_motion set (run_pm_fwd asserts the same on what a
    kernel stored)"""
    worst = 0.0
    sets = [K.pm_set(*shape, **v) for shape in K.PM_SETS for v in K.PM_VARIANTS] + [K.pm_set(*K.PM_BIG, jac=True, bg="near"),
                                                                                  K.pm_set(*K.PM_ODD, jac=False, bg="eye", exact=True)]
    for S in sets:
        share = K.warp_bounds(K.pm_warp(S, stored(S)))["share"]
        worst = max(worst, share)
        assert share <= K.KINK_CAP, (S.B, S.K, S.H, S.W, share)
    print(f"[{K.TAG}] largest kink share over {len(sets)} sets: {worst:.2e}")


# ------------------------------------------------------------------------------------------------------------------ the bounds discriminate
def breaks(mutant, ref, bound):
    """the mutant's output, finite everywhere, leaves the bound at some element"""
    mutant = mutant.reshape(ref.shape)
    assert torch.isfinite(mutant).all()
    return bool(((mutant - ref).abs() > bound.reshape(ref.shape)).any())


PM0 = K.PM_SETS[0]


def pm_mutant(S, wrong, where):
    """(mutant, reference, bound) of one output of the prior_motion pair on the motions an exact kernel would store"""
    mot = stored(S)
    if where in ("motions", "heat"):
        m = R.prior_fwd(S.kd, S.ks, S.jd, S.js, S.bg, S.H, S.W, S.inv_var, wrong=wrong)
        return m[where], S.f[where], S.fb[where]
    wp = K.pm_warp(S, mot)
    wb = K.warp_bounds(wp)
    if where == "warp":
        return K.pm_warp(S, mot, wrong)["val"], wp["val"], wb["val"]
    _, out = K.pm_expect(S, wp, wb)
    if wrong == "grid hw":
        Sm = K.types.SimpleNamespace(**vars(S))
        Sm.f = R.prior_fwd(S.kd, S.ks, S.jd, S.js, S.bg, S.H, S.W, S.inv_var, wrong=wrong)
        _, mut = K.pm_expect(Sm, wp, wb)
    else:
        _, mut = K.pm_expect(S, wp, wb, wrong=wrong)
    return mut[where][0], out[where][0], out[where][1]


@pytest.mark.parametrize("wrong,where,variant", [
    ("grid hw", "motions", 0), ("grid hw", "heat", 0), ("grid hw", "dkd", 0),
    ("warp hw", "dks", 0), ("warp hw", "dbg", 0),
    ("align corners", "warp", 0),
    ("heat sign", "heat", 0),
    ("inv transposed", "motions", 0), ("inv transposed", "motions", 3),
    ("dkd no heat", "dkd", 0), ("dkd no heat", "dkd", 1),
    ("dks no heat", "dks", 0), ("dks no heat", "dks", 1),
    ("clamp border", "warp", 0), ("clamp border", "warp", 1), ("x1 le W", "warp", 0),
    ("dbg no hz", "dbg", 0), ("dbg no hz", "dbg", 2)])
def test_wrong_prior_motion_formulas_break_the_bounds(wrong, where, variant):
    """the 16 x 12 set (K = 10, C = 3) in the variants of the GPU file"""
    S = K.pm_set(*PM0, **K.PM_VARIANTS[variant])
    assert breaks(*pm_mutant(S, wrong, where)), (wrong, where)


@pytest.mark.parametrize("shape", [(2, 10, 7, 5, 12), (3, 10, 64, 48, 16)])
def test_wrong_kp_gaussian_formulas_break_the_bounds(shape):
    S = K.gauss_set(*shape, 0.1)
    B, K_, H, W = shape[:4]
    r = R.kp_gaussian_fwd(S.kp, S.pos, H, W, S.var)
    m = R.kp_gaussian_fwd(S.kp, S.pos, H, W, S.var, wrong="grid hw")
    assert breaks(m["out"], r["out"], K.gauss_fwd_bound(r, 1.0 / S.var, True)), "grid hw: out"
    dout = S.dout.view(B, H, W, K_)
    rb = R.kp_gaussian_bwd(S.kp, dout, H, W, S.var)
    b_dkp, b_dpos = K.gauss_bwd_bounds(S, rb)
    assert breaks(R.kp_gaussian_bwd(S.kp, dout, H, W, S.var, wrong="grid hw")["dkp"], rb["dkp"], b_dkp + K.U * (S.dkp0.double().abs() + (S.dkp0 + rb["dkp"]).abs())), "grid hw: dkp"
    assert breaks(R.kp_gaussian_bwd(S.kp, dout, H, W, S.var, wrong="dpos one b")["dpos"], rb["dpos"], b_dpos), "dpos one b: dpos"


@pytest.mark.parametrize("K1", (2, 11, 32))
def test_softmax_backward_without_the_dot_term_breaks_dlogit(K1):
    S = K.sc_set(K1, 2, 9, 7)
    B, H, W = S.B, S.H, S.W
    mot5 = S.mot.view(B, K1, H, W, 2)
    mask = R.softmax_combine_fwd(S.logit.view(B, H, W, K1), mot5)["mask"].float()
    args = (mot5, mask, S.ddef, S.dmask, S.dnchw)
    r, m = R.softmax_combine_bwd(*args), R.softmax_combine_bwd(*args, wrong="no dot")
    r["dd"] = S.ddef.double()
    ref_l, b_l, _, _ = K.sc_bwd_bounds(r, K1, S.dl0.view(B, H, W, K1), S.dm0.view(B, K1, H, W, 2))
    assert breaks(S.dl0.view(B, H, W, K1).double() + m["dlogit"], ref_l, b_l)


@pytest.mark.parametrize("shape,wrong", [(s, "E no jac") for s in K.KH_SETS] + [(s, "grid hw") for s in K.KH_SETS if s[1] != s[2]])
def test_wrong_kp_head_formulas_break_the_bounds(shape, wrong):
    """(a square image cannot see H and W swapped: the non-square sets are what catches it)"""
    B, H, W, K_ = shape
    S = K.kh_set(*shape)
    T = K.f32(0.1)
    lg4, jm4 = S.logits.view(B, H, W, K_), S.jm.view(B, H, W, 4)
    f = R.kp_head_fwd(lg4, jm4, T)
    f["jm4"] = S.jm.double().view(B, H * W, 1, 4)
    bf = K.kh_fwd_bounds(f, H * W)
    if wrong == "grid hw":
        assert breaks(R.kp_head_fwd(lg4, jm4, T, wrong=wrong)["kp"], f["kp"], bf["kp"]), "grid hw: kp"
    args = (lg4, jm4, T, f["kp"].float(), f["jac"].float(), f["stat"].float(), S.dkp, S.djac)
    r, m = R.kp_head_bwd(*args), R.kp_head_bwd(*args, wrong=wrong)
    r["g"] = f["g"].view(1, H * W, 1, 2)
    ref, bound = K.kh_bwd_bounds(S, r, bf, T, S.dl0.view(B, H, W, K_), S.djm0.view(B, H, W, 4))["dlogits"]
    assert breaks(S.dl0.view(B, H, W, K_).double() + m["dlogits"], ref, bound), f"{wrong}: dlogits"
