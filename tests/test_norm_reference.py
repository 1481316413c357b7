"""tests/ref_norm.py (the float64 reference the kernel tests of csrc/norm.hip compare against) held against ATen in double, and the per-element bounds of
tests/test_norm_kernels_gpu.py held from both sides on every input set of that file, through the same drivers: the fp32 specification of the ABI
(oracle/capi_emulator.py) meets them -- no bound is tighter than fp32 arithmetic allows -- and each of ten deliberately wrong float64 formulas breaks one.
No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import ref_norm as R
from tests import test_norm_kernels_gpu as K
from tests.kernel_check import report

F64 = torch.float64


def _rel(a, b, what, tol=1e-12):
    err = (a - b).abs().max().item()
    scale = max(b.abs().max().item(), 1e-300)
    assert err <= tol * scale, f"{what}: {err:.3e} vs scale {scale:.3e}"


def nchw(t):
    return t.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------ the reference against ATen in double
@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("train,G", [(1, 1), (1, 3), (0, 1)])
def test_reference_equals_aten_in_double(mode, train, G):
    """F.batch_norm (train: one call per statistic group, in group order, on shared running statistics; eval), relu, avg_pool2d, the blend of generator.py:57
    and y = relu(bn(x) + res), forward and through autograd"""
    g = torch.Generator().manual_seed(7)
    N, H, W, C, eps, mom = 6, 4, 6, 5, 1e-5, 0.1
    n = N // G
    pool = mode == "pool"
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    x, gamma, beta, dy = rnd(N, H, W, C) * 2 + 1, rnd(C) + 2, rnd(C), rnd(N, Ho, Wo, C)
    res = rnd(N, H, W, C) if mode == "res" else None
    A, occ = (rnd(N, H, W, C), torch.rand(N, H, W, 1, generator=g, dtype=F64)) if mode == "blend" else (None, None)
    rm0, rv0 = rnd(C), torch.rand(C, generator=g, dtype=F64) + 0.5
    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta)] + [t.clone().requires_grad_(True) for t in (res, A, occ) if t is not None]
    xl, gl, bl = leaves[:3]
    rm, rv = rm0.clone(), rv0.clone()
    parts = [F.batch_norm(nchw(xl[i * n:(i + 1) * n]), rm, rv, gl, bl, bool(train), mom, eps) for i in range(G)]
    v = torch.cat(parts).permute(0, 2, 3, 1)
    if mode == "res":
        v = v + leaves[3]
    v = F.relu(v)
    if pool:
        v = F.avg_pool2d(nchw(v), 2).permute(0, 2, 3, 1)
    if mode == "blend":
        v = leaves[3] * leaves[4] + v * (1 - leaves[4])
    grads = torch.autograd.grad(v, leaves, dy)
    # the reference
    rows = x.reshape(-1, C)
    if train:
        st = torch.stack([torch.cat([s["s1"], s["s2"]]) for s in (R.stats_ref(rows[i * n * H * W:(i + 1) * n * H * W]) for i in range(G))])
        fin = R.finalize_ref(st, n * H * W, gamma, beta, rm0, rv0, mom, eps)
        _rel(fin["rm"][-1], rm, "running_mean")
        _rel(fin["rv"][-1], rv, "running_var")
    else:
        fin = R.finalize_ref(None, 0, gamma, beta, rm0, rv0, mom, eps, train=False)
    f = R.fwd_ref(x, fin["scale"], fin["shift"], 1, pool, res, A, occ)
    _rel(f["y"], v.detach(), "y")
    b1 = R.bwd1_ref(f, dy, fin["mean"], fin["invstd"], 1, pool, G)
    b2 = R.bwd2_ref(f, b1, torch.cat([b1["s1"], b1["s2"]], 1), gamma, fin["invstd"], train, G)
    _rel(b2["dx"], grads[0], "dx")
    _rel(b2["dgamma"], grads[1], "dgamma")
    _rel(b2["dbeta"], grads[2], "dbeta")
    if mode == "res":
        _rel(b1["du"], grads[3], "dres")
    if mode == "blend":
        _rel(b1["dA"], grads[3], "dblend_a")
        _rel(b1["docc"], grads[4], "docc")
    assert (b1["s1"].abs() <= b1["S1"] * (1 + 1e-12)).all() and (b1["s2"].abs() <= b1["S2"] * (1 + 1e-12)).all()


def test_dispatch_mirror():
    """the row counts of the issue's slot cases, from the mirror of pick_rows_per_block: 15 / 16 / 63 / 64 row blocks of 64 rows -> 1 / 8 / 8 / 32 slots; the
    statistics-accuracy set runs 4096 rows per block; the grid-stride sets make a second trip"""
    for rows, rb, slots in ((960, 15, 1), (1024, 16, 8), (4032, 63, 8), (4096, 64, 32)):
        assert K.geometry(rows, 64) == (1, 64, rb) and K.red_slots(rb) == slots
    assert K.geometry(4096, 132) == (3, 64, 64) and K.slot_set(3, 64, 32) == list(range(32))
    assert K.geometry(K.BIG_ROWS, 4)[1] == 4096 and K.geometry(4000, 4)[1] == 64
    assert K.slot_set(1, 15, 1) == [0] and K.slot_set(1, 16, 8) == list(range(8)) and K.slot_set(3, 2, 32) == [0, 1, 2, 3]
    assert K.geometry(216, 64, 3) == (1, 64, 2) and K.geometry(216, 64, 2) == (1, 64, 2)
    assert K.steps(8200 * 512 // 4) == 2 and K.steps(8200 * 129) == 2 and K.steps(8190 * 512 // 4) == 1


# ------------------------------------------------------------------------------------------------------------------ the bounds can be met
@pytest.mark.parametrize("rows,C", K.STAT_SHAPES)
def test_fp32_specification_meets_the_statistics_bounds(rows, C):
    K.run_stats(K.Spec(), K.gen(f"norm/stats/{rows}.{C}", (rows, C), -2, 2), f"spec stats {rows}x{C}")


@pytest.mark.parametrize("ratio", K.STAT_RATIOS)
@pytest.mark.parametrize("rows", [4000, K.BIG_ROWS])
def test_fp32_specification_meets_the_accuracy_bounds(rows, ratio):
    K.run_stats(K.Spec(), K.noise_set(rows, 4, ratio), "spec stats accuracy")


@pytest.mark.parametrize("C,G,count,momentum", K.FIN_CASES)
def test_fp32_specification_meets_the_finalize_bounds(C, G, count, momentum):
    test = f"spec finalize C{C} G{G} n{count} m{momentum}"
    K.finalize_cases(K.Spec(), C, G, count, momentum, test)
    K.clamp_case(K.Spec(), test)
    report(test, K.TAG)


@pytest.mark.parametrize("C,mode,relu,G", K.FWD_CELLS)
def test_fp32_specification_meets_the_forward_bounds(C, mode, relu, G):
    K.run_fwd(K.Spec(), K.bn_set(6, 6, 6, C, mode, G, relu), "spec fwd")


def test_fp32_specification_meets_the_forward_bounds_on_the_other_sets():
    be, test = K.Spec(), "spec fwd others"
    for C in K.SCALAR_C:
        for mode in K.MODES:
            K.run_fwd(be, K.bn_set(2, 4, 6, C, mode), test, expect="scalar")
    for key in K.FWD_ROUTES:
        K.run_fwd(be, K.bn_set(2, 4, 6, 64, "res"), test, lay=K.route(key, 64), expect="scalar")
    for rows, C in ((8200, 512), (8200, 129)):
        K.run_fwd(be, K.bn_set(1, 1, rows, C, "plain", fwd_only=True), test, sample=True)
    report(test, K.TAG)


@pytest.mark.parametrize("C,mode,train", K.BWD_CELLS)
def test_fp32_specification_meets_the_backward_bounds(C, mode, train):
    test = f"spec bwd C{C} {mode} train{train}"
    K.bwd_cell(K.Spec(), C, mode, train, test)
    report(test, K.TAG)


@pytest.mark.parametrize("N,C,slots", K.SLOT_CASES)
def test_fp32_specification_meets_the_slot_case_bounds(N, C, slots):
    K.slot_case(K.Spec(), N, C, slots, "spec slots")


def test_fp32_specification_meets_the_backward_bounds_on_the_other_sets():
    be, test = K.Spec(), "spec bwd others"
    for C in K.RAGGED_C:
        for rows in K.RAGGED_ROWS:
            for mode in ("plain", "res"):
                K.run_bwd(be, K.bn_set(1, 1, rows, C, mode), test, overwrite=rows % 2)
    for C in K.SCALAR_C:
        for mode in K.MODES:
            K.run_bwd(be, K.bn_set(2, 4, 6, C, mode), test, expect="scalar")
    for mode, keys in K.BWD_ROUTES.items():
        for key in keys:
            K.run_bwd(be, K.bn_set(2, 4, 6, 64, mode), test, lay=K.route(key, 64), expect="scalar")
    for H, W in ((2, 6), (6, 2)):
        for C in (64, 37):
            K.run_fwd(be, K.bn_set(3, H, W, C, "pool"), test)
            K.run_bwd(be, K.bn_set(3, H, W, C, "pool"), test)
    for C in (64, 37):
        for mode in K.MODES:
            for train in (1, 0):
                S = K.bn_set(2, 4, 6, C, mode, 1, 1, train, True)
                K.run_fwd(be, S, test)
                K.run_bwd(be, S, test, overwrite=1)
    report(test, K.TAG)


@pytest.mark.parametrize("C,mode,G", K.GROUP_CASES)
def test_fp32_specification_meets_the_group_bounds(C, mode, G):
    K.group_case(K.Spec(), C, mode, G, "spec groups")


@pytest.mark.parametrize("C,mode,G", [(64, "res", 2), (37, "blend", 1), (132, "pool", 3)])
def test_fp32_specification_meets_the_chain_bounds(C, mode, G):
    test = f"spec chain C{C} {mode} G{G}"
    S = K.chain_case(K.Spec(), C, mode, G, test)
    K.run_bwd(K.Spec(), S, test, expect2=K.chain_expect)
    report(test, K.TAG)


def test_the_kink_holds_at_most_one_percent_of_any_set():
    """the reference alone: |u_ref| <= b_u (b_u > 0) on the det_uniform inputs of every backward set (bn_set asserts the same when it builds a set)"""
    worst = 0.0
    sets = [K.bn_set(6, 6, 6, C, mode, G, 1, train) for C in K.FWD_C for mode in K.MODES for G, train in ((1, 1), (1, 0), (2, 1), (3, 1))]
    sets += [K.bn_set(N, 8, 8, C) for N, C, _ in K.SLOT_CASES] + [K.bn_set(1, 1, rows, C, mode) for C in K.RAGGED_C for rows in K.RAGGED_ROWS for mode in ("plain", "res")]
    sets += [K.bn_set(2, 4, 6, C, mode, 1, 1, train, True) for C in (64, 37) for mode in K.MODES for train in (1, 0)]
    for S in sets:
        worst = max(worst, S.kink_share)
        assert S.kink_share <= 0.01
    print(f"[{K.TAG}] largest kink share over {len(sets)} sets: {worst:.2e}")


# ------------------------------------------------------------------------------------------------------------------ the bounds discriminate
def breaks(mutant, ref, bound, mask=None):
    """the mutant's output, finite everywhere, leaves the bound at some (compared) element"""
    mutant = mutant.reshape(ref.shape)
    assert torch.isfinite(mutant).all()
    bad = (mutant - ref).abs() > bound.reshape(ref.shape)
    if mask is not None:
        bad = bad & mask.reshape(ref.shape)
    return bool(bad.any())


def phase2(S, red_world=1, wrong="", red=None):
    """phase 2 (dx overwritten) on the exact sums of phase 1: (reference, bound) or, with `wrong`, the mutant's outputs"""
    exact = torch.cat([S.b1["s1"], S.b1["s2"]], 1) * max(red_world, 1)
    return K.bwd2_expect(S, exact if red is None else red, exact.abs(), 1, red_world, wrong=wrong)


def v4(S, t, pooled=False):
    H, W = (S.H // 2, S.W // 2) if pooled and S.pool else (S.H, S.W)
    return t.view(S.N, H, W, -1)


def phase1_mutant(S, wrong):
    return R.bwd1_ref(S.f, v4(S, S.dy, True), S.mean, S.invstd, S.relu, S.pool, S.G, wrong=wrong)


def test_phase_2_summing_only_slot_0_breaks_dx_and_dgamma():
    """16 row blocks x 64 channels (8 slots filled): dx and dgamma"""
    S = K.bn_set(16, 8, 8, 64)
    exact = torch.cat([S.b1["s1"], S.b1["s2"]], 1)
    slots = K.spread(exact, K.red_slots(S.row_blocks), 11)
    ref, bound = phase2(S, red=slots.sum(1))
    mut, _ = phase2(S, red=slots[:, 0])
    live = ~S.bounds1(1)["kink"]
    assert breaks(mut["dx"], ref["dx"], bound["dx"], live), "slots case N16 C64: dx"
    assert breaks(mut["dgamma"], ref["dgamma"], bound["dgamma"]), "slots case N16 C64: dgamma"


def finalize_mutant(C, G, count, momentum, wrong):
    st, gamma, beta, rm, rv = K.fin_set(C, G, count)
    mom = K.f32(momentum)
    r = R.finalize_ref(st.sum(1), count, gamma, beta, rm, rv, mom, K.EPS)
    return r, K.fin_bounds(r, count, gamma, mom), R.finalize_ref(st.sum(1), count, gamma, beta, rm, rv, mom, K.EPS, wrong=wrong)


def test_biased_running_var_breaks_running_var():
    """finalize C64 G1 count 4096 momentum 0.1: running_var"""
    r, b, m = finalize_mutant(64, 1, 4096, 0.1, "biased running_var")
    assert breaks(m["rv"][-1:], r["rv"][-1:], b["rv"])
    assert not breaks(m["rm"][-1:], r["rm"][-1:], b["rm"])


def test_momentum_updates_in_reverse_group_order_break_the_running_statistics():
    """finalize C257 G3 count 108 momentum 0.25: running_mean and running_var"""
    r, b, m = finalize_mutant(257, 3, 108, 0.25, "reverse group order")
    assert breaks(m["rm"][-1:], r["rm"][-1:], b["rm"]) and breaks(m["rv"][-1:], r["rv"][-1:], b["rv"])


@pytest.mark.parametrize("C", (64, 37))
def test_relu_gradient_1_at_0_breaks_dres_and_red(C):
    """the planted-zeros set (residual, train): dres at the planted elements, and sum du"""
    S = K.bn_set(2, 4, 6, C, "res", 1, 1, 1, True)
    b, m = S.bounds1(1), phase1_mutant(S, "relu'(0) = 1")
    assert breaks(S.dres0.view_as(m["du"]).double() + m["du"], S.dres0.view_as(m["du"]).double() + S.b1["du"], b["dres"], ~b["kink"]), "zeros res: dres"
    assert breaks(m["s1"], S.b1["s1"], b["red1"]), "zeros res: red (sum du)"


@pytest.mark.parametrize("C", (64, 37))
def test_pool_gradient_without_the_quarter_breaks_red(C):
    """the pool cell (6 x 6 x 6, train): both halves of red"""
    S = K.bn_set(6, 6, 6, C, "pool", 1, 1, 1)
    b, m = S.bounds1(16), phase1_mutant(S, "pool without 0.25")
    assert breaks(m["s1"], S.b1["s1"], b["red1"]) and breaks(m["s2"], S.b1["s2"], b["red2"])


@pytest.mark.parametrize("C", (64, 37))
def test_docc_without_the_activation_term_breaks_docc(C):
    """the blend cell (6 x 6 x 6, train): docc"""
    S = K.bn_set(6, 6, 6, C, "blend", 1, 1, 1)
    b, m = S.bounds1(16), phase1_mutant(S, "docc without -a")
    old = S.docc0.view_as(m["docc"]).double()
    assert breaks(old + m["docc"], old + S.b1["docc"], b["docc"])


@pytest.mark.parametrize("wrong,G,red_world,key", [("dx without xhat k2", 1, 1, "dx"), ("means over all rows", 2, 1, "dx"), ("red_world ignored", 1, 3, "dx"),
                                                   ("dgamma once per group run", 2, 1, "dgamma"), ("dgamma once per group run", 3, 1, "dbeta")])
@pytest.mark.parametrize("C,mode", [(64, "plain"), (37, "res"), (64, "pool"), (37, "blend")])
def test_wrong_phase_2_formulas_break_the_bounds(C, mode, wrong, G, red_world, key):
    """the cell / group sets (6 x 6 x 6): the output named by `key`"""
    S = K.bn_set(6, 6, 6, C, mode, G, 1, 1)
    ref, bound = phase2(S, red_world)
    mut, _ = phase2(S, red_world, wrong)
    assert breaks(mut[key], ref[key], bound[key], ~S.bounds1(1)["kink"] if key == "dx" else None), (wrong, key)
