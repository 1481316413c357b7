"""Is tests/ref_equiv.py -- the fp64 reference of every equivariance test -- right?  Held against mrfa_amd.losses.Transform and the torch expressions of
GeneratorFullLoss run in float64 on the CPU (the double backward included), and against the reference's own run in tests/golden/losses.npz."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mrfa_amd.equivariance  # noqa: F401  (the feature these references serve)
from mrfa_amd.losses import Transform, _inv2x2
from mrfa_amd.modules.util import make_coordinate_grid
from tests import cases
from tests import ref_equiv as R

W_E, W_J = 10.0, 10.0


def _draw(B, K, seed, tps=True, on_lines=True):
    """a float64 Transform and the four keypoint tensors; with on_lines some keypoints lie exactly on control rows / columns and one on a control point"""
    gen = torch.Generator().manual_seed(seed)
    kw = dict(sigma_affine=0.05, sigma_tps=0.005, points_tps=5) if tps else dict(sigma_affine=0.05)
    t = Transform(B, generator=gen, **kw)
    t.theta = t.theta.double()
    if tps:
        t.control_points, t.control_params = t.control_points.double(), t.control_params.double()
    kp_t = torch.rand(B, K, 2, generator=gen, dtype=torch.float64) * 1.8 - 0.9
    if on_lines and K >= 3:
        kp_t[0, 0] = torch.tensor([0.5, -0.5])          # a control point of the 5 x 5 grid
        kp_t[0, 1, 0] = 0.0                             # a control column
        kp_t[-1, 2, 1] = -1.0                           # a control row
    kp_d = torch.rand(B, K, 2, generator=gen, dtype=torch.float64) * 1.8 - 0.9
    jac_t = torch.eye(2, dtype=torch.float64) + 0.3 * torch.randn(B, K, 2, 2, generator=gen, dtype=torch.float64)
    jac_d = torch.eye(2, dtype=torch.float64) + 0.3 * torch.randn(B, K, 2, 2, generator=gen, dtype=torch.float64)
    return t, kp_d, jac_d, kp_t, jac_t


def _np(t):
    th = t.theta.numpy()
    return (th, t.control_points.numpy().reshape(-1, 2), t.control_params.numpy().reshape(th.shape[0], -1)) if t.tps else (th, None, None)


def _torch_terms(t, kp_d, jac_d, kp_t, jac_t):
    value = W_E * torch.abs(kp_d - t.warp_coordinates(kp_t)).mean()
    v = torch.matmul(_inv2x2(jac_d), torch.matmul(t.jacobian(kp_t), jac_t))
    return value, W_J * torch.abs(torch.eye(2, dtype=v.dtype).view(1, 1, 2, 2) - v)


@pytest.mark.parametrize("B,K,tps", [(2, 10, True), (1, 3, True), (2, 10, False)])
def test_forward_and_all_four_gradients_match_the_double_backward(B, K, tps):
    t, kp_d, jac_d, kp_t, jac_t = _draw(B, K, seed=3 + B, tps=tps)
    leaves = [x.requires_grad_(True) for x in (kp_d, jac_d, kp_t, jac_t)]
    value, term = _torch_terms(t, *leaves)
    gen = torch.Generator().manual_seed(11)
    g_value, g_term = 0.7, torch.randn(B, K, 2, 2, generator=gen, dtype=torch.float64)
    (g_value * value + (g_term * term).sum()).backward()
    th, q, c = _np(t)
    a = [x.detach().numpy() for x in leaves]
    fwd = R.loss_fwd(a[0], a[1], a[2], a[3], th, q, c, W_E, W_J)
    assert abs(fwd["value"].v - value.item()) <= 1e-12
    assert np.abs(fwd["term"].v - term.detach().numpy()).max() <= 1e-12
    assert np.abs(R.warp_points(th, q, c, a[2]).v - t.warp_coordinates(kp_t).detach().numpy()).max() <= 1e-12
    assert np.abs(R.jacobian(th, q, c, a[2]).v - t.jacobian(kp_t).detach().numpy()).max() <= 1e-12
    bwd = R.loss_bwd(a[0], a[1], a[2], a[3], th, q, c, W_E, W_J, g_value, g_term.numpy())
    for name, leaf in zip(("d_kp_d", "d_jac_d", "d_kp_t", "d_jac_t"), leaves):
        assert np.abs(bwd[name].v - leaf.grad.numpy()).max() <= 1e-12, name
    # without the Jacobian term: the value's gradients alone
    for x in leaves:
        x.grad = None
    (g_value * _torch_terms(t, *leaves)[0]).backward()
    bwd = R.loss_bwd(a[0], None, a[2], None, th, q, c, W_E, 0.0, g_value, None)
    assert bwd["d_jac_d"] is None and bwd["d_jac_t"] is None
    assert np.abs(bwd["d_kp_d"].v - leaves[0].grad.numpy()).max() <= 1e-12 and np.abs(bwd["d_kp_t"].v - leaves[2].grad.numpy()).max() <= 1e-12


def test_magnitudes_dominate_values_and_depths_are_what_the_formulas_say():
    t, kp_d, jac_d, kp_t, jac_t = _draw(2, 10, seed=5)
    th, q, c = _np(t)
    a = [x.numpy() for x in (kp_d, jac_d, kp_t, jac_t)]
    u = R.tps_sums(a[2][..., 0], a[2][..., 1], q, c[:, None, :])
    for k, vm in u.items():
        assert (vm.m >= np.abs(vm.v)).all(), k
    # U:   dx (1) -> d (2) -> d + eps (3) -> log (5) -> d d log (6) -> c U (7) -> 25 terms in any order (31)
    # U':  2 d log (6) + d d / de (4) -> (7) -> c U' (8) -> times the sign (9) -> (33)
    # U'': q = d / de (4);  2 log (6) + 4 q (5) -> (7) - q q (5) -> (8) -> c U'' (9) -> times sx sx (10) -> (34)
    assert (u["s"].n, u["gx"].n, u["hxx"].n) == (7 + 24, 9 + 24, 10 + 24)
    fwd = R.loss_fwd(*a, th, q, c, W_E, W_J)
    bwd = R.loss_bwd(*a, th, q, c, W_E, W_J, 1.0, np.ones((2, 10, 2, 2)))
    for vm in (fwd["value"], fwd["term"], bwd["d_kp_d"], bwd["d_kp_t"], bwd["d_jac_d"], bwd["d_jac_t"]):
        assert (vm.m >= np.abs(vm.v) * (1 - 1e-12)).all() and 0 < vm.n < 120
    # the points on control rows and columns have exact zero distances and signs
    assert u["s"].v.shape == (2, 10) and np.isfinite(bwd["d_kp_t"].v).all()


def test_against_the_references_own_run(golden_dir):
    """theta, control_points, control_params and the three recorded results of tests/golden/losses.npz, at the tolerances tests/test_losses.py:59-61 applies to
    the oracle"""
    g = dict(np.load(os.path.join(golden_dir, "losses.npz")))
    th, q, c = g["theta"], g["control_points"].reshape(-1, 2), g["control_params"].reshape(1, -1)
    kq = cases.keypoints("g7/kq", 1)
    assert np.abs(R.warp_points(th, q, c, kq["kp"].numpy()).v - g["warp_kp"]).max() <= 1e-6
    assert np.abs(R.jacobian(th, q, c, kq["kp"].numpy()).v - g["warp_jac"]).max() <= 1e-5
    real = cases.images("g7/real", 1, 256)
    out, bound = R.warp_frame(real.numpy(), th, q, c)
    assert np.abs(out[:, :, ::4, ::4] - g["warp_frame_s4"]).max() <= 1e-5
    assert (bound > 0).all() and bound.max() < 1e-3


@pytest.mark.parametrize("sigma_affine", [0.05, 1.0])
def test_frame_warp_is_grid_sample_with_reflection(sigma_affine):
    """against Transform.warp_coordinates + F.grid_sample(padding_mode="reflection") in float64, on the float64 grid"""
    gen = torch.Generator().manual_seed(7)
    N, Cc, H, W = 2, 3, 9, 13
    t = Transform(N, generator=gen, sigma_affine=sigma_affine, sigma_tps=0.005, points_tps=5)
    t.theta, t.control_points, t.control_params = t.theta.double(), t.control_points.double(), t.control_params.double()
    img = torch.rand(N, Cc, H, W, generator=gen, dtype=torch.float64)
    grid = t.warp_coordinates(make_coordinate_grid((H, W), img).reshape(1, H * W, 2)).view(N, H, W, 2)
    want = F.grid_sample(img, grid, padding_mode="reflection", align_corners=False)
    out, _ = R.warp_frame(img.numpy(), *_np(t), grid_dtype=np.float64)
    assert np.abs(out - want.numpy()).max() <= 1e-12
    assert np.array_equal(R.coordinate_grid(H, W), make_coordinate_grid((H, W), torch.zeros(1)).numpy())
