"""tests/ref_sample.py (the float64 reference the kernel tests of csrc/sample.hip compare against) held against ATen in double on generic coordinates, and
against hand-written values on the deliberate ones (integers, borders, non-finite).  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from oracle.capi_emulator import Emulator
from tests import ref_sample as R
from tests.sample_grids import FLOWS, flow_grid, gs_grid

F64 = torch.float64


def _rel(a, b, what, tol=1e-12):
    err = (a - b).abs().max().item()
    scale = max(b.abs().max().item(), 1e-300)
    assert err <= tol * scale, f"{what}: {err:.3e} vs scale {scale:.3e}"


def _generic_grid(N, Ho, Wo, mode, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N, Ho, Wo, 2, generator=g) * 2.6 - 1.3) if mode == 0 else (torch.rand(N, Ho, Wo, 2, generator=g) * 10 - 5)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("in_rep", [1, 3])
def test_grid_sample_reference_equals_aten_in_double(mode, in_rep):
    Nin, Hi, Wi, Ho, Wo, Cc = 2, 9, 7, 6, 13, 5
    N = Nin * in_rep
    g = torch.Generator().manual_seed(11 + mode)
    x = torch.randn(Nin, Hi, Wi, Cc, generator=g, dtype=F64)
    dout = torch.randn(N, Ho, Wo, Cc, generator=g, dtype=F64)
    grid = _generic_grid(N, Ho, Wo, mode, 3)
    out = R.grid_sample_ref(x, grid, mode, in_rep)
    din, dgrid = R.grid_sample_grads_ref(x, grid, dout, mode, in_rep)
    xl = x.clone().requires_grad_(True)
    gl = grid.to(F64).requires_grad_(True)
    if mode == 0:
        gn, ac = gl, False
    else:                                                                       # pixel flow on the identity grid == align_corners=True on 2 p / (size - 1) - 1
        xs = torch.arange(Wo, dtype=F64).view(1, 1, Wo)
        ys = torch.arange(Ho, dtype=F64).view(1, Ho, 1)
        gn, ac = torch.stack([2 * (gl[..., 0] + xs) / (Wi - 1) - 1, 2 * (gl[..., 1] + ys) / (Hi - 1) - 1], dim=-1), True
    y = F.grid_sample(xl.permute(0, 3, 1, 2).repeat_interleave(in_rep, dim=0), gn, mode="bilinear", padding_mode="zeros", align_corners=ac)
    gx, gg = torch.autograd.grad(y, [xl, gl], dout.permute(0, 3, 1, 2))
    _rel(out, y.permute(0, 2, 3, 1).detach(), "out")
    _rel(din, gx, "din")
    _rel(dgrid, gg, "dgrid")
    r = R.grid_sample_grads_ref(x, grid, dout, mode, in_rep, full=True)
    assert (r["out"].abs() <= r["S_out"] + 1e-300).all() and (r["S_out"] <= r["tap_wide"] * (1 + 1e-15)).all()
    assert (r["din"].abs() <= r["S_din"] * (1 + 1e-12)).all() and r["k_din"].sum().item() == sum(
        ((r["x0"] + dx >= 0) & (r["x0"] + dx < Wi) & (r["y0"] + dy >= 0) & (r["y0"] + dy < Hi) & r["live"]).sum().item() for dx in (0, 1) for dy in (0, 1))
    assert (r["gx"].abs() <= r["S_gx"] * (1 + 1e-12)).all() and (r["S_gx"] <= r["T"] * (1 + 1e-12)).all()


@pytest.mark.parametrize("shape", [(7, 5, 50, 64, 3), (50, 64, 7, 5, 2), (8, 24, 16, 9, 1), (1, 9, 9, 1, 2), (6, 6, 6, 6, 2), (64, 64, 256, 256, 1)])
def test_resize_reference_equals_aten_in_double(shape):
    Hi, Wi, Ho, Wo, Cc = shape
    N = 2
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, Hi, Wi, Cc, generator=g, dtype=F64)
    dout = torch.randn(N, Ho, Wo, Cc, generator=g, dtype=F64)
    acc = torch.randn(N, Ho, Wo, Cc, generator=g, dtype=F64)
    xl = x.clone().requires_grad_(True)
    y = F.interpolate(xl.permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=True)
    (gx,) = torch.autograd.grad(y, xl, dout.permute(0, 3, 1, 2) * 0.5)
    _rel(R.resize_ref(x, Ho, Wo), y.permute(0, 2, 3, 1).detach(), "out")
    _rel(R.resize_ref(x, Ho, Wo, 2.0, acc), y.permute(0, 2, 3, 1).detach() * 2 + acc, "out (mul, acc)")
    _rel(R.resize_grads_ref(x.shape, dout, 0.5), gx, "din")
    x32 = x.float()                                                              # the adjoint identity the GPU test checks on device results
    _rel((R.resize_ref(x32, Ho, Wo) * dout).sum(), (x32.double() * R.resize_grads_ref(x.shape, dout)).sum(), "adjoint", tol=1e-11)


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_corr_lookup_reference_equals_the_corrblock_formulation_in_double(radius):
    Q, Hs, Ws = 40, 8, 24
    g = torch.Generator().manual_seed(7)
    v0 = torch.randn(Q, Hs, Ws, generator=g, dtype=F64)
    v1 = torch.randn(Q, Hs // 2, Ws // 2, generator=g, dtype=F64)
    coords = torch.rand(Q, 2, generator=g) * torch.tensor([Ws + 8.0, Hs + 8.0]) - 4
    nwin = (2 * radius + 1) ** 2
    dout = torch.randn(Q, 2 * nwin, generator=g, dtype=F64)
    a, b, c = v0.clone().requires_grad_(True), v1.clone().requires_grad_(True), coords.to(F64).requires_grad_(True)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64)                                                 # (_lookup builds its window offsets in the default dtype)
    try:
        y = Emulator._lookup(a[:, None], b[:, None], c, radius)
    finally:
        torch.set_default_dtype(prev)
    g0, g1, gc = torch.autograd.grad(y, [a, b, c], dout)
    _rel(R.corr_lookup_ref(v0, v1, coords, radius), y.detach(), "out")
    d0, d1, dc = R.corr_lookup_grads_ref(v0, v1, coords, dout, radius)
    _rel(d0, g0, "dvol0")
    _rel(d1, g1, "dvol1")
    _rel(dc, gc, "dcoords")


# ------------------------------------------------------------------------------------------------------------------ deliberate coordinates, by hand
def _at(x, pts, mode=1):
    """sample the one-image map x [H, W] at pixel coordinates pts (mode 1 with Ho = 1, flows relative to ox)"""
    H, W = x.shape
    grid = torch.tensor([[px - i, py] for i, (px, py) in enumerate(pts)], dtype=torch.float32).view(1, 1, len(pts), 2)
    dout = torch.ones(1, 1, len(pts), 1, dtype=F64)
    r = R.grid_sample_grads_ref(x.view(1, H, W, 1), grid, dout, 1, full=True)
    return r["out"].view(-1), r["din"].view(H, W), r["dgrid"].view(-1, 2), r


def test_reference_on_integer_border_and_non_finite_coordinates():
    x = torch.tensor([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]], dtype=F64)            # H = 2, W = 3
    nan, inf = float("nan"), float("inf")
    pts = [(0.0, 0.0), (2.0, 1.0), (1.0, 0.5), (-1.0, 0.0), (3.0, 0.0), (0.0, 2.0), (0.0, -1.0), (nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, -inf), (1e30, 0.0),
           (-0.5, 0.0), (2.5, 1.0), (1.0, -0.25), (0.5, 1.75), (2.0, 0.0)]
    out, din, dgrid, r = _at(x, pts)
    exp = [1.0, 32.0, 9.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 16.0, 1.5, 3.0, 4.0]
    assert torch.equal(out, torch.tensor(exp, dtype=F64))
    dead = [3, 4, 5, 6, 7, 8, 9, 10, 11]
    assert not r["live"][dead].any() and r["live"][[0, 1, 2, 12, 13, 14, 15, 16]].all()
    assert (dgrid[dead] == 0).all() and torch.isinf(r["dist_x"][dead]).all()
    # one-sided derivatives at integers (cell [x0, x0 + 1)): (0, 0): d/dx = x[0,1] - x[0,0] = 1, d/dy = x[1,0] - x[0,0] = 7
    assert dgrid[0].tolist() == [1.0, 7.0]
    # (2, 1) = (W - 1, H - 1): the right and lower taps do not exist (value 0): d/dx = 0 - 32, d/dy = 0 - 32
    assert dgrid[1].tolist() == [-32.0, -32.0]
    # (1, 0.5): d/dx = .5 (4 - 2) + .5 (32 - 16) = 9, d/dy = 16 - 2 = 14
    assert dgrid[2].tolist() == [9.0, 14.0]
    # (-0.5, 0): left tap missing: out = .5 * 1, d/dx = 1 - 0 = 1, d/dy = .5 (8 - 1) = 3.5 (the missing taps count as 0 on both rows)
    assert dgrid[12].tolist() == [1.0, 3.5]
    # (2, 0): weight 1 on the last column, nothing beyond
    assert dgrid[16].tolist() == [-4.0, 28.0]
    # din: weights of the live points only; the dead ones scatter nothing
    w = torch.tensor([[1 + 0.5, 0.5 + 0.75, 1.0],                               # (0,0) + (-.5,0) | (1,.5) + (1,-.25) | (2,0)
                      [0.125, 0.5 + 0.125, 1 + 0.5]], dtype=F64)                # (.5,1.75) | (1,.5) + (.5,1.75) | (2,1) + (2.5,1)
    assert torch.allclose(din, w, rtol=0, atol=1e-15)
    assert r["dist_x"][[0, 1, 2, 16]].tolist() == [0.0, 0.0, 0.0, 0.0] and r["dist_x"][12].item() == 0.5 and r["dist_y"][15].item() == 0.25


def test_reference_identity_flow_returns_the_input_exactly():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 8, 16, 3, generator=g)
    for mode in (0, 1):
        grid = flow_grid("identity", 2, 8, 16, 8, 16, mode).view(2, 8, 16, 2)
        assert torch.equal(R.grid_sample_ref(x, grid, mode), x.double()), mode
        r = R.grid_sample_ref(x, grid, mode, full=True)
        assert (r["dist_x"] == 0).all() and (r["dist_y"] == 0).all()


def test_flow_grids_are_the_same_pixel_coordinates_in_both_modes():
    N, Ho, Wo, Hi, Wi = 2, 6, 21, 8, 32
    for kind in FLOWS:
        c0 = R.gs_coords(flow_grid(kind, N, Ho, Wo, Hi, Wi, 0).view(N, Ho, Wo, 2), 0, Hi, Wi)
        c1 = R.gs_coords(flow_grid(kind, N, Ho, Wo, Hi, Wi, 1).view(N, Ho, Wo, 2), 1, Hi, Wi)
        assert torch.equal(c0[0], c1[0]) and torch.equal(c0[1], c1[1]), kind          # power-of-two sizes: exact in fp32 in either convention
    ix = R.gs_coords(flow_grid("sinus", N, Ho, Wo, Hi, Wi, 1).view(N, Ho, Wo, 2), 1, Hi, Wi)[0].view(N, Ho, Wo)
    live = (ix > -1) & (ix < Wi)
    flips = (live[..., 1:8] != live[..., :7]).sum(-1)                             # inside the first run of eight
    assert (flips >= 2).any() and (~live).any() and live.any()


def test_share_of_near_integer_coordinates_on_a_random_grid():
    """the kernel tests leave d grid elements out where a coordinate lies within its fp32 evaluation error of an integer; on uniform fp32 coordinates of the
    sizes used there that is ~1e-5 of them (the error is ~2^-22 of a unit-spaced lattice, two coordinates per point)"""
    for mode, Hi, Wi in ((0, 64, 64), (1, 64, 64), (1, 256, 256)):
        grid = _generic_grid(4, 256, 256, mode, 9)
        x = torch.zeros(1, Hi, Wi, 1, dtype=F64)
        r = R.grid_sample_ref(x, grid, mode, in_rep=4, full=True)
        ix, iy, dx, dy = R.gs_coords(grid, mode, Hi, Wi)
        near = r["live"] & ((r["dist_x"] <= dx) | (r["dist_y"] <= dy))
        share = near.double().mean().item()
        print(f"[ref] near-integer share mode {mode} {Hi}x{Wi}: {share:.2e}")
        assert share <= 1e-4


def test_gs_grid_special_rows():
    for mode in (0, 1):
        N, Ho, Wo, Hi, Wi = 1, 11, 13, 9, 7
        grid, outside = gs_grid(N, Ho, Wo, Hi, Wi, mode, seed=1)
        r = R.grid_sample_ref(torch.ones(1, Hi, Wi, 1), grid.view(N, Ho, Wo, 2), mode, full=True)
        assert not r["live"][outside].any() and (r["out"][outside] == 0).all()
