"""Clip metrics on the GPU (-m gpu): mrfa_frame_metrics against float64 on the same fp32 numbers with bounds counted from the kernel's own roundings in
its own order, on shapes placed on the tile seams; identical frames, repeatability, canaries, the specification; and reconstruction(metrics="device") on the
dry model, eager and captured."""
import numpy as np
import pytest
import torch

from mrfa_amd import engine, hip
from mrfa_amd.utils.prng import det_uniform
from oracle.capi_emulator import Emulator
from oracle.infer_spec import C1, C2, _window, gauss_window

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
CANARY = -1234.5
PAD = 64                   # canary words on either side of the output and of the workspace
TH, TW = engine.METRICS_TILE
SECOND_ORDER = 1.1         # products of two first-order terms
CHAIN = 16                 # the longest chain of fp32 additions behind a workgroup's partial sum: 7 in a thread, 6 shuffle steps, 3 across the waves
CAP = 2e-5                 # the frame bound of the three gate families may not exceed this at any shape (a seam mistake moves a frame by >= 1e-3)

# (N, C, H, W): one window; one row of windows; the valid region exactly one tile; one over and one under; several partial tiles with odd W
SSIM_SHAPES = [(1, 1, 11, 11), (3, 3, 11, 40), (1, 4, TH + 10, TW + 10), (3, 1, TH + 11, TW + 9), (1, 3, 2 * TH + 13, TW + 21)]
ILL_SHAPE = SSIM_SHAPES[-1]
FAMILIES = ("random", "near", "flipped")


def _draw(family, shape):
    tag = f"metricsgpu/{shape}"
    p = det_uniform(tag + "/p", shape, 0, 1)
    if family == "random":
        return p, det_uniform(tag + "/t", shape, 0, 1)
    if family == "near":
        return p, (p + 0.02 * det_uniform(tag + "/n", shape, -1, 1)).clamp(0, 1)
    if family == "flipped":
        return p, 1 - p
    if family == "identical":
        return p, p.clone()
    if family == "flat":                                       # near-constant: 0.9 +- 5e-4, the variances are all rounding-sized beside the means
        return 0.9 + 5e-4 * det_uniform(tag + "/f1", shape, -1, 1), 0.9 + 5e-4 * det_uniform(tag + "/f2", shape, -1, 1)
    if family == "black":                                      # black against 0.01 noise: both constants of S matter
        return torch.zeros(shape), 0.01 * det_uniform(tag + "/b", shape, 0, 1)
    raise KeyError(family)


def reference(p: torch.Tensor, t: torch.Tensor, want_ssim=True):
    """float64 on the fp32 numbers -> (rows (N,4), bounds (N,4)) of the kernel's error on them, as test_kernel_against_float64's docstring counts them"""
    x, y = p.double().numpy(), t.double().numpy()
    N = x.shape[0]
    rows, bound = np.zeros((N, 4)), np.zeros((N, 4))
    d = x - y
    rows[:, 0], rows[:, 1] = np.abs(d).mean(axis=(1, 2, 3)), (d * d).mean(axis=(1, 2, 3))
    bound[:, 0] = SECOND_ORDER * (1 + CHAIN + 1) * U * rows[:, 0]
    bound[:, 1] = SECOND_ORDER * (2 + 1 + CHAIN + 1) * U * rows[:, 1]
    if not want_ssim:
        return rows, bound
    g = gauss_window()
    e = abs(1.0 - g.sum())                                     # the eleven fp32 weights do not add up to 1 exactly
    a, b = x - 0.5, y - 0.5
    w = lambda v: _window(v, g)
    ma, mb = w(a), w(b)
    n1, n2 = (11 + 11 + 3) * U, (11 + 11 + 5) * U
    d_ma, d_mb = n1 * w(np.abs(a)), n1 * w(np.abs(b))
    d_maa, d_mbb, d_mab = n2 * w(a * a), n2 * w(b * b), n2 * w(np.abs(a * b))
    # the specification's quantities, on x and y themselves
    mx, my = w(x), w(y)
    sxx, syy, sxy = w(x * x) - mx * mx, w(y * y) - my * my, w(x * y) - mx * my
    d_mx, d_my = d_ma + U * np.abs(mx) + 0.5 * e, d_mb + U * np.abs(my) + 0.5 * e
    d_sxx = d_maa + 2 * np.abs(ma) * d_ma + U * ma * ma + U * np.abs(sxx) + (np.abs(ma) + 0.25) * e
    d_syy = d_mbb + 2 * np.abs(mb) * d_mb + U * mb * mb + U * np.abs(syy) + (np.abs(mb) + 0.25) * e
    d_sxy = d_mab + np.abs(ma) * d_mb + np.abs(mb) * d_ma + U * np.abs(ma * mb) + U * np.abs(sxy) + (0.5 * np.abs(ma) + 0.5 * np.abs(mb) + 0.25) * e
    A1, A2 = 2 * mx * my + C1, 2 * sxy + C2
    B1, B2 = mx * mx + my * my + C1, sxx + syy + C2
    d_A1 = 2 * (np.abs(mx) * d_my + np.abs(my) * d_mx) + U * C1 + 2 * U * (2 * np.abs(mx * my) + C1)
    d_A2 = 2 * d_sxy + U * C2 + U * (2 * np.abs(sxy) + C2)
    d_B1 = 2 * np.abs(mx) * d_mx + 2 * np.abs(my) * d_my + U * C1 + 4 * U * B1
    d_B2 = d_sxx + d_syy + U * C2 + 2 * U * (np.abs(sxx) + np.abs(syy) + C2)
    S = A1 * A2 / (B1 * B2)
    d_S = (np.abs(A2) * d_A1 + np.abs(A1) * d_A2) / (B1 * B2) + np.abs(S) * (d_B1 / B1 + d_B2 / B2) + 4 * U * np.abs(S)
    rows[:, 2] = S.mean(axis=(1, 2, 3))
    bound[:, 2] = SECOND_ORDER * (d_S.mean(axis=(1, 2, 3)) + CHAIN * U * np.abs(S).mean(axis=(1, 2, 3)) + U * np.abs(rows[:, 2]))
    return rows, bound


def _guarded(n, dtype):
    buf = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def _launch(dp, dt, want_ssim=1, check=True):
    """one call on device tensors, out and the workspace inside canary words -> rows (N,4) on the CPU"""
    N, C, H, W = dp.shape
    L = hip.lib()
    need = L.mrfa_frame_metrics_workspace(N, C, H, W)
    assert need == N * C * -(-H // TH) * -(-W // TW) * 24
    obuf, out = _guarded(4 * N, torch.float32)
    wbuf, ws = _guarded(need // 8, torch.float64)
    hip.check(L.mrfa_frame_metrics(hip.stream_ptr(), dp.data_ptr(), dt.data_ptr(), N, C, H, W, want_ssim, ws.data_ptr(), need, out.data_ptr()),
              "mrfa_frame_metrics")
    torch.cuda.synchronize()
    for buf, n in ((obuf, 4 * N), (wbuf, need // 8)):
        assert bool((buf[:PAD] == CANARY).all() and (buf[PAD + n:] == CANARY).all()), "wrote outside its output or its workspace"
    assert not bool((out == CANARY).any()) and not bool((ws == CANARY).any())
    return out.cpu().view(N, 4)


_CACHE = {}


def _case(family, shape, want_ssim=True):
    """inputs, float64 rows and bounds of one case, computed once"""
    key = (family, shape, want_ssim)
    if key not in _CACHE:
        p, t = _draw(family, shape)
        _CACHE[key] = (p, t) + reference(p, t, want_ssim)
    return _CACHE[key]


def _check(family, shape, want_ssim=True):
    p, t, rows64, bound = _case(family, shape, want_ssim)
    dp, dt = p.to(DEV), t.to(DEV)
    got = _launch(dp, dt, int(want_ssim))
    again = _launch(dp, dt, int(want_ssim))
    assert torch.equal(got, again), "two runs differ"
    assert torch.equal(dp.cpu(), p) and torch.equal(dt.cpu(), t), "inputs must not be written"
    err = np.abs(got.double().numpy() - rows64)
    ratio = err[:, :3] / np.maximum(bound[:, :3], 1e-300)
    print(f"[metrics] {family} {shape} ssim={want_ssim}: l1 {rows64[:, 0].max():.4f} err/bound {ratio[:, 0].max():.3f}, mse err/bound {ratio[:, 1].max():.3f}, "
          f"ssim {rows64[:, 2].tolist()} bound {bound[:, 2].max():.2e} err/bound {ratio[:, 2].max():.3f}")
    assert torch.isfinite(got).all() and (got[:, 3] == 0).all()
    assert (err <= bound).all(), (err, bound)
    if not want_ssim:
        assert (got[:, 2] == 0).all()
    # the specification on the same numbers: float64, then ITS one rounding
    spec = torch.full((p.shape[0], 4), CANARY)
    ws = torch.zeros(max(Emulator().mrfa_frame_metrics_workspace(*shape) // 8, 1), dtype=torch.float64)
    assert Emulator().mrfa_frame_metrics(0, p.data_ptr(), t.data_ptr(), *shape, int(want_ssim), ws.data_ptr(), ws.numel() * 8, spec.data_ptr()) == 0
    assert (np.abs((got.double() - spec.double()).numpy()) <= bound + U * np.abs(rows64)).all()
    return got, rows64, bound


@pytest.mark.parametrize("shape", SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64(shape):
    """u = 2^-24; the inputs are fp32 numbers in [0, 1], the expected values float64 on the same numbers (oracle/infer_spec.py's window sums with the
    eleven fp32 weights in float64).  The kernel's roundings in its own order, first order in u; a multiplication and an addition contracted into one fused
    operation removes a rounding and never adds one.  Nothing is measured from the kernel.

    L1 and MSE: d = fl(p - t), one rounding (|d| is exact); d^2 carries it twice and is rounded once more.  A workgroup's sum passes every term through at
    most CHAIN = 16 fp32 additions (7 in a thread: the first one onto 0 is exact; 6 shuffle steps; 3 across the four waves); all terms are >= 0, so that
    is 16 u of the sum.  The partials are added and divided in float64 (2^-53 per operation: nothing beside u) and rounded once.
      l1: (1 + 16 + 1) u = 18 u relative;  mse: (2 + 1 + 16 + 1) u = 20 u relative;  x 1.1 for second order: 1.3e-6 <= 1e-5, asserted below.
    SSIM, per window, with a = x - 0.5, b = y - 0.5 and W(.) the window average: a = fl(x - 0.5) is one rounding.  First moments: fl(g a) once, 11
    additions in the horizontal pass; fl(g h) and 11 additions in the vertical pass -> (1 + 12 + 12) u W|a| = (n_h + n_v + 3) u W|a|.  Second moments: the
    two factors carry their rounding (2), fl(g a) (1), the product (1), 11 additions; then 12 in the vertical pass -> (n_h + n_v + 5) u W(a^2), W(b^2),
    W|ab|.  mu_x = fl(ma + 0.5): one more u |mu_x|.  s_xx = fl(maa - fl(ma ma)): d_maa + 2 |ma| d_ma + u ma^2 + u |s_xx|; s_yy and s_xy likewise.
    The window's fp32 weights add up to 1 - e, e = 1.4e-9, so the specification's W(x) is W(a) + 0.5 (1 - e), not W(a) + 0.5: that moves mu by 0.5 e,
    s_xx by (|ma| + 0.25) e, s_xy by (|ma| / 2 + |mb| / 2 + 0.25) e; the bounds carry these terms.
    A1 = 2 mu_x mu_y + C1 (C1 rounded once; a product and a sum), A2 = 2 s_xy + C2, B1 = mu_x^2 + mu_y^2 + C1 (four operations), B2 = s_xx + s_yy + C2;
      dS <= (|A2| dA1 + |A1| dA2) / (B1 B2) + |S| (dB1 / B1 + dB2 / B2) + 4 u |S|     (two products and a correctly rounded division: 3 <= 4).
    The frame: the mean of dS, 16 u mean|S| for the additions, u |ssim| for the last rounding; x 1.1 for second order.
    The three gate families must come out <= 2e-5 at every shape (asserted: the bound itself, before the kernel runs)."""
    for family in FAMILIES:
        _, _, _, bound = _case(family, shape)
        assert bound[:, 2].max() <= CAP, f"{family} {shape}: frame bound {bound[:, 2].max():.2e} above {CAP:.0e}: change the draw, not the cap"
        assert (bound[:, :2].max(axis=0) <= 1e-5 * _case(family, shape)[2][:, :2].max(axis=0)).all()
    for family in FAMILIES:
        got, rows64, _ = _check(family, shape)
        if family == "flipped":
            assert (got[:, 2] < 0).all()


def test_identical_frames():
    for shape in SSIM_SHAPES[1:]:
        got, _, bound = _check("identical", shape)
        assert (got[:, :2] == 0).all() and ((got[:, 2].double() - 1).abs().numpy() <= bound[:, 2]).all()
        assert bound[:, 2].max() <= CAP


def test_ill_conditioned_frames_stay_finite():
    """near-constant frames and black against faint noise: s_xx + s_yy + C2 is hardly more than C2 and the moments' roundings are a visible fraction of it.
    Their own counted bounds (printed; about 4e-3) say how far fp32 can be from float64 here; the output is finite and no larger than 1 + bound"""
    for family in ("flat", "black"):
        got, rows64, bound = _check(family, ILL_SHAPE)
        print(f"[metrics] ill-conditioned {family}: counted ssim bound {bound[:, 2].tolist()}")
        assert (got[:, 2].double().numpy() <= 1 + bound[:, 2]).all() and bound[:, 2].max() <= 2e-2


def test_l1_and_mse_alone_on_a_frame_smaller_than_a_window():
    shape = (3, 4, 7, 5)
    for family in ("random", "identical"):
        got, rows64, _ = _check(family, shape, want_ssim=False)
        assert (got[:, 2:] == 0).all() and ((got[:, 0] > 0).all() if family == "random" else (got[:, :2] == 0).all())
    shape = ILL_SHAPE                                          # the same kernel path on several tiles: equal to the SSIM path's two columns
    p, t, _, _ = _case("random", shape)
    with_ssim, without = _launch(p.to(DEV), t.to(DEV), 1), _launch(p.to(DEV), t.to(DEV), 0)
    assert torch.equal(with_ssim[:, :2], without[:, :2]) and (without[:, 2] == 0).all()


def test_kernel_refuses_bad_arguments_and_writes_nothing():
    shape = (2, 3, 20, 15)
    p, t = (x.to(DEV) for x in _draw("random", shape))
    L = hip.lib()
    need = L.mrfa_frame_metrics_workspace(*shape)
    obuf, out = _guarded(8, torch.float32)
    wbuf, ws = _guarded(need // 8, torch.float64)
    good = dict(pred=p.data_ptr(), target=t.data_ptr(), N=2, C=3, H=20, W=15, want_ssim=1, workspace=ws.data_ptr(), workspace_bytes=need, out=out.data_ptr())
    for bad in (dict(pred=None), dict(target=None), dict(workspace=None), dict(out=None), dict(N=0), dict(C=-1), dict(H=0), dict(W=0),
                dict(workspace_bytes=need - 1), dict(H=10), dict(W=10), dict(pred=p.data_ptr() + 2), dict(target=t.data_ptr() + 1),
                dict(out=out.data_ptr() + 2), dict(workspace=ws.data_ptr() + 4)):
        rc = L.mrfa_frame_metrics(hip.stream_ptr(), *{**good, **bad}.values())
        msg = L.mrfa_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and "frame_metrics" in msg and len(msg) > 25, (bad, rc, msg)
        assert (obuf == CANARY).all() and (wbuf == CANARY).all(), bad                                             # nothing was launched
    for dims in ((0, 3, 20, 15), (2, 3, 20, -1)):
        assert L.mrfa_frame_metrics_workspace(*dims) < 0
    hip.check(L.mrfa_frame_metrics(hip.stream_ptr(), *good.values()), "mrfa_frame_metrics")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == CANARY).any()


# ------------------------------------------------------------------------------------------------------------- reconstruction
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_reconstruction_device_metrics(graph):
    """the dry model at 64 x 64, 2 sources, 4 frames in groups of 3 and 1: metrics="device" against metrics="host" under tests/test_clip_modules_gpu.py's gate
    between two runs (the metrics launches between two replays leave the captured programs alone), l1 and psnr to 1e-5 relative, and ssim within the
    counted bound of float64 on the returned prediction"""
    from mrfa_amd.infer import reconstruction
    from tests.test_bf16_cache import _dry_model
    from tests.test_clip_cpu import _clips
    from tests.test_clip_modules_gpu import _gate
    m = _dry_model().to(DEV)
    clip = _clips(4)[1].to(DEV)
    host = reconstruction(m, clip, graph=graph, frames_per_call=3)
    dev = reconstruction(m, clip, graph=graph, frames_per_call=3, metrics="device")
    assert set(host) == {"prediction", "l1", "psnr"} and dev["prediction"].shape == clip.shape
    _gate(dev["prediction"], host["prediction"], f"reconstruction graph={graph}: metrics='device' vs 'host'")
    for k in ("l1", "psnr"):
        rel = max(abs(a - b) / abs(b) for a, b in zip(dev[k], host[k]))
        print(f"[metrics] reconstruction graph={graph} {k}: device {dev[k]}, host {host[k]}, max relative difference {rel:.2e}")
        assert len(dev[k]) == 4 and rel <= 1e-5, k
    pred, drv = dev["prediction"].cpu(), clip.cpu()
    for j in range(4):
        rows64, bound = reference(pred[:, :, j].contiguous(), drv[:, :, j].contiguous())
        for k, col in (("l1", 0), ("mse", 1), ("ssim", 2)):
            assert (np.abs(dev["per_source"][k][:, j] - rows64[:, col]) <= bound[:, col]).all(), (k, j)
        assert abs(dev["ssim"][j] - rows64[:, 2].mean()) <= bound[:, 2].mean()
    print(f"[metrics] reconstruction graph={graph}: ssim {dev['ssim']}")
