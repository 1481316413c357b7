"""Clip metrics on the CPU through the specification of mrfa_frame_metrics (oracle/capi_emulator.py on oracle/infer_spec.py): the specification against a float64 torch restatement
written with F.conv2d, known values, what the entry and Ctx.frame_metrics refuse, ClipMetrics, infer.ssim and
reconstruction(metrics="device") on the dry model."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mrfa_amd import engine, hip
from mrfa_amd.infer import ClipMetrics, psnr, reconstruction, ssim
from mrfa_amd.utils.prng import det_uniform
from oracle import capi_emulator
from oracle.capi_emulator import Emulator
from oracle.infer_spec import frame_metrics
from tests.emu import emulated_hip

CANARY = -1234.5
PAD = 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_window() -> torch.Tensor:
    i = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(i - 5) ** 2 / 4.5)
    return (g / g.sum()).float().double()


def torch_metrics(p: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """the formulas of include/mrfa_hip.h restated in float64 torch with F.conv2d (depthwise, the 2-D outer-product window): (N,4) rows"""
    p, t = p.double(), t.double()
    C = p.shape[1]
    g = torch_window()
    w = (g[:, None] * g[None, :]).expand(C, 1, 11, 11).contiguous()
    win = lambda x: F.conv2d(x, w, groups=C)
    mx, my = win(p), win(t)
    sxx, syy, sxy = win(p * p) - mx * mx, win(t * t) - my * my, win(p * t) - mx * my
    S = (2 * mx * my + 0.01 ** 2) * (2 * sxy + 0.03 ** 2) / ((mx * mx + my * my + 0.01 ** 2) * (sxx + syy + 0.03 ** 2))
    d = p - t
    return torch.stack([d.abs().mean(dim=(1, 2, 3)), (d * d).mean(dim=(1, 2, 3)), S.mean(dim=(1, 2, 3)), torch.zeros(p.shape[0], dtype=torch.float64)], dim=1)


def families(tag, shape):
    """the three gate families of an (N,C,H,W) shape: name -> (p, t), fp32 in [0, 1]"""
    p = det_uniform(tag + "/p", shape, 0, 1)
    return {"random": (p, det_uniform(tag + "/t", shape, 0, 1)),
            "near": (p, (p + 0.02 * det_uniform(tag + "/n", shape, -1, 1)).clamp(0, 1)),
            "flipped": (p, 1 - p)}


def _entry(emu, p, t, want_ssim=1, **over):
    """one call of the entry on (N,C,H,W) fp32 tensors -> (rc, rows (N,4)), out and the workspace inside canary words; over: arguments by name"""
    N, C, H, W = p.shape
    need = max(emu.mrfa_frame_metrics_workspace(N, C, H, W), 24)
    obuf, wbuf = torch.full((4 * N + 2 * PAD,), CANARY), torch.full((need // 8 + 2 * PAD,), CANARY, dtype=torch.float64)
    a = dict(pred=p.data_ptr(), target=t.data_ptr(), N=N, C=C, H=H, W=W, want_ssim=want_ssim, workspace=wbuf.data_ptr() + 8 * PAD, workspace_bytes=need,
             out=obuf.data_ptr() + 4 * PAD)
    a.update(over)
    rc = emu.mrfa_frame_metrics(0, *a.values())
    assert (obuf[:PAD] == CANARY).all() and (obuf[PAD + 4 * N:] == CANARY).all() and (wbuf[:PAD] == CANARY).all() and (wbuf[-PAD:] == CANARY).all()
    return rc, obuf[PAD:PAD + 4 * N].view(N, 4)


def test_window_constants_of_the_kernel_and_the_tile_in_the_header():
    """the eleven fp32 literals of csrc/metrics.hip are the formula's numbers, and engine.METRICS_TILE and the emulator's METRICS_TILE are the header's tile"""
    src = open(os.path.join(ROOT, "mrfa_amd", "csrc", "metrics.hip")).read()
    body = re.search(r"GAUSS\[TAPS\]\s*=\s*\{([^}]*)\}", src).group(1)
    lits = [float.fromhex(x.strip().rstrip("f")) for x in body.split(",")]
    assert lits == torch_window().tolist() and len(lits) == 11
    hdr = open(os.path.join(ROOT, "include", "mrfa_hip.h")).read()
    tile = tuple(int(re.search(rf"#define MRFA_METRICS_TILE_{k}\s+(\d+)", hdr).group(1)) for k in "HW")
    assert tile == engine.METRICS_TILE == capi_emulator.METRICS_TILE
    assert {"mrfa_frame_metrics", "mrfa_frame_metrics_workspace"} <= set(hip.EXPORTED_SYMBOLS)


def test_specification_against_the_torch_restatement():
    for shape in ((2, 3, 40, 29), (1, 1, 11, 17), (3, 4, 23, 64)):
        for name, (p, t) in families(f"metrics/spec/{shape}", shape).items():
            got = frame_metrics(p.numpy(), t.numpy(), True)
            ref = torch_metrics(p, t).numpy()
            err = np.abs(got - ref).max()
            print(f"[metrics] specification vs F.conv2d restatement {shape} {name}: max |diff| {err:.2e}, ssim {ref[:, 2].tolist()}")
            assert err <= 1e-12
            assert (frame_metrics(p.numpy(), t.numpy(), False)[:, 2] == 0).all()
    emu = Emulator()
    p, t = families("metrics/spec/entry", (3, 3, 40, 29))["near"]
    rc, rows = _entry(emu, p, t)
    assert rc == 0 and torch.equal(rows, torch_metrics(p, t).float()) and (rows[:, 3] == 0).all()          # float64 to 1e-12, then the one rounding
    rc, rows0 = _entry(emu, p, t, want_ssim=0)
    assert rc == 0 and torch.equal(rows0[:, :2], rows[:, :2]) and (rows0[:, 2:] == 0).all()


def test_known_values():
    emu = Emulator()
    p = det_uniform("metrics/known/p", (2, 3, 30, 21), 0, 1)
    rc, rows = _entry(emu, p, p.clone())
    assert rc == 0 and (rows[:, :2] == 0).all() and (rows[:, 2].double() - 1).abs().max().item() <= 1e-12
    assert np.abs(frame_metrics(p.numpy(), p.numpy(), True)[:, 2] - 1).max() <= 1e-12
    with emulated_hip():
        cm = ClipMetrics()
        cm.add(p, p.clone())
        res = cm.result()
        assert np.isinf(res["psnr"]).all() and (res["psnr"] > 0).all() and (res["mse"] == 0).all() and (res["l1"] == 0).all()
        assert psnr(p, p.clone()) == float("inf")
    # an 11 x 11 frame is exactly one window: S from the five window sums, by hand
    x, y = det_uniform("metrics/known/x", (1, 1, 11, 11), 0, 1), det_uniform("metrics/known/y", (1, 1, 11, 11), 0, 1)
    g = torch_window()
    w2 = g[:, None] * g[None, :]
    xs, ys = x[0, 0].double(), y[0, 0].double()
    mx, my = (w2 * xs).sum(), (w2 * ys).sum()
    sxx, syy, sxy = (w2 * xs * xs).sum() - mx * mx, (w2 * ys * ys).sum() - my * my, (w2 * xs * ys).sum() - mx * my
    S = (2 * mx * my + 1e-4) * (2 * sxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    rc, rows = _entry(emu, x, y)
    assert rc == 0 and abs(frame_metrics(x.numpy(), y.numpy(), True)[0, 2] - S.item()) <= 1e-12 and rows[0, 2].item() == np.float32(S.item())
    # t = 1 - p: the covariance is minus the variance
    rc, rows = _entry(emu, p, 1 - p)
    assert rc == 0 and (rows[:, 2] < -0.5).all(), rows


def test_entry_refuses_bad_arguments_before_writing():
    emu = Emulator()
    p, t = det_uniform("metrics/bad/p", (2, 3, 20, 15), 0, 1), det_uniform("metrics/bad/t", (2, 3, 20, 15), 0, 1)
    rc, rows = _entry(emu, p, t)
    assert rc == 0 and not (rows == CANARY).any()
    need = emu.mrfa_frame_metrics_workspace(2, 3, 20, 15)
    TH, TW = engine.METRICS_TILE
    assert need == 2 * 3 * math.ceil(20 / TH) * math.ceil(15 / TW) * 24
    for dims in ((0, 3, 20, 15), (2, 0, 20, 15), (2, 3, 0, 15), (2, 3, 20, -1)):
        assert emu.mrfa_frame_metrics_workspace(*dims) < 0
    bads = [dict(pred=None), dict(target=None), dict(workspace=None), dict(out=None),
            dict(N=0), dict(C=0), dict(H=0), dict(W=-2),
            dict(workspace_bytes=need - 1), dict(workspace_bytes=0),
            dict(H=10), dict(W=10),                                                    # want_ssim with min(H, W) < 11
            dict(pred=p.data_ptr() + 2), dict(target=t.data_ptr() + 1)]
    for bad in bads:
        rc, rows = _entry(emu, p, t, **bad)
        assert rc != 0 and b"frame_metrics" in emu.mrfa_last_error() and len(emu.mrfa_last_error()) > 25, bad
        assert (rows == CANARY).all(), bad
    obuf, wbuf = torch.full((16,), CANARY), torch.full((need // 8 + 2,), CANARY, dtype=torch.float64)
    for over in (dict(out=obuf.data_ptr() + 2), dict(workspace=wbuf.data_ptr() + 4)):
        a = dict(pred=p.data_ptr(), target=t.data_ptr(), N=2, C=3, H=20, W=15, want_ssim=1, workspace=wbuf.data_ptr(), workspace_bytes=need, out=obuf.data_ptr())
        a.update(over)
        assert emu.mrfa_frame_metrics(0, *a.values()) != 0 and (obuf == CANARY).all() and (wbuf == CANARY).all()
    rc, rows = _entry(emu, p[..., :10, :].contiguous(), t[..., :10, :].contiguous(), want_ssim=0)          # without SSIM any size goes
    assert rc == 0 and (rows[:, 2] == 0).all() and (rows[:, 0] > 0).all()


def test_ctx_frame_metrics_checks_and_a_recording_context():
    p, t = det_uniform("metrics/ctx/p", (2, 3, 20, 15), 0, 1), det_uniform("metrics/ctx/t", (2, 3, 20, 15), 0, 1)
    with emulated_hip(counting=True) as lib:
        e = engine.Ctx(torch.device("cpu"), train=False, record=False)
        launches = lambda: [c for c, _ in lib.calls if c == "mrfa_frame_metrics"]
        for args, kw in (((p, t[:1]), {}), ((p[0], t[0]), {}), ((p.double(), t.double()), {}), ((p, t.half()), {}), ((p[..., ::2], t[..., ::2]), {}),
                         ((p.permute(0, 1, 3, 2), t.permute(0, 1, 3, 2)), {}), ((p[..., :10, :].contiguous(), t[..., :10, :].contiguous()), {}),
                         ((p[:0], t[:0]), {}), ((p, t.numpy()), {}), ((p.to("meta"), t), {})):
            with pytest.raises(ValueError, match="frame_metrics"):
                e.frame_metrics(*args, **kw)
        with pytest.raises(RuntimeError, match="no backward"):
            engine.Ctx(torch.device("cpu"), train=False, record=True).frame_metrics(p, t)
        assert launches() == []                                                       # refused before anything was launched
        rows = e.frame_metrics(p, t)
        again = engine.Ctx(torch.device("cpu"), train=False, record=False).frame_metrics(p, t, want_ssim=False)
        assert rows.shape == (2, 4) and rows.dtype == torch.float32 and torch.equal(rows, torch_metrics(p, t).float())
        assert torch.equal(again[:, :2], rows[:, :2]) and (again[:, 2:] == 0).all() and len(launches()) == 2
        ws = [a[8] for c, a in lib.calls if c == "mrfa_frame_metrics"]
        assert ws[0] == ws[1]                                                         # one workspace per shape, kept
        assert [c for c, _ in lib.calls].count("mrfa_frame_metrics_workspace") == 1
        assert torch.equal(ssim(p, t), rows[:, 2]) and ssim(p, t).shape == (2,)
        small = e.frame_metrics(p[..., :7, :5].contiguous(), t[..., :7, :5].contiguous(), want_ssim=False)
        assert small.shape == (2, 4) and (small[:, 2] == 0).all()


def test_clip_metrics_groups_equal_one_group(monkeypatch):
    p, t = families("metrics/groups", (7, 3, 24, 19))["near"]
    with emulated_hip(counting=True) as lib:
        reads = []
        real = torch.Tensor.cpu
        monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append("cpu"), real(self, *a, **k))[1])
        one, three = ClipMetrics(), ClipMetrics()
        one.add(p, t)
        for a, b in ((0, 3), (3, 6), (6, 7)):
            three.add(p[a:b].contiguous(), t[a:b].contiguous())
        assert not reads and len(one) == len(three) == 7
        r1, r3 = one.result(), three.result()
        assert reads == ["cpu", "cpu"]                                                # one host read per result()
        assert [c for c, _ in lib.calls].count("mrfa_frame_metrics") == 4
        ref = torch_metrics(p, t).float().double().numpy()
        for k, col in (("l1", 0), ("mse", 1), ("ssim", 2)):
            assert r1[k].dtype == np.float64 and r1[k].shape == (7,) and np.array_equal(r1[k], r3[k]) and np.array_equal(r1[k], ref[:, col]), k
        assert np.array_equal(r1["psnr"], 20 * np.log10(1 / np.sqrt(ref[:, 1]))) and np.array_equal(r1["psnr"], r3["psnr"])
        nos = ClipMetrics(ssim=False)
        nos.add(p[..., :7, :5].contiguous(), t[..., :7, :5].contiguous())
        assert (nos.result()["ssim"] == 0).all() and ClipMetrics().result()["l1"].shape == (0,)


def test_reconstruction_device_metrics_on_the_dry_model():
    from tests.test_bf16_cache import _dry_model
    from tests.test_clip_cpu import _clips
    with emulated_hip(counting=True) as lib:
        m = _dry_model()
        _, clip = _clips(4)
        host = reconstruction(m, clip, frames_per_call=3)
        assert set(host) == {"prediction", "l1", "psnr"}                             # the default is today's path and return value
        same = reconstruction(m, clip, frames_per_call=3, metrics="host")
        assert torch.equal(same["prediction"], host["prediction"]) and same["l1"] == host["l1"] and same["psnr"] == host["psnr"]
        assert "mrfa_frame_metrics" not in [c for c, _ in lib.calls]
        del lib.calls[:]
        dev = reconstruction(m, clip, frames_per_call=3, metrics="device")
        calls = [a for c, a in lib.calls if c == "mrfa_frame_metrics"]
        assert len(calls) == math.ceil(4 / 3) and [(a[3], a[4], a[5], a[6], a[7]) for a in calls] == [(6, 3, 64, 64, 1), (2, 3, 64, 64, 1)]
        assert torch.equal(dev["prediction"], host["prediction"]) and dev["prediction"].shape == clip.shape
        for k in ("l1", "psnr"):
            rel = max(abs(a - b) / abs(b) for a, b in zip(dev[k], host[k]))
            print(f"[metrics] reconstruction device vs host {k}: max relative difference {rel:.2e}")
            assert len(dev[k]) == 4 and all(isinstance(v, float) for v in dev[k]) and rel <= 1e-6, k
        # row s T + j of a group is source s, frame t0 + j: per-source numbers against the restatement on the returned prediction
        ref = torch.stack([torch_metrics(dev["prediction"][:, :, j].contiguous(), clip[:, :, j].contiguous()) for j in range(4)], dim=1)      # (B,T,4)
        ref32 = ref.float().double().numpy()
        for k, col in (("l1", 0), ("mse", 1), ("ssim", 2)):
            assert dev["per_source"][k].shape == (2, 4) and np.array_equal(dev["per_source"][k], ref32[:, :, col]), k
        assert np.array_equal(dev["per_source"]["psnr"], 20 * np.log10(1 / np.sqrt(ref32[:, :, 1])))
        assert dev["ssim"] == ref32[:, :, 2].mean(axis=0).tolist() and len(dev["ssim"]) == 4
        assert not np.allclose(ref32[0, :, 2], ref32[1, :, 2])                        # the two sources are told apart
        with pytest.raises(ValueError, match="metrics"):
            reconstruction(m, clip, metrics="bogus")
