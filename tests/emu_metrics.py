"""CPU specification of mrfa_frame_metrics / mrfa_frame_metrics_workspace (include/mrfa_hip_ext.h): MetricsEmulator adds them to tests/emu_ext.py's
ExtEmulator in float64 numpy with the entry's refusals and its one rounding; emulated_hip_metrics installs it the way emulated_hip_ext installs that one."""
import contextlib
import ctypes as C

import numpy as np

from mrfa_amd import engine, hip
from tests.emu import Counting
from tests.emu_ext import ExtEmulator

TAPS = 11
C1, C2 = 0.01 ** 2, 0.03 ** 2


def gauss_window() -> np.ndarray:
    """the eleven fp32 numbers that define the window, as float64: g_i = exp(-(i - 5)^2 / 4.5) / sum in float64, rounded to fp32"""
    g = np.exp(-(np.arange(TAPS, dtype=np.float64) - 5.0) ** 2 / 4.5)
    return (g / g.sum()).astype(np.float32).astype(np.float64)


def _window(x: np.ndarray, g: np.ndarray) -> np.ndarray:
    """(..., H, W) -> (..., H - 10, W - 10): the separable "valid" window as two sums of shifted slices"""
    H, W = x.shape[-2:]
    rows = sum(g[i] * x[..., i:i + H - TAPS + 1, :] for i in range(TAPS))
    return sum(g[i] * rows[..., :, i:i + W - TAPS + 1] for i in range(TAPS))


def ssim_map(p: np.ndarray, t: np.ndarray) -> np.ndarray:
    """float64 S of every window of (N,C,H,W) float64 images: (N,C,H-10,W-10)"""
    g = gauss_window()
    mx, my = _window(p, g), _window(t, g)
    sxx, syy, sxy = _window(p * p, g) - mx * mx, _window(t * t, g) - my * my, _window(p * t, g) - mx * my
    return (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def frame_metrics(p: np.ndarray, t: np.ndarray, want_ssim: bool) -> np.ndarray:
    """(N,4) float64 rows {l1, mse, ssim or 0, 0} of (N,C,H,W) images: the specification before its one rounding"""
    p, t = p.astype(np.float64), t.astype(np.float64)
    out = np.zeros((p.shape[0], 4))
    with np.errstate(all="ignore"):
        d = p - t
        out[:, 0] = np.abs(d).mean(axis=(1, 2, 3))
        out[:, 1] = (d * d).mean(axis=(1, 2, 3))
        if want_ssim:
            out[:, 2] = ssim_map(p, t).mean(axis=(1, 2, 3))
    return out


def _f32(ptr: int, n: int) -> np.ndarray:
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr))


class MetricsEmulator(ExtEmulator):
    def mrfa_frame_metrics_workspace(self, N, Cc, H, W):
        if N < 1 or Cc < 1 or H < 1 or W < 1:
            return -1
        TH, TW = engine.METRICS_TILE
        wgs = N * Cc * (-(-H // TH)) * (-(-W // TW))
        return -1 if wgs > 2 ** 31 - 1 else wgs * 24

    def mrfa_frame_metrics(self, stream, pred, target, N, Cc, H, W, want_ssim, workspace, workspace_bytes, out):
        bad = None
        if not (pred and target and workspace and out):
            bad = "null pointer"
        elif N < 1 or Cc < 1 or H < 1 or W < 1:
            bad = f"N, C, H and W must be >= 1 (N {N}, C {Cc}, H {H}, W {W})"
        elif self.mrfa_frame_metrics_workspace(N, Cc, H, W) < 0:
            bad = "the workgroups exceed one grid"
        elif workspace_bytes < self.mrfa_frame_metrics_workspace(N, Cc, H, W):
            bad = f"the workspace holds {workspace_bytes} bytes, mrfa_frame_metrics_workspace asks for {self.mrfa_frame_metrics_workspace(N, Cc, H, W)}"
        elif want_ssim and min(H, W) < TAPS:
            bad = f"SSIM needs one {TAPS} x {TAPS} window, min(H, W) >= {TAPS} (H {H}, W {W})"
        elif pred % 4 or target % 4 or out % 4 or workspace % 8:
            bad = "pred, target and out must be 4-byte aligned (scalar fp32 accesses), the workspace 8-byte aligned (doubles)"
        if bad:
            self._err = ("frame_metrics: " + bad).encode()
            return 1
        n = N * Cc * H * W
        rows = frame_metrics(_f32(pred, n).reshape(N, Cc, H, W), _f32(target, n).reshape(N, Cc, H, W), bool(want_ssim))
        with np.errstate(over="ignore"):
            _f32(out, N * 4)[:] = rows.astype(np.float32).reshape(-1)                              # the one rounding
        return 0


@contextlib.contextmanager
def emulated_hip_metrics(counting=False):
    """installs a MetricsEmulator as the loaded library and yields it; counting: behind tests.emu.Counting"""
    old_lib, old_stream = hip._lib, hip.stream_ptr
    lib = MetricsEmulator()
    hip._lib = Counting(lib) if counting else lib
    hip.stream_ptr = lambda: 0
    try:
        yield hip._lib
    finally:
        hip._lib, hip.stream_ptr = old_lib, old_stream
