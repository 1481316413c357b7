"""CPU specification of mrfa_frames_from_u8 / mrfa_frames_to_u8 (include/mrfa_hip_ext.h): FramesEmulator adds them to tests/emu_metrics.py's
MetricsEmulator in fp32 numpy, one rounding per operation in the header's order, with the entries' refusals; emulated_hip_frames installs it the way
emulated_hip_metrics installs that one."""
import contextlib
import ctypes as C
import math

import numpy as np

from mrfa_amd import hip
from tests.emu import Counting
from tests.emu_metrics import MetricsEmulator

MAX_TILES, MAX_KP = 8, 64
F = np.float32


def _f32(ptr: int, n: int) -> np.ndarray:
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr))


def _u8(ptr: int, n: int) -> np.ndarray:
    return np.ctypeslib.as_array((C.c_ubyte * n).from_address(ptr))


def from_u8(src: np.ndarray) -> np.ndarray:
    """uint8 (N,H,W,Cin) -> fp32 (N,3,H,W): fl32(v) * fl32(1 / 255); grey in all three planes, alpha dropped"""
    v = src[..., [0, 0, 0]] if src.shape[3] == 1 else src[..., :3]
    return np.ascontiguousarray((v.astype(F) * F(1.0 / 255.0)).transpose(0, 3, 1, 2))


def quantise(s: np.ndarray, rounding: int) -> np.ndarray:
    """fp32 samples -> bytes: p = s * 255 in fp32, rint (ties to even) or trunc, clamped to [0,255]; NaN 0, +inf 255, -inf 0"""
    with np.errstate(all="ignore"):
        p = s.astype(F) * F(255.0)
        r = np.rint(p) if rounding == 0 else np.trunc(p)
        r = np.where(r > 0, np.minimum(r, F(255.0)), F(0.0))                              # (a NaN compares false: 0)
    return r.astype(np.uint8)


def disc_index(kp: np.ndarray, H: int, W: int, radius: float) -> np.ndarray:
    """(K,2) keypoints of one image -> (H,W) int: the largest k whose disc covers the pixel, -1 for none; fp32, each operation rounded once"""
    hit = np.full((H, W), -1, dtype=np.int64)
    rr, cc = np.arange(H, dtype=F)[:, None], np.arange(W, dtype=F)[None, :]
    r2 = F(radius) * F(radius)
    with np.errstate(all="ignore"):
        for k in range(kp.shape[0]):
            x, y = F(kp[k, 0]), F(kp[k, 1])
            if not (np.isfinite(x) and np.isfinite(y)):
                continue
            cx, cy = (F(W) * (x + F(1.0))) * F(0.5), (F(H) * (y + F(1.0))) * F(0.5)
            dy, dx = rr - cy, cc - cx
            hit[(dy * dy + dx * dx) < r2] = k
    return hit


def compose_tile(src, kp, radius, colors, border, rounding) -> np.ndarray:
    """one tile: fp32 (N,3,H,W) -> uint8 (N,H,W,3) with discs and border"""
    N, _, H, W = src.shape
    out = np.ascontiguousarray(quantise(src, rounding).transpose(0, 2, 3, 1))
    if kp is not None:
        cq = quantise(colors, rounding)
        for n in range(N):
            hit = disc_index(kp[n], H, W, radius)
            out[n][hit >= 0] = cq[hit[hit >= 0]]
    if border:
        out[:, :, 0, :] = 255
        out[:, :, W - 1, :] = 255
    return out


class FramesEmulator(MetricsEmulator):
    def mrfa_frames_from_u8(self, stream, src, N, H, W, Cin, dst):
        bad = None
        if not (src and dst):
            bad = "null pointer"
        elif N < 1 or H < 1 or W < 1:
            bad = f"N, H and W must be >= 1 (N {N}, H {H}, W {W})"
        elif Cin not in (1, 3, 4):
            bad = f"Cin must be 1 (grey), 3 or 4 (alpha is dropped), not {Cin}"
        elif dst % 4:
            bad = "dst must be 4-byte aligned (fp32 stores)"
        if bad:
            self._err = ("frames_from_u8: " + bad).encode()
            return 1
        _f32(dst, N * 3 * H * W)[:] = from_u8(_u8(src, N * H * W * Cin).reshape(N, H, W, Cin)).reshape(-1)
        return 0

    def mrfa_frames_to_u8(self, stream, tiles, n_tiles, N, dst, Hd, Wd, rounding):
        bad = None
        if not (tiles and dst):
            bad = "null pointer"
        elif not 1 <= n_tiles <= MAX_TILES:
            bad = f"1 <= n_tiles <= {MAX_TILES} (n_tiles {n_tiles})"
        elif N < 1 or Hd < 1 or Wd < 1:
            bad = f"N, Hd and Wd must be >= 1 (N {N}, Hd {Hd}, Wd {Wd})"
        elif rounding not in (0, 1):
            bad = f"rounding must be 0 (nearest, ties to even) or 1 (floor), not {rounding}"
        ts = []
        if not bad:
            arr = C.cast(tiles, C.POINTER(hip.U8Tile))
            ts = [arr[i] for i in range(n_tiles)]
        for i, t in enumerate(ts):
            if bad:
                break
            if not t.src:
                bad = f"tile {i} has a null src"
            elif t.src % 4:
                bad = f"tile {i}: src must be 4-byte aligned"
            elif t.H < 1 or t.W < 1:
                bad = f"tile {i}: H and W must be >= 1 (H {t.H}, W {t.W})"
            elif t.y0 < 0 or t.x0 < 0 or t.y0 + t.H > Hd or t.x0 + t.W > Wd:
                bad = f"tile {i} ({t.H} x {t.W} at y0 {t.y0}, x0 {t.x0}) lies outside dst ({Hd} x {Wd})"
            elif t.kp and not t.colors:
                bad = f"tile {i} has keypoints and colors == NULL"
            elif t.kp and not 1 <= t.K <= MAX_KP:
                bad = f"tile {i}: 1 <= K <= {MAX_KP} (K {t.K})"
            elif t.kp and not (math.isfinite(t.radius) and t.radius > 0):
                bad = f"tile {i}: the radius must be finite and > 0 (radius {t.radius:g})"
            elif t.kp and (t.kp % 4 or t.colors % 4):
                bad = f"tile {i}: kp and colors must be 4-byte aligned"
            else:
                for j, u in enumerate(ts[:i]):
                    if not (t.y0 >= u.y0 + u.H or u.y0 >= t.y0 + t.H or t.x0 >= u.x0 + u.W or u.x0 >= t.x0 + t.W):
                        bad = f"tiles {j} ({u.H} x {u.W} at y0 {u.y0}, x0 {u.x0}) and {i} ({t.H} x {t.W} at y0 {t.y0}, x0 {t.x0}) overlap"
        if bad:
            self._err = ("frames_to_u8: " + bad).encode()
            return 1
        out = _u8(dst, N * Hd * Wd * 3).reshape(N, Hd, Wd, 3)
        for t in ts:
            src = _f32(t.src, N * 3 * t.H * t.W).reshape(N, 3, t.H, t.W)
            kp = _f32(t.kp, N * t.K * 2).reshape(N, t.K, 2) if t.kp else None
            colors = _f32(t.colors, t.K * 3).reshape(t.K, 3) if t.kp else None
            out[:, t.y0:t.y0 + t.H, t.x0:t.x0 + t.W, :] = compose_tile(src, kp, t.radius, colors, t.border, rounding)
        return 0


@contextlib.contextmanager
def emulated_hip_frames(counting=False):
    """installs a FramesEmulator as the loaded library and yields it; counting: behind tests.emu.Counting"""
    old_lib, old_stream = hip._lib, hip.stream_ptr
    lib = FramesEmulator()
    hip._lib = Counting(lib) if counting else lib
    hip.stream_ptr = lambda: 0
    try:
        yield hip._lib
    finally:
        hip._lib, hip.stream_ptr = old_lib, old_stream
