"""The CPU specification of libmrfa_data_hip.so: a numpy restatement of the rules of include/mrfa_data_hip.h (each operation rounded where the header says so)
and of the whole entry mrfa_pair_augment -- the refusals, the per-frame contrast mean, the flips, byte -> float.  tests/test_augment_reference.py holds it
against Pillow on all 2^24 colours and against the committed goldens; tests/emu_data.py installs `Library` as the loaded library of mrfa_amd.data_hip."""
import ctypes as C
import math

import numpy as np

f32, f64, i64 = np.float32, np.float64, np.int64
NONE, BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3, 4
MAX_PAIRS, PARTS, MAX_PIXELS, VERSION = 32, 64, 1 << 30, 1
INV255 = f32(1.0 / 255.0)


def all_colours() -> np.ndarray:
    """the 2^24 colours as a (4096, 4096, 3) uint8 image: pixel v holds (v >> 16, v >> 8 & 255, v & 255)"""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def luma(rgb: np.ndarray) -> np.ndarray:
    r, g, b = (rgb[..., k].astype(i64) for k in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def blend(d, x: np.ndarray, f) -> np.ndarray:
    """d: a byte or an array of bytes that broadcasts against x; f: the factor (rounded to f32 here)"""
    fd = np.asarray(d).astype(f32)
    t = (fd + (f32(f) * (x.astype(f32) - fd)).astype(f32)).astype(f32)
    return np.clip(np.trunc(t), 0, 255).astype(np.uint8)


def brightness(rgb, f):
    return blend(0, rgb, f)


def saturation(rgb, f):
    return blend(luma(rgb)[..., None], rgb, f)


def contrast_mean(rgb) -> int:
    L = luma(rgb)
    return int((2 * int(L.sum()) + L.size) // (2 * L.size))


def contrast(rgb, f):
    return blend(contrast_mean(rgb), rgb, f)


def rgb_to_hsv(rgb: np.ndarray) -> np.ndarray:
    r, g, b = (rgb[..., k].astype(i64) for k in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    with np.errstate(all="ignore"):
        cr = (mx - mn).astype(f32)
        sat = (cr / mx.astype(f32)).astype(f32)
        rc, gc, bc = (((mx - c).astype(f32) / cr).astype(f32) for c in (r, g, b))
        rd, gd, bd = rc.astype(f64), gc.astype(f64), bc.astype(f64)
        h = np.where(r == mx, (bc - gc).astype(f32), np.where(g == mx, (2.0 + rd - bd).astype(f32), (4.0 + gd - rd).astype(f32))).astype(f32)
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        H = np.clip(np.nan_to_num(h.astype(f64) * 255.0).astype(i64), 0, 255)
        S = np.clip(np.nan_to_num(sat.astype(f64) * 255.0).astype(i64), 0, 255)
    grey = mx == mn
    return np.stack([np.where(grey, 0, H), np.where(grey, 0, S), mx], -1).astype(np.uint8)


def _round_byte(v: np.ndarray) -> np.ndarray:
    """C round() of v >= 0, halves away from zero: floor and the (exact) fraction"""
    fl = np.floor(v)
    return np.clip(fl.astype(i64) + (v - fl >= 0.5), 0, 255)


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    H, S, V = (hsv[..., k] for k in range(3))
    hf = H.astype(f32).astype(f64) * 6.0 / 255.0
    fi = np.floor(hf)
    f = (hf - fi).astype(f32).astype(f64)
    fs = (S.astype(f32).astype(f64) / 255.0).astype(f32).astype(f64)
    v = V.astype(f64)
    p, q, t = _round_byte(v * (1.0 - fs)), _round_byte(v * (1.0 - fs * f)), _round_byte(v * (1.0 - fs * (1.0 - f)))
    Vi, k = V.astype(i64), fi.astype(i64) % 6
    R, G, B = np.choose(k, [Vi, q, p, p, t, Vi]), np.choose(k, [t, Vi, Vi, q, p, p]), np.choose(k, [p, p, t, Vi, Vi, q])
    z = S == 0
    return np.stack([np.where(z, Vi, R), np.where(z, Vi, G), np.where(z, Vi, B)], -1).astype(np.uint8)


def hue_shift_of(h: float) -> int:
    """the byte added to H for a hue factor h in [-0.5, 0.5]: trunc(255 h) modulo 256 (two's complement for h < 0)"""
    return int(math.trunc(255.0 * h)) % 256


def hue(rgb, shift: int):
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = (hsv[..., 0].astype(i64) + int(shift)) % 256
    return hsv_to_rgb(hsv)


def apply_ops(rgb: np.ndarray, ops, factor, shift: int) -> np.ndarray:
    """one frame (H,W,3) through the op chain: ops are codes in application order (NONE skipped), factor = (brightness, contrast, saturation)"""
    for o in ops:
        if o == BRIGHTNESS:
            rgb = brightness(rgb, factor[0])
        elif o == CONTRAST:
            rgb = contrast(rgb, factor[1])
        elif o == SATURATION:
            rgb = saturation(rgb, factor[2])
        elif o == HUE:
            rgb = hue(rgb, shift)
    return rgb


def to_rgb(frame: np.ndarray) -> np.ndarray:
    """(H,W,Cin) bytes -> (H,W,3): grey fills all three channels, alpha is dropped (the rules of mrfa_frames_from_u8)"""
    return np.repeat(frame, 3, axis=-1) if frame.shape[-1] == 1 else frame[..., :3]


def unit(bytes_: np.ndarray) -> np.ndarray:
    """byte -> float: ONE fp32 multiply by fl32(1 / 255)"""
    return bytes_.astype(f32) * INV255


def pair_augment_bytes(src: np.ndarray, params) -> tuple:
    """src uint8 (B,2,H,W,Cin); params: per pair a mapping / object with ops, factor, hue_shift, time_flip, hflip.  Returns (source, driving) as uint8
    (B,3,H,W): the bytes whose `unit` the entry writes."""
    B = src.shape[0]
    out = [np.empty((B, 3) + src.shape[2:4], np.uint8) for _ in range(2)]
    for b in range(B):
        ops, factor, shift, tflip, hflip = params[b]
        for t in range(2):
            x = apply_ops(to_rgb(src[b, t]), ops, factor, shift)
            if hflip:
                x = x[:, ::-1]
            out[t ^ int(bool(tflip))][b] = x.transpose(2, 0, 1)
    return out[0], out[1]


# ----------------------------------------------------------------------------------------------------------------------- the entry, on CPU memory
class PairAug(C.Structure):
    """mrfa_pair_aug (mrfa_amd.data_hip.PairAug has the same fields; kept apart so that the specification does not import what it specifies)"""
    _fields_ = [("factor", C.c_float * 3), ("op", C.c_ubyte * 4), ("hue_shift", C.c_ubyte), ("time_flip", C.c_ubyte), ("hflip", C.c_ubyte),
                ("reserved", C.c_ubyte)]


def _view(ptr: int, n: int, dtype) -> np.ndarray:
    return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype)


class Library:
    """stands where ctypes.CDLL(libmrfa_data_hip.so) stands: the same four entries, pointers are addresses of CPU memory"""

    def __init__(self):
        self.error = b""

    def mrfa_data_version(self):
        return VERSION

    def mrfa_data_last_error(self):
        return self.error

    def mrfa_pair_augment_workspace(self, B, H, W):
        if min(B, H, W) < 1 or H * W > MAX_PIXELS or B > MAX_PAIRS:
            return -1
        return 2 * B * PARTS * 4

    def _refuse(self, msg):
        self.error = ("pair_augment: " + msg).encode()
        return 1

    def mrfa_pair_augment(self, stream, src, B, H, W, Cin, params, workspace, workspace_bytes, source, driving):
        if not (src and params and workspace and source and driving):
            return self._refuse("null pointer")
        if min(B, H, W) < 1:
            return self._refuse(f"B, H and W must be >= 1 (B {B}, H {H}, W {W})")
        if H * W > MAX_PIXELS:
            return self._refuse(f"H W must be <= {MAX_PIXELS}")
        if B > MAX_PAIRS:
            return self._refuse(f"B must be <= {MAX_PAIRS} pairs per call (B {B})")
        if Cin not in (1, 3, 4):
            return self._refuse(f"Cin must be 1 (grey), 3 or 4 (alpha is dropped), not {Cin}")
        descs = []
        for b in range(B):
            a = params[b]
            ops = list(a.op)
            for k, o in enumerate(ops):
                if o > HUE:
                    return self._refuse(f"pair {b}: op[{k}] is {o}, not one of 0 (none) .. {HUE}")
                if o != NONE and o in ops[:k]:
                    return self._refuse(f"pair {b}: op {o} appears twice")
            for k, f in enumerate(a.factor):
                if not (math.isfinite(f) and f >= 0):
                    return self._refuse(f"pair {b}: factor[{k}] must be finite and >= 0 ({f})")
            descs.append((ops, tuple(a.factor), a.hue_shift, a.time_flip, a.hflip))
        need = self.mrfa_pair_augment_workspace(B, H, W)
        if workspace_bytes < need:
            return self._refuse(f"the workspace has {workspace_bytes} bytes, mrfa_pair_augment_workspace({B}, {H}, {W}) asks for {need}")
        if workspace % 8:
            return self._refuse("workspace must be 8-byte aligned")
        if source % 4 or driving % 4:
            return self._refuse("source and driving must be 4-byte aligned (fp32 stores)")
        s, d = pair_augment_bytes(_view(src, B * 2 * H * W * Cin, np.uint8).reshape(B, 2, H, W, Cin), descs)
        _view(source, B * 3 * H * W, f32)[:] = unit(s).reshape(-1)
        _view(driving, B * 3 * H * W, f32)[:] = unit(d).reshape(-1)
        return 0


# ----------------------------------------------------------------------------------------------------------------------- shared test inputs
def det_bytes(name: str, shape) -> np.ndarray:
    """uint8 test frames, a pure function of (name, shape): mrfa_amd/utils/prng.py's stream, so goldens store only parameters and outputs"""
    from mrfa_amd.utils.prng import uniform01
    return np.minimum(np.floor(uniform01(name, int(np.prod(shape))) * 256.0), 255).astype(np.uint8).reshape(shape)


def ops_of(case_ops):
    """[(name, value), ...] of a golden case -> (op codes, factor triple, hue shift)"""
    code = {"brightness": BRIGHTNESS, "contrast": CONTRAST, "saturation": SATURATION, "hue": HUE}
    factor, shift = [1.0, 1.0, 1.0], 0
    for n, v in case_ops:
        if n == "hue":
            shift = hue_shift_of(v)
        else:
            factor[code[n] - 1] = v
    return [code[n] for n, _ in case_ops], tuple(factor), shift
