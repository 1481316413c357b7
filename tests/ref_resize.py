"""The numpy specification of the resize entries of libmrfa_data_hip.so (include/mrfa_resize_hip.h): Pillow's Image.resize(size, resample, box) on 8-bit
channels, restated operation by operation, and a `Library` that stands where the binding's ctypes library stands (pointers are addresses of CPU memory), the
way tests/ref_augment.py's does for the augmenter.  tests/test_resize_reference.py holds it against Pillow in every byte."""
import ctypes as C
import math

import numpy as np

VERSION = 1
MAX_TAPS = 383
BOX, BILINEAR, HAMMING, BICUBIC, LANCZOS = 0, 1, 2, 3, 4
FILTERS = {"box": BOX, "bilinear": BILINEAR, "hamming": HAMMING, "bicubic": BICUBIC, "lanczos": LANCZOS}
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, HAMMING: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
PRECISION_BITS = 22
f32 = np.float32

# (source H, W), (output H, W), box (left, upper, right, lower) or None: the geometry list of the tests
GEOMETRIES = [
    ((1, 1), (1, 1), None),
    ((1, 1), (2, 3), None),
    ((2, 3), (7, 5), None),
    ((37, 53), (16, 16), None),
    ((64, 64), (16, 16), None),
    ((90, 70), (24, 16), (3.5, 2.25, 60.75, 81.0)),
    ((17, 19), (64, 64), (2.2, 3.3, 9.9, 12.1)),
    ((8, 300), (17, 5), None),
    ((200, 333), (70, 130), None),
    ((270, 480), (64, 64), (100, 7, 370, 267)),
    ((256, 256), (256, 256), None),
]


# tests/golden/resize_pillow.npz (tools/make_resize_golden.py): Pillow's bytes of (index into GEOMETRIES, C, filter, "random" | "extreme"); the input is
# case_input(...), a pure function of the case, so the file stores outputs only
GOLDEN_CASES = [(1, 3, "bilinear", "random"), (2, 3, "bicubic", "random"), (3, 1, "lanczos", "random"), (3, 3, "hamming", "extreme"),
                (4, 3, "box", "random"), (5, 3, "bilinear", "random"), (5, 3, "lanczos", "extreme"), (6, 3, "bicubic", "extreme"),
                (6, 1, "hamming", "random"), (7, 3, "lanczos", "random"), (9, 3, "bilinear", "random")]


def case_input(gi: int, C_: int, kind: str, N: int = 1) -> np.ndarray:
    """the uint8 (N,Hi,Wi,C) input of a test case"""
    hi, wi = GEOMETRIES[gi][0]
    return (extreme_bytes if kind == "extreme" else det_bytes)(f"resize/{gi}/{C_}/{kind}", (N, hi, wi, C_))


def geometry_id(g) -> str:
    (hi, wi), (ho, wo), box = g
    return f"{hi}x{wi}-{ho}x{wo}" + ("" if box is None else "-box")


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def filter_value(f: int, x: float) -> float:
    if f == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if f == BILINEAR:
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if f == HAMMING:
        x = abs(x)
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))
    if f == BICUBIC:
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if f == LANCZOS:
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    raise ValueError(f"unknown filter {f!r}")


def box_ok(in_size: int, in0, in1) -> bool:
    in0, in1 = f32(in0), f32(in1)
    return bool(np.isfinite(in0) and np.isfinite(in1) and in0 >= 0 and in1 <= in_size and f32(in1 - in0) > 0)


def ksize_of(in0, in1, out_size: int, f: int) -> int:
    """taps per output sample of one axis (not held against MAX_TAPS here)"""
    d = float(f32(f32(in1) - f32(in0)))
    fscale = max(d / out_size, 1.0)
    return 2 * int(math.ceil(SUPPORT[f] * fscale)) + 1


def coeffs(in_size: int, in0, in1, out_size: int, f: int):
    """-> bounds (out_size,2) int32 rows (xmin, cnt), kk (out_size, ksize) int32"""
    in0 = float(f32(in0))
    d = float(f32(f32(in1) - f32(in0)))
    scale = d / out_size
    fscale = max(scale, 1.0)
    support = SUPPORT[f] * fscale
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fscale
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                      # int(): C truncation
        cnt = min(int(center + support + 0.5), in_size) - xmin
        w = [filter_value(f, (x + xmin - center + 0.5) * ss) for x in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(cnt):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(v * 4194304.0 + (-0.5 if v < 0 else 0.5))
        bounds[xx] = (xmin, cnt)
    return bounds, kk


def resample_axis(img: np.ndarray, axis: int, bounds: np.ndarray, kk: np.ndarray) -> np.ndarray:
    """one pass over `axis` of a uint8 array: bytes out"""
    a = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.uint8)
    for xx, (xmin, cnt) in enumerate(bounds):
        k = kk[xx, :cnt].astype(np.int64).reshape((cnt,) + (1,) * (a.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (a[xmin:xmin + cnt] * k).sum(axis=0)
        assert np.abs(acc).max(initial=0) < 2 ** 31                     # (the int32 accumulator of the kernel does not wrap)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def full_box(Hi: int, Wi: int, box):
    return (0.0, 0.0, float(Wi), float(Hi)) if box is None else tuple(float(v) for v in box)


def tables(Hi: int, Wi: int, size, box, f: int):
    """(bounds_h, kk_h, bounds_v, kk_v) of a geometry; size = (Ho, Wo), box = (left, upper, right, lower)"""
    left, upper, right, lower = full_box(Hi, Wi, box)
    return coeffs(Wi, left, right, size[1], f) + coeffs(Hi, upper, lower, size[0], f)


def rgb_of(frames: np.ndarray) -> np.ndarray:
    """(N,H,W,C), C in {1,3,4} -> (N,H,W,3): grey fills three channels, the fourth byte is dropped"""
    return np.repeat(frames, 3, axis=3) if frames.shape[3] == 1 else frames[..., :3]


def resize_bytes(frames: np.ndarray, size, box=None, f: int = BILINEAR) -> np.ndarray:
    """uint8 (N,Hi,Wi,C) -> uint8 (N,Ho,Wo,3): the horizontal pass to BYTES, then the vertical pass, always both"""
    bh, kh, bv, kv = tables(frames.shape[1], frames.shape[2], size, box, f)
    return resample_axis(resample_axis(rgb_of(frames), 2, bh, kh), 1, bv, kv)


def unit(b: np.ndarray) -> np.ndarray:
    """bytes (N,H,W,3) -> fp32 (N,3,H,W): fl32(byte) * fl32(1 / 255), one multiply"""
    return np.ascontiguousarray((b.astype(f32) * f32(1.0 / 255.0)).transpose(0, 3, 1, 2))


def det_bytes(name: str, shape) -> np.ndarray:
    from tests.ref_augment import det_bytes as d
    return d(name, shape)


def extreme_bytes(name: str, shape) -> np.ndarray:
    """a 0/255-only image: bicubic and Lanczos overshoot both ways and clamp"""
    return np.where(det_bytes(name, shape) >= 128, 255, 0).astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------- the entries, on CPU memory
def _view(ptr: int, n: int, dtype) -> np.ndarray:
    return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype)


def _addr(p) -> int:
    if p is None:
        return 0
    if isinstance(p, int):
        return p
    return C.cast(p, C.c_void_p).value or 0


class Library:
    """stands where ctypes.CDLL(libmrfa_data_hip.so) stands for mrfa_amd.resize_hip: the resize entries and the library's error message"""

    def __init__(self):
        self.error = b""

    def mrfa_resize_version(self):
        return VERSION

    def mrfa_data_last_error(self):
        return self.error

    def _refuse(self, msg, rc=1):
        self.error = msg.encode()
        return rc

    def _axis(self, who, in_size, in0, in1, out_size, filt):
        if in_size < 1 or out_size < 1:
            return self._refuse(f"{who}: in_size and out_size must be >= 1 (in_size {in_size}, out_size {out_size})", -1)
        if filt not in SUPPORT:
            return self._refuse(f"{who}: unknown filter {filt}", -1)
        if not box_ok(in_size, in0, in1):
            return self._refuse(f"{who}: the box [{in0}, {in1}] must lie in [0, {in_size}] with in1 - in0 > 0", -1)
        k = ksize_of(in0, in1, out_size, filt)
        if k > MAX_TAPS:
            return self._refuse(f"{who}: {k} taps per output sample, at most {MAX_TAPS}", -1)
        return k

    def mrfa_resize_ksize(self, in_size, in0, in1, out_size, filt):
        return self._axis("resize_ksize", in_size, in0, in1, out_size, filt)

    def mrfa_resize_coeffs(self, in_size, in0, in1, out_size, filt, bounds, kk):
        bounds, kk = _addr(bounds), _addr(kk)
        if not (bounds and kk):
            return self._refuse("resize_coeffs: null table")
        k = self._axis("resize_coeffs", in_size, in0, in1, out_size, filt)
        if k < 0:
            return 1
        b, c = coeffs(in_size, in0, in1, out_size, filt)
        _view(bounds, 2 * out_size, np.int32)[:] = b.reshape(-1)
        _view(kk, out_size * k, np.int32)[:] = c.reshape(-1)
        return 0

    def mrfa_frames_resize_u8(self, stream, src, N, Hi, Wi, Cin, bounds_h, kk_h, ksize_h, bounds_v, kk_v, ksize_v, Ho, Wo, out_f32, out_u8):
        out_f32, out_u8 = out_f32 or 0, out_u8 or 0
        if not (src and bounds_h and kk_h and bounds_v and kk_v):
            return self._refuse("frames_resize_u8: null pointer")
        if not (out_f32 or out_u8):
            return self._refuse("frames_resize_u8: out_f32 and out_u8 are both null")
        if min(N, Hi, Wi, Ho, Wo) < 1:
            return self._refuse(f"frames_resize_u8: N, Hi, Wi, Ho and Wo must be >= 1 ({N}, {Hi}, {Wi}, {Ho}, {Wo})")
        if Cin not in (1, 3, 4):
            return self._refuse(f"frames_resize_u8: Cin must be 1 (grey), 3 or 4 (the fourth byte is dropped), not {Cin}")
        if not (1 <= ksize_h <= MAX_TAPS and 1 <= ksize_v <= MAX_TAPS):
            return self._refuse(f"frames_resize_u8: ksize_h {ksize_h} and ksize_v {ksize_v} must lie in [1, {MAX_TAPS}]")
        if out_f32 % 4:
            return self._refuse("frames_resize_u8: out_f32 must be 4-byte aligned")
        bh, kh = _view(bounds_h, 2 * Wo, np.int32).reshape(Wo, 2), _view(kk_h, Wo * ksize_h, np.int32).reshape(Wo, ksize_h)
        bv, kv = _view(bounds_v, 2 * Ho, np.int32).reshape(Ho, 2), _view(kk_v, Ho * ksize_v, np.int32).reshape(Ho, ksize_v)
        frames = _view(src, N * Hi * Wi * Cin, np.uint8).reshape(N, Hi, Wi, Cin)
        out = resample_axis(resample_axis(rgb_of(frames), 2, bh, kh), 1, bv, kv)
        if out_f32:
            _view(out_f32, N * 3 * Ho * Wo, f32)[:] = unit(out).reshape(-1)
        if out_u8:
            _view(out_u8, N * Ho * Wo * 3, np.uint8)[:] = out.reshape(-1)
        return 0
