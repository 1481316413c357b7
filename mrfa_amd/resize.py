"""Byte frames brought to the model's size on the device: a decoded clip's uint8 frames, of any size, are cropped to a box and resized in ONE launch
(mrfa_frames_resize_u8, include/mrfa_resize_hip.h) into the fp32 (N,3,H,W) frames every entry of mrfa_amd.infer takes, or into uint8 (N,H,W,3) frames
for PairAugmenter -- with the bytes of Pillow's Image.resize(size, resample, box), to the byte.

The host's share is the coefficient tables of a geometry, computed by the library once per (source size, box, size, filter), uploaded once and kept; a call
with a geometry seen before reads nothing back, waits for nothing and uploads nothing."""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from typing import Optional

import torch

from . import resize_hip

FILTERS = tuple(resize_hip.FILTERS)


def _describe(t) -> str:
    return f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__


class _Tables:
    """the device copy of one geometry's four tables (one int32 tensor) and where each starts"""

    def __init__(self, data: torch.Tensor, offsets, ksize_h: int, ksize_v: int):
        self.data, self.ksize_h, self.ksize_v = data, ksize_h, ksize_v
        base = data.data_ptr()
        self.bounds_h, self.kk_h, self.bounds_v, self.kk_v = (base + 4 * o for o in offsets)


class FrameResizer:
    """FrameResizer(size=(H, W), box=None, filter="bilinear", output="float")(frames_u8, out=None)

    size: (H, W) of the result -- this project's order, not Pillow's (width, height).  box: Pillow's (left, upper, right, lower) in source pixels, floats
    allowed, the region that is resized; None: the whole frame.  One box per call.  filter: "box", "bilinear", "hamming", "bicubic" or "lanczos", Pillow's
    filters of those names.  output: "float" gives fp32 (N,3,H,W) in [0,1] (byte * fl32(1/255), as frames_from_uint8), "uint8" gives uint8 (N,H,W,3).
    A FrameResizer passed as `prepare=` to Animator, BestFrameSearch, find_best_frame, reconstruction or make_animation takes the place of their
    frames_from_uint8, so that they accept byte frames of any size.  For training, FrameResizer(output="uint8") on the (2B,Hi,Wi,C) frames of B pairs,
    viewed as (B,2,H,W,3), feeds PairAugmenter."""

    MAX_GEOMETRIES = 8                                     # cached table sets; the least recently used one goes first

    def __init__(self, size, box=None, filter: str = "bilinear", output: str = "float"):
        if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in size)):
            raise ValueError(f"FrameResizer: size is (H, W), two integers >= 1, not {size!r}")
        if box is not None:
            if not (isinstance(box, (tuple, list)) and len(box) == 4
                    and all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in box)):
                raise ValueError(f"FrameResizer: box is (left, upper, right, lower), four finite numbers in source pixels, or None, not {box!r}")
            if not (0 <= box[0] < box[2] and 0 <= box[1] < box[3]):
                raise ValueError(f"FrameResizer: box (left, upper, right, lower) needs 0 <= left < right and 0 <= upper < lower, not {tuple(box)!r}")
            box = tuple(float(v) for v in box)
        if filter not in resize_hip.FILTERS:
            raise ValueError(f"FrameResizer: filter is one of {FILTERS}, not {filter!r}")
        if output not in ("float", "uint8"):
            raise ValueError(f"FrameResizer: output must be \"float\" or \"uint8\", not {output!r}")
        self.size, self.box, self.filter, self.output = (int(size[0]), int(size[1])), box, filter, output
        self._tables: "OrderedDict[tuple, _Tables]" = OrderedDict()

    def __repr__(self):
        return f"FrameResizer(size={self.size}, box={self.box}, filter={self.filter!r}, output={self.output!r})"

    # ------------------------------------------------------------------------------------------------------------------------- the tables
    def _make_tables(self, Hi: int, Wi: int, device) -> _Tables:
        L, f = resize_hip.lib(), resize_hip.FILTERS[self.filter]
        left, upper, right, lower = (0.0, 0.0, float(Wi), float(Hi)) if self.box is None else self.box
        axes = ((Wi, left, right, self.size[1]), (Hi, upper, lower, self.size[0]))          # horizontal, vertical
        ks = []
        for (n, a, b, m), name in zip(axes, ("horizontal", "vertical")):
            k = L.mrfa_resize_ksize(n, a, b, m, f)
            if k < 0:
                raise ValueError(f"FrameResizer: {self!r} on {Hi} x {Wi} (H x W) frames, {name} axis: {resize_hip.last_error()}")
            ks.append(k)
        offsets, total = [], 0
        for (n, a, b, m), k in zip(axes, ks):
            offsets += [total, total + 2 * m]
            total += 2 * m + m * k
        host = (C.c_int * total)()
        at = lambda o: C.cast(C.addressof(host) + 4 * o, C.POINTER(C.c_int))
        for i, ((n, a, b, m), k) in enumerate(zip(axes, ks)):
            resize_hip.check(L.mrfa_resize_coeffs(n, a, b, m, f, at(offsets[2 * i]), at(offsets[2 * i + 1])), "mrfa_resize_coeffs")
        data = torch.frombuffer(host, dtype=torch.int32).clone().to(device)                  # the one upload of this geometry
        return _Tables(data, offsets, ks[0], ks[1])

    def _tables_for(self, Hi: int, Wi: int, device) -> _Tables:
        key = (Hi, Wi, str(device))
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = self._make_tables(Hi, Wi, device)
            while len(self._tables) > self.MAX_GEOMETRIES:
                self._tables.popitem(last=False)
        else:
            self._tables.move_to_end(key)
        return t

    # ------------------------------------------------------------------------------------------------------------------------- the call
    @torch.no_grad()
    def __call__(self, frames: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """frames: uint8 (N,Hi,Wi,C) or one frame (Hi,Wi,C), C in {1,3,4}: grey fills three channels, a fourth byte is dropped (never read).  out: a
        contiguous tensor of the result's shape and dtype on the frames' device to write into (e.g. a captured program's static input).  One launch."""
        if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() not in (3, 4):
            raise ValueError(f"FrameResizer: frames are a uint8 (N,H,W,C) or (H,W,C) tensor, not {_describe(frames)}")
        if frames.dim() == 3:
            frames = frames[None]
        if frames.shape[3] not in (1, 3, 4) or min(frames.shape) < 1:
            raise ValueError(f"FrameResizer: (N,H,W,C) with N, H, W >= 1 and C in (1, 3, 4) -- grey, RGB, RGBA --, not {tuple(frames.shape)}")
        N, Hi, Wi, Cin = frames.shape
        if self.box is not None and not (self.box[2] <= Wi and self.box[3] <= Hi):
            raise ValueError(f"FrameResizer: box {self.box} (left, upper, right, lower) does not lie in a {Hi} x {Wi} (H x W) frame")
        H, W = self.size
        as_float = self.output == "float"
        shape, dtype = ((N, 3, H, W), torch.float32) if as_float else ((N, H, W, 3), torch.uint8)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=frames.device)
        elif not torch.is_tensor(out) or out.dtype != dtype or tuple(out.shape) != shape or out.device != frames.device or not out.is_contiguous():
            raise ValueError(f"FrameResizer: out is a contiguous {dtype} {shape} tensor on {frames.device}, not {_describe(out)}")
        t = self._tables_for(Hi, Wi, frames.device)
        frames = frames.contiguous()
        resize_hip.check(resize_hip.lib().mrfa_frames_resize_u8(
            resize_hip.stream_ptr(), frames.data_ptr(), N, Hi, Wi, Cin, t.bounds_h, t.kk_h, t.ksize_h, t.bounds_v, t.kk_v, t.ksize_v, H, W,
            out.data_ptr() if as_float else None, None if as_float else out.data_ptr()), "mrfa_frames_resize_u8")
        return out
