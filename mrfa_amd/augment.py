"""Training pairs augmented on the device: a batch of uint8 frame pairs, as the image reader returns them, becomes the fp32 `source` / `driving` batches that
HotPath and train_step take -- the flips and the colour jitter of the reference's AllAugmentationTransform (augmentation.py:325-355; frames_dataset.py:119,161)
in one entry call of libmrfa_data_hip.so (include/mrfa_data_hip.h), with arithmetic that is the reference's Pillow path to the byte.

The host's share is the random draw, which consumes the generator exactly as the reference does per clip (RandomFlip.__call__, ColorJitter.get_params and its
random.shuffle), so that a seed gives the reference's parameters."""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import data_hip

OPS = ("brightness", "contrast", "saturation", "hue")
_SHUFFLED = ("brightness", "saturation", "hue", "contrast")          # the list ColorJitter.__call__ builds and shuffles (augmentation.py:280-288)
_CODE = {"brightness": data_hip.AUG_BRIGHTNESS, "contrast": data_hip.AUG_CONTRAST, "saturation": data_hip.AUG_SATURATION, "hue": data_hip.AUG_HUE}


def _describe(t) -> str:
    return f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__


def hue_shift_of(h: float) -> int:
    """the byte added to H (of HSV) for a hue factor h: trunc(255 h) modulo 256, two's complement for h < 0 -- what the uint8 add of adjust_hue gives"""
    return int(math.trunc(255.0 * h)) % 256


@dataclass(frozen=True)
class PairDraw:
    """one pair's augmentation: the two flips, the factors of the enabled colour ops (None: the op is off) and the order they apply in"""
    time_flip: bool = False
    hflip: bool = False
    brightness: Optional[float] = None
    contrast: Optional[float] = None
    saturation: Optional[float] = None
    hue: Optional[float] = None
    order: Tuple[str, ...] = ()

    def __post_init__(self):
        on = [n for n in OPS if getattr(self, n) is not None]
        if sorted(self.order) != sorted(on):
            raise ValueError(f"PairDraw: order {tuple(self.order)!r} must be a permutation of the ops that have a factor, {tuple(on)!r}")
        for n in ("brightness", "contrast", "saturation"):
            f = getattr(self, n)
            if f is not None and not (math.isfinite(f) and f >= 0):
                raise ValueError(f"PairDraw: the {n} factor must be finite and >= 0, not {f!r}")
        if self.hue is not None and not -0.5 <= self.hue <= 0.5:
            raise ValueError(f"PairDraw: the hue factor lies in [-0.5, 0.5], not {self.hue!r}")

    @property
    def hue_shift(self) -> int:
        return 0 if self.hue is None else hue_shift_of(self.hue)

    def descriptor(self) -> data_hip.PairAug:
        a = data_hip.PairAug()
        for k, n in enumerate(("brightness", "contrast", "saturation")):
            f = getattr(self, n)
            a.factor[k] = 1.0 if f is None else f
        for k in range(4):
            a.op[k] = _CODE[self.order[k]] if k < len(self.order) else data_hip.AUG_NONE
        a.hue_shift, a.time_flip, a.hflip = self.hue_shift, int(bool(self.time_flip)), int(bool(self.hflip))
        return a


@dataclass(frozen=True)
class PairParams:
    """the augmentation of a batch: one PairDraw per pair"""
    pairs: Tuple[PairDraw, ...]

    def __post_init__(self):
        object.__setattr__(self, "pairs", tuple(self.pairs))
        if not self.pairs or not all(isinstance(p, PairDraw) for p in self.pairs):
            raise ValueError("PairParams: pairs is a non-empty sequence of PairDraw")

    def __len__(self):
        return len(self.pairs)


class PairAugmenter:
    """flip_param = {horizontal_flip, time_flip}, jitter_param = {brightness, contrast, saturation, hue}: the reference's augmentation_params (vox1.yaml,
    celebvhq.yaml).  rotation_param, resize_param and crop_param, off in both configs, are not implemented.  rng: a random.Random; None: the random module."""

    def __init__(self, flip_param=None, jitter_param=None, rotation_param=None, resize_param=None, crop_param=None, rng=None):
        for name, v in (("rotation_param", rotation_param), ("resize_param", resize_param), ("crop_param", crop_param)):
            if v is not None:
                raise NotImplementedError(f"PairAugmenter: {name} is not implemented (got {v!r}); only flip_param and jitter_param are")
        self.flip = None if flip_param is None else {"time_flip": bool(flip_param.get("time_flip", False)),
                                                     "horizontal_flip": bool(flip_param.get("horizontal_flip", False))}
        if flip_param is not None and set(flip_param) - {"time_flip", "horizontal_flip"}:
            raise ValueError(f"PairAugmenter: flip_param has the keys time_flip and horizontal_flip, not {sorted(flip_param)}")
        self.jitter = None
        if jitter_param is not None:
            if set(jitter_param) - set(OPS):
                raise ValueError(f"PairAugmenter: jitter_param has the keys {OPS}, not {sorted(jitter_param)}")
            self.jitter = {n: float(jitter_param.get(n, 0)) for n in OPS}
            if not 0 <= self.jitter["hue"] <= 0.5 or any(v < 0 or not math.isfinite(v) for v in self.jitter.values()):
                raise ValueError(f"PairAugmenter: jitter strengths are finite and >= 0, hue at most 0.5, not {jitter_param!r}")
        self.rng = random if rng is None else rng
        self._workspace = {}

    @classmethod
    def from_config(cls, augmentation_params: dict, rng=None):
        """augmentation_params: dataset_params.augmentation_params of a reference config"""
        return cls(rng=rng, **augmentation_params)

    # --------------------------------------------------------------------------------------------------------------------------- the draw
    def _draw_one(self) -> PairDraw:
        rng, kw = self.rng, {}
        if self.flip is not None:                                       # RandomFlip.__call__: a time flip returns early, before the horizontal draw
            kw["time_flip"] = rng.random() < 0.5 and self.flip["time_flip"]
            if not kw["time_flip"]:
                kw["hflip"] = rng.random() < 0.5 and self.flip["horizontal_flip"]
        if self.jitter is not None:                                     # ColorJitter.get_params, then the shuffle of the transform list
            for n in ("brightness", "contrast", "saturation"):
                s = self.jitter[n]
                if s > 0:
                    kw[n] = rng.uniform(max(0, 1 - s), 1 + s)
            if self.jitter["hue"] > 0:
                kw["hue"] = rng.uniform(-self.jitter["hue"], self.jitter["hue"])
            order = [n for n in _SHUFFLED if n in kw]
            rng.shuffle(order)
            kw["order"] = tuple(order)
        return PairDraw(**kw)

    def draw(self, B: int) -> PairParams:
        """the parameters of B pairs, drawn pair by pair as the reference draws them clip by clip"""
        if not isinstance(B, int) or B < 1:
            raise ValueError(f"PairAugmenter.draw: B is an int >= 1, not {B!r}")
        return PairParams(tuple(self._draw_one() for _ in range(B)))

    # --------------------------------------------------------------------------------------------------------------------------- the call
    def _ws(self, device, B, H, W):
        key = (str(device), B, H, W)
        ws = self._workspace.get(key)
        if ws is None:
            n = data_hip.lib().mrfa_pair_augment_workspace(B, H, W)
            if n < 0:
                raise ValueError(f"PairAugmenter: mrfa_pair_augment_workspace refuses B {B}, H {H}, W {W}")
            ws = self._workspace[key] = torch.empty(max(n, 8) // 8, dtype=torch.int64, device=device)
        return ws

    @torch.no_grad()
    def __call__(self, pairs: torch.Tensor, params: Optional[PairParams] = None, out=None):
        """pairs: uint8 (B,2,H,W,C), C in {1,3,4}, frame 0 of a pair the earlier one.  Returns (source, driving), fp32 (B,3,H,W) in [0,1] on the same device.
        params: None draws them (draw(B)).  out = (source, driving): contiguous fp32 (B,3,H,W) tensors to write into (e.g. the static inputs of a
        GraphedTrainStep).  No host read, no synchronisation."""
        if not torch.is_tensor(pairs) or pairs.dtype != torch.uint8 or pairs.dim() != 5 or pairs.shape[1] != 2 or pairs.shape[4] not in (1, 3, 4) \
                or min(pairs.shape) < 1:
            raise ValueError(f"PairAugmenter: pairs are a uint8 (B,2,H,W,C) tensor with C in (1, 3, 4), not {_describe(pairs)}")
        B, _, H, W, Cin = pairs.shape
        if params is None:
            params = self.draw(B)
        if not isinstance(params, PairParams) or len(params) != B:
            raise ValueError(f"PairAugmenter: params are the PairParams of {B} pairs, not {type(params).__name__}"
                             + (f" of {len(params)}" if isinstance(params, PairParams) else ""))
        if out is None:
            out = (torch.empty(B, 3, H, W, device=pairs.device), torch.empty(B, 3, H, W, device=pairs.device))
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 2:
                raise ValueError(f"PairAugmenter: out is the pair (source, driving), not {type(out).__name__}")
            for name, t in zip(("source", "driving"), out):
                if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (B, 3, H, W) or t.device != pairs.device or not t.is_contiguous():
                    raise ValueError(f"PairAugmenter: out's {name} is a contiguous fp32 {(B, 3, H, W)} tensor on {pairs.device}, not {_describe(t)}")
        pairs = pairs.contiguous()
        L = data_hip.lib()
        for b0 in range(0, B, data_hip.AUG_MAX_PAIRS):
            n = min(data_hip.AUG_MAX_PAIRS, B - b0)
            descs = (data_hip.PairAug * n)(*(p.descriptor() for p in params.pairs[b0:b0 + n]))
            ws = self._ws(pairs.device, n, H, W)
            data_hip.check(L.mrfa_pair_augment(data_hip.stream_ptr(), pairs[b0:b0 + n].data_ptr(), n, H, W, Cin, descs, ws.data_ptr(),
                                               ws.numel() * 8, out[0][b0:b0 + n].data_ptr(), out[1][b0:b0 + n].data_ptr()), "mrfa_pair_augment")
        return out[0], out[1]
