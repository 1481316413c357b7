"""Records tests/golden/augment_reference.npz / .json and tests/golden/augment_pillow.npz / .json with Pillow, where the reference checkout is at hand.

(a) augment_reference: the reference's own AllAugmentationTransform(**vox1 augmentation_params) (augmentation.py) run end to end on float clips of two
    frames, random.seed(s) for s in 0..15.  Stored per seed: the parameters it drew, its float32 outputs, and those outputs as bytes.
    Two libraries the reference imports are not installed where this tool runs; each is replaced by a stand-in of a few lines that hands the call on the way
    the real one does:
      skimage.img_as_ubyte        rint(255 x) clipped, as uint8 (the clips here are exact multiples of 1/255: the byte comes back)
      skimage.img_as_float        np.multiply(u8, 1 / 255, dtype=float64)
      skimage.transform.resize / rotate, skimage.util.pad      raise: rotation, resize and crop are off in both configs
      torchvision.transforms.ToPILImage()                      PIL.Image.fromarray(uint8 H x W x 3)
      torchvision.transforms.functional.adjust_brightness / adjust_contrast / adjust_saturation      PIL.ImageEnhance.Brightness / Contrast / Color (f)
      torchvision.transforms.functional.adjust_hue            the H channel of convert("HSV") plus uint8(trunc(255 h) mod 256), merged, convert("RGB")
                                                               (torchvision 0.11.2's in-place uint8 add; numpy 2 refuses np.uint8 of a negative number,
                                                               so the two's-complement wrap is written out)
    The drawn parameters are read off the run itself: the adjust_* stand-ins log (op, factor) in call order, and the flips are the one of the four
    combinations under which Pillow applied to the input frames reproduces the returned clip.
(b) augment_pillow: Pillow applied directly, op by op and order by order, to the small frames the device tests use.
Inputs come from mrfa_amd/utils/prng.py (tests.ref_augment.det_bytes), so only parameters and outputs are stored.

    python tools/make_augment_goldens.py [--reference /path/to/reference]
"""
import argparse
import itertools
import json
import os
import random
import sys
import types

import numpy as np
import PIL
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.ref_augment import det_bytes, to_rgb  # noqa: E402

STAND_INS = {
    "skimage.img_as_ubyte": "rint(255 x) clipped to [0, 255] as uint8",
    "skimage.img_as_float": "np.multiply(u8, 1 / 255, dtype=float64)",
    "skimage.transform.resize, rotate; skimage.util.pad": "raise (off in both configs)",
    "torchvision.transforms.ToPILImage": "PIL.Image.fromarray",
    "torchvision.transforms.functional.adjust_brightness / adjust_contrast / adjust_saturation": "PIL.ImageEnhance.Brightness / Contrast / Color",
    "torchvision.transforms.functional.adjust_hue": "H of convert('HSV') + uint8(trunc(255 h) mod 256), merge, convert('RGB')",
}
LOG = []


def pil_hue(img, h):
    hh, s, v = img.convert("HSV").split()
    nh = np.array(hh, dtype=np.uint8)
    nh += np.uint8(int(h * 255) % 256)
    return Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")


PIL_OP = {"brightness": lambda im, f: ImageEnhance.Brightness(im).enhance(f), "contrast": lambda im, f: ImageEnhance.Contrast(im).enhance(f),
          "saturation": lambda im, f: ImageEnhance.Color(im).enhance(f), "hue": pil_hue}


def pil_chain(rgb: np.ndarray, ops) -> np.ndarray:
    im = Image.fromarray(np.ascontiguousarray(rgb), "RGB")
    for name, v in ops:
        im = PIL_OP[name](im, v)
    return np.array(im)


def install_stand_ins():
    def missing(*a, **k):
        raise RuntimeError("not available: rotation, resize and crop are off in both configs")

    def logged(name):
        def fn(img, f):
            LOG.append((name, float(f)))
            return PIL_OP[name](img, f)
        return fn

    sk, skt, sku = types.ModuleType("skimage"), types.ModuleType("skimage.transform"), types.ModuleType("skimage.util")
    sk.img_as_ubyte = lambda x: np.clip(np.rint(np.asarray(x, dtype=np.float64) * 255.0), 0, 255).astype(np.uint8)
    sk.img_as_float = lambda x: np.multiply(x, 1.0 / 255, dtype=np.float64)
    skt.resize = skt.rotate = sku.pad = missing
    sk.transform, sk.util = skt, sku
    tv, tvt, tvf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")
    tvt.ToPILImage = lambda: (lambda a: Image.fromarray(a, "RGB"))
    tvf.adjust_brightness, tvf.adjust_contrast, tvf.adjust_saturation, tvf.adjust_hue = (logged(n) for n in ("brightness", "contrast", "saturation", "hue"))
    tvt.functional, tv.transforms = tvf, tvt
    sys.modules.update({"skimage": sk, "skimage.transform": skt, "skimage.util": sku, "torchvision": tv, "torchvision.transforms": tvt,
                        "torchvision.transforms.functional": tvf})


VOX1_AUG = {"flip_param": {"horizontal_flip": True, "time_flip": True}, "jitter_param": {"brightness": 0.1, "contrast": 0.1, "saturation": 0.1, "hue": 0.1}}
REF_H, REF_W = 16, 12


def golden_reference(ref_root, out_dir):
    install_stand_ins()
    sys.path.insert(0, ref_root)
    import yaml
    with open(os.path.join(ref_root, "config", "vox1.yaml")) as f:
        aug_params = yaml.safe_load(f)["dataset_params"]["augmentation_params"]
    assert aug_params == VOX1_AUG, aug_params
    import augmentation
    seeds, params, floats = list(range(16)), [], []
    for s in seeds:
        u8 = det_bytes(f"augment/reference/{s}", (2, REF_H, REF_W, 3))
        clip = [np.multiply(f, 1.0 / 255, dtype=np.float32) for f in u8]            # what the reader hands the transform: img_as_float32 frames
        transform = augmentation.AllAugmentationTransform(**aug_params)
        random.seed(s)
        del LOG[:]
        out = transform(clip)
        out = np.stack([np.array(out[0], dtype="float32"), np.array(out[1], dtype="float32")])          # frames_dataset.py:165-166: source, driving
        ops = LOG[:len(LOG) // 2]                                                    # the same chain ran on both frames
        assert LOG[len(LOG) // 2:] == ops and len(ops) == 4
        got = np.clip(np.rint(out.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
        match = [(t, h) for t in (0, 1) for h in (0, 1)
                 if all(np.array_equal(got[k], pil_chain(u8[k ^ t], ops)[:, ::-1] if h else pil_chain(u8[k ^ t], ops)) for k in (0, 1))]
        assert len(match) == 1, (s, match)
        params.append({"seed": s, "time_flip": bool(match[0][0]), "hflip": bool(match[0][1]), "ops": [[n, v] for n, v in ops]})
        floats.append(out)
    floats = np.stack(floats)                                                        # (16, 2, H, W, 3): [:, 0] source, [:, 1] driving
    np.savez_compressed(os.path.join(out_dir, "augment_reference.npz"), out_float=floats,
                        out_bytes=np.clip(np.rint(floats.astype(np.float64) * 255.0), 0, 255).astype(np.uint8))
    with open(os.path.join(out_dir, "augment_reference.json"), "w") as f:
        json.dump({"what": "AllAugmentationTransform(**vox1 augmentation_params) on two-frame float clips, random.seed(seed)", "pillow": PIL.__version__,
                   "numpy": np.__version__, "stand_ins": STAND_INS, "augmentation_params": aug_params, "shape": [2, REF_H, REF_W, 3],
                   "input": "tests.ref_augment.det_bytes('augment/reference/<seed>', shape) * (1 / 255) as float32", "clips": params}, f, indent=1)
    flips = [(p["time_flip"], p["hflip"]) for p in params]
    print("(a)", len(params), "seeds; (time_flip, hflip) seen:", sorted(set(flips)))
    assert {(True, False), (False, True), (False, False)} <= set(flips)


def pillow_cases():
    """(name, H, W, C, ops) of golden (b)"""
    single = [(n, f) for n in ("brightness", "contrast", "saturation") for f in (0.0, 0.9, 1.0, 1.1, 2.0)] + [("hue", h) for h in (-0.5, -0.1, 0.1, 0.5)]
    cases = []
    for H, W, C in ((1, 1, 3), (1, 2, 3), (5, 7, 3), (8, 12, 1), (8, 12, 3), (8, 12, 4), (33, 20, 3)):
        cases += [(f"{n}{v:g}/{H}x{W}x{C}", H, W, C, [(n, v)]) for n, v in single]
    full = {"brightness": 1.07, "contrast": 0.93, "saturation": 1.09, "hue": -0.08}
    for order in itertools.permutations(full):
        cases.append(("order-" + "-".join(o[:3] for o in order) + "/8x12x3", 8, 12, 3, [(n, full[n]) for n in order]))
    for H, W, C in ((5, 7, 4), (33, 20, 1), (96, 128, 3)):
        for order in (("hue", "contrast", "brightness", "saturation"), ("saturation", "brightness", "hue", "contrast")):
            cases.append(("order-" + "-".join(o[:3] for o in order) + f"/{H}x{W}x{C}", H, W, C, [(n, full[n]) for n in order]))
    return cases


def golden_pillow(out_dir):
    arrays, meta = {}, []
    for i, (name, H, W, C, ops) in enumerate(pillow_cases()):
        frame = det_bytes(f"augment/pillow/{H}x{W}x{C}", (H, W, C))
        arrays[f"out{i}"] = pil_chain(to_rgb(frame), ops)
        meta.append({"name": name, "H": H, "W": W, "C": C, "ops": [[n, v] for n, v in ops], "key": f"out{i}"})
    np.savez_compressed(os.path.join(out_dir, "augment_pillow.npz"), **arrays)
    with open(os.path.join(out_dir, "augment_pillow.json"), "w") as f:
        json.dump({"what": "Pillow applied directly to one frame: ImageEnhance.Brightness / Contrast / Color, and the HSV round trip with the uint8 add",
                   "pillow": PIL.__version__, "numpy": np.__version__,
                   "input": "tests.ref_augment.det_bytes('augment/pillow/<H>x<W>x<C>', (H, W, C)); grey fills three channels, alpha is dropped",
                   "cases": meta}, f, indent=1)
    print("(b)", len(meta), "cases")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MRFA_REFERENCE"), required="MRFA_REFERENCE" not in os.environ,
                    help="a checkout of the reference (or MRFA_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    golden_pillow(a.out)
    golden_reference(a.reference, a.out)
    for n in ("augment_reference.npz", "augment_reference.json", "augment_pillow.npz", "augment_pillow.json"):
        print(n, os.path.getsize(os.path.join(a.out, n)), "bytes")
