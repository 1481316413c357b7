"""Writes tests/golden/resize_pillow.npz: Pillow's Image.resize bytes of tests/ref_resize.py's GOLDEN_CASES, so that the GPU tests of the resize kernel
need no Pillow.  Inputs are ref_resize.case_input(...), a pure function of the case; the file holds the outputs, key "<index>", uint8 (Ho,Wo,3), and the
Pillow version that made them.

    python tools/make_resize_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import ref_resize as R  # noqa: E402


def pillow_resize(frame: np.ndarray, size, box, filter_name: str) -> np.ndarray:
    """frame uint8 (Hi,Wi,C), C in {1,3} -> Pillow's bytes (Ho,Wo,3); size = (Ho, Wo)"""
    from PIL import Image
    im = Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame)
    out = np.asarray(im.resize((size[1], size[0]), getattr(Image, filter_name.upper()), box=box))
    return np.repeat(out[..., None], 3, axis=2) if out.ndim == 2 else out


def main():
    import PIL
    arrays = {"pillow_version": np.array(PIL.__version__)}
    for i, (gi, c, name, kind) in enumerate(R.GOLDEN_CASES):
        _, size, box = R.GEOMETRIES[gi]
        arrays[str(i)] = pillow_resize(R.case_input(gi, c, kind)[0], size, box, name)
    path = os.path.join(ROOT, "tests", "golden", "resize_pillow.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
