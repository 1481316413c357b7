"""tests/ref_resize.py, the numpy specification of the resize entries, against Pillow's Image.resize(size, resample, box) in EVERY byte: all five filters,
grey and RGB, the geometry list of the GPU test, random bytes and a 0/255-only image (bicubic and Lanczos overshoot and clamp).  The specification always
runs both passes; Pillow skips the pass of an axis it need not touch, and the bytes are the same.  CPU; needs Pillow (the GPU tests read the recorded
tests/golden/resize_pillow.npz instead)."""
import os

import numpy as np
import pytest

from tests import ref_resize as R

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pillow(frame, size, box, name):
    from tools.make_resize_golden import pillow_resize
    return pillow_resize(frame, size, box, name)


@pytest.mark.parametrize("name", list(R.FILTERS))
@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=[R.geometry_id(g) for g in R.GEOMETRIES])
def test_specification_equals_pillow_in_every_byte(gi, name):
    _, size, box = R.GEOMETRIES[gi]
    for c in (1, 3):
        for kind in ("random", "extreme"):
            a = R.case_input(gi, c, kind)
            got = R.resize_bytes(a, size, box, R.FILTERS[name])[0]
            want = pillow(a[0], size, box, name)
            assert got.shape == want.shape == (size[0], size[1], 3)
            assert np.array_equal(got, want), (c, kind, int((got != want).sum()))


def test_overshoot_clamps_both_ways():
    """the 0/255-only cases above do reach both clamps: the unclamped sums of bicubic and Lanczos leave [0, 255]"""
    gi = 6                                                               # 17x19 -> 64x64, an upscale: single taps carry negative lobes
    _, size, box = R.GEOMETRIES[gi]
    a = R.rgb_of(R.case_input(gi, 3, "extreme")).astype(np.int64)
    for f in (R.BICUBIC, R.LANCZOS):
        bh, kh, _, _ = R.tables(a.shape[1], a.shape[2], size, box, f)
        acc = np.stack([(a[:, :, x0:x0 + n] * kh[xx, :n].astype(np.int64)[None, None, :, None]).sum(axis=2) for xx, (x0, n) in enumerate(bh)], axis=2)
        v = ((1 << 21) + acc) >> 22
        assert v.min() < 0 and v.max() > 255


@pytest.mark.parametrize("name", list(R.FILTERS))
def test_a_pass_pillow_skips_is_the_identity(name):
    """m == n with a full box: Pillow leaves that axis alone; these coefficients give the identity, so always running both passes changes no byte"""
    f = R.FILTERS[name]
    for n in (1, 2, 7, 256):
        bounds, kk = R.coeffs(n, 0.0, float(n), n, f)
        a = R.det_bytes(f"resize/identity/{n}", (3, n, 2))
        assert np.array_equal(R.resample_axis(a, 1, bounds, kk), a)
    a = R.det_bytes("resize/one-axis", (1, 40, 56, 3))                   # one axis resized, the other skipped by Pillow
    for size in ((40, 20), (13, 56), (40, 56)):
        assert np.array_equal(R.resize_bytes(a, size, None, f)[0], pillow(a[0], size, None, name)), size


def test_channel_conventions():
    a = R.det_bytes("resize/rgba", (2, 9, 11, 4))
    want = R.resize_bytes(a[..., :3].copy(), (5, 7), (1.5, 0.0, 10.0, 8.25), R.BICUBIC)
    assert np.array_equal(R.resize_bytes(a, (5, 7), (1.5, 0.0, 10.0, 8.25), R.BICUBIC), want)        # the fourth byte is never read: NOT premultiplied
    for n in range(2):
        assert np.array_equal(want[n], pillow(a[n, ..., :3], (5, 7), (1.5, 0.0, 10.0, 8.25), "bicubic"))
    g = R.det_bytes("resize/grey", (1, 9, 11, 1))
    out = R.resize_bytes(g, (5, 7), None, R.LANCZOS)
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    u = R.unit(out)
    assert u.dtype == np.float32 and u.shape == (1, 3, 5, 7) and np.array_equal(u[0, 1], out[0, ..., 1].astype(np.float32) * np.float32(1.0 / 255.0))


def test_the_golden_is_what_pillow_gives_now():
    z = np.load(os.path.join(ROOT, "tests", "golden", "resize_pillow.npz"))
    assert len(R.GOLDEN_CASES) == len([k for k in z.files if k.isdigit()])
    for i, (gi, c, name, kind) in enumerate(R.GOLDEN_CASES):
        _, size, box = R.GEOMETRIES[gi]
        assert np.array_equal(z[str(i)], pillow(R.case_input(gi, c, kind)[0], size, box, name)), i
        assert np.array_equal(z[str(i)], R.resize_bytes(R.case_input(gi, c, kind), size, box, R.FILTERS[name])[0]), i
