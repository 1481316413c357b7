"""tests/ref_augment.py, the CPU specification of libmrfa_data_hip.so, against Pillow itself on all 2^24 colours -- luma, the three blends, both HSV
conversions, the hue shift -- and against every committed golden (tools/make_augment_goldens.py; that half needs no Pillow).  No GPU."""
import json
import os

import numpy as np
import pytest

from tests import ref_augment as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTORS = [0.0, 0.9, 1.0, 1.1, 2.0, 0.9428090415820634, 1.0471975511965976]           # ..., sqrt(8) / 3, pi / 3
SHIFTS = [1, 25, 231, 128]


@pytest.fixture(scope="module")
def colours():
    return R.all_colours()


@pytest.fixture(scope="module")
def image(colours):
    from PIL import Image
    return Image.fromarray(colours, "RGB")


def test_luma_is_pillows_convert_L(colours, image):
    assert np.array_equal(np.asarray(image.convert("L")), R.luma(colours))


@pytest.mark.parametrize("f", FACTORS, ids=lambda f: f"f{f:.4g}")
def test_the_three_blends_are_pillows_enhancers(colours, image, f):
    from PIL import ImageEnhance
    assert np.array_equal(np.asarray(ImageEnhance.Brightness(image).enhance(f)), R.brightness(colours, f))
    assert np.array_equal(np.asarray(ImageEnhance.Color(image).enhance(f)), R.saturation(colours, f))
    assert np.array_equal(np.asarray(ImageEnhance.Contrast(image).enhance(f)), R.contrast(colours, f))


def test_rgb_to_hsv_is_pillows(colours, image):
    assert np.array_equal(np.asarray(image.convert("HSV")), R.rgb_to_hsv(colours))


def test_hsv_to_rgb_is_pillows(colours):
    from PIL import Image
    assert np.array_equal(np.asarray(Image.fromarray(colours, "HSV").convert("RGB")), R.hsv_to_rgb(colours))


@pytest.mark.parametrize("shift", SHIFTS)
def test_hue_is_the_hsv_round_trip_with_a_byte_added(colours, image, shift):
    from PIL import Image
    h, s, v = image.convert("HSV").split()
    nh = np.array(h, dtype=np.uint8)
    nh += np.uint8(shift)
    want = np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))
    assert np.array_equal(want, R.hue(colours, shift))


def test_hue_shift_of_a_factor_wraps_like_a_uint8_add():
    assert [R.hue_shift_of(h) for h in (0.1, -0.1, 0.5, -0.5, 0.0, 0.003, -0.003)] == [25, 231, 127, 129, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------------- the committed goldens
def _load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, name + ".npz"))


def test_specification_reproduces_every_pillow_golden():
    meta, arrays = _load("augment_pillow")
    assert len(meta["cases"]) >= 150
    for case in meta["cases"]:
        frame = R.det_bytes(f"augment/pillow/{case['H']}x{case['W']}x{case['C']}", (case["H"], case["W"], case["C"]))
        ops, factor, shift = R.ops_of(case["ops"])
        assert np.array_equal(R.apply_ops(R.to_rgb(frame), ops, factor, shift), arrays[case["key"]]), case["name"]


def test_specification_reproduces_the_reference_transform_golden():
    """the reference's AllAugmentationTransform end to end, seeds 0..15: bytes exact; its floats (b / 255 in float64, cast) within one ulp of b * fl32(1/255)"""
    meta, arrays = _load("augment_reference")
    assert [c["seed"] for c in meta["clips"]] == list(range(16))
    for i, clip in enumerate(meta["clips"]):
        u8 = R.det_bytes(f"augment/reference/{clip['seed']}", tuple(meta["shape"]))
        ops, factor, shift = R.ops_of(clip["ops"])
        s, d = R.pair_augment_bytes(u8[None], [(ops, factor, shift, clip["time_flip"], clip["hflip"])])
        got = np.stack([s[0], d[0]]).transpose(0, 2, 3, 1)
        assert np.array_equal(got, arrays["out_bytes"][i]), clip["seed"]
        assert np.abs(R.unit(got).astype(np.float64) - arrays["out_float"][i].astype(np.float64)).max() <= 2.0 ** -24, clip["seed"]
