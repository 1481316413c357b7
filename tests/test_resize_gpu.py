"""FrameResizer and `prepare=` on the GPU (-m gpu): the public object against the numpy specification (tests/ref_resize.py) on a 270x480 input, exactly; an
Animator(graph=True, prepare=...) fed small oversized byte frames against the same Animator fed those frames resized beforehand (the static driving buffer
exactly, the generated frames within the Animator's own run-to-run gate); and prepare=None unchanged."""
import numpy as np
import pytest
import torch

from mrfa_amd import FrameResizer
from mrfa_amd.infer import Animator, frames_from_uint8
from tests import ref_resize as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("name,box", [("bilinear", (100, 7, 370, 267)), ("lanczos", (105.5, 0.0, 375.5, 270.0)), ("bicubic", None)])
def test_frame_resizer_against_the_specification(name, box):
    src = R.det_bytes("resize/gpu/270x480", (2, 270, 480, 3))
    want = R.resize_bytes(src, (64, 48), box, R.FILTERS[name])
    dsrc = torch.from_numpy(src).to(DEV)
    rf, rb = FrameResizer((64, 48), box=box, filter=name), FrameResizer((64, 48), box=box, filter=name, output="uint8")
    gf, gb = rf(dsrc), rb(dsrc)
    assert gf.shape == (2, 3, 64, 48) and gf.dtype == torch.float32 and np.array_equal(gf.cpu().numpy(), R.unit(want))
    assert gb.shape == (2, 64, 48, 3) and gb.dtype == torch.uint8 and np.array_equal(gb.cpu().numpy(), want)
    out = torch.full((2, 3, 64, 48), -7.0, device=DEV)
    assert rf(dsrc, out=out) is out and torch.equal(out, gf)
    tables = rf._tables[(270, 480, DEV)].data
    assert torch.equal(rf(dsrc[0]), gf[:1]) and rf._tables[(270, 480, DEV)].data is tables     # a single frame; the geometry's tables are kept
    if box is None:                                                                            # another source size: its own tables, the same object
        half = np.ascontiguousarray(src[:, :135, :240])
        assert np.array_equal(rf(torch.from_numpy(half).to(DEV)).cpu().numpy(), R.unit(R.resize_bytes(half, (64, 48), None, R.FILTERS[name])))
        assert len(rf._tables) == 2


@pytest.fixture(scope="module")
def model():
    from tests.test_bf16_cache import _dry_model
    return _dry_model().to(DEV)


def test_animator_graph_with_prepare_equals_resizing_first(model):
    from tests.test_clip_modules_gpu import _gate
    B, T, Hi, Wi = 2, 3, 90, 120
    src8 = torch.from_numpy(R.det_bytes("resize/gpu/an/src", (B, Hi, Wi, 3))).to(DEV)
    drv8 = torch.from_numpy(R.det_bytes("resize/gpu/an/drv", (B * T, Hi, Wi, 3))).to(DEV)
    r = FrameResizer((64, 64), box=(20.5, 3.0, 108.25, 88.0), filter="bicubic")
    an = Animator(model, graph=True, corr="direct", prepare=r)
    an.set_source(src8)
    assert torch.equal(an.source, r(src8)) and an.source.shape == (B, 3, 64, 64)
    out8 = an(drv8).clone()                                                                 # captures, the bytes resized into the static buffer
    again8 = an(drv8).clone()                                                               # a replay fed bytes
    want = R.unit(R.resize_bytes(drv8.cpu().numpy(), (64, 64), r.box, R.BICUBIC))
    assert np.array_equal(an._graphs[T][1].cpu().numpy(), want)                             # the static driving buffer holds the specification's floats
    outf = an(r(drv8)).clone()                                                              # the same Animator fed the frames resized beforehand
    assert set(an._graphs) == {T}
    _gate(out8, outf, "Animator(graph=True, prepare=): byte frames vs the same frames resized first")
    _gate(again8, outf, "Animator(graph=True, prepare=): byte frames, replay, vs resized first")


def test_prepare_none_leaves_byte_frames_as_they_were(model):
    B, S = 2, 64
    src8 = torch.from_numpy(R.det_bytes("resize/gpu/none/src", (B, S, S, 3))).to(DEV)
    drv8 = torch.from_numpy(R.det_bytes("resize/gpu/none/drv", (B, S, S, 4))).to(DEV)
    an = Animator(model, graph=True, corr="direct")
    an.set_source(src8)
    an(drv8)
    assert an.prepare is None and torch.equal(an.source, frames_from_uint8(src8)) and torch.equal(an._graphs[1][1], frames_from_uint8(drv8))
    ident = FrameResizer((S, S))                                                            # the identity geometry gives frames_from_uint8's floats
    assert torch.equal(ident(drv8), frames_from_uint8(drv8))
