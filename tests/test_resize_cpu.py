"""FrameResizer and the `prepare=` keyword of the inference callers on CPU memory: the numpy specification of the resize entries (tests/ref_resize.py's
Library) stands where mrfa_amd.resize_hip's library stands, the C-ABI emulator (tests/emu.py) where the model library stands.  The object's checks, its table
cache, out=, the (H, W) order; every caller with prepare= against resizing first and calling it without; prepare=None unchanged; the binding's refusals; and
that the three headers share no name."""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

import mrfa_amd
from mrfa_amd import data_hip, hip, resize_hip
from mrfa_amd.infer import Animator, BestFrameSearch, find_best_frame, frames_from_uint8, make_animation, reconstruction
from mrfa_amd.resize import FrameResizer
from tests import ref_resize as R
from tests.emu import Counting, emulated_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@contextlib.contextmanager
def emulated_resize_hip():
    """the specification as the loaded library of mrfa_amd.resize_hip, behind a proxy that lists its calls"""
    old_lib, old_stream = resize_hip._lib, hip.stream_ptr
    resize_hip._lib = Counting(R.Library())
    hip.stream_ptr = lambda: 0
    try:
        yield resize_hip._lib
    finally:
        resize_hip._lib, hip.stream_ptr = old_lib, old_stream


def names(lib):
    return [c for c, _ in lib.calls if c != "mrfa_data_last_error"]


def frames(tag, shape) -> torch.Tensor:
    return torch.from_numpy(R.det_bytes("resize/cpu/" + tag, shape).copy())


# --------------------------------------------------------------------------------------------------------------------------------- FrameResizer
@pytest.mark.parametrize("output", ["float", "uint8"])
def test_frame_resizer_gives_the_specification_and_size_is_h_w(output):
    src = frames("a", (2, 21, 34, 3))
    box = (2.5, 1.0, 30.25, 20.0)
    with emulated_resize_hip() as lib:
        got = FrameResizer(size=(9, 14), box=box, filter="bicubic", output=output)(src)
        assert names(lib).count("mrfa_frames_resize_u8") == 1                                   # one launch
    want = R.resize_bytes(src.numpy(), (9, 14), box, R.BICUBIC)
    if output == "float":
        assert got.dtype == torch.float32 and got.shape == (2, 3, 9, 14) and np.array_equal(got.numpy(), R.unit(want))
    else:
        assert got.dtype == torch.uint8 and got.shape == (2, 9, 14, 3) and np.array_equal(got.numpy(), want)
    with emulated_resize_hip():
        one = FrameResizer((9, 14), box, "bicubic", output)(src[0])                             # a single frame (H,W,C); positional arguments
        assert torch.equal(one, got[:1])
        for c in (1, 4):
            s = frames(f"c{c}", (1, 21, 34, c))
            g = FrameResizer((9, 14), output="uint8")(s)
            assert np.array_equal(g.numpy(), R.resize_bytes(s.numpy(), (9, 14), None, R.BILINEAR))
        assert FrameResizer((5, 7)).filter == "bilinear" and FrameResizer((5, 7)).output == "float"


def test_frame_resizer_writes_into_out_and_checks_it():
    src = frames("out", (2, 12, 10, 3))
    with emulated_resize_hip():
        for output, shape, dtype in (("float", (2, 3, 6, 5), torch.float32), ("uint8", (2, 6, 5, 3), torch.uint8)):
            r = FrameResizer((6, 5), output=output)
            out = torch.zeros(shape, dtype=dtype)
            assert r(src, out=out) is out and torch.equal(out, r(src))
            for bad in (torch.zeros(shape, dtype=torch.float64), torch.zeros((2, 3, 5, 6), dtype=dtype), torch.zeros(shape + (2,), dtype=dtype)[..., 0],
                        np.zeros(shape)):
                with pytest.raises(ValueError, match="out is a contiguous"):
                    r(src, out=bad)


def test_frame_resizer_refuses_with_the_offending_value():
    for kw, msg in ((dict(size=(0, 4)), r"\(0, 4\)"), (dict(size=(4,)), r"\(4,\)"), (dict(size=(4.0, 4)), "size is"), (dict(size=(4, 4), filter="nearest"), "'nearest'"),
                    (dict(size=(4, 4), output="bytes"), "'bytes'"), (dict(size=(4, 4), box=(0, 0, 4)), r"\(0, 0, 4\)"),
                    (dict(size=(4, 4), box=(3, 0, 3, 4)), "left < right"), (dict(size=(4, 4), box=(-1, 0, 3, 4)), "0 <= left"),
                    (dict(size=(4, 4), box=(0, 0, float("nan"), 4)), "finite")):
        with pytest.raises(ValueError, match=msg):
            FrameResizer(**kw)
    r = FrameResizer((4, 4), box=(0, 0, 9, 9))
    with emulated_resize_hip() as lib:
        with pytest.raises(ValueError, match=r"does not lie in a 8 x 9"):
            r(torch.zeros(1, 8, 9, 3, dtype=torch.uint8))
        for bad in (torch.zeros(1, 8, 9, 3), torch.zeros(8, 9, dtype=torch.uint8), torch.zeros(1, 8, 9, 2, dtype=torch.uint8),
                    torch.zeros(0, 8, 9, 3, dtype=torch.uint8), "frames"):
            with pytest.raises(ValueError, match="FrameResizer"):
                r(bad)
        with pytest.raises(ValueError, match="751 taps"):                                       # the library's refusal, with the geometry around it
            FrameResizer((1, 16), filter="lanczos")(torch.zeros(1, 1, 2000, 3, dtype=torch.uint8))
        assert "mrfa_frames_resize_u8" not in names(lib)


def test_tables_are_made_once_per_geometry_and_the_cache_is_bounded(monkeypatch):
    r = FrameResizer((6, 5), filter="hamming")
    uploads = []
    real = torch.Tensor.to
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: (uploads.append(tuple(self.shape)), real(self, *a, **k))[1])
    with emulated_resize_hip() as lib:
        a, b = frames("cache/a", (1, 12, 10, 3)), frames("cache/b", (3, 12, 10, 1))
        first = r(a)
        assert names(lib) == ["mrfa_resize_ksize", "mrfa_resize_ksize", "mrfa_resize_coeffs", "mrfa_resize_coeffs", "mrfa_frames_resize_u8"]
        assert len(uploads) == 1                                                                # the four tables travel as one tensor
        del lib.calls[:]
        assert torch.equal(r(a), first)
        r(b)                                                                                    # N and C are not part of the geometry
        assert names(lib) == ["mrfa_frames_resize_u8"] * 2 and len(uploads) == 1                # nothing computed, nothing uploaded
        for h in range(20, 20 + FrameResizer.MAX_GEOMETRIES):                                   # as many further geometries as the cache holds
            r(torch.zeros(1, h, 10, 3, dtype=torch.uint8))
        assert len(r._tables) == FrameResizer.MAX_GEOMETRIES and (12, 10, "cpu") not in r._tables
        del lib.calls[:]
        assert torch.equal(r(a), first)                                                         # dropped, so made again: same result
        assert names(lib).count("mrfa_resize_coeffs") == 2 and len(r._tables) == FrameResizer.MAX_GEOMETRIES


# --------------------------------------------------------------------------------------------------------------------------------- the callers
@pytest.fixture(scope="module")
def dry():
    from tests.test_bf16_cache import _dry_model
    with emulated_hip():
        m = _dry_model()
    B, T, Hi, Wi = 2, 3, 80, 100
    src8, clip8 = frames("anim/src8", (B, Hi, Wi, 3)), frames("anim/clip8", (B, T, Hi, Wi, 4))
    return m, src8, clip8


BOX = (10.5, 4.0, 90.0, 76.5)


def resized(r, x):
    """byte frames (N,.,.,C) or a byte clip (B,T,.,.,C) resized beforehand: fp32 (N,3,H,W) / (B,3,T,H,W)"""
    if x.dim() == 4:
        return r(x)
    B, T = x.shape[:2]
    return r(x.reshape(B * T, *x.shape[2:])).view(B, T, 3, *r.size).permute(0, 2, 1, 3, 4).contiguous()


def test_animator_and_best_frame_search_with_prepare_equal_resizing_first(dry):
    m, src8, clip8 = dry
    r = FrameResizer((64, 64), box=BOX, filter="bilinear")
    drv8 = clip8[:, :2].reshape(4, *clip8.shape[2:])
    with emulated_hip(), emulated_resize_hip() as lib:
        a, b = Animator(m, relative=True, prepare=r), Animator(m, relative=True)
        a.set_source(src8, drv8[::2].contiguous())
        b.set_source(resized(r, src8), resized(r, drv8[::2].contiguous()))
        del lib.calls[:]
        out = a(drv8)
        assert names(lib) == ["mrfa_frames_resize_u8"]                                          # one launch; the tables were made for the source
        assert out.shape == (4, 3, 64, 64) and torch.equal(out, b(resized(r, drv8)))
        assert torch.equal(a(resized(r, drv8)), out)                                            # float frames pass through untouched
        s, t = BestFrameSearch(m, prepare=r), BestFrameSearch(m)
        s.set_source(src8)
        t.set_source(resized(r, src8))
        s.add(drv8)
        t.add(resized(r, drv8))
        assert s.result() == t.result()
        assert find_best_frame(m, src8, clip8, frames_per_call=2, prepare=r) == find_best_frame(m, resized(r, src8), resized(r, clip8), frames_per_call=2)
    for bad in (FrameResizer((64, 64), output="uint8"), frames_from_uint8, "resize"):
        with pytest.raises(ValueError, match="prepare is None or a FrameResizer"):
            Animator(m, prepare=bad)
        with pytest.raises(ValueError, match="prepare is None or a FrameResizer"):
            BestFrameSearch(m, prepare=bad)


def test_make_animation_and_reconstruction_with_prepare_equal_resizing_first(dry):
    m, src8, clip8 = dry
    r = FrameResizer((64, 64), box=BOX, filter="bicubic")
    with emulated_hip(), emulated_resize_hip():
        srcf, clipf = resized(r, src8), resized(r, clip8)
        got = make_animation(m, src8, clip8, relative=True, frames_per_call=2, initial_frame="best", prepare=r)
        assert got.shape == (2, 3, 3, 64, 64) and torch.equal(got, make_animation(m, srcf, clipf, relative=True, frames_per_call=2, initial_frame="best"))
        got8 = make_animation(m, src8, clip8, relative=False, frames_per_call=3, output="uint8", prepare=r)
        assert got8.shape == (2, 3, 64, 64, 3) and torch.equal(got8, make_animation(m, srcf, clipf, relative=False, frames_per_call=3, output="uint8"))
        for metrics in ("host", "device"):
            a = reconstruction(m, clip8, frames_per_call=2, metrics=metrics, visualize=True, prepare=r)
            b = reconstruction(m, clipf, frames_per_call=2, metrics=metrics, visualize=True)
            assert set(a) == set(b) and torch.equal(a["prediction"], b["prediction"]) and torch.equal(a["visualization"], b["visualization"])
            assert a["l1"] == b["l1"] and a["psnr"] == b["psnr"]                                # the metrics are taken on the resized floats
        with pytest.raises(ValueError, match="prepare is None or a FrameResizer"):
            make_animation(m, src8, clip8, prepare=FrameResizer((64, 64), output="uint8"))
        with pytest.raises(ValueError, match="prepare is None or a FrameResizer"):
            reconstruction(m, clip8, prepare=3)


def test_prepare_none_is_the_path_as_it_was(dry):
    m, _, _ = dry
    src8, drv8 = frames("none/src8", (2, 64, 64, 3)), frames("none/drv8", (2, 64, 64, 1))
    with emulated_hip(counting=True) as model_lib, emulated_resize_hip() as lib:
        a, b = Animator(m), Animator(m, prepare=None)
        a.set_source(src8)
        b.set_source(frames_from_uint8(src8))
        assert a.prepare is None and torch.equal(a(drv8), b(frames_from_uint8(drv8)))
        assert [c for c, _ in model_lib.calls].count("mrfa_frames_from_u8") == 4
        assert not lib.calls                                                                    # the resize entries are not reached, nor is their library loaded


# --------------------------------------------------------------------------------------------------------------------------------- resize_hip.lib()
class _Entry:
    def __init__(self, value=0):
        self.value = value

    def __call__(self, *args):
        return self.value


def _stand_in(monkeypatch, version, lacks=()):
    """resize_hip.lib() will load a plain object with every symbol of the binding except `lacks`, whose mrfa_resize_version() returns `version`"""
    L = type("StandIn", (), {})()
    for name in resize_hip._SIGNATURES:
        if name not in lacks:
            setattr(L, name, _Entry(version if name == "mrfa_resize_version" else 0))
    monkeypatch.setattr(resize_hip, "_lib", None)
    monkeypatch.setattr(data_hip, "LIB_PATH", os.path.abspath(__file__))
    monkeypatch.setattr(resize_hip.C, "CDLL", lambda path: L)
    return L


@pytest.mark.parametrize("version", [resize_hip.ABI_VERSION - 1, resize_hip.ABI_VERSION + 1])
def test_lib_refuses_a_library_of_another_version(monkeypatch, version):
    _stand_in(monkeypatch, version)
    with pytest.raises(RuntimeError) as err:
        resize_hip.lib()
    assert f"speaks resize ABI version {version}," in str(err.value) and "rebuild the library" in str(err.value)
    assert resize_hip._lib is None


@pytest.mark.parametrize("name", list(resize_hip._SIGNATURES))
def test_lib_refuses_a_library_that_lacks_an_entry(monkeypatch, name):
    _stand_in(monkeypatch, resize_hip.ABI_VERSION, lacks=(name,))
    with pytest.raises(AttributeError) as err:
        resize_hip.lib()
    assert name in str(err.value) and resize_hip._lib is None


def test_lib_accepts_the_matching_stand_in_and_a_missing_file_is_an_error(monkeypatch):
    L = _stand_in(monkeypatch, resize_hip.ABI_VERSION)
    assert resize_hip.lib() is L
    monkeypatch.setattr(resize_hip, "_lib", None)
    monkeypatch.setattr(data_hip, "LIB_PATH", os.path.join(ROOT, "no", "such", "libmrfa_data_hip.so"))
    with pytest.raises(hip.HipLibraryMissing, match="no CPU fallback"):
        resize_hip.lib()


def test_header_binding_and_specification_agree_and_share_no_name_with_the_other_headers():
    header = open(os.path.join(ROOT, "include", "mrfa_resize_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", header).group(1))

    assert define("MRFA_RESIZE_ABI_VERSION") == resize_hip.ABI_VERSION == R.VERSION == R.Library().mrfa_resize_version()
    assert define("MRFA_RESIZE_MAX_TAPS") == resize_hip.MAX_TAPS == R.MAX_TAPS
    for n in ("BOX", "BILINEAR", "HAMMING", "BICUBIC", "LANCZOS"):
        assert define("MRFA_RESIZE_" + n) == getattr(resize_hip, n) == getattr(R, n) == resize_hip.FILTERS[n.lower()] == R.FILTERS[n.lower()]
    code = header[header.index("#ifndef"):]
    declared = set(re.findall(r"\b(mrfa_\w+)\s*\(", code))
    assert declared == set(resize_hip.EXPORTED_SYMBOLS) == {n for n in dir(R.Library) if n.startswith("mrfa_")} - {"mrfa_data_last_error"}
    assert set(resize_hip._SIGNATURES) - declared == {"mrfa_data_last_error"}                   # the one entry of the other group that this binding reads
    data = open(os.path.join(ROOT, "include", "mrfa_data_hip.h")).read()
    model = open(os.path.join(ROOT, "include", "mrfa_hip.h")).read()
    for n in declared:
        assert not re.search(rf"\b{n}\b", data) and not re.search(rf"\b{n}\b", model), n
    assert not declared & set(data_hip._SIGNATURES) and not declared & set(hip._SIGNATURES)
    assert mrfa_amd.FrameResizer is FrameResizer
