"""Frames as bytes on the CPU through the specification of mrfa_frames_from_u8 / mrfa_frames_to_u8 (oracle/capi_emulator.py on oracle/infer_spec.py): the conversions and the Visualizer
grid against numpy written here from the rules of include/mrfa_hip.h, the wiring of make_animation / reconstruction / Animator on the dry model, and
what the entries, Ctx and the public functions refuse."""
import sys

import numpy as np
import pytest
import torch

from mrfa_amd import engine, hip
from mrfa_amd.engine import FrameTile
from mrfa_amd.infer import Animator, BestFrameSearch, Visualizer, frames_from_uint8, frames_to_uint8, make_animation, reconstruction
from mrfa_amd.utils.prng import det_uniform
from oracle.capi_emulator import Emulator
from tests.emu import emulated_hip

FILL = 0x5A


def bytes_of(tag, shape) -> torch.Tensor:
    return (det_uniform(tag, shape, 0, 1) * 256).clamp(0, 255).to(torch.uint8)


def np_from_u8(u8: np.ndarray) -> np.ndarray:
    """(N,H,W,C) uint8 -> (N,3,H,W) fp32: one fp32 multiply by the fp32-rounded reciprocal"""
    f = np.multiply(u8, 1. / 255, dtype=np.float32)
    f = np.repeat(f, 3, axis=3) if u8.shape[3] == 1 else f[..., :3]
    return np.ascontiguousarray(f.transpose(0, 3, 1, 2))


def np_quantise(x: np.ndarray, rounding: str) -> np.ndarray:
    """fp32 samples -> bytes by the header's rule: the fp32 product, rint or trunc, a clip; NaN is 0"""
    with np.errstate(invalid="ignore"):
        p = np.multiply(x, np.float32(255.0), dtype=np.float32)
        r = np.rint(p) if rounding == "nearest" else np.trunc(p)
        return np.where(np.isnan(r), 0, np.clip(r, 0, 255)).astype(np.uint8)


def np_to_u8(x: np.ndarray, rounding: str) -> np.ndarray:
    return np.ascontiguousarray(np_quantise(x, rounding).transpose(0, 2, 3, 1))


def margin_ok(kp: np.ndarray, H: int, W: int, radius: float) -> bool:
    """no pixel of an H x W tile within 1e-3 radius^2 of the edge of a disc (float64): fp32 and float64 then agree on every pixel"""
    rr, cc = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    for x, y in kp.reshape(-1, 2).astype(np.float64):
        if not (np.isfinite(x) and np.isfinite(y)):
            continue
        d = (rr - H * (y + 1) / 2) ** 2 + (cc - W * (x + 1) / 2) ** 2
        if not (np.abs(d - radius ** 2) > 1e-3 * radius ** 2).all():
            return False
    return True


def draw_keypoints(tag, N, K, H, W, radius, lo=-1.1, hi=1.1, fix=lambda kp: None) -> torch.Tensor:
    """(N,K,2) keypoints from a fixed seed, `fix` applied (the cases a test places by hand), redrawn (next seed) until margin_ok holds"""
    for attempt in range(200):
        kp = det_uniform(f"{tag}/{attempt}", (N, K, 2), lo, hi)
        fix(kp)
        if margin_ok(kp.numpy(), H, W, radius):
            return kp
    raise AssertionError("no admissible keypoints in 200 draws")


def np_column(x, kp, radius, colors, border, rounding) -> np.ndarray:
    """one column of the grid, float64 disc test: (N,3,H,W) -> (N,H,W,3)"""
    out = np_to_u8(x, rounding)
    N, H, W = out.shape[:3]
    if kp is not None:
        cq = np_quantise(colors, rounding)
        rr, cc = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
        for n in range(N):
            for k in range(kp.shape[1]):                       # in order: a later keypoint overwrites an earlier one
                x_, y_ = float(kp[n, k, 0]), float(kp[n, k, 1])
                if not (np.isfinite(x_) and np.isfinite(y_)):
                    continue
                inside = (rr - H * (y_ + 1) / 2) ** 2 + (cc - W * (x_ + 1) / 2) ** 2 < radius ** 2
                out[n][inside] = cq[k]
    if border:
        out[:, :, [0, -1]] = 255
    return out


# --------------------------------------------------------------------------------------------------------------------- conversions
@pytest.mark.parametrize("cin", [1, 3, 4])
def test_frames_from_uint8_is_one_multiply(cin):
    with emulated_hip(counting=True) as lib:
        u8 = bytes_of(f"fio/from/{cin}", (8, 5, 7, cin))
        u8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)           # every byte value
        got = frames_from_uint8(u8)
        assert got.dtype == torch.float32 and got.shape == (8, 3, 5, 7) and got.is_contiguous()
        assert torch.equal(got, torch.from_numpy(np_from_u8(u8.numpy())))
        one = frames_from_uint8(u8[1])                                      # a 3-D input is one frame
        assert one.shape == (1, 3, 5, 7) and torch.equal(one[0], got[1])
        assert [c for c, _ in lib.calls].count("mrfa_frames_from_u8") == 2
        into = torch.full((8, 3, 5, 7), -1.0)
        assert frames_from_uint8(u8, out=into) is into and torch.equal(into, got)
    v = np.arange(256, dtype=np.uint8)
    assert (np.multiply(v, 1. / 255, dtype=np.float32) != v.astype(np.float32) / np.float32(255)).any()      # the rule is not the division


@pytest.mark.parametrize("rounding", ["nearest", "floor"])
def test_frames_to_uint8_rounds_and_clamps(rounding):
    x = det_uniform("fio/to", (2, 3, 6, 9), -0.05, 1.05)
    k = np.arange(256, dtype=np.float64)
    ties = ((k[:-1] + 0.5) / 255).astype(np.float32)                       # near the ties of "nearest"
    special = torch.tensor([0.0, -0.0, 1.0, -1e-3, 1.001, float("nan"), float("inf"), -float("inf")])
    x.view(-1)[:255] = torch.from_numpy(ties)
    x.view(-1)[255:263] = special
    with emulated_hip():
        got = frames_to_uint8(x, rounding)
        assert got.dtype == torch.uint8 and got.shape == (2, 6, 9, 3)
        assert torch.equal(got, torch.from_numpy(np_to_u8(x.numpy(), rounding)))
        assert frames_to_uint8(special.view(1, 1, 1, 8).expand(1, 3, 1, 8).contiguous(), rounding)[0, 0, :, 0].tolist() == [0, 0, 255, 0, 255, 0, 255, 0]
        half = torch.tensor([0.5 / 255, 1.5 / 255, 2.5 / 255], dtype=torch.float64).float()
        exact = (half * 255 == torch.tensor([0.5, 1.5, 2.5]))
        q = frames_to_uint8(half.view(1, 1, 1, 3).expand(1, 3, 1, 3).contiguous(), rounding)[0, 0, :, 0]
        for i, (lo, even) in enumerate(((0, 0), (1, 2), (2, 2))):
            if exact[i]:
                assert q[i].item() == (even if rounding == "nearest" else lo)      # half to even / toward zero
        u8 = bytes_of("fio/round-trip", (1, 4, 4, 3))
        assert torch.equal(frames_to_uint8(frames_from_uint8(u8), "nearest"), u8)   # a byte survives the two conversions


# --------------------------------------------------------------------------------------------------------------------- Visualizer
@pytest.mark.parametrize("border", [False, True])
def test_visualizer_grid_against_numpy(border):
    N, H, W, K, R = 2, 20, 24, 6, 5
    src, drv = det_uniform("fio/viz/src", (N, 3, H, W), 0, 1), det_uniform("fio/viz/drv", (N, 3, H, W), 0, 1)
    out = det_uniform("fio/viz/out", (N, 3, H, 2 * W), 0, 1)               # wider: cat([warp_img, out], 3)
    def placed(kp):
        kp[0, 0] = torch.tensor([-0.1, 0.2])
        kp[0, 1] = torch.tensor([-0.03, 0.26])                              # two discs overlap: the later one wins
        kp[1, 2] = torch.tensor([0.98, -0.97])                              # clipped by a corner
        kp[1, 3, 0] = float("nan")                                          # draws nothing
    kp_s, kp_d = draw_keypoints("fio/viz/kps", N, K, H, W, R, fix=placed), draw_keypoints("fio/viz/kpd", N, K, H, W, R)
    assert margin_ok(kp_s.numpy(), H, W, R) and margin_ok(kp_d.numpy(), H, W, R)
    colors = det_uniform("fio/viz/colors", (K, 3), 0, 1)
    with emulated_hip(counting=True) as lib:
        viz = Visualizer(draw_border=border, kp_size=R, colors=colors.numpy())
        assert viz.rounding == "floor"
        grid = viz.visualize(drv, src, out, kp_s={"kp": kp_s}, kp_d=kp_d)
        assert [c for c, _ in lib.calls].count("mrfa_frames_to_u8") == 1    # one entry call per visualize
        plain = Visualizer(draw_border=border).visualize(drv, src, out)
        nearest = Visualizer(rounding="nearest").visualize(drv, src, out)
    assert grid.dtype == torch.uint8 and grid.shape == (N * H, 4 * W, 3)
    cols = [np_column(src.numpy(), kp_s.numpy(), R, colors.numpy(), border, "floor"), np_column(drv.numpy(), kp_d.numpy(), R, colors.numpy(), border, "floor"),
            np_column(out.numpy(), None, R, None, border, "floor")]
    want = np.concatenate([np.concatenate(list(c), axis=0) for c in cols], axis=1)      # images stacked downwards, columns side by side
    assert np.array_equal(grid.numpy(), want)
    assert (want[:H, :W] != np_column(src.numpy(), None, R, None, border, "floor")[0]).any()          # discs were drawn
    nokp = np.concatenate([np.concatenate(list(np_column(t.numpy(), None, R, None, border, "floor")), axis=0) for t in (src, drv, out)], axis=1)
    assert np.array_equal(plain.numpy(), nokp)
    if border:
        assert (grid[:, [0, W - 1, W, 2 * W - 1, 2 * W, 4 * W - 1]] == 255).all() and not (grid[0] == 255).all()       # columns, no rows
    assert np.array_equal(nearest.numpy(), np.concatenate([np.concatenate(list(np_to_u8(t.numpy(), "nearest")), axis=0) for t in (src, drv, out)], axis=1))


def test_visualizer_colours_need_matplotlib_or_colors(monkeypatch):
    src = det_uniform("fio/viz/mpl", (1, 3, 8, 8), 0, 1)
    kp = torch.zeros(1, 4, 2)
    monkeypatch.setitem(sys.modules, "matplotlib", None)                    # absent, wherever this runs
    monkeypatch.setitem(sys.modules, "matplotlib.pyplot", None)
    with emulated_hip():
        with pytest.raises(RuntimeError, match=r"colors=.*\(4,3\)"):
            Visualizer().visualize(src, src, src, kp_s=kp)
        assert Visualizer().visualize(src, src, src).shape == (8, 24, 3)    # without keypoints no colours are needed
        with pytest.raises(ValueError, match="3 colors for 4 keypoints"):
            Visualizer(colors=torch.zeros(3, 3)).visualize(src, src, src, kp_d=kp)
        for bad, msg in ((dict(kp_size=0), "kp_size"), (dict(rounding="round"), "'round'"), (dict(colors=torch.zeros(4, 2)), r"\(4, 2\)")):
            with pytest.raises(ValueError, match=msg):
                Visualizer(**bad)
        with pytest.raises(ValueError, match=r"\(1, 3, 9, 8\)"):
            Visualizer().visualize(src, src, det_uniform("fio/viz/tall", (1, 3, 9, 8), 0, 1))
        with pytest.raises(ValueError, match="kp_s"):
            Visualizer(colors=torch.zeros(4, 3)).visualize(src, src, src, kp_s=torch.zeros(2, 4, 2))


# --------------------------------------------------------------------------------------------------------------------- wiring
@pytest.fixture(scope="module")
def dry():
    from tests.test_bf16_cache import _dry_model
    from tests.test_clip_cpu import _clips
    with emulated_hip():
        m = _dry_model()
    src, clip = _clips(4)
    return m, src, clip


def test_make_animation_uint8_output_and_input(dry):
    m, src, clip = dry
    with emulated_hip(counting=True) as lib:
        base = make_animation(m, src, clip, relative=True, frames_per_call=3)
        assert torch.equal(base, make_animation(m, src, clip, relative=True, frames_per_call=3, output="float")) and base.dtype == torch.float32
        assert not [c for c, _ in lib.calls if c.startswith("mrfa_frames_")]          # the defaults do not touch the new entries
        got = make_animation(m, src, clip, relative=True, frames_per_call=3, output="uint8")
        B, _, T, H, W = clip.shape
        assert got.dtype == torch.uint8 and got.shape == (B, T, H, W, 3)
        want = frames_to_uint8(base.permute(0, 2, 1, 3, 4).reshape(B * T, 3, H, W), "nearest").view(B, T, H, W, 3)
        assert torch.equal(got, want)
        # bytes in: bit for bit the result of their frames_from_uint8 floats in
        src8, clip8 = bytes_of("fio/anim/src8", (B, H, W, 3)), bytes_of("fio/anim/clip8", (B, T, H, W, 4))
        srcf = frames_from_uint8(src8)
        clipf = frames_from_uint8(clip8.view(B * T, H, W, 4)).view(B, T, 3, H, W).permute(0, 2, 1, 3, 4).contiguous()
        assert torch.equal(make_animation(m, src8, clip8, relative=True, frames_per_call=3), make_animation(m, srcf, clipf, relative=True, frames_per_call=3))
        with pytest.raises(ValueError, match="'bytes'"):
            make_animation(m, src, clip, output="bytes")
        with pytest.raises(ValueError, match=r"\(2, 4, 64, 64, 2\)"):
            make_animation(m, src, torch.zeros(B, T, H, W, 2, dtype=torch.uint8))


def test_reconstruction_uint8_output_and_visualization(dry):
    m, _, clip = dry
    B, _, T, H, W = clip.shape
    with emulated_hip():
        for metrics in ("host", "device"):
            base = reconstruction(m, clip, frames_per_call=3, metrics=metrics)
            same = reconstruction(m, clip, frames_per_call=3, metrics=metrics, output="float", visualize=False)
            assert set(base) == set(same) and torch.equal(base["prediction"], same["prediction"]) and base["l1"] == same["l1"] and base["psnr"] == same["psnr"]
            got = reconstruction(m, clip, frames_per_call=3, metrics=metrics, output="uint8", visualize=True)
            assert set(got) == set(base) | {"visualization"}
            want = frames_to_uint8(base["prediction"].permute(0, 2, 1, 3, 4).reshape(B * T, 3, H, W), "floor").view(B, T, H, W, 3)
            assert got["prediction"].dtype == torch.uint8 and torch.equal(got["prediction"], want)
            assert got["l1"] == base["l1"] and got["psnr"] == base["psnr"]                # the metrics are taken on the floats
            vis = got["visualization"]
            assert vis.dtype == torch.uint8 and vis.shape == (T, B * H, 4 * W, 3)
            source_column = frames_to_uint8(clip[:, :, 0].contiguous(), "floor").reshape(B * H, W, 3)
            for t in range(T):
                assert torch.equal(vis[t, :, :W], source_column)
                assert torch.equal(vis[t, :, W:2 * W], frames_to_uint8(clip[:, :, t].contiguous(), "floor").reshape(B * H, W, 3))
                assert torch.equal(vis[t, :, 3 * W:], want[:, t].reshape(B * H, W, 3))
        clip8 = bytes_of("fio/rec/clip8", (B, T, H, W, 1))
        clipf = frames_from_uint8(clip8.view(B * T, H, W, 1)).view(B, T, 3, H, W).permute(0, 2, 1, 3, 4).contiguous()
        a, b = reconstruction(m, clip8, frames_per_call=3, metrics="device"), reconstruction(m, clipf, frames_per_call=3, metrics="device")
        assert torch.equal(a["prediction"], b["prediction"]) and a["l1"] == b["l1"] and a["ssim"] == b["ssim"]
        with pytest.raises(ValueError, match="'bytes'"):
            reconstruction(m, clip, output="bytes")


def test_animator_and_best_frame_take_bytes(dry):
    m, _, _ = dry
    B, H, W = 2, 64, 64
    src8, drv8 = bytes_of("fio/an/src8", (B, H, W, 3)), bytes_of("fio/an/drv8", (2 * B, H, W, 3))
    with emulated_hip(counting=True) as lib:
        a8, af = Animator(m, relative=True), Animator(m, relative=True)
        a8.set_source(src8, drv8[::2].contiguous())
        af.set_source(frames_from_uint8(src8), frames_from_uint8(drv8[::2].contiguous()))
        del lib.calls[:]
        out8 = a8(drv8)
        assert [c for c, _ in lib.calls].count("mrfa_frames_from_u8") == 1
        assert torch.equal(out8, af(frames_from_uint8(drv8)))
        kept = Animator(m, keep_warp=True)
        kept.set_source(src8)
        o = kept(drv8)
        full, warp = kept._frame(frames_from_uint8(drv8), want_warp=True)
        assert torch.equal(o, full) and torch.equal(kept.warp, warp) and warp.shape[:2] == (2 * B, 3) and af.warp is None
        s8, sf = BestFrameSearch(m), BestFrameSearch(m)
        s8.set_source(src8)
        sf.set_source(frames_from_uint8(src8))
        s8.add(drv8)
        sf.add(frames_from_uint8(drv8))
        assert s8.result() == sf.result()
        with pytest.raises(ValueError, match=r"\(64, 64, 3\)"):
            a8(drv8[0])


# --------------------------------------------------------------------------------------------------------------------- refusals
def _tile(src, **kw):
    t = hip.U8Tile()
    t.src, t.H, t.W = src.data_ptr(), src.shape[2], src.shape[3]
    for k, v in kw.items():
        setattr(t, k, v.data_ptr() if torch.is_tensor(v) else v)
    return t


def test_entries_refuse_before_writing():
    emu = Emulator()
    u8 = bytes_of("fio/bad/u8", (1, 4, 6, 3))
    dst = torch.full((1, 3, 4, 6), -7.0)
    for bad, word in ((dict(Cin=2), b"not 2"), (dict(Cin=5), b"not 5"), (dict(N=0), b"N 0"), (dict(W=-1), b"W -1"), (dict(src=None), b"null"),
                      (dict(dst=None), b"null")):
        a = dict(src=u8.data_ptr(), N=1, H=4, W=6, Cin=3, dst=dst.data_ptr())
        a.update(bad)
        assert emu.mrfa_frames_from_u8(0, *a.values()) != 0 and word in emu.mrfa_last_error() and b"frames_from_u8" in emu.mrfa_last_error(), bad
        assert (dst == -7.0).all()
    x, y = det_uniform("fio/bad/x", (1, 3, 4, 6), 0, 1), det_uniform("fio/bad/y", (1, 3, 4, 6), 0, 1)
    kp, colors = torch.zeros(1, 65, 2), torch.zeros(65, 3)
    out = torch.full((1, 8, 12, 3), FILL, dtype=torch.uint8)
    good_kp = dict(kp=kp, K=3, radius=2.0, colors=colors)
    cases = [([_tile(x), _tile(y, x0=5)], {}, b"overlap"),                                  # columns 0..5 and 5..10
             ([_tile(x), _tile(y, y0=3, x0=2)], {}, b"overlap"),
             ([_tile(x, x0=7)], {}, b"outside"), ([_tile(x, y0=5)], {}, b"outside"), ([_tile(x, x0=-1)], {}, b"outside"),
             ([_tile(x, **{**good_kp, "K": 0})], {}, b"K 0"), ([_tile(x, **{**good_kp, "K": 65})], {}, b"K 65"),
             ([_tile(x, **{**good_kp, "radius": 0.0})], {}, b"radius 0"), ([_tile(x, **{**good_kp, "radius": float("nan")})], {}, b"radius nan"),
             ([_tile(x, kp=kp, K=3, radius=2.0)], {}, b"colors == NULL"),
             ([_tile(x)], dict(rounding=2), b"not 2"), ([_tile(x)], dict(n_tiles=0), b"n_tiles 0"), ([_tile(x)] * 9, {}, b"n_tiles 9"),
             ([_tile(x)], dict(dst=None), b"null"), ([_tile(x)], dict(N=0), b"N 0")]
    for tiles, over, word in cases:
        arr = (hip.U8Tile * len(tiles))(*tiles)
        a = dict(tiles=arr, n_tiles=len(tiles), N=1, dst=out.data_ptr(), Hd=8, Wd=12, rounding=0)
        a.update(over)
        assert emu.mrfa_frames_to_u8(0, *a.values()) != 0, word
        assert word in emu.mrfa_last_error() and b"frames_to_u8" in emu.mrfa_last_error(), (word, emu.mrfa_last_error())
        assert (out == FILL).all(), word
    arr = (hip.U8Tile * 2)(_tile(x, y0=1, x0=1), _tile(y, y0=1, x0=7, W=5))
    y5 = y[..., :5].contiguous()
    arr[1].src = y5.data_ptr()
    assert emu.mrfa_frames_to_u8(0, arr, 2, 1, out.data_ptr(), 8, 12, 1) == 0
    want = np.full((1, 8, 12, 3), FILL, dtype=np.uint8)
    want[:, 1:5, 1:7], want[:, 1:5, 7:12] = np_to_u8(x.numpy(), "floor"), np_to_u8(y5.numpy(), "floor")
    assert np.array_equal(out.numpy(), want)                                               # bytes that no tile covers are not written


def test_ctx_and_public_functions_refuse_with_the_offending_value():
    x = det_uniform("fio/ctx/x", (2, 3, 4, 6), 0, 1)
    u8 = bytes_of("fio/ctx/u8", (2, 4, 6, 3))
    with emulated_hip(counting=True) as lib:
        e = engine.Ctx(torch.device("cpu"), train=False, record=False)
        for bad, msg in ((u8.float(), "float32"), (u8.int(), "int32"), (u8[..., :2], r"\(2, 4, 6, 2\)"), (u8[0, 0], r"\(6, 3\)"), (u8.numpy(), "ndarray")):
            with pytest.raises(ValueError, match=msg):
                frames_from_uint8(bad)
        with pytest.raises(ValueError, match="float32"):
            frames_from_uint8(x.permute(0, 2, 3, 1).contiguous())                          # fp32 NHWC is not byte frames
        with pytest.raises(ValueError, match=r"\(2, 4, 6, 3\)"):
            frames_to_uint8(x.permute(0, 2, 3, 1).contiguous())                            # and not planar frames either
        for bad, msg in ((x.double(), "float64"), (u8, "uint8"), (x[0], r"\(3, 4, 6\)")):
            with pytest.raises(ValueError, match=msg):
                frames_to_uint8(bad)
        with pytest.raises(ValueError, match="'round'"):
            frames_to_uint8(x, rounding="round")
        with pytest.raises(ValueError, match="strided"):
            e.frames_from_u8(u8[:, :, ::2])
        with pytest.raises(ValueError, match=r"\(2, 3, 4, 7\)"):
            e.frames_from_u8(u8, out=torch.zeros(2, 3, 4, 7))
        kp, colors = torch.zeros(2, 3, 2), torch.zeros(3, 3)
        for tiles, kw, msg in (([FrameTile(x), FrameTile(x, 0, 5)], {}, "overlap"), ([FrameTile(x, -1, 0)], {}, "-1"),
                               ([FrameTile(x, 0, 8)], dict(out=torch.zeros(2, 4, 12, 3, dtype=torch.uint8)), r"column 14.*4 x 12"),
                               ([FrameTile(x, kp=torch.zeros(2, 0, 2), radius=2.0, colors=colors)], {}, r"\(K 0\)"),
                               ([FrameTile(x, kp=torch.zeros(2, 65, 2), radius=2.0, colors=torch.zeros(65, 3))], {}, r"\(K 65\)"),
                               ([FrameTile(x, kp=kp, radius=0, colors=colors)], {}, "not 0"), ([FrameTile(x, kp=kp, radius=2.0)], {}, "NoneType"),
                               ([FrameTile(x)] * 9, {}, "not 9"), ([], {}, "not 0"), ([FrameTile(x[:1])] + [FrameTile(x, 0, 6)], {}, r"\(2, 3, 4, 6\)"),
                               ([FrameTile(x)], dict(rounding="up"), "'up'"), ([FrameTile(x)], dict(out=torch.zeros(2, 4, 6, 3)), "float32")):
            with pytest.raises(ValueError, match=msg):
                e.frames_to_u8(tiles, **kw)
        rec = engine.Ctx(torch.device("cpu"), train=False, record=True)
        with pytest.raises(RuntimeError, match="no backward"):
            rec.frames_from_u8(u8)
        with pytest.raises(RuntimeError, match="no backward"):
            rec.frames_to_u8([FrameTile(x)])
        assert not [c for c, _ in lib.calls if c.startswith("mrfa_frames_")]               # all of it before any launch
        # a fresh output is zero where no tile lies
        got = e.frames_to_u8([FrameTile(x, 1, 0), FrameTile(x, 1, 7)], rounding="floor")
        assert got.shape == (2, 5, 13, 3) and (got[:, 0] == 0).all() and (got[:, :, 6] == 0).all()
        assert np.array_equal(got[:, 1:, 7:].numpy(), np_to_u8(x.numpy(), "floor"))


def test_the_header_and_the_binding_agree():
    assert {"mrfa_frames_from_u8", "mrfa_frames_to_u8"} <= set(hip.EXPORTED_SYMBOLS)
    import ctypes as C
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mrfa_hip.h")).read()
    assert int(re.search(r"#define MRFA_U8_MAX_TILES\s+(\d+)", hdr).group(1)) == hip.U8_MAX_TILES == 8
    assert int(re.search(r"#define MRFA_U8_MAX_KP\s+(\d+)", hdr).group(1)) == hip.U8_MAX_KP == 64
    body = re.search(r"typedef struct \{([^}]*)\} mrfa_u8_tile;", hdr).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("*", " ").split(None, 2 if "const" in decl else 1)[-1].split(",")]
    assert fields == [f[0] for f in hip.U8Tile._fields_] and C.sizeof(hip.U8Tile) == 56
