"""Frames as bytes on the GPU (-m gpu): mrfa_frames_from_u8 / mrfa_frames_to_u8 against the numpy rules of tests/test_frame_io_cpu.py, exactly
(torch.equal, no tolerance), on widths and offsets that take every load and store path; discs and border; the emulator against the kernels; bit identity;
a captured pair replayed on changing bytes; and the module level on the dry model."""
import numpy as np
import pytest
import torch

from mrfa_amd import hip
from mrfa_amd.engine import Ctx, FrameTile
from mrfa_amd.infer import Animator, frames_from_uint8, frames_to_uint8, make_animation, reconstruction
from mrfa_amd.utils.prng import det_uniform
from oracle.capi_emulator import Emulator
from tests.test_frame_io_cpu import FILL, bytes_of, draw_keypoints, margin_ok, np_column, np_from_u8, np_to_u8

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROUNDINGS = ("nearest", "floor")


def _ctx():
    return Ctx(torch.device(DEV), train=False, record=False)


# --------------------------------------------------------------------------------------------------------------------- from_u8
def all_bytes(N, H, W, cin) -> torch.Tensor:
    """(N,H,W,cin) bytes: channel c of pixel p holds (37 p + 85 c) % 256 -- 37 is odd, so any 256 consecutive pixels show every value in every channel"""
    p = torch.arange(N * H * W, dtype=torch.int64)[:, None]
    return ((37 * p + 85 * torch.arange(cin)[None, :]) % 256).to(torch.uint8).view(N, H, W, cin)


# odd widths; a single column; W % 4 == 0 (four pixels per lane); whole vectors and a tail of two
FROM_SHAPES = [(2, 5, 7), (1, 3, 1), (2, 16, 64), (1, 4, 130)]


@pytest.mark.parametrize("cin", [1, 3, 4])
@pytest.mark.parametrize("shape", FROM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_from_u8_is_the_fp32_multiply(shape, cin):
    N, H, W = shape
    u8 = all_bytes(N, H, W, cin)
    if N * H * W >= 256:
        assert all(len(set(u8[..., c].reshape(-1).tolist())) == 256 for c in range(cin))
    want = torch.from_numpy(np_from_u8(u8.numpy()))
    got = frames_from_uint8(u8.to(DEV))
    assert got.shape == (N, 3, H, W) and got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    assert torch.equal(frames_from_uint8(u8.to(DEV)).cpu(), got.cpu())                     # two runs, bit for bit


@pytest.mark.parametrize("cin", [1, 3, 4])
def test_from_u8_source_at_an_odd_address(cin):
    """W % 4 == 0 and an aligned dst, but src one byte past an aligned allocation: the pixel-per-lane path; the floats behind dst keep their canary"""
    N, H, W = 2, 16, 64
    u8 = all_bytes(N, H, W, cin)
    buf = torch.zeros(u8.numel() + 1, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[1:].copy_(u8.view(-1))
    dst = torch.full((N * 3 * H * W + 64,), -7.0, device=DEV)
    hip.check(hip.lib().mrfa_frames_from_u8(hip.stream_ptr(), buf.data_ptr() + 1, N, H, W, cin, dst.data_ptr()), "mrfa_frames_from_u8")
    assert torch.equal(dst[:-64].view(N, 3, H, W).cpu(), torch.from_numpy(np_from_u8(u8.numpy()))) and (dst[-64:] == -7.0).all()


# --------------------------------------------------------------------------------------------------------------------- to_u8
def special_values() -> torch.Tensor:
    """for k in 0..255: fl32(k / 255) and its two fp32 neighbours; every fp32 s within 4 steps of fl32((k + 0.5) / 255) whose fp32 product with 255 is
    EXACTLY k + 0.5 (the ties), with its two neighbours; and 0, -0.0, 1, -1e-3, 1.001, NaN, +inf, -inf"""
    f = np.float32
    vals, ties = [], {}
    for k in range(256):
        s = f(k / 255)
        vals += [np.nextafter(s, f(-np.inf)), s, np.nextafter(s, f(np.inf))]
        if k == 255:
            break
        c = f((k + 0.5) / 255)
        cand = [c]
        for _ in range(4):
            cand = [np.nextafter(cand[0], f(-np.inf))] + cand + [np.nextafter(cand[-1], f(np.inf))]
        for s in cand:
            if np.multiply(s, f(255.0), dtype=f) == f(k + 0.5):
                ties.setdefault(k, []).append(s)
                vals += [np.nextafter(s, f(-np.inf)), s, np.nextafter(s, f(np.inf))]
    # half to even must show in both directions: ties that round down (k even) and up (k odd)
    assert any(k % 2 == 0 for k in ties) and any(k % 2 == 1 for k in ties) and len(ties) >= 128, len(ties)
    vals += [f(0.0), f(-0.0), f(1.0), f(-1e-3), f(1.001), f(np.nan), f(np.inf), f(-np.inf)]
    return torch.from_numpy(np.array(vals, dtype=f))


_VALS = {}


def filled(N, H, W, off) -> torch.Tensor:
    """(N,3,H,W) fp32 cycling through special_values() from offset `off`"""
    if "v" not in _VALS:
        _VALS["v"] = special_values()
    v = _VALS["v"]
    idx = (torch.arange(N * 3 * H * W) + off) % v.numel()
    return v[idx].view(N, 3, H, W)


def rows_for(W) -> int:
    """enough rows that ONE plane of width W holds every special value"""
    if "v" not in _VALS:
        _VALS["v"] = special_values()
    return -(-_VALS["v"].numel() // W)


def _grids():
    """name -> (N, Hd, Wd, [(H, W, y0, x0)]): 3 Wd % 4 takes 0, 1, 2, 3; x0 in {0, 1, 3} and beyond; y0 > 0; two, three and eight tiles"""
    h5, h7, h64, h130 = rows_for(5), rows_for(7), rows_for(64), rows_for(130)
    g = {"two-Wd15": (2, h5 + 3, 15, [(h5, 5, 1, 1), (h7, 7, 2, 7)]),                                   # 3 Wd % 4 == 1
         "three-Wd200": (1, h64 + 2, 200, [(h64, 64, 1, 0), (h130, 130, 1, 64), (9, 5, 2, 195)]),          # == 0: aligned rows, dword stores
         "two-Wd77": (2, h64 + 4, 77, [(h64, 64, 3, 3), (9, 7, 1, 68)]),                                  # == 3, odd x0
         "eight-Wd302": (1, h130 + 2, 302, [(h130, 130, 1, 1), (5, 64, 1, 132), (6, 7, 1, 197), (7, 5, 1, 205), (3, 64, 1, 211), (4, 5, 9, 197),
                                          (2, 7, 9, 203), (9, 20, 1, 276)])}                               # == 2
    assert sorted(3 * v[2] % 4 for v in g.values()) == [0, 1, 2, 3]
    return g


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("name", ["two-Wd15", "three-Wd200", "two-Wd77", "eight-Wd302"])
def test_to_u8_rounds_exactly_and_writes_only_its_tiles(name, rounding):
    N, Hd, Wd, geo = _grids()[name]
    srcs = [filled(N, H, W, 1009 * i) for i, (H, W, _, _) in enumerate(geo)]
    assert srcs[0].shape[2] * srcs[0].shape[3] >= _VALS["v"].numel()                        # one plane holds them all
    want = np.full((N, Hd, Wd, 3), FILL, dtype=np.uint8)
    for s, (H, W, y0, x0) in zip(srcs, geo):
        want[:, y0:y0 + H, x0:x0 + W] = np_to_u8(s.numpy(), rounding)
    covered = np.zeros((Hd, Wd), dtype=bool)
    for H, W, y0, x0 in geo:
        assert y0 > 0 and not covered[y0:y0 + H, x0:x0 + W].any()
        covered[y0:y0 + H, x0:x0 + W] = True
    assert not covered.all()
    dev = [s.to(DEV) for s in srcs]
    if name == "two-Wd77":                                                                  # W % 4 == 0 but src only 4-byte aligned: scalar loads
        buf = torch.zeros(dev[0].numel() + 1, device=DEV)
        buf[1:].copy_(dev[0].view(-1))
        dev[0] = buf[1:].view_as(dev[0])
        assert dev[0].data_ptr() % 16 == 4
    outs = []
    for _ in range(2):
        out = torch.full((N, Hd, Wd, 3), FILL, dtype=torch.uint8, device=DEV)
        got = _ctx().frames_to_u8([FrameTile(s, y0, x0) for s, (_, _, y0, x0) in zip(dev, geo)], out=out, rounding=rounding)
        assert got is out
        outs.append(out.cpu())
    assert torch.equal(outs[0], torch.from_numpy(want))                                     # every tile exact AND every other byte still 0x5A
    assert (outs[0].numpy()[:, ~covered] == FILL).all()
    assert torch.equal(outs[0], outs[1])                                                    # two runs, bit for bit


def test_to_u8_ties_go_to_even():
    f = np.float32
    ties = [s for s in special_values().numpy() if np.isfinite(s) and np.multiply(s, f(255.0), dtype=f) % 1 == f(0.5)]
    x = torch.from_numpy(np.array(ties, dtype=f))
    x = x.view(1, 1, 1, -1).expand(1, 3, 1, -1).contiguous()
    p = np.multiply(np.array(ties, dtype=f), f(255.0), dtype=f).astype(np.float64)
    near, floor = (frames_to_uint8(x.to(DEV), r).cpu()[0, 0, :, 0].numpy().astype(np.float64) for r in ROUNDINGS)
    assert (floor == p - 0.5).all() and (near % 2 == 0).all() and (np.abs(near - p) == 0.5).all()
    assert (near == p - 0.5).any() and (near == p + 0.5).any()                             # both directions occur


# --------------------------------------------------------------------------------------------------------------------- discs and border
H_D, W_D, K_D, R_D = 32, 48, 10, 5.0


def _px(col, row):
    """pixel centre (col, row) of the 32 x 48 tile as a keypoint: cx = W (x + 1) / 2"""
    return torch.tensor([2 * col / W_D - 1, 2 * row / H_D - 1])


def _disc_keypoints() -> torch.Tensor:
    def placed(kp):
        kp[0, 0] = _px(23.5, 15.5)                                                          # the centre of the pixel grid ((0, 0): the test below)
        kp[0, 1], kp[0, 2] = _px(1.3, 0.8), _px(W_D - 1.7, 1.2)                             # the four corners: clipped on two sides
        kp[0, 3], kp[0, 4] = _px(0.6, H_D - 1.4), _px(W_D - 0.9, H_D - 0.7)
        kp[0, 5] = _px(W_D + 9.3, 11.2)                                                     # entirely outside (towards the right neighbour)
        kp[0, 6] = torch.tensor([float("nan"), 0.1])
        kp[0, 7], kp[0, 8] = _px(20.3, 20.6), _px(23.1, 22.4)                               # two that overlap: 8 wins
        kp[0, 9] = _px(40.2, 8.3)                                                           # (away from the others)
        kp[1, 0], kp[1, 1] = _px(24.4, 1.1), _px(25.1, H_D - 1.1)                          # the four edges
        kp[1, 2], kp[1, 3] = _px(0.7, 15.3), _px(W_D - 1.2, 17.9)
        kp[1, 4] = torch.tensor([0.3, float("inf")])
    return draw_keypoints("fio/gpu/discs", 2, K_D, H_D, W_D, R_D, fix=placed)


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("border", [False, True])
def test_discs_and_border(border, rounding):
    kp = _disc_keypoints()
    assert margin_ok(kp.numpy(), H_D, W_D, R_D)                                             # fp32 and float64 agree on every pixel
    mid = det_uniform("fio/gpu/disc/mid", (2, 3, H_D, W_D), 0, 1)
    left, right = det_uniform("fio/gpu/disc/left", (2, 3, H_D, 16), 0, 1), det_uniform("fio/gpu/disc/right", (2, 3, H_D, 16), 0, 1)
    colors = det_uniform("fio/gpu/disc/colors", (K_D, 3), 0, 1)
    cols = [np_column(left.numpy(), None, R_D, None, False, rounding), np_column(mid.numpy(), kp.numpy(), R_D, colors.numpy(), border, rounding),
            np_column(right.numpy(), None, R_D, None, False, rounding)]
    want = np.concatenate(cols, axis=2)
    plain = np_column(mid.numpy(), None, R_D, None, False, rounding)
    drawn = (cols[1] != plain).any(axis=3)
    assert drawn[0, 13:18, 21:26].all() and drawn[0, 0, 0] and drawn[0, H_D - 1, W_D - 1] and drawn[1, 0, 24] and drawn[1, 16, 0]      # centre, corners, edges
    tiles = [FrameTile(left.to(DEV), 0, 0), FrameTile(mid.to(DEV), 0, 16, kp=kp.to(DEV), radius=R_D, colors=colors.to(DEV), border=border),
             FrameTile(right.to(DEV), 0, 16 + W_D)]
    got = _ctx().frames_to_u8(tiles, rounding=rounding).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, :, :16], cols[0]) and np.array_equal(got[:, :, 16 + W_D:], cols[2])     # the neighbours' pixels stay their own
    cq = np_column(colors.numpy().reshape(1, K_D, 1, 3).transpose(0, 3, 1, 2), None, R_D, None, False, rounding)[0, :, 0]      # (K,3) quantised
    assert (got[0, 21, 16 + 22] == cq[8]).all() and (got[0, 20, 16 + 18] == cq[7]).all()                # the overlap is 8's, beside it 7's
    if border:
        assert (got[:, :, [16, 16 + W_D - 1]] == 255).all()


def test_disc_at_the_exact_centre():
    """keypoint (0, 0): cx = 24 and cy = 16 exactly, every r - cy and c - cx an integer and every sum of squares an integer below 2^24: fp32 and float64
    compute the same numbers, so this keypoint needs no margin.  Pixels (16 +- 3, 24 +- 4) and (16 +- 4, 24 +- 3) lie ON the circle (9 + 16 = 25): the
    test is <, they are not drawn"""
    x = det_uniform("fio/gpu/disc/exact", (1, 3, H_D, W_D), 0.25, 0.75)
    colors = torch.tensor([[1.0, 0.0, 1.0]])
    got = _ctx().frames_to_u8([FrameTile(x.to(DEV), kp=torch.zeros(1, 1, 2, device=DEV), radius=R_D, colors=colors.to(DEV))], rounding="floor").cpu().numpy()
    rr, cc = np.arange(H_D)[:, None], np.arange(W_D)[None, :]
    inside = (rr - 16) ** 2 + (cc - 24) ** 2 < 25
    want = np_to_u8(x.numpy(), "floor")
    want[0][inside] = (255, 0, 255)
    assert np.array_equal(got, want) and inside.sum() == 69 and not inside[19, 28] and inside[19, 27]


# --------------------------------------------------------------------------------------------------------------------- the emulator and the kernels
def test_emulator_equals_the_kernels():
    emu = Emulator()
    u8 = bytes_of("fio/gpu/emu/u8", (2, 6, 10, 4))
    spec = torch.full((2, 3, 6, 10), -1.0)
    assert emu.mrfa_frames_from_u8(0, u8.data_ptr(), 2, 6, 10, 4, spec.data_ptr()) == 0
    assert torch.equal(frames_from_uint8(u8.to(DEV)).cpu(), spec)
    kp = _disc_keypoints()
    x, y = filled(2, H_D, W_D, 77), det_uniform("fio/gpu/emu/y", (2, 3, H_D, 7), -0.1, 1.1)
    colors = det_uniform("fio/gpu/emu/colors", (K_D, 3), 0, 1)
    for rounding in ROUNDINGS:
        def compose(lib, stream, to):
            xs, ys, kps, cs = (to(t) for t in (x, y, kp, colors))
            out = to(torch.full((2, H_D + 1, W_D + 9, 3), FILL, dtype=torch.uint8))
            arr = (hip.U8Tile * 2)()
            arr[0].src, arr[0].H, arr[0].W, arr[0].y0, arr[0].x0, arr[0].border = xs.data_ptr(), H_D, W_D, 1, 1, 1
            arr[0].kp, arr[0].K, arr[0].radius, arr[0].colors = kps.data_ptr(), K_D, R_D, cs.data_ptr()
            arr[1].src, arr[1].H, arr[1].W, arr[1].y0, arr[1].x0 = ys.data_ptr(), H_D, 7, 0, W_D + 2
            assert lib.mrfa_frames_to_u8(stream, arr, 2, 2, out.data_ptr(), H_D + 1, W_D + 9, hip.U8_ROUNDINGS[rounding]) == 0
            return out.cpu()
        assert torch.equal(compose(hip.lib(), hip.stream_ptr(), lambda t: t.to(DEV)), compose(emu, 0, lambda t: t.clone()))


def test_kernels_refuse_bad_arguments_and_write_nothing():
    L = hip.lib()
    x = det_uniform("fio/gpu/bad/x", (1, 3, 4, 6), 0, 1).to(DEV)
    u8 = bytes_of("fio/gpu/bad/u8", (1, 4, 6, 3)).to(DEV)
    dst, out = torch.full((1, 3, 4, 6), -7.0, device=DEV), torch.full((1, 8, 12, 3), FILL, dtype=torch.uint8, device=DEV)
    for cin in (0, 2, 5):
        assert L.mrfa_frames_from_u8(hip.stream_ptr(), u8.data_ptr(), 1, 4, 6, cin, dst.data_ptr()) != 0 and f"not {cin}".encode() in L.mrfa_last_error()
    assert L.mrfa_frames_from_u8(hip.stream_ptr(), None, 1, 4, 6, 3, dst.data_ptr()) != 0
    kp, colors = torch.zeros(1, 65, 2, device=DEV), torch.zeros(65, 3, device=DEV)

    def tile(**kw):
        t = hip.U8Tile()
        t.src, t.H, t.W = x.data_ptr(), 4, 6
        for k, v in kw.items():
            setattr(t, k, v)
        return t
    kpargs = dict(kp=kp.data_ptr(), K=3, radius=2.0, colors=colors.data_ptr())
    for tiles, rounding, word in (([tile(), tile(x0=5)], 0, b"overlap"), ([tile(x0=7)], 0, b"outside"), ([tile(**{**kpargs, "K": 0})], 0, b"K 0"),
                                  ([tile(**{**kpargs, "K": 65})], 0, b"K 65"), ([tile(**{**kpargs, "radius": 0.0})], 0, b"radius 0"),
                                  ([tile(**{**kpargs, "colors": None})], 0, b"colors == NULL"), ([tile()], 2, b"not 2"), ([tile()] * 9, 0, b"n_tiles 9")):
        arr = (hip.U8Tile * len(tiles))(*tiles)
        assert L.mrfa_frames_to_u8(hip.stream_ptr(), arr, len(tiles), 1, out.data_ptr(), 8, 12, rounding) != 0 and word in L.mrfa_last_error(), word
    torch.cuda.synchronize()
    assert (dst == -7.0).all() and (out == FILL).all()


# --------------------------------------------------------------------------------------------------------------------- capture
def test_captured_pair_replays_on_changing_bytes():
    from mrfa_amd import graph_replay_safe
    graph_replay_safe("test_frame_io_gpu")
    N, H, W = 2, 12, 20
    src = all_bytes(N, H, W, 3).to(DEV)
    e = _ctx()
    fl = e.frames_from_u8(src)                                                              # warm: the library is loaded outside the capture
    out = e.frames_to_u8([FrameTile(fl, 1, 3)], out=torch.full((N, H + 2, W + 5, 3), FILL, dtype=torch.uint8, device=DEV), rounding="nearest")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        e.frames_from_u8(src, out=fl)
        e.frames_to_u8([FrameTile(fl, 1, 3)], out=out, rounding="nearest")
    for k in range(3):
        fresh = bytes_of(f"fio/gpu/capture/{k}", (N, H, W, 3))
        src.copy_(fresh.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu()
        assert torch.equal(got[:, 1:H + 1, 3:W + 3], fresh), k                              # byte -> float -> nearest byte is the identity: this replay's bytes
        assert torch.equal(fl.cpu(), torch.from_numpy(np_from_u8(fresh.numpy()))), k
        got[:, 1:H + 1, 3:W + 3] = FILL
        assert (got == FILL).all()


# --------------------------------------------------------------------------------------------------------------------- module level
@pytest.fixture(scope="module")
def model():
    from tests.test_bf16_cache import _dry_model
    return _dry_model().to(DEV)


def test_animator_graph_takes_bytes(model):
    from tests.test_clip_modules_gpu import _gate
    B, T, S = 2, 3, 64
    src8, drv8 = bytes_of("fio/gpu/an/src", (B, S, S, 3)).to(DEV), bytes_of("fio/gpu/an/drv", (B * T, S, S, 3)).to(DEV)
    an = Animator(model, graph=True, corr="direct")
    an.set_source(src8)
    out8 = an(drv8).clone()                                                                 # captures, the bytes converted into the static buffer
    again8 = an(drv8).clone()                                                               # a replay fed bytes
    outf = an(frames_from_uint8(drv8)).clone()                                              # the same Animator fed the floats
    assert set(an._graphs) == {T}
    _gate(out8, outf, "Animator(graph=True): uint8 frames vs their frames_from_uint8 floats")
    _gate(again8, outf, "Animator(graph=True): uint8 frames, replay, vs floats")
    assert torch.equal(an._graphs[T][1].cpu(), torch.from_numpy(np_from_u8(drv8.cpu().numpy())))
    for rounding in ROUNDINGS:
        kept = out8.clone()
        assert torch.equal(frames_to_uint8(kept, rounding).cpu(), torch.from_numpy(np_to_u8(kept.cpu().numpy(), rounding)))


def test_make_animation_uint8_within_two_levels(model):
    """the float clip and the byte clip come from two runs, which the Animator's gate allows to differ by 5e-3: 5e-3 x 255 = 1.275 across a rounding
    boundary is at most 2 levels"""
    from tests.test_clip_cpu import _clips
    src, clip = (t.to(DEV) for t in _clips(4))
    fl = make_animation(model, src, clip, relative=True, frames_per_call=3, graph=True)
    u8 = make_animation(model, src, clip, relative=True, frames_per_call=3, graph=True, output="uint8")
    B, _, T, H, W = clip.shape
    assert u8.dtype == torch.uint8 and u8.shape == (B, T, H, W, 3)
    want = np_to_u8(fl.permute(0, 2, 1, 3, 4).reshape(B * T, 3, H, W).cpu().numpy(), "nearest").reshape(B, T, H, W, 3)
    d = np.abs(u8.cpu().numpy().astype(np.int32) - want.astype(np.int32))
    print(f"[frame_io] make_animation uint8 vs quantised float: max level difference {d.max()}, differing bytes {(d > 0).mean():.2e}")
    assert d.max() <= 2


def test_reconstruction_new_keywords_leave_the_metrics_alone(model):
    """metrics="device" with output="uint8", visualize=True against the plain call.  The new keywords only READ the Animator's output (one more launch
    per group, one per frame), so the metrics may move by what two plain calls move by: the split-K atomics' summation order.  That spread is measured here
    from two plain calls, never from the new path: s = their largest difference over frames and sources, per metric.  Two samples show the SCALE of a
    random difference, not its bound -- a third run lies outside the range of two others one time in three -- so the tolerance is 4 s (for differences
    of a common light-tailed scale, 4 times the largest of eight observed ones is not reached), plus one fp32 step of the value: the rows are rounded to
    fp32 once, and runs whose sums differ in their last bits land on the same or on adjacent fp32 numbers.  Seen: s = 2e-8 on SSIM values of 1e-2, the
    new path 3e-8 from the first plain call; a mistake in the wiring (a stale or overwritten output) moves a frame's metrics by 1e-3 and more."""
    from tests.test_clip_cpu import _clips
    clip = _clips(4)[1].to(DEV)
    B, _, T, H, W = clip.shape
    p1 = reconstruction(model, clip, frames_per_call=3, metrics="device")
    p2 = reconstruction(model, clip, frames_per_call=3, metrics="device")
    new = reconstruction(model, clip, frames_per_call=3, metrics="device", output="uint8", visualize=True)
    for k in ("l1", "mse", "ssim"):
        a, b, c = (r["per_source"][k] for r in (p1, p2, new))
        spread = np.abs(a - b).max()
        tol = 4 * spread + 2.0 ** -23 * np.abs(a)
        print(f"[frame_io] reconstruction {k}: spread of two plain calls {spread:.3e}, new keywords vs plain {np.abs(c - a).max():.3e}")
        assert (np.abs(c - a) <= tol).all(), k
    assert new["prediction"].dtype == torch.uint8 and new["prediction"].shape == (B, T, H, W, 3)
    want = np_to_u8(p1["prediction"].permute(0, 2, 1, 3, 4).reshape(B * T, 3, H, W).cpu().numpy(), "floor").reshape(B, T, H, W, 3)
    assert np.abs(new["prediction"].cpu().numpy().astype(np.int32) - want.astype(np.int32)).max() <= 2
    vis = new["visualization"]
    assert vis.dtype == torch.uint8 and vis.shape == (T, B * H, 4 * W, 3)
    source_column = np_to_u8(clip[:, :, 0].contiguous().cpu().numpy(), "floor").reshape(B * H, W, 3)
    for t in range(T):
        assert np.array_equal(vis[t, :, :W].cpu().numpy(), source_column)
        assert np.array_equal(vis[t, :, 3 * W:].cpu().numpy(), new["prediction"][:, t].reshape(B * H, W, 3).cpu().numpy())
