"""mrfa_pair_augment on the GPU (-m gpu) against Pillow's recorded outputs (golden augment_pillow) and the numpy specification tests/ref_augment.py.  Floats
are compared EXACTLY with bytes.astype(f32) * f32(1 / 255).  Shapes take every path: one pixel per lane (1x1, 1x2, 5x7), four per lane (8x12, 33x20), and
96x128 -- 3072 quads per frame, more than one workgroup and more than one luma partial, 12 per workgroup of the luma pass and so no multiple of its 256 lanes."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

from mrfa_amd import data_hip, hip
from tests import ref_augment as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 1), (1, 2), (5, 7), (8, 12), (33, 20), (96, 128)]
ORDERS = list(itertools.permutations((R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE)))
CANARY = -7.0


def descriptors(descs):
    arr = (data_hip.PairAug * len(descs))()
    for a, (ops, factor, shift, tflip, hflip) in zip(arr, descs):
        for k in range(4):
            a.op[k] = ops[k] if k < len(ops) else R.NONE
        a.factor[:] = list(factor)
        a.hue_shift, a.time_flip, a.hflip = shift, int(tflip), int(hflip)
    return arr


def run(src: np.ndarray, descs, src_offset=0, out_offset=0, ws_fill=None):
    """one entry call on src (B,2,H,W,C); src_offset: bytes past an aligned allocation; out_offset: floats past one.  Returns (source, driving) as numpy
    and checks the canaries around both outputs."""
    B, _, H, W, C = src.shape
    L = data_hip.lib()
    buf = torch.zeros(src.size + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[src_offset:src_offset + src.size].copy_(torch.from_numpy(src.reshape(-1)))
    n = B * 3 * H * W
    outs = [torch.full((n + 8,), CANARY, device=DEV) for _ in range(2)]
    assert all(o.data_ptr() % 16 == 0 for o in outs)
    nbytes = L.mrfa_pair_augment_workspace(B, H, W)
    assert nbytes == 2 * B * R.PARTS * 4
    ws = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    data_hip.check(L.mrfa_pair_augment(hip.stream_ptr(), buf.data_ptr() + src_offset, B, H, W, C, descriptors(descs), ws.data_ptr(), nbytes,
                                       outs[0].data_ptr() + 4 * out_offset, outs[1].data_ptr() + 4 * out_offset), "mrfa_pair_augment")
    got = []
    for o in outs:
        o = o.cpu().numpy()
        assert (o[:out_offset] == CANARY).all() and (o[out_offset + n:] == CANARY).all()
        got.append(o[out_offset:out_offset + n].reshape(B, 3, H, W))
    return got


def expect(src, descs):
    s, d = R.pair_augment_bytes(src, descs)
    return R.unit(s), R.unit(d)


def check(src, descs, **kw):
    got, want = run(src, descs, **kw), expect(src, descs)
    assert got[0].dtype == np.float32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


def mixed(B):
    """B descriptors that differ in every field: all four ops in another order each, factors on both sides of 1, both hue signs, the flips taking turns"""
    out = []
    for b in range(B):
        f = (0.9 + 0.07 * b, 1.1 - 0.06 * b, 0.93 + 0.1 * b)
        out.append((list(ORDERS[(7 * b + 3) % 24]), f, R.hue_shift_of(0.1 if b % 2 else -0.1), b % 2, (b // 2) % 2))
    return out


# ------------------------------------------------------------------------------------------------------------------------ Pillow's own outputs
with open(os.path.join(GOLDEN, "augment_pillow.json")) as _f:
    PILLOW = json.load(_f)["cases"]
PILLOW_GROUPS = sorted({(c["H"], c["W"], c["C"]) for c in PILLOW})


@pytest.mark.parametrize("group", PILLOW_GROUPS, ids=lambda g: "x".join(map(str, g)))
def test_every_pillow_golden_of_a_shape_as_pairs_of_one_call(group):
    """per op alone (f = 0, 0.9, 1, 1.1, 2; hue +-0.1, +-0.5), all 24 orders at 8x12, two orders elsewhere: each golden case is one PAIR of a call (both frames
    the golden's input), so one call carries pairs with different parameters"""
    H, W, C = group
    arrays = np.load(os.path.join(GOLDEN, "augment_pillow.npz"))
    cases = [c for c in PILLOW if (c["H"], c["W"], c["C"]) == group]
    frame = R.det_bytes(f"augment/pillow/{H}x{W}x{C}", (H, W, C))
    for b0 in range(0, len(cases), R.MAX_PAIRS):
        part = cases[b0:b0 + R.MAX_PAIRS]
        src = np.broadcast_to(frame, (len(part), 2, H, W, C)).copy()
        source, driving = run(src, [R.ops_of(c["ops"]) + (0, 0) for c in part])
        for b, c in enumerate(part):
            want = R.unit(arrays[c["key"]].transpose(2, 0, 1))
            assert np.array_equal(source[b], want) and np.array_equal(driving[b], want), c["name"]


# ------------------------------------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pairs_with_different_parameters_equal_the_specification(shape, B, C):
    H, W = shape
    src = R.det_bytes(f"augment/gpu/{H}x{W}x{C}/{B}", (B, 2, H, W, C))
    descs = mixed(B)
    if B == 3:
        descs[1] = ([], (1.0, 1.0, 1.0), 0, 0, 1)                                           # one pair with no op at all (flipped, so not a plain copy)
    a = check(src, descs)
    b = run(src, descs, ws_fill=0xFF)                                                      # nothing in the workspace needs zeroing; two runs, bit for bit
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("shape", [(8, 12), (96, 128)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("src_offset,out_offset", [(1, 0), (0, 1), (3, 3), (2, 2)])
def test_source_at_an_odd_byte_and_outputs_off_the_16_byte_grid(shape, src_offset, out_offset):
    """W % 4 == 0 keeps four pixels per lane; a src that is not 4-byte aligned loads bytes, outputs that are only 4-byte aligned store scalars"""
    H, W = shape
    for C in (1, 3, 4):
        check(R.det_bytes(f"augment/gpu/offset/{C}", (2, 2, H, W, C)), mixed(2), src_offset=src_offset, out_offset=out_offset)


@pytest.mark.parametrize("shape", [(5, 7), (8, 12), (96, 128)], ids=lambda s: "x".join(map(str, s)))
def test_all_four_flip_combinations(shape):
    """both flips at once included: PairAugmenter.draw never produces it, the entry accepts it"""
    H, W = shape
    src = R.det_bytes("augment/gpu/flips", (4, 2, H, W, 3))
    ops = ([R.CONTRAST, R.HUE], (1.0, 1.2, 1.0), 40)
    got = check(src, [ops + (t, h) for t in (0, 1) for h in (0, 1)])
    plain = check(src, [ops + (0, 0)] * 4)
    for b, (t, h) in enumerate((t, h) for t in (0, 1) for h in (0, 1)):
        want = [plain[0][b], plain[1][b]][::-1 if t else 1]
        assert np.array_equal(got[0][b], want[0][..., ::-1] if h else want[0]) and np.array_equal(got[1][b], want[1][..., ::-1] if h else want[1])


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "".join("_bcsh"[k] for k in o))
def test_all_24_orders(order):
    src = R.det_bytes("augment/gpu/orders", (2, 2, 8, 12, 3))
    check(src, [(list(order), (1.07, 0.93, 1.09), R.hue_shift_of(-0.08), 0, 0), (list(order[:2]), (0.5, 1.6, 2.0), 3, 1, 0)])


@pytest.mark.parametrize("op,values", [(R.BRIGHTNESS, (0.0, 0.9, 1.0, 1.1, 2.0)), (R.CONTRAST, (0.0, 0.9, 1.0, 1.1, 2.0)),
                                       (R.SATURATION, (0.0, 0.9, 1.0, 1.1, 2.0)), (R.HUE, (-0.5, -0.1, 0.1, 0.5))], ids=["brightness", "contrast", "saturation", "hue"])
def test_each_op_alone(op, values):
    for H, W in ((5, 7), (33, 20)):
        src = R.det_bytes(f"augment/gpu/alone/{H}x{W}", (len(values), 2, H, W, 3))
        descs = []
        for v in values:
            factor = [1.0, 1.0, 1.0]
            if op != R.HUE:
                factor[op - 1] = v
            descs.append(([op], tuple(factor), R.hue_shift_of(v) if op == R.HUE else 0, 0, 0))
        got = check(src, descs)
        if op != R.HUE:                                                                   # f = 1 is the identity, f = 0 the degenerate image
            assert np.array_equal(got[0][2], R.unit(src[2, 0].transpose(2, 0, 1)))


# ------------------------------------------------------------------------------------------------------------------------ the contrast mean
def grey(values, H, W):
    return np.repeat(np.asarray(values, np.uint8).reshape(H, W, 1), 3, axis=2)


def test_contrast_mean_rounds_a_half_up_and_is_taken_per_frame():
    """1 x 2 frames.  L = 10, 11: mean 10.5 -> m = 11, so f = 2 gives 2 x - 11 = (9, 11) (m = 10 would give (10, 12)).  The pair's other frame, L = 200, 100,
    has m = 150: (250, 50) -- one mean for the pair, 80, would give (255, 120)."""
    src = np.stack([grey([10, 11], 1, 2), grey([200, 100], 1, 2)])[None]
    source, driving = check(src, [([R.CONTRAST], (1.0, 2.0, 1.0), 0, 0, 0)])
    assert np.array_equal(source[0, :, 0], R.unit(np.array([[9, 11]] * 3))) and np.array_equal(driving[0, :, 0], R.unit(np.array([[250, 50]] * 3)))


@pytest.mark.parametrize("shape", [(5, 7), (96, 128)], ids=lambda s: "x".join(map(str, s)))
def test_contrast_mean_just_below_and_at_a_half(shape):
    """n pixels of L = 10 of which k are 11: the mean is 10 + k / n.  k = ceil(n / 2) - 1 is the last count below a half (m = 10), the next one reaches it (m = 11)"""
    H, W = shape
    n = H * W
    below = (n + 1) // 2 - 1
    frames = []
    for k in (below, below + 1):
        v = np.full(n, 10)
        v[(np.arange(k) * 7919) % n if n > 7919 else np.arange(k)] = 11                   # spread over the partial sums (7919 is prime to 96 x 128)
        assert v.sum() == 10 * n + k
        frames.append(grey(v, H, W))
    src = np.stack(frames)[None]
    assert [R.contrast_mean(f) for f in src[0]] == [10, 11]
    source, driving = check(src, [([R.CONTRAST], (1.0, 2.0, 1.0), 0, 0, 0)])
    assert set(np.rint(source * 255).reshape(-1)) == {10, 12} and set(np.rint(driving * 255).reshape(-1)) == {9, 11}


def test_contrast_mean_follows_the_ops_before_it():
    src = R.det_bytes("augment/gpu/before", (2, 2, 96, 128, 3))
    descs = [([R.BRIGHTNESS, R.HUE, R.CONTRAST, R.SATURATION], (0.5, 1.5, 1.3), 100, 0, 0), ([R.CONTRAST, R.BRIGHTNESS], (0.5, 1.5, 1.0), 0, 0, 0)]
    check(src, descs)
    assert R.contrast_mean(R.brightness(src[0, 0], 0.5)) != R.contrast_mean(src[0, 0])   # the order shows in the mean


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_the_outputs_untouched():
    L = data_hip.lib()
    B, H, W = 2, 4, 8
    src = torch.zeros(B * 2 * H * W * 3, dtype=torch.uint8, device=DEV)
    outs = [torch.full((B * 3 * H * W + 4,), CANARY, device=DEV) for _ in range(2)]
    nbytes = L.mrfa_pair_augment_workspace(B, H, W)
    ws = torch.zeros(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
    ok = [([R.CONTRAST], (1.0, 1.0, 1.0), 0, 0, 0)] * 2
    good = dict(src=src.data_ptr(), B=B, H=H, W=W, Cin=3, params=descriptors(ok), workspace=ws.data_ptr(), workspace_bytes=nbytes,
                source=outs[0].data_ptr(), driving=outs[1].data_ptr())

    def bad_desc(ops=(R.CONTRAST,), factor=(1.0, 1.0, 1.0)):
        return descriptors([ok[0], (list(ops), factor, 0, 0, 0)])

    cases = [dict(src=None), dict(params=None), dict(workspace=None), dict(source=None), dict(driving=None), dict(B=0), dict(H=0), dict(W=-1),
             dict(B=R.MAX_PAIRS + 1), dict(H=1 << 16, W=1 << 15), dict(Cin=2), dict(Cin=5), dict(params=bad_desc(ops=(1, 5))),
             dict(params=bad_desc(ops=(2, 0, 2))), dict(params=bad_desc(factor=(1.0, float("inf"), 1.0))), dict(params=bad_desc(factor=(1.0, 1.0, float("nan")))),
             dict(params=bad_desc(factor=(-0.5, 1.0, 1.0))), dict(workspace_bytes=nbytes - 1), dict(workspace=ws.data_ptr() + 4),
             dict(source=outs[0].data_ptr() + 2), dict(driving=outs[1].data_ptr() + 1)]
    for kw in cases:
        a = {**good, **kw}
        rc = L.mrfa_pair_augment(hip.stream_ptr(), a["src"], a["B"], a["H"], a["W"], a["Cin"], a["params"], a["workspace"], a["workspace_bytes"],
                                 a["source"], a["driving"])
        assert rc != 0 and L.mrfa_data_last_error().startswith(b"pair_augment: "), kw
        with pytest.raises(RuntimeError, match="pair_augment"):
            data_hip.check(rc, "mrfa_pair_augment")
    torch.cuda.synchronize()
    assert all((o == CANARY).all() for o in outs) and (ws == 0).all()
    assert L.mrfa_pair_augment_workspace(0, H, W) < 0 and L.mrfa_pair_augment_workspace(R.MAX_PAIRS + 1, H, W) < 0 \
        and L.mrfa_pair_augment_workspace(1, 1 << 16, 1 << 15) < 0
    assert ctypes.sizeof(data_hip.PairAug) == 20 and L.mrfa_data_version() == data_hip.ABI_VERSION


# ------------------------------------------------------------------------------------------------------------------------ all 2^24 colours
@pytest.mark.parametrize("quarter", range(4))
@pytest.mark.parametrize("op", ["hue", "saturation"])
def test_all_colours_in_quarters(op, quarter):
    """hue is the one op with divisions and float64: a rounding difference between the device's arithmetic and the host's shows only on the whole colour
    cube.  One 2048 x 2048 frame pair per test (2^22 colours); most of the seconds are the host's restatement."""
    v = np.arange(quarter << 22, (quarter + 1) << 22, dtype=np.uint32)
    frame = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(2048, 2048, 3)
    shift = (25, 231, 128, 1)[quarter]
    desc = ([R.HUE], (1.0, 1.0, 1.0), shift, 0, 0) if op == "hue" else ([R.SATURATION], (1.0, 1.0, 1.3), 0, 0, 0)
    want = R.hue(frame, shift) if op == "hue" else R.saturation(frame, 1.3)
    L = data_hip.lib()
    src = torch.from_numpy(frame).to(DEV)[None, None].expand(1, 2, 2048, 2048, 3).contiguous()
    source, driving = torch.empty(1, 3, 2048, 2048, device=DEV), torch.empty(1, 3, 2048, 2048, device=DEV)
    ws = torch.zeros(L.mrfa_pair_augment_workspace(1, 2048, 2048) // 8, dtype=torch.int64, device=DEV)
    data_hip.check(L.mrfa_pair_augment(hip.stream_ptr(), src.data_ptr(), 1, 2048, 2048, 3, descriptors([desc]), ws.data_ptr(), ws.numel() * 8,
                                       source.data_ptr(), driving.data_ptr()), "mrfa_pair_augment")
    want = torch.from_numpy(R.unit(want.transpose(2, 0, 1)))[None]
    assert torch.equal(source.cpu(), want) and torch.equal(driving, source)
