"""mrfa_frames_resize_u8 on the GPU (-m gpu) against Pillow's recorded bytes (golden resize_pillow) and the numpy specification tests/ref_resize.py: bytes and
floats compared EXACTLY, the floats with bytes.astype(f32) * f32(1 / 255), canaries around both outputs.  The geometries take every path of the kernel: one
workgroup and many, ragged tiles, clipped bounds, fractional boxes, the float4 / dword stores (Wo % 4 == 0, aligned outputs) and the scalar ones, a vertical
footprint of more rows than a workgroup holds at a time (two rounds), and the tap cap on either axis."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mrfa_amd import hip, resize_hip
from tests import ref_resize as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_pillow.npz")
CANARY_F, CANARY_B, PAD = -7.0, 0xA5, 16
IDS = [R.geometry_id(g) for g in R.GEOMETRIES]
_P = ctypes.POINTER(ctypes.c_int)


def host_tables(n, in0, in1, m, f):
    """one axis through mrfa_resize_ksize / mrfa_resize_coeffs, held against the specification -> (bounds, kk) as numpy"""
    L = resize_hip.lib()
    k = L.mrfa_resize_ksize(n, in0, in1, m, f)
    assert k == R.ksize_of(in0, in1, m, f), resize_hip.last_error()
    bounds, kk = np.full(2 * m, -1, np.int32), np.full(m * k, -1, np.int32)
    resize_hip.check(L.mrfa_resize_coeffs(n, in0, in1, m, f, bounds.ctypes.data_as(_P), kk.ctypes.data_as(_P)), "mrfa_resize_coeffs")
    wb, wk = R.coeffs(n, in0, in1, m, f)
    assert np.array_equal(bounds.reshape(m, 2), wb) and np.array_equal(kk.reshape(m, k), wk)
    return bounds, kk


_TABLES = {}


def device_tables(Hi, Wi, size, box, f):
    key = (Hi, Wi, size, box, f)
    if key not in _TABLES:
        left, upper, right, lower = R.full_box(Hi, Wi, box)
        bh, kh = host_tables(Wi, left, right, size[1], f)
        bv, kv = host_tables(Hi, upper, lower, size[0], f)
        _TABLES[key] = tuple(torch.from_numpy(t).to(DEV) for t in (bh, kh, bv, kv)) + (kh.size // size[1], kv.size // size[0])
    return _TABLES[key]


def launch(src: np.ndarray, size, box, f, want=("f32", "u8"), src_offset=0, f32_offset=4, u8_offset=4, tables=None):
    """one entry call on src (N,Hi,Wi,C); src_offset: bytes past an aligned allocation; f32_offset / u8_offset: floats / bytes past one.  Returns
    (rc, floats (N,3,Ho,Wo) or None, bytes (N,Ho,Wo,3) or None) and checks the canaries around both outputs."""
    N, Hi, Wi, C = src.shape
    Ho, Wo = size
    bh, kh, bv, kv, ksh, ksv = device_tables(Hi, Wi, size, box, f) if tables is None else tables
    buf = torch.zeros(src.size + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[src_offset:src_offset + src.size].copy_(torch.from_numpy(src.reshape(-1)))
    n = N * 3 * Ho * Wo
    of = torch.full((n + 2 * PAD,), CANARY_F, device=DEV)
    ob = torch.full((n + 2 * PAD,), CANARY_B, dtype=torch.uint8, device=DEV)
    assert of.data_ptr() % 16 == 0 and ob.data_ptr() % 16 == 0
    rc = resize_hip.lib().mrfa_frames_resize_u8(hip.stream_ptr(), buf.data_ptr() + src_offset, N, Hi, Wi, C, bh.data_ptr(), kh.data_ptr(), ksh, bv.data_ptr(),
                                                kv.data_ptr(), ksv, Ho, Wo, of.data_ptr() + int(4 * f32_offset) if "f32" in want else None,
                                                ob.data_ptr() + u8_offset if "u8" in want else None)
    torch.cuda.synchronize()
    of, ob = of.cpu().numpy(), ob.cpu().numpy()
    gf = gb = None
    if "f32" in want and rc == 0:
        assert (of[:f32_offset] == CANARY_F).all() and (of[f32_offset + n:] == CANARY_F).all()
        gf = of[f32_offset:f32_offset + n].reshape(N, 3, Ho, Wo)
    else:
        assert (of == CANARY_F).all()
    if "u8" in want and rc == 0:
        assert (ob[:u8_offset] == CANARY_B).all() and (ob[u8_offset + n:] == CANARY_B).all()
        gb = ob[u8_offset:u8_offset + n].reshape(N, Ho, Wo, 3)
    else:
        assert (ob == CANARY_B).all()
    return rc, gf, gb


_WANT = {}


def expected(name, src, size, box, f):
    """the specification's bytes of a named input, computed once and shared"""
    key = (name, size, box, f)
    if key not in _WANT:
        _WANT[key] = R.resize_bytes(src, size, box, f)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def check(name, src, size, box, f, **kw):
    rc, gf, gb = launch(src, size, box, f, **kw)
    assert rc == 0, resize_hip.last_error()
    want = expected(name, src, size, box, f)
    if gb is not None:
        assert gb.dtype == np.uint8 and np.array_equal(gb, want), int((gb != want).sum())
    if gf is not None:
        assert gf.dtype == np.float32 and np.array_equal(gf, R.unit(want))
    return gf, gb


# ---------------------------------------------------------------------------------------------------------------------------- Pillow's own bytes
def test_every_pillow_golden():
    z = np.load(GOLDEN)
    for i, (gi, c, name, kind) in enumerate(R.GOLDEN_CASES):
        _, size, box = R.GEOMETRIES[gi]
        rc, gf, gb = launch(R.case_input(gi, c, kind), size, box, R.FILTERS[name])
        assert rc == 0, resize_hip.last_error()
        assert np.array_equal(gb[0], z[str(i)]), (i, int((gb[0] != z[str(i)]).sum()))
        assert np.array_equal(gf, R.unit(z[str(i)][None])), i


# ---------------------------------------------------------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("name", list(R.FILTERS))
@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=IDS)
def test_geometry_and_filter_rgb_both_outputs(gi, name):
    _, size, box = R.GEOMETRIES[gi]
    check(f"g{gi}/3/random", R.case_input(gi, 3, "random"), size, box, R.FILTERS[name])


@pytest.mark.parametrize("gi", range(len(R.GEOMETRIES)), ids=IDS)
def test_three_frames_grey_and_rgba_at_an_odd_address(gi):
    """N = 3; C = 1 and 4; the source 1 and 3 bytes past an aligned address; the outputs 4 and 1 floats / 4, 1 and 2 bytes past one (vector and scalar stores)"""
    _, size, box = R.GEOMETRIES[gi]
    f = (R.BILINEAR, R.LANCZOS, R.BICUBIC)[gi % 3]
    g = R.case_input(gi, 1, "random", N=3)
    check(f"g{gi}/1/random/3", g, size, box, f, src_offset=1, f32_offset=1, u8_offset=1)
    a = R.case_input(gi, 4, "random", N=3)
    check(f"g{gi}/4/random/3", a, size, box, f, src_offset=3, u8_offset=2)
    rgb = np.ascontiguousarray(a[..., :3])
    assert np.array_equal(expected(f"g{gi}/4/random/3", a, size, box, f), expected(f"g{gi}/4/random/3/rgb", rgb, size, box, f))      # alpha is never read


@pytest.mark.parametrize("gi", [3, 6, 8, 9], ids=[IDS[i] for i in (3, 6, 8, 9)])
def test_float_only_bytes_only_and_both_agree(gi):
    _, size, box = R.GEOMETRIES[gi]
    src = R.case_input(gi, 3, "random")
    name = f"g{gi}/3/random"
    gf, none = check(name, src, size, box, R.HAMMING, want=("f32",))
    assert none is None
    none, gb = check(name, src, size, box, R.HAMMING, want=("u8",))
    assert none is None
    bf, bb = check(name, src, size, box, R.HAMMING)
    assert np.array_equal(bf, gf) and np.array_equal(bb, gb)
    again = check(name, src, size, box, R.HAMMING)
    assert np.array_equal(again[0], bf) and np.array_equal(again[1], bb)              # every run bit-identical


@pytest.mark.parametrize("name", ["bicubic", "lanczos"])
@pytest.mark.parametrize("gi", [2, 5, 6, 8], ids=[IDS[i] for i in (2, 5, 6, 8)])
def test_zero_and_255_only_images_clamp(gi, name):
    _, size, box = R.GEOMETRIES[gi]
    check(f"g{gi}/3/extreme", R.case_input(gi, 3, "extreme"), size, box, R.FILTERS[name])


# ---------------------------------------------------------------------------------------------------------------------------- the cap and the rounds
def test_geometries_at_the_cap_and_either_side_of_the_staging_threshold_run_each_way():
    """Lanczos at scale 63.5: 2 ceil(190.5) + 1 = 383 taps = MRFA_RESIZE_MAX_TAPS; at scale 21: 127 taps, the most whose tables a workgroup keeps in LDS;
    at 21.25: 129, the first geometry of the kernel that reads them where they lie -- horizontally and vertically"""
    assert R.ksize_of(0, 254, 4, R.LANCZOS) == R.MAX_TAPS == resize_hip.MAX_TAPS == 383
    assert R.ksize_of(0, 84, 4, R.LANCZOS) == 127 and R.ksize_of(0, 85, 4, R.LANCZOS) == 129
    for n in (254, 84, 85):
        check(f"cap/h/{n}", R.det_bytes(f"resize/cap/h/{n}", (2, 3, n, 3)), (3, 4), None, R.LANCZOS)
        check(f"cap/v/{n}", R.det_bytes(f"resize/cap/v/{n}", (2, n, 3, 3)), (4, 3), None, R.LANCZOS)


@pytest.mark.parametrize("rows,out,taps,held", [(399, 19, 127, 192), (1270, 20, 383, 384)])
def test_a_footprint_of_more_rows_than_a_round_holds(rows, out, taps, held):
    """Lanczos at 21x (tables in LDS, 192 rows held) and at 63.5x (384 held): the first tile's 8 output rows read more source rows than that: several rounds"""
    src = R.det_bytes(f"resize/rounds/{rows}", (1, rows, 5, 3))
    bounds, _ = R.coeffs(rows, 0, rows, out, R.LANCZOS)
    assert bounds[7].sum() - bounds[0, 0] > held and R.ksize_of(0, rows, out, R.LANCZOS) == taps
    check(f"rounds/{rows}", src, (out, 2), None, R.LANCZOS)
    check(f"rounds/{rows}/1", src[..., :1].copy(), (out, 2), None, R.LANCZOS, want=("u8",), u8_offset=3)


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_too_many_taps_are_refused_with_the_outputs_untouched():
    L = resize_hip.lib()
    assert R.ksize_of(0, 2000, 16, R.LANCZOS) == 751
    assert L.mrfa_resize_ksize(2000, 0.0, 2000.0, 16, R.LANCZOS) < 0 and "751 taps" in resize_hip.last_error()
    bounds, kk = np.full(32, -1, np.int32), np.full(16 * 751, -1, np.int32)
    assert L.mrfa_resize_coeffs(2000, 0.0, 2000.0, 16, R.LANCZOS, bounds.ctypes.data_as(_P), kk.ctypes.data_as(_P)) != 0
    assert (bounds == -1).all() and (kk == -1).all()
    # the launch: tables of 751 taps a row, as the specification makes them
    wb, wk = R.coeffs(2000, 0, 2000, 16, R.LANCZOS)
    vb, vk = R.coeffs(1, 0, 1, 1, R.LANCZOS)
    tables = tuple(torch.from_numpy(np.ascontiguousarray(t.reshape(-1))).to(DEV) for t in (wb, wk, vb, vk)) + (751, vk.shape[1])
    rc, gf, gb = launch(R.det_bytes("resize/refused", (1, 1, 2000, 3)), (1, 16), None, R.LANCZOS, tables=tables)         # (launch checks the canaries)
    assert rc != 0 and gf is None and gb is None and "751" in resize_hip.last_error()


def test_the_other_refusals_come_before_any_write():
    L = resize_hip.lib()
    src = R.det_bytes("resize/refusals", (1, 6, 8, 3))
    t = device_tables(6, 8, (4, 4), None, R.BILINEAR)
    ok = dict(size=(4, 4), box=None, f=R.BILINEAR)
    assert launch(src, **ok)[0] == 0
    for want in ((),):                                                                                # both outputs null
        assert launch(src, want=want, **ok)[0] != 0 and "both null" in resize_hip.last_error()
    assert launch(src, f32_offset=0.5, **ok)[0] != 0 and "4-byte aligned" in resize_hip.last_error()  # out_f32 2 bytes past a float
    for k in range(4):                                                                                # a null table
        bad = list(t)
        bad[k] = torch.empty(0, dtype=torch.int32)                                                    # (data_ptr() == 0)
        assert bad[k].data_ptr() == 0
        assert launch(src, tables=tuple(bad), **ok)[0] != 0 and "null pointer" in resize_hip.last_error()
    for ks in ((0, 3), (3, 0), (R.MAX_TAPS + 1, 3), (3, R.MAX_TAPS + 1)):
        assert launch(src, tables=t[:4] + ks, **ok)[0] != 0 and "ksize" in resize_hip.last_error()
    of = torch.full((64,), CANARY_F, device=DEV)
    dsrc = torch.from_numpy(src).to(DEV)

    def raw(src_ptr=None, N=1, Hi=6, Wi=8, Cin=3, Ho=4, Wo=4):
        return L.mrfa_frames_resize_u8(hip.stream_ptr(), dsrc.data_ptr() if src_ptr is None else src_ptr, N, Hi, Wi, Cin, t[0].data_ptr(), t[1].data_ptr(),
                                       t[4], t[2].data_ptr(), t[3].data_ptr(), t[5], Ho, Wo, of.data_ptr(), None)
    assert raw(src_ptr=0) != 0 and "null pointer" in resize_hip.last_error()
    for kw in (dict(N=0), dict(Hi=0), dict(Wi=0), dict(Ho=0), dict(Wo=0), dict(N=-1), dict(N=65536)):
        assert raw(**kw) != 0, kw
    for cin in (0, 2, 5):
        assert raw(Cin=cin) != 0 and f"not {cin}" in resize_hip.last_error()
    torch.cuda.synchronize()
    assert (of.cpu().numpy() == CANARY_F).all()
    assert raw() == 0
    torch.cuda.synchronize()
    assert (of.cpu().numpy()[:48] != CANARY_F).all() and (of.cpu().numpy()[48:] == CANARY_F).all()


def test_the_coefficient_entries_refuse_boxes_filters_and_sizes():
    L = resize_hip.lib()
    bounds, kk = np.full(8, -1, np.int32), np.full(64, -1, np.int32)
    pb, pk = bounds.ctypes.data_as(_P), kk.ctypes.data_as(_P)
    bad = [(0, 0, 1, 4, 1), (4, 0, 4, 0, 1), (4, 0, 4, 4, 5), (4, 0, 4, 4, -1), (4, -0.5, 4, 4, 1), (4, 0, 4.5, 4, 1), (4, 2, 2, 4, 1), (4, 3, 1, 4, 1),
           (4, float("nan"), 4, 4, 1), (4, 0, float("inf"), 4, 1)]
    for n, a, b, m, f in bad:
        assert L.mrfa_resize_ksize(n, a, b, m, f) < 0 and resize_hip.last_error(), (n, a, b, m, f)
        assert L.mrfa_resize_coeffs(n, a, b, m, f, pb, pk) != 0
    assert L.mrfa_resize_coeffs(4, 0.0, 4.0, 4, 1, None, pk) != 0 and L.mrfa_resize_coeffs(4, 0.0, 4.0, 4, 1, pb, None) != 0
    assert "null table" in resize_hip.last_error()
    assert (bounds == -1).all() and (kk == -1).all()
    assert L.mrfa_resize_version() == resize_hip.ABI_VERSION == R.VERSION
