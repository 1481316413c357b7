"""mrfa_pack_conv_weights_multi / mrfa_unpack_wgrads_multi (csrc/pack_multi.hip) byte for byte (-m gpu).

A pack is a copy (plus, for the bf16 planes, an exact integer / fp32 split): there is no tolerance.  Every destination buffer is compared WHOLE, padding
included, as integers:
  * against a host restatement of the layouts written here (the index formulas of the pack-mode table in include/mrfa_hip.h, chunk_major for the bf16
    planes, the three-piece chop split, round-to-nearest-even, the phase-tap sums in their row-outer / column-inner order), once on zero-filled buffers
    and once on buffers filled with a sentinel: padding elements must keep whatever they held (the 4-byte-store kernels this file was written
    against passed every zero-filled comparison and failed the sentinel one for modes 12 / 13 with an odd channel count only: they paired a lone
    last channel with a zero written into the padding element beside it, invisible in the zero-filled buffers the engine allocates);
  * the fp32 layouts also against the single-tensor pack of csrc/layout.hip (mrfa_pack_conv_weight), which writes zeros into the padding, on the
    zero-filled buffers.
Shapes: Cout in {1, 3, 33, 126, 128} x Cin in {2, 3, 16, 33, 98, 160} (every tail of the 8-element runs, the float4 runs, the 32-channel tiles and the
16-channel chunks; channel counts that are and are not multiples of 4) x taps 1x1, 3x3 (32-row tiles), 5x5 (16) and 7x7 (8); the 30 shapes of one tap
count travel in ONE launch of 120 descriptors (more than the 48 of the first table size), and one case is a launch of a single descriptor.
The unpack: the [tap][Cout][Cin] / [Cout][tap][Cin] images of a random OIHW tensor come back as that tensor exactly (into zeros), and += into a non-zero
gradient equals the single-tensor unpack of csrc/layout.hip bit for bit (one fp32 addition per element either way)."""
import ctypes as C
import zlib

import pytest
import torch

from mrfa_amd import engine, hip

pytestmark = pytest.mark.gpu

COUTS, CINS = (1, 3, 33, 126, 128), (2, 3, 16, 33, 98, 160)
F32_MODES, BF16_MODES, PHASE_MODES = (0, 1, 2, 3, 5, 7), (8, 9, 14, 15), (12, 13)
SENTINEL = 0x5A5A


def _up(a, b):
    return (a + b - 1) // b * b


def _rand(name, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(zlib.crc32(name.encode())))


def _split3(x):
    """the three bf16 chop pieces of fp32 x as int16 bit patterns: p1 + p2 + p3 == x exactly"""
    out = []
    for _ in range(3):
        u = x.contiguous().view(torch.int32) & -65536
        out.append((u >> 16).to(torch.int16))
        x = x - u.view(torch.float32)
    return out


def _rne(x):
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return ((r ^ 0x8000) - 0x8000).to(torch.int16)


def _phase_weights(wv):
    """[Cout][Cin][16]: phase tap (py, px, a, b) = sum of the 3x3 taps on its source pixel, rows outer, columns inner, from 0"""
    sets = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
    out = torch.zeros(wv.shape[0], wv.shape[1], 16)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    s = torch.zeros(wv.shape[0], wv.shape[1])
                    for r in sets[(py, a)]:
                        for c in sets[(px, b)]:
                            s = s + wv[:, :, r * 3 + c]
                    out[:, :, (py * 2 + px) * 4 + a * 2 + b] = s
    return out


def restate(w, mode):
    """-> (dtype, elements of the buffer, [(flat indices, values)]) of pack mode `mode` of OIHW w: the elements the pack writes, nothing else"""
    Cout, Cin, R, S = w.shape
    T = R * S
    wv = w.reshape(Cout, Cin, T)
    if mode in PHASE_MODES:
        wv, T = _phase_weights(wv), 16
    co, ci, t = torch.meshgrid(torch.arange(Cout), torch.arange(Cin), torch.arange(T), indexing="ij")
    tf = T - 1 - t
    if mode in F32_MODES:
        if mode == 0:
            n, idx = T * _up(Cout, 128) * _up(Cin, 32), (t * _up(Cout, 128) + co) * _up(Cin, 32) + ci
        elif mode == 1:
            n, idx = _up(Cout, 128) * _up(T * Cin, 32), co * _up(T * Cin, 32) + t * Cin + ci
        elif mode == 2:
            n, idx = T * _up(Cin, 128) * _up(Cout, 32), (tf * _up(Cin, 128) + ci) * _up(Cout, 32) + co
        elif mode == 3:
            n, idx = _up(Cin, 128) * _up(T * Cout, 32), ci * _up(T * Cout, 32) + tf * Cout + co
        elif mode == 5:
            n, idx = Cout * Cin * T, (co * T + t) * Cin + ci
        else:
            n, idx = Cout * Cin * T, (ci * T + tf) * Cout + co
        return torch.int32, n, [(idx.reshape(-1), wv.contiguous().view(torch.int32).reshape(-1))]
    fwd = mode in (8, 12, 14)
    rows, cols, rowsP, colsP = (co, ci, _up(Cout, 128), _up(Cin, 32)) if fwd else (ci, co, _up(Cin, 128), _up(Cout, 32))
    tt = t if (fwd or mode == 13) else tf
    idx = tt * rowsP * colsP + (cols // 16) * (rowsP * 16) + rows * 16 + cols % 16          # k16-chunk-major
    plane = T * rowsP * colsP
    pieces = [_rne(wv)] if mode in (14, 15) else _split3(wv)
    return torch.int16, len(pieces) * plane, [(idx.reshape(-1) + k * plane, p.reshape(-1)) for k, p in enumerate(pieces)]


def _modes(R):
    return F32_MODES + BF16_MODES + (PHASE_MODES if R == 3 else ())


def _pack_case(shapes, fill, dev):
    """packs every shape into every layout in ONE launch (three destinations per descriptor); -> [(shape, mode, buffer, weight)]"""
    descs, out, keep = [], [], []
    for Cout, Cin, R in shapes:
        w = _rand(f"pack/{Cout}/{Cin}/{R}", (Cout, Cin, R, R))
        wd = w.to(dev)
        keep.append(wd)
        modes = _modes(R)
        for i in range(0, len(modes), 3):
            d = hip.PackDesc()
            d.src, d.Cout, d.Cin, d.R, d.S = wd.data_ptr(), Cout, Cin, R, R
            part = modes[i:i + 3]
            d.ndst = len(part)
            for k, m in enumerate(part):
                dtype, n = torch.int32 if m in F32_MODES else torch.int16, _count(Cout, Cin, R * R, m)
                buf = torch.full((n,), fill if dtype == torch.int16 else fill * 65537, dtype=dtype, device=dev)
                d.dst[k], d.mode[k] = buf.data_ptr(), m
                out.append(((Cout, Cin, R), m, buf, w))
            descs.append(d)
    table = (hip.PackDesc * len(descs))(*descs)
    hip.check(hip.lib().mrfa_pack_conv_weights_multi(hip.stream_ptr(), table, len(descs)), "pack_conv_weights_multi")
    torch.cuda.synchronize()
    return out, len(descs)


def _count(Cout, Cin, T, m):
    if m == 0:
        return T * _up(Cout, 128) * _up(Cin, 32)
    if m == 1:
        return _up(Cout, 128) * _up(T * Cin, 32)
    if m == 2:
        return T * _up(Cin, 128) * _up(Cout, 32)
    if m == 3:
        return _up(Cin, 128) * _up(T * Cout, 32)
    if m in (5, 7):
        return Cout * Cin * T
    planes, taps = (1 if m in (14, 15) else 3), (16 if m in PHASE_MODES else T)
    return planes * taps * (_up(Cout, 128) * _up(Cin, 32) if m in (8, 12, 14) else _up(Cin, 128) * _up(Cout, 32))


def _expected(w, m, fill, cache={}):
    key = (id(w), m)
    if key not in cache:
        cache.clear()                                         # (the two fills of one buffer follow each other)
        cache[key] = (w, restate(w, m))                       # (holds w: its id cannot be handed out again meanwhile)
    dtype, n, writes = cache[key][1]
    assert n == _count(w.shape[0], w.shape[1], w.shape[2] * w.shape[3], m)
    exp = torch.full((n,), fill if dtype == torch.int16 else fill * 65537, dtype=dtype)
    for idx, val in writes:
        exp[idx] = val
    return exp


def test_modes_cover_the_layout_table():
    used = {m for lay in engine.LAYOUTS.values() for m in lay.modes}
    assert used <= set(F32_MODES + BF16_MODES + PHASE_MODES), used


@pytest.mark.parametrize("R", [1, 3, 5, 7])
def test_pack_multi_bytes(R):
    dev = torch.device("cuda", 0)
    shapes = [(co, ci, R) for co in COUTS for ci in CINS]
    zero, ndesc = _pack_case(shapes, 0, dev)
    assert ndesc > 48
    sent, _ = _pack_case(shapes, SENTINEL, dev)
    bad = []
    for (shape, m, bz, w), (_, _, bs, _) in zip(zero, sent):
        if not torch.equal(bz.cpu(), _expected(w, m, 0)):
            bad.append((shape, m, "zero-filled"))
        if not torch.equal(bs.cpu(), _expected(w, m, SENTINEL)):
            bad.append((shape, m, "sentinel-filled: padding written, or an element missed"))
        if m in F32_MODES:                                    # the single-tensor pack (it writes the padding as zeros)
            ref = torch.full_like(bz, 0x7FC00000)
            hip.check(hip.lib().mrfa_pack_conv_weight(hip.stream_ptr(), w.to(dev).data_ptr(), ref.data_ptr(), shape[0], shape[1], R, R, m),
                      "pack_conv_weight")
            torch.cuda.synchronize()
            if not torch.equal(bz, ref):
                bad.append((shape, m, "single-tensor pack"))
    assert not bad, bad


def test_pack_single_descriptor():
    dev = torch.device("cuda", 0)
    Cout, Cin, R = 33, 98, 3
    w = _rand("pack/single", (Cout, Cin, R, R))
    wd = w.to(dev)
    for modes in ((8, 9, 12), (13,), (0, 15, 7)):
        for fill in (0, SENTINEL):
            d = hip.PackDesc()
            d.src, d.Cout, d.Cin, d.R, d.S, d.ndst = wd.data_ptr(), Cout, Cin, R, R, len(modes)
            bufs = []
            for k, m in enumerate(modes):
                dtype = torch.int32 if m in F32_MODES else torch.int16
                bufs.append(torch.full((_count(Cout, Cin, R * R, m),), fill if dtype == torch.int16 else fill * 65537, dtype=dtype, device=dev))
                d.dst[k], d.mode[k] = bufs[-1].data_ptr(), m
            hip.check(hip.lib().mrfa_pack_conv_weights_multi(hip.stream_ptr(), C.pointer(d), 1), "pack_conv_weights_multi")
            torch.cuda.synchronize()
            for m, b in zip(modes, bufs):
                assert torch.equal(b.cpu(), _expected(w, m, fill)), (m, fill)


def test_pack_unaligned_destination():
    """destinations 4 (fp32) / 2 (bf16) bytes off a 16-byte boundary take the element-by-element stores: same bytes"""
    dev = torch.device("cuda", 0)
    Cout, Cin, R = 33, 160, 3
    w = _rand("pack/unaligned", (Cout, Cin, R, R))
    wd = w.to(dev)
    for m in (0, 2, 8, 9, 12, 13, 14):
        dtype = torch.int32 if m in F32_MODES else torch.int16
        n = _count(Cout, Cin, R * R, m)
        raw = torch.full((n + 1,), SENTINEL if dtype == torch.int16 else SENTINEL * 65537, dtype=dtype, device=dev)
        d = hip.PackDesc()
        d.src, d.Cout, d.Cin, d.R, d.S, d.ndst = wd.data_ptr(), Cout, Cin, R, R, 1
        d.dst[0], d.mode[0] = raw[1:].data_ptr(), m
        hip.check(hip.lib().mrfa_pack_conv_weights_multi(hip.stream_ptr(), C.pointer(d), 1), "pack_conv_weights_multi")
        torch.cuda.synchronize()
        assert torch.equal(raw[1:].cpu(), _expected(w, m, SENTINEL)), m
        assert int(raw[0]) == (SENTINEL if dtype == torch.int16 else SENTINEL * 65537)


@pytest.mark.parametrize("R", [1, 3, 5, 7])
def test_unpack_multi(R):
    dev = torch.device("cuda", 0)
    T = R * R
    shapes = [(co, ci) for co in COUTS for ci in CINS]
    descs, cases, keep = [], [], []
    for Cout, Cin in shapes:
        w = _rand(f"unpack/{Cout}/{Cin}/{R}", (Cout, Cin, R, R))
        g0 = _rand(f"unpack/g/{Cout}/{Cin}/{R}", (Cout, Cin, R, R))
        wd = w.to(dev)
        for few in (0, 1):
            if few:                                           # [Cout][tap][Cin] through the pack itself (mode 5)
                acc = torch.zeros(Cout * Cin * T, device=dev)
                d = hip.PackDesc()
                d.src, d.Cout, d.Cin, d.R, d.S, d.ndst = wd.data_ptr(), Cout, Cin, R, R, 1
                d.dst[0], d.mode[0] = acc.data_ptr(), 5
                hip.check(hip.lib().mrfa_pack_conv_weights_multi(hip.stream_ptr(), C.pointer(d), 1), "pack_conv_weights_multi")
            else:                                             # [tap][Cout][Cin]
                acc = w.reshape(Cout, Cin, T).permute(2, 0, 1).contiguous().to(dev)
            into_zero, into_g, ref_g = torch.zeros_like(wd), g0.to(dev), g0.to(dev)
            for dst in (into_zero, into_g):
                u = hip.UnpackDesc()
                u.src, u.dst, u.Cout, u.Cin, u.T, u.fewout = acc.data_ptr(), dst.data_ptr(), Cout, Cin, T, few
                descs.append(u)
            hip.check(hip.lib().mrfa_pack_conv_weight(hip.stream_ptr(), acc.data_ptr(), ref_g.data_ptr(), Cout, Cin, R, R,
                                                      hip.UNPACK_ACC_FEWOUT if few else hip.UNPACK_ACC), "unpack(single)")
            cases.append(((Cout, Cin, few), wd, into_zero, into_g, ref_g))
            keep.append(acc)
    table = (hip.UnpackDesc * len(descs))(*descs)
    assert len(descs) > 48
    hip.check(hip.lib().mrfa_unpack_wgrads_multi(hip.stream_ptr(), table, len(descs)), "unpack_wgrads_multi")
    torch.cuda.synchronize()
    bad = []
    for what, wd, into_zero, into_g, ref_g in cases:
        if not torch.equal(into_zero.view(torch.int32), wd.view(torch.int32)):
            bad.append((what, "round trip"))
        if not torch.equal(into_g.view(torch.int32), ref_g.view(torch.int32)):
            bad.append((what, "+= against the single-tensor unpack"))
    assert not bad, bad
