"""The bf16 source-feature cache of the animation loop: RaftFlow.encode_source(feature_dtype=torch.bfloat16) / Animator(cache_dtype=torch.bfloat16),
the two kernels behind it (mrfa_cast_bf16, mrfa_grid_sample_bf16_fwd) and the dtype rule of engine.View.

Module parity (CPU through the ABI emulator, tests/emu.py, and on the GPU): the expected value is the reference-pinned oracle run on THE SAME
ROUNDED PYRAMID -- the bf16 cache is read back, widened (exact) and handed to the oracle in place of its own generator_encode -- so everything downstream of
the pyramid is the same program on both sides and the project's module-parity bound applies for its usual reason: max |diff| <= 1e-3, mean <= 1e-4
(tests/test_parity_gpu.py::_cmp).  That the rounded pyramid itself is right is the cast test (bit-identical round-to-nearest-even) plus the existing fp32
pyramid tests."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mrfa_amd import engine, hip
from mrfa_amd.modules import RaftFlow
from oracle import mrfa_oracle as O
from tests import cases
from tests.emu import cache_pyramid_bytes, cache_pyramid_nchw, emulated_hip, oracle_pyramid
from tests.sample_grids import gs_grid as _gs_grid
from tests.test_oracle_golden import raft_inputs

DEV = "cuda:0"


def _cmp(got, ref, max_tol=1e-3, mean_tol=1e-4, what=""):
    got = got.detach().float().cpu().numpy()
    ref = ref.detach().float().cpu().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    d = np.abs(got - ref)
    print(f"[bf16 cache] {what}: max |diff| {d.max():.3e}  mean {d.mean():.3e}")
    assert d.max() <= max_tol and d.mean() <= mean_tol, f"{what}: max {d.max():.3e} mean {d.mean():.3e}"


def _raft(size, prior_only, dev):
    rf = RaftFlow(**cases.raft_cfg(size, prior_only))
    sd = cases.weights_for(rf.state_dict(), "rf")
    rf.load_state_dict(sd)
    return rf.to(dev).eval(), sd


def _raft_parity(size, b, prior_only, dev, tag):
    """RaftFlow from a bf16 source cache against the oracle on the same rounded pyramid"""
    rf, sd = _raft(size, prior_only, dev)
    kp_s, kp_d, dmo, img, img_full = raft_inputs(size, b, tag)
    to = lambda t: t.to(dev)
    with torch.no_grad():
        cache = rf.encode_source(to(kp_s), to(img), to(img_full), feature_dtype=torch.bfloat16)
        assert cache["dtype"] == torch.bfloat16 and all(f.dtype == torch.bfloat16 for f in cache["feature"])
        o, w, s = rf(to(kp_s), to(kp_d), {k: to(v) for k, v in dmo.items()}, to(img), to(img_full), source_cache=cache)
        with oracle_pyramid(cache_pyramid_nchw(cache)):
            oo, ow, _ = O.raft_flow(kp_s, kp_d, dmo, img, img_full, {k: v.clone() for k, v in sd.items()}, "", size=size, prior_only=prior_only)
    what = f"{size}^2 b{b} {'prior_only' if prior_only else 'refinement'}"
    _cmp(o, oo, what="out " + what)
    _cmp(w, ow, what="warp " + what)
    assert s.shape == (b, 1, size, (6 if prior_only else 7) * size)


# ------------------------------------------------------------------------------------------------------------------ CPU, through the emulator
def test_encode_source_bf16_storages_and_bytes():
    size, b = 64, 2
    with emulated_hip():
        rf, _ = _raft(size, False, "cpu")
        kp_s, _, _, img, img_full = raft_inputs(size, b, "bf16/enc")
        c32 = rf.encode_source(kp_s, img, img_full)
        c16 = rf.encode_source(kp_s, img, img_full, feature_dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="float32.*bfloat16"):
            rf.encode_source(kp_s, img, img_full, feature_dtype=torch.float16)
    assert len(c16["feature"]) == 6 and all(f.C % 8 == 0 for f in c32["feature"])
    for f32, f16 in zip(c32["feature"], c16["feature"]):
        assert f32.dtype == torch.float32 and f32.st.data.dtype == torch.float32
        assert f16.dtype == torch.bfloat16 and f16.st.data.dtype == torch.bfloat16 and f16.st.grad is None
        assert (f16.N, f16.H, f16.W, f16.C) == (f32.N, f32.H, f32.W, f32.C)
        assert torch.equal(f16.st.data, f32.tensor().reshape(f32.rows, f32.C).to(torch.bfloat16))          # the cast IS round-to-nearest-even
    for k in ("imgf", "k_s", "k_pool"):
        assert c16[k].dtype == torch.float32 and torch.equal(c16[k].tensor(), c32[k].tensor()), k
    assert c16["dtype"] == torch.bfloat16 and c32["dtype"] == torch.float32
    assert 2 * cache_pyramid_bytes(c16) == cache_pyramid_bytes(c32)


def test_bf16_view_never_reaches_an_fp32_kernel():
    with emulated_hip():
        e = engine.Ctx(torch.device("cpu"), train=False, record=False)
        x = e.new(1, 4, 4, 16)
        x.tensor().copy_(torch.randn(1, 4, 4, 16))
        h = e.to_bf16(x)
        assert h.dtype == torch.bfloat16 and x.dtype == torch.float32 and h.ld == h.C == 16
        assert h.ptr16 == h.st.data.data_ptr() and h.slice(8, 16).ptr16 == h.st.data.data_ptr() + 16
        with pytest.raises(TypeError, match="fp32 kernel"):
            h.ptr
        with pytest.raises(TypeError):
            x.ptr16
        with pytest.raises(TypeError):
            h.gptr                                                            # no gradient buffer, ever
        conv = torch.nn.Conv2d(16, 8, 1)
        with pytest.raises(TypeError, match="fp32 kernel"):
            e.conv(h, conv)
        for op in (lambda: e.copy(h), lambda: e.resize(h, 8, 8), lambda: e.to_nchw(h), lambda: e.act(h, 2), lambda: e.to_bf16(h)):
            with pytest.raises(TypeError):
                op()
        grid = e.new(1, 4, 4, 2, zero=True)
        with pytest.raises(TypeError):                                        # a bf16 GRID is refused too: only the sampled input may be bf16
            e.grid_sample(x, e.to_bf16(e.new(1, 4, 4, 8, zero=True)).slice(0, 2), 1)
        out = e.grid_sample(h, grid, 1)                                       # zero flow on the identity grid: the widened input
        assert (out.tensor() - h.tensor().float()).abs().max().item() <= 1e-5
        with pytest.raises(RuntimeError, match="C % 8"):                      # a channel count the kernel does not take is an error, not a slow path
            e.grid_sample(e.to_bf16(e.new(1, 4, 4, 16, zero=True)).slice(0, 12), grid, 1)
        r = engine.Ctx(torch.device("cpu"), train=False, record=True)
        with pytest.raises(RuntimeError, match="inference"):
            r.to_bf16(x)
        with pytest.raises(RuntimeError, match="no backward"):
            r.grid_sample(h, grid, 1)


def _dry_model():
    from mrfa_amd.train import HotPath
    from mrfa_amd.utils.prng import fill_state_dict
    from tests.bench_dry_run import DRY_CFG
    model = HotPath(DRY_CFG, prior="fomm")
    for pfx, mod in (("encoder.", model.encoder), ("dense_motion.", model.dense_motion), ("decoder.", model.decoder)):
        mod.load_state_dict(fill_state_dict(mod.state_dict(), tag="bf16/" + pfx))
    return model.eval()


def test_animator_cache_dtype_argument():
    from mrfa_amd.infer import Animator, make_animation, reconstruction
    from mrfa_amd.utils.prng import det_uniform
    with emulated_hip():
        m = _dry_model()
        for bad in (torch.float16, torch.float64, None):
            with pytest.raises(ValueError, match="torch.float32 or torch.bfloat16"):
                Animator(m, cache_dtype=bad)
        src = det_uniform("bf16/anim/src", (1, 3, 64, 64), 0, 1)
        drv = [det_uniform(f"bf16/anim/drv{t}", (1, 3, 64, 64), 0, 1) for t in range(2)]
        clip = torch.stack(drv, dim=2)
        with pytest.raises(ValueError):
            make_animation(m, src, clip, cache_dtype=torch.float16)
        with pytest.raises(ValueError):
            reconstruction(m, clip, cache_dtype=torch.float16)
        a, b, h = Animator(m), Animator(m, cache_dtype=torch.float32), Animator(m, cache_dtype=torch.bfloat16)
        for an in (a, b, h):
            an.set_source(src)
        assert all(f.dtype == torch.float32 for f in a.cache["feature"] + b.cache["feature"])
        assert all(f.dtype == torch.bfloat16 for f in h.cache["feature"])
        for d in drv:
            fa, fb, fh = a(d).clone(), b(d).clone(), h(d).clone()
            assert torch.equal(fa, fb)                                        # the default path is the old path
            assert torch.isfinite(fh).all() and (fh - fa).abs().max().item() > 0
        r = reconstruction(m, clip, cache_dtype=torch.bfloat16)
        h.set_source(drv[0])                                                  # (reconstruction: source = frame 0 of the clip)
        assert torch.equal(r["prediction"][:, :, 1], h(drv[1]))
        assert make_animation(m, src, clip, cache_dtype=torch.bfloat16).shape == clip.shape


@pytest.mark.parametrize("prior_only", [False, True])
def test_raft_flow_from_bf16_cache_through_emulator(prior_only):
    with emulated_hip():
        _raft_parity(64, 2, prior_only, "cpu", "bf16/raft64")


# ------------------------------------------------------------------------------------------------------------------ GPU: the kernels
def _bits(t):
    return t.contiguous().view(torch.int16)


def _cast(x2d, Cc, coff=0):
    """mrfa_cast_bf16 on channels [coff, coff + Cc) of the [rows, ld] fp32 tensor x2d -> [rows, Cc] bf16"""
    rows, ld = x2d.shape
    y = torch.empty((rows, Cc), dtype=torch.bfloat16, device=x2d.device)
    hip.check(hip.lib().mrfa_cast_bf16(hip.stream_ptr(), x2d.data_ptr() + 4 * coff, ld, rows, Cc, y.data_ptr(), Cc), "cast_bf16")
    torch.cuda.synchronize()
    return y


@pytest.mark.gpu
def test_cast_bf16_is_bit_identical_round_to_nearest_even():
    g = torch.Generator().manual_seed(5)
    parts = [torch.randn(4096, generator=g) * 3.0, torch.randn(4096, generator=g) * 1e-3, torch.randn(2048, generator=g) * 1e20]
    k = torch.arange(-300, 300, dtype=torch.float32)
    ties = k * 2.0 ** -8 + 2.0 ** -9                                         # exactly half-way between two bf16 values when 1 <= |value| < 2
    for ex in (-100, -20, -1, 0, 1, 7, 60, 120):
        parts.append(ties * 2.0 ** ex)
    tie_bits = torch.tensor([0x3F808000, 0x3F818000, 0x3F828000, 0x3F838000, 0xBF808000, 0xBF818000, 0x7F7F8000, 0x00008000, 0x00018000],
                            dtype=torch.int64).to(torch.int32).view(torch.float32)                # mantissa ...|1000 0000 0000 0000: ties, even / odd upper halves
    parts.append(tie_bits)
    den = torch.tensor([1, 2, 0x7FFF, 0x8000, 0x8001, 0x17FFF, 0x18000, 0x7FFFFF, 0x400000, 0x3F8000], dtype=torch.int32)
    parts += [den.view(torch.float32), (den | -0x80000000).view(torch.float32)]                  # denormals of both signs
    fmax = torch.finfo(torch.float32).max
    parts.append(torch.tensor([0.0, -0.0, float("inf"), float("-inf"), fmax, -fmax, 1.0, -1.0]))
    x = torch.cat(parts)
    x = torch.cat([x, torch.zeros(-x.numel() % 64)]).view(-1, 64)
    ref = x.to(torch.bfloat16)                                                # the specification
    assert torch.isinf(ref[x.abs() == fmax]).all()                            # the largest finite fp32 rounds to infinity, as torch does
    pos = ties[(ties >= 1) & (ties < 2)]                                      # (half an ulp of bf16 is 2^-8 there: every one is a tie)
    rt = pos.to(torch.bfloat16).float()
    assert (rt > pos).any() and (rt < pos).any() and (rt != pos).all()        # the ties round up to even AND down to even
    got = _cast(x.to(DEV), 64)
    assert torch.equal(_bits(got).cpu(), _bits(ref)), "contiguous source"
    # source view with ld > C and a channel offset
    wide = torch.full((x.shape[0], 96), float("nan"))
    wide[:, 24:88] = x
    got = _cast(wide.to(DEV), 64, coff=24)
    assert torch.equal(_bits(got).cpu(), _bits(ref)), "ld > C, channel offset"
    got = _cast(wide.to(DEV), 8, coff=32)
    assert torch.equal(_bits(got).cpu(), _bits(ref[:, 8:16])), "C = 8"
    # NaN stays NaN, whatever its payload (the rounding carry alone would turn 0x7F80xxxx / 0x7FFFxxxx payloads into +-inf / -0)
    nan_bits = torch.tensor([0x7FC00000, 0x7F800001, 0x7F80FFFF, 0x7FFFFFFF, 0x7FFF8000, 0xFF800001, 0xFFFFFFFF, 0x7F808000], dtype=torch.int64)
    xn = torch.ones(8, 8)
    xn[:, 3] = nan_bits.to(torch.int32).view(torch.float32)
    assert torch.isnan(xn[:, 3]).all()
    got = _cast(xn.to(DEV), 8).cpu()
    assert torch.isnan(got[:, 3]).all() and (got.float()[:, [0, 1, 2, 4, 5, 6, 7]] == 1).all()


def _tap_max(xw, grid, N, in_rep, Hi, Wi, Ho, Wo, mode):
    """max |tap| over the (existing) four taps of every output element: the scale of the derived bound.  xw: [Nin, Hi, Wi, C] fp32 (widened input)"""
    gx, gy = grid[:, 0].view(N, Ho, Wo), grid[:, 1].view(N, Ho, Wo)
    if mode == 0:
        ix, iy = ((gx + 1) * Wi - 1) * 0.5, ((gy + 1) * Hi - 1) * 0.5
    else:
        ix = gx + torch.arange(Wo, dtype=torch.float32).view(1, 1, Wo)
        iy = gy + torch.arange(Ho, dtype=torch.float32).view(1, Ho, 1)
    inr = (ix > -1) & (iy > -1) & (ix < Wi) & (iy < Hi)
    ix, iy = torch.where(inr, ix, torch.zeros_like(ix)), torch.where(inr, iy, torch.zeros_like(iy))
    x0, y0 = ix.floor().long(), iy.floor().long()
    src = xw.abs().repeat_interleave(in_rep, dim=0)[:N]
    n_idx = torch.arange(N).view(N, 1, 1).expand(N, Ho, Wo)
    m = torch.zeros(N, Ho, Wo, xw.shape[-1])
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            ok = inr & (xx >= 0) & (xx < Wi) & (yy >= 0) & (yy < Hi)
            t = src[n_idx, yy.clamp(0, Hi - 1), xx.clamp(0, Wi - 1)]
            m = torch.maximum(m, torch.where(ok[..., None], torch.nan_to_num(t, nan=0.0, posinf=0.0), torch.zeros_like(t)))
    return m


def _gs_pair(x16, ldi, Cc, grid, N, in_rep, Hi, Wi, Ho, Wo, mode, ldo, ooff):
    """(bf16 kernel on x16, fp32 kernel on the widened copy of x16), both [N*Ho*Wo, Cc], written into channel slices of wider buffers"""
    L = hip.lib()
    x16 = x16.to(DEV)
    x32 = x16.float()
    gd = grid.to(DEV)
    outs = []
    for bf in (True, False):
        out = torch.full((N * Ho * Wo, ldo), -77.0, device=DEV)
        fn = L.mrfa_grid_sample_bf16_fwd if bf else L.mrfa_grid_sample_fwd
        src = x16 if bf else x32
        hip.check(fn(hip.stream_ptr(), src.data_ptr(), ldi, Hi * Wi * ldi, in_rep, Hi, Wi, Cc, gd.data_ptr(), 2, N, Ho, Wo,
                     out.data_ptr() + 4 * ooff, ldo, mode), "grid_sample")
        torch.cuda.synchronize()
        assert (out[:, :ooff] == -77).all() and (out[:, ooff + Cc:] == -77).all(), "wrote outside its channel slice"
        outs.append(out[:, ooff:ooff + Cc].cpu())
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Cc", [8, 24, 64, 128, 256, 512, 520])
def test_grid_sample_bf16_equals_fp32_kernel_on_widened_input(Cc, mode):
    """expected difference: zero (identical inputs after widening, the same expression).  Allowed: what two evaluation orders of a four-term fp32 dot product
    can differ by -- four roundings of half an ulp (2^-24 relative) on terms bounded by the largest tap, weights summing to at most one: 2^-22 max|tap|"""
    Hi, Wi, Ho, Wo = 9, 7, 11, 13
    seen = 0.0
    for in_rep, Nin in ((1, 3), (3, 1)):
        N = Nin * in_rep
        for ldi, ldo, ooff in ((Cc, Cc, 0), (Cc + 8, 2 * Cc + 4, Cc + 4)):       # dense; input in a wider row, output = a channel slice of a wider buffer
            g = torch.Generator().manual_seed(Cc * 10 + mode)
            x16 = (torch.randn(Nin * Hi * Wi, ldi, generator=g) * 4).to(torch.bfloat16)
            grid, outside = _gs_grid(N, Ho, Wo, Hi, Wi, mode, seed=Cc + in_rep)
            got, ref = _gs_pair(x16, ldi, Cc, grid, N, in_rep, Hi, Wi, Ho, Wo, mode, ldo, ooff)
            assert torch.isfinite(got).all()
            assert (got[outside] == 0).all() and (ref[outside] == 0).all()
            bound = 2.0 ** -22 * _tap_max(x16.float().view(Nin, Hi, Wi, ldi)[..., :Cc], grid, N, in_rep, Hi, Wi, Ho, Wo, mode).view(-1, Cc)
            d = (got - ref).abs()
            seen = max(seen, d.max().item())
            assert (d <= bound).all(), (in_rep, ldi, d.max().item())
            assert got.abs().max() > 1                                              # (it sampled something)
    print(f"[bf16 cache] grid_sample_bf16 vs fp32 kernel on the widened input, C={Cc} mode={mode}: max |diff| seen {seen:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_grid_sample_bf16_outside_sample_is_selected_away(mode):
    """a sample wholly outside the image reads the clamped pixel (0, 0); a non-finite value there must not leak (0 * inf = NaN)"""
    Hi, Wi, Ho, Wo, Cc = 5, 6, 4, 4, 64
    x16 = torch.ones(Hi * Wi, Cc).to(torch.bfloat16)
    x16[0] = float("inf")
    x16[1, :8] = float("nan")
    grid = torch.full((Ho * Wo, 2), -50.0)
    grid[5] = torch.tensor([float("nan"), 0.0])
    got, ref = _gs_pair(x16, Cc, Cc, grid, 1, 1, Hi, Wi, Ho, Wo, mode, Cc, 0)
    assert (got == 0).all() and (ref == 0).all()


@pytest.mark.gpu
def test_bf16_kernels_refuse_what_they_do_not_take():
    L = hip.lib()
    x = torch.zeros(64, 32, device=DEV)
    x16 = torch.zeros(64, 32, dtype=torch.bfloat16, device=DEV)
    grid = torch.zeros(64, 2, device=DEV)
    canary = torch.full((64, 32), 5.0, device=DEV)
    s = hip.stream_ptr()

    def refused(rc):
        msg = L.mrfa_last_error().decode()
        assert rc != 0 and len(msg) > 10, (rc, msg)
        return msg
    gs = lambda inp, ldi, Cc, out, ldo: L.mrfa_grid_sample_bf16_fwd(s, inp, ldi, 64 * ldi, 1, 8, 8, Cc, grid.data_ptr(), 2, 1, 8, 8, out, ldo, 1)
    assert "grid_sample_bf16_fwd" in refused(gs(x16.data_ptr(), 32, 12, canary.data_ptr(), 32))          # C = 12
    refused(gs(x16.data_ptr() + 2, 32, 8, canary.data_ptr(), 32))                                        # misaligned input
    refused(gs(x16.data_ptr(), 32, 8, canary.data_ptr() + 4, 32))                                        # misaligned output
    refused(gs(x16.data_ptr(), 12, 8, canary.data_ptr(), 32))                                            # ldi % 8
    refused(gs(x16.data_ptr(), 32, 8, canary.data_ptr(), 30))                                            # ldo % 4
    y16 = torch.full((64, 32), 5.0, dtype=torch.bfloat16, device=DEV)
    cast = lambda src, ldx, Cc, dst, ldy: L.mrfa_cast_bf16(s, src, ldx, 64, Cc, dst, ldy)
    assert "cast_bf16" in refused(cast(x.data_ptr(), 32, 12, y16.data_ptr(), 32))
    refused(cast(x.data_ptr() + 4, 32, 8, y16.data_ptr(), 32))
    refused(cast(x.data_ptr(), 32, 8, y16.data_ptr() + 2, 32))
    refused(cast(x.data_ptr(), 28, 8, y16.data_ptr(), 32))
    refused(cast(x.data_ptr(), 32, 8, y16.data_ptr(), 12))
    torch.cuda.synchronize()
    assert (canary == 5).all() and (y16 == 5).all()                                                      # nothing was launched


# ------------------------------------------------------------------------------------------------------------------ GPU: modules
@pytest.mark.gpu
@pytest.mark.parametrize("size,b,prior_only", [(256, 2, False), (256, 2, True), (512, 1, False)])
def test_raft_flow_from_bf16_cache_vs_oracle_on_the_same_pyramid(size, b, prior_only):
    _raft_parity(size, b, prior_only, DEV, "c5/raft" if size == 512 else "bf16/raft256")


@functools.lru_cache(maxsize=1)
def _mtia_model():
    import bench
    from mrfa_amd.train import VOX1, HotPath
    model = HotPath(VOX1, prior="mtia")
    P = {k: v.clone() for k, v in bench.init_weights(model).items()}
    return model.to(DEV).eval(), P


@pytest.mark.gpu
def test_graphed_animator_from_bf16_cache():
    """Animator(graph=True, cache_dtype=torch.bfloat16) captures and replays (its own eager-versus-replay gate applies), and every replayed frame passes the
    comparison of the eager module test: the oracle's whole forward on the same rounded pyramid"""
    from mrfa_amd.infer import Animator
    model, P = _mtia_model()
    b = 2
    src = cases.images("bf16/anim/src", b, 256)
    drv = [cases.images(f"bf16/anim/drv{t}", b, 256) for t in range(2)]
    an = Animator(model, graph=True, cache_dtype=torch.bfloat16)
    an.set_source(src.to(DEV))
    assert all(f.dtype == torch.bfloat16 and f.st.data.dtype == torch.bfloat16 for f in an.cache["feature"])
    pyr = cache_pyramid_nchw(an.cache)
    eager = Animator(model, graph=False, cache_dtype=torch.bfloat16)
    eager.set_source(src.to(DEV))
    for t in (0, 1, 0):                                                       # the third call replays the first frame's inputs through the static buffers
        out = an(drv[t].to(DEV)).clone()
        assert an._g is not None
        with torch.no_grad(), oracle_pyramid(pyr):
            ogen = O.mrfa_forward(src, drv[t], P, size=256, train=False, prior="mtia")[0]
        _cmp(out, ogen, what=f"replayed frame (driving {t})")
        d = (out - eager(drv[t].to(DEV))).abs()
        assert d.mean().item() <= 2e-5 and d.max().item() <= 5e-3                  # Animator's own eager-versus-replay gate, on fresh inputs


@pytest.mark.gpu
def test_bf16_cache_is_really_on():
    from mrfa_amd.infer import Animator
    model, _ = _mtia_model()
    src, drv = cases.images("bf16/on/src", 2, 256).to(DEV), cases.images("bf16/on/drv", 2, 256).to(DEV)
    a32, a16 = Animator(model), Animator(model, cache_dtype=torch.bfloat16)
    a32.set_source(src)
    a16.set_source(src)
    assert all(f.st.data.dtype == torch.float32 for f in a32.cache["feature"])
    assert all(f.st.data.dtype == torch.bfloat16 for f in a16.cache["feature"])
    assert 2 * cache_pyramid_bytes(a16.cache) == cache_pyramid_bytes(a32.cache)
    f32, f16 = a32(drv).clone(), a16(drv).clone()
    d = (f16 - f32).abs()
    print(f"[bf16 cache] bf16-cache frame vs fp32-cache frame: max |diff| {d.max().item():.3e} mean {d.mean().item():.3e} (recorded, not a gate)")
    assert torch.isfinite(f16).all() and d.max().item() > 0
