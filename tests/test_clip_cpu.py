"""A clip against one cached source on the CPU, through the ABI emulator (tests/emu.py; mrfa_corr_direct_rep_fwd =
mrfa_corr_direct_fwd on repeated keys): B = Bs T driving frames, frame n of source n // T, against the same program on a physically replicated source
(repeat_interleave(T) of source, kp_s and cache); what the default paths hand the library; what is refused."""
import pytest
import torch

from mrfa_amd import engine, hip
from mrfa_amd.engine import Storage, View
from mrfa_amd.modules import RaftFlow
from oracle.capi_emulator import Emulator
from tests import cases
from tests.emu import emulated_hip
from tests.test_oracle_golden import raft_inputs

SIZE, BS, T = 64, 2, 3
GOLDEN_MAX, GOLDEN_MEAN = 1e-3, 1e-4


def _raft(prior_only=False):
    rf = RaftFlow(**cases.raft_cfg(SIZE, prior_only))
    rf.load_state_dict(cases.weights_for(rf.state_dict(), "rf"))
    return rf.eval()


def clip_inputs(to=lambda t: t):
    """BS sources and BS*T driving inputs: (kp_s, img, img_full) of raft_inputs(SIZE, BS), (kp_d, deformation, occlusion) of raft_inputs(SIZE, BS*T)"""
    kp_s, _, _, img, img_full = raft_inputs(SIZE, BS, "clip/src")
    _, kp_d, dmo, _, _ = raft_inputs(SIZE, BS * T, "clip/drv")
    return to(kp_s), to(kp_d), {k: to(v) for k, v in dmo.items()}, to(img), to(img_full)


def replicate_view(v: View, t: int) -> View:
    data = v.st.data.view(v.N, v.H * v.W, v.ld).repeat_interleave(t, dim=0).reshape(-1, v.ld).contiguous()
    return View(Storage(data), v.N * t, v.H, v.W, v.C, v.coff, v.zpad)


def replicate_cache(cache: dict, t: int) -> dict:
    """the cache encode_source would return for the sources repeated t times each (the parent's workaround)"""
    rep = dict(cache)
    rep["imgf"] = replicate_view(cache["imgf"], t)
    rep["feature"] = [replicate_view(f, t) for f in cache["feature"]]
    rep["shape"] = (cache["shape"][0] * t,) + tuple(cache["shape"][1:])
    for k in ("k_s", "k_pool"):
        if k in cache:
            rep[k] = replicate_view(cache[k], t)
    return rep


def test_emulator_rep_entry_refuses_its_two_bad_arguments_and_the_parents():
    emu = Emulator()
    assert emu.mrfa_version() == hip.ABI_VERSION
    assert "mrfa_corr_direct_rep_fwd" in hip.EXPORTED_SYMBOLS
    q, k0, k1 = torch.randn(4 * 6, 8), torch.randn(16 * 2, 8), torch.randn(4 * 2, 8)
    c, out = torch.zeros(4 * 6, 2), torch.full((4 * 6, 98), 7.0)
    args = dict(q=q.data_ptr(), ldq=8, k0=k0.data_ptr(), ldk0=8, k1=k1.data_ptr(), ldk1=8, N=6, k_rep=3, h1=2, w1=2, Hs=4, Ws=4, D=8, coords=c.data_ptr(),
                ldc=2, radius=3, scale=0.5, out=out.data_ptr(), ldo=98)
    assert emu.mrfa_corr_direct_rep_fwd(0, **args) == 0 and not (out == 7).any()
    for bad in (dict(k_rep=4), dict(k_rep=0), dict(k_rep=-1), dict(radius=4), dict(D=6), dict(ldo=97), dict(Hs=3), dict(ldk0=4), dict(k1=k1.data_ptr() + 4)):
        out.fill_(7.0)
        assert emu.mrfa_corr_direct_rep_fwd(0, **{**args, **bad}) != 0 and len(emu.mrfa_last_error()) > 10, bad
        assert (out == 7).all(), bad


def test_ctx_corr_direct_k_rep_equals_repeated_keys():
    with emulated_hip(counting=True) as lib:
        e = engine.Ctx(torch.device("cpu"), train=False, record=False)
        g = torch.Generator().manual_seed(5)
        q, k0, co = e.new(6, 3, 5, 16), e.new(2, 6, 4, 16), e.new(6, 3, 5, 2)
        q.tensor().copy_(torch.randn(6, 3, 5, 16, generator=g))
        k0.tensor().copy_(torch.randn(2, 6, 4, 16, generator=g))
        co.tensor().copy_(torch.rand(6, 3, 5, 2, generator=g) * 8 - 2)
        k1 = e.avgpool2(k0)
        del lib.calls[:]
        got = e.corr_direct(q, k0, k1, co, 0.25, radius=2, k_rep=3)
        assert [n for n, _ in lib.calls] == ["mrfa_corr_direct_rep_fwd"]
        del lib.calls[:]
        ref = e.corr_direct(q, replicate_view(k0, 3), replicate_view(k1, 3), co, 0.25, radius=2)
        assert [n for n, _ in lib.calls] == ["mrfa_corr_direct_fwd"]
        assert torch.equal(got.tensor(), ref.tensor()) and got.tensor().abs().max() > 0.1
        # key image n // k_rep, not n % k_rep: frames 0..2 read key 0
        wrong = e.corr_direct(q, View(Storage(k0.st.data.view(2, -1, k0.ld).repeat(3, 1, 1).reshape(-1, k0.ld).contiguous()), 6, 6, 4, 16),
                              View(Storage(k1.st.data.view(2, -1, k1.ld).repeat(3, 1, 1).reshape(-1, k1.ld).contiguous()), 6, 3, 2, 16), co, 0.25, radius=2)
        assert not torch.equal(got.tensor(), wrong.tensor())
        with pytest.raises(AssertionError, match="k_rep"):
            e.corr_direct(q, k0, k1, co, 0.25, radius=2, k_rep=2)
        r = engine.Ctx(torch.device("cpu"), train=False, record=True)
        with pytest.raises(RuntimeError, match="no backward"):
            r.corr_direct(q, k0, k1, co, 0.25, k_rep=3)


@pytest.mark.parametrize("corr", ["direct", "volume"])
@pytest.mark.parametrize("prior_only", [False, True])
def test_raft_flow_clip_equals_replicated_source(corr, prior_only):
    """corr="direct" (and the prior-only program, which has no correlation): every emulated operation has the same shape in both runs -> torch.equal.
    corr="volume": the volume matmul has another batch shape (Bs problems of T Q rows against B of Q) -> the golden gate."""
    with emulated_hip():
        rf = _raft(prior_only)
        kp_s, kp_d, dmo, img, img_full = clip_inputs()
        with torch.no_grad():
            cache = rf.encode_source(kp_s, img, img_full)
            got = rf(kp_s, kp_d, dmo, img, img_full, source_cache=cache, corr=corr)
            ri = lambda t: t.repeat_interleave(T, dim=0)
            ref = rf(ri(kp_s), kp_d, dmo, ri(img), ri(img_full), source_cache=replicate_cache(cache, T), corr=corr)
    for name, a, b in zip(("out", "warp", "strip"), got, ref):
        assert a.shape == b.shape and a.shape[0] == BS * T and torch.isfinite(a).all()
        d = (a - b).abs()
        print(f"[clip] emulator, corr={corr}, prior_only={prior_only}, {name}: max |diff| {d.max().item():.3e} mean {d.mean().item():.3e}")
        if corr == "direct" or prior_only:
            assert torch.equal(a, b), name
        else:
            assert d.max().item() <= GOLDEN_MAX and d.mean().item() <= GOLDEN_MEAN, name
    assert (got[1][:T] - got[1][T:]).abs().mean().item() > 1e-3           # two sources, really distinct


@pytest.mark.parametrize("corr", ["direct", "volume"])
def test_same_batch_reaches_only_the_parents_entry_points(corr):
    with emulated_hip(counting=True) as lib:
        rf = _raft()
        kp_s, kp_d, dmo, img, img_full = raft_inputs(SIZE, BS, "clip/src")
        with torch.no_grad():
            cache = rf.encode_source(kp_s, img, img_full)
            del lib.calls[:]
            rf(kp_s, kp_d, dmo, img, img_full, source_cache=cache, corr=corr)
            rf(kp_s, kp_d, dmo, img, img_full, corr=corr)
        names = [n for n, _ in lib.calls]
        assert "mrfa_corr_direct_rep_fwd" not in names
        assert names.count("mrfa_corr_direct_fwd") == (12 if corr == "direct" else 0)
        warps = [a for n, a in lib.calls if n in ("mrfa_grid_sample_fwd", "mrfa_grid_sample_bf16_fwd")]
        assert len(warps) > 20 and all(a[4] == 1 for a in warps)              # in_rep: (stream, in, ldi, in_bstride, in_rep, ...)


def test_clip_reaches_the_rep_entry_and_in_rep():
    with emulated_hip(counting=True) as lib:
        rf = _raft()
        kp_s, kp_d, dmo, img, img_full = clip_inputs()
        with torch.no_grad():
            cache = rf.encode_source(kp_s, img, img_full, feature_dtype=torch.bfloat16)
            del lib.calls[:]
            rf(kp_s, kp_d, dmo, img, img_full, source_cache=cache, corr="direct")
        names = [n for n, _ in lib.calls]
        assert names.count("mrfa_corr_direct_rep_fwd") == 6 and "mrfa_corr_direct_fwd" not in names
        assert all(a[8] == T for n, a in lib.calls if n == "mrfa_corr_direct_rep_fwd")
        warps = [a for n, a in lib.calls if n in ("mrfa_grid_sample_fwd", "mrfa_grid_sample_bf16_fwd")]
        assert "mrfa_grid_sample_bf16_fwd" in names and all(a[4] == T for a in warps)


def test_batch_mismatch_is_refused():
    with emulated_hip(counting=True) as lib:
        rf = _raft()
        kp_s, kp_d, dmo, img, img_full = clip_inputs()
        with torch.no_grad():
            cache = rf.encode_source(kp_s, img, img_full)
            del lib.calls[:]
            bad = {k: v[:5] for k, v in dmo.items()}
            with pytest.raises(ValueError, match=r"5.*2"):
                rf(kp_s, kp_d[:5], bad, img, img_full, source_cache=cache)
            with pytest.raises(ValueError, match="source_cache"):
                rf(kp_s, kp_d, dmo, img, img_full)
        with torch.enable_grad():
            with pytest.raises(ValueError, match="no backward"):
                rf(kp_s, kp_d, dmo, img, img_full, source_cache=cache)
        rf.train()
        with torch.no_grad():
            with pytest.raises(ValueError, match="inference"):
                rf(kp_s, kp_d, dmo, img, img_full, source_cache=cache)
        assert not lib.calls                                                   # refused before anything was launched
        rf.eval()


def _clips(n):
    from mrfa_amd.utils.prng import det_uniform
    src = det_uniform("clip/anim/src", (BS, 3, SIZE, SIZE), 0, 1)
    clip = torch.stack([det_uniform(f"clip/anim/drv{t}", (BS, 3, SIZE, SIZE), 0, 1) for t in range(n)], dim=2)
    return src, clip


def _gate(a, b, what):
    d = (a - b).abs()
    print(f"[clip] {what}: max |diff| {d.max().item():.3e} mean {d.mean().item():.3e}")
    assert a.shape == b.shape and torch.isfinite(a).all()
    assert d.max().item() <= GOLDEN_MAX and d.mean().item() <= GOLDEN_MEAN, what


def test_callers_frames_per_call():
    from mrfa_amd.infer import Animator, make_animation, reconstruction
    from tests.test_bf16_cache import _dry_model
    with emulated_hip(counting=True) as lib:
        m = _dry_model()
        src, clip = _clips(4)                                                  # groups of 3: one full group and a tail of 1
        for bad in (0, -1):
            with pytest.raises(ValueError, match="frames_per_call"):
                make_animation(m, src, clip, frames_per_call=bad)
            with pytest.raises(ValueError, match="frames_per_call"):
                reconstruction(m, clip, frames_per_call=bad)
        an = Animator(m)
        an.set_source(src)
        with pytest.raises(ValueError, match=r"3.*2"):
            an(clip[:, :, 0][[0, 1, 0]].contiguous())
        # B == Bs: the per-frame program, no clip entry point and in_rep == 1 everywhere
        del lib.calls[:]
        f0 = an(clip[:, :, 0].contiguous()).clone()
        assert "mrfa_corr_direct_rep_fwd" not in [n for n, _ in lib.calls]
        assert all(a[4] == 1 for n, a in lib.calls if n in ("mrfa_grid_sample_fwd", "mrfa_grid_sample_bf16_fwd"))
        # one call of Bs*3 frames against three per-frame calls
        group = clip[:, :, :3].permute(0, 2, 1, 3, 4).reshape(BS * 3, 3, SIZE, SIZE).contiguous()
        fc = an(group).view(BS, 3, 3, SIZE, SIZE)
        _gate(fc[:, 0], f0, "Animator clip frame 0 vs per-frame")
        _gate(fc[:, 2], an(clip[:, :, 2].contiguous()), "Animator clip frame 2 vs per-frame")
        for corr in ("volume", "direct"):
            a1 = make_animation(m, src, clip, relative=True, adapt_movement_scale=True, corr=corr, frames_per_call=1)
            a3 = make_animation(m, src, clip, relative=True, adapt_movement_scale=True, corr=corr, frames_per_call=3)
            assert a1.shape == a3.shape == clip.shape
            _gate(a3, a1, f"make_animation corr={corr} frames_per_call 3 vs 1")
        r1, r3 = reconstruction(m, clip, frames_per_call=1), reconstruction(m, clip, frames_per_call=3)
        assert r1["prediction"].shape == r3["prediction"].shape == clip.shape and len(r3["l1"]) == len(r3["psnr"]) == 4
        _gate(r3["prediction"], r1["prediction"], "reconstruction frames_per_call 3 vs 1")
        assert max(abs(a - b) for a, b in zip(r1["l1"], r3["l1"])) <= 1e-4


def test_one_source_many_frames():
    """Bs = 1 (the demo loop's case): a repeat of ONE image is a stride-0 expansion until it is copied"""
    from mrfa_amd.infer import Animator
    from tests.test_bf16_cache import _dry_model
    with emulated_hip():
        m = _dry_model()
        src, clip = _clips(2)
        an = Animator(m, corr="direct")
        an.set_source(src[:1].contiguous())
        out = an(clip[0].permute(1, 0, 2, 3).contiguous())
        for t in range(2):
            _gate(out[t:t + 1], an(clip[:1, :, t].contiguous()), f"one source, frame {t} of a 2-frame call vs the per-frame call")
