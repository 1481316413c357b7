"""Relative-motion animation on the CPU, through the ABI emulator (tests/emu.py; mrfa_kp_relative_fwd = normalize_kp on repeated first
frames and sources, the scale handed in): the entry against the reference's recorded normalize_kp, rep against physical repeats, what it refuses, the relative
Animator against the reference's recorded animation, and which Animator reaches the entry how often."""
import os

import numpy as np
import pytest
import torch

from mrfa_amd import hip
from mrfa_amd.infer import Animator, _hull_area, relative_kp
from oracle.capi_emulator import Emulator
from tests import cases
from tests.emu import emulated_hip


def _clone(kp):
    return {k: v.clone() for k, v in kp.items()}


def _entry(emu, kd, k0, ks, scale=None, rep=1, jac=True, **over):
    """one call of the emulated entry on keypoint dicts -> (rc, kp_out, jac_out); over: arguments replaced by name"""
    B, K = kd["kp"].shape[:2]
    kp_out, jac_out = torch.full((B, K, 2), 7.0), torch.full((B, K, 2, 2), 7.0)
    p = lambda t: t.data_ptr()
    a = dict(kp_d=p(kd["kp"]), jac_d=p(kd["jacobian"]) if jac else None, kp_0=p(k0["kp"]), jac_0=p(k0["jacobian"]) if jac else None, kp_s=p(ks["kp"]),
             jac_s=p(ks["jacobian"]) if jac else None, scale=p(scale) if scale is not None else None, B=B, rep=rep, K=K, kp_out=p(kp_out),
             jac_out=p(jac_out) if jac else None)
    a.update(over)
    return emu.mrfa_kp_relative_fwd(0, **a), kp_out, jac_out


def test_entry_reproduces_the_references_normalize_kp(golden_dir):
    """all six flag combinations of callers.npz through the wrapper (what the Animator does with its flags: relative=False hands the driving keypoints on)
    within the 1e-5 of tests/test_callers.py::test_normalize_kp_and_psnr_match_reference"""
    g = dict(np.load(os.path.join(golden_dir, "callers.npz")))
    ks, kd, k0 = cases.keypoints("g6/ks", 2), cases.keypoints("g6/kd", 2), cases.keypoints("g6/k0", 2)
    before = [_clone(t) for t in (ks, kd, k0)]
    assert "mrfa_kp_relative_fwd" in hip.EXPORTED_SYMBOLS and Emulator().mrfa_version() == hip.ABI_VERSION
    with emulated_hip(counting=True) as lib:
        for adapt in (False, True):
            scale = (torch.sqrt(_hull_area(ks["kp"][0])) / torch.sqrt(_hull_area(k0["kp"][0]))).reshape(1) if adapt else None
            for rel, relj in ((False, False), (True, False), (True, True)):
                del lib.calls[:]
                r = relative_kp(ks, kd, k0, scale=scale, use_relative_jacobian=relj) if rel else dict(kd)
                assert [n for n, _ in lib.calls if n == "mrfa_kp_relative_fwd"] == ["mrfa_kp_relative_fwd"] * int(rel)
                tag = f"a{int(adapt)}_r{int(rel)}_j{int(relj)}"
                ek, ej = np.abs(r["kp"].numpy() - g[f"norm_kp_{tag}"]).max(), np.abs(r["jacobian"].numpy() - g[f"norm_jac_{tag}"]).max()
                print(f"[relative] {tag}: kp max |diff| {ek:.3e}  jacobian max |diff| {ej:.3e}")
                assert ek <= 1e-5 and ej <= 1e-5, tag
                if rel and not relj:
                    assert r["jacobian"] is kd["jacobian"]                 # passed through, like every other key
    for now, was in zip((ks, kd, k0), before):
        assert all(torch.equal(now[k], was[k]) for k in was), "inputs must not be modified"


@pytest.mark.parametrize("jac", [True, False])
def test_rep_equals_physically_repeated_inputs(jac):
    emu, rep = Emulator(), 3
    kd, k0, ks = cases.keypoints("rel/rep/kd", 6, 15), cases.keypoints("rel/rep/k0", 2, 15), cases.keypoints("rel/rep/ks", 2, 15)
    scale = torch.tensor([0.37])
    rc, kp, jo = _entry(emu, kd, k0, ks, scale, rep=rep, jac=jac)
    ri = lambda d: {k: v.repeat_interleave(rep, dim=0).contiguous() for k, v in d.items()}
    rc1, kp1, jo1 = _entry(emu, kd, ri(k0), ri(ks), scale, rep=1, jac=jac)
    assert rc == 0 and rc1 == 0 and torch.equal(kp, kp1) and not (kp == 7).any()
    assert torch.equal(jo, jo1) and bool((jo == 7).all()) != jac
    # entry n // rep, not n % rep
    rp = lambda d: {k: v.repeat(rep, 1, 1) if v.dim() == 3 else v.repeat(rep, 1, 1, 1) for k, v in d.items()}
    _, kp2, _ = _entry(emu, kd, rp(k0), rp(ks), scale, rep=1, jac=jac)
    assert not torch.equal(kp, kp2)


def test_entry_refuses_bad_arguments_and_leaves_the_outputs_untouched():
    emu = Emulator()
    kd, k0, ks = cases.keypoints("rel/bad/kd", 6), cases.keypoints("rel/bad/k0", 2), cases.keypoints("rel/bad/ks", 2)
    rc, kp, jo = _entry(emu, kd, k0, ks, rep=3)
    assert rc == 0 and not (kp == 7).any() and not (jo == 7).any()
    bads = [dict(jac_d=None), dict(jac_0=None), dict(jac_s=None), dict(jac_out=None), dict(jac_d=None, jac_0=None, jac_s=None),      # partial Jacobian sets
            dict(kp_d=None), dict(kp_0=None), dict(kp_s=None), dict(kp_out=None),                                                     # null required pointer
            dict(B=0), dict(B=-3), dict(K=0), dict(rep=0), dict(rep=-1),                                                              # sizes < 1
            dict(rep=4), dict(rep=5), dict(B=5)]                                                                                      # B % rep != 0
    for bad in bads:
        rc, kp, jo = _entry(emu, kd, k0, ks, **{"rep": 3, **bad})
        assert rc != 0 and len(emu.mrfa_last_error()) > 10, bad
        assert (kp == 7).all() and (jo == 7).all(), bad
    rc, kp, jo = _entry(emu, kd, k0, ks, rep=3, kp_0=k0["kp"].data_ptr() + 4)         # a keypoint pair that straddles two vector loads
    assert rc != 0 and (kp == 7).all() and (jo == 7).all()


def test_wrapper_refuses_a_missing_jacobian_and_a_recording_context():
    kd, k0, ks = cases.keypoints("rel/w/kd", 2), cases.keypoints("rel/w/k0", 2), cases.keypoints("rel/w/ks", 2)
    with emulated_hip(counting=True) as lib:
        for i in range(3):
            kps = [dict(ks), dict(kd), dict(k0)]
            del kps[i]["jacobian"]
            with pytest.raises(ValueError, match="has no 'jacobian'"):
                relative_kp(*kps)
        only_kp = [{"kp": t["kp"]} for t in (ks, kd, k0)]
        r = relative_kp(*only_kp, use_relative_jacobian=False)
        assert set(r) == {"kp"} and torch.equal(r["kp"], (kd["kp"] - k0["kp"]) * 1 + ks["kp"])
        extra = dict(kd, heatmap="h")
        assert relative_kp(ks, extra, k0)["heatmap"] == "h"
        n = len(lib.calls)
        leaf = dict(kd, kp=kd["kp"].clone().requires_grad_(True))
        with torch.enable_grad():
            with pytest.raises(RuntimeError, match="no backward"):
                relative_kp(ks, leaf, k0)
        assert len(lib.calls) == n                                                    # refused before anything was launched


def test_relative_animator_needs_an_initial_frame():
    from tests.test_bf16_cache import _dry_model
    from tests.test_clip_cpu import _clips
    with emulated_hip():
        m = _dry_model()
        src, clip = _clips(2)
        an = Animator(m, relative=True)
        an.set_source(src)
        with pytest.raises(RuntimeError, match="initial driving frame"):
            an(clip[:, :, 0].contiguous())
        with pytest.raises(ValueError, match="one initial driving frame per source"):
            an.set_driving_initial(clip[:1, :, 0].contiguous())
        an.set_driving_initial(clip[:, :, 0].contiguous())
        assert an(clip[:, :, 1].contiguous()).shape == src.shape
        with pytest.raises(ValueError, match="relative=False"):
            Animator(m).set_driving_initial(clip[:, :, 0].contiguous())
        an.set_source(src)                                                            # a new source: the initial frame goes with the old one
        with pytest.raises(RuntimeError, match="initial driving frame"):
            an(clip[:, :, 1].contiguous())


def test_make_animation_is_one_animator_loop_that_reaches_the_entry():
    """the default make_animation (relative, eager) calls the entry once per group of frames; initial_frame names the reference frame"""
    from mrfa_amd.infer import make_animation
    from tests.test_bf16_cache import _dry_model
    from tests.test_clip_cpu import _clips, _gate
    with emulated_hip(counting=True) as lib:
        m = _dry_model()
        src, clip = _clips(3)
        del lib.calls[:]
        a = make_animation(m, src, clip, frames_per_call=2)                           # groups of 2 and 1
        reps = [args[9] for n, args in lib.calls if n == "mrfa_kp_relative_fwd"]
        assert reps == [2, 1] and a.shape == clip.shape
        del lib.calls[:]
        make_animation(m, src, clip, relative=False)
        assert "mrfa_kp_relative_fwd" not in [n for n, _ in lib.calls]
        b = make_animation(m, src, clip, adapt_movement_scale=True, initial_frame=1)
        absolute = Animator(m)
        absolute.set_source(src)
        _gate(b[:, :, 1], absolute(src), "initial_frame=1: frame 1 vs the self-reconstruction")
        assert (b[:, :, 0] - b[:, :, 1]).abs().max().item() > 1e-3
        for bad in (3, -1, 1.0):
            with pytest.raises(ValueError, match="initial_frame"):
                make_animation(m, src, clip, initial_frame=bad)


def test_a_misaligned_jacobian_view_is_copied_not_refused():
    """an operand at an offset the kernel's float4 loads cannot take is copied first: one launch, the aligned operand's result bit for bit"""
    kd, k0, ks = cases.keypoints("rel/old/kd", 6), cases.keypoints("rel/old/k0", 2), cases.keypoints("rel/old/ks", 2)
    with emulated_hip(counting=True) as lib:
        flat = torch.zeros(6 * 10 * 4 + 1)
        odd = dict(kd, jacobian=flat[1:].view(6, 10, 2, 2).copy_(kd["jacobian"]))     # 4 bytes past a 16-byte boundary
        assert odd["jacobian"].data_ptr() % 16 == 4
        r = relative_kp(ks, odd, k0, rep=3)
        assert [n for n, _ in lib.calls].count("mrfa_kp_relative_fwd") == 1 and torch.isfinite(r["jacobian"]).all()
        assert torch.equal(r["jacobian"], relative_kp(ks, kd, k0, rep=3)["jacobian"])


def _launches(lib):
    """entry points reached since the list was cleared, without the host-side mode query every program asks first"""
    return [n for n, _ in lib.calls if n != "mrfa_get_mfma_mode"]


def test_which_animator_reaches_the_entry_and_how_often():
    from tests.test_bf16_cache import _dry_model
    from tests.test_clip_cpu import BS, _clips, _gate
    with emulated_hip(counting=True) as lib:
        m = _dry_model()
        src, clip = _clips(3)
        group = lambda T: clip[:, :, :T].permute(0, 2, 1, 3, 4).reshape(BS * T, *clip.shape[1:2], *clip.shape[3:]).contiguous()
        absolute = Animator(m, adapt_movement_scale=True, use_relative_jacobian=True)        # relative=False: both are ignored, as in normalize_kp
        absolute.set_source(src)
        rel = Animator(m, relative=True, adapt_movement_scale=True)
        rel.set_source(src, clip[:, :, 0].contiguous())
        K = rel.kp_s["kp"].shape[1]
        for T in (1, 3):
            absolute(group(T)), rel(group(T))                                                 # weight packs and tables of this shape: once, not per call
            del lib.calls[:]
            a = absolute(group(T))
            n_abs = _launches(lib)
            assert "mrfa_kp_relative_fwd" not in n_abs
            del lib.calls[:]
            out = rel(group(T))
            calls = [args for n, args in lib.calls if n == "mrfa_kp_relative_fwd"]
            assert len(calls) == 1, T                                                         # once per call, whatever T is
            assert calls[0][8:11] == (BS * T, T, K) and calls[0][7] == rel._scale.data_ptr()  # (B, rep, K): kp_0 / kp_s at the source batch, rep = T
            assert out.shape == a.shape and (out - a).abs().max().item() > 1e-3
            print(f"[relative] C-ABI calls of one Animator call, Bs={BS} T={T}: relative {len(_launches(lib))}, absolute {len(n_abs)}")
            assert len(_launches(lib)) == len(n_abs) + 1                                      # the absolute program plus one launch
        # driving == initial: the relative keypoints are the source's, whatever the scale -> the absolute Animator driven by the source itself
        _gate(rel(group(1)), absolute(src), "relative frame 0 vs the absolute self-reconstruction")


def test_relative_animator_clip_against_the_references_animation(golden_dir):
    """Animator(relative=True, adapt_movement_scale=True), FOMM prior, source and dropin/drv* frames of tests/test_callers.py's
    _check_against_reference_callers, the three frames in ONE call (T = 3), against the reference's recorded demo.make_animation at that test's tolerance"""
    from tests.test_callers import _dropin_model
    g = np.load(os.path.join(golden_dir, "dropin_fomm.npz"))
    with emulated_hip(counting=True) as lib:
        m = _dropin_model("fomm", "cpu")
        src = cases.images("dropin/src", 1, 256)
        drv = [cases.images(f"dropin/drv{t}", 1, 256) for t in range(3)]
        an = Animator(m, relative=True, adapt_movement_scale=True)
        an.set_source(src, drv[0])
        del lib.calls[:]
        out = an(torch.cat(drv, dim=0))
        assert [n for n, _ in lib.calls].count("mrfa_kp_relative_fwd") == 1
    d = np.abs(out.permute(0, 2, 3, 1)[:, ::2, ::2, :].numpy() - g["animation"])
    print(f"[relative] T=3 clip vs the reference's animation: max |diff| {d.max():.3e} mean {d.mean():.3e}")
    assert d.mean() <= 1e-4 and d.max() <= 5e-3, (d.max(), d.mean())
