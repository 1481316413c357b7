"""Relative-motion animation on the GPU (-m gpu): mrfa_kp_relative_fwd against float64 with bounds counted from its own roundings, the relative Animator
(eager, captured, clips, a new initial frame after a capture) against the reference's recorded demo.make_animation and against itself, and
make_animation on the Animator (graph replays really happen, initial_frame)."""
import os

import numpy as np
import pytest
import torch

from mrfa_amd import hip
from mrfa_amd.infer import Animator, make_animation
from tests import cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
CANARY = -1234.5
PAD = 64                   # canary floats on either side of an output


def _inputs(B, rep, K, seed):
    """entries in [-2, 2]; |det jac_0| >= 0.25 (a draw below it is replaced by a fixed matrix of determinant 1.75)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, generator=g) * 4 - 2
    Bs = B // rep
    kd, k0, ks, jd, j0, js = r(B, K, 2), r(Bs, K, 2), r(Bs, K, 2), r(B, K, 2, 2), r(Bs, K, 2, 2), r(Bs, K, 2, 2)
    det = j0[..., 0, 0] * j0[..., 1, 1] - j0[..., 0, 1] * j0[..., 1, 0]
    j0[det.abs() < 0.3] = torch.tensor([[1.5, -0.5], [0.5, 1.0]])
    det = j0[..., 0, 0].double() * j0[..., 1, 1].double() - j0[..., 0, 1].double() * j0[..., 1, 0].double()
    assert det.abs().min() >= 0.25 and max(t.abs().max() for t in (kd, k0, ks, jd, j0, js)) <= 2
    return kd, k0, ks, jd, j0, js


def _guarded(shape):
    """an output inside canary floats: (whole buffer, the output's view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), CANARY, device=DEV)
    return buf, buf[PAD:PAD + n].view(*shape)


def _launch(dev_in, scale, B, rep, K, jac):
    kd, k0, ks, jd, j0, js = dev_in
    kbuf, kp_out = _guarded((B, K, 2))
    jbuf, jac_out = _guarded((B, K, 2, 2))
    p = lambda t, on=True: t.data_ptr() if on and t is not None else None
    hip.check(hip.lib().mrfa_kp_relative_fwd(hip.stream_ptr(), p(kd), p(jd, jac), p(k0), p(j0, jac), p(ks), p(js, jac), p(scale), B, rep, K, p(kp_out),
                                             p(jac_out, jac)), "mrfa_kp_relative_fwd")
    torch.cuda.synchronize()
    for buf, n, written in ((kbuf, B * K * 2, True), (jbuf, B * K * 4, jac)):
        assert (buf[:PAD] == CANARY).all() and (buf[PAD + n:] == CANARY).all(), "wrote outside its output"
        assert bool((buf[PAD:PAD + n] == CANARY).any()) != written
    return kp_out.cpu(), jac_out.cpu()


@pytest.mark.parametrize("K", [1, 10, 15])
@pytest.mark.parametrize("B,rep", [(1, 1), (6, 1), (6, 3), (5, 5)])
def test_kp_relative_kernel_against_float64(B, rep, K):
    """With and without Jacobians, scale null and a device scalar (0.37).  u = 2^-24; every input is an exact fp32 number, the expected value is float64 on
    the same numbers (its own error, ~1e-16 relative, is far below one fp32 rounding of any term).

    Keypoints: fl(fl(fl(kd - k0) s) + ks) is three roundings -- u |kd - k0| |s| from the difference, u |(kd - k0) s| from the product, u |result| <=
    u (|(kd - k0) s| + |ks|) from the sum: at most 3 u |(kd - k0) s| + u |ks| <= 3 u (|(kd - k0) s| + |ks|).

    Jacobians, in the kernel's order out = ((J_d adj J_0) J_s) / det, det = a d - b c of J_0 = [a b; c d], M = |J_d| |adj J_0| |J_s| (entrywise absolute
    values, matrix products): an entry of the first product is two multiplications and one addition, each rounding at most u times the absolute-value
    product -> 3 u; its error passes through the second product unamplified beyond M, and the second product adds its own 3 u M -> 6 u M; the division
    rounds once -> 7 u M / |det|.  The determinant is two products and one subtraction: each rounding is at most u (|ad| + |bc|) (the subtraction's because
    |det| <= |ad| + |bc|) -> |det' - det| <= 3 u (|ad| + |bc|), which reaches the quotient as the relative error 3 u (|ad| + |bc|) / |det|.  One more u on
    either count absorbs every second-order term ((1 + e)^-1 and products of roundings: with entries <= 2 and |det| >= 0.25, (|ad| + |bc|) / |det| <= 32 and
    u 33^2 << 1):   |out - ref| <= u (8 + 4 (|ad| + |bc|) / |det|) M / |det|.
    A contraction of a multiplication and an addition into one fused operation removes a rounding and never adds one.  Nothing here is measured.
    Also: two runs are bit-identical, nothing outside the outputs is written, the inputs are not written, and the CPU specification (oracle/capi_emulator.py)
    lies within the same bounds of the kernel."""
    from oracle.capi_emulator import Emulator
    ins = _inputs(B, rep, K, seed=1000 * B + 10 * rep + K)
    dev_in = [t.to(DEV) for t in ins]
    kd, k0, ks, jd, j0, js = (t.double() for t in ins)
    ri = lambda t: t.repeat_interleave(rep, dim=0)
    for s_val in (None, 0.37):
        scale = torch.tensor([s_val], dtype=torch.float32) if s_val is not None else None
        s64 = float(scale[0]) if scale is not None else 1.0               # the fp32 number the kernel reads
        move = (kd - ri(k0)) * s64
        kp_ref, kp_bound = move + ri(ks), 3 * U * (move.abs() + ri(ks).abs())
        a, b, c, d = (ri(j0)[..., i, j] for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)))
        det = (a * d - b * c)[..., None, None]
        adj = torch.stack([torch.stack([d, -b], dim=-1), torch.stack([-c, a], dim=-1)], dim=-2)
        jac_ref = jd @ adj @ ri(js) / det
        kappa = ((a * d).abs() + (b * c).abs())[..., None, None] / det.abs()
        jac_bound = U * (8 + 4 * kappa) * (jd.abs() @ adj.abs() @ ri(js).abs()) / det.abs()
        for jac in (True, False):
            kp, jo = _launch(dev_in, scale.to(DEV) if scale is not None else None, B, rep, K, jac)
            kp2, jo2 = _launch(dev_in, scale.to(DEV) if scale is not None else None, B, rep, K, jac)
            assert torch.equal(kp, kp2) and torch.equal(jo, jo2), "two runs differ"
            ek = ((kp.double() - kp_ref).abs() / kp_bound).max().item()
            print(f"[relative] B={B} rep={rep} K={K} scale={s_val} jac={jac}: kp max err / bound {ek:.3f}", end="")
            assert ek <= 1.0
            # the specification on the same numbers
            e_kp, e_jac = torch.full((B, K, 2), CANARY), torch.full((B, K, 2, 2), CANARY)
            q = lambda t, on=True: t.data_ptr() if on and t is not None else None
            assert Emulator().mrfa_kp_relative_fwd(0, q(ins[0]), q(ins[3], jac), q(ins[1]), q(ins[4], jac), q(ins[2]), q(ins[5], jac), q(scale), B, rep,
                                                           K, q(e_kp), q(e_jac, jac)) == 0
            assert ((kp.double() - e_kp.double()).abs() <= kp_bound).all()
            if jac:
                ej = ((jo.double() - jac_ref).abs() / jac_bound).max().item()
                em = ((jo.double() - e_jac.double()).abs() / jac_bound).max().item()
                print(f", jacobian max err / bound {ej:.3f}, kernel vs emulator / bound {em:.3f}", end="")
                assert ej <= 1.0 and em <= 1.0
            print()
    assert all(torch.equal(t.cpu(), o) for t, o in zip(dev_in, ins)), "inputs must not be written"


def test_kp_relative_kernel_refuses_bad_arguments_and_leaves_the_outputs_untouched():
    B, rep, K = 6, 3, 10
    dev_in = [t.to(DEV) for t in _inputs(B, rep, K, seed=7)]
    kd, k0, ks, jd, j0, js = dev_in
    kbuf, kp_out = _guarded((B, K, 2))
    jbuf, jac_out = _guarded((B, K, 2, 2))
    p = lambda t: t.data_ptr()
    good = dict(kp_d=p(kd), jac_d=p(jd), kp_0=p(k0), jac_0=p(j0), kp_s=p(ks), jac_s=p(js), scale=None, B=B, rep=rep, K=K, kp_out=p(kp_out), jac_out=p(jac_out))
    L = hip.lib()
    for bad in (dict(jac_d=None), dict(jac_0=None), dict(jac_s=None), dict(jac_out=None), dict(jac_d=None, jac_0=None, jac_s=None), dict(kp_d=None),
                dict(kp_0=None), dict(kp_s=None), dict(kp_out=None), dict(B=0), dict(B=-3), dict(K=0), dict(rep=0), dict(rep=-1), dict(rep=4), dict(B=5),
                dict(kp_0=p(k0) + 4), dict(jac_s=p(js) + 8)):
        rc = L.mrfa_kp_relative_fwd(hip.stream_ptr(), *{**good, **bad}.values())
        msg = L.mrfa_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and "kp_relative_fwd" in msg and len(msg) > 25, (bad, rc, msg)
        assert (kbuf == CANARY).all() and (jbuf == CANARY).all(), bad               # nothing was launched
    hip.check(L.mrfa_kp_relative_fwd(hip.stream_ptr(), *good.values()), "mrfa_kp_relative_fwd")
    torch.cuda.synchronize()
    assert torch.isfinite(kp_out).all() and torch.isfinite(jac_out).all() and not (kp_out == CANARY).any()


# ------------------------------------------------------------------------------------------------------------- the Animator
_SCENE = {}


def _scene(prior):
    """model, source and the three dropin/drv* frames of tests/test_callers.py's _check_against_reference_callers, once per prior"""
    if prior not in _SCENE:
        from tests.test_callers import _dropin_model
        m = _dropin_model(prior, DEV)
        src = cases.images("dropin/src", 1, 256).to(DEV)
        drv = [cases.images(f"dropin/drv{t}", 1, 256).to(DEV) for t in range(3)]
        _SCENE[prior] = (m, src, drv)
    return _SCENE[prior]


_EAGER = {}


def _eager_frames(prior, initial=0, **kw):
    """the three frames of an eager relative, scale-adapting Animator, one frame per call (computed once per configuration, never modified)"""
    key = (prior, initial, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _EAGER:
        m, src, drv = _scene(prior)
        an = Animator(m, relative=True, adapt_movement_scale=True, **kw)
        an.set_source(src, drv[initial])
        _EAGER[key] = torch.cat([an(f).clone() for f in drv], dim=0)
    return _EAGER[key]


def _replay_gate(a, b, what):
    d = (a - b).abs()
    print(f"[relative] {what}: max |diff| {d.max().item():.3e} mean {d.mean().item():.3e}")
    assert a.shape == b.shape and torch.isfinite(a).all()
    assert d.mean().item() <= 2e-5 and d.max().item() <= 5e-3, what              # Animator.__call__'s own replay gate


@pytest.mark.parametrize("prior", ["fomm", "mtia"])
def test_relative_animator_against_the_references_animation(golden_dir, prior):
    ref = np.load(os.path.join(golden_dir, f"dropin_{prior}.npz"))["animation"]          # (T,H/2,W/2,3): relative + adapted scale
    out = _eager_frames(prior)
    d = np.abs(out.permute(0, 2, 3, 1)[:, ::2, ::2, :].cpu().numpy() - ref)
    print(f"[relative] {prior}: eager relative Animator vs the reference's animation: max |diff| {d.max():.3e} mean {d.mean():.3e}")
    assert d.mean() <= 1e-4 and d.max() <= 5e-3, (d.max(), d.mean())


@pytest.mark.parametrize("corr,cache_dtype", [("volume", torch.float32), ("direct", torch.float32), ("direct", torch.bfloat16)])
def test_captured_clip_and_a_new_initial_frame(corr, cache_dtype):
    """one captured program of T = 3 frames against the eager one-frame-per-call Animator; then a new initial frame on the same object (which drops the
    captured program: the next call captures again) against an eager Animator built fresh with that frame"""
    prior = "mtia"
    m, src, drv = _scene(prior)
    clip = torch.cat(drv, dim=0)
    an = Animator(m, graph=True, relative=True, adapt_movement_scale=True, corr=corr, cache_dtype=cache_dtype)
    an.set_source(src, drv[0])
    first = an(clip).clone()
    _replay_gate(first, _eager_frames(prior, 0, corr=corr, cache_dtype=cache_dtype), f"{corr} {cache_dtype}: captured T=3 vs eager per frame")
    assert list(an._graphs) == [3]
    an.set_driving_initial(drv[2])
    assert not an._graphs                                                                # nothing captured with the old frame is left to replay
    second = an(clip).clone()
    _replay_gate(second, _eager_frames(prior, 2, corr=corr, cache_dtype=cache_dtype), f"{corr} {cache_dtype}: new initial frame vs fresh eager")
    assert (second - first).abs().max().item() > 1e-3                                    # a stale initial frame or scale would give `first` again


# ------------------------------------------------------------------------------------------------------------- make_animation
def test_make_animation_graph_really_replays(monkeypatch):
    m, src, drv = _scene("fomm")
    clip = torch.stack(drv, dim=2)
    replays = []
    real = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(id(self)), real(self))[1])
    an = Animator(m, graph=True, relative=True)
    an.set_source(src, drv[0])
    an(drv[0])
    own = len(replays) - 1                                                               # what a capture replays to check itself
    del replays[:]
    out = make_animation(m, src, clip, relative=True, adapt_movement_scale=True, graph=True, frames_per_call=1)
    print(f"[relative] make_animation(graph=True), 3 frames at 1 per call: {len(replays)} replays, {own} of them the capture's own")
    assert len(replays) >= own + 3 and len(set(replays)) == 1
    _replay_gate(out[0].permute(1, 0, 2, 3), _eager_frames("fomm"), "make_animation(graph=True) vs the eager relative Animator")


def test_default_make_animation_reaches_the_kernel(monkeypatch):
    """make_animation(relative=True) without a graph -- its default -- goes through mrfa_kp_relative_fwd of the built library, once per group of frames"""
    from tests.emu import Counting
    m, src, drv = _scene("fomm")
    assert "mrfa_kp_relative_fwd" in hip.EXPORTED_SYMBOLS
    proxy = Counting(hip.lib())
    monkeypatch.setattr(hip, "_lib", proxy)
    out = make_animation(m, src, torch.stack(drv, dim=2), relative=True, adapt_movement_scale=True)
    calls = [args for n, args in proxy.calls if n == "mrfa_kp_relative_fwd"]
    assert len(calls) == 3 and all(a[7] is not None and a[8:11] == (1, 1, 10) for a in calls)
    _replay_gate(out[0].permute(1, 0, 2, 3), _eager_frames("fomm"), "make_animation (eager) vs the eager relative Animator")


@pytest.mark.parametrize("graph", [False, True])
def test_make_animation_initial_frame(graph):
    """tests/test_callers.py::test_reconstruction_and_animation_loops_on_synthetic_video's gate for frame 0, asked of frame 1 with initial_frame=1"""
    import bench
    from mrfa_amd.train import VOX1, HotPath
    model = HotPath(VOX1, prior="mtia")
    bench.init_weights(model)
    model.to(DEV).eval()
    clip = torch.stack([cases.images(f"clip/{t}", 2, 256) for t in range(3)], dim=2).to(DEV)
    source = clip[:, :, 0].contiguous()
    anim = make_animation(model, source, clip, relative=True, initial_frame=1, graph=graph)
    with torch.no_grad():
        self_rec = model(source, source)
    d = (anim[:, :, 1] - self_rec).abs().max().item()
    print(f"[relative] make_animation(initial_frame=1, graph={graph}): frame 1 vs model(source, source) max |diff| {d:.3e}")
    assert anim.shape == clip.shape and d <= 2e-4
    assert (anim[:, :, 0] - anim[:, :, 1]).abs().max().item() > 1e-3
    with pytest.raises(ValueError, match="initial_frame"):
        make_animation(model, source, clip, initial_frame=3)
