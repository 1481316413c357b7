"""RaftFlow.forward(corr="direct") and its callers on the GPU (-m gpu): against the reference's recorded outputs at the tolerance
tests/test_parity_gpu.py::test_raft_flow_vs_reference_goldens holds the volume path to (max |diff| <= 1e-3, mean <= 1e-4; the output means <= 1e-4),
from a source cache of either dtype (bf16: against the oracle on the same rounded pyramid, as tests/test_bf16_cache.py judges it), replayed from a
hipGraph, and the memory the mode exists to save."""
import os

import numpy as np
import pytest
import torch

from mrfa_amd.modules import RaftFlow
from oracle import mrfa_oracle as O
from tests import cases
from tests.emu import cache_pyramid_nchw, oracle_pyramid
from tests.test_oracle_golden import raft_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cmp(got, ref, max_tol=1e-3, mean_tol=1e-4, what=""):
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else got
    ref = ref.detach().float().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    d = np.abs(got - ref)
    print(f"[corr direct] {what}: max |diff| {d.max():.3e}  mean {d.mean():.3e}")
    assert d.max() <= max_tol and d.mean() <= mean_tol, f"{what}: max {d.max():.3e} mean {d.mean():.3e}"


def _raft(size, prior_only=False):
    rf = RaftFlow(**cases.raft_cfg(size, prior_only))
    sd = cases.weights_for(rf.state_dict(), "rf")
    rf.load_state_dict(sd)
    return rf.to(DEV).eval(), sd


def _to(ins):
    kp_s, kp_d, dmo, img, img_full = ins
    return kp_s.to(DEV), kp_d.to(DEV), {k: v.to(DEV) for k, v in dmo.items()}, img.to(DEV), img_full.to(DEV)


@pytest.mark.parametrize("cache", [None, torch.float32])
@pytest.mark.parametrize("prior_only", [False, True])
def test_raft_flow_direct_vs_reference_goldens(golden_dir, prior_only, cache):
    """the eval cases of tests/golden/raft_64.npz (prior_only: the argument is accepted; that program has no correlation to replace)"""
    g = dict(np.load(os.path.join(golden_dir, "raft_64.npz")))
    rf, _ = _raft(64, prior_only)
    kp_s, kp_d, dmo, img, img_full = _to(raft_inputs(64, 2, "g3/raft64"))
    with torch.no_grad():
        kw = {} if cache is None else {"source_cache": rf.encode_source(kp_s, img, img_full, feature_dtype=cache)}
        o, w, s = rf(kp_s, kp_d, dmo, img, img_full, corr="direct", **kw)
    sfx = ("prior_" if prior_only else "") + "eval"
    _cmp(o, g[f"out_{sfx}"], what=f"out {sfx} cache={cache}")
    _cmp(w, g[f"warp_{sfx}"], what=f"warp {sfx} cache={cache}")
    _cmp(s[:, :, ::2, ::2], g[f"strip_{sfx}"], what=f"strip {sfx} cache={cache}")
    _cmp(o.mean(dim=(2, 3)), g[f"out_mean_{sfx}"], 1e-4, 1e-4, what=f"out mean {sfx} cache={cache}")


def test_raft_flow_direct_from_bf16_cache_vs_oracle_on_the_same_pyramid():
    size, b = 64, 2
    rf, sd = _raft(size)
    ins = raft_inputs(size, b, "g3/raft64")
    kp_s, kp_d, dmo, img, img_full = _to(ins)
    with torch.no_grad():
        cache = rf.encode_source(kp_s, img, img_full, feature_dtype=torch.bfloat16)
        assert all(f.dtype == torch.bfloat16 for f in cache["feature"]) and cache["k_s"].dtype == cache["k_pool"].dtype == torch.float32
        o, w, _ = rf(kp_s, kp_d, dmo, img, img_full, source_cache=cache, corr="direct")
        with oracle_pyramid(cache_pyramid_nchw(cache)):
            oo, ow, _ = O.raft_flow(*ins, {k: v.clone() for k, v in sd.items()}, "", size=size)
    _cmp(o, oo, what="out, bf16 cache")
    _cmp(w, ow, what="warp, bf16 cache")


def test_direct_and_volume_agree_and_direct_is_refused_where_it_has_no_backward():
    rf, _ = _raft(64)
    ins = _to(raft_inputs(64, 2, "g3/raft64"))
    with torch.no_grad():
        ov, od = rf(*ins)[0], rf(*ins, corr="direct")[0]
    _cmp(od, ov, what="direct vs volume")
    with pytest.raises(ValueError, match="no backward"):
        rf(*ins, corr="direct")
    with pytest.raises(ValueError, match="volume.*direct"), torch.no_grad():
        rf(*ins, corr="bogus")
    rf.train()
    with pytest.raises(ValueError, match="inference"), torch.no_grad():
        rf(*ins, corr="direct")


def test_graphed_animator_direct():
    """Animator(graph=True, corr="direct") at 64^2 captures (its own three-replay gate against the eager frame applies unchanged), and later replays on
    fresh inputs agree with an eager direct Animator under the same gate"""
    from mrfa_amd.infer import Animator
    from mrfa_amd.utils.prng import det_uniform
    from tests.test_bf16_cache import _dry_model
    model = _dry_model().to(DEV)
    src = det_uniform("cd/anim/src", (2, 3, 64, 64), 0, 1).to(DEV)
    drv = [det_uniform(f"cd/anim/drv{t}", (2, 3, 64, 64), 0, 1).to(DEV) for t in range(2)]
    an, eager, vol = Animator(model, graph=True, corr="direct"), Animator(model, corr="direct"), Animator(model)
    for a in (an, eager, vol):
        a.set_source(src)
    for t in (0, 1, 0):
        out = an(drv[t]).clone()
        assert an._g is not None
        d = (out - eager(drv[t])).abs()
        print(f"[corr direct] replay vs eager, driving {t}: max |diff| {d.max().item():.3e} mean {d.mean().item():.3e}")
        assert d.mean().item() <= 2e-5 and d.max().item() <= 5e-3              # Animator's own eager-versus-replay gate
        _cmp(out, vol(drv[t]), what=f"replayed direct frame vs the volume frame (driving {t})")


def test_direct_forward_saves_the_volumes_memory():
    """256^2, B = 1: the volumes of all query levels are 5 440 x 5 120 floats = 111.4 MB; the direct forward's peak must lie at least 100 MB below the
    volume forward's (10 % left for allocator rounding)"""
    rf, _ = _raft(256)
    ins = _to(raft_inputs(256, 1, "cd/mem256"))
    peak = {}
    with torch.no_grad():
        for mode in ("volume", "direct"):
            rf(*ins, corr=mode)                                                 # weight packs, constant grids: outside the measurement
        for mode in ("direct", "volume", "direct"):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = rf(*ins, corr=mode)
            torch.cuda.synchronize()
            peak.setdefault(mode, []).append(torch.cuda.max_memory_allocated())
            del out
    saved = peak["volume"][0] - max(peak["direct"])
    print(f"[corr direct] peak allocated at 256^2 B=1: volume {peak['volume'][0] / 1e6:.1f} MB, direct {[p / 1e6 for p in peak['direct']]} MB, "
          f"saved {saved / 1e6:.1f} MB (allocated before the last forward {base / 1e6:.1f} MB)")
    assert saved >= 100e6
