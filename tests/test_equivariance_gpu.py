"""mrfa_amd.equivariance on the MI355X at module level: parity with the reference's own run (tests/golden/losses.npz) at the tolerances tests/test_losses.py
applies to the torch path, hipGraph capture of the three launches, and the reference objective of a HotPath on either path."""
import json
import os

import numpy as np
import pytest
import torch

from mrfa_amd.equivariance import equivariance_terms, transform_frame
from mrfa_amd.losses import GeneratorFullLoss, Transform
from tests import cases
from tests.test_losses import TRAIN_PARAMS, _g, _transform, _vgg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------------------------------- (a) golden parity
def test_golden_frame_warp(golden_dir):
    g = _g(golden_dir)
    real = cases.images("g7/real", 1, 256).to(DEV)
    t = _transform(g, DEV)
    got = transform_frame(t, real)
    assert np.abs(got[:, :, ::4, ::4].cpu().numpy() - g["warp_frame_s4"]).max() <= 1e-4                  # tests/test_losses.py:86
    # and the torch path's own result on the same draw: two fp32 evaluations of one position, a few 1e-6 of a pixel value apart
    assert (got - t.transform_frame(real)).abs().max().item() <= 1e-4


def test_golden_full_training_forward(golden_dir):
    """tests/test_losses.py:_check_full with GeneratorFullLoss(equivariance="library"): the values of lines 107-109 and the gradient-norm gate of 110-123"""
    from mrfa_amd.train import VOX1, HotPath
    g = _g(golden_dir)
    model = HotPath(VOX1, prior="fomm")
    for pfx, mod in (("encoder.", model.encoder), ("dense_motion.", model.dense_motion), ("decoder.", model.decoder)):
        mod.load_state_dict(cases.weights_for(mod.state_dict(), pfx))
    model.to(DEV).train(True)
    src, drv = cases.images("g7/src", 1, 256).to(DEV), cases.images("g7/drv", 1, 256).to(DEV)
    full = GeneratorFullLoss(TRAIN_PARAMS, _vgg(DEV), equivariance="library").to(DEV)
    kp_s, kp_d = model.encoder(src), model.encoder(drv)
    dm = model.dense_motion(src, kp_d, kp_s)
    gen, _, _ = model.decoder(kp_s["kp"], kp_d["kp"], dm, img=model.down(src), img_full=src)
    lv = full(model.encoder, drv, gen, kp_d, transform=_transform(g, DEV))
    assert abs(lv["perceptual"].item() - g["perceptual"][0]) <= 1e-3 * g["perceptual"][0]
    assert abs(lv["equivariance"].item() - g["equivariance"][0]) <= 1e-3 * g["equivariance"][0] + 1e-4
    ej = lv["equivariance_jacobian"].detach().cpu().numpy()
    assert ej.shape == g["equivariance_jacobian"].shape
    assert np.abs(ej - g["equivariance_jacobian"]).max() <= 1e-3 * np.abs(g["equivariance_jacobian"]).max() + 1e-3
    sum(v.mean() for v in lv.values()).backward()
    names = json.load(open(os.path.join(golden_dir, "losses_param_names.json")))
    params = dict(model.named_parameters())
    ref = g["param_grad_norms"]
    big = ref.max()
    errs = []
    for n, rn in zip(names, ref):
        if n.startswith("vgg."):
            continue
        gn = float(params[n].grad.norm()) if params[n].grad is not None else 0.0
        errs.append(abs(gn - rn) / max(rn, 1e-3 * big))
    print(f"[equiv] golden gradient norms on the library path: median {np.median(errs):.2e} max {max(errs):.2e}")
    assert len(errs) > 300 and np.median(errs) <= 1e-2 and max(errs) <= 0.2, (np.median(errs), max(errs))


# ------------------------------------------------------------------------------------------------------------------------------------- (b) capture
def test_captured_warp_and_terms_replay_bit_identically():
    from mrfa_amd import graph_replay_safe
    graph_replay_safe("test_equivariance_gpu")
    B, K, S = 2, 10, 64
    gen = torch.Generator(device=DEV).manual_seed(3)
    t = Transform(B, generator=gen, device=DEV, sigma_affine=0.05, sigma_tps=0.005, points_tps=5)
    names = ("frame", "kp_d", "jac_d", "kp_t", "jac_t", "g_term")

    def draw(k):
        d = {"frame": cases.images(f"equiv/cap/{k}", B, S)}
        for side in "dt":
            kp = cases.keypoints(f"equiv/cap/{k}/{side}", B, K)
            d["kp_" + side], d["jac_" + side] = kp["kp"], kp["jacobian"]
        d["g_term"] = cases.keypoints(f"equiv/cap/{k}/g", B, K)["jacobian"]
        d["theta"] = torch.eye(2, 3).view(1, 2, 3) + 0.05 * cases.keypoints(f"equiv/cap/{k}/th", B, 3)["kp"].transpose(1, 2)
        return {n: v.to(DEV) for n, v in d.items()}

    def run(x):
        leaves = [x[n].requires_grad_(True) for n in ("kp_d", "jac_d", "kp_t", "jac_t")]
        warped = transform_frame(t, x["frame"])
        out = equivariance_terms(t, {"kp": leaves[0], "jacobian": leaves[1]}, {"kp": leaves[2], "jacobian": leaves[3]}, 10.0, 10.0)
        grads = torch.autograd.grad(0.7 * out["equivariance"] + (out["equivariance_jacobian"] * x["g_term"]).sum(), leaves)
        return [warped, out["equivariance"], out["equivariance_jacobian"], *grads]

    static = draw(0)
    t.theta.copy_(static["theta"])
    run(static)                                                        # warm: the library is loaded outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run(static)
    for k in (1, 2):
        fresh = draw(k)
        for n in names:
            static[n].detach().copy_(fresh[n])
        t.theta.copy_(fresh["theta"])
        g.replay()
        torch.cuda.synchronize()
        got = [o.detach().clone() for o in outs]
        want = run({n: v.clone() for n, v in fresh.items()})
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a.view(torch.int32), b.detach().view(torch.int32)), (k, i)
        assert got[1].item() > 0 and got[0].std().item() > 0


# ------------------------------------------------------------------------------------------------------------------------------------- (c) the objective
def test_reference_loss_agrees_between_the_two_paths():
    """train.reference_loss on a FOMM HotPath at B = 1 under the same device seed (the Transform draw), to the loss_tol of GraphedTrainStep.verify"""
    from mrfa_amd.train import VOX1, HotPath, reference_loss
    model = HotPath(VOX1, prior="fomm")
    for pfx, mod in (("encoder.", model.encoder), ("dense_motion.", model.dense_motion), ("decoder.", model.decoder)):
        mod.load_state_dict(cases.weights_for(mod.state_dict(), pfx))
    model.to(DEV).train(True)
    src, drv = cases.images("g7/src", 1, 256).to(DEV), cases.images("g7/drv", 1, 256).to(DEV)
    vgg = _vgg(DEV)
    losses = {}
    for path in ("torch", "library"):
        full = GeneratorFullLoss(TRAIN_PARAMS, vgg, equivariance=path).to(DEV)
        torch.cuda.manual_seed(1234)
        model.zero_grad(set_to_none=True)
        loss = reference_loss(model, full, src, drv)
        loss.backward()                                                # (the step as training runs it; train-mode BatchNorm normalises with batch statistics)
        losses[path] = loss.item()
        assert all(p.grad is None or torch.isfinite(p.grad).all() for p in model.parameters())
    print(f"[equiv] reference_loss torch {losses['torch']:.6f} library {losses['library']:.6f}")
    assert np.isfinite(losses["torch"]) and abs(losses["library"] - losses["torch"]) <= 1e-4 * abs(losses["torch"])
