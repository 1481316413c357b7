"""The equivariance constraint of the reference's objective (modules/model.py:231-247) on the library's three entries (include/mrfa_equiv_hip.h):

  transform_frame(transform, frame)                    the driving frame warped by T, the sampling position computed inside the one launch
  equivariance_terms(transform, kp_driving, transformed_kp, w_value, w_jacobian)
                                                       {'equivariance': w_e mean|kp_d - T(kp_t)|, 'equivariance_jacobian': w_j |I - inv(jac_d) JT(kp_t) jac_t|}

Both take a mrfa_amd.losses.Transform as it is (theta, control_points, control_params, tps), so one draw feeds this path or the torch path of
mrfa_amd.losses.  The terms are one autograd.Function around one forward and one backward launch: the thin-plate spline's first and second derivatives are
closed-form, so the graph is first-order (no create_graph), deterministic, and its backward recomputes from the inputs."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import equiv_hip


def _describe(t) -> str:
    return f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__


def _f32(what: str, name: str, t, device=None) -> torch.Tensor:
    if not (torch.is_tensor(t) and t.dtype == torch.float32):
        raise TypeError(f"{what}: {name} must be a float32 tensor, not {_describe(t)}")
    if device is not None and t.device != device:
        raise ValueError(f"{what}: {name} is on {t.device}, but the first tensor is on {device}: all tensors live on one device")
    return t


def _transform_tensors(what: str, transform, B: int, device):
    """(theta (B,2,3), points (P,2) or None, params (B,P) or None, P) of a Transform, contiguous"""
    theta = _f32(what, "transform.theta", getattr(transform, "theta", None), device)
    if tuple(theta.shape) != (B, 2, 3):
        raise ValueError(f"{what}: transform.theta must be ({B}, 2, 3) for a batch of {B}, not {tuple(theta.shape)}")
    if not getattr(transform, "tps", False):
        return theta.contiguous(), None, None, 0
    points = _f32(what, "transform.control_points", transform.control_points, device)
    params = _f32(what, "transform.control_params", transform.control_params, device)
    if points.dim() < 2 or points.shape[-1] != 2 or points.numel() == 0 or points.numel() != 2 * math.prod(points.shape[1:-1]):
        raise ValueError(f"{what}: transform.control_points must be (1, P, 2) -- or the reference's (1, p, p, 2) --, not {tuple(points.shape)}")
    P = points.numel() // 2
    if tuple(params.shape) != (B, 1, P):
        raise ValueError(f"{what}: transform.control_params must be ({B}, 1, {P}) for {P} control points, not {tuple(params.shape)}")
    if P > equiv_hip.MAX_POINTS:
        raise ValueError(f"{what}: {P} control points, the library takes at most {equiv_hip.MAX_POINTS} (MRFA_EQUIV_MAX_POINTS)")
    return theta.contiguous(), points.reshape(P, 2).contiguous(), params.reshape(B, P).contiguous(), P


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def transform_frame(transform, frame: torch.Tensor) -> torch.Tensor:
    """Transform.transform_frame(frame) (model.py:44-48) as one launch: (B,C,H,W) fp32 -> (B,C,H,W) fp32, no gradient (the frame is data, the draw a constant)"""
    what = "transform_frame"
    _f32(what, "frame", frame)
    if frame.dim() != 4:
        raise ValueError(f"{what}: frame must be (B, C, H, W), not {tuple(frame.shape)}")
    B, Cc, H, W = frame.shape
    if H < 2 or W < 2:
        raise ValueError(f"{what}: frame must be at least 2 x 2 (the sampling grid divides by size - 1), not {H} x {W}")
    theta, points, params, P = _transform_tensors(what, transform, B, frame.device)
    src = frame.detach().contiguous()
    out = torch.empty_like(src)
    equiv_hip.check(equiv_hip.lib().mrfa_equiv_warp_frame(equiv_hip.stream_ptr(), src.data_ptr(), B, Cc, H, W, theta.data_ptr(), _ptr(points), _ptr(params), P,
                                                          out.data_ptr()), "mrfa_equiv_warp_frame")
    return out


class _Terms(torch.autograd.Function):
    """(value, term) = mrfa_equiv_loss_fwd(...); backward = mrfa_equiv_loss_bwd(...) on the same inputs (nothing else is saved)"""

    @staticmethod
    def forward(ctx, kp_d, jac_d, kp_t, jac_t, theta, points, params, P, w_e, w_j):
        B, K = kp_d.shape[:2]
        kp_d, kp_t = kp_d.detach().contiguous(), kp_t.detach().contiguous()
        if jac_d is not None:
            jac_d, jac_t = jac_d.detach().contiguous(), jac_t.detach().contiguous()
        value = torch.empty((), dtype=torch.float32, device=kp_d.device)
        term = torch.empty((B, K, 2, 2), dtype=torch.float32, device=kp_d.device) if jac_d is not None else None
        equiv_hip.check(equiv_hip.lib().mrfa_equiv_loss_fwd(equiv_hip.stream_ptr(), B, K, kp_d.data_ptr(), _ptr(jac_d), kp_t.data_ptr(), _ptr(jac_t),
                                                            theta.data_ptr(), _ptr(points), _ptr(params), P, w_e, w_j, value.data_ptr(), _ptr(term)),
                        "mrfa_equiv_loss_fwd")
        ctx.save_for_backward(kp_d, jac_d, kp_t, jac_t, theta, points, params)
        ctx.consts = (B, K, P, w_e, w_j)
        if term is None:
            term = value.new_empty(0)                                   # (no Jacobian term: a placeholder that nothing differentiates)
            ctx.mark_non_differentiable(term)
        return value, term

    @staticmethod
    def backward(ctx, g_value, g_term):
        kp_d, jac_d, kp_t, jac_t, theta, points, params = ctx.saved_tensors
        B, K, P, w_e, w_j = ctx.consts
        g_value = torch.zeros_like(kp_d[0, 0, 0]) if g_value is None else g_value.detach().to(torch.float32).contiguous()
        d_kp_d, d_kp_t = torch.empty_like(kp_d), torch.empty_like(kp_t)
        d_jac_d = d_jac_t = None
        if jac_d is not None:
            g_term = torch.zeros_like(jac_d) if g_term is None else g_term.detach().to(torch.float32).contiguous()
            d_jac_d, d_jac_t = torch.empty_like(jac_d), torch.empty_like(jac_t)
        else:
            g_term = None
        equiv_hip.check(equiv_hip.lib().mrfa_equiv_loss_bwd(equiv_hip.stream_ptr(), B, K, kp_d.data_ptr(), _ptr(jac_d), kp_t.data_ptr(), _ptr(jac_t),
                                                            theta.data_ptr(), _ptr(points), _ptr(params), P, w_e, w_j, g_value.data_ptr(), _ptr(g_term),
                                                            d_kp_d.data_ptr(), _ptr(d_jac_d), d_kp_t.data_ptr(), _ptr(d_jac_t)), "mrfa_equiv_loss_bwd")
        return d_kp_d, d_jac_d, d_kp_t, d_jac_t, None, None, None, None, None, None


def equivariance_terms(transform, kp_driving: Dict[str, torch.Tensor], transformed_kp: Dict[str, torch.Tensor], w_value: float,
                       w_jacobian: float) -> Dict[str, torch.Tensor]:
    """{'equivariance': scalar} and, when w_jacobian != 0, {'equivariance_jacobian': (B,K,2,2)}: the two entries GeneratorFullLoss computes from
    kp_driving = encoder(driving) and transformed_kp = encoder(transform_frame(driving)), the weights included; gradients reach the 'kp' and 'jacobian'
    tensors of both dictionaries that require them."""
    what = "equivariance_terms"
    w_value, w_jacobian = float(w_value), float(w_jacobian)
    kp_d = _f32(what, "kp_driving['kp']", kp_driving.get("kp"))
    dev = kp_d.device
    kp_t = _f32(what, "transformed_kp['kp']", transformed_kp.get("kp"), dev)
    if kp_d.dim() != 3 or kp_d.shape[-1] != 2:
        raise ValueError(f"{what}: kp_driving['kp'] must be (B, K, 2), not {tuple(kp_d.shape)}")
    B, K = kp_d.shape[:2]
    if B < 1 or K < 1:
        raise ValueError(f"{what}: kp_driving['kp'] must hold at least one keypoint, not {tuple(kp_d.shape)}")
    if tuple(kp_t.shape) != (B, K, 2):
        raise ValueError(f"{what}: transformed_kp['kp'] must be ({B}, {K}, 2) like kp_driving['kp'], not {tuple(kp_t.shape)}")
    jac_d = jac_t = None
    if w_jacobian != 0:
        for name, d in (("kp_driving", kp_driving), ("transformed_kp", transformed_kp)):
            if d.get("jacobian") is None:
                raise ValueError(f"{what}: w_jacobian is {w_jacobian:g} but {name} has no 'jacobian' (a prior without Jacobians sets equivariance_jacobian: 0)")
        jac_d = _f32(what, "kp_driving['jacobian']", kp_driving["jacobian"], dev)
        jac_t = _f32(what, "transformed_kp['jacobian']", transformed_kp["jacobian"], dev)
        for name, j in (("kp_driving['jacobian']", jac_d), ("transformed_kp['jacobian']", jac_t)):
            if tuple(j.shape) != (B, K, 2, 2):
                raise ValueError(f"{what}: {name} must be ({B}, {K}, 2, 2) beside keypoints ({B}, {K}, 2), not {tuple(j.shape)}")
    theta, points, params, P = _transform_tensors(what, transform, B, dev)
    value, term = _Terms.apply(kp_d, jac_d, kp_t, jac_t, theta, points, params, P, w_value, w_jacobian)
    out = {"equivariance": value}
    if w_jacobian != 0:
        out["equivariance_jacobian"] = term
    return out
