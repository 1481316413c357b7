"""float64 reference of the token-transformer operations of include/mrfa_hip.h (K21: attention, LayerNorm, exact GELU, each with its backward), the ABI's
formulas spelled out in plain torch -- no softmax, layer_norm or gelu call.  With full=True each function returns a dict that also holds the companion
quantities the per-element bounds of tests/test_token_kernels_gpu.py are built from: the sums of the absolute contributions to each element (S_*), and for
attention, per (row, key), the score s, the absolute score sum A = scale sum_c |q_ic k_jc| and x = s - lse.

Attention tensors inside the dicts are in head layout (B, heads, n, .); rows() turns one into the ABI's (B n) x (heads d) rows."""
import math

import torch

F64 = torch.float64


def heads_of(t, B, n, heads, d):
    """(B n) x (heads d) rows -> (B, heads, n, d)"""
    return t.to(F64).view(B, n, heads, d).permute(0, 2, 1, 3)


def rows(t):
    """(B, heads, n, d) -> (B n) x (heads d) rows"""
    B, h, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * n, h * d)


def split_qkv(qkv, B, n, heads, d):
    t = qkv.to(F64).view(B, n, 3, heads, d)
    return [t[:, :, i].permute(0, 2, 1, 3) for i in range(3)]


def attend(q, k, v, scale):
    """softmax(scale q k^T) v on (B, heads, n, d) operands (k / v may have another number of rows than q)"""
    s = scale * torch.einsum("bhic,bhjc->bhij", q, k)
    A = scale * torch.einsum("bhic,bhjc->bhij", q.abs(), k.abs())
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    lse = (m + torch.log(l)).squeeze(-1)
    return dict(s=s, A=A, m=m.squeeze(-1), l=l.squeeze(-1), p=p, lse=lse, x=s - lse[..., None], o=p @ v, S_o=p @ v.abs())


def attention_ref(qkv, B, n, heads, d, scale, full=False):
    """out (B n) x (heads d) and lse [B heads n]"""
    q, k, v = split_qkv(qkv, B, n, heads, d)
    r = attend(q, k, v, scale)
    r.update(q=q, k=k, v=v, out=rows(r["o"]), lse_flat=r["lse"].reshape(-1))
    return r if full else (r["out"], r["lse_flat"])


def attention_grads_ref(qkv, dout, B, n, heads, d, scale, full=False, delta=None):
    """dq, dk, dv, each (B n) x (heads d).  delta [B, heads, n]: the backward's dO . O, given only to evaluate a deliberately wrong one"""
    r = attention_ref(qkv, B, n, heads, d, scale, full=True)
    q, k, v, p = r["q"], r["k"], r["v"], r["p"]
    do = heads_of(dout, B, n, heads, d)
    dl = (do * r["o"]).sum(-1) if delta is None else delta
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - dl[..., None])
    dq, dk, dv = scale * (ds @ k), scale * (ds.transpose(-1, -2) @ q), p.transpose(-1, -2) @ do
    if not full:
        return rows(dq), rows(dk), rows(dv)
    r.update(do=do, delta=dl, S_delta=(do * r["o"]).abs().sum(-1), dp=dp, S_dp=do.abs() @ v.abs().transpose(-1, -2), ds=ds, dq=dq, dk=dk, dv=dv,
             S_dq=scale * (ds.abs() @ k.abs()), S_dk=scale * (ds.abs().transpose(-1, -2) @ q.abs()), S_dv=p.transpose(-1, -2) @ do.abs())
    return r


def layernorm_ref(x, gamma, beta, eps, full=False):
    """y, mean, rstd of torch.nn.LayerNorm over the last dimension: biased variance, eps inside the square root"""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    C = x.shape[1]
    mean = x.sum(1) / C
    d = x - mean[:, None]
    var = (d * d).sum(1) / C
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd[:, None] * gamma + beta
    if not full:
        return y, mean, rstd
    return dict(y=y, mean=mean, rstd=rstd, d=d, var=var, xh=d * rstd[:, None], A1=x.abs().sum(1) / C, gamma=gamma, beta=beta)


def layernorm_grads_ref(x, dy, gamma, eps, full=False):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)) with g = dy gamma; dgamma = sum_r dy xhat; dbeta = sum_r dy"""
    f = layernorm_ref(x, gamma, torch.zeros_like(gamma), eps, full=True)
    dy, C = dy.to(F64), x.shape[1]
    xh, rstd = f["xh"], f["rstd"]
    g = dy * f["gamma"]
    k1 = g.sum(1) / C
    k2 = (g * xh).sum(1) / C
    t = g - k1[:, None] - xh * k2[:, None]
    dx, dgamma, dbeta = rstd[:, None] * t, (dy * xh).sum(0), dy.sum(0)
    if not full:
        return dx, dgamma, dbeta
    f.update(dy=dy, g=g, k1=k1, k2=k2, t=t, dx=dx, dgamma=dgamma, dbeta=dbeta, G1=g.abs().sum(1) / C, S_k2=(g * xh).abs().sum(1) / C,
             S_dg=(dy * xh).abs().sum(0), S_db=dy.abs().sum(0))
    return f


SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794


def gelu_ref(x, full=False):
    """y = x Phi(x) = 0.5 x (1 + erf(x / sqrt 2))"""
    x = x.to(F64)
    erf = torch.erf(x * SQRT1_2)
    y = 0.5 * x * (1.0 + erf)
    return dict(y=y, x=x, erf=erf, t=x * SQRT1_2) if full else y


def gelu_grads_ref(x, dy, full=False):
    """dx = dy (Phi(x) + x phi(x)), phi(x) = exp(-x^2 / 2) / sqrt(2 pi)"""
    f = gelu_ref(x, full=True)
    x, dy = f["x"], dy.to(F64)
    cdf = 0.5 * (1.0 + f["erf"])
    pdf = INV_SQRT_2PI * torch.exp(-0.5 * x * x)
    dx = dy * (cdf + x * pdf)
    if not full:
        return dx
    f.update(dy=dy, cdf=cdf, pdf=pdf, dx=dx)
    return f


assert abs(SQRT1_2 - math.sqrt(0.5)) < 1e-16 and abs(INV_SQRT_2PI - 1 / math.sqrt(2 * math.pi)) < 1e-16
