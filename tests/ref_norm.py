"""float64 reference of the BatchNorm operations of include/mrfa_hip.h (K5 / K6 / K7: statistics, finalize, the fused forward apply, the two-phase backward), the
ABI's formulas spelled out in plain torch -- no batch_norm, relu or avg_pool2d call.  Every function returns a dict that also holds the companion quantities
the per-element bounds of tests/test_norm_kernels_gpu.py are built from (sums of absolute contributions, the intermediates each rounding acts on).

Activations are (N, H, W, C); per-channel arrays are [groups][C] (statistic groups: sample n uses row n // (N / groups)).  `wrong` names one deliberately wrong
formula; it is given only by tests/test_norm_reference.py, to show that the bounds notice it."""
import torch

F64 = torch.float64


def per_sample(t, N):
    """[G][C] -> (N, 1, 1, C): row n // (N / G) for sample n"""
    G, Cc = t.shape
    return t.to(F64).view(G, 1, Cc).expand(G, N // G, Cc).reshape(N, 1, 1, Cc)


def group_sum(t, G):
    """(N, H, W, C) -> [G][C]: the sum over each statistic group's rows"""
    return t.reshape(G, -1, t.shape[-1]).sum(1)


def stats_ref(x):
    """mrfa_bn_stats on x [rows][C]: s1 = sum x, s2 = sum x^2 per channel; A1 = sum |x|"""
    x = x.to(F64)
    return dict(s1=x.sum(0), s2=(x * x).sum(0), A1=x.abs().sum(0))


def finalize_ref(stats, count, gamma, beta, rmean, rvar, momentum, eps, train=True, wrong=""):
    """mrfa_bn_finalize / mrfa_bn_finalize_groups.  stats: [G][2C] float64, already summed over the slots (train); rmean / rvar [C] or None.  The outputs are
    [G][C]; `rm` / `rv` hold the running statistics after every group's momentum update, in group order ([G][C]; the last row is what is stored)."""
    gamma, beta = gamma.to(F64), beta.to(F64)
    Cc = gamma.numel()
    r = dict()
    if not train:
        mean, var = rmean.to(F64).view(1, Cc), rvar.to(F64).view(1, Cc)
        invstd = 1.0 / torch.sqrt(var + eps)
        r.update(m=mean, var=var)
    else:
        G = stats.shape[0]
        t1, t2 = stats[:, :Cc], stats[:, Cc:]
        mean = t1 / count
        raw = t2 / count - mean * mean
        var = raw.clamp_min(0.0)
        invstd = 1.0 / torch.sqrt(var + eps)
        unb = var * count / (count - 1) if count > 1 and wrong != "biased running_var" else var
        r.update(m=mean, q=t2 / count, raw=raw, var=var, unb=unb)
        if rmean is not None:
            rm, rv, rms, rvs, prm, prv = rmean.to(F64), rvar.to(F64), [], [], [], []
            order = range(G - 1, -1, -1) if wrong == "reverse group order" else range(G)
            for g in order:
                prm.append(rm)
                prv.append(rv)
                rm = (1.0 - momentum) * rm + momentum * mean[g]
                rv = (1.0 - momentum) * rv + momentum * unb[g]
                rms.append(rm)
                rvs.append(rv)
            r.update(rm=torch.stack(rms), rv=torch.stack(rvs), rm_prev=torch.stack(prm), rv_prev=torch.stack(prv))
    scale = gamma * invstd
    r.update(mean=mean, invstd=invstd, scale=scale, ms=mean * scale, shift=beta - mean * scale)
    return r


def pool_sum(t):
    """(N, H, W, C) -> (N, H / 2, W / 2, C): the sum over each 2 x 2 window"""
    N, H, W, Cc = t.shape
    return t.view(N, H // 2, 2, W // 2, 2, Cc).sum((2, 4))


def unpool(t):
    """(N, H / 2, W / 2, C) -> (N, H, W, C): every output pixel's value at its four input pixels"""
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def fwd_ref(x, scale, shift, relu, pool=False, res=None, blend_a=None, occ=None):
    """mrfa_bn_act_fwd: u = x scale + shift (+ res); a = relu(u); v = avgpool2x2(a); y = A occ + v (1 - occ).  x (N, H, W, C), occ (N, H, W, 1)"""
    x = x.to(F64)
    N = x.shape[0]
    sc, sh = per_sample(scale, N), per_sample(shift, N)
    xs = x * sc
    v0 = xs + sh
    u = v0 + res.to(F64) if res is not None else v0
    a = u.clamp_min(0.0) if relu else u
    r = dict(x=x, sc=sc, sh=sh, xs=xs, v0=v0, u=u, a=a)
    v = a
    if pool:
        v = 0.25 * pool_sum(a)
        r["S_pool"] = pool_sum(a.abs())
    y = v
    if blend_a is not None:
        A, o = blend_a.to(F64), occ.to(F64)
        y = A * o + v * (1.0 - o)
        r.update(A=A, o=o)
    r.update(v=v, y=y)
    return r


def bwd1_ref(f, dy, mean, invstd, relu, pool=False, G=1, wrong=""):
    """phase 1 of mrfa_bn_act_bwd on the forward's intermediates f = fwd_ref(..): du, the residual's and the blend's gradients and the per-group sums
    s1 = sum du, s2 = sum du xhat ([G][C]) with S1 = sum |du|, S2 = sum |du xhat|.  mean / invstd None (eval mode without them): xhat = 0"""
    x, u, a = f["x"], f["u"], f["a"]
    N = x.shape[0]
    dy = dy.to(F64)
    da0 = (1.0 if wrong == "pool without 0.25" else 0.25) * unpool(dy) if pool else dy
    r = dict(da0=da0)
    da = da0
    if "A" in f:
        A, o = f["A"], f["o"]
        r["dA"] = da0 * o
        r["docc_terms"] = da0 * (A if wrong == "docc without -a" else A - a)
        r["docc"] = r["docc_terms"].sum(-1, keepdim=True)
        da = da0 * (1.0 - o)
    if relu:
        live = (u >= 0) if wrong == "relu'(0) = 1" else (u > 0)
        du = torch.where(live, da, torch.zeros_like(da))
    else:
        du = da
    if mean is not None:
        d = x - per_sample(mean, N)
        xhat = d * per_sample(invstd, N)
    else:
        d, xhat = x, torch.zeros_like(x)
    r.update(da=da, du=du, d=d, xhat=xhat, s1=group_sum(du, G), s2=group_sum(du * xhat, G), S1=group_sum(du.abs(), G), S2=group_sum((du * xhat).abs(), G))
    return r


def bwd2_ref(f, b1, red, gamma, invstd, train, G=1, red_world=1, wrong=""):
    """phase 2 on the sums red [G][2C] (what phase 1 left, summed over the slots; over the ranks too with red_world > 1):
    dx = gamma invstd (du - k1 - xhat k2) with k = red / (rows per group x red_world) (train) or du scale (eval); dgamma / dbeta = the groups' sums added up"""
    x, du, xhat = f["x"], b1["du"], b1["xhat"]
    N, Cc = x.shape[0], x.shape[-1]
    r = dict(dbeta=red[:, :Cc].sum(0), dgamma=red[:, Cc:].sum(0), T1=red[:, :Cc].abs().sum(0), T2=red[:, Cc:].abs().sum(0))
    if wrong == "dgamma once per group run":                # every group's run adds the sum of ALL groups
        r.update(dbeta=G * r["dbeta"], dgamma=G * r["dgamma"])
    if not train:
        r.update(dx=du * f["sc"])
        return r
    rows = x[0].numel() // Cc * N
    cnt = float(rows if wrong == "means over all rows" else rows // G) * (1 if wrong == "red_world ignored" else max(red_world, 1))
    k1, k2 = red[:, :Cc] / cnt, red[:, Cc:] / cnt
    k1s, k2s = per_sample(k1, N), per_sample(k2, N)
    gi = per_sample((gamma.to(F64) * invstd.to(F64)), N)
    t0 = du - k1s
    t = t0 - (0.0 if wrong == "dx without xhat k2" else 1.0) * xhat * k2s
    r.update(k1=k1s, k2=k2s, gi=gi, t0=t0, t=t, dx=gi * t)
    return r
