"""The float64 reference of the prior-motion stage (csrc/prior.hip: mrfa_kp_gaussian_*, mrfa_prior_motion_*, mrfa_softmax_combine_*, mrfa_kp_head_*), written from
include/mrfa_hip.h and the kernels in explicit formulas -- no autograd -- so that every term of a rounding bound has a name.  Each function returns its values
together with the companion quantities the bounds of tests/test_prior_kernels_gpu.py need (sums of absolute terms, per-pixel slopes).  tests/test_prior_reference.py
holds it against ATen in double.  `wrong` plants one deliberately wrong formula (the mutants of that file); "" is the reference."""
import torch
import torch.nn.functional as F

F64 = torch.float64
PAD = 4                                                    # zero frame around the source image: every tap of every cell a bound looks at exists


def grid(H, W, wrong=""):
    """g(j, n) = 2 j / (n - 1) - 1 in exact double: (gx, gy), each [H][W]"""
    nx, ny = (H, W) if wrong == "grid hw" else (W, H)
    gx = 2.0 * torch.arange(W, dtype=F64) / (nx - 1) - 1.0
    gy = 2.0 * torch.arange(H, dtype=F64) / (ny - 1) - 1.0
    return gx.view(1, W).expand(H, W), gy.view(H, 1).expand(H, W)


def gauss(kp, H, W, inv_var, wrong=""):
    """kp [B][K][2] -> dx, dy = g - kp, q = dx^2 + dy^2, a = -q inv_var / 2, G = exp(a), all [B][K][H][W]"""
    gx, gy = grid(H, W, wrong)
    kp = kp.to(F64)
    dx, dy = gx - kp[..., 0, None, None], gy - kp[..., 1, None, None]
    q = dx * dx + dy * dy
    a = -0.5 * q * inv_var
    return dict(gx=gx, gy=gy, dx=dx, dy=dy, q=q, a=a, G=torch.exp(a))


# ------------------------------------------------------------------------------------------------------------------ kp_gaussian
def kp_gaussian_fwd(kp, pos, H, W, variance, wrong=""):
    """out [B][H][W][K] = G (+ pos [K][H][W])"""
    g = gauss(kp, H, W, 1.0 / variance, wrong)
    out = g["G"] if pos is None else g["G"] + pos.to(F64).unsqueeze(0)
    return dict(out=out.permute(0, 2, 3, 1), g=g)


def kp_gaussian_bwd(kp, dout, H, W, variance, wrong=""):
    """dout [B][H][W][K] -> dkp [B][K][2] = sum_pixels dout G (g - kp) / var with S_dkp the sum of the absolute terms; dpos [K][H][W] = sum_b dout with
    S_dpos = sum_b |dout|.  w = dout G / var and the terms tx, ty per pixel ride along"""
    g = gauss(kp, H, W, 1.0 / variance, wrong)
    d = dout.to(F64).permute(0, 3, 1, 2)
    w = d * g["G"] / variance
    tx, ty = w * g["dx"], w * g["dy"]
    dkp = torch.stack([tx.sum((2, 3)), ty.sum((2, 3))], -1)
    S_dkp = torch.stack([tx.abs().sum((2, 3)), ty.abs().sum((2, 3))], -1)
    dpos = d[0] if wrong == "dpos one b" else d.sum(0)
    return dict(dkp=dkp, S_dkp=S_dkp, dpos=dpos, S_dpos=d.abs().sum(0), w=w, tx=tx, ty=ty, g=g)


# ------------------------------------------------------------------------------------------------------------------ prior_motion
def affine(jd, js, wrong=""):
    """J = js inv(jd) from the closed-form inverse ([B][K][4] row-major each).  inv = (i00, i01, i10, i11), J likewise; Jabs: the absolute terms of each entry of
    J; det, detabs = |a0 a3| + |a1 a2|, rdet = 1 / |det|"""
    a0, a1, a2, a3 = jd.to(F64).unbind(-1)
    s0, s1, s2, s3 = js.to(F64).unbind(-1)
    det = a0 * a3 - a1 * a2
    idet = 1.0 / det
    i00, i01, i10, i11 = a3 * idet, -a1 * idet, -a2 * idet, a0 * idet
    if wrong == "inv transposed":
        i01, i10 = i10, i01
    J = (s0 * i00 + s1 * i10, s0 * i01 + s1 * i11, s2 * i00 + s3 * i10, s2 * i01 + s3 * i11)
    Jabs = ((s0 * i00).abs() + (s1 * i10).abs(), (s0 * i01).abs() + (s1 * i11).abs(), (s2 * i00).abs() + (s3 * i10).abs(), (s2 * i01).abs() + (s3 * i11).abs())
    return dict(det=det, detabs=(a0 * a3).abs() + (a1 * a2).abs(), rdet=idet.abs(), inv=(i00, i01, i10, i11), J=J, Jabs=Jabs, jd=(a0, a1, a2, a3),
                js=(s0, s1, s2, s3))


def prior_fwd(kd, ks, jd, js, bg, H, W, inv_var, wrong=""):
    """motions [B][K1][H][W][2] and heat [B][K1][H][W] (heat_0 = 0) with their parts: gd / gs (gauss() of kd / ks), A (affine() or None), for the background
    h = (hx, hy, hz) and habs (the absolute terms of each) [B][H][W]"""
    B, K = kd.shape[:2]
    gd, gs = gauss(kd, H, W, inv_var, wrong), gauss(ks, H, W, inv_var, wrong)
    gx, gy = gd["gx"], gd["gy"]
    ks64 = ks.to(F64)
    A = affine(jd, js, wrong) if jd is not None else None
    one, zero = torch.ones(B, K, dtype=F64), torch.zeros(B, K, dtype=F64)
    J = A["J"] if A else (one, zero, zero, one)
    e = lambda t: t[..., None, None]
    mx = e(J[0]) * gd["dx"] + e(J[1]) * gd["dy"] + e(ks64[..., 0])
    my = e(J[2]) * gd["dx"] + e(J[3]) * gd["dy"] + e(ks64[..., 1])
    mabs = ((e(J[0]) * gd["dx"]).abs() + (e(J[1]) * gd["dy"]).abs() + e(ks64[..., 0]).abs(), (e(J[2]) * gd["dx"]).abs() + (e(J[3]) * gd["dy"]).abs() + e(ks64[..., 1]).abs())
    heat = gd["G"] + gs["G"] if wrong == "heat sign" else gd["G"] - gs["G"]
    r = dict(gd=gd, gs=gs, A=A, J=J, mabs=mabs, gx=gx, gy=gy, inv_var=inv_var)
    bx, by = gx.expand(B, H, W), gy.expand(B, H, W)
    if bg is not None:
        m = bg.to(F64).view(B, 9, 1, 1)
        h = [m[:, 3 * i] * gx + m[:, 3 * i + 1] * gy + m[:, 3 * i + 2] for i in range(3)]
        r["h"] = h
        r["habs"] = [(m[:, 3 * i] * gx).abs() + (m[:, 3 * i + 1] * gy).abs() + m[:, 3 * i + 2].abs() for i in range(3)]
        r["m"] = m
        bx, by = h[0] / h[2], h[1] / h[2]
    r["motions"] = torch.stack([torch.cat([bx.unsqueeze(1), mx], 1), torch.cat([by.unsqueeze(1), my], 1)], -1)
    r["heat"] = torch.cat([torch.zeros(B, 1, H, W, dtype=F64), heat], 1)
    return r


def _pool(d, kh, kw):
    return F.max_pool2d(d.permute(0, 3, 1, 2), (kh, kw), stride=1).permute(0, 2, 3, 1)


def warp(src, motions, wrong=""):
    """the bilinear warp (align_corners=False, zeros outside) of src [B][H][W][C] at motions [B][K1][H][W][2] (double: the caller's, e.g. what a kernel stored).
    val [B][K1][C][H][W]; tapabs = sum_taps |weight tap|; slope_h / slope_v: the largest |difference| of horizontally / vertically adjacent taps over the
    3 x 3 cells around the sampled one (taps outside the image are 0); ix, iy, fx, fy [B][K1][H][W], inside, and the four taps v00 v01 v10 v11"""
    B, H, W, C = src.shape
    K1 = motions.shape[1]
    mx, my = motions[..., 0].to(F64), motions[..., 1].to(F64)
    if wrong == "align corners":
        ix, iy = (mx + 1.0) * 0.5 * (W - 1), (my + 1.0) * 0.5 * (H - 1)
    else:
        ix, iy = ((mx + 1.0) * W - 1.0) * 0.5, ((my + 1.0) * H - 1.0) * 0.5
    inside = (ix > -1.0) & (iy > -1.0) & (ix < W) & (iy < H)
    fx0, fy0 = torch.floor(ix), torch.floor(iy)
    fx, fy = ix - fx0, iy - fy0
    x0 = fx0.clamp(-(PAD - 1), W + PAD - 3).long() + PAD
    y0 = fy0.clamp(-(PAD - 1), H + PAD - 3).long() + PAD
    Hp, Wp = H + 2 * PAD, W + 2 * PAD
    P = torch.zeros(B, Hp, Wp, C, dtype=F64)
    P[:, PAD:PAD + H, PAD:PAD + W] = src.to(F64)
    if wrong == "x1 le W":                                 # the right tap admitted at x0 + 1 == W: it reads the first pixel of the next row
        P[:, PAD:PAD + H - 1, PAD + W] = src.to(F64)[:, 1:, 0]
    if wrong == "clamp border":                            # padding_mode="border": the frame repeats the edge
        P = F.pad(src.to(F64).permute(0, 3, 1, 2), (PAD,) * 4, mode="replicate").permute(0, 2, 3, 1).contiguous()
    ph = _pool((P[:, :, 1:] - P[:, :, :-1]).abs(), 4, 3)    # [y][x]: rows y .. y+3, pairs starting at x .. x+2
    pv = _pool((P[:, 1:] - P[:, :-1]).abs(), 3, 4)

    def take(Tb, wid, Y, X):                                # Tb [.][wid][C] at (Y, X) [K1][H][W] -> [K1][C][H][W]
        return Tb.reshape(-1, C)[(Y * wid + X).reshape(-1)].view(K1, H, W, C).permute(0, 3, 1, 2)
    out = {k: [] for k in ("v00", "v01", "v10", "v11", "slope_h", "slope_v")}
    for b in range(B):
        out["v00"].append(take(P[b], Wp, y0[b], x0[b]))
        out["v01"].append(take(P[b], Wp, y0[b], x0[b] + 1))
        out["v10"].append(take(P[b], Wp, y0[b] + 1, x0[b]))
        out["v11"].append(take(P[b], Wp, y0[b] + 1, x0[b] + 1))
        out["slope_h"].append(take(ph[b], ph.shape[2], y0[b] - 1, x0[b] - 1))
        out["slope_v"].append(take(pv[b], pv.shape[2], y0[b] - 1, x0[b] - 1))
    r = {k: torch.stack(v) for k, v in out.items()}
    m = inside.unsqueeze(2).to(F64)
    for k in ("v00", "v01", "v10", "v11"):
        r[k] = r[k] * m
    ex, ey = fx.unsqueeze(2), fy.unsqueeze(2)
    w = ((1 - ex) * (1 - ey), ex * (1 - ey), (1 - ex) * ey, ex * ey)
    taps = (r["v00"], r["v01"], r["v10"], r["v11"])
    r["val"] = sum(wi * ti for wi, ti in zip(w, taps))
    r["tapabs"] = sum((wi * ti).abs() for wi, ti in zip(w, taps))
    r.update(ix=ix, iy=iy, fx=fx, fy=fy, inside=inside, W=W, H=H)
    return r


def prior_bwd(f, wp, dheat, dwarp, dmot, old=None, wrong=""):
    """f = prior_fwd(..), wp = warp(src, the stored motions); dheat [B][K1][H][W], dwarp [B][K1][C][H][W] (dinp's warp channels + dsparse), dmot
    [B][K1][H][W][2] or None.  Per pixel: gix, giy (the warp's gradient in pixels), their tap companions Tx, Ty = sum_c |g| sum_taps |weight tap| and the mixed
    differences Xc = sum_c |g| |v11 - v10 - v01 + v00|, dm = (dmx, dmy).  acc / Sacc [B][K][10]: the kernel's ten sums and their absolute companions; dbg9 /
    Sdbg9 [B][9]; then dks, dkd [B][K][2], djs, djd [B][K][4], dbg [B][9] (the increments) and, for the 2 x 2 pushes, the absolute companions Cjs, Cjd"""
    W, H = wp["W"], wp["H"]
    g = dwarp.to(F64)
    ex, ey = wp["fx"].unsqueeze(2), wp["fy"].unsqueeze(2)
    v00, v01, v10, v11 = wp["v00"], wp["v01"], wp["v10"], wp["v11"]
    ins = wp["inside"].to(F64)
    gix = (g * ((v01 - v00) * (1 - ey) + (v11 - v10) * ey)).sum(2) * ins
    giy = (g * ((v10 - v00) * (1 - ex) + (v11 - v01) * ex)).sum(2) * ins
    Tx = (g.abs() * ((v01.abs() + v00.abs()) * (1 - ey) + (v11.abs() + v10.abs()) * ey)).sum(2) * ins
    Ty = (g.abs() * ((v10.abs() + v00.abs()) * (1 - ex) + (v11.abs() + v01.abs()) * ex)).sum(2) * ins
    Xc = (g.abs() * (v11 - v10 - v01 + v00).abs()).sum(2) * ins
    sw, sh = (0.5 * H, 0.5 * W) if wrong == "warp hw" else (0.5 * W, 0.5 * H)
    d0x = dmot[..., 0].to(F64) if dmot is not None else torch.zeros_like(gix)
    d0y = dmot[..., 1].to(F64) if dmot is not None else torch.zeros_like(giy)
    dmx, dmy = d0x + gix * sw, d0y + giy * sh
    r = dict(gix=gix, giy=giy, Tx=Tx, Ty=Ty, Xc=Xc, dmx=dmx, dmy=dmy, d0x=d0x, d0y=d0y,
             jump_x=(g.abs() * 2 * wp["slope_h"]).sum(2) * sw, jump_y=(g.abs() * 2 * wp["slope_v"]).sum(2) * sh)
    gd, gs = f["gd"], f["gs"]
    inv_var = f["inv_var"]
    x, y, dh = dmx[:, 1:], dmy[:, 1:], dheat.to(F64)[:, 1:]
    wd, ws = dh * gd["G"] * inv_var, dh * gs["G"] * inv_var
    terms = [x, y, x * gd["dx"], x * gd["dy"], y * gd["dx"], y * gd["dy"], wd * gd["dx"], wd * gd["dy"], ws * gs["dx"], ws * gs["dy"]]
    acc = torch.stack([t.sum((2, 3)) for t in terms], -1)
    r.update(terms=terms, wd=wd, ws=ws, acc=acc, Sacc=torch.stack([t.abs().sum((2, 3)) for t in terms], -1))
    J = f["J"]
    h8, h9 = (0.0, 0.0) if wrong == "dks no heat" else (acc[..., 8], acc[..., 9])
    h6, h7 = (0.0, 0.0) if wrong == "dkd no heat" else (acc[..., 6], acc[..., 7])
    r["dks"] = torch.stack([acc[..., 0] - h8, acc[..., 1] - h9], -1)
    r["dkd"] = torch.stack([-(J[0] * acc[..., 0] + J[2] * acc[..., 1]) + h6, -(J[1] * acc[..., 0] + J[3] * acc[..., 1]) + h7], -1)
    if f["A"] is not None:
        A = f["A"]
        i00, i01, i10, i11 = A["inv"]
        s0, s1, s2, s3 = A["js"]
        d00, d01, d10, d11 = acc[..., 2], acc[..., 3], acc[..., 4], acc[..., 5]
        r["djs"] = torch.stack([d00 * i00 + d01 * i01, d00 * i10 + d01 * i11, d10 * i00 + d11 * i01, d10 * i10 + d11 * i11], -1)
        ab = torch.abs
        r["Cjs"] = torch.stack([ab(d00 * i00) + ab(d01 * i01), ab(d00 * i10) + ab(d01 * i11), ab(d10 * i00) + ab(d11 * i01), ab(d10 * i10) + ab(d11 * i11)], -1)
        M = lambda a, b, c, d: torch.stack([torch.stack([a, b], -1), torch.stack([c, d], -1)], -2)
        inv, S, dJ = M(i00, i01, i10, i11), M(s0, s1, s2, s3), M(d00, d01, d10, d11)
        e = S.transpose(-1, -2) @ dJ
        r["djd"] = (-(inv.transpose(-1, -2) @ e @ inv.transpose(-1, -2))).reshape(*d00.shape, 4)
        # absolute companions of both routes to d jd: -inv^T (S^T dJ) inv^T entry by entry, and through adj / det (d adj = d inv / det, d det = -sum d inv adj / det^2)
        eabs = S.abs().transpose(-1, -2) @ dJ.abs()
        c1 = inv.abs().transpose(-1, -2) @ eabs @ inv.abs().transpose(-1, -2)
        a0, a1, a2, a3 = A["jd"]
        adj = M(a3, -a1, -a2, a0)
        rd = A["rdet"][..., None, None]
        swap = M(eabs[..., 1, 1], eabs[..., 0, 1], eabs[..., 1, 0], eabs[..., 0, 0])           # d adj lands on jd with the diagonal swapped
        c2 = swap * rd + M(a3, a2, a1, a0).abs() * ((eabs * adj.abs()).sum((-1, -2))[..., None, None] * rd * rd)
        r["Cjd"] = (c1 + c2).reshape(*d00.shape, 4)
        r["einv"] = (inv.abs().transpose(-1, -2), S.abs().transpose(-1, -2))
    if "h" in f:
        hx, hy, hz = f["h"]
        x0, y0 = dmx[:, 0], dmy[:, 0]
        dhx, dhy = x0 / hz, y0 / hz
        dhz = -(x0 * hx + y0 * hy) / (hz * hz)
        if wrong == "dbg no hz":
            dhz = torch.zeros_like(dhz)
        t9 = [dhx * f["gx"], dhx * f["gy"], dhx, dhy * f["gx"], dhy * f["gy"], dhy, dhz * f["gx"], dhz * f["gy"], dhz]
        r.update(t9=t9, dh3=(dhx, dhy, dhz), dbg=torch.stack([t.sum((1, 2)) for t in t9], -1), Sdbg=torch.stack([t.abs().sum((1, 2)) for t in t9], -1),
                 dhzabs=((x0 * hx).abs() + (y0 * hy).abs()) / (hz * hz))
    return r


# ------------------------------------------------------------------------------------------------------------------ softmax_combine
def softmax_combine_fwd(logit, motions):
    """logit [B][H][W][K1], motions [B][K1][H][W][2] -> mask [B][K1][H][W], deformation [B][H][W][2], logit_nchw; a = l - max, s = sum exp(a), the terms
    mask_k motion_k and Sdef = sum_k |mask_k motion_k|"""
    l = logit.to(F64)
    a = l - l.max(-1, keepdim=True).values
    e = torch.exp(a)
    s = e.sum(-1, keepdim=True)
    mask = e / s
    mo = motions.to(F64).permute(0, 2, 3, 1, 4)            # [B][H][W][K1][2]
    t = mask.unsqueeze(-1) * mo
    return dict(mask=mask.permute(0, 3, 1, 2), deformation=t.sum(3), Sdef=t.abs().sum(3), logit_nchw=l.permute(0, 3, 1, 2), a=a, s=s, m=mask, mo=mo)


def softmax_combine_bwd(motions, mask, ddef, dmask, dlogit_nchw, wrong=""):
    """mask [B][K1][H][W] as given (what the forward stored) -> dlogit [B][H][W][K1] and dmotions [B][K1][H][W][2] (the increments); dm_k = ddef . motion_k +
    dmask_k with S3 its absolute terms, dot = sum_k mask_k dm_k with Sdot = sum_k |mask_k dm_k|"""
    m = mask.to(F64).permute(0, 2, 3, 1)
    mo = motions.to(F64).permute(0, 2, 3, 1, 4)
    B, H, W, K1 = m.shape
    dd = ddef.to(F64) if ddef is not None else torch.zeros(B, H, W, 2, dtype=F64)
    p = mo * dd.unsqueeze(3)
    dk = dmask.to(F64).permute(0, 2, 3, 1) if dmask is not None else torch.zeros_like(m)
    dm = p.sum(-1) + dk
    S3 = p.abs().sum(-1) + dk.abs()
    dot = (m * dm).sum(-1, keepdim=True)
    Sdot = (m * dm).abs().sum(-1, keepdim=True)
    core = m * (dm if wrong == "no dot" else dm - dot)
    nchw = dlogit_nchw.to(F64).permute(0, 2, 3, 1) if dlogit_nchw is not None else torch.zeros_like(m)
    dmot = (m.unsqueeze(-1) * dd.unsqueeze(3)).permute(0, 3, 1, 2, 4)
    return dict(dlogit=core + nchw, core=core, nchw=nchw, dm=dm, S3=S3, dot=dot, Sdot=Sdot, m=m, dmotions=dmot)


# ------------------------------------------------------------------------------------------------------------------ kp_head
def kp_head_fwd(logits, jm, T, mx=None, wrong=""):
    """logits [B][H][W][K], jm [B][H][W][4] or None, for a common maximum mx [B][K] of logits / T (None: the exact one) -> heat [B][HW][K], kp [B][K][2], jac
    [B][K][4], stat [B][K][2] = (mx, 1 / sum exp(logits / T - mx)); s = logits / T, a = s - mx, e = exp(a), S = sum e; Skp / Sjac the sums of |heat grid| /
    |heat jm|"""
    B, H, W, K = logits.shape
    s = logits.to(F64).reshape(B, H * W, K) / T
    mx = s.max(1).values if mx is None else mx.to(F64)
    a = s - mx.unsqueeze(1)
    e = torch.exp(a)
    S = e.sum(1)
    heat = e / S.unsqueeze(1)
    gx, gy = grid(H, W, wrong)
    g = torch.stack([gx.reshape(-1), gy.reshape(-1)], -1)   # [HW][2]
    tk = heat.unsqueeze(-1) * g.view(1, H * W, 1, 2)
    r = dict(heat=heat, kp=tk.sum(1), Skp=tk.abs().sum(1), stat=torch.stack([mx, 1.0 / S], -1), s=s, a=a, e=e, S=S, g=g)
    if jm is not None:
        tj = heat.unsqueeze(-1) * jm.to(F64).reshape(B, H * W, 1, 4)
        r.update(jac=tj.sum(1), Sjac=tj.abs().sum(1))
    return r


def kp_head_bwd(logits, jm, T, kp, jac, stat, dkp, djac, wrong=""):
    """recomputed from what the forward stored, as the kernel does: p_k = exp(logits / T - stat0) stat1, t = g . dkp + jm . djac - (kp . dkp + jac . djac),
    dlogits [B][H][W][K] = p_k t / T, djm [B][H][W][4] = sum_k p_k djac_k (the increments); Tabs: the absolute terms of t; Sjm = sum_k |p_k djac_k|"""
    B, H, W, K = logits.shape
    s = logits.to(F64).reshape(B, H * W, K) / T
    st = stat.to(F64)
    a = s - st[..., 0].unsqueeze(1)
    pk = torch.exp(a) * st[..., 1].unsqueeze(1)
    gx, gy = grid(H, W, wrong)
    g = torch.stack([gx.reshape(-1), gy.reshape(-1)], -1).view(1, H * W, 1, 2)
    gk = dkp.to(F64).view(B, 1, K, 2) if dkp is not None else torch.zeros(B, 1, K, 2, dtype=F64)
    k64 = kp.to(F64).view(B, 1, K, 2)
    t = (g * gk).sum(-1) - (k64 * gk).sum(-1)
    Tabs = (g * gk).abs().sum(-1) + (k64 * gk).abs().sum(-1)
    r = dict(s=s, a=a, pk=pk, gk=gk)
    if jm is not None and djac is not None:
        j = jm.to(F64).reshape(B, H * W, 1, 4)
        dj = djac.to(F64).view(B, 1, K, 4)
        ja = jac.to(F64).view(B, 1, K, 4)
        t = t + ((j * dj).sum(-1) if wrong == "E no jac" else ((j - ja) * dj).sum(-1))
        Tabs = Tabs + ((j - ja) * dj).abs().sum(-1)
        pj = pk.unsqueeze(-1) * dj
        r.update(djm=pj.sum(2).view(B, H, W, 4), Sjm=pj.abs().sum(2).view(B, H, W, 4), dj=dj)
    r.update(t=t, Tabs=Tabs, dlogits=(pk * t / T).view(B, H, W, K))
    return r
