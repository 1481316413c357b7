"""Plain float64 reference of the sampling operations of include/mrfa_hip.h (grid_sample, the correlation-window lookup, the align_corners=True resize)
with the companion outputs a derived, per-element error bound needs.  torch float64 only; nothing from mrfa_amd or oracle; no call into F.grid_sample /
F.interpolate (tests/test_sample_reference.py holds this file against them).  Every function runs on the device of its arguments.

One engine, `bilinear`: P sample points (image index, ix, iy) on a [Nimg, H, W, C] map, zeros padding:
  * tap (y, x) of the four (y0 | y0+1, x0 | x0+1), x0 = floor(ix), exists when it lies inside the image; a tap that does not exist has value 0, in the
    output AND in the difference quotients of d out / d(ix, iy);
  * a point whose coordinate is NaN, +-inf, <= -1 or >= W (H) is `dead`: output 0, nothing to the input gradient, coordinate gradient 0;
  * at an exact integer coordinate fx = 0 and the derivative is the one-sided one of the cell [x0, x0 + 1) (what the kernels and ATen compute).

Companions (the bound of tests/test_sample_kernels_gpu.py is built from these, never from a tensor-wide maximum):
  S_out  [P, C]   sum |w v| over the taps of an output element
  tap_wide [P, C] max |v| over the existing pixels of the 4 x 4 neighbourhood x0-1 .. x0+2: the four taps and the ones a coordinate that moves by a rounding
                  error across an integer would use instead
  S_din, k_din    per input-gradient element the sum of |contribution| and (per pixel) their number
  C_din           per input-gradient element sum |g_p| * delta_p over the points p whose 4 x 4 neighbourhood holds it (delta_p: the caller's coordinate error)
  S_gx, S_gy [P]  sum over channels of |g| (|v01| + |v00|)(1 - fy) + ... : the absolute sum behind d / d ix, d / d iy
  T      [P]      sum over channels of |g| (|v00| + |v01| + |v10| + |v11|)
  dist_x, dist_y  distance of the coordinate to the nearest integer (inf for dead points)"""
import torch
import torch.nn.functional as F

F64 = torch.float64


def ulp32(v):
    """spacing of fp32 numbers at |v| (float64 tensor): 2^(e - 24) for |v| = m 2^e, m in [0.5, 1); the spacing of the smallest normal below it"""
    a = torch.nan_to_num(v.abs().to(F64), nan=0.0, posinf=3e38, neginf=3e38).clamp(min=2.0 ** -126)
    _, e = torch.frexp(a)
    return torch.ldexp(torch.ones_like(a), e - 24)


def bilinear(src, n, ix, iy, g=None, delta=None, din0=None):
    Nimg, H, W, Cc = src.shape
    dev = src.device
    P = ix.numel()
    live = torch.isfinite(ix) & torch.isfinite(iy) & (ix > -1) & (iy > -1) & (ix < W) & (iy < H)
    zx, zy = torch.where(live, ix, torch.zeros_like(ix)), torch.where(live, iy, torch.zeros_like(iy))
    fx0, fy0 = zx.floor(), zy.floor()
    x0, y0 = fx0.long(), fy0.long()
    fx, fy = zx - fx0, zy - fy0
    flat = src.reshape(Nimg * H * W, Cc)
    taps = []                                          # (linear index, exists [P], weight [P], value [P, C])
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xx, yy = x0 + dx, y0 + dy
        ok = live & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        idx = (n * H + yy.clamp(0, H - 1)) * W + xx.clamp(0, W - 1)
        w = (fx if dx else 1 - fx) * (fy if dy else 1 - fy)
        w = torch.where(ok, w, torch.zeros_like(w))
        v = torch.where(ok[:, None], flat[idx], torch.zeros((), dtype=F64, device=dev))
        taps.append((idx, ok, w, v))
    r = {"live": live, "fx": fx, "fy": fy, "x0": x0, "y0": y0}
    r["out"] = sum(w[:, None] * v for _, _, w, v in taps)
    r["S_out"] = sum(w[:, None] * v.abs() for _, _, w, v in taps)
    inf = torch.full_like(ix, float("inf"))
    r["dist_x"] = torch.where(live, torch.minimum(fx, 1 - fx), inf)
    r["dist_y"] = torch.where(live, torch.minimum(fy, 1 - fy), inf)
    # max |v| over the 4 x 4 neighbourhood [y0 - 1, y0 + 2] x [x0 - 1, x0 + 2]: pool once per image, gather once per point
    a = F.pad(src.abs().permute(0, 3, 1, 2), (2, 2, 2, 2))                        # [Nimg, C, H + 4, W + 4]; padded index = index + 2
    a = F.max_pool2d(a, 4, 1)                                                    # [.., H + 1, W + 1]; entry j covers padded j .. j + 3 = index j - 2 .. j + 1
    a = a.permute(0, 2, 3, 1).reshape(Nimg * (H + 1) * (W + 1), Cc)
    wide = a[(n * (H + 1) + (y0 + 1).clamp(0, H)) * (W + 1) + (x0 + 1).clamp(0, W)]  # entry x0 + 1 covers x0 - 1 .. x0 + 2
    r["tap_wide"] = torch.where(live[:, None], wide, torch.zeros((), dtype=F64, device=dev))
    if g is None:
        return r
    din = torch.zeros(Nimg * H * W, Cc, dtype=F64, device=dev)
    S = torch.zeros_like(din) if din0 is None else din0.reshape(Nimg * H * W, Cc).abs().clone()
    k = torch.zeros(Nimg * H * W, dtype=F64, device=dev)
    for idx, ok, w, _ in taps:
        din.index_add_(0, idx, w[:, None] * g)
        S.index_add_(0, idx, w[:, None] * g.abs())
        k.index_add_(0, idx, ok.to(F64))
    r["din"], r["S_din"], r["k_din"] = din.view(Nimg, H, W, Cc), S.view(Nimg, H, W, Cc), k.view(Nimg, H, W)
    if delta is not None:
        # scatter |g| delta at (y0, x0) of a map padded by (2 before, 1 after), then a 4 x 4 box sum: pixel x collects the points with x0 in [x - 2, x + 1]
        sc = torch.zeros(Nimg * (H + 3) * (W + 3), Cc, dtype=F64, device=dev)
        d = torch.where(live, delta, torch.zeros_like(delta))
        sc.index_add_(0, (n * (H + 3) + y0 + 2) * (W + 3) + x0 + 2, g.abs() * d[:, None])     # x0 in [-1, W - 1] -> padded [1, W + 1]
        sc = sc.view(Nimg, H + 3, W + 3, Cc).permute(0, 3, 1, 2)
        r["C_din"] = (F.avg_pool2d(sc, 4, 1) * 16).permute(0, 2, 3, 1)             # entry x covers padded x .. x + 3 = x0 in [x - 2, x + 1]
    (_, _, _, v00), (_, _, _, v01), (_, _, _, v10), (_, _, _, v11) = taps
    fxc, fyc = fx[:, None], fy[:, None]
    r["gx"] = (g * ((v01 - v00) * (1 - fyc) + (v11 - v10) * fyc)).sum(1)
    r["gy"] = (g * ((v10 - v00) * (1 - fxc) + (v11 - v01) * fxc)).sum(1)
    ga = g.abs()
    r["S_gx"] = (ga * ((v01.abs() + v00.abs()) * (1 - fyc) + (v11.abs() + v10.abs()) * fyc)).sum(1)
    r["S_gy"] = (ga * ((v10.abs() + v00.abs()) * (1 - fxc) + (v11.abs() + v01.abs()) * fxc)).sum(1)
    r["T"] = (ga * (v00.abs() + v01.abs() + v10.abs() + v11.abs())).sum(1)
    return r


# ---------------------------------------------------------------------------------------------------------------- grid_sample
def gs_coords(grid, mode, Hi, Wi):
    """grid [N, Ho, Wo, 2] fp32 -> (ix, iy, dx, dy) float64 [N*Ho*Wo]: the header's coordinate formula evaluated in float64 on the fp32 grid values, and the
    error an fp32 evaluation of it may make: one ulp (twice the rounding error) of the result of each fp32 operation, carried to the end of the formula.
    mode 0: ((g + 1) W - 1) / 2  (add, multiply, subtract; the halving is exact).  mode 1: ox + g (one add)."""
    N, Ho, Wo, _ = grid.shape
    gd = grid.to(F64)
    out = []
    for k, (size, no) in enumerate(((Wi, Wo), (Hi, Ho))):
        gk = gd[..., k]
        if mode == 0:
            t1 = gk + 1
            t2 = t1 * size
            c = (t2 - 1) / 2
            d = (ulp32(t1) * size + ulp32(t2) + ulp32(t2 - 1)) / 2
        else:
            o = torch.arange(no, dtype=F64, device=grid.device)
            c = gk + (o.view(1, 1, no) if k == 0 else o.view(1, no, 1))
            d = ulp32(c)
        out.append((c.reshape(-1), torch.nan_to_num(d, nan=0.0).reshape(-1)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def gs_coords_exact(grid, mode, Hi, Wi):
    """[N*Ho*Wo] bool: every fp32 step of the coordinate formula is exact on this grid value (then an fp32 evaluation, contracted to fma or not, gives
    the reference's coordinate itself: the deliberate integer and border coordinates)"""
    N, Ho, Wo, _ = grid.shape
    ok = torch.ones(N, Ho, Wo, dtype=torch.bool, device=grid.device)
    for k, (size, no) in enumerate(((Wi, Wo), (Hi, Ho))):
        g32, g64 = grid[..., k].float(), grid[..., k].to(F64)
        if mode == 0:
            a32, a64 = g32 + 1, g64 + 1
            b32, b64 = a32 * float(size), a64 * size
            ok &= (a32.to(F64) == a64) & (b32.to(F64) == b64) & ((b32 - 1).to(F64) == b64 - 1)
        else:
            o = torch.arange(no, device=grid.device)
            o = o.view(1, 1, no) if k == 0 else o.view(1, no, 1)
            ok &= (g32 + o.float()).to(F64) == g64 + o.to(F64)
    return ok.reshape(-1)


def corr_coords_exact(coords, radius):
    """[Q] bool: c / 2^lvl + (a - r) is exact in fp32 for every window element of both levels"""
    c32, c64 = coords.float(), coords.to(F64)
    ok = torch.ones(coords.shape[0], dtype=torch.bool, device=coords.device)
    for inv in (1.0, 0.5):
        for off in range(-radius, radius + 1):
            ok &= ((c32 * inv + float(off)).to(F64) == c64 * inv + off).all(dim=1)
    return ok


def _gs(x, grid, mode, in_rep, dout=None, din0=None):
    Nin, Hi, Wi, Cc = x.shape
    N, Ho, Wo, _ = grid.shape
    ix, iy, dx, dy = gs_coords(grid, mode, Hi, Wi)
    n = (torch.arange(N, device=x.device) // in_rep).view(N, 1, 1).expand(N, Ho, Wo).reshape(-1)
    g = None if dout is None else dout.to(F64).reshape(-1, Cc)
    r = bilinear(x.to(F64), n, ix, iy, g, dx + dy, None if din0 is None else din0.to(F64))
    r["dx"], r["dy"] = dx, dy
    r["mx"], r["my"] = (0.5 * Wi, 0.5 * Hi) if mode == 0 else (1.0, 1.0)
    return r


def grid_sample_ref(x, grid, mode, in_rep=1, full=False):
    """x [Nin, Hi, Wi, C], grid [N, Ho, Wo, 2] (fp32 values) -> out [N, Ho, Wo, C] float64 (full=True: the engine's dictionary with every companion)"""
    r = _gs(x, grid, mode, in_rep)
    return r if full else r["out"].view(*grid.shape[:3], x.shape[-1])


def grid_sample_grads_ref(x, grid, dout, mode, in_rep=1, full=False, din0=None):
    """-> (din [Nin, Hi, Wi, C], dgrid [N, Ho, Wo, 2]) float64; dgrid is d / d(grid value): mode 0 carries the factors W / 2, H / 2"""
    r = _gs(x, grid, mode, in_rep, dout, din0)
    r["dgrid"] = torch.stack([r["gx"] * r["mx"], r["gy"] * r["my"]], dim=1).view(*grid.shape[:3], 2)
    return r if full else (r["din"], r["dgrid"])


# ---------------------------------------------------------------------------------------------------------------- correlation-window lookup
def _corr(vols, coords, radius, dout=None, dvol0=None):
    Q = coords.shape[0]
    win = 2 * radius + 1
    nwin = win * win
    dev = coords.device
    c = coords.to(F64)
    e = torch.arange(nwin, device=dev)
    a, b = (e // win - radius).to(F64), (e % win - radius).to(F64)
    n = torch.arange(Q, device=dev).view(Q, 1).expand(Q, nwin).reshape(-1)
    res = []
    for lvl, vol in enumerate(vols):
        inv = 0.5 ** lvl
        ix = (c[:, 0:1] * inv + a.view(1, nwin)).reshape(-1)
        iy = (c[:, 1:2] * inv + b.view(1, nwin)).reshape(-1)
        delta = torch.nan_to_num(ulp32(ix) + ulp32(iy), nan=0.0)                  # one fp32 add each (the halving is exact)
        g = None if dout is None else dout.to(F64)[:, lvl * nwin:(lvl + 1) * nwin].reshape(-1, 1)
        d0 = None if dvol0 is None else dvol0[lvl].to(F64)[..., None]
        r = bilinear(vol.to(F64)[..., None], n, ix, iy, g, delta, d0)
        r["delta_x"], r["delta_y"], r["inv"] = ulp32(ix), ulp32(iy), inv
        res.append(r)
    return res


def corr_lookup_ref(vol0, vol1, coords, radius, full=False):
    """vol0 [Q, Hs, Ws], vol1 [Q, Hs/2, Ws/2], coords [Q, 2] (x, y) -> out [Q, 2 (2r+1)^2]: channel lvl nwin + a win + b at (x / 2^lvl + a - r, y / 2^lvl + b - r)"""
    res = _corr((vol0, vol1), coords, radius)
    Q = coords.shape[0]
    return res if full else torch.cat([r["out"].view(Q, -1) for r in res], dim=1)


def corr_lookup_grads_ref(vol0, vol1, coords, dout, radius, full=False, dvol0=None):
    """-> (dvol0, dvol1, dcoords [Q, 2]); the level-1 coordinate gradient carries the factor 1 / 2"""
    res = _corr((vol0, vol1), coords, radius, dout, dvol0)
    Q = coords.shape[0]
    dc = sum(torch.stack([r["gx"].view(Q, -1).sum(1), r["gy"].view(Q, -1).sum(1)], dim=1) * r["inv"] for r in res)
    return (res, dc) if full else (res[0]["din"][..., 0], res[1]["din"][..., 0], dc)


# ---------------------------------------------------------------------------------------------------------------- resize, align_corners=True
def resize_coords(Ni, No, dev):
    """source coordinate of output o: o (Ni - 1) / (No - 1) (0 when No == 1), and the error of its fp32 evaluation: the quotient is rounded once (one ulp of
    it, times o) and so is the product"""
    o = torch.arange(No, dtype=F64, device=dev)
    s = (Ni - 1) / (No - 1) if No > 1 else 0.0
    c = o * (Ni - 1) / (No - 1) if No > 1 else o * 0.0                            # (integer product, one correctly rounded division)
    d = ulp32(torch.tensor(s, dtype=F64, device=dev)) * o + ulp32(c) if s != 0.0 else torch.zeros_like(c)
    return c, d


def _resize(x, Ho, Wo, dout=None, mul=1.0, din0=None):
    N, Hi, Wi, Cc = x.shape
    dev = x.device
    cx, dx = resize_coords(Wi, Wo, dev)
    cy, dy = resize_coords(Hi, Ho, dev)
    ix = cx.view(1, 1, Wo).expand(N, Ho, Wo).reshape(-1)
    iy = cy.view(1, Ho, 1).expand(N, Ho, Wo).reshape(-1)
    delta = (dx.view(1, 1, Wo) + dy.view(1, Ho, 1)).expand(N, Ho, Wo).reshape(-1)
    n = torch.arange(N, device=dev).view(N, 1, 1).expand(N, Ho, Wo).reshape(-1)
    g = None if dout is None else dout.to(F64).reshape(-1, Cc) * mul
    r = bilinear(x.to(F64), n, ix, iy, g, delta, None if din0 is None else din0.to(F64))
    r["delta"] = delta
    return r


def resize_ref(x, Ho, Wo, mul=1.0, acc=None, full=False):
    """x [N, Hi, Wi, C] -> out [N, Ho, Wo, C] = (acc +) mul * bilinear(x) at (ox (Wi-1)/(Wo-1), oy (Hi-1)/(Ho-1)); the tap one past the last pixel has weight 0"""
    r = _resize(x, Ho, Wo)
    N, _, _, Cc = x.shape
    a = 0 if acc is None else acc.to(F64).reshape(-1, Cc)
    r["S_out"] = r["S_out"] * abs(mul) + (0 if acc is None else a.abs())
    r["out"] = r["out"] * mul + a
    return r if full else r["out"].view(N, Ho, Wo, Cc)


def resize_grads_ref(x_shape, dout, mul=1.0, full=False, din0=None):
    """dout [N, Ho, Wo, C] -> din [N, Hi, Wi, C] = mul * adjoint; x_shape = (N, Hi, Wi, C)"""
    N, Ho, Wo, Cc = dout.shape
    r = _resize(torch.zeros(x_shape, dtype=F64, device=dout.device), Ho, Wo, dout, mul, din0)
    return r if full else r["din"]
