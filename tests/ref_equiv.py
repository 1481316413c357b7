"""The numpy fp64 specification of the equivariance entries of libmrfa_hip.so (include/mrfa_equiv_hip.h): the thin-plate-spline transform, its closed-form
Jacobian, the two loss terms forward and backward, the frame warp -- and a `Library` that stands where the binding's ctypes library stands (pointers are
addresses of CPU memory), the way tests/ref_resize.py does for the resize entries.

Every function evaluates on `VM` values: a VM carries the fp64 value `v`, the ABSOLUTE-VALUE EVALUATION `m` -- the same expression with every operand and
every partial result replaced by its magnitude -- and the operation depth `n`, the largest number of roundings on a path from an input to this result.  The
standard forward bound of an fp32 evaluation of the same expression, in any order of its sums and with or without fused multiply-adds, is then

    |fl32(f) - f|  <=  n * U * f(|.|)  =  bound(vm)            U = 2^-24 (tests/kernel_check.py), first order in U

Three rules go beyond +, -, * of magnitudes:
  * dx = x - q of two fp32 INPUTS is one correctly rounded operation: it enters as an operand of magnitude |dx| and depth 1 (not |x| + |q|).
  * 1 / b has magnitude m(b) / b^2: the relative error of b, at most n U m(b) / |b|, is the relative error of 1 / b.  For the 2x2 inverse that is
    (|a||d| + |b||c|) over the true |det|, once more over |det|.
  * log(a) has magnitude |log a| + m(a) / a and two roundings more than a: HIP's logf is accurate to 1 ulp = 2 U relative (ROCm documentation, "HIP math
    API", table "Single precision mathematical functions", row logf: maximum error 1 ULP), and a relative error of its argument moves a logarithm by the
    same amount absolutely.
sign() is exact where its argument's sign is; the tests leave out the elements where the argument is smaller than its own bound."""
import ctypes as C

import numpy as np

VERSION = 1
MAX_POINTS = 64
U = 2.0 ** -24
EPS = 1e-6                                   # the specification's eps
EPS32 = float(np.float32(1e-6))              # what the fp32 kernels add (1e-6f)


class VM:
    """value, absolute-value evaluation and operation depth (module docstring); numpy arrays broadcast"""
    __slots__ = ("v", "m", "n")

    def __init__(self, v, m=None, n=0):
        self.v = np.asarray(v, dtype=np.float64)
        self.m = np.abs(self.v) if m is None else np.asarray(m, dtype=np.float64)
        self.n = int(n)

    @staticmethod
    def of(x):
        return x if isinstance(x, VM) else VM(x)

    def __add__(self, o):
        o = VM.of(o)
        return VM(self.v + o.v, self.m + o.m, max(self.n, o.n) + 1)

    def __sub__(self, o):
        o = VM.of(o)
        return VM(self.v - o.v, self.m + o.m, max(self.n, o.n) + 1)

    def __mul__(self, o):
        o = VM.of(o)
        return VM(self.v * o.v, self.m * o.m, max(self.n, o.n) + 1)

    def __truediv__(self, o):
        o = VM.of(o)
        return VM(self.v / o.v, self.m * o.m / (o.v * o.v), max(self.n, o.n) + 1)

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return VM.of(o) - self

    def __neg__(self):
        return VM(-self.v, self.m, self.n)

    def abs(self):
        return VM(np.abs(self.v), self.m, self.n)

    def sign(self):
        return VM(np.sign(self.v), np.abs(np.sign(self.v)), 0)

    def log(self):
        return VM(np.log(self.v), np.abs(np.log(self.v)) + self.m / self.v, self.n + 2)

    def sum(self, axis):
        """a sum of k terms in any order: at most k - 1 additions deep"""
        k = self.v.shape[axis]
        return VM(self.v.sum(axis), self.m.sum(axis), self.n + max(k - 1, 0))

    def __getitem__(self, idx):
        return VM(self.v[idx], self.m[idx], self.n)

    @property
    def bound(self):
        return self.n * U * self.m


def stack(vms, axis=-1):
    return VM(np.stack(np.broadcast_arrays(*[x.v for x in vms]), axis), np.stack(np.broadcast_arrays(*[x.m for x in vms]), axis), max(x.n for x in vms))


def exact_diff(x, q):
    """x - q of fp32 inputs: one rounding, magnitude |x - q|"""
    d = np.asarray(x, np.float64) - np.asarray(q, np.float64)
    return VM(d, np.abs(d), 1)


# ------------------------------------------------------------------------------------------------------------------------------------- the spline
def u_of(d, eps=EPS):
    d = VM.of(d)
    return d * d * (d + eps).log()


def du_of(d, eps=EPS):
    d = VM.of(d)
    de = d + eps
    return 2.0 * d * de.log() + d * d / de


def ddu_of(d, eps=EPS):
    d = VM.of(d)
    de = d + eps
    q = d / de
    return 2.0 * de.log() + 4.0 * q - q * q


def tps_sums(x, y, points, c, eps=EPS):
    """the six sums at points (x, y) of shape S, control points (P,2), weights c broadcastable to S + (P,): dict of VM of shape S"""
    x, y, c = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(c, np.float64)
    points = np.asarray(points, np.float64).reshape(-1, 2)
    if points.shape[0] == 0:
        z = VM(np.zeros(x.shape))
        return dict(s=z, gx=z, gy=z, hxx=z, hxy=z, hyy=z)
    dx, dy = exact_diff(x[..., None], points[:, 0]), exact_diff(y[..., None], points[:, 1])
    d = dx.abs() + dy.abs()
    sx, sy, ck = dx.sign(), dy.sign(), VM(c)
    c1, c2 = ck * du_of(d, eps), ck * ddu_of(d, eps)
    return dict(s=(ck * u_of(d, eps)).sum(-1), gx=(c1 * sx).sum(-1), gy=(c1 * sy).sum(-1),
                hxx=(c2 * (sx * sx)).sum(-1), hxy=(c2 * (sx * sy)).sum(-1), hyy=(c2 * (sy * sy)).sum(-1))


def _split(theta, points, params, B):
    theta = np.asarray(theta, np.float64).reshape(B, 2, 3)
    points = np.zeros((0, 2)) if points is None else np.asarray(points, np.float64).reshape(-1, 2)
    P = points.shape[0]
    params = np.zeros((B, 0)) if P == 0 else np.asarray(params, np.float64).reshape(B, P)
    return theta, points, params


def _point_terms(theta, points, params, pts, eps):
    """pts (B,S,2) -> (sums, Tx, Ty, JT as (a, b, c, d)), every VM of shape (B,S)"""
    B = pts.shape[0]
    theta, points, params = _split(theta, points, params, B)
    x, y = pts[..., 0], pts[..., 1]
    u = tps_sums(x, y, points, params[:, None, :], eps)
    th = [[VM(theta[:, r, k][:, None]) for k in range(3)] for r in range(2)]
    tx = th[0][0] * x + th[0][1] * y + th[0][2] + u["s"]
    ty = th[1][0] * x + th[1][1] * y + th[1][2] + u["s"]
    jt = (th[0][0] + u["gx"], th[0][1] + u["gy"], th[1][0] + u["gx"], th[1][1] + u["gy"])
    return u, tx, ty, jt


def warp_points(theta, points, params, pts, eps=EPS):
    """T(pts): pts (B,S,2) -> VM (B,S,2)"""
    pts = np.asarray(pts, np.float64)
    _, tx, ty, _ = _point_terms(theta, points, params, pts, eps)
    return stack([tx, ty])


def jacobian(theta, points, params, pts, eps=EPS):
    """JT(pts): pts (B,S,2) -> VM (B,S,2,2)"""
    pts = np.asarray(pts, np.float64)
    _, _, _, jt = _point_terms(theta, points, params, pts, eps)
    return _m2_stack(jt)


# ------------------------------------------------------------------------------------------------------------------------------------- 2 x 2
def _m2(a):
    a = np.asarray(a, np.float64)
    return tuple(VM(a[..., i, j]) for i in range(2) for j in range(2))


def _m2_stack(m):
    return stack([stack([m[0], m[1]]), stack([m[2], m[3]])], axis=-2)


def _mul(x, y):
    return (x[0] * y[0] + x[1] * y[2], x[0] * y[1] + x[1] * y[3], x[2] * y[0] + x[3] * y[2], x[2] * y[1] + x[3] * y[3])


def _tr(x):
    return (x[0], x[2], x[1], x[3])


def _inv(m):
    det = m[0] * m[3] - m[1] * m[2]
    return (m[3] / det, -m[1] / det, -m[2] / det, m[0] / det)


# ------------------------------------------------------------------------------------------------------------------------------------- the terms
def loss_fwd(kp_d, jac_d, kp_t, jac_t, theta, points, params, w_e, w_j, eps=EPS):
    """-> dict(value VM (), r VM (B,K,2), term VM (B,K,2,2) or None, e = I - V VM (B,K,2,2) or None)"""
    kp_d, kp_t = np.asarray(kp_d, np.float64), np.asarray(kp_t, np.float64)
    B, K = kp_d.shape[:2]
    _, tx, ty, jt = _point_terms(theta, points, params, kp_t, eps)
    r = stack([VM(kp_d[..., 0]) - tx, VM(kp_d[..., 1]) - ty])
    total = VM(r.v.reshape(-1), r.m.reshape(-1), r.n).abs().sum(0)
    value = (VM(w_e) / float(2 * B * K)) * total
    out = dict(value=value, r=r, term=None, e=None)
    if jac_d is not None:
        v = _mul(_inv(_m2(jac_d)), _mul(jt, _m2(jac_t)))
        e = (1.0 - v[0], 0.0 - v[1], 0.0 - v[2], 1.0 - v[3])
        out["e"] = _m2_stack(e)
        out["term"] = _m2_stack(tuple(VM(w_j) * x.abs() for x in e))
    return out


def loss_bwd(kp_d, jac_d, kp_t, jac_t, theta, points, params, w_e, w_j, g_value, g_term, eps=EPS):
    """-> dict(d_kp_d, d_kp_t VM (B,K,2); d_jac_d, d_jac_t VM (B,K,2,2) or None)"""
    kp_d, kp_t = np.asarray(kp_d, np.float64), np.asarray(kp_t, np.float64)
    B, K = kp_d.shape[:2]
    u, tx, ty, jt = _point_terms(theta, points, params, kp_t, eps)
    gscale = VM(float(g_value)) * (VM(w_e) / float(2 * B * K))
    dk = (gscale * (VM(kp_d[..., 0]) - tx).sign(), gscale * (VM(kp_d[..., 1]) - ty).sign())
    gt = (-dk[0], -dk[1])
    dx, dy = jt[0] * gt[0] + jt[2] * gt[1], jt[1] * gt[0] + jt[3] * gt[1]
    out = dict(d_kp_d=stack(dk), d_jac_d=None, d_jac_t=None)
    if jac_d is not None:
        jt_in, ji, g = _m2(jac_t), _inv(_m2(jac_d)), _m2(g_term)
        m = _mul(jt, jt_in)
        v = _mul(ji, m)
        e = (1.0 - v[0], 0.0 - v[1], 0.0 - v[2], 1.0 - v[3])
        gv = tuple(-(VM(w_j) * gg * ee.sign()) for gg, ee in zip(g, e))
        jit = _tr(ji)
        gm, gji = _mul(jit, gv), _mul(gv, _tr(m))
        out["d_jac_d"] = _m2_stack(tuple(-x for x in _mul(jit, _mul(gji, jit))))
        out["d_jac_t"] = _m2_stack(_mul(_tr(jt), gm))
        gjt = _mul(gm, _tr(jt_in))
        ggx, ggy = gjt[0] + gjt[2], gjt[1] + gjt[3]
        dx = dx + (ggx * u["hxx"] + ggy * u["hxy"])
        dy = dy + (ggx * u["hxy"] + ggy * u["hyy"])
    out["d_kp_t"] = stack([dx, dy])
    return out


# ------------------------------------------------------------------------------------------------------------------------------------- the frame warp
def coordinate_grid(H, W, dtype=np.float32):
    """make_coordinate_grid((H, W)) in `dtype`: (H,W,2), last axis (x, y).  In float32 these are the kernel's own grid values to the bit: 2 * q is exact, so
    a fused multiply-add gives the same two roundings' result."""
    xs = dtype(2.0) * (np.arange(W, dtype=dtype) / dtype(W - 1)) - dtype(1.0)
    ys = dtype(2.0) * (np.arange(H, dtype=dtype) / dtype(H - 1)) - dtype(1.0)
    return np.stack(np.broadcast_arrays(xs[None, :], ys[:, None]), -1)


def reflect_coord(v, size):
    """torch's reflect_coordinates(v, -1, 2 size - 1) then clip_coordinates: about the pixel edges -0.5 and size - 0.5, then into [0, size - 1]"""
    v = np.abs(v + 0.5)
    flips = np.floor(v / size)
    extra = v - flips * size
    v = np.where(flips.astype(np.int64) & 1, size - extra - 0.5, extra - 0.5)
    return np.clip(v, 0.0, size - 1.0)


BILINEAR_DEPTH = 8        # wx0 = 1 - wx1 (1), tap * wx * wy (2), four terms summed (3), and the weights' own wx1 = x - floor(x) (1), one to spare


def warp_frame(img, theta, points, params, eps=EPS, grid_dtype=np.float32):
    """img (N,C,H,W) -> (out fp64 (N,C,H,W), bound (N,C,H,W)).  The bound at a pixel is the coordinate bound in pixels (both axes added) times the largest
    difference between adjacent pixels of the reflect-aware 4x4 patch around the fp64 sample position -- bilinear interpolation is continuous, piecewise linear
    with those slopes, and reflection and clipping do not stretch -- plus BILINEAR_DEPTH * U * the patch's largest magnitude for the interpolation itself.
    The coordinate bound: bound() of the pixel coordinate ((T + 1) size - 1) / 2, plus U (|v| + 3 size) for reflect_coord's own four roundings."""
    img = np.asarray(img, np.float64)
    N, Cc, H, W = img.shape
    g = coordinate_grid(H, W, grid_dtype).astype(np.float64).reshape(1, H * W, 2)
    t = warp_points(theta, points, params, np.broadcast_to(g, (N, H * W, 2)), eps)
    pos, delta = [], 0.0
    for axis, size in ((0, W), (1, H)):
        pix = ((t[..., axis] + 1.0) * float(size) - 1.0) * 0.5
        pos.append(reflect_coord(pix.v, float(size)).reshape(N, H, W))
        delta = delta + (pix.bound + U * (np.abs(pix.v) + 3.0 * size)).reshape(N, H, W)
    if not (delta < 0.5).all():
        raise ValueError("the coordinate bound exceeds half a pixel: the 4x4 patch argument does not hold")
    x, y = pos
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    wx1, wy1 = x - x0, y - y0
    n_i = np.arange(N)[:, None, None, None]
    c_i = np.arange(Cc)[None, :, None, None]

    def tap(yy, xx):
        ok = ((xx < W) & (yy < H))[:, None]
        return np.where(ok, img[n_i, c_i, np.minimum(yy, H - 1)[:, None], np.minimum(xx, W - 1)[:, None]], 0.0)
    out = (tap(y0, x0) * ((1 - wx1) * (1 - wy1))[:, None] + tap(y0, x0 + 1) * (wx1 * (1 - wy1))[:, None]
           + tap(y0 + 1, x0) * ((1 - wx1) * wy1)[:, None] + tap(y0 + 1, x0 + 1) * (wx1 * wy1)[:, None])
    rows = np.clip(y0[..., None] + np.arange(-1, 3), 0, H - 1)                      # (N,H,W,4): reflection about an edge repeats the edge pixel
    cols = np.clip(x0[..., None] + np.arange(-1, 3), 0, W - 1)
    patch = img[n_i[..., None, None], c_i[..., None, None], rows[:, None, :, :, :, None], cols[:, None, :, :, None, :]]       # (N,C,H,W,4,4)
    slope = np.maximum(np.abs(np.diff(patch, axis=-1)).max((-1, -2)), np.abs(np.diff(patch, axis=-2)).max((-1, -2)))
    bound = delta[:, None] * slope + BILINEAR_DEPTH * U * np.abs(patch).max((-1, -2))
    return out, bound


# ----------------------------------------------------------------------------------------------------------------------- the entries, on CPU memory
def _view(ptr, shape):
    n = int(np.prod(shape))
    return np.frombuffer((C.c_char * (n * 4)).from_address(ptr), dtype=np.float32).reshape(shape)


class Library:
    """stands where ctypes.CDLL(libmrfa_hip.so) stands for mrfa_amd.equiv_hip: the four entries and the library's error message; fp64 results rounded to
    fp32.  `calls` lists (entry, arguments) of every call."""

    def __init__(self):
        self.error = b""
        self.calls = []

    def mrfa_equiv_version(self):
        return VERSION

    def mrfa_last_error(self):
        return self.error

    def _refuse(self, msg):
        self.error = msg.encode()
        return 1

    def _control(self, who, N, points, params, P):
        if not 0 <= P <= MAX_POINTS:
            return self._refuse(f"{who}: P must be in [0, {MAX_POINTS}], not {P}")
        if P and not (points and params):
            return self._refuse(f"{who}: null points or params with P = {P}")
        return (_view(points, (P, 2)), _view(params, (N, P))) if P else (None, None)

    def mrfa_equiv_warp_frame(self, stream, src, N, Cc, H, W, theta, points, params, P, out):
        self.calls.append(("mrfa_equiv_warp_frame", (stream, src, N, Cc, H, W, theta, points, params, P, out)))
        if N < 1 or Cc < 1:
            return self._refuse(f"equiv_warp_frame: N and C must be >= 1 (N {N}, C {Cc})")
        if H < 2 or W < 2:
            return self._refuse(f"equiv_warp_frame: H and W must be >= 2, the grid divides by size - 1 (H {H}, W {W})")
        if not (src and theta and out):
            return self._refuse("equiv_warp_frame: null pointer (in, theta or out)")
        ctl = self._control("equiv_warp_frame", N, points, params, P)
        if ctl == 1:
            return 1
        res, _ = warp_frame(_view(src, (N, Cc, H, W)), _view(theta, (N, 2, 3)), ctl[0], ctl[1], EPS32)
        _view(out, (N, Cc, H, W))[:] = res
        return 0

    def _loss_args(self, who, B, K, kp_d, kp_t, theta, points, params, P, w_j, jac):
        if B < 1 or K < 1:
            return self._refuse(f"{who}: B and K must be >= 1 (B {B}, K {K})")
        ctl = self._control(who, B, points, params, P)
        if ctl == 1:
            return 1
        if not (kp_d and kp_t and theta):
            return self._refuse(f"{who}: null pointer (kp_d, kp_t or theta)")
        n_set = sum(1 for p in jac if p)
        if n_set not in (0, len(jac)):
            return self._refuse(f"{who}: the Jacobian pointers are NULL together or not at all ({n_set} of {len(jac)} are set)")
        if (n_set != 0) != (w_j != 0):
            return self._refuse(f"{who}: the Jacobian pointers are set exactly when w_j != 0")
        return ctl

    def mrfa_equiv_loss_fwd(self, stream, B, K, kp_d, jac_d, kp_t, jac_t, theta, points, params, P, w_e, w_j, value, term):
        self.calls.append(("mrfa_equiv_loss_fwd", (stream, B, K, kp_d, jac_d, kp_t, jac_t, theta, points, params, P, w_e, w_j, value, term)))
        ctl = self._loss_args("equiv_loss_fwd", B, K, kp_d, kp_t, theta, points, params, P, w_j, (jac_d, jac_t, term))
        if ctl == 1:
            return 1
        if not value:
            return self._refuse("equiv_loss_fwd: null value")
        jd, jt = (_view(jac_d, (B, K, 2, 2)), _view(jac_t, (B, K, 2, 2))) if jac_d else (None, None)
        res = loss_fwd(_view(kp_d, (B, K, 2)), jd, _view(kp_t, (B, K, 2)), jt, _view(theta, (B, 2, 3)), ctl[0], ctl[1], w_e, w_j, EPS32)
        _view(value, (1,))[:] = res["value"].v
        if term:
            _view(term, (B, K, 2, 2))[:] = res["term"].v
        return 0

    def mrfa_equiv_loss_bwd(self, stream, B, K, kp_d, jac_d, kp_t, jac_t, theta, points, params, P, w_e, w_j, g_value, g_term, d_kp_d, d_jac_d, d_kp_t,
                            d_jac_t):
        self.calls.append(("mrfa_equiv_loss_bwd", (stream, B, K, kp_d, jac_d, kp_t, jac_t, theta, points, params, P, w_e, w_j, g_value, g_term, d_kp_d,
                                                   d_jac_d, d_kp_t, d_jac_t)))
        ctl = self._loss_args("equiv_loss_bwd", B, K, kp_d, kp_t, theta, points, params, P, w_j, (jac_d, jac_t, g_term, d_jac_d, d_jac_t))
        if ctl == 1:
            return 1
        if not (g_value and d_kp_d and d_kp_t):
            return self._refuse("equiv_loss_bwd: null pointer (g_value, d_kp_d or d_kp_t)")
        jd, jt, gt = (_view(jac_d, (B, K, 2, 2)), _view(jac_t, (B, K, 2, 2)), _view(g_term, (B, K, 2, 2))) if jac_d else (None, None, None)
        res = loss_bwd(_view(kp_d, (B, K, 2)), jd, _view(kp_t, (B, K, 2)), jt, _view(theta, (B, 2, 3)), ctl[0], ctl[1], w_e, w_j,
                       float(_view(g_value, (1,))[0]), gt, EPS32)
        _view(d_kp_d, (B, K, 2))[:] = res["d_kp_d"].v
        _view(d_kp_t, (B, K, 2))[:] = res["d_kp_t"].v
        if jac_d:
            _view(d_jac_d, (B, K, 2, 2))[:] = res["d_jac_d"].v
            _view(d_jac_t, (B, K, 2, 2))[:] = res["d_jac_t"].v
        return 0
