"""The BatchNorm kernels (csrc/norm.hip: statistics, finalize, the fused forward apply, the two-phase backward, the parameter gradients) on every dispatch path
against the float64 reference of tests/ref_norm.py (-m gpu), element by element.  tests/test_norm_reference.py runs the same drivers, inputs and bounds on the
fp32 specification (oracle/capi_emulator.py) and on deliberately wrong formulas, without a GPU: that is what shows the bounds can be met and that they
discriminate.

ISOLATION.  Every kernel is fed fp32 values the test holds (scale / shift / mean / invstd are the float64 finalize rounded once to fp32, so exactly representable)
and the reference is evaluated on those same values; phase 2 is checked against the `red` that phase 1 left (read back), finalize against float64 statistics the
test constructs over all 32 slots.  Each kernel answers for its own roundings only.  test_chain composes the bounds along stats -> finalize -> forward ->
phase 1 -> phase 2 by handing each bound the input perturbations d_* that the stage before it is allowed.

THE BOUNDS.  Every assertion is |got - ref| <= bound per element; no bound is a fraction of a tensor's maximum.  u = 2^-24, D = 2^-53.  To first order a
k-term fp32 sum errs by at most (k - 1) u sum|terms| in any order, a product or a sum by u |result|, a += by u |old + new| on top of the addend's error.  A
fused multiply-add makes fewer roundings than counted, never more.  The second-order terms are covered by taking u as 2^-24 (1 + 2^-12) throughout: the exact
factor of a k-term count is 1 / (1 - k u), 1 + 6.1e-5 for the longest sum here (k = 1024), and an elementwise chain has at most eight roundings.  What is accumulated in float64 (slot sums, atomics of the workgroups) is charged
(blocks + slots) D sum|terms|.
  sqrt and division in fp32 (eval-mode finalize only): the OpenCL full-profile limits the device library is written to, as for the transcendentals of
  tests/test_token_kernels_gpu.py: sqrt 3 ulp, x / y 2.5 ulp, one ulp at most 2 u relative: E_SQRT = 6 u, E_DIV = 5 u.  In float64 both are correctly rounded.

  mrfa_bn_stats (k = ceil(rows_per_block / 4) terms per thread, then float64):   s1: (k - 1) u sum|x|;   s2: k u sum x^2 (the square, k - 1 additions)
  finalize, train (float64 until the casts; d_t the error of the statistics, 0 where the test constructed them):
      m = t1 / n: d_m = d_t1 / n + 4 D |m|;   var = t2 / n - m^2: d_var = d_t2 / n + 2 |m| d_m + 4 D (t2 / n + m^2)   (the clamp at 0 is 1-Lipschitz)
      mean  d_m + u |m|;   invstd  i (0.5 d_var / (var + eps) + 4 D) + u i;   scale  |gamma| b_invstd + u |scale|
      shift = beta - mean scale:  b_mean |scale| + |mean| b_scale + u |mean scale| + u |shift|
      running r' = (1 - mom) r + mom s, once per group in group order, b carried along:
                   |1 - mom| b + mom b_s + 3 u (|(1 - mom) r| + |mom s|) + u |r'|     (1 - mom is a rounding; two products, the sum)
      with s = mean (b_s = b_mean) or the unbiased variance (b_s = (d_var + 4 D var) n / (n - 1) + u s)
  finalize, eval: mean = running_mean exactly; invstd = 1 / sqrtf(rv + eps): i (0.5 u + E_SQRT + E_DIV); scale, shift as above
  forward:  u = x scale + shift (+ res):   b_u = u (|x scale| + |x scale + shift| (+ |u|))  (+ |x| d_scale + d_shift)
      ReLU is 1-Lipschitz: b_a = b_u, no element of y is excluded.   pool: 0.25 (sum_4 b_a + 3 u sum_4 |a|)
      blend y = A o + v (1 - o):   |1 - o| b_v + 2 u |v (1 - o)| + u |A o| + u |y|      (1 - o is a rounding, the product, the product A o, the sum)
  backward, phase 1 (da0 = dy, or 0.25 dy at the four pixels: exact):
      dblend_a += da0 o:   u |da0 o| + u |old + da0 o|
      docc += sum_c da0 (A - a):   sum_c (|da0| b_a + 2 u |da0 (A - a)|) + (C + chunks) u (sum_c |da0 (A - a)| + |old|)     (C-term sum, one atomic per chunk)
      da = da0 (1 - o): b_da = 2 u |da|;   du = da where u > 0: b_du = b_da off the kink (below)
      dres += du:   b_du + u |old + du|
      xhat = (x - mean) invstd:   ex = 2 u |xhat| (+ d_mean invstd + |x - mean| d_invstd)
      red[c]     = sum du        (k terms per thread: ceil(rpb / 4) scalar, ceil(rpb / 16) float4):   sum b_du + (k - 1) u sum|du|
      red[C + c] = sum du xhat:  sum (|xhat| b_du + |du| ex + u |du xhat|) + (k - 1) u sum|du xhat|
  backward, phase 2 (t1, t2 the float64 slot sums of the red it is given; n = rows per group x red_world):
      k1 = t1 / n, k2 = t2 / n cast to fp32: u |k|  (+ (blocks + slots) D sum_slots |red| / n for the order of the slot sum; + b_red / n in the chain)
      gi = gamma invstd: u |gi|  (+ |gamma| b_invstd)
      dx = gi (du - k1 - xhat k2):   |gi| (b_du + b_k1 + ex |k2| + |xhat| b_k2 + u |xhat k2| + u |du - k1| + u |t|) + (b_gi + u |gi|) |t|
      eval: dx = du scale:   |scale| b_du + u |du scale|;        dx +=: + u |old + dx|
      dgamma += sum_g t2_g (G atomics of fp32 casts):   u sum_g |t2_g| + G u (|old| + sum_g |t2_g|);   dbeta likewise with t1
THE RELU KINK.  Where |u_ref| <= b_u (and b_u > 0) fp32 and float64 may disagree on the sign of u.  Those elements are left out of the dx and dres
comparisons; in everything summed over them (both halves of red, and through red whatever the chain derives from it) |da| + b_da is ADDED to the bound.  y
needs no exclusion (ReLU is continuous) and neither do dblend_a and docc (they use a, not the mask).  Every set asserts that the kink holds at most 1 % of its
elements (bn_set; measured: none to 3e-6 of them).  Planted exact zeros (x = 0, shift = 0, res = 0: u == 0 and b_u == 0) are NOT kink elements: both kernels
must give y = 0 and du = 0 there.

Every operand sits in a wider buffer (kernel_check.Buf): inputs NaN outside their [.., :C] slice, outputs a canary that must survive; every += output starts
from random values; after each call the inputs are bit-identical.  The dispatch is predicted from the operands (fwd_vec / bwd_vec, geometry, red_slots,
slot_set: mirrors of mrfa_bn_act_fwd / mrfa_bn_act_bwd / pick_rows_per_block) and the slot prediction is asserted from the non-zero blocks of `stats` / `red`.

MEASURED on an MI355X, largest err / bound per family (each test prints its own through report()):
  mrfa_bn_stats             s1 0.021  s2 0.450      (ratio 100, 1024 terms per thread: the variance E[x^2] - m^2 off by 3.3e-4 relative, the sums' bounds allow 1.8)
  finalize, constructed     scale 0.812  shift 0.651  mean 0.954  invstd 0.968  running_mean 0.350  running_var 0.320;  eval: scale 0.165  shift 0.586  invstd 0.133
  forward                   y 0.972 (cells, layouts, grid-stride)  0.947 (groups)  0.393 (odd pool geometry)
  backward, phase 1         red 0.229 / 0.140 (sum du / sum du xhat)  dres 1.000  dblend_a 0.988  docc 0.384
  backward, phase 2         dx 0.994  dgamma 0.927  dbeta 0.968
  the chain                 stats 0.044 / 0.093  finalize 0.045 .. 0.192  y 0.552  red 0.124 / 0.027  dx 0.722  dgamma 0.023  dbeta 0.132
dres, dblend_a, y and dx are one to four roundings on elements of order 1: their worst element comes close to the count, which is why the ratios stand near 1
and stay below it; the sums sit far inside theirs.  A library built with phase 2 ignoring red_all, the running variance left biased and the scalar backward
taking relu'(0) = 1 failed test_backward_slot_counts (1 and 8 slots), test_finalize_on_constructed_statistics, test_exact_zeros_are_on_the_closed_side and
test_chain, and nothing else.
"""
import ctypes
import functools
import types
import zlib

import pytest
import torch

from mrfa_amd import hip
from mrfa_amd.utils.prng import det_uniform
from tests import ref_norm as R
from tests.kernel_check import CANARY, F64, NAN, Buf, check, note, report
from tests.kernel_check import U as U0
from tests.test_token_kernels_gpu import CAP, Library, Spec, f32, steps, unwritten

pytestmark = pytest.mark.gpu

U = U0 * (1 + 2.0 ** -12)                                 # the second-order terms of the counts (docstring)
D = 2.0 ** -53
E_SQRT, E_DIV = 6 * U, 5 * U
SLOTS = hip.STATS_SLOTS
CH = 64                                                    # channels per workgroup (csrc/norm.hip)
EPS = f32(1e-5)
TAG = "norm"
MODES = ("plain", "res", "pool", "blend")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ mirrors of the dispatch
def pick_rows_per_block(rows, chunks, C):
    target = min(max(rows * C * 4 // 65536, 256), 1024)
    want = cdiv(target, chunks)
    return min(max(cdiv(rows, want), 64), 4096)


def red_slots(row_blocks):
    return SLOTS if row_blocks >= 64 else (8 if row_blocks >= 16 else 1)


def geometry(rows, C, G=1):
    """(channel chunks, rows per block, row blocks per statistic group) of mrfa_bn_stats (G = 1) and mrfa_bn_act_bwd"""
    chunks = cdiv(C, CH)
    rpb = pick_rows_per_block(rows, chunks, C)
    return chunks, rpb, cdiv(rows // G, rpb)


def slot_set(chunks, row_blocks, slots):
    return sorted({(by + bx) % slots for by in range(row_blocks) for bx in range(chunks)})


def filled(blocks):
    """[.., SLOTS, 2C] -> per leading index the sorted list of slot blocks that hold a non-zero"""
    nz = (blocks != 0).any(-1)
    return [sorted(torch.nonzero(row).flatten().tolist()) for row in nz.reshape(-1, SLOTS)]


def al(b):
    return b is None or b.ptr % 16 == 0


def ld4(b):
    return b is None or b.ld % 4 == 0


def fwd_vec(S, bx, by, bsc, bsh, br):
    return S.mode in ("plain", "res") and S.C % 4 == 0 and all(al(b) for b in (bx, by, bsc, bsh, br)) and all(ld4(b) for b in (bx, by, br))


def bwd_vec(S, phase, bx, bdy, bsc, bsh, bm, bi, bg, bdx, br, bdr, ba, bda):
    return (S.C % 4 == 0 and all(al(b) for b in (bx, bdy, bsc, bsh, bm, bi, bg, br, bdr, ba, bda)) and all(ld4(b) for b in (bx, bdy, br, bdr, ba, bda))
            and (phase == 1 or (ld4(bdx) and al(bdx))))


# ------------------------------------------------------------------------------------------------------------------ bounds
def fin_bounds(r, count, gamma, momentum, train=True, d_t1=0.0, d_t2=0.0, eps=EPS):
    """bounds of the docstring on finalize_ref's outputs (all [G][C])"""
    gam = gamma.to(F64).abs()
    inv = r["invstd"]
    if train:
        m, var = r["m"], r["var"]
        d_m = d_t1 / count + 4 * D * m.abs()
        d_var = d_t2 / count + 2 * m.abs() * d_m + 4 * D * (r["q"].abs() + m * m)
        b_mean = d_m + U * m.abs()
        b_inv = inv * (0.5 * d_var / (var + eps) + 4 * D) + U * inv
    else:
        b_mean = torch.zeros_like(inv)
        b_inv = inv * (0.5 * U + E_SQRT + E_DIV)
    b_scale = gam * b_inv + U * r["scale"].abs()
    b_shift = b_mean * r["scale"].abs() + r["mean"].abs() * b_scale + U * r["ms"].abs() + U * r["shift"].abs()
    b = dict(mean=b_mean, invstd=b_inv, scale=b_scale, shift=b_shift)
    if train and "rm" in r:
        b_unb = (d_var + 4 * D * var) * (count / (count - 1) if count > 1 else 1.0) + U * r["unb"]
        om = abs(1.0 - momentum)
        for key, prev, stat, b_s in (("rm", r["rm_prev"], r["mean"], b_mean), ("rv", r["rv_prev"], r["unb"], b_unb)):
            acc = torch.zeros_like(prev[0])
            for g in range(prev.shape[0]):
                acc = om * acc + momentum * b_s[g] + 3 * U * (om * prev[g].abs() + momentum * stat[g].abs()) + U * r[key][g].abs()
            b[key] = acc.view(1, -1)
    return b


def fwd_bounds(f, pool, d_sc=0.0, d_sh=0.0):
    b_u = U * (f["xs"].abs() + f["v0"].abs() + (f["u"].abs() if f["u"] is not f["v0"] else 0.0)) + f["x"].abs() * d_sc + d_sh
    b_v = b_u
    if pool:
        b_v = 0.25 * (R.pool_sum(b_u) + 3 * U * f["S_pool"])
    b_y = b_v
    if "A" in f:
        o1 = 1.0 - f["o"]
        b_y = o1.abs() * b_v + 2 * U * (f["v"] * o1).abs() + U * (f["A"] * f["o"]).abs() + U * f["y"].abs()
    return dict(u=b_u, y=b_y)


def bwd1_bounds(S, f, r, b_u, k, d_mean=None, d_invstd=None):
    """k: fp32 terms per thread.  dres / dA / docc bounds hold for the random old values of the set"""
    G, Cc, N = S.G, S.C, S.N
    kink = (f["u"].abs() <= b_u) & (b_u > 0) if S.relu else torch.zeros_like(f["u"], dtype=torch.bool)
    b = dict(kink=kink)
    b_da = torch.zeros_like(r["da"])
    if "A" in f:
        b["dA"] = U * r["dA"].abs() + U * (S.dA0.view_as(r["dA"]).double() + r["dA"]).abs()
        b["docc"] = ((r["da0"].abs() * b_u).sum(-1, keepdim=True) + 2 * U * r["docc_terms"].abs().sum(-1, keepdim=True)
                     + (Cc + cdiv(Cc, CH)) * U * (r["docc_terms"].abs().sum(-1, keepdim=True) + S.docc0.view_as(r["docc"]).double().abs()))
        b_da = 2 * U * r["da"].abs()
    flip = kink * (r["da"].abs() + b_da)                    # what a kink element may add to a sum, on top of b_du
    b_du = b_da + flip
    b["du"] = b_da
    if S.mode == "res":
        b["dres"] = b_da + U * (S.dres0.view_as(r["du"]).double() + r["du"]).abs()
    xh = r["xhat"].abs()
    ex = 2 * U * xh
    if d_mean is not None:
        ex = ex + R.per_sample(d_mean * S.invstd.double().abs(), N) + r["d"].abs() * R.per_sample(d_invstd, N)
    b["ex"] = ex
    sum_du = r["S1"] + R.group_sum(kink * r["da"].abs(), G)
    sum_dx = r["S2"] + R.group_sum(kink * (r["da"] * r["xhat"]).abs(), G)
    fp64 = (S.row_blocks + SLOTS) * D
    b["red1"] = R.group_sum(b_du, G) + ((k - 1) * U + fp64) * sum_du
    b["red2"] = R.group_sum(xh * b_du + (r["du"].abs() + flip) * ex + U * (r["du"] * r["xhat"]).abs(), G) + ((k - 1) * U + fp64) * sum_dx
    return b


def bwd2_expect(S, red, red_abs, overwrite, red_world=1, b1=None, d_red1=0.0, d_red2=0.0, b_inv=None, wrong=""):
    """reference and bounds of phase 2 on the slot-summed red [G][2C] (red_abs: the sum of the slots' absolute values)"""
    G, Cc, N = S.G, S.C, S.N
    f, r1 = S.f, S.b1
    b1 = b1 or S.bounds1(1)
    r = R.bwd2_ref(f, r1, red, S.gamma, getattr(S, "ref_invstd", S.invstd), S.train, G, red_world, wrong=wrong)
    old = 0.0 if overwrite else S.dx0.view_as(r["dx"]).double()
    ref = dict(dx=old + r["dx"], dgamma=(S.dg0.double() + r["dgamma"]).view(1, -1), dbeta=(S.db0.double() + r["dbeta"]).view(1, -1))
    b_du, ex = b1["du"], b1["ex"]
    if S.train:
        cnt = float(S.rows // G * max(red_world, 1))
        fp64 = (S.row_blocks + SLOTS) * D
        b_k1 = R.per_sample((d_red1 + fp64 * red_abs[:, :Cc]) / cnt, N) + U * r["k1"].abs()
        b_k2 = R.per_sample((d_red2 + fp64 * red_abs[:, Cc:]) / cnt, N) + U * r["k2"].abs()
        gi, xh = r["gi"].abs(), r1["xhat"].abs()
        b_gi = U * gi + (R.per_sample(S.gamma.double().abs() * b_inv, N) if b_inv is not None else 0.0)
        b_dx = (gi * (b_du + b_k1 + ex * r["k2"].abs() + xh * b_k2 + U * (xh * r["k2"].abs()) + U * r["t0"].abs() + U * r["t"].abs())
                + (b_gi + U * gi) * r["t"].abs())
    else:
        b_dx = f["sc"].abs() * b_du + U * r["dx"].abs()
    if not overwrite:
        b_dx = b_dx + U * ref["dx"].abs()
    tiny = torch.full((1, Cc), 1e-300, dtype=F64)
    sum_g = lambda d: d.sum(0) if torch.is_tensor(d) else d
    bound = dict(dx=b_dx, dgamma=(U * r["T2"] + G * U * (S.dg0.double().abs() + r["T2"]) + sum_g(d_red2)).view(1, -1) + tiny,
                 dbeta=(U * r["T1"] + G * U * (S.db0.double().abs() + r["T1"]) + sum_g(d_red1)).view(1, -1) + tiny)
    return ref, bound


# ------------------------------------------------------------------------------------------------------------------ input sets
def gen(name, shape, lo, hi):
    """det_uniform; a seeded torch generator where the tensor is large (det_uniform hashes every element)"""
    n = 1
    for s in shape:
        n *= s
    if n <= 1 << 17:
        return det_uniform(name, shape, lo, hi)
    return torch.rand(shape, generator=torch.Generator().manual_seed(zlib.crc32(name.encode()))) * (hi - lo) + lo


@functools.lru_cache(maxsize=None)
def bn_set(N, H, W, C, mode="plain", G=1, relu=1, train=1, zeros=False, fwd_only=False):
    """one input set with its float64 reference and bounds (computed once, shared, never modified).  x ~ U(-2, 2), gamma ~ U(0.5, 1.5), beta ~ U(-0.5, 0.5) (so that no channel has u < 0 everywhere); train:
    scale / shift / mean / invstd are the float64 finalize of each group's statistics rounded to fp32; eval: of running statistics U(-0.5, 0.5) / U(0.5, 2)
    (mean = running_mean).
    zeros: shift = 0 and every 11th x (and res) exactly 0, so u == 0 there."""
    name = f"norm/{N}.{H}.{W}.{C}.{mode}.{G}.{relu}.{train}.{int(zeros)}"
    nomean, train = train < 0, int(train > 0)              # train = -1: eval mode with mean / invstd / gamma NULL (xhat = 0: red[C + c] and dgamma stay as they were)
    rows, pool = N * H * W, mode == "pool"
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    orow = N * Ho * Wo
    S = types.SimpleNamespace(N=N, H=H, W=W, C=C, mode=mode, G=G, relu=relu, train=train, rows=rows, orow=orow, pool=pool, zeros=zeros, nomean=nomean)
    S.chunks, S.rpb, S.row_blocks = geometry(rows, C, G)
    S.x = gen(name + "/x", (rows, C), -2, 2)
    S.gamma, S.beta = gen(name + "/g", (C,), 0.5, 1.5), gen(name + "/b", (C,), -0.5, 0.5)
    if zeros:
        S.x.view(-1)[::11] = 0.0
    if train:
        xg = S.x.double().view(G, rows // G, C)
        fin = R.finalize_ref(torch.cat([xg.sum(1), (xg * xg).sum(1)], 1), rows // G, S.gamma, S.beta, None, None, 0.0, EPS)
    else:
        assert G == 1
        S.rmean, S.rvar = gen(name + "/rm", (C,), -0.5, 0.5), gen(name + "/rv", (C,), 0.5, 2)
        fin = R.finalize_ref(None, 0, S.gamma, S.beta, S.rmean, S.rvar, 0.0, EPS, train=False)
    S.mean, S.invstd, S.sc, S.sh = [fin[k].float().contiguous() for k in ("mean", "invstd", "scale", "shift")]
    if zeros:
        S.sh.zero_()
    S.res = S.A = S.occ = None
    if mode == "res":
        S.res = gen(name + "/res", (rows, C), -1, 1)
        if zeros:
            S.res.view(-1)[::11] = 0.0
    if mode == "blend":
        S.A, S.occ = gen(name + "/A", (orow, C), -1, 1), gen(name + "/occ", (orow, 1), 0, 1)
    v4 = lambda t, h=H, w=W: None if t is None else t.view(N, h, w, -1)
    S.f = f = R.fwd_ref(v4(S.x), S.sc, S.sh, relu, pool, v4(S.res), v4(S.A), v4(S.occ))
    S.fb = fwd_bounds(f, pool)
    S.y_ref, S.y_bound = f["y"].reshape(orow, C), S.fb["y"].reshape(orow, C)
    if fwd_only:
        return S
    S.dy = gen(name + "/dy", (orow, C), -1, 1)
    S.dx0, S.dg0, S.db0 = gen(name + "/dx0", (rows, C), -1, 1), gen(name + "/dg0", (C,), -1, 1), gen(name + "/db0", (C,), -1, 1)
    S.dres0 = gen(name + "/dres0", (rows, C), -1, 1) if mode == "res" else None
    S.dA0, S.docc0 = (gen(name + "/dA0", (orow, C), -1, 1), gen(name + "/docc0", (orow, 1), -1, 1)) if mode == "blend" else (None, None)
    S.b1 = R.bwd1_ref(f, v4(S.dy, Ho, Wo), None if nomean else S.mean, None if nomean else S.invstd, relu, pool, G)
    cache = {}

    def bounds1(k):
        if k not in cache:
            cache[k] = bwd1_bounds(S, f, S.b1, S.fb["u"], k)
        return cache[k]
    S.bounds1 = bounds1
    S.kink_share = bounds1(1)["kink"].double().mean().item()
    assert S.kink_share <= 0.01, (name, S.kink_share)
    if zeros:
        z = (f["u"] == 0) & (S.fb["u"] == 0)
        assert z.double().mean().item() > 0.05 and not (z & bounds1(1)["kink"]).any(), name
        S.zero_share = z.double().mean().item()
    return S


# ------------------------------------------------------------------------------------------------------------------ drivers
def maker(be, lay):
    def mk(vals, key, fill, dtype=torch.float32):
        if vals is None:
            return None
        return Buf(vals, 1, lay.get("ld" + key, vals.shape[1] + 4), fill, lead=lay.get("lead" + key, 4), dev=be.dev, dtype=dtype)
    return mk


def ptr(b):
    return b.ptr if b is not None else None


def ldof(b):
    return b.ld if b is not None else 0


def run_stats(be, x, test, what="stats"):
    """mrfa_bn_stats on x [rows][C] (leading dimension C + 3, base offset by 4 bytes): the slot-summed statistics in float64, the predicted slot blocks filled"""
    rows, C = x.shape
    chunks, rpb, rb = geometry(rows, C)
    bx = Buf(x, 1, C + 3, NAN, lead=1, dev=be.dev)
    bst = Buf(torch.zeros(1, SLOTS * 2 * C, dtype=F64), 1, SLOTS * 2 * C + 2, CANARY, lead=2, dev=be.dev, dtype=F64)
    rc = be.call("mrfa_bn_stats", bx.ptr, bx.ld, rows, C, bst.ptr)
    assert rc == 0, be.error()
    st = bst.get().view(SLOTS, 2 * C)
    if not be.spec:
        want = slot_set(chunks, rb, SLOTS)
        assert filled(st) == [want], (filled(st), want)
    r = R.stats_ref(x)
    k = cdiv(min(rpb, rows), 4)
    fp64 = (rb + SLOTS) * D
    tot = st.sum(0)
    b1, b2 = ((k - 1) * U + fp64) * r["A1"] + 1e-300, (k * U + fp64) * r["s2"] + 1e-300
    note(test, f"{what} s1", check(tot[:C], r["s1"], b1, f"{what} sum x {rows} x {C}"))
    note(test, f"{what} s2", check(tot[C:], r["s2"], b2, f"{what} sum x^2 {rows} x {C}"))
    assert bx.untouched(), "an input changed"
    return st, r, b1, b2, (rpb, rb)


def spread(total, nslots, seed):
    """[.., 2C] float64 sums -> [.., SLOTS, 2C]: random shares in the first nslots slot blocks that add up to the total (to float64 rounding), the rest 0"""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(total.shape[:-1] + (nslots, total.shape[-1]), generator=g, dtype=F64) + 0.1
    w = w / w.sum(-2, keepdim=True)
    out = torch.zeros(total.shape[:-1] + (SLOTS, total.shape[-1]), dtype=F64)
    out[..., :nslots, :] = w * total.unsqueeze(-2)
    return out


def run_finalize(be, test, stats, count, gamma, beta, rmean, rvar, momentum, eps=EPS, train=True, grouped=False, null=(), d_t=(0.0, 0.0), ref_stats=None,
                 what="finalize"):
    """stats [G][SLOTS][2C] float64 (None in eval mode); rmean / rvar None: NULL running statistics.  Returns the kernel's outputs and the reference"""
    C = gamma.numel()
    G = stats.shape[0] if train else 1
    mk = maker(be, {})
    bst = mk(stats.reshape(1, -1), "st", NAN, F64) if train else None
    bg, bb = Buf(gamma.view(1, C), 1, C + 1, NAN, lead=1, dev=be.dev), Buf(beta.view(1, C), 1, C + 3, NAN, lead=3, dev=be.dev)
    brm = Buf(rmean.view(1, C), 1, C + 2, CANARY, lead=1, dev=be.dev) if rmean is not None else None
    brv = Buf(rvar.view(1, C), 1, C + 1, CANARY, lead=2, dev=be.dev) if rvar is not None else None
    outs = {k: Buf(unwritten((1, G * C)), 1, G * C + 1 + i, CANARY, lead=1 + i, dev=be.dev) for i, k in enumerate(("scale", "shift", "mean", "invstd"))}
    args = [ptr(bst), count, bg.ptr, bb.ptr, ptr(brm), ptr(brv), momentum, eps, C]
    tail = [outs["scale"].ptr, outs["shift"].ptr, None if "mean" in null else outs["mean"].ptr, None if "invstd" in null else outs["invstd"].ptr]
    if grouped:
        rc = be.call("mrfa_bn_finalize_groups", *args, G, *tail)
    else:
        assert G == 1
        rc = be.call("mrfa_bn_finalize", *args, int(train), *tail)
    assert rc == 0, be.error()
    ssum = (ref_stats if ref_stats is not None else stats.sum(1)) if train else None
    r = R.finalize_ref(ssum, count, gamma, beta, rmean, rvar, momentum, eps, train)
    b = fin_bounds(r, count, gamma, momentum, train, d_t[0], d_t[1], eps)
    got = {}
    for k, buf in outs.items():
        if k in null:
            assert buf.untouched()
            continue
        got[k] = buf.get().view(G, C)
        note(test, f"{what} {k}", check(got[k], r[k].expand(G, C), b[k].expand(G, C), f"{what} {k} C={C} G={G} count={count}"))
    if rmean is not None:
        if train:
            for key, buf in (("rm", brm), ("rv", brv)):
                note(test, f"{what} {key}", check(buf.get(), r[key][-1:].clone(), b[key], f"{what} running {key} C={C} G={G} momentum={momentum}"))
        else:
            assert brm.untouched() and brv.untouched(), "eval mode changed the running statistics"
    assert bg.untouched() and bb.untouched() and (bst is None or bst.untouched()), "an input changed"
    return got, r, b


def fwd_rows(rows):
    """the first and last 64 rows and every 37th between"""
    return torch.cat([torch.arange(64), torch.arange(64, rows - 64, 37), torch.arange(rows - 64, rows)])


def run_fwd(be, S, test, lay=None, expect=None, sample=False, sc=None, sh=None, ref=None, bound=None, what="y"):
    """mrfa_bn_act_fwd; lay: leading dimensions / leads that differ from (C + 4, 4 floats).  Returns y's values"""
    lay = lay or {}
    mk = maker(be, lay)
    C = S.C
    bx, br, ba, bo = mk(S.x, "x", NAN), mk(S.res, "r", NAN), mk(S.A, "a", NAN), mk(S.occ, "o", NAN)
    bsc, bsh = mk((S.sc if sc is None else sc).reshape(1, -1), "sc", NAN), mk((S.sh if sh is None else sh).reshape(1, -1), "sh", NAN)
    by = mk(unwritten((S.orow, C)), "y", CANARY)
    vec = fwd_vec(S, bx, by, bsc, bsh, br)
    want = (S.mode in ("plain", "res") and C % 4 == 0 and not lay) if expect is None else expect == "float4"
    assert vec == want, (test, lay, vec, want)
    p = hip.BnActParams(x=bx.ptr, ldx=bx.ld, N=S.N, H=S.H, W=S.W, C=C, scale=bsc.ptr, shift=bsh.ptr, relu=S.relu, pool=int(S.pool), blend_a=ptr(ba), lda=ldof(ba),
                        occ=ptr(bo), ldo=ldof(bo), y=by.ptr, ldy=by.ld, res=ptr(br), ldr=ldof(br), groups=S.G)
    rc = be.call("mrfa_bn_act_fwd", ctypes.byref(p))
    assert rc == 0, be.error()
    y = by.get()
    ref, bound = S.y_ref if ref is None else ref, S.y_bound if bound is None else bound
    path = "float4" if vec else "scalar"
    if sample:
        idx = fwd_rows(S.orow)
        note(test, f"{what}[{path}]", check(y[idx], ref[idx], bound[idx], f"{what} [{path}] {test}"))
    else:
        note(test, f"{what}[{path}]", check(y, ref, bound, f"{what} [{path}] {test}"))
    if S.zeros and S.relu and S.mode in ("plain", "res"):
        assert (y[(S.f["u"] == 0).reshape(-1, C)] == 0).all(), "y at u == 0"
    assert all(b is None or b.untouched() for b in (bx, br, ba, bo, bsc, bsh)), "an input changed"
    return y, path


def run_bwd(be, S, test, lay=None, expect=None, overwrite=0, null=(), red_all=0, red_world=1, keep=None, expect2=None):
    """phase 1, its outputs and the slot blocks it filled; phase 2 on the red it left (red_all / red_world: on a red the test spreads itself from those sums,
    as a bst_* epilogue / an all-reduce over the ranks would leave it).  null: outputs passed as NULL (dres, dblend_a, docc, dgamma, dbeta)"""
    lay = lay or {}
    mk = maker(be, lay)
    C, G, N = S.C, S.G, S.N
    flat = lambda t: t.reshape(-1, t.shape[-1])
    bx, br, ba, bo, bdy = mk(S.x, "x", NAN), mk(S.res, "r", NAN), mk(S.A, "a", NAN), mk(S.occ, "o", NAN), mk(S.dy, "dy", NAN)
    bsc, bsh = mk(S.sc.reshape(1, -1), "sc", NAN), mk(S.sh.reshape(1, -1), "sh", NAN)
    bm, bi, bg = [mk(t.reshape(1, -1), k, NAN) if not S.nomean else None for t, k in ((S.mean, "m"), (S.invstd, "i"), (S.gamma, "g"))]
    bdr = mk(S.dres0, "dr", CANARY) if "dres" not in null else None
    bda = mk(S.dA0, "da", CANARY) if "dblend_a" not in null else None
    bdo = mk(S.docc0, "do", CANARY) if "docc" not in null else None
    bdx = mk(unwritten((S.rows, C)) if overwrite else S.dx0, "dx", CANARY)
    bdg = mk(S.dg0.view(1, C), "dg", CANARY)
    bdb = mk(S.db0.view(1, C), "db", CANARY)
    bred = mk(torch.zeros(1, G * SLOTS * 2 * C, dtype=F64), "red", CANARY, F64)
    vecs = [bwd_vec(S, ph, bx, bdy, bsc, bsh, bm, bi, bg, bdx, br, bdr, ba, bda) for ph in (1, 2)]
    want = (C % 4 == 0 and not lay) if expect is None else expect == "float4"
    assert vecs[1] == want and (vecs[0] == want or "lddx" in lay or "leaddx" in lay), (test, lay, vecs, want)
    paths = ["float4" if v else "scalar" for v in vecs]
    local_pg = red_world > 1
    P = dict(x=bx.ptr, ldx=bx.ld, N=N, H=S.H, W=S.W, C=C, scale=bsc.ptr, shift=bsh.ptr, relu=S.relu, pool=int(S.pool), mean=ptr(bm), invstd=ptr(bi), gamma=ptr(bg),
             dy=bdy.ptr, lddy=bdy.ld, blend_a=ptr(ba), lda=ldof(ba), occ=ptr(bo), ldo=ldof(bo), dblend_a=ptr(bda), ldda=ldof(bda), docc=ptr(bdo), lddo=ldof(bdo),
             red=bred.ptr, dx=bdx.ptr, lddx=bdx.ld, dgamma=None if "dgamma" in null or local_pg else bdg.ptr, dbeta=None if "dbeta" in null or local_pg else bdb.ptr,
             train=S.train, dx_overwrite=overwrite, res=ptr(br), ldr=ldof(br), dres=ptr(bdr), lddr=ldof(bdr), sync=None, red_world=red_world, red_all=red_all,
             groups=G)
    inputs = [b for b in (bx, br, ba, bo, bdy, bsc, bsh, bm, bi, bg) if b is not None]
    # ---- phase 1
    p = hip.BnBwdParams(phase=1, **P)
    rc = be.call("mrfa_bn_act_bwd", ctypes.byref(p))
    assert rc == 0, be.error()
    k = cdiv(min(S.rpb, S.rows // G), 16 if vecs[0] else 4)
    b1 = S.bounds1(k)
    r1 = S.b1
    red = bred.get().view(G, SLOTS, 2 * C)
    nslots = red_slots(S.row_blocks)
    if not be.spec:
        want_slots = slot_set(S.chunks, S.row_blocks, nslots)
        want_all = [want_slots if r1["S1"][g].any() else [] for g in range(G)]      # (C = 1 with gamma < -beta: u < 0 everywhere, every du is 0)
        assert filled(red) == want_all, (test, filled(red), want_all)
    rsum = red.sum(1)
    tag = f"[{paths[0]} {S.mode}]"
    note(test, f"red1{tag}", check(rsum[:, :C], r1["s1"], b1["red1"] + 1e-300, f"red sum du {tag} {test}"))
    note(test, f"red2{tag}", check(rsum[:, C:], r1["s2"], b1["red2"] + 1e-300, f"red sum du xhat {tag} {test}"))
    live = ~b1["kink"].reshape(-1, C)
    if bdr is not None:
        note(test, f"dres{tag}", check(bdr.get(), S.dres0.double() + flat(r1["du"]), flat(b1["dres"]), f"dres {tag} {test}", mask=live))
        if S.zeros and S.relu:
            z = (S.f["u"] == 0).reshape(-1, C)
            assert torch.equal(bdr.get()[z], S.dres0[z]), "du at u == 0"
    if bda is not None:
        note(test, f"dblend_a{tag}", check(bda.get(), S.dA0.double() + flat(r1["dA"]), flat(b1["dA"]), f"dblend_a {tag} {test}"))
    if bdo is not None:
        note(test, f"docc{tag}", check(bdo.get(), S.docc0.double() + flat(r1["docc"]), flat(b1["docc"]), f"docc {tag} {test}"))
    assert bdx.untouched() and bdg.untouched() and bdb.untouched(), "phase 1 wrote a phase-2 output"
    assert all(b.untouched() for b in inputs), "phase 1 changed an input"
    # ---- the red that phase 2 is given
    if local_pg:                                            # the header: the LOCAL sums, before the exchange
        rc = be.call("mrfa_bn_param_grad_groups" if G > 1 else "mrfa_bn_param_grad", bred.ptr, C, *([G] if G > 1 else []),
                     None if "dgamma" in null else bdg.ptr, None if "dbeta" in null else bdb.ptr)
        assert rc == 0, be.error()
    local = rsum
    if red_all or red_world > 1:
        others = torch.rand(rsum.shape, generator=torch.Generator().manual_seed(7), dtype=F64) * 2 - 1
        total = rsum + (others * r1["S1"].repeat(1, 2) * (red_world - 1) if red_world > 1 else 0.0)
        red2 = spread(total, SLOTS if red_all else nslots, 11)
        bred2 = mk(red2.reshape(1, -1), "red", CANARY, F64)
        p_red = bred2
    else:
        red2, p_red = red, bred
    expect2 = expect2 or bwd2_expect
    ref, bound = expect2(S, red2.sum(1), red2.abs().sum(1), overwrite, red_world, b1)
    if local_pg:                                            # dgamma / dbeta came from the local red
        lref, lbound = expect2(S, local, red.abs().sum(1), overwrite, 1, b1)
        ref.update(dgamma=lref["dgamma"], dbeta=lref["dbeta"])
        bound.update(dgamma=lbound["dgamma"], dbeta=lbound["dbeta"])
    # ---- phase 2
    side = [b.bits() for b in (bdr, bda, bdo) if b is not None]
    red_bits = p_red.bits()
    P["red"] = p_red.ptr
    p = hip.BnBwdParams(phase=2, **P)
    rc = be.call("mrfa_bn_act_bwd", ctypes.byref(p))
    assert rc == 0, be.error()
    tag = f"[{paths[1]} {S.mode}{' train' if S.train else ' eval'}{' =' if overwrite else ' +='}]"
    dx = bdx.get()
    note(test, f"dx{tag}", check(dx, flat(ref["dx"]), flat(bound["dx"]), f"dx {tag} {test}", mask=live))
    if S.zeros and S.relu and not S.train and overwrite:
        assert (dx[(S.f["u"] == 0).reshape(-1, C)] == 0).all(), "dx at u == 0"
    for key, buf in (("dgamma", bdg), ("dbeta", bdb)):
        if key in null:
            assert buf.untouched(), f"{key} NULL but written"
        else:
            note(test, f"{key}{tag}", check(buf.get(), ref[key], bound[key], f"{key} {tag} {test}"))
    assert torch.equal(p_red.bits(), red_bits), "phase 2 changed red"
    assert all(torch.equal(b.bits(), s) for b, s in zip([b for b in (bdr, bda, bdo) if b is not None], side)), "phase 2 changed a phase-1 output"
    assert all(b.untouched() for b in inputs), "phase 2 changed an input"
    if keep is not None:
        keep.update(dx=dx, dres=bdr.get() if bdr is not None else None, red=rsum, dgamma=bdg.get(), dbeta=bdb.get())
    return paths


# ------------------------------------------------------------------------------------------------------------------ statistics
STAT_SHAPES = [(960, 64), (1024, 64), (4096, 64), (4096, 132), (1, 1), (3, 3), (65, 37), (97, 65), (1000, 4), (300, 257)]
STAT_RATIOS = (0, 10, 100)
BIG_ROWS = 1048400                                         # C = 4: 256 row blocks of 4096 rows, 1024 terms per thread


def noise_set(rows, C, ratio):
    g = torch.Generator().manual_seed(rows + 1000 * ratio + C)
    return torch.randn(rows, C, generator=g) + float(ratio)


@pytest.mark.parametrize("rows,C", STAT_SHAPES)
def test_stats_every_geometry(rows, C):
    """1 .. 64 row blocks, 1 .. 5 channel chunks with and without a tail, a single row; the filled slot blocks are (row block + chunk) % 32"""
    test = f"stats {rows}x{C}"
    run_stats(Library(), gen(f"norm/stats/{rows}.{C}", (rows, C), -2, 2), test)
    report(test, TAG)


@pytest.mark.parametrize("ratio", STAT_RATIOS)
@pytest.mark.parametrize("rows", [4000, BIG_ROWS])
def test_stats_accuracy_with_a_large_mean(rows, ratio):
    """x = ratio + noise (std 1) at the 64-row floor (16 terms per thread) and at rows_per_block = 4096 (1024 terms): the sums against float64 within the
    derived bound, and -- printed, not asserted: the bound on the sums is what the kernel answers for -- the relative error of the variance E[x^2] - m^2
    formed from them"""
    test = f"stats accuracy rows {rows} ratio {ratio}"
    x = noise_set(rows, 4, ratio)
    assert geometry(rows, 4)[1] == (4096 if rows == BIG_ROWS else 64)
    st, r, b1, b2, _ = run_stats(Library(), x, test)
    tot = st.sum(0)
    var = tot[4:] / rows - (tot[:4] / rows) ** 2
    ref = r["s2"] / rows - (r["s1"] / rows) ** 2
    print(f"[{TAG}] {test}: variance relative error {((var - ref).abs() / ref).max().item():.3e}, allowed by the sums' bounds "
          f"{((b2 / rows + 2 * (r['s1'] / rows).abs() * b1 / rows) / ref).max().item():.3e}")
    report(test, TAG)


# ------------------------------------------------------------------------------------------------------------------ finalize
FIN_C = (1, 255, 256, 257)


def fin_set(C, G, count, seed=0):
    """constructed float64 statistics over all 32 slots: mean U(-3, 3), E[x^2] = mean^2 + U(0.1, 2)"""
    g = torch.Generator().manual_seed(C + 10 * G + seed)
    m = torch.rand(G, C, generator=g, dtype=F64) * 6 - 3
    q = m * m + torch.rand(G, C, generator=g, dtype=F64) * 1.9 + 0.1
    st = spread(torch.cat([m, q], 1) * count, SLOTS, C + G)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) * 2 - 1
    rm, rv = torch.rand(C, generator=g) - 0.5, torch.rand(C, generator=g) + 0.5
    return st, gamma, beta, rm, rv


FIN_CASES = [(C, 1, 4096, 0.1) for C in FIN_C] + [(64, 1, 1, 0.1), (64, 1, 4096, 0.0), (64, 1, 4096, 1.0), (37, 2, 72, 0.1), (257, 3, 108, 0.25), (64, 3, 1, 1.0)]


def finalize_cases(be, C, G, count, momentum, test):
    st, gamma, beta, rm, rv = fin_set(C, G, count)
    mom = f32(momentum)
    if G == 1:
        run_finalize(be, test, st, count, gamma, beta, rm, rv, mom)
        run_finalize(be, test, st, count, gamma, beta, None, None, mom, null=("mean", "invstd"), what="finalize(null)")
        run_finalize(be, test, None, count, gamma, beta, rm, rv, mom, train=False, what="finalize(eval)")
    run_finalize(be, test, st, count, gamma, beta, rm, rv, mom, grouped=True, what="finalize_groups")
    run_finalize(be, test, st, count, gamma, beta, None, None, mom, grouped=True, what="finalize_groups(null running)")


def clamp_case(be, test):
    """t2 / count < m^2 in every channel: the variance is clamped to 0, invstd = 1 / sqrt(eps)"""
    C, count = 37, 100
    m = torch.linspace(-3, 3, C, dtype=F64).view(1, C)
    st = spread(torch.cat([m, m * m - 0.1], 1) * count, SLOTS, 5)
    _, gamma, beta, rm, rv = fin_set(C, 1, count)
    got, r, _ = run_finalize(be, test, st, count, gamma, beta, rm, rv, f32(0.1), what="finalize(clamp)")
    assert (r["raw"] < 0).all() and (r["var"] == 0).all()
    assert (got["invstd"] == f32(1.0 / float(torch.tensor(EPS, dtype=F64).sqrt()))).all()


@pytest.mark.parametrize("C,G,count,momentum", FIN_CASES)
def test_finalize_on_constructed_statistics(C, G, count, momentum):
    """C around the 256-thread block, count = 1 (no unbiased correction), momentum 0 and 1, eval mode, NULL running statistics and NULL mean / invstd outputs,
    the grouped entry point with 1 .. 3 groups"""
    test = f"finalize C{C} G{G} n{count} m{momentum}"
    finalize_cases(Library(), C, G, count, momentum, test)
    report(test, TAG)


def test_finalize_clamps_a_negative_variance():
    clamp_case(Library(), "finalize clamp")
    report("finalize clamp", TAG)


# ------------------------------------------------------------------------------------------------------------------ forward
FWD_C = (64, 37)                                           # float4 (plain / residual only) and scalar
FWD_CELLS = [(C, mode, relu, G) for C in FWD_C for mode in MODES for relu in (0, 1) for G in (1, 3)]
SCALAR_C = (1, 3, 37, 65)
FWD_ROUTES = ["ldx", "ldy", "ldr", "leadx", "leady", "leadr", "leadsc", "leadsh"]


def route(key, C):
    """a layout that makes `key` the one operand that is not 16-byte aligned / whose leading dimension is not a multiple of 4"""
    return {key: (C + 5 if key.startswith("ld") else 1)}


@pytest.mark.parametrize("C,mode,relu,G", FWD_CELLS)
def test_forward_every_cell(C, mode, relu, G):
    """N = 6, 6 x 6 pixels (72 rows per group of 3: no multiple of the 64-row block)"""
    test = f"fwd C{C} {mode} relu{relu} G{G}"
    run_fwd(Library(), bn_set(6, 6, 6, C, mode, G, relu), test)
    report(test, TAG)


@pytest.mark.parametrize("C", SCALAR_C)
def test_forward_scalar_by_channel_count(C):
    test = f"fwd scalar C{C}"
    for mode in MODES:
        run_fwd(Library(), bn_set(2, 4, 6, C, mode), test, expect="scalar")
    report(test, TAG)


@pytest.mark.parametrize("key", FWD_ROUTES)
def test_forward_scalar_by_layout(key):
    """C = 64: one leading dimension not a multiple of 4, or one base pointer offset by 4 bytes, sends the call to the scalar kernel"""
    test = f"fwd scalar by {key}"
    run_fwd(Library(), bn_set(2, 4, 6, 64, "res"), test, lay=route(key, 64), expect="scalar")
    report(test, TAG)


@pytest.mark.parametrize("H,W", [(2, 6), (6, 2)])
def test_pool_geometry(H, W):
    test = f"pool {H}x{W}"
    for C in (64, 37):
        S = bn_set(3, H, W, C, "pool")
        run_fwd(Library(), S, test)
        run_bwd(Library(), S, test)
    report(test, TAG)


@pytest.mark.parametrize("rows,C", [(8200, 512), (8200, 129)])
def test_forward_grid_stride_second_trip(rows, C):
    """just over CAP x 256 work items (float4: C / 4 per row): the busiest thread makes a second trip.  Compared: the first and last 64 rows, every 37th between"""
    test = f"fwd grid-stride {rows}x{C}"
    assert steps(rows * C // (4 if C % 4 == 0 else 1)) == 2 and CAP == 4096
    run_fwd(Library(), bn_set(1, 1, rows, C, "plain", fwd_only=True), test, sample=True)
    report(test, TAG)


# ------------------------------------------------------------------------------------------------------------------ backward
BWD_CELLS = [(C, mode, train) for C in FWD_C for mode in MODES for train in (1, 0)]
NULLS = {"plain": (), "res": ("dres",), "pool": (), "blend": ("dblend_a", "docc")}


def bwd_cell(be, C, mode, train, test):
    S = bn_set(6, 6, 6, C, mode, 1, 1, train)
    for overwrite in (0, 1):
        run_bwd(be, S, test, overwrite=overwrite)
    run_bwd(be, S, test, null=NULLS[mode] + ("dgamma",))
    run_bwd(be, S, test, null=NULLS[mode][:1] + ("dbeta",), overwrite=1)
    run_bwd(be, bn_set(6, 6, 6, C, mode, 1, 0, train), test)
    if not train:
        run_bwd(be, bn_set(6, 6, 6, C, mode, 1, 1, -1), test)


@pytest.mark.parametrize("C,mode,train", BWD_CELLS)
def test_backward_every_cell(C, mode, train):
    """{scalar, float4} x {plain, residual, pool, blend} x {train, eval} x {+=, overwrite}, both phases; optional outputs NULL and not; relu 0 and 1; eval mode with
    mean / invstd (dgamma = sum du xhat of the running statistics) and without"""
    test = f"bwd C{C} {mode} train{train}"
    bwd_cell(Library(), C, mode, train, test)
    report(test, TAG)


SLOT_CASES = [(15, 64, 1), (16, 64, 8), (63, 64, 8), (64, 64, 32), (64, 132, 32)]      # samples of 8 x 8 pixels, C -> slots


def slot_case(be, N, C, slots, test):
    S = bn_set(N, 8, 8, C)
    assert S.rpb == 64 and S.row_blocks == N and red_slots(S.row_blocks) == slots
    for red_all in (0, 1):
        run_bwd(be, S, test, red_all=red_all, overwrite=red_all)
        run_bwd(be, S, test, red_all=red_all, red_world=3)
    if C == 132:
        run_bwd(be, bn_set(N, 8, 8, C, "res"), test, red_all=1)


@pytest.mark.parametrize("N,C,slots", SLOT_CASES)
def test_backward_slot_counts(N, C, slots):
    """15 / 16 / 63 / 64 row blocks: 1, 8, 8 and 32 slot blocks of red, asserted from the blocks phase 1 filled; phase 2 with red_all 0 and 1 (red spread
    over all 32 slots by the test) and red_world 1 and 3 (dgamma / dbeta NULL, taken from the local red by mrfa_bn_param_grad)"""
    test = f"bwd slots N{N} C{C}"
    slot_case(Library(), N, C, slots, test)
    report(test, TAG)


RAGGED_ROWS = (65, 79, 80, 81, 95, 97)
RAGGED_C = (4, 60, 64, 68)


@pytest.mark.parametrize("C", RAGGED_C)
def test_backward_ragged_row_blocks(C):
    """a last row block of 1, 15, 16, 17, 31, 33 rows in the two-rows-per-trip loop (plain and residual), with partial channel chunks (C = 4, 60, 68) whose
    idle lanes re-read channel 0"""
    test = f"bwd ragged C{C}"
    for rows in RAGGED_ROWS:
        assert geometry(rows, C)[1] == 64
        for mode in ("plain", "res"):
            run_bwd(Library(), bn_set(1, 1, rows, C, mode), test, overwrite=rows % 2)
    report(test, TAG)


@pytest.mark.parametrize("C", SCALAR_C)
def test_backward_scalar_by_channel_count(C):
    test = f"bwd scalar C{C}"
    for mode in MODES:
        run_bwd(Library(), bn_set(2, 4, 6, C, mode), test, expect="scalar")
    report(test, TAG)


BWD_ROUTES = {"plain": ["ldx", "lddy", "lddx", "leadx", "leaddy", "leaddx", "leadsc", "leadsh", "leadm", "leadi", "leadg"],
              "res": ["ldr", "lddr", "leadr", "leaddr"], "blend": ["lda", "ldda", "leada", "leadda"]}


@pytest.mark.parametrize("mode", list(BWD_ROUTES))
def test_backward_scalar_by_layout(mode):
    """C = 64: each leading dimension in turn not a multiple of 4, each base pointer in turn offset by 4 bytes (dx: phase 2 alone goes scalar)"""
    test = f"bwd scalar by layout {mode}"
    for key in BWD_ROUTES[mode]:
        run_bwd(Library(), bn_set(2, 4, 6, 64, mode), test, lay=route(key, 64), expect="scalar")
    report(test, TAG)


def test_exact_zeros_are_on_the_closed_side():
    """x = 0, shift = 0 (res = 0) at every 11th element: u == 0 exactly; y = 0 and du = 0 there, in the scalar and the float4 kernels, without exclusion"""
    test = "zeros"
    for C in (64, 37):
        for mode in MODES:
            for train in (1, 0):
                S = bn_set(2, 4, 6, C, mode, 1, 1, train, True)
                run_fwd(Library(), S, test)
                run_bwd(Library(), S, test, overwrite=1)
    report(test, TAG)


# ------------------------------------------------------------------------------------------------------------------ statistic groups
GROUP_CASES = [(C, mode, G) for C in FWD_C for mode in MODES for G in (2, 3)]


def sub_set(S, g):
    """group g's samples as an ungrouped set with the group's scale / shift / mean / invstd (no reference: compared with the grouped call bit for bit)"""
    n = S.N // S.G
    T = types.SimpleNamespace(**vars(S))
    cut = lambda t, rows: None if t is None else t[g * rows:(g + 1) * rows].contiguous()
    T.N, T.G, T.rows, T.orow = n, 1, S.rows // S.G, S.orow // S.G
    for k in ("x", "res", "dx0", "dres0"):
        setattr(T, k, cut(getattr(S, k), T.rows))
    for k in ("A", "occ", "dy", "dA0", "docc0"):
        setattr(T, k, cut(getattr(S, k), T.orow))
    for k in ("sc", "sh", "mean", "invstd"):
        setattr(T, k, getattr(S, k)[g:g + 1].contiguous())
    return T


def raw_calls(be, T, overwrite):
    """forward and both backward phases of an ungrouped set, nothing compared: y, dx, dres"""
    mk = maker(be, {})
    C = T.C
    bx, br, ba, bo, bdy = mk(T.x, "x", NAN), mk(T.res, "r", NAN), mk(T.A, "a", NAN), mk(T.occ, "o", NAN), mk(T.dy, "dy", NAN)
    bsc, bsh, bm, bi, bg = [mk(t.reshape(1, -1), "p", NAN) for t in (T.sc, T.sh, T.mean, T.invstd, T.gamma)]
    by, bdx, bdr = mk(unwritten((T.orow, C)), "y", CANARY), mk(T.dx0, "dx", CANARY), mk(T.dres0, "dr", CANARY)
    bred = mk(torch.zeros(1, SLOTS * 2 * C, dtype=F64), "red", CANARY, F64)
    p = hip.BnActParams(x=bx.ptr, ldx=bx.ld, N=T.N, H=T.H, W=T.W, C=C, scale=bsc.ptr, shift=bsh.ptr, relu=T.relu, pool=int(T.pool), blend_a=ptr(ba), lda=ldof(ba),
                        occ=ptr(bo), ldo=ldof(bo), y=by.ptr, ldy=by.ld, res=ptr(br), ldr=ldof(br), groups=1)
    assert be.call("mrfa_bn_act_fwd", ctypes.byref(p)) == 0, be.error()
    for phase in (1, 2):
        p = hip.BnBwdParams(x=bx.ptr, ldx=bx.ld, N=T.N, H=T.H, W=T.W, C=C, scale=bsc.ptr, shift=bsh.ptr, relu=T.relu, pool=int(T.pool), mean=bm.ptr, invstd=bi.ptr,
                            gamma=bg.ptr, dy=bdy.ptr, lddy=bdy.ld, blend_a=ptr(ba), lda=ldof(ba), occ=ptr(bo), ldo=ldof(bo), red=bred.ptr, dx=bdx.ptr, lddx=bdx.ld,
                            train=1, phase=phase, dx_overwrite=overwrite, res=ptr(br), ldr=ldof(br), dres=ptr(bdr), lddr=ldof(bdr), groups=0)
        assert be.call("mrfa_bn_act_bwd", ctypes.byref(p)) == 0, be.error()
    return by.get(), bdx.get(), bdr.get() if bdr is not None else None


def group_case(be, C, mode, G, test):
    S = bn_set(6, 6, 6, C, mode, G)
    assert (S.rows // G) % S.rpb != 0
    y, _ = run_fwd(be, S, test)
    keep = {}
    run_bwd(be, S, test, keep=keep)
    run_bwd(be, S, test, red_world=3, overwrite=1)         # mrfa_bn_param_grad_groups on the local red
    parts = [raw_calls(be, sub_set(S, g), 0) for g in range(G)]
    assert torch.equal(torch.cat([p[0] for p in parts]), y), "y: grouped call != G ungrouped calls"
    assert torch.equal(torch.cat([p[1] for p in parts]), keep["dx"]), "dx: grouped call != G ungrouped calls"
    if mode == "res":
        assert torch.equal(torch.cat([p[2] for p in parts]), keep["dres"]), "dres: grouped call != G ungrouped calls"


@pytest.mark.parametrize("C,mode,G", GROUP_CASES)
def test_statistic_groups(C, mode, G):
    """G = 2, 3 (108 and 72 rows per group: no multiple of the 64-row block) plain, residual, pool and blend, float4 and scalar: against the reference, and
    bit for bit against G ungrouped calls on the sample ranges (y, dx, dres: the same arithmetic, element by element)"""
    test = f"groups C{C} {mode} G{G}"
    group_case(Library(), C, mode, G, test)
    report(test, TAG)


# ------------------------------------------------------------------------------------------------------------------ the chain
def chain_case(be, C, mode, G, test, ratio=0):
    """stats -> finalize -> forward -> phase 1 -> phase 2, every stage on what the one before it produced, against the float64 reference of the whole chain on
    x, gamma, beta, with the bounds composed"""
    S0 = bn_set(6, 6, 6, C, mode, G)
    S = types.SimpleNamespace(**vars(S0))
    n, N = S.rows // G, S.N
    rm0, rv0 = gen("norm/chain/rm", (C,), -0.5, 0.5), gen("norm/chain/rv", (C,), 0.5, 2)
    sts, d1, d2, refs = [], [], [], []
    for g in range(G):
        st, r, b1, b2, _ = run_stats(be, S.x[g * n:(g + 1) * n].contiguous(), test, "chain stats")
        sts.append(st)
        d1.append(b1)
        d2.append(b2)
        refs.append(torch.cat([r["s1"], r["s2"]]))
    d_t = (torch.stack(d1), torch.stack(d2))
    got, fr, fb = run_finalize(be, test, torch.stack(sts), n, S.gamma, S.beta, rm0, rv0, f32(0.1), grouped=True, d_t=d_t, ref_stats=torch.stack(refs), what="chain finalize")
    v4 = lambda t, h=S.H, w=S.W: None if t is None else t.view(N, h, w, -1)
    Ho, Wo = (S.H // 2, S.W // 2) if S.pool else (S.H, S.W)
    f = R.fwd_ref(v4(S.x), fr["scale"], fr["shift"], S.relu, S.pool, v4(S.res), v4(S.A), v4(S.occ))
    bf = fwd_bounds(f, S.pool, R.per_sample(fb["scale"], N), R.per_sample(fb["shift"], N))
    run_fwd(be, S, test, sc=got["scale"], sh=got["shift"], ref=f["y"].reshape(-1, C), bound=bf["y"].reshape(-1, C), what="chain y")
    # the backward on the kernel's own scale / shift / mean / invstd, against the exact chain
    S.sc, S.sh, S.mean, S.invstd = got["scale"], got["shift"], got["mean"], got["invstd"]
    S.f = f
    S.b1 = R.bwd1_ref(f, v4(S.dy, Ho, Wo), fr["mean"], fr["invstd"], S.relu, S.pool, G)
    cache = {}

    def bounds1(k):
        if k not in cache:
            cache[k] = bwd1_bounds(S, f, S.b1, bf["u"], k, fb["mean"], fb["invstd"])
        return cache[k]
    S.bounds1 = bounds1
    assert bounds1(1)["kink"].double().mean().item() <= 0.01
    S.chain, S.ref_invstd = (fr, fb), fr["invstd"]
    return S


def chain_expect(S, red, red_abs, overwrite, red_world=1, b1=None):
    """the composed phase-2 bounds: the reference's k1 / k2 come from the EXACT sums, the kernel's from the red phase 1 left (within b1's red bounds)"""
    exact = torch.cat([S.b1["s1"], S.b1["s2"]], 1)
    return bwd2_expect(S, exact, red_abs, overwrite, red_world, b1, d_red1=b1["red1"], d_red2=b1["red2"], b_inv=S.chain[1]["invstd"])


@pytest.mark.parametrize("C,mode,G", [(64, "res", 2), (37, "blend", 1), (132, "pool", 3)])
def test_chain(C, mode, G):
    test = f"chain C{C} {mode} G{G}"
    S = chain_case(Library(), C, mode, G, test)
    run_bwd(Library(), S, test, expect2=chain_expect)
    report(test, TAG)


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_norm_entry_points_refuse_what_they_do_not_take():
    """every MRFA_CHECK_ARG of the six entry points: non-zero, its message, nothing launched (the outputs stay bit-identical)"""
    be = Library()
    C, N, H, W = 8, 2, 4, 6
    rows = N * H * W
    outs = [Buf(unwritten((rows, C)), 1, C, CANARY) for _ in range(8)]
    dred = Buf(torch.zeros(1, SLOTS * 2 * C * 2, dtype=F64), 1, SLOTS * 2 * C * 2, 0.0, dtype=F64)
    z = Buf(torch.zeros(rows, C), 1, C, 0.0)
    o, zp = [b.ptr for b in outs], z.ptr

    def refused(rc, *words):
        msg = be.error()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)

    def fwd(**kw):
        a = dict(x=zp, ldx=C, N=N, H=H, W=W, C=C, scale=zp, shift=zp, relu=1, y=o[0], ldy=C)
        a.update(kw)
        return be.call("mrfa_bn_act_fwd", ctypes.byref(hip.BnActParams(**a)))

    def bwd(**kw):
        a = dict(x=zp, ldx=C, N=N, H=H, W=W, C=C, scale=zp, shift=zp, relu=1, mean=zp, invstd=zp, gamma=zp, dy=zp, lddy=C, red=dred.ptr, dx=o[1], lddx=C,
                 dgamma=o[2], dbeta=o[3], train=1, phase=1)
        a.update(kw)
        return be.call("mrfa_bn_act_bwd", ctypes.byref(hip.BnBwdParams(**a)))
    refused(fwd(pool=1, H=3), "bn_act_fwd", "even")
    refused(fwd(pool=1, W=5), "bn_act_fwd", "even")
    refused(fwd(pool=1, blend_a=zp, lda=C, occ=zp, ldo=1), "bn_act_fwd", "exclusive")
    refused(fwd(pool=1, res=zp, ldr=C), "bn_act_fwd", "residual")
    refused(fwd(blend_a=zp, lda=C, occ=zp, ldo=1, res=zp, ldr=C), "bn_act_fwd", "residual")
    refused(fwd(groups=3), "bn_act_fwd", "groups")
    refused(fwd(y=None), "bn_act_fwd", "null")
    refused(bwd(pool=1, res=zp, ldr=C), "bn_act_bwd", "residual")
    refused(bwd(dres=o[4], lddr=C), "bn_act_bwd", "residual")
    refused(bwd(pool=1, blend_a=zp, lda=C, occ=zp, ldo=1), "bn_act_bwd", "exclusive")
    refused(bwd(groups=3), "bn_act_bwd", "groups")
    for phase in (0, 3):
        refused(bwd(phase=phase), "bn_act_bwd", "phase")
    refused(bwd(phase=2, dx=None), "bn_act_bwd", "dx")              # float4 path
    refused(bwd(phase=2, dx=None, ldx=C + 1), "bn_act_bwd", "dx")   # scalar path
    refused(bwd(mean=None), "bn_act_bwd", "train")
    refused(bwd(red=None), "bn_act_bwd", "null")
    fin = [dred.ptr, rows, zp, zp]
    refused(be.call("mrfa_bn_finalize", None, rows, zp, zp, None, None, 0.1, EPS, C, 0, o[5], o[6], None, None), "bn_finalize", "statistics")
    refused(be.call("mrfa_bn_finalize", None, rows, zp, zp, None, None, 0.1, EPS, C, 1, o[5], o[6], None, None), "bn_finalize", "statistics")
    refused(be.call("mrfa_bn_finalize_groups", *fin, o[7], None, 0.1, EPS, C, 2, o[5], o[6], None, None), "bn_finalize_groups", "together")
    refused(be.call("mrfa_bn_finalize_groups", *fin, None, o[7], 0.1, EPS, C, 2, o[5], o[6], None, None), "bn_finalize_groups", "together")
    refused(be.call("mrfa_bn_finalize_groups", *fin, None, None, 0.1, EPS, C, 0, o[5], o[6], None, None), "bn_finalize_groups", "bad args")
    refused(be.call("mrfa_bn_stats", zp, C, 0, C, dred.ptr), "bn_stats")
    refused(be.call("mrfa_bn_param_grad", dred.ptr, C, None, None), "bn_param_grad")
    refused(be.call("mrfa_bn_param_grad_groups", dred.ptr, C, 0, o[2], o[3]), "bn_param_grad")
    assert all(b.untouched() for b in outs) and dred.untouched() and z.untouched(), "a refused call wrote"
