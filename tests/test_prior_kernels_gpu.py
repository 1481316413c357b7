"""The keypoint and prior-motion kernels (csrc/prior.hip: mrfa_kp_gaussian_*, mrfa_prior_motion_*, mrfa_softmax_combine_*, mrfa_kp_head_*) on every path against
the float64 reference of tests/ref_prior.py (-m gpu), element by element.  tests/test_prior_reference.py runs the same drivers, inputs and bounds on the fp32
specification (oracle/capi_emulator.py) and on deliberately wrong formulas, without a GPU: that is what shows the bounds can be met and that they discriminate.

ISOLATION.  Each kernel answers for its own roundings only: the warp of prior_motion_fwd is compared with the reference warp evaluated at the motions the kernel
stored (read back), prior_motion_bwd and its reference both read those stored motions, softmax_combine_bwd is given the mask the forward wrote, kp_head_bwd the
forward's kp / jac / stat.  test_chain_* compose the bounds: each stage is compared with the reference of the exact float64 stage before it, and its bound is
handed the perturbation the previous bound allows.

THE BOUNDS.  Every assertion is |got - ref| <= bound per element; no bound is a fraction of a tensor's maximum.  u = 2^-24 (1 + 2^-12) (the factor covers the
second-order terms, as in tests/test_norm_kernels_gpu.py).  To first order a k-term fp32 sum errs by at most (k - 1) u sum|terms| in any order, a product or a sum by
u |result|, a += (plain or atomic) by u (|old| + |new|), an atomic accumulation over b as a sum of that length.  A fused multiply-add makes fewer roundings than
counted, never more.  From tests/test_token_kernels_gpu.py / test_norm_kernels_gpu.py: exp 3 ulp (E_EXP = 6 u relative) plus the argument's movement, x / y 2.5
ulp (E_DIV = 5 u), TINY = 2^-126 absolute for a flushed result.
  grid  g = 2 (j / (n - 1)) - 1:   eg = E_DIV |g + 1| + u |g|          z = g - kp:   ez = eg + u |z|
  Gaussian  a = -(zx^2 + zy^2) inv_var / 2:   d_a = inv_var (|zx| ezx + |zy| ezy + u q) + 2 u |a|      (squares, their sum; inv_var = 1 / variance and the product -- the
      specification divides by the variance: one rounding);   G = exp(a):  G (E_EXP + d_a) + TINY
  mrfa_kp_gaussian   out: G's bound (+ u |out| with pos)
      dkp += sum_pixels t, t = dout G inv_var z:   sum [|t| (E_EXP + d_a + 4 u) + |dout G inv_var| ez + TINY |dout inv_var z|] + (HW - 1) u S_dkp + u (|old| + |new|)
      dpos += sum_b dout (atomic over b, B + 1 terms):   B u (|old| + S_dpos)
  mrfa_softmax_combine   a_k = l_k - max: rel_k = E_EXP + u |a_k|;   A = sum_j mask_j rel_j + (K1 - 1) u + K1 TINY (the sum of the exponentials)
      mask_k: mask_k (rel_k + A + E_DIV + u) + TINY    (1 / s then a product; the specification divides: fewer)        logit_nchw: exact
      deformation: sum_k (b_mask_k |motion_k| + u |mask_k motion_k|) + (K1 - 1) u Sdef
      backward, on the stored mask:  dm_k = ddef . motion_k + dmask_k: 3 u S3;   dot = sum_k mask_k dm_k: sum_k mask_k b_dm_k + K1 u Sdot
      dlogit_k += mask_k (dm_k - dot) + nchw_k:   mask_k (b_dm_k + b_dot + u |dm_k - dot|) + u |core| + u |core + nchw| + u (|old| + |new|)
      dmotions += mask_k ddef:   u |mask_k ddef| + u (|old| + |new|)
  mrfa_kp_head   s = l / T (the kernel: l (1 / T): 2 u |s|), stat0 = max s: 2 u |max|.  Everything else is compared for the stored stat0 as the common maximum:
      a = s - stat0: d_a = 2 u |s| + u |a|;  r_p = E_EXP + d_a;   S = sum e: relS = sum e r_p / S + (HW - 1) u + HW TINY / S;   stat1 = 1 / S: stat1 (relS + E_DIV)
      kp = sum heat g:   sum |heat g| (r_p + relS + E_DIV + 2 u) + sum heat eg + (HW - 1) u Skp + HW TINY      (holds (sum e g) (1 / S) and sum (e / S) g); jac likewise, eg = 0
      backward, on the stored kp / jac / stat:  p_k = exp(a) stat1: rel_p = r_p + u
      t = g . dkp - kp . dkp + (jm - jac) . djac:   b_t = eg . |dkp| + 10 u Tabs + [b_kp . |dkp| + b_jac . |djac|]
      dlogits += p_k t / T:   (p_k / T) b_t + |p_k t / T| (rel_p + [relS + E_DIV + u] + 3 u) + u (|old| + |new|)
      djm += sum_k p_k djac_k:   sum_k |p_k djac_k| (rel_p + [relS + E_DIV + u] + u) + (K - 1) u Sjm + u (|old| + |new|)
      DEPARTURE: the terms in [] are the forward's bounds.  The specification differentiates its own forward (it never reads kp / jac / stat: E_k[t] is a sum over
      the pixels, 1 / S its own), so a bound that holds both orderings carries what the forward may have rounded.  They are counted, not fitted, and the same
      terms are what test_chain_kp_head hands on.
  mrfa_prior_motion, forward   det = a0 a3 - a1 a2: b_det = 2 u (|a0 a3| + |a1 a2|);  inv = adj (1 / det): rel_inv = b_det / |det| + E_DIV + u (grows with 1 / |det|)
      J = js inv: b_J = Jabs (rel_inv + 2 u)      motion_k = J z + ks:  sum_j (b_J |z_j| + |J| ez_j) + 3 u mabs       (Jacobians null: J = I, b_J = 0)
      motion_0 = g: eg;  with bg  h = m (g, 1): b_h = |m0| egx + |m1| egy + 3 u habs;  hx / hz: (b_hx + |motion| b_hz) / |hz| + E_DIV |motion|
      heat = Gd - Gs:  both Gaussians' bounds (inv_var is given: the product, or the specification's 1 / (1 / inv_var) and division: 2 u |a|) + u |heat|
      warp at the STORED motions:  ix = ((mx + 1) W - 1) / 2, four roundings: d_ix = (W u |mx + 1| + u |(mx + 1) W| + u |(mx + 1) W - 1|) / 2 + u |ix|
          value: 8 u sum_taps |weight tap| + slope_h d_ix + slope_v d_iy   (fx, 1 - fx, the weight, the product: 4 u; 3 sums.  The value is continuous in the
          position: no element is excluded; slope = the largest tap difference over the 3 x 3 cells around)            sparse: bit-identical to inp's warp
  mrfa_prior_motion, backward (per pixel, then sums of HW terms, then the push)
      gix = sum_c g sum_taps (+-weight tap):  (4 C + 6) u Tx + Xc d_iy     (4 C terms in ATen's tap order, 6 roundings per term; Xc: the mixed difference the
          other coordinate's error is multiplied by);   dmx = dmot + gix W / 2:  (W / 2) b_gix + u |gix W / 2| + u |dmx|
      acc0 = sum dmx: sum b_dm + (HW - 1) u S;  acc2 = sum dmx zx: sum (b_dm |zx| + |dmx| ez + u |dmx zx|) + (HW - 1) u S;  acc6 = sum dheat Gd inv_var zx: as dkp
      dks += acc0 - acc8:  b0 + b8 + u |dks| + u (|old| + |new|)       dkd += -(J00 acc0 + J10 acc1) + acc6:  sum (b_J |acc| + |J| b_acc) + b6 + 3 u (abs terms) + +=
      djs += dJ inv^T:  |inv| b_dJ + Cjs (rel_inv + 3 u) + +=
      djd += -inv^T (js^T dJ) inv^T:  |inv|^T |js|^T b_dJ |inv|^T + Cjd (10 u + 2 rel_inv) + +=     (Cjd: the absolute terms of the kernel's three products AND of
          autograd's route through adj / det, whose terms cancel where the kernel's do not: DEPARTURE from the sketch, needed to hold both orderings)
      dbg:  dhx = dmx / hz: b_dm / |hz| + |dhx| (b_hz / |hz| + E_DIV);   dhz = -(dmx hx + dmy hy) / hz^2:  (b_dm |h| + |dm| b_h) / hz^2 + dhzabs (2 b_hz / |hz| + E_DIV + 4 u)
          sums of HW terms dh (g, 1):  sum (b_dh |g| + |dh| eg + u |t|) + (HW - 1) u Sdbg + u (|old| + |new|)
THE KINKS.  The warp's gradient jumps where ix or iy crosses an integer.  A pixel whose float64 coordinate lies within d_ix (d_iy) of an integer is a kink pixel:
its possible jump (|g| times twice the 3 x 3 slope -- at least the tap differences of both adjacent cells -- times W / 2 or H / 2) is ADDED to b_dm and so to
every sum the pixel enters; nothing is excluded.  Every set asserts that kink pixels are at most 0.1 % of its (b, k, pixel) triples.  Where every fp32 step of the
coordinate is exact (asserted: the centre row / column of an odd image under the identity motion, with bg the exact identity) d_ix = 0: an exact integer is no kink
pixel and is compared in full against the floor convention (the cell to the right).

BUFFERS.  Every operand sits in a kernel_check.Buf: inputs NaN outside their slice, outputs NaN inside and a canary outside that must survive (the pad32 padding
channels of inp and the unused columns of motions among it); every += output starts from random values; after each call every input is bit-identical.

MEASURED on an MI355X, largest err / bound per family (each test prints its own through report()):
  mrfa_kp_gaussian        out 0.999  dkp 0.149  dpos 0.758       (out: an element whose fp32 Gaussian is flushed to 0 just under 2^-126 -- the TINY term, met by construction)
  mrfa_softmax_combine    mask 0.295  deformation 0.231  dlogit 0.725  dmotions 0.500
  mrfa_kp_head            stat 0.570 / 0.042  kp 0.030  jac 0.052  dlogits 0.495  djm 0.480;   the chain: dlogits 0.491  djm 0.469
  mrfa_prior_motion       motions 0.269  heat 0.503  warp 0.446  dkd 0.066  dks 0.101  djd 0.040  djs 0.085  dbg 0.060
  the chain               warp 0.351  mask 0.240  deformation 0.113  dlogit 0.662  dmotions 0.481  dkd 0.008  dks 0.008  djd 0.008  djs 0.009  dbg 0.004
The elementwise outputs (one to a dozen roundings on values of order 1) stand at a quarter to three quarters of their count; the sums over H W pixels sit far
inside theirs, (HW - 1) u sum|terms| being a worst case no summation order attains.  That the bounds still discriminate is shown by the mutants of
tests/test_prior_reference.py and on the library itself: built with H and W swapped in kp_head_bwd_kernel's gcoord and with the heat-map term (- acc[8]) of dks
dropped, it failed test_kp_head and test_chain_kp_head at every non-square shape (a square one cannot see the swap), test_prior_motion at every shape with
more than one keypoint, test_prior_motion_exact_integer_positions and the kp_head determinism case (its driver asserts the bounds), and nothing else: the 224 x 216 set
did not notice the dropped term (48 384 pixels: the counted bound of the sum is wider than the heat-map term there).  A third planted error, the right tap admitted at
x0 + 1 == W, reads past the last column and is run in the float64 reference only (test_prior_reference.py), never on the device.
"""
import ctypes
import functools
import types

import pytest
import torch

from mrfa_amd import hip
from tests import ref_prior as R
from tests.kernel_check import CANARY, F64, NAN, Buf, check, note, report
from tests.kernel_check import U as U0
from tests.test_norm_kernels_gpu import gen
from tests.test_token_kernels_gpu import CAP, Library, Spec, f32, steps, unwritten

pytestmark = pytest.mark.gpu

U = U0 * (1 + 2.0 ** -12)
E_EXP, E_DIV = 6 * U, 5 * U
TINY = 2.0 ** -126
TAG = "prior"
KINK_CAP = 1e-3
Z = 1e-300                                                 # keeps err / bound defined where both are 0


def fb(be, t, fill, lead=3):
    """a tensor as one row of a Buf with watched surroundings"""
    if t is None:
        return None
    v = t.reshape(1, -1).float()
    return Buf(v, 1, v.shape[1], fill, lead=lead, gap=2, dev=be.dev)


def rb(be, t, ld, fill, lead=5):
    """[rows][C] with leading dimension ld"""
    if t is None:
        return None
    return Buf(t.float(), 1, ld, fill, lead=lead, gap=3, dev=be.dev)


def ptr(b):
    return b.ptr if b is not None else None


def same(bufs, what="an input changed"):
    assert all(b is None or b.untouched() for b in bufs), what


def eg(g):
    return E_DIV * (g + 1).abs() + U * g.abs()


def gauss_err(g, inv_var):
    """(ezx, ezy, d_a) of a ref_prior.gauss() record"""
    ezx, ezy = eg(g["gx"]) + U * g["dx"].abs(), eg(g["gy"]) + U * g["dy"].abs()
    d_a = inv_var * (g["dx"].abs() * ezx + g["dy"].abs() * ezy + U * g["q"]) + 2 * U * g["a"].abs()
    return ezx, ezy, d_a


def acc_add(old, inc, b_inc):
    """reference and bound of old += inc"""
    old = old.double().view_as(inc)
    return old + inc, b_inc + U * (old.abs() + (old + inc).abs()) + Z


# ================================================================================================================== kp_gaussian
GAUSS_SETS = [(2, 10, 7, 5, 12), (1, 1, 2, 2, 1), (3, 10, 64, 48, 16), (5, 10, 160, 144, 10)]
GAUSS_VAR = (0.01, 0.1)


@functools.lru_cache(maxsize=None)
def gauss_set(B, K, H, W, ld, variance):
    """kp ~ U(-0.9, 0.9) with planted keypoints: on a grid node, at (+1, -1), outside the grid (1.3, -1.3)"""
    name = f"prior/gauss/{B}.{K}.{H}.{W}"
    S = types.SimpleNamespace(B=B, K=K, H=H, W=W, ld=ld, var=f32(variance))
    kp = gen(name + "/kp", (B * K, 2), -0.9, 0.9)
    gx, gy = R.grid(H, W)
    plant = [(1.0, -1.0), (float(gx[0, 1]), float(gy[H - 1, 0])), (1.3, -1.3)]
    for i, v in enumerate(plant[:B * K]):
        kp[i * 7 % (B * K)] = torch.tensor(v)
    S.kp = kp.view(B, K, 2)
    S.pos = gen(name + "/pos", (K, H, W), -0.1, 0.1)
    S.dout = gen(name + "/dout", (B * H * W, K), -1, 1)
    S.dkp0, S.dpos0 = gen(name + "/dkp0", (B, K, 2), -1, 1), gen(name + "/dpos0", (K, H, W), -1, 1)
    return S


def gauss_fwd_bound(r, inv_var, with_pos):
    _, _, d_a = gauss_err(r["g"], inv_var)
    b = (r["g"]["G"] * (E_EXP + d_a) + TINY).permute(0, 2, 3, 1)
    return b + U * r["out"].abs() if with_pos else b


def gauss_bwd_bounds(S, r):
    inv_var = 1.0 / S.var
    g = r["g"]
    ezx, ezy, d_a = gauss_err(g, inv_var)
    d = S.dout.double().view(S.B, S.H, S.W, S.K).permute(0, 3, 1, 2).abs()
    per = lambda t, ez, z: (t.abs() * (E_EXP + d_a + 4 * U) + r["w"].abs() * ez + TINY * d * inv_var * z.abs()).sum((2, 3))
    b_dkp = torch.stack([per(r["tx"], ezx, g["dx"]), per(r["ty"], ezy, g["dy"])], -1) + (S.H * S.W - 1) * U * r["S_dkp"]
    return b_dkp, S.B * U * (S.dpos0.double().abs() + r["S_dpos"]) + Z


def run_gauss(be, S, test, with_pos=True, null=(), wrong="", keep=None):
    B, K, H, W = S.B, S.K, S.H, S.W
    bkp, bpos = fb(be, S.kp, NAN), fb(be, S.pos, NAN) if with_pos else None
    bout = rb(be, unwritten((B * H * W, K)), S.ld, CANARY)
    rc = be.call("mrfa_kp_gaussian_fwd", bkp.ptr, ptr(bpos), B, K, H, W, S.var, bout.ptr, S.ld)
    assert rc == 0, be.error()
    r = R.kp_gaussian_fwd(S.kp, S.pos if with_pos else None, H, W, S.var)
    got = bout.get()
    note(test, "out", check(got, r["out"].reshape(-1, K), gauss_fwd_bound(r, 1.0 / S.var, with_pos).reshape(-1, K), f"kp_gaussian out {test}"))
    same((bkp, bpos))
    # ---- backward
    bdout = rb(be, S.dout, S.ld, NAN)
    bdkp = fb(be, S.dkp0, CANARY) if "dkp" not in null else None
    bdpos = fb(be, S.dpos0, CANARY) if "dpos" not in null else None
    rc = be.call("mrfa_kp_gaussian_bwd", bkp.ptr, B, K, H, W, S.var, bdout.ptr, S.ld, ptr(bdkp), ptr(bdpos))
    assert rc == 0, be.error()
    rbk = R.kp_gaussian_bwd(S.kp, S.dout.view(B, H, W, K), H, W, S.var)
    b_dkp, b_dpos = gauss_bwd_bounds(S, rbk)
    if bdkp is not None:
        ref, bound = acc_add(S.dkp0, rbk["dkp"], b_dkp)
        note(test, "dkp", check(bdkp.get().view(B, K, 2), ref, bound, f"kp_gaussian dkp {test}"))
    if bdpos is not None:
        note(test, "dpos", check(bdpos.get().view(K, H, W), S.dpos0.double() + rbk["dpos"], b_dpos, f"kp_gaussian dpos {test}"))
    same((bkp, bdout))
    if keep is not None:
        keep.update(out=bout.bits())


def gauss_cases(be, B, K, H, W, ld, test):
    big = B * K * H * W > CAP * 256
    for variance in GAUSS_VAR[:1] if big else GAUSS_VAR:
        S = gauss_set(B, K, H, W, ld, variance)
        run_gauss(be, S, test)
        if not big:
            run_gauss(be, S, test, with_pos=False, null=("dpos",))
            run_gauss(be, S, test, null=("dkp",))


@pytest.mark.parametrize("B,K,H,W,ld", GAUSS_SETS)
def test_kp_gaussian(B, K, H, W, ld):
    """non-square shapes, one pixel row of two, the second grid-stride trip; variance 0.01 (the Gaussian underflows) and 0.1; pos, dkp, dpos null and given"""
    test = f"kp_gaussian {B}x{K}x{H}x{W}"
    assert steps(5 * 10 * 160 * 144) == 2
    gauss_cases(Library(), B, K, H, W, ld, test)
    report(test, TAG)


# ================================================================================================================== softmax_combine
SC_K1 = (1, 2, 11, 32)
SC_REGIMES = ("mild", "peak", "equal")
SC_BIG = (2, 1, 1032, 1032)
SC_NULLS = [(), ("ddef",), ("dmask",), ("dnchw",), ("ddef", "dmask"), ("ddef", "dnchw"), ("dmask", "dnchw")]      # what engine.py can produce: any subset but all three


@functools.lru_cache(maxsize=None)
def sc_set(K1, B, H, W, regime="mild"):
    name = f"prior/sc/{K1}.{B}.{H}.{W}.{regime}"
    S = types.SimpleNamespace(K1=K1, B=B, H=H, W=W, regime=regime)
    n = B * H * W
    if regime == "equal":
        S.logit = torch.full((n, K1), 0.7)
    else:
        S.logit = gen(name + "/l", (n, K1), -3, 3)
        if regime == "peak":
            S.logit[torch.arange(n), torch.arange(n) % K1] += 100.0
    S.mot = gen(name + "/m", (B * K1 * H * W, 2), -1, 1)
    S.ddef, S.dmask, S.dnchw = gen(name + "/dd", (B, H, W, 2), -1, 1), gen(name + "/dk", (B, K1, H, W), -1, 1), gen(name + "/dn", (B, K1, H, W), -1, 1)
    S.dl0, S.dm0 = gen(name + "/dl0", (n, K1), -1, 1), gen(name + "/dm0", (B * K1 * H * W, 2), -1, 1)
    return S


def sc_fwd_bounds(r, K1, d_mo=0.0):
    """d_mo: what the motions may be off by (the chain)"""
    rel = E_EXP + U * r["a"].abs()
    A = (r["m"] * rel).sum(-1, keepdim=True) + (K1 - 1) * U + K1 * TINY
    b_mask = r["m"] * (rel + A + E_DIV + U) + TINY
    t = r["m"].unsqueeze(-1) * r["mo"]
    b_def = (b_mask.unsqueeze(-1) * r["mo"].abs() + U * t.abs() + r["m"].unsqueeze(-1) * d_mo).sum(3) + (K1 - 1) * U * r["Sdef"] + Z
    return b_mask.permute(0, 3, 1, 2), b_def


def sc_bwd_bounds(r, K1, old_l, old_m, d_mask=0.0, d_mo=0.0):
    """bounds of dlogit [B][H][W][K1] and dmotions [B][K1][H][W][2] (old values included); d_mask [B][H][W][K1], d_mo: input perturbations (the chain)"""
    m = r["m"]
    dd = r["dd"]
    d_mask = d_mask if torch.is_tensor(d_mask) else torch.zeros_like(m)
    b_dm = 3 * U * r["S3"] + (dd.abs().unsqueeze(3) * d_mo).sum(-1)
    b_dot = (m * b_dm).sum(-1, keepdim=True) + K1 * U * r["Sdot"] + (d_mask * r["dm"].abs()).sum(-1, keepdim=True)
    dev = (r["dm"] - r["dot"]).abs()
    b_core = m * (b_dm + b_dot + U * dev) + U * r["core"].abs() + d_mask * dev
    b_new = b_core + U * r["dlogit"].abs()
    ref_l, b_l = acc_add(old_l, r["dlogit"], b_new)
    inc = r["dmotions"]
    ref_m, b_m = acc_add(old_m, inc, U * inc.abs() + d_mask.permute(0, 3, 1, 2).unsqueeze(-1) * dd.unsqueeze(1).abs())
    return ref_l, b_l, ref_m, b_m


def run_sc(be, S, test, ldl=None, ldm=2, null=(), fwd_only=False, keep=None):
    K1, B, H, W = S.K1, S.B, S.H, S.W
    ldl = ldl or K1
    n = B * H * W
    bl, bm = rb(be, S.logit, ldl, NAN), rb(be, S.mot, ldm, NAN)
    bdef, bmask, bnchw = fb(be, unwritten((n, 2)), CANARY), fb(be, unwritten((B, K1, H, W)), CANARY), fb(be, unwritten((B, K1, H, W)), CANARY)
    rc = be.call("mrfa_softmax_combine_fwd", bl.ptr, ldl, bm.ptr, ldm, B, H, W, K1, bdef.ptr, bmask.ptr, bnchw.ptr)
    assert rc == 0, be.error()
    mot5 = S.mot.view(B, K1, H, W, 2)
    r = R.softmax_combine_fwd(S.logit.view(B, H, W, K1), mot5)
    b_mask, b_def = sc_fwd_bounds(r, K1)
    mask = bmask.get().view(B, K1, H, W)
    note(test, "mask", check(mask, r["mask"], b_mask, f"softmax_combine mask {test}"))
    note(test, "deformation", check(bdef.get().view(B, H, W, 2), r["deformation"], b_def, f"softmax_combine deformation {test}"))
    assert torch.equal(bnchw.get().view(B, K1, H, W), S.logit.view(B, H, W, K1).permute(0, 3, 1, 2)), "logit_nchw is a copy"
    same((bl, bm))
    if keep is not None:
        keep.update(mask=bmask.bits(), deformation=bdef.bits())
    if fwd_only:
        return
    dd, dk, dn = [None if k in null else t for k, t in (("ddef", S.ddef), ("dmask", S.dmask), ("dnchw", S.dnchw))]
    bdd, bdk, bdn = fb(be, dd, NAN), fb(be, dk, NAN), fb(be, dn, NAN)
    bmk = fb(be, mask, NAN)                                 # the mask the forward wrote
    lddl = ldl + 1
    bdl = rb(be, S.dl0, lddl, CANARY)
    bdm = rb(be, S.dm0, ldm, CANARY) if dd is not None else None
    rc = be.call("mrfa_softmax_combine_bwd", bm.ptr, ldm, B, H, W, K1, bmk.ptr, ptr(bdd), ptr(bdk), ptr(bdn), bdl.ptr, lddl, ptr(bdm))
    assert rc == 0, be.error()
    rbk = R.softmax_combine_bwd(mot5, mask, dd, dk, dn)
    rbk["dd"] = dd.double() if dd is not None else torch.zeros(B, H, W, 2, dtype=F64)
    ref_l, b_l, ref_m, b_m = sc_bwd_bounds(rbk, K1, S.dl0.view(B, H, W, K1), S.dm0.view(B, K1, H, W, 2))
    tag = "" if not null else "[" + " ".join(null) + " null]"
    note(test, "dlogit" + tag, check(bdl.get().view(B, H, W, K1), ref_l, b_l, f"softmax_combine dlogit {test} {tag}"))
    if bdm is not None:
        note(test, "dmotions" + tag, check(bdm.get().view(B, K1, H, W, 2), ref_m, b_m, f"softmax_combine dmotions {test} {tag}"))
    same((bm, bmk, bdd, bdk, bdn))
    if keep is not None:
        keep.update(dlogit=bdl.bits(), dmotions=bdm.bits() if bdm is not None else None)


def sc_cases(be, K1, test):
    for i, regime in enumerate(SC_REGIMES):
        S = sc_set(K1, 2, 9, 7, regime)
        run_sc(be, S, test, ldl=K1 + i % 2, ldm=2 + 2 * (i % 2))
    S = sc_set(K1, 2, 9, 7)
    for i, null in enumerate(SC_NULLS[1:]):
        run_sc(be, S, test, ldl=K1 + 1 - i % 2, ldm=4 - 2 * (i % 2), null=null)


@pytest.mark.parametrize("K1", SC_K1)
def test_softmax_combine(K1):
    """K1 = 1, 2, 11 and 32 (the limit); logits in [-3, 3], one logit 100 above the rest, all equal; ldl = K1 and K1 + 1, ldm = 2 and 4; every combination of null
    gradients engine.py can produce (dmotions null exactly when ddeformation is)"""
    test = f"softmax_combine K1={K1}"
    sc_cases(Library(), K1, test)
    report(test, TAG)


def test_softmax_combine_grid_stride_second_trip():
    test = "softmax_combine 1032x1032"
    assert steps(1032 * 1032) == 2
    run_sc(Library(), sc_set(*SC_BIG), test)
    report(test, TAG)


# ================================================================================================================== kp_head
KH_SETS = [(2, 58, 58, 10), (2, 5, 9, 3), (1, 2, 2, 1), (1, 16, 17, 10), (2, 64, 48, 10)]
KH_BIG = (1, 1032, 1032, 1)
KH_T = (0.1, 1.0)
KH_REGIMES = ("mild", "peak", "equal")


@functools.lru_cache(maxsize=None)
def kh_set(B, H, W, K, regime="mild"):
    name = f"prior/kh/{B}.{H}.{W}.{K}.{regime}"
    S = types.SimpleNamespace(B=B, H=H, W=W, K=K, regime=regime)
    n = B * H * W
    if regime == "equal":
        S.logits = torch.full((n, K), -0.3)
    else:
        S.logits = gen(name + "/l", (n, K), -1, 1)
        if regime == "peak":
            lg = S.logits.view(B, H * W, K)
            for b in range(B):
                for k in range(K):
                    lg[b, (b * 31 + k * 17) % (H * W), k] += 3.0
    S.jm = gen(name + "/j", (n, 4), -1, 1)
    S.dkp, S.djac = gen(name + "/dk", (B, K, 2), -1, 1), gen(name + "/dj", (B, K, 4), -1, 1)
    S.dl0, S.djm0 = gen(name + "/dl0", (n, K), -1, 1), gen(name + "/djm0", (n, 4), -1, 1)
    return S


def kh_fwd_bounds(r, HW, d_s=0.0):
    """bounds of stat1, kp, jac for the common maximum r was computed with; d_s: what s - max may be off by on top (the chain: 0 here)"""
    d_a = 2 * U * r["s"].abs() + U * r["a"].abs() + d_s
    rp = E_EXP + d_a
    relS = (r["e"] * rp).sum(1) / r["S"] + (HW - 1) * U + HW * TINY / r["S"]
    rel = (rp + (relS + E_DIV + 2 * U).unsqueeze(1)).unsqueeze(-1)
    h = r["heat"].unsqueeze(-1)
    g = r["g"].view(1, HW, 1, 2)
    b = dict(relS=relS, rp=rp, stat1=r["stat"][..., 1] * (relS + E_DIV) + Z)
    b["kp"] = ((h * g).abs() * rel + h * eg(g)).sum(1) + (HW - 1) * U * r["Skp"] + HW * TINY + Z
    if "jac" in r:
        b["jac"] = ((h * r["jm4"]).abs() * rel).sum(1) + (HW - 1) * U * r["Sjac"] + HW * TINY + Z
    return b


def kh_bwd_bounds(S, r, bf, T, old_l, old_j):
    """bf: the forward's bounds (the terms in [] of the docstring)"""
    B, H, W, K = S.B, S.H, S.W, S.K
    HW = H * W
    d_a = 2 * U * r["s"].abs() + U * r["a"].abs()
    rel_p = E_EXP + d_a + U
    rel_st = (bf["relS"] + E_DIV + U).unsqueeze(1)
    g = r["g"]
    b_t = (eg(g) * r["gk"].abs()).sum(-1) + 10 * U * r["Tabs"] + (bf["kp"].unsqueeze(1) * r["gk"].abs()).sum(-1)
    if "dj" in r:
        b_t = b_t + (bf["jac"].unsqueeze(1) * r["dj"].abs()).sum(-1)
    v = r["dlogits"].view(B, HW, K)
    b_v = r["pk"] / T * b_t + v.abs() * (rel_p + rel_st + 3 * U) + TINY / T * r["t"].abs()
    ref_l, b_l = acc_add(old_l, r["dlogits"], b_v.view(B, H, W, K))
    out = dict(dlogits=(ref_l, b_l))
    if "djm" in r:
        pj = r["pk"].unsqueeze(-1) * r["dj"]
        b_j = (pj.abs() * (rel_p + rel_st + U).unsqueeze(-1)).sum(2).view(B, H, W, 4) + (K - 1) * U * r["Sjm"]
        out["djm"] = acc_add(old_j, r["djm"], b_j)
    return out


def run_kh(be, S, test, T=0.1, ldl=None, ldj=4, with_jm=True, null=(), fwd_only=False, keep=None, chain=False):
    B, H, W, K = S.B, S.H, S.W, S.K
    HW, n = H * W, B * H * W
    ldl = ldl or K
    T = f32(T)
    bl, bj = rb(be, S.logits, ldl, NAN), rb(be, S.jm, ldj, NAN) if with_jm else None
    bkp, bjac, bst = fb(be, unwritten((B, K, 2)), CANARY), fb(be, unwritten((B, K, 4)), CANARY), fb(be, unwritten((B, K, 2)), CANARY)
    rc = be.call("mrfa_kp_head_fwd", bl.ptr, ldl, ptr(bj), ldj if with_jm else 0, B, H, W, K, T, bkp.ptr, bjac.ptr if with_jm else None, bst.ptr)
    assert rc == 0, be.error()
    lg4, jm4 = S.logits.view(B, H, W, K), S.jm.view(B, H, W, 4) if with_jm else None
    stat = bst.get().view(B, K, 2)
    exact = R.kp_head_fwd(lg4, jm4, T)
    note(test, "stat0", check(stat[..., 0], exact["stat"][..., 0], 2 * U * exact["stat"][..., 0].abs() + Z, f"kp_head max {test}"))
    r = R.kp_head_fwd(lg4, jm4, T, mx=stat[..., 0])
    if with_jm:
        r["jm4"] = S.jm.double().view(B, HW, 1, 4)
    bf = kh_fwd_bounds(r, HW)
    kp = bkp.get().view(B, K, 2)
    note(test, "stat1", check(stat[..., 1], r["stat"][..., 1], bf["stat1"], f"kp_head 1/sum {test}"))
    note(test, "kp", check(kp, r["kp"], bf["kp"], f"kp_head kp {test}"))
    if S.regime == "equal":
        assert (kp.double().abs() <= bf["kp"]).all(), "all logits equal: kp is the grid mean, 0"
    if with_jm:
        jac = bjac.get().view(B, K, 4)
        note(test, "jac", check(jac, r["jac"], bf["jac"], f"kp_head jac {test}"))
    else:
        assert bjac.untouched(), "jac written without maps"
        jac = None
    same((bl, bj))
    if keep is not None:
        keep.update(kp=bkp.bits(), jac=bjac.bits(), stat=bst.bits())
    if fwd_only:
        return
    dkp, djac = None if "dkp" in null else S.dkp, None if ("djac" in null or not with_jm) else S.djac
    ikp, ijac, ist = fb(be, kp, NAN), fb(be, jac, NAN), fb(be, stat, NAN)
    bdk, bdj = fb(be, dkp, NAN), fb(be, djac, NAN)
    lddl, lddj = ldl + 1, ldj + 1
    bdl = rb(be, S.dl0, lddl, CANARY)
    bdjm = rb(be, S.djm0, lddj, CANARY) if with_jm and "djm" not in null else None
    rc = be.call("mrfa_kp_head_bwd", bl.ptr, ldl, ptr(bj), ldj if with_jm else 0, B, H, W, K, T, ikp.ptr, ptr(ijac), ist.ptr, ptr(bdk), ptr(bdj), bdl.ptr, lddl,
                 ptr(bdjm), lddj if with_jm else 0)
    assert rc == 0, be.error()
    if chain:                                               # against the backward of the exact forward: the forward's bounds are the perturbation handed on
        rbk = R.kp_head_bwd(lg4, jm4, T, exact["kp"], exact.get("jac"), exact["stat"], dkp, djac)
    else:
        rbk = R.kp_head_bwd(lg4, jm4, T, kp, jac, stat, dkp, djac)
    rbk["g"] = r["g"].view(1, HW, 1, 2)
    out = kh_bwd_bounds(S, rbk, bf, T, S.dl0.view(B, H, W, K), S.djm0.view(B, H, W, 4))
    tag = ("" if not null else "[" + " ".join(null) + " null]") + ("" if with_jm else "[no maps]")
    note(test, "dlogits" + tag, check(bdl.get().view(B, H, W, K), *out["dlogits"], f"kp_head dlogits {test} {tag}"))
    if bdjm is not None:
        if djac is not None:
            note(test, "djm" + tag, check(bdjm.get().view(B, H, W, 4), *out["djm"], f"kp_head djm {test} {tag}"))
        else:
            assert bdjm.untouched(), "djm written without djac"
    same((bl, bj, ikp, ijac, ist, bdk, bdj))
    if keep is not None:
        keep.update(dlogits=bdl.bits(), djm=bdjm.bits() if bdjm is not None else None)


def kh_cases(be, B, H, W, K, test):
    for i, regime in enumerate(KH_REGIMES):
        S = kh_set(B, H, W, K, regime)
        run_kh(be, S, test, T=KH_T[i % 2], ldl=K + 2 * (i % 2), ldj=4 + 2 * (i % 2))
    S = kh_set(B, H, W, K)
    run_kh(be, S, test, T=1.0, ldl=K + 2, ldj=6, null=("dkp",))
    run_kh(be, S, test, T=0.1, null=("djac",))
    run_kh(be, S, test, T=0.1, ldl=K + 2, null=("djm",))
    run_kh(be, S, test, T=1.0, with_jm=False)


@pytest.mark.parametrize("B,H,W,K", KH_SETS)
def test_kp_head(B, H, W, K):
    """58 x 58 (the model's), 45 pixels (one partial wave), 4 pixels, 272 (one pixel column past the workgroup), 64 x 48; T = 0.1 and 1; logits in [-1, 1], one peak 3
    above the rest, all equal; ldl = K and K + 2, ldj = 4 and 6; maps null and given; dkp null, djac null, djm null with djac given"""
    test = f"kp_head {B}x{H}x{W}x{K}"
    kh_cases(Library(), B, H, W, K, test)
    report(test, TAG)


def test_kp_head_grid_stride_second_trip():
    """1032 x 1032 pixels, K = 1: 4160 trips of the forward's workgroup, the backward's second grid-stride trip"""
    test = "kp_head 1032x1032"
    assert steps(1032 * 1032) == 2
    run_kh(Library(), kh_set(*KH_BIG), test, T=1.0, ldl=3, ldj=6)
    report(test, TAG)


@pytest.mark.parametrize("B,H,W,K", [(2, 5, 9, 3), (1, 16, 17, 10)])
def test_chain_kp_head(B, H, W, K):
    """forward -> backward: the backward's outputs against the backward of the exact float64 forward, within its own bound plus what the forward's bounds allow"""
    test = f"chain kp_head {B}x{H}x{W}x{K}"
    run_kh(Library(), kh_set(B, H, W, K, "peak"), test, T=0.1, ldl=K + 2, ldj=6, chain=True)
    report(test, TAG)


# ================================================================================================================== prior_motion
PM_SETS = [(2, 10, 16, 12, 3, 4, 4, 64), (1, 1, 2, 3, 1, 1, 2, 4), (2, 3, 9, 16, 8, 8, 2, 36), (1, 2, 15, 11, 3, 3, 4, 12)]
PM_BIG = (2, 10, 224, 216, 1, 1, 2, 22)
PM_ODD = (1, 2, 15, 11, 3, 3, 4, 12)
PM_VAR = 0.01
EYE4 = torch.tensor([1.0, 0.0, 0.0, 1.0])
EYE9 = torch.tensor([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])


@functools.lru_cache(maxsize=None)
def pm_set(B, K, H, W, C, lds, ldm, ldi, jac=True, bg="near", det="normal", exact=False):
    """kd ~ U(-0.8, 0.8); ks by keypoint: well inside (U(-0.8, 0.8)); kd -+ (0.7 / W, 0.7 / H) (0.35 of a pixel; with the identity's own half-pixel bands at the image border: pixels in
    (-1, 0) and (W - 1, W) in both axes); kd + 6 (every pixel fully outside unless |det jd| is small).  jd = I + 0.2 U(-1, 1) (|det| in [0.5, 1.5]; det="small": scaled to |det| near 0.1),
    js likewise; bg = I + 0.1 U(-1, 1) with the last row (0.1 U, 0.1 U, 1 + 0.1 U): hz in [0.7, 1.3].  exact: keypoint 0 has kd = ks = 0 (the identity motion)"""
    name = f"prior/pm/{B}.{K}.{H}.{W}.{C}.{int(jac)}.{bg}.{det}"
    S = types.SimpleNamespace(B=B, K=K, H=H, W=W, C=C, lds=lds, ldm=ldm, ldi=ldi, K1=K + 1, HW=H * W, exact=exact, det=det)
    S.inv_var = f32(1.0 / PM_VAR)
    S.kd = gen(name + "/kd", (B, K, 2), -0.8, 0.8)
    S.ks = gen(name + "/ks", (B, K, 2), -0.8, 0.8)
    step = torch.tensor([0.7 / W, 0.7 / H])                # 0.35 of a pixel: no pixel of any set lands on an integer
    for k in range(K):
        if k % 3 == 1:
            S.ks[:, k] = S.kd[:, k] + (step if k % 2 else -step)
        if k % 3 == 2:
            S.ks[:, k] = S.kd[:, k] + 6.0
    S.outside = [k + 1 for k in range(K) if k % 3 == 2]
    if exact:
        S.kd[:, 0] = 0.0
        S.ks[:, 0] = 0.0
    S.jd = S.js = None
    if jac:
        S.jd, S.js = EYE4 + 0.2 * gen(name + "/jd", (B, K, 4), -1, 1), EYE4 + 0.2 * gen(name + "/js", (B, K, 4), -1, 1)
        if det == "small":
            S.jd = S.jd * 0.32
        d = (S.jd[..., 0] * S.jd[..., 3] - S.jd[..., 1] * S.jd[..., 2]).abs()
        assert (d >= (0.05 if det == "small" else 0.5)).all() and (d <= (0.2 if det == "small" else 1.5)).all(), name
    S.bg = None if bg == "none" else (EYE9.repeat(B, 1) if bg == "eye" else EYE9 + 0.1 * gen(name + "/bg", (B, 9), -1, 1))
    S.src = gen(name + "/src", (B * H * W, C), 0, 1)
    n = B * S.K1 * H * W
    S.dinp = gen(name + "/dinp", (B * H * W, S.K1 * (C + 1)), -1, 1)
    S.dmot, S.dsp = gen(name + "/dmot", (n, 2), -1, 1), gen(name + "/dsp", (B, S.K1, C, H, W), -1, 1)
    S.g0 = {k: gen(name + "/g0" + k, shp, -1, 1) for k, shp in (("dkd", (B, K, 2)), ("dks", (B, K, 2)), ("djd", (B, K, 4)), ("djs", (B, K, 4)), ("dbg", (B, 9)))}
    S.f = R.prior_fwd(S.kd, S.ks, S.jd, S.js, S.bg, H, W, S.inv_var)
    if S.bg is not None:
        assert (S.f["h"][2] >= 0.7).all() and (S.f["h"][2] <= 1.3).all(), name
    S.fb = pm_fwd_bounds(S.f)
    return S


def pm_fwd_bounds(f):
    """bounds of the motions [B][K1][H][W][2] and of heat [B][K1][H][W]"""
    gd, gs = f["gd"], f["gs"]
    inv_var = f["inv_var"]
    ezx, ezy, da_d = gauss_err(gd, inv_var)
    _, _, da_s = gauss_err(gs, inv_var)
    b_heat = gd["G"] * (E_EXP + da_d) + gs["G"] * (E_EXP + da_s) + 2 * TINY + U * (gd["G"] - gs["G"]).abs()
    e = lambda t: t[..., None, None]
    J = f["J"]
    if f["A"] is not None:
        A = f["A"]
        rel_inv = 2 * U * A["detabs"] * A["rdet"] + E_DIV + U
        bJ = [ja * (rel_inv + 2 * U) for ja in A["Jabs"]]
    else:
        rel_inv, bJ = None, [torch.zeros_like(J[0])] * 4
    zx, zy = gd["dx"].abs(), gd["dy"].abs()
    b_mx = e(bJ[0]) * zx + e(bJ[1]) * zy + e(J[0].abs()) * ezx + e(J[1].abs()) * ezy + 3 * U * f["mabs"][0]
    b_my = e(bJ[2]) * zx + e(bJ[3]) * zy + e(J[2].abs()) * ezx + e(J[3].abs()) * ezy + 3 * U * f["mabs"][1]
    egx, egy = eg(f["gx"]), eg(f["gy"])
    B = b_mx.shape[0]
    b = dict(bJ=bJ, rel_inv=rel_inv, egx=egx, egy=egy, ezx=ezx, ezy=ezy, da_d=da_d, da_s=da_s)
    if "h" in f:
        m = f["m"].abs()
        bh = [m[:, 3 * i] * egx + m[:, 3 * i + 1] * egy + 3 * U * f["habs"][i] for i in range(3)]
        hz = f["h"][2].abs()
        mo0 = f["motions"][:, 0]
        b0x = (bh[0] + mo0[..., 0].abs() * bh[2]) / hz + E_DIV * mo0[..., 0].abs()
        b0y = (bh[1] + mo0[..., 1].abs() * bh[2]) / hz + E_DIV * mo0[..., 1].abs()
        b["bh"] = bh
    else:
        b0x, b0y = egx.expand(B, *egx.shape), egy.expand(B, *egy.shape)
    b["motions"] = torch.stack([torch.cat([b0x.unsqueeze(1), b_mx], 1), torch.cat([b0y.unsqueeze(1), b_my], 1)], -1) + Z
    b["heat"] = torch.cat([torch.zeros_like(b_heat[:, :1]), b_heat], 1)
    return b


def coord_err(m, n, extra=None):
    """the pixel coordinate i = ((m + 1) n - 1) / 2 of a stored fp32 motion m (as double), its counted error d_i (0 where every fp32 step is exact) and that flag.
    extra: what i may be off by before any rounding (the chain: m is then the exact motion, not a stored one)"""
    s1 = m + 1.0
    s2 = s1 * n
    s3 = s2 - 1.0
    i = 0.5 * s3
    d = 0.5 * (n * U * s1.abs() + U * s2.abs() + U * s3.abs()) + U * i.abs()
    f = m.float()
    t1 = f + 1.0
    t2 = t1 * float(n)
    t3 = t2 - 1.0
    exact = (t1.double() == s1) & (t2.double() == s2) & (t3.double() == s3)
    if extra is not None:
        exact = exact & (extra == 0)
        d = d + extra
    return i, torch.where(exact, torch.zeros_like(d), d), exact


def warp_bounds(wp, extra=(None, None)):
    """the value's bound [B][K1][C][H][W], the coordinate errors and the kink flags [B][K1][H][W]"""
    _, d_ix, ex_x = coord_err(wp["mx"], wp["W"], extra[0])
    _, d_iy, ex_y = coord_err(wp["my"], wp["H"], extra[1])
    b_val = 8 * U * wp["tapabs"] + wp["slope_h"] * d_ix.unsqueeze(2) + wp["slope_v"] * d_iy.unsqueeze(2)
    near = lambda i, d: (i - torch.round(i)).abs() <= d
    kx, ky = near(wp["ix"], d_ix) & ~ex_x, near(wp["iy"], d_iy) & ~ex_y
    return dict(val=b_val, d_ix=d_ix, d_iy=d_iy, kx=kx, ky=ky, exact_x=ex_x, exact_y=ex_y, share=(kx | ky).double().mean().item())


def pm_warp(S, motions, wrong=""):
    """the reference warp at the given (stored) motions [B][K1][H][W][2]"""
    m = motions.double()
    wp = R.warp(S.src.view(S.B, S.H, S.W, S.C), m, wrong)
    wp["mx"], wp["my"] = m[..., 0], m[..., 1]
    return wp


def pm_params(S, bufs, bwd=None):
    p = hip.PriorParams()
    p.kd, p.ks, p.jd, p.js, p.bg = [ptr(bufs[k]) for k in ("kd", "ks", "jd", "js", "bg")]
    p.src, p.lds, p.B, p.K, p.H, p.W, p.C, p.inv_var = bufs["src"].ptr, S.lds, S.B, S.K, S.H, S.W, S.C, S.inv_var
    p.motions, p.ldm, p.inp, p.ldi, p.sparse = bufs["motions"].ptr, S.ldm, ptr(bufs.get("inp")), S.ldi, ptr(bufs.get("sparse"))
    if bwd:
        p.dinp, p.lddi, p.dmotions, p.dsparse = bwd["dinp"].ptr, bwd["dinp"].ld, ptr(bwd.get("dmotions")), ptr(bwd.get("dsparse"))
        p.dkd, p.dks, p.djd, p.djs, p.dbg = [ptr(bwd.get(k)) for k in ("dkd", "dks", "djd", "djs", "dbg")]
    return p


def pm_split(S, inp):
    """inp [B HW][K1 (C + 1)] -> heat [B][K1][H][W], warp [B][K1][C][H][W]"""
    t = inp.view(S.B, S.H, S.W, S.K1, S.C + 1).permute(0, 3, 4, 1, 2)
    return t[:, :, 0], t[:, :, 1:]


def run_pm_fwd(be, S, test, sparse=True, keep=None):
    """-> (the input Bufs, the stored motions [B][K1][H][W][2] fp32, the reference warp at them, its bounds)"""
    B, K1, H, W, C = S.B, S.K1, S.H, S.W, S.C
    bufs = dict(kd=fb(be, S.kd, NAN), ks=fb(be, S.ks, NAN), jd=fb(be, S.jd, NAN), js=fb(be, S.js, NAN), bg=fb(be, S.bg, NAN), src=rb(be, S.src, S.lds, NAN))
    bufs["motions"] = rb(be, unwritten((B * K1 * H * W, 2)), S.ldm, CANARY)
    bufs["inp"] = rb(be, unwritten((B * H * W, K1 * (C + 1))), S.ldi, CANARY)
    bufs["sparse"] = fb(be, unwritten((B, K1, C, H, W)), CANARY) if sparse else None
    p = pm_params(S, bufs)
    rc = be.call("mrfa_prior_motion_fwd", ctypes.byref(p))
    assert rc == 0, be.error()
    mot = bufs["motions"].get().view(B, K1, H, W, 2)
    note(test, "motions", check(mot, S.f["motions"], S.fb["motions"], f"prior_motion motions {test}"))
    heat, val = pm_split(S, bufs["inp"].get())
    note(test, "heat", check(heat, S.f["heat"], S.fb["heat"] + Z, f"prior_motion heat {test}"))
    assert (heat[:, 0] == 0).all(), "heat_0 is 0"
    wp = pm_warp(S, mot)
    wb = warp_bounds(wp)
    assert wb["share"] <= KINK_CAP, (test, wb["share"])
    note(test, "warp", check(val, wp["val"], wb["val"] + Z, f"prior_motion warp {test}"))
    out = ((wp["ix"] < -1 - wb["d_ix"]) | (wp["ix"] > W + wb["d_ix"]) | (wp["iy"] < -1 - wb["d_iy"]) | (wp["iy"] > H + wb["d_iy"])).unsqueeze(2).expand_as(val)
    assert (val[out] == 0).all(), "outside the image the warp is exactly 0"
    if S.det == "normal":
        assert all(out[:, k].all() for k in S.outside), "the block that is to lie fully outside does"
    if sparse:
        assert torch.equal(bufs["sparse"].get().view(B, K1, C, H, W), val), "sparse_deformed is the warp of inp"
    same([bufs[k] for k in ("kd", "ks", "jd", "js", "bg", "src")])
    if keep is not None:
        keep.update(motions=bufs["motions"].bits(), inp=bufs["inp"].bits())
    return bufs, mot, wp, wb


def pm_bwd_bounds(S, r, wp, wb, old, d_dmot=None):
    """-> {name: (reference, bound)} of dks, dkd, djs, djd, dbg on top of the old values.  d_dmot [B][K1][H][W][2]: what dmotions may be off by (the chain)"""
    f, fbd = S.f, S.fb
    HW, C = S.HW, S.C
    sw, sh = 0.5 * S.W, 0.5 * S.H
    b_gix = (4 * C + 6) * U * r["Tx"] + r["Xc"] * wb["d_iy"]
    b_giy = (4 * C + 6) * U * r["Ty"] + r["Xc"] * wb["d_ix"]
    b_dmx = sw * b_gix + U * (r["gix"] * sw).abs() + U * r["dmx"].abs() + wb["kx"] * r["jump_x"]
    b_dmy = sh * b_giy + U * (r["giy"] * sh).abs() + U * r["dmy"].abs() + wb["ky"] * r["jump_y"]
    if d_dmot is not None:
        b_dmx, b_dmy = b_dmx + d_dmot[..., 0], b_dmy + d_dmot[..., 1]
    out = {}
    # ---- k >= 1: the ten sums
    gd, gs = f["gd"], f["gs"]
    inv_var = f["inv_var"]
    bx, by, x, y = b_dmx[:, 1:], b_dmy[:, 1:], r["dmx"][:, 1:].abs(), r["dmy"][:, 1:].abs()
    zx, zy, ezx, ezy = gd["dx"].abs(), gd["dy"].abs(), fbd["ezx"], fbd["ezy"]
    esx, esy, da_s = gauss_err(gs, inv_var)
    t, n1 = r["terms"], (HW - 1) * U
    dh = S.dinp.double().view(S.B, S.H, S.W, S.K1, C + 1)[..., 0].permute(0, 3, 1, 2)[:, 1:].abs()
    heat_b = lambda tt, w, da, ez, z: tt.abs() * (E_EXP + da + 4 * U) + w.abs() * ez + TINY * dh * inv_var * z
    per = [bx, by, bx * zx + x * ezx + U * t[2].abs(), bx * zy + x * ezy + U * t[3].abs(), by * zx + y * ezx + U * t[4].abs(), by * zy + y * ezy + U * t[5].abs(),
           heat_b(t[6], r["wd"], fbd["da_d"], ezx, zx), heat_b(t[7], r["wd"], fbd["da_d"], ezy, zy),
           heat_b(t[8], r["ws"], da_s, esx, gs["dx"].abs()), heat_b(t[9], r["ws"], da_s, esy, gs["dy"].abs())]
    b_acc = torch.stack([p.sum((2, 3)) for p in per], -1) + n1 * r["Sacc"]
    acc, J, bJ = r["acc"], f["J"], fbd["bJ"]
    a, ba = (lambda i: acc[..., i]), (lambda i: b_acc[..., i])
    b_dks = torch.stack([ba(0) + ba(8), ba(1) + ba(9)], -1) + U * r["dks"].abs()
    out["dks"] = acc_add(old["dks"], r["dks"], b_dks)
    kd_b = lambda j0, j1, h: (bJ[j0] * a(0).abs() + J[j0].abs() * ba(0) + bJ[j1] * a(1).abs() + J[j1].abs() * ba(1) + ba(h)
                              + 3 * U * ((J[j0] * a(0)).abs() + (J[j1] * a(1)).abs() + a(h).abs()))
    out["dkd"] = acc_add(old["dkd"], r["dkd"], torch.stack([kd_b(0, 2, 6), kd_b(1, 3, 7)], -1))
    if f["A"] is not None:
        rel_inv = fbd["rel_inv"]
        i00, i01, i10, i11 = [v.abs() for v in f["A"]["inv"]]
        b_js = torch.stack([i00 * ba(2) + i01 * ba(3), i10 * ba(2) + i11 * ba(3), i00 * ba(4) + i01 * ba(5), i10 * ba(4) + i11 * ba(5)], -1)
        out["djs"] = acc_add(old["djs"], r["djs"], b_js + r["Cjs"] * (rel_inv + 3 * U).unsqueeze(-1))
        invT, ST = r["einv"]
        bdJ = torch.stack([torch.stack([ba(2), ba(3)], -1), torch.stack([ba(4), ba(5)], -1)], -2)
        b_jd = (invT @ (ST @ bdJ) @ invT).reshape(*ba(0).shape, 4) + r["Cjd"] * (10 * U + 2 * rel_inv).unsqueeze(-1)
        out["djd"] = acc_add(old["djd"], r["djd"], b_jd)
    if "h" in f:
        hx, hy, hz = [h.abs() for h in f["h"]]
        bh = fbd["bh"]
        x0, y0, bx0, by0 = r["dmx"][:, 0].abs(), r["dmy"][:, 0].abs(), b_dmx[:, 0], b_dmy[:, 0]
        dhx, dhy, dhz = [d.abs() for d in r["dh3"]]
        b_dh = [bx0 / hz + dhx * (bh[2] / hz + E_DIV), by0 / hz + dhy * (bh[2] / hz + E_DIV),
                (bx0 * hx + x0 * bh[0] + by0 * hy + y0 * bh[1]) / (hz * hz) + r["dhzabs"] * (2 * bh[2] / hz + E_DIV + 4 * U)]
        gxa, gya = f["gx"].abs(), f["gy"].abs()
        per9 = []
        for i, (bd, d) in enumerate(zip(b_dh, (dhx, dhy, dhz))):
            per9 += [bd * gxa + d * fbd["egx"] + U * r["t9"][3 * i].abs(), bd * gya + d * fbd["egy"] + U * r["t9"][3 * i + 1].abs(), bd]
        b_bg = torch.stack([p.sum((1, 2)) for p in per9], -1) + n1 * r["Sdbg"]
        out["dbg"] = acc_add(old["dbg"], r["dbg"], b_bg)
    return out


def pm_expect(S, wp, wb, null=(), wrong=""):
    """the backward's reference record and {name: (reference, bound)} for the warp record wp of the stored motions"""
    dheat, dwarp = pm_split(S, S.dinp.double())
    if "dsparse" not in null:
        dwarp = dwarp + S.dsp.double()
    dmot = S.dmot.view(S.B, S.K1, S.H, S.W, 2) if "dmotions" not in null else None
    r = R.prior_bwd(S.f, wp, dheat, dwarp, dmot, wrong=wrong)
    return r, pm_bwd_bounds(S, r, wp, wb, S.g0)


def run_pm_bwd(be, S, test, fwd, null=()):
    """mrfa_prior_motion_bwd on the motions the forward stored.  null: pointers passed as NULL (dmotions, dsparse, dkd, dks, djd (with djs), dbg)"""
    bufs, mot, wp, wb = fwd
    B, K1, H, W, C = S.B, S.K1, S.H, S.W, S.C
    lddi = S.K1 * (C + 1) + 3
    bw = dict(dinp=rb(be, S.dinp, lddi, NAN))
    bw["dmotions"] = rb(be, S.dmot, S.ldm, NAN) if "dmotions" not in null else None
    bw["dsparse"] = fb(be, S.dsp, NAN) if "dsparse" not in null else None
    live = [k for k in ("dkd", "dks") if k not in null]
    if S.jd is not None and "djd" not in null:
        live += ["djd", "djs"]
    if S.bg is not None and "dbg" not in null:
        live += ["dbg"]
    for k in live:
        bw[k] = fb(be, S.g0[k], CANARY)
    fin = dict(bufs, inp=None, sparse=None)
    p = pm_params(S, fin, bw)
    mbits = bufs["motions"].bits()
    rc = be.call("mrfa_prior_motion_bwd", ctypes.byref(p))
    assert rc == 0, be.error()
    r, out = pm_expect(S, wp, wb, null)
    tag = "" if not null else "[" + " ".join(null) + " null]"
    for k in live:
        ref, bound = out[k]
        note(test, k + tag, check(bw[k].get().view(ref.shape), ref, bound, f"prior_motion {k} {test} {tag}"))
    assert torch.equal(bufs["motions"].bits(), mbits), "the backward changed the stored motions"
    same([bufs[k] for k in ("kd", "ks", "jd", "js", "bg", "src")] + [bw["dinp"], bw["dmotions"], bw["dsparse"]])


PM_NULLS = [(), ("dmotions",), ("dsparse",), ("dkd",), ("dks",), ("djd",), ("dbg",)]
PM_VARIANTS = [dict(jac=True, bg="near"), dict(jac=False, bg="none"), dict(jac=True, bg="eye"), dict(jac=True, bg="near", det="small")]


def pm_cases(be, shape, test):
    for i, v in enumerate(PM_VARIANTS):
        S = pm_set(*shape, **v)
        fwd = run_pm_fwd(be, S, test, sparse=i != 1)
        for null in (PM_NULLS if i == 0 else [()]):
            run_pm_bwd(be, S, test, fwd, null=null)


@pytest.mark.parametrize("shape", PM_SETS, ids=lambda s: "x".join(map(str, s)))
def test_prior_motion(shape):
    """non-square images; Jacobians given and null; bg null, near identity, the exact identity; |det jd| in [0.5, 1.5] and near 0.1; keypoint pairs well inside, with
    border bands, fully outside; sparse null and given; the backward with each optional pointer null in turn and all given"""
    test = "prior_motion " + "x".join(map(str, shape))
    pm_cases(Library(), shape, test)
    report(test, TAG)


def pm_exact_case(be, test):
    """15 x 11, the identity motion (bg the exact identity matrix; keypoint 0 with kd = ks = 0 and null Jacobians): the centre column and row sample exact integers.
    Every fp32 step of their coordinate is exact (asserted), so they are no kink pixels and are compared in full, dbg included"""
    S = pm_set(*PM_ODD, jac=False, bg="eye", exact=True)
    fwd = run_pm_fwd(be, S, test)
    _, mot, wp, wb = fwd
    H, W = S.H, S.W
    for k in (0, 1):
        assert (wp["ix"][:, k, :, W // 2] == W // 2).all() and wb["exact_x"][:, k, :, W // 2].all(), "the centre column is an exact integer"
        assert (wp["iy"][:, k, H // 2, :] == H // 2).all() and wb["exact_y"][:, k, H // 2, :].all(), "the centre row is an exact integer"
        assert not (wb["kx"][:, k, :, W // 2].any() or wb["ky"][:, k, H // 2, :].any())
    run_pm_bwd(be, S, test, fwd)


def test_prior_motion_exact_integer_positions():
    test = "prior_motion exact integers"
    pm_exact_case(Library(), test)
    report(test, TAG)


def pm_big_case(be, test):
    S = pm_set(*PM_BIG, jac=True, bg="near")
    fwd = run_pm_fwd(be, S, test, sparse=False)
    run_pm_bwd(be, S, test, fwd)


def test_prior_motion_grid_stride_second_trip():
    """224 x 216, K = 10: 1 064 448 work items, the forward's second trip; one backward (189 pixels per thread)"""
    test = "prior_motion 224x216"
    assert steps(2 * 11 * 224 * 216) == 2
    pm_big_case(Library(), test)
    report(test, TAG)


def run_chain_pm(be, S, test):
    """prior_motion_fwd -> softmax_combine_fwd -> softmax_combine_bwd -> prior_motion_bwd on the buffers each stage left, every stage against the float64
    reference of the EXACT stages before it: its own bound plus what the bounds before it allow (motions: b_mot into the deformation, into dm_k and -- as
    (W / 2) b_mot, (H / 2) b_mot of coordinate error, kink window included -- into the warp and its gradient; the mask: b_mask; dmotions: its bound)"""
    B, K1, H, W, C = S.B, S.K1, S.H, S.W, S.C
    Q = sc_set(K1, B, H, W)
    bufs, mot, _, _ = run_pm_fwd(be, S, test)
    M, b_mot = S.f["motions"], S.fb["motions"]
    d_mo = b_mot.permute(0, 2, 3, 1, 4)
    wp = pm_warp(S, M)
    wb = warp_bounds(wp, extra=(0.5 * W * b_mot[..., 0], 0.5 * H * b_mot[..., 1]))
    assert wb["share"] <= KINK_CAP, (test, wb["share"])
    _, val = pm_split(S, bufs["inp"].get())
    note(test, "warp", check(val, wp["val"], wb["val"] + Z, f"chain warp {test}"))
    # ---- softmax_combine forward on the motions buffer
    ldl = K1 + 1
    bl = rb(be, Q.logit, ldl, NAN)
    bdef, bmask, bnchw = fb(be, unwritten((B * H * W, 2)), CANARY), fb(be, unwritten((B, K1, H, W)), CANARY), fb(be, unwritten((B, K1, H, W)), CANARY)
    mbits = bufs["motions"].bits()
    rc = be.call("mrfa_softmax_combine_fwd", bl.ptr, ldl, bufs["motions"].ptr, S.ldm, B, H, W, K1, bdef.ptr, bmask.ptr, bnchw.ptr)
    assert rc == 0, be.error()
    r = R.softmax_combine_fwd(Q.logit.view(B, H, W, K1), M)
    b_mask, b_def = sc_fwd_bounds(r, K1, d_mo)
    note(test, "mask", check(bmask.get().view(B, K1, H, W), r["mask"], b_mask, f"chain mask {test}"))
    note(test, "deformation", check(bdef.get().view(B, H, W, 2), r["deformation"], b_def, f"chain deformation {test}"))
    # ---- softmax_combine backward on the mask and motions buffers
    bdd, bdk, bdn = fb(be, Q.ddef, NAN), fb(be, Q.dmask, NAN), fb(be, Q.dnchw, NAN)
    bdl, bdm = rb(be, Q.dl0, ldl, CANARY), rb(be, Q.dm0, S.ldm, CANARY)
    kbits = bmask.bits()
    rc = be.call("mrfa_softmax_combine_bwd", bufs["motions"].ptr, S.ldm, B, H, W, K1, bmask.ptr, bdd.ptr, bdk.ptr, bdn.ptr, bdl.ptr, ldl, bdm.ptr)
    assert rc == 0, be.error()
    rbk = R.softmax_combine_bwd(M, r["mask"], Q.ddef, Q.dmask, Q.dnchw)
    rbk["dd"] = Q.ddef.double()
    ref_l, b_l, ref_m, b_m = sc_bwd_bounds(rbk, K1, Q.dl0.view(B, H, W, K1), Q.dm0.view(B, K1, H, W, 2), d_mask=b_mask.permute(0, 2, 3, 1), d_mo=d_mo)
    note(test, "dlogit", check(bdl.get().view(B, H, W, K1), ref_l, b_l, f"chain dlogit {test}"))
    note(test, "dmotions", check(bdm.get().view(B, K1, H, W, 2), ref_m, b_m, f"chain dmotions {test}"))
    assert torch.equal(bmask.bits(), kbits) and torch.equal(bufs["motions"].bits(), mbits), "an input changed"
    same((bl, bdd, bdk, bdn))
    # ---- prior_motion backward on the motions and dmotions buffers
    bw = dict(dinp=rb(be, S.dinp, S.K1 * (C + 1), NAN), dmotions=bdm, dsparse=fb(be, S.dsp, NAN))
    live = ["dkd", "dks"] + (["djd", "djs"] if S.jd is not None else []) + (["dbg"] if S.bg is not None else [])
    for k in live:
        bw[k] = fb(be, S.g0[k], CANARY)
    dbits = bdm.bits()
    p = pm_params(S, dict(bufs, inp=None, sparse=None), bw)
    rc = be.call("mrfa_prior_motion_bwd", ctypes.byref(p))
    assert rc == 0, be.error()
    dheat, dwarp = pm_split(S, S.dinp.double())
    r4 = R.prior_bwd(S.f, wp, dheat, dwarp + S.dsp.double(), ref_m)
    out = pm_bwd_bounds(S, r4, wp, wb, S.g0, d_dmot=b_m)
    for k in live:
        ref, bound = out[k]
        note(test, k, check(bw[k].get().view(ref.shape), ref, bound, f"chain {k} {test}"))
    assert torch.equal(bdm.bits(), dbits) and torch.equal(bufs["motions"].bits(), mbits), "an input changed"
    same([bufs[k] for k in ("kd", "ks", "jd", "js", "bg", "src")] + [bw["dinp"], bw["dsparse"]])


PM_CHAIN = [(PM_SETS[0], 0), (PM_SETS[2], 3), (PM_SETS[0], 1)]     # (even sizes: under a perturbed motion an exact integer of an odd image is a kink like any other)


@pytest.mark.parametrize("shape,variant", PM_CHAIN, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_chain_prior_motion_softmax_combine(shape, variant):
    test = "chain prior_motion " + "x".join(map(str, shape)) + f" v{variant}"
    run_chain_pm(Library(), pm_set(*shape, **PM_VARIANTS[variant]), test)
    report(test, TAG)


# ================================================================================================================== determinism
DETERMINISTIC = {
    "prior_motion_fwd": lambda be, keep: run_pm_fwd(be, pm_set(*PM_SETS[0]), "determinism", keep=keep),
    "softmax_combine": lambda be, keep: run_sc(be, sc_set(11, 2, 9, 7), "determinism", ldl=12, ldm=4, keep=keep),
    "kp_head": lambda be, keep: run_kh(be, kh_set(1, 16, 17, 10, "peak"), "determinism", ldl=12, ldj=6, keep=keep),
    "kp_gaussian_fwd": lambda be, keep: run_gauss(be, gauss_set(2, 10, 7, 5, 12, 0.01), "determinism", keep=keep),
}


@pytest.mark.parametrize("which", sorted(DETERMINISTIC))
def test_kernels_without_atomics_are_bit_identical_run_to_run(which):
    """both forwards of the stage, softmax_combine (forward and backward) and kp_head (forward: a workgroup reduction in a fixed order; backward) write every element
    from one thread: two launches agree bit for bit, canaries and all.  The atomic paths (dpos over b, the parameter gradients onto a non-zero start) are bounded above"""
    runs = []
    for _ in range(2):
        keep = {}
        DETERMINISTIC[which](Library(), keep)
        runs.append(keep)
    a, b = runs
    assert a.keys() == b.keys() and len(a) > 0
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), f"{which}: {k} differs between two launches"


# ================================================================================================================== refusals
def refusal_cases(be):
    """(entry point, arguments, the Bufs involved): every call stays inside its buffers even if it were launched, except the null-pointer and K1 = 33 cases, which
    csrc/prior.hip refuses at this commit (read there: the first MRFA_CHECK_ARG of each entry point) before anything is launched"""
    B, K, H, W = 1, 2, 3, 4
    n = B * H * W
    t = lambda *s: torch.rand(*s) - 0.5
    kp, out, dout = fb(be, t(B, K + 1, 2), NAN), rb(be, t(n, K + 1), K + 1, CANARY), rb(be, t(n, K + 1), K + 1, NAN)
    dkp = fb(be, t(B, K + 1, 2), CANARY)
    yield "kp_gaussian_fwd", (kp.ptr, None, B, K + 1, H, W, 0.1, out.ptr, K), (kp, out)                 # ldo < K
    yield "kp_gaussian_fwd", (kp.ptr, None, B, K, 1, W, 0.1, out.ptr, K), (kp, out)                     # H = 1
    yield "kp_gaussian_bwd", (kp.ptr, B, K + 1, H, W, 0.1, dout.ptr, K, dkp.ptr, None), (kp, dout, dkp)  # lddo < K
    K1 = 3
    lg, mo = rb(be, t(n, K1), K1, NAN), rb(be, t(B * K1 * n, 2), 2, NAN)
    de, mk, nc = fb(be, t(n, 2), CANARY), fb(be, t(B, K1, H, W), CANARY), fb(be, t(B, K1, H, W), CANARY)
    dl = rb(be, t(n, K1), K1, CANARY)
    sc = (lg, mo, de, mk, nc, dl)
    yield "softmax_combine_fwd", (lg.ptr, K1 - 1, mo.ptr, 2, B, H, W, K1, de.ptr, mk.ptr, nc.ptr), sc   # ldl < K1
    yield "softmax_combine_fwd", (lg.ptr, K1, mo.ptr, 1, B, H, W, K1, de.ptr, mk.ptr, nc.ptr), sc       # ldm < 2
    yield "softmax_combine_fwd", (lg.ptr, K1, mo.ptr, 2, 0, H, W, K1, de.ptr, mk.ptr, nc.ptr), sc       # B = 0
    yield "softmax_combine_fwd", (lg.ptr, K1, mo.ptr, 2, B, H, -1, K1, de.ptr, mk.ptr, nc.ptr), sc      # W < 0
    yield "softmax_combine_fwd", (lg.ptr, 33, mo.ptr, 2, B, H, W, 33, de.ptr, mk.ptr, nc.ptr), sc       # K1 = 33 (refused by the first check)
    yield "softmax_combine_fwd", (None, K1, mo.ptr, 2, B, H, W, K1, de.ptr, mk.ptr, nc.ptr), sc         # null logit (the first check)
    yield "softmax_combine_bwd", (mo.ptr, 2, B, H, W, K1, mk.ptr, None, nc.ptr, None, dl.ptr, K1 - 1, None), sc     # lddl < K1
    yield "softmax_combine_bwd", (mo.ptr, 1, B, H, W, K1, mk.ptr, None, nc.ptr, None, dl.ptr, K1, None), sc         # ldm < 2
    yield "softmax_combine_bwd", (mo.ptr, 2, B, 0, W, K1, mk.ptr, None, nc.ptr, None, dl.ptr, K1, None), sc         # H = 0
    hl, jm = rb(be, t(n, K), K, NAN), rb(be, t(n, 4), 4, NAN)
    hk, hj, hs = fb(be, t(B, K, 2), CANARY), fb(be, t(B, K, 4), CANARY), fb(be, t(B, K, 2), CANARY)
    dk, dj = fb(be, t(B, K, 2), NAN), fb(be, t(B, K, 4), NAN)
    hdl, hdj = rb(be, t(n, K), K, CANARY), rb(be, t(n, 4), 4, CANARY)
    kh = (hl, jm, hk, hj, hs, dk, dj, hdl, hdj)
    yield "kp_head_fwd", (hl.ptr, K - 1, jm.ptr, 4, B, H, W, K, 0.1, hk.ptr, hj.ptr, hs.ptr), kh        # ldl < K
    yield "kp_head_fwd", (hl.ptr, K, jm.ptr, 3, B, H, W, K, 0.1, hk.ptr, hj.ptr, hs.ptr), kh            # ldj < 4 with maps
    bwd = lambda **o: tuple({**dict(a=hl.ptr, ldl=K, jm=jm.ptr, ldj=4, B=B, H=H, W=W, K=K, T=0.1, kp=hk.ptr, jac=hj.ptr, st=hs.ptr, dk=dk.ptr, dj=dj.ptr, dl=hdl.ptr,
                                         lddl=K, djm=hdj.ptr, lddj=4), **o}.values())
    yield "kp_head_bwd", bwd(H=1, W=H * W), kh                                                        # H = 1 (the same pixels as one row)
    yield "kp_head_bwd", bwd(jac=None), kh                                                              # maps and djac without the forward's jac
    yield "kp_head_bwd", bwd(ldl=K - 1), kh
    yield "kp_head_bwd", bwd(lddl=K - 1), kh
    yield "kp_head_bwd", bwd(ldj=3), kh
    yield "kp_head_bwd", bwd(lddj=3), kh


def prior_refusals(be):
    """mrfa_prior_motion_bwd with djd / djs but no jd, and with dbg but no bg"""
    S = pm_set(*PM_SETS[1], jac=False, bg="none")
    B, K1, H, W, C = S.B, S.K1, S.H, S.W, S.C
    bufs = dict(kd=fb(be, S.kd, NAN), ks=fb(be, S.ks, NAN), jd=None, js=None, bg=None, src=rb(be, S.src, S.lds, NAN),
                motions=rb(be, torch.zeros(B * K1 * H * W, 2), S.ldm, NAN))
    for extra in (("djd",), ("djs",), ("dbg",)):
        bw = dict(dinp=rb(be, S.dinp, S.K1 * (C + 1), NAN), dkd=fb(be, S.g0["dkd"], CANARY), dks=fb(be, S.g0["dks"], CANARY))
        for k in extra:
            bw[k] = fb(be, S.g0[k], CANARY)
        p = pm_params(S, dict(bufs), bw)
        yield "prior_motion_bwd", (ctypes.byref(p),), tuple(bufs[k] for k in ("kd", "ks", "src", "motions")) + tuple(bw.values()), p


def refusals(be):
    for name, args, bufs, *hold in list(refusal_cases(be)) + list(prior_refusals(be)):
        rc = be.call("mrfa_" + name, *args)
        assert rc != 0, f"{name}{args}: accepted"
        assert name in be.error(), (name, be.error())
        assert all(b.untouched() for b in bufs), f"{name}: a refused call wrote"


def test_prior_kernels_refuse_what_they_do_not_take():
    """the return code is non-zero, mrfa_last_error names the entry point, outputs and inputs are bit-identical"""
    refusals(Library())
