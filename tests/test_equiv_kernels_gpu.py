"""The equivariance entries of libmrfa_hip.so (include/mrfa_equiv_hip.h) called directly on the MI355X: operands inside wider buffers whose surroundings are
watched (tests/kernel_check.py), results against the fp64 reference tests/ref_equiv.py within its per-element bounds n * U * f(|.|) -- nothing in a bound
comes from the kernels.  The shapes cover a single point, less than a wave, a count that is no multiple of 64, more than a wave, more points than the one
workgroup has threads, and a params tensor beyond what the loss kernels stage in LDS (MRFA_EQUIV_LDS_PARAMS).

A sign() may flip where its argument is smaller than the argument's own bound: those elements are left out of the backward comparison, at most 1 % of a
case; the seeds are such that the reference leaves out none, which test_the_seeds_leave_no_element_out checks without a GPU.

MEASURED on an MI355X, largest err / bound over all cases (each test prints its own through report()): value 0.08, term 0.46, d_kp_d 0.29, d_kp_t 0.21,
d_jac_d 0.59, d_jac_t 0.47; frame warp 0.16 on the smooth image, 0.07 on noise."""
import numpy as np
import pytest
import torch

import mrfa_amd.equivariance  # noqa: F401
from mrfa_amd import equiv_hip, hip
from tests import ref_equiv as R
from tests.kernel_check import CANARY, NAN, Buf, check, note, report

SHAPES = [(1, 1), (1, 10), (3, 7), (8, 10), (5, 60)]
POINTS = [0, 1, 25, 64]
# (B, K, P, seed, w_j, on_lines, upstream): every shape with every P, then the legs
RESEED = {(5, 60, 64): 1143}                               # (seed 143 puts one |I - V| entry at 0.8 of its bound)
CASES = [(B, K, P, RESEED.get((B, K, P), 100 + 10 * i + j), 10.0, False, False) for i, (B, K) in enumerate(SHAPES) for j, P in enumerate(POINTS)]
CASES += [(3, 7, 25, 201, 0.0, False, False),             # no Jacobian term: the NULL set
          (2, 10, 25, 202, 10.0, True, False),            # keypoints on control rows and columns and on a control point
          (3, 7, 25, 203, 10.0, False, True),             # g_value and g_term other than 1
          (3, 7, 0, 204, 0.0, False, True),
          (33, 2, 64, 205, 10.0, False, False)]           # B P = 2112 > MRFA_EQUIV_LDS_PARAMS: params read from global memory
W_E = 10.0


def _ids(c):
    return f"B{c[0]}K{c[1]}P{c[2]}" + ("-nojac" if c[4] == 0 else "") + ("-lines" if c[5] else "") + ("-g" if c[6] else "")


def control_points(P, rng):
    side = int(round(P ** 0.5))
    if side * side == P and side > 1:                       # the reference's grid: make_coordinate_grid((side, side)) in fp32
        return R.coordinate_grid(side, side).reshape(P, 2).copy()
    return rng.uniform(-1, 1, (P, 2)).astype(np.float32)


def draw(case):
    B, K, P, seed, w_j, on_lines, upstream = case
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    d = dict(theta=f(np.eye(2, 3)[None] + 0.05 * rng.standard_normal((B, 2, 3))), points=control_points(P, rng),
             params=f(0.005 * rng.standard_normal((B, P))), kp_d=f(rng.uniform(-0.9, 0.9, (B, K, 2))), kp_t=f(rng.uniform(-0.9, 0.9, (B, K, 2))),
             jac_d=f(np.eye(2) + 0.2 * rng.standard_normal((B, K, 2, 2))), jac_t=f(np.eye(2) + 0.2 * rng.standard_normal((B, K, 2, 2))))
    if on_lines:
        q = d["points"]
        d["kp_t"][0, 0] = q[P // 2]
        d["kp_t"][0, 1, 0] = q[1, 0]
        d["kp_t"][-1, 2, 1] = q[-1, 1]
        d["kp_t"][-1, 3] = (q[3, 0], q[7, 1])
    d["g_value"] = np.float32(0.37) if upstream else np.float32(1.0)
    d["g_term"] = f(rng.standard_normal((B, K, 2, 2))) if upstream else np.ones((B, K, 2, 2), np.float32)
    if w_j == 0:
        d["jac_d"] = d["jac_t"] = d["g_term"] = None
    return d


def reference(case, d):
    """(forward, backward, masks): the masks say which backward elements have every sign they depend on decided beyond its argument's bound"""
    w_j = case[4]
    pts = (d["points"], d["params"]) if case[2] else (None, None)
    fwd = R.loss_fwd(d["kp_d"], d["jac_d"], d["kp_t"], d["jac_t"], d["theta"], *pts, W_E, w_j, R.EPS32)
    bwd = R.loss_bwd(d["kp_d"], d["jac_d"], d["kp_t"], d["jac_t"], d["theta"], *pts, W_E, w_j, float(d["g_value"]), d["g_term"], R.EPS32)
    r_ok = np.abs(fwd["r"].v) > fwd["r"].bound                                                   # (B,K,2)
    e_ok = (np.abs(fwd["e"].v) > fwd["e"].bound).all((-1, -2)) if w_j else np.ones(r_ok.shape[:2], bool)
    both = r_ok.all(-1) & e_ok
    masks = dict(d_kp_d=r_ok, d_kp_t=np.broadcast_to(both[..., None], r_ok.shape), d_jac_d=np.broadcast_to(e_ok[..., None, None], r_ok.shape + (2,)),
                 d_jac_t=np.broadcast_to(e_ok[..., None, None], r_ok.shape + (2,)))
    return fwd, bwd, masks


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_seeds_leave_no_element_out(case):
    d = draw(case)
    fwd, bwd, masks = reference(case, d)
    assert all(m.all() for m in masks.values())
    assert np.isfinite(fwd["value"].v) and all(v is None or np.isfinite(v.bound).all() for v in bwd.values())
    if case[5]:                                                                                 # the points on control lines really are
        q, p = d["points"], d["kp_t"]
        assert (p[0, 0] == q[case[2] // 2]).all() and (p[0, 1, 0] == q[:, 0]).any() and (p[-1, 2, 1] == q[:, 1]).any()


# ------------------------------------------------------------------------------------------------------------------------------------- on the device
def _in(a, lead):
    """an input (or None) inside a NaN-filled buffer, `lead` floats in and with a watched tail"""
    return None if a is None else Buf(torch.from_numpy(np.ascontiguousarray(a, np.float32)).reshape(1, -1), 1, a.size, NAN, lead=lead, gap=5)


def _out(n, lead):
    return Buf(torch.full((1, n), CANARY), 1, n, CANARY, lead=lead, gap=3)


def _p(b):
    return None if b is None else b.ptr


def _t(vm, shape=None):
    return torch.from_numpy(np.array(np.broadcast_to(vm, shape) if shape else vm)).reshape(1, -1)


class Launch:
    """the operands of one case on the device and the two calls"""

    def __init__(self, case, d):
        B, K, P = case[:3]
        self.case, self.n = case, B * K
        names = ("kp_d", "jac_d", "kp_t", "jac_t", "theta", "points", "params", "g_term")
        self.i = {k: _in(d[k] if (k not in ("points", "params") or P) else None, lead=1 + j) for j, k in enumerate(names)}
        self.i["g_value"] = _in(np.array([d["g_value"]]), lead=3)
        self.jac = case[4] != 0
        self.fresh()

    def fresh(self):
        n, j = self.n, self.jac
        self.o = dict(value=_out(1, 2), term=_out(4 * n, 1) if j else None, d_kp_d=_out(2 * n, 3), d_jac_d=_out(4 * n, 2) if j else None,
                      d_kp_t=_out(2 * n, 1), d_jac_t=_out(4 * n, 5) if j else None)

    def fwd(self, **over):
        B, K, P, _, w_j = self.case[:5]
        i, o = self.i, self.o
        a = dict(jac_d=_p(i["jac_d"]), jac_t=_p(i["jac_t"]), P=P, term=_p(o["term"]), w_j=w_j)
        a.update(over)
        return equiv_hip.lib().mrfa_equiv_loss_fwd(hip.stream_ptr(), B, K, i["kp_d"].ptr, a["jac_d"], i["kp_t"].ptr, a["jac_t"], i["theta"].ptr, _p(i["points"]),
                                                   _p(i["params"]), a["P"], W_E, a["w_j"], o["value"].ptr, a["term"])

    def bwd(self, **over):
        B, K, P, _, w_j = self.case[:5]
        i, o = self.i, self.o
        a = dict(jac_d=_p(i["jac_d"]), g_term=_p(i["g_term"]), P=P, d_jac_t=_p(o["d_jac_t"]))
        a.update(over)
        return equiv_hip.lib().mrfa_equiv_loss_bwd(hip.stream_ptr(), B, K, i["kp_d"].ptr, a["jac_d"], i["kp_t"].ptr, _p(i["jac_t"]), i["theta"].ptr,
                                                   _p(i["points"]), _p(i["params"]), a["P"], W_E, w_j, i["g_value"].ptr, a["g_term"], o["d_kp_d"].ptr,
                                                   _p(o["d_jac_d"]), o["d_kp_t"].ptr, a["d_jac_t"])

    def inputs_untouched(self):
        return all(b is None or b.untouched() for b in self.i.values())

    def outputs_untouched(self):
        return all(b is None or b.untouched() for b in self.o.values())


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_loss_forward_and_backward(case):
    test = "loss " + _ids(case)
    d = draw(case)
    fwd, bwd, masks = reference(case, d)
    L = Launch(case, d)
    assert L.fwd() == 0, equiv_hip.last_error()
    assert L.bwd() == 0, equiv_hip.last_error()
    note(test, "value", check(L.o["value"].get(), _t(fwd["value"].v, (1,)), _t(fwd["value"].bound, (1,)), f"value {test}"))
    if L.jac:
        note(test, "term", check(L.o["term"].get(), _t(fwd["term"].v), _t(fwd["term"].bound), f"term {test}"))
    for k in ("d_kp_d", "d_kp_t", "d_jac_d", "d_jac_t"):
        if bwd[k] is None:
            assert L.o[k] is None
            continue
        m = masks[k]
        assert (~m).sum() <= 0.01 * m.size, f"{k}: {(~m).sum()} of {m.size} elements left out"
        note(test, k, check(L.o[k].get(), _t(bwd[k].v), _t(bwd[k].bound), f"{k} {test}", mask=_t(m)))
    assert L.inputs_untouched(), "an input changed"
    first = {k: b.bits() for k, b in L.o.items() if b is not None}
    L.fresh()                                                    # new CANARY-filled outputs: every element is written again, to the same bits
    assert L.fwd() == 0 and L.bwd() == 0
    for k, bits in first.items():
        assert torch.equal(L.o[k].bits(), bits), f"{k}: two runs differ"
    report(test, tag="equiv")


@pytest.mark.gpu
def test_refused_calls_leave_every_output_untouched():
    case = (3, 7, 25, 203, 10.0, False, True)
    L = Launch(case, draw(case))
    err = equiv_hip.last_error
    assert L.fwd(P=65) != 0 and "P must be in [0, 64], not 65" in err()
    assert L.bwd(P=65) != 0 and "P must be in [0, 64], not 65" in err()
    assert L.fwd(term=None) != 0 and "NULL together or not at all (2 of 3 are set)" in err()
    assert L.fwd(jac_d=None) != 0 and "2 of 3" in err()
    assert L.bwd(d_jac_t=None) != 0 and "4 of 5 are set" in err()
    assert L.bwd(g_term=None, jac_d=None) != 0 and "3 of 5" in err()
    assert L.fwd(w_j=0.0) != 0 and "set exactly when w_j != 0" in err()
    assert L.fwd(P=-1) != 0
    lib = equiv_hip.lib()
    i, o = L.i, L.o
    assert lib.mrfa_equiv_loss_fwd(hip.stream_ptr(), 0, 7, i["kp_d"].ptr, None, i["kp_t"].ptr, None, i["theta"].ptr, None, None, 0, W_E, 0.0, o["value"].ptr,
                                   None) != 0 and "B and K must be >= 1" in err()
    assert lib.mrfa_equiv_loss_fwd(hip.stream_ptr(), 3, 7, i["kp_d"].ptr, None, i["kp_t"].ptr, None, i["theta"].ptr, None, i["params"].ptr, 25, W_E, 0.0,
                                   o["value"].ptr, None) != 0 and "null points or params" in err()
    assert lib.mrfa_equiv_loss_fwd(hip.stream_ptr(), 3, 7, i["kp_d"].ptr, None, i["kp_t"].ptr, None, i["theta"].ptr, None, None, 0, W_E, 0.0, None,
                                   None) != 0 and "null value" in err()
    # the frame warp: H = 1, too many points, a null frame
    img, out = _in(np.zeros((1, 1, 1, 8), np.float32), 1), _out(8, 1)
    warp = lambda H, W, P, src=img.ptr: lib.mrfa_equiv_warp_frame(hip.stream_ptr(), src, 1, 1, H, W, i["theta"].ptr, i["points"].ptr, i["params"].ptr, P, out.ptr)
    assert warp(1, 8, 25) != 0 and "H and W must be >= 2" in err()
    assert warp(8, 1, 25) != 0 and "H and W must be >= 2" in err()
    assert warp(2, 4, 65) != 0 and "P must be in [0, 64], not 65" in err()
    assert warp(2, 4, 25, src=None) != 0 and "null pointer" in err()
    torch.cuda.synchronize()
    assert L.outputs_untouched() and L.inputs_untouched() and out.untouched() and img.untouched()


# ------------------------------------------------------------------------------------------------------------------------------------- the frame warp
FRAMES = [(1, 1, 2, 2), (1, 3, 5, 7), (3, 1, 33, 17), (2, 3, 64, 64)]
DRAWS = {"vox": dict(sigma_affine=0.05, P=25), "far": dict(sigma_affine=1.0, P=25), "affine": dict(sigma_affine=0.05, P=0)}


def images(N, Cc, H, W, rng):
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    smooth = np.stack([np.stack([0.5 + 0.4 * np.sin(3.0 * xx + c + n) * np.cos(2.0 * yy - c) for c in range(Cc)]) for n in range(N)])
    return {"smooth": smooth.astype(np.float32), "noise": rng.uniform(0, 1, (N, Cc, H, W)).astype(np.float32)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DRAWS))
@pytest.mark.parametrize("shape", FRAMES, ids=lambda s: "x".join(map(str, s)))
def test_frame_warp(shape, name):
    N, Cc, H, W = shape
    test = f"warp {'x'.join(map(str, shape))} {name}"
    rng = np.random.default_rng(300 + H + len(name))
    P = DRAWS[name]["P"]
    theta = (np.eye(2, 3)[None] + DRAWS[name]["sigma_affine"] * rng.standard_normal((N, 2, 3))).astype(np.float32)
    points, params = control_points(P, rng), (0.005 * rng.standard_normal((N, P))).astype(np.float32)
    bt, bq, bc = _in(theta, 1), (_in(points, 2) if P else None), (_in(params, 3) if P else None)
    for kind, img in images(N, Cc, H, W, rng).items():
        ref, bound = R.warp_frame(img, theta, points if P else None, params if P else None, R.EPS32)
        bi, bo = _in(img, 1), _out(img.size, 3)
        call = lambda o: equiv_hip.lib().mrfa_equiv_warp_frame(hip.stream_ptr(), bi.ptr, N, Cc, H, W, bt.ptr, _p(bq), _p(bc), P, o.ptr)
        assert call(bo) == 0, equiv_hip.last_error()
        note(test, kind, check(bo.get(), _t(ref), _t(bound), f"{test} {kind}"))
        again = _out(img.size, 3)
        assert call(again) == 0 and torch.equal(again.bits(), bo.bits()), "two runs differ"
        assert bi.untouched() and bt.untouched() and (bq is None or (bq.untouched() and bc.untouched())), "an input changed"
    if name == "far":                                             # the draw does leave [-1, 1] by more than a period (2) of the reflection somewhere
        t = R.warp_points(theta, points, params, np.broadcast_to(R.coordinate_grid(H, W).reshape(1, H * W, 2), (N, H * W, 2)), R.EPS32).v
        assert np.abs(t).max() > 3.0
    report(test, tag="equiv")
