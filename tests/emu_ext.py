"""CPU specification of the entries of include/mrfa_hip_ext.h (mrfa_amd.hip._EXT_SIGNATURES): ExtEmulator adds them to the ABI emulator of
include/mrfa_hip.h (oracle/capi_emulator.py), which keeps mirroring that header alone; emulated_hip_ext installs it the way tests/emu.emulated_hip installs
the Emulator."""
import contextlib
import ctypes as C
import math

import numpy as np

from mrfa_amd import hip
from oracle.capi_emulator import Emulator
from tests.emu import Counting

MAXK = 64


def hull_area(q: np.ndarray) -> float:
    """area of the convex hull of (K,2) float64 points by Andrew's monotone chain: sort by (x, y), a lower and an upper chain that pop while the turn is
    not strictly counter-clockwise (collinear and duplicate points never stay), the shoelace sum over the chains' edges"""
    pts = [tuple(p) for p in q.tolist()]
    order = list(range(len(pts)))
    for i in range(len(pts)):                                 # the kernel's insertion sort: a NaN compares false and travels to the front
        j = i
        while j > 0:
            w, v = pts[order[j - 1]], pts[i]
            if w[0] < v[0] or (w[0] == v[0] and w[1] <= v[1]):
                break
            order[j] = order[j - 1]
            j -= 1
        order[j] = i
    acc = 0.0
    for chain_order in (order, order[::-1]):
        chain = []
        for i in chain_order:
            v = pts[i]
            while len(chain) >= 2:
                o, a = pts[chain[-2]], pts[chain[-1]]
                if not ((a[0] - o[0]) * (v[1] - o[1]) - (a[1] - o[1]) * (v[0] - o[0]) <= 0.0):
                    break
                chain.pop()
            chain.append(i)
        for s, t in zip(chain[:-1], chain[1:]):
            acc += pts[s][0] * pts[t][1] - pts[t][0] * pts[s][1]
    return 0.5 * acc


def centre_and_area(p: np.ndarray):
    """(centred points, hull area, all inputs finite) of (K,2) float64 points, in the entry's order"""
    with np.errstate(all="ignore"):
        q = p - p.sum(axis=0) / p.shape[0]
        return q, hull_area(q), bool(np.isfinite(p).all())


def pose_dist(kd: np.ndarray, ks: np.ndarray, rep: int):
    """float64 (dist (B), area (B)) of frames kd (B,K,2) against sources ks (B/rep,K,2): the specification of mrfa_kp_pose_dist before its one rounding"""
    B = kd.shape[0]
    dist, area = np.full(B, np.inf), np.empty(B)
    src = [centre_and_area(s) for s in ks.astype(np.float64)]
    with np.errstate(all="ignore"):
        for n in range(B):
            qs, As, fin_s = src[n // rep]
            qd, Ad, fin_d = centre_and_area(kd[n].astype(np.float64))
            area[n] = Ad
            if fin_s and fin_d and math.isfinite(As) and math.isfinite(Ad) and As > 0 and Ad > 0:
                d = qd / math.sqrt(Ad) - qs / math.sqrt(As)
                acc = float((d * d).sum())
                dist[n] = acc if math.isfinite(acc) else np.inf                # finite or +inf, never NaN
    return dist, area


def _f32(ptr: int, n: int) -> np.ndarray:
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr))


class ExtEmulator(Emulator):
    def mrfa_kp_pose_dist(self, stream, kp_d, kp_s, B, rep, K, dist_out, area_out, state):
        bad = None
        if not (kp_d and kp_s):
            bad = "null keypoint pointer"
        elif not (dist_out or area_out or state):
            bad = "dist_out, area_out and state are all null (nothing to compute)"
        elif B < 1 or rep < 1 or K < 1:
            bad = f"B, rep and K must be >= 1 (B {B}, rep {rep}, K {K})"
        elif B % rep:
            bad = f"rep must divide B (B {B}, rep {rep})"
        elif not 3 <= K <= MAXK:
            bad = f"a hull needs 3 <= K <= {MAXK} keypoints (K {K})"
        elif kp_d % 8 or kp_s % 8 or any(p and p % 4 for p in (dist_out, area_out, state)):
            bad = "keypoints must be 8-byte aligned (vector loads), the outputs and the state 4-byte aligned"
        if bad:
            self._err = ("kp_pose_dist: " + bad).encode()
            return 1
        Bs = B // rep
        dist64, area64 = pose_dist(_f32(kp_d, B * K * 2).reshape(B, K, 2), _f32(kp_s, Bs * K * 2).reshape(Bs, K, 2), rep)
        with np.errstate(over="ignore"):
            dist, area = dist64.astype(np.float32), area64.astype(np.float32)                 # the one rounding
        if dist_out:
            _f32(dist_out, B)[:] = dist
        if area_out:
            _f32(area_out, B)[:] = area
        if state:
            best, words = _f32(state, Bs * 4).reshape(Bs, 4), np.ctypeslib.as_array((C.c_int * (Bs * 4)).from_address(state)).reshape(Bs, 4)
            for s in range(Bs):
                for j in range(rep):
                    if dist[s * rep + j] < best[s, 0]:                                        # strict: ties keep the earliest, NaN and +inf never win
                        best[s, 0] = dist[s * rep + j]
                        words[s, 1] = words[s, 2] + j
                words[s, 2] += rep
        return 0


@contextlib.contextmanager
def emulated_hip_ext(counting=False):
    """installs an ExtEmulator as the loaded library and yields it; counting: behind tests.emu.Counting"""
    old_lib, old_stream = hip._lib, hip.stream_ptr
    lib = ExtEmulator()
    hip._lib = Counting(lib) if counting else lib
    hip.stream_ptr = lambda: 0
    try:
        yield hip._lib
    finally:
        hip._lib, hip.stream_ptr = old_lib, old_stream
