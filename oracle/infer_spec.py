"""Reference functions of the inference-loop entries of include/mrfa_hip.h (mrfa_kp_pose_dist, mrfa_frame_metrics, mrfa_frames_from_u8, mrfa_frames_to_u8)
on numpy arrays: the arithmetic of each entry before its one rounding (float64) or with a rounding per operation in the header's order (fp32).  The ABI
emulator (oracle/capi_emulator.py) decodes the pointers, refuses what the entries refuse and calls these; the tests call them directly.  numpy only."""
import math

import numpy as np

# ---------------------------------------------------------------- mrfa_kp_pose_dist


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


# ---------------------------------------------------------------- mrfa_frame_metrics
TAPS = 11
C1, C2 = 0.01 ** 2, 0.03 ** 2


def gauss_window() -> np.ndarray:
    """the eleven fp32 numbers that define the window, as float64: g_i = exp(-(i - 5)^2 / 4.5) / sum in float64, rounded to fp32"""
    g = np.exp(-(np.arange(TAPS, dtype=np.float64) - 5.0) ** 2 / 4.5)
    return (g / g.sum()).astype(np.float32).astype(np.float64)


def _window(x: np.ndarray, g: np.ndarray) -> np.ndarray:
    """(..., H, W) -> (..., H - 10, W - 10): the separable "valid" window as two sums of shifted slices"""
    H, W = x.shape[-2:]
    rows = sum(g[i] * x[..., i:i + H - TAPS + 1, :] for i in range(TAPS))
    return sum(g[i] * rows[..., :, i:i + W - TAPS + 1] for i in range(TAPS))


def ssim_map(p: np.ndarray, t: np.ndarray) -> np.ndarray:
    """float64 S of every window of (N,C,H,W) float64 images: (N,C,H-10,W-10)"""
    g = gauss_window()
    mx, my = _window(p, g), _window(t, g)
    sxx, syy, sxy = _window(p * p, g) - mx * mx, _window(t * t, g) - my * my, _window(p * t, g) - mx * my
    return (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def frame_metrics(p: np.ndarray, t: np.ndarray, want_ssim: bool) -> np.ndarray:
    """(N,4) float64 rows {l1, mse, ssim or 0, 0} of (N,C,H,W) images: the specification before its one rounding"""
    p, t = p.astype(np.float64), t.astype(np.float64)
    out = np.zeros((p.shape[0], 4))
    with np.errstate(all="ignore"):
        d = p - t
        out[:, 0] = np.abs(d).mean(axis=(1, 2, 3))
        out[:, 1] = (d * d).mean(axis=(1, 2, 3))
        if want_ssim:
            out[:, 2] = ssim_map(p, t).mean(axis=(1, 2, 3))
    return out


# ---------------------------------------------------------------- mrfa_frames_from_u8 / mrfa_frames_to_u8: fp32, one rounding per operation
F = np.float32


def from_u8(src: np.ndarray) -> np.ndarray:
    """uint8 (N,H,W,Cin) -> fp32 (N,3,H,W): fl32(v) * fl32(1 / 255); grey in all three planes, alpha dropped"""
    v = src[..., [0, 0, 0]] if src.shape[3] == 1 else src[..., :3]
    return np.ascontiguousarray((v.astype(F) * F(1.0 / 255.0)).transpose(0, 3, 1, 2))


def quantise(s: np.ndarray, rounding: int) -> np.ndarray:
    """fp32 samples -> bytes: p = s * 255 in fp32, rint (ties to even) or trunc, clamped to [0,255]; NaN 0, +inf 255, -inf 0"""
    with np.errstate(all="ignore"):
        p = s.astype(F) * F(255.0)
        r = np.rint(p) if rounding == 0 else np.trunc(p)
        r = np.where(r > 0, np.minimum(r, F(255.0)), F(0.0))                              # (a NaN compares false: 0)
    return r.astype(np.uint8)


def disc_index(kp: np.ndarray, H: int, W: int, radius: float) -> np.ndarray:
    """(K,2) keypoints of one image -> (H,W) int: the largest k whose disc covers the pixel, -1 for none; fp32, each operation rounded once"""
    hit = np.full((H, W), -1, dtype=np.int64)
    rr, cc = np.arange(H, dtype=F)[:, None], np.arange(W, dtype=F)[None, :]
    r2 = F(radius) * F(radius)
    with np.errstate(all="ignore"):
        for k in range(kp.shape[0]):
            x, y = F(kp[k, 0]), F(kp[k, 1])
            if not (np.isfinite(x) and np.isfinite(y)):
                continue
            cx, cy = (F(W) * (x + F(1.0))) * F(0.5), (F(H) * (y + F(1.0))) * F(0.5)
            dy, dx = rr - cy, cc - cx
            hit[(dy * dy + dx * dx) < r2] = k
    return hit


def compose_tile(src, kp, radius, colors, border, rounding) -> np.ndarray:
    """one tile: fp32 (N,3,H,W) -> uint8 (N,H,W,3) with discs and border"""
    N, _, H, W = src.shape
    out = np.ascontiguousarray(quantise(src, rounding).transpose(0, 2, 3, 1))
    if kp is not None:
        cq = quantise(colors, rounding)
        for n in range(N):
            hit = disc_index(kp[n], H, W, radius)
            out[n][hit >= 0] = cq[hit[hit >= 0]]
    if border:
        out[:, :, 0, :] = 255
        out[:, :, W - 1, :] = 255
    return out
