"""Streaming animation of ONE source by many driving frames (the reference's make_animation loop, demo.py:47-73 /
animate_ddp.py:88-105) with everything that depends only on the source computed once: KPDetector(source), the 1/4-scale
source, the generator's feature pyramid and the source structure keys (~38 GF of 375 per frame and
one encoder pass).  Optionally the per-frame program is replayed as a hipGraph."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .modules.dense_motion import repeat_frames
from .modules.raft import check_corr


def _check_cache_dtype(cache_dtype):
    if cache_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"cache_dtype must be torch.float32 or torch.bfloat16, not {cache_dtype}")
    return cache_dtype


def _expand_kp(kp: dict, T: int) -> dict:
    """the keypoint dict of Bs images for the Bs T frames of a clip group: element n of the result is element n // T"""
    return kp if T == 1 else {k: (repeat_frames(v, T) if torch.is_tensor(v) else v) for k, v in kp.items()}


def _frames_per_source(b: int, bs: int, what: str) -> int:
    if b < bs or b % bs != 0:
        raise ValueError(f"{what}: the driving batch {b} is no multiple of the source batch {bs} (every source needs the same number of frames, "
                         "consecutive: frame n belongs to source n // T)")
    return b // bs


class Animator:
    def __init__(self, model: nn.Module, graph: bool = False, cache_dtype: torch.dtype = torch.float32, corr: str = "volume", relative: bool = False,
                 adapt_movement_scale: bool = False, use_relative_jacobian: Optional[bool] = None):
        """model: mrfa_amd.train.HotPath or mrfa_amd.modules.model.MRFA (attributes encoder / dense_motion / decoder / down).
        cache_dtype: storage of the cached source feature pyramid (RaftFlow.encode_source(feature_dtype=)); torch.bfloat16 halves what the cache holds
        and what the per-frame warps gather, at the cost of one rounding of the source features.
        corr: RaftFlow.forward(corr=): "direct" correlates each looked-up window where it is read and builds no correlation volume per frame.
        relative: the driving keypoints go through normalize_kp against an initial driving frame (set_source(source, driving_initial) or
        set_driving_initial(frame), one frame per source) before the motion network sees them, as one kernel of the frame program (relative_kp);
        adapt_movement_scale: the displacement is scaled by sqrt(hull area(source kp)) / sqrt(hull area(initial kp)) of batch element 0, kept on the device;
        use_relative_jacobian: None follows `relative`.  relative=False ignores the other two, like normalize_kp, and is the absolute Animator call for call.
        After set_source of Bs sources a call takes Bs T driving frames for any T >= 1, frame n driving source n // T: one batch-(Bs T) program against the
        one cached copy of every source (the frames of a clip, T at a time).  graph=True keeps one captured program per T it has seen."""
        self.m = model.eval()
        self.use_graph = graph
        self.cache_dtype = _check_cache_dtype(cache_dtype)
        self.corr = check_corr(corr)
        self.relative = bool(relative)
        self.adapt_movement_scale = self.relative and bool(adapt_movement_scale)
        self.relative_jacobian = self.relative and bool(relative if use_relative_jacobian is None else use_relative_jacobian)
        self.source = None
        self._graphs: dict = {}                               # T -> (graph, static driving frames, static output)
        self._kp_s_rep: dict = {}                             # T -> source keypoints expanded to the Bs T frames
        # relative mode: keypoints of the initial driving frames (Bs of them) and the movement scale (one float on the device); a new initial frame or a
        # new source drops the captured programs, which have the old tensors' addresses in them
        self._kp_init: Optional[dict] = None
        self._scale: Optional[torch.Tensor] = None

    @property
    def _g(self) -> Optional[torch.cuda.CUDAGraph]:
        """the captured one-frame-per-source program (T == 1), if any"""
        return self._graphs[1][0] if 1 in self._graphs else None

    @torch.no_grad()
    def set_source(self, source: torch.Tensor, driving_initial: Optional[torch.Tensor] = None):
        """driving_initial (relative mode): set_driving_initial(driving_initial) after the source.  A new source drops the captured programs AND an initial
        frame set earlier (the movement scale depends on both): pass it here or call set_driving_initial again."""
        m = self.m
        self.source = source
        self.kp_s = m.encoder(source)
        self.img_down = m.down(source)
        self.cache = m.decoder.encode_source(self.kp_s["kp"], self.img_down, source, feature_dtype=self.cache_dtype)
        self._graphs, self._kp_s_rep = {}, {}
        self._kp_init = self._scale = None
        if driving_initial is not None:
            self.set_driving_initial(driving_initial)

    @torch.no_grad()
    def set_driving_initial(self, frame: torch.Tensor):
        """frame (Bs,3,H,W): the driving frame whose keypoints the relative motion is measured from, one per source (the first frame of the driving clip in
        demo.py:47-73; demo.py:150-157's best frame).  Drops the captured programs, like set_source: the next call of each T captures again."""
        if not self.relative:
            raise ValueError("Animator.set_driving_initial: this Animator was built with relative=False and has no use for an initial driving frame")
        assert self.source is not None, "call set_source(source) first"
        if frame.shape[0] != self.source.shape[0]:
            raise ValueError(f"Animator.set_driving_initial: one initial driving frame per source ({frame.shape[0]} frames, {self.source.shape[0]} sources)")
        kp = {k: v for k, v in self.m.encoder(frame).items() if torch.is_tensor(v)}
        if self.relative_jacobian and "jacobian" not in kp:
            raise ValueError("Animator(use_relative_jacobian=True): the keypoint detector returns no 'jacobian'")
        self._kp_init, self._graphs = kp, {}
        if self.adapt_movement_scale:
            # normalize_kp's scale, from batch element 0 as there; stays on the device (no .item(): nothing here waits for the host)
            self._scale = (torch.sqrt(_hull_area(self.kp_s["kp"][0])) / torch.sqrt(_hull_area(kp["kp"][0]))).reshape(1)

    def _kp_source(self, T: int) -> dict:
        if T not in self._kp_s_rep:                           # once per T, not per call
            self._kp_s_rep[T] = _expand_kp(self.kp_s, T)
        return self._kp_s_rep[T]

    @torch.no_grad()
    def _frame(self, driving):
        m = self.m
        T = _frames_per_source(driving.shape[0], self.source.shape[0], "Animator")
        kp_d = m.encoder(driving)
        if self.relative:                                     # kp_s and kp_init stay at the source batch: the kernel reads entry n // T
            kp_d = relative_kp(self.kp_s, kp_d, self._kp_init, scale=self._scale, rep=T, use_relative_jacobian=self.relative_jacobian)
        dm = m.dense_motion(self.source, kp_d, self._kp_source(T))
        out, _, _ = m.decoder(self.kp_s["kp"], kp_d["kp"], dm, img=self.img_down, img_full=self.source, source_cache=self.cache, corr=self.corr)
        return out

    @torch.no_grad()
    def __call__(self, driving: torch.Tensor) -> torch.Tensor:
        assert self.source is not None, "call set_source(source) first"
        if self.relative and self._kp_init is None:
            raise RuntimeError("Animator(relative=True): no initial driving frame yet -- call set_driving_initial(frame) or set_source(source, driving_initial)")
        T = _frames_per_source(driving.shape[0], self.source.shape[0], "Animator")
        if not self.use_graph:
            return self._frame(driving)
        if T not in self._graphs:                             # capture the program of T frames per source once per source and T
            from . import graph_replay_safe
            graph_replay_safe("Animator(graph=True)")
            drv = driving.clone()
            eager = self._frame(drv).clone()                  # packs / tables outside the graph
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = self._frame(drv)
            for k in range(3):                                # first AND later replays against the eager frame (mrfa_amd/graph.py)
                g.replay()
                torch.cuda.synchronize()
                diff = (out - eager).abs()
                d, dm = float(diff.max()), float(diff.mean())
                # run-to-run summation-order noise (split-K atomics) reaches ~1e-4 on single border pixels of sharply warped frames;
                # a mis-ordered graph is wrong everywhere (stale or zero inputs): gate the mean tightly, the max loosely
                if not (dm <= 2e-5 and d <= 5e-3):
                    raise RuntimeError(f"Animator: hipGraph replay {k} differs from the eager frame (max |diff| {d:.3e}, mean {dm:.3e})")
            self._graphs[T] = (g, drv, out)
        g, drv, out = self._graphs[T]
        drv.copy_(driving)
        g.replay()
        return out


# ----------------------------------------------------------------------------------------------- callers of the path
def _hull_area(pts: torch.Tensor) -> torch.Tensor:
    """Area of the convex hull of (N,2) points, on the device and without a host round trip (the reference calls
    scipy.spatial.ConvexHull(...).volume on the host, animate_ddp.py:20-21): a directed edge (i,j) belongs to the
    counter-clockwise hull iff no point lies strictly to its right; the shoelace sum over those edges is the area.  N = 10:
    900 cross products.  Points in general position (no three hull points collinear), as qhull assumes after joggling."""
    d = pts[None, :, :] - pts[:, None, :]                                   # d[i,j] = p_j - p_i
    rel = pts[None, None, :, :] - pts[:, None, None, :]                     # rel[i,.,k] = p_k - p_i
    cross = d[:, :, None, 0] * rel[:, :, :, 1] - d[:, :, None, 1] * rel[:, :, :, 0]       # (i,j,k)
    scale = pts.abs().max().clamp_min(1e-12) ** 2
    on_hull = (cross >= -1e-7 * scale).all(dim=2) & ~torch.eye(pts.shape[0], dtype=torch.bool, device=pts.device)
    shoelace = pts[:, None, 0] * pts[None, :, 1] - pts[None, :, 0] * pts[:, None, 1]      # p_i x p_j
    return 0.5 * (shoelace * on_hull).sum()


def _inv2x2(m: torch.Tensor) -> torch.Tensor:
    a, b, c, d = m[..., 0, 0], m[..., 0, 1], m[..., 1, 0], m[..., 1, 1]
    det = a * d - b * c
    return torch.stack([torch.stack([d, -b], dim=-1), torch.stack([-c, a], dim=-1)], dim=-2) / det[..., None, None]


def normalize_kp(kp_source, kp_driving, kp_driving_initial, adapt_movement_scale=False, use_relative_movement=False,
                 use_relative_jacobian=False):
    """Relative-motion transfer of an animation loop: the driving keypoints' displacement (and Jacobian change) since the
    first driving frame, applied to the source keypoints.  reference: animate_ddp.py:17-37 (same arguments and result; the
    movement scale sqrt(hull area(source)) / sqrt(hull area(driving_initial)) is taken from batch element 0, as there)."""
    scale = 1
    if adapt_movement_scale:
        scale = torch.sqrt(_hull_area(kp_source['kp'][0])) / torch.sqrt(_hull_area(kp_driving_initial['kp'][0]))
    kp_new = dict(kp_driving)
    if use_relative_movement:
        kp_new['kp'] = (kp_driving['kp'] - kp_driving_initial['kp']) * scale + kp_source['kp']
        if use_relative_jacobian:
            diff = torch.matmul(kp_driving['jacobian'], _inv2x2(kp_driving_initial['jacobian']))
            kp_new['jacobian'] = torch.matmul(diff, kp_source['jacobian'])
    return kp_new


def relative_kp(kp_source: dict, kp_driving: dict, kp_driving_initial: dict, scale: Optional[torch.Tensor] = None, rep: int = 1,
                use_relative_jacobian: bool = True) -> dict:
    """normalize_kp(use_relative_movement=True) as ONE kernel launch (mrfa_kp_relative_fwd) for a clip: kp_driving holds B = Bs rep frames, kp_source and
    kp_driving_initial the Bs sources / initial frames, frame n reads entry n // rep (no repeated copies).  scale: the movement scale as a one-element
    fp32 tensor ON THE DEVICE (the kernel reads it there: nothing waits for the host), None for 1.  Every other key of kp_driving passes through;
    use_relative_jacobian=False passes the driving Jacobian through as well.  Inference only."""
    ins = [kp_source["kp"], kp_driving["kp"], kp_driving_initial["kp"]]
    if use_relative_jacobian:
        for name, kp in (("kp_source", kp_source), ("kp_driving", kp_driving), ("kp_driving_initial", kp_driving_initial)):
            if "jacobian" not in kp:
                raise ValueError(f"relative_kp(use_relative_jacobian=True): {name} has no 'jacobian' (a keypoint detector without Jacobians: pass "
                                 "use_relative_jacobian=False)")
        ins += [kp_source["jacobian"], kp_driving["jacobian"], kp_driving_initial["jacobian"]]
    if torch.is_grad_enabled() and any(t.requires_grad for t in ins):
        raise RuntimeError("relative_kp: the relative keypoints have no backward, not legal in a recording (training) program; normalize_kp is the "
                           "differentiable torch form")
    from .engine import Ctx
    e = Ctx(kp_driving["kp"].device, train=False, record=False)
    jacs = dict(jd=kp_driving["jacobian"], j0=kp_driving_initial["jacobian"], js=kp_source["jacobian"]) if use_relative_jacobian else {}
    kp, jac = e.kp_relative(kp_driving["kp"], kp_driving_initial["kp"], kp_source["kp"], scale=scale, rep=rep, **jacs)
    kp_new = dict(kp_driving)
    kp_new["kp"] = kp
    if jac is not None:
        kp_new["jacobian"] = jac
    return kp_new


_INF_BITS = 0x7F800000          # +inf as the int32 that shares its bits


def pose_state(bs: int, device) -> torch.Tensor:
    """a fresh running argmin for bs sources (mrfa_kp_pose_dist's state, include/mrfa_hip_ext.h): (bs,4) int32 rows {best distance as fp32 bits = +inf,
    best index 0, frames seen 0, pad}.  Column 1 is the answer; a clip with no finite distance leaves it at 0, as the reference's loop does."""
    st = torch.zeros(bs, 4, dtype=torch.int32, device=device)
    st[:, 0] = _INF_BITS
    return st


class BestFrameSearch:
    """demo.py:75-98 (find_best_frame) for the clips of Bs sources, on the model's own keypoints: the driving frame whose pose -- keypoints centred and
    divided by the square root of their hull area -- is closest to the source's.  set_source(source), add(frames) group after group, result().  add is the
    keypoint detector plus ONE launch (mrfa_kp_pose_dist) that also keeps the running argmin and the frame count on the device: nothing waits for the host
    until result().  graph=True keeps one captured program per group size T (the frame offset lives in the state, so one program serves every group); as
    with Animator(graph=True), do not run the model's modules eagerly between two replays of a capture."""

    def __init__(self, model: nn.Module, graph: bool = False):
        self.m = model.eval()
        self.use_graph = graph
        self.kp_s: Optional[torch.Tensor] = None
        self.state: Optional[torch.Tensor] = None
        self._graphs: dict = {}                               # T -> (graph, static driving frames)

    @torch.no_grad()
    def set_source(self, source: torch.Tensor):
        """the keypoints of the Bs sources and a fresh state; drops the captured programs (they hold the old tensors' addresses)"""
        self.kp_s = self.m.encoder(source)["kp"]
        self.state = pose_state(source.shape[0], source.device)
        self._graphs = {}

    def reset(self):
        """a new clip against the same sources: the state is refilled in place, the captured programs stay valid"""
        assert self.state is not None, "call set_source(source) first"
        self.state.copy_(pose_state(self.state.shape[0], self.state.device))

    @torch.no_grad()
    def _group(self, frames: torch.Tensor, state: torch.Tensor, want_dist: bool):
        from .engine import Ctx
        T = _frames_per_source(frames.shape[0], self.kp_s.shape[0], "BestFrameSearch")
        kp_d = self.m.encoder(frames)["kp"]
        return Ctx(kp_d.device, train=False, record=False).kp_pose_dist(kp_d, self.kp_s, rep=T, state=state, want_dist=want_dist)[0]

    @torch.no_grad()
    def add(self, frames: torch.Tensor):
        """the next Bs T frames of the clips, frame n of source n // T (any T >= 1, groups of different sizes in any order)"""
        assert self.state is not None, "call set_source(source) first"
        T = _frames_per_source(frames.shape[0], self.kp_s.shape[0], "BestFrameSearch")
        if not self.use_graph:
            self._group(frames, self.state, False)
            return
        if T not in self._graphs:                             # capture once per T, as Animator.__call__ does
            from . import graph_replay_safe
            graph_replay_safe("BestFrameSearch(graph=True)")
            drv = frames.clone()
            eager = self._group(drv, pose_state(self.state.shape[0], self.state.device), True).clone()      # packs / tables outside the graph; a scratch state
            torch.cuda.synchronize()
            kept = self.state.clone()                         # the check replays below advance the state: put it back, whatever they find
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                dist = self._group(drv, self.state, True)
            try:
                for k in range(3):
                    g.replay()
                    torch.cuda.synchronize()
                    # the detector's split-K sums differ run to run in their last bits; a mis-ordered graph reads stale or zero keypoints
                    if not (torch.isfinite(dist) == torch.isfinite(eager)).all() or not torch.allclose(dist, eager, rtol=1e-3, atol=1e-6, equal_nan=True):
                        raise RuntimeError(f"BestFrameSearch: hipGraph replay {k} differs from the eager distances ({dist.tolist()} vs {eager.tolist()})")
            finally:
                self.state.copy_(kept)
            self._graphs[T] = (g, drv)
        g, drv = self._graphs[T]
        drv.copy_(frames)
        g.replay()

    def result(self) -> list:
        """the index of the best frame of each source's clip: the one read of the host"""
        assert self.state is not None, "call set_source(source) first"
        return self.state[:, 1].tolist()


@torch.no_grad()
def find_best_frame(model: nn.Module, source: torch.Tensor, driving_video: torch.Tensor, frames_per_call: int = 1, graph: bool = False) -> list:
    """demo.py:75-98 on a driving clip (B,3,T,H,W): per source the index of the frame whose normalised keypoints are closest to the source's.  The keypoints
    are the model's K, not 68 face landmarks, so the index can differ from the reference's on the same clip.  frames_per_call frames per group (a shorter last
    group at its own size); one host read, at the end."""
    fpc = _check_frames_per_call(frames_per_call)
    search = BestFrameSearch(model, graph=graph)
    search.set_source(source)
    n = driving_video.shape[2]
    for t0 in range(0, n, fpc):
        search.add(_clip_group(driving_video, t0, min(fpc, n - t0)))
    return search.result()


def psnr(img1: torch.Tensor, img2: torch.Tensor):
    """20 log10(1 / sqrt(mse)) for images in [0,1].  reference: reconstruction.py:13-19"""
    mse = torch.mean((img1 - img2) ** 2)
    if mse == 0:
        return float('inf')
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def _psnr_of_mse(mse):
    """infer.psnr on float64 numpy mean squared errors: 20 log10(1 / sqrt(mse)), inf where mse == 0"""
    import numpy as np
    with np.errstate(divide="ignore"):
        return np.where(mse == 0, np.inf, 20.0 * np.log10(1.0 / np.sqrt(mse)))


def ssim(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """SSIM of image n of img1 against image n of img2, both (N,C,H,W) contiguous fp32 in [0,1] on one device -> (N,) fp32 on that device: Wang et al.
    2004 with an 11-tap Gaussian window (sigma 1.5), no padding, C1 = 0.01^2, C2 = 0.03^2, the mean over channels and windows (include/mrfa_hip_ext.h,
    mrfa_frame_metrics).  The reference declares a loss_list_ssim and never fills it (reconstruction.py:43)."""
    from .engine import Ctx
    return Ctx(img1.device, train=False, record=False).frame_metrics(img1, img2, want_ssim=True)[:, 2]


class ClipMetrics:
    """The full-reference metrics of a clip, kept on the device: add(pred, target) group after group, result() once.  add is ONE entry call
    (mrfa_frame_metrics) for the N frames of a group; its (N,4) rows {l1, mse, ssim, 0} stay on the device in the order added, and nothing waits for the
    host until result().  ssim=False leaves the SSIM windows out (its column is 0) and takes frames of any size; with SSIM, min(H, W) >= 11."""

    def __init__(self, ssim: bool = True):
        self.want_ssim = bool(ssim)
        self.rows: list = []

    @torch.no_grad()
    def add(self, pred: torch.Tensor, target: torch.Tensor):
        """frame n of pred (N,C,H,W) against frame n of target, both contiguous fp32 on one device"""
        from .engine import Ctx
        self.rows.append(Ctx(pred.device, train=False, record=False).frame_metrics(pred, target, want_ssim=self.want_ssim))

    def __len__(self) -> int:
        return sum(r.shape[0] for r in self.rows)

    def result(self) -> dict:
        """the one read of the host: {'l1', 'mse', 'psnr', 'ssim'}, float64 numpy arrays with one value per frame added, in that order.
        psnr = 20 log10(1 / sqrt(mse)), inf where mse == 0 (infer.psnr, reconstruction.py:13-19)"""
        import numpy as np
        rows = torch.cat(self.rows, dim=0).cpu().numpy().astype(np.float64) if self.rows else np.zeros((0, 4))
        return {"l1": rows[:, 0].copy(), "mse": rows[:, 1].copy(), "psnr": _psnr_of_mse(rows[:, 1]), "ssim": rows[:, 2].copy()}


def _check_frames_per_call(frames_per_call) -> int:
    if not isinstance(frames_per_call, int) or frames_per_call < 1:
        raise ValueError(f"frames_per_call must be an integer >= 1, not {frames_per_call!r}")
    return frames_per_call


def _clip_group(video: torch.Tensor, t0: int, T: int) -> torch.Tensor:
    """frames t0 .. t0 + T - 1 of a clip (Bs,3,.,H,W) as a driving batch (Bs T,3,H,W): the frames of one source consecutive"""
    g = video[:, :, t0:t0 + T]
    return g.permute(0, 2, 1, 3, 4).reshape(g.shape[0] * g.shape[2], g.shape[1], g.shape[3], g.shape[4]).contiguous()


@torch.no_grad()
def reconstruction(model: nn.Module, video: torch.Tensor, graph: bool = False, cache_dtype: torch.dtype = torch.float32, corr: str = "volume",
                   frames_per_call: int = 1, metrics: str = "host"):
    """The reference's reconstruction loop (reconstruction.py:52-70) on one clip: source = frame 0, driving = every frame t,
    metrics mean|out - driving| and PSNR per frame.  video: (B,3,T,H,W) in [0,1].  The source is fixed for the whole clip, so
    the source half of the path is computed once (Animator).  frames_per_call: that many frames of the clip run as one batch against the one cached
    source (a shorter last group at its own size).
    metrics="host": torch operations per frame, three host reads each.  Returns {'prediction': (B,3,T,H,W), 'l1': [T], 'psnr': [T]}.
    metrics="device": one ClipMetrics.add per group of frames (row s T + j of a group: source s, frame t0 + j) and ONE host read at the end of the clip;
    SSIM comes with it (min(H, W) >= 11).  Returns 'prediction' as above; 'l1', 'psnr', 'ssim': [T] floats -- the mean over sources of the per-source l1
    (the host path's number up to rounding), the PSNR of the mean per-source mse (likewise) and the mean per-source SSIM --; and 'per_source':
    {'l1', 'mse', 'psnr', 'ssim'}, float64 numpy arrays (B,T)."""
    fpc = _check_frames_per_call(frames_per_call)
    if metrics not in ("host", "device"):
        raise ValueError(f"reconstruction: metrics must be \"host\" or \"device\", not {metrics!r}")
    anim = Animator(model, graph=graph, cache_dtype=cache_dtype, corr=corr)
    anim.set_source(video[:, :, 0].contiguous())
    bs = video.shape[0]
    if metrics == "device":
        return _reconstruction_device_metrics(anim, video, fpc)
    preds, l1, ps = [], [], []
    for t0 in range(0, video.shape[2], fpc):
        T = min(fpc, video.shape[2] - t0)
        outs = anim(_clip_group(video, t0, T)).view(bs, T, *video.shape[1:2], *video.shape[3:])
        for j in range(T):
            driving = video[:, :, t0 + j].contiguous()
            out = outs[:, j].clone()
            preds.append(out)
            l1.append(float(torch.abs(out - driving).mean()))
            ps.append(float(psnr(driving, out)))
    return {"prediction": torch.stack(preds, dim=2), "l1": l1, "psnr": ps}


def _reconstruction_device_metrics(anim: Animator, video: torch.Tensor, fpc: int) -> dict:
    """reconstruction(metrics="device") behind its set_source: the clip in groups, the metrics of each group from one entry call on the Animator's output
    where it lies (before the next call overwrites a captured program's output: the same stream), one host read after the last group"""
    import numpy as np
    bs, n = video.shape[0], video.shape[2]
    cm, preds, sizes = ClipMetrics(ssim=True), [], []
    for t0 in range(0, n, fpc):
        T = min(fpc, n - t0)
        driving = _clip_group(video, t0, T)
        outs = anim(driving).contiguous()
        cm.add(outs, driving)
        preds.append(outs.view(bs, T, *outs.shape[1:]).clone())
        sizes.append(T)
    res = cm.result()
    per_source, row = {}, np.cumsum([0] + [bs * T for T in sizes])
    for name, v in res.items():                               # rows of group g: (bs, T_g) -> (bs, n), the groups side by side
        per_source[name] = np.concatenate([v[row[g]:row[g + 1]].reshape(bs, T) for g, T in enumerate(sizes)], axis=1)
    return {"prediction": torch.cat(preds, dim=1).permute(0, 2, 1, 3, 4).contiguous(),
            "l1": per_source["l1"].mean(axis=0).tolist(), "psnr": _psnr_of_mse(per_source["mse"].mean(axis=0)).tolist(),
            "ssim": per_source["ssim"].mean(axis=0).tolist(), "per_source": per_source}


@torch.no_grad()
def make_animation(model: nn.Module, source: torch.Tensor, driving_video: torch.Tensor, relative: bool = True,
                   adapt_movement_scale: bool = False, graph: bool = False, cache_dtype: torch.dtype = torch.float32, corr: str = "volume",
                   frames_per_call: int = 1, initial_frame=0):
    """demo.py:47-73 / animate_ddp.py:88-105: animate ONE source by the motion of a driving clip (B,3,T,H,W); with
    relative=True the driving keypoints go through normalize_kp against driving frame `initial_frame` (0: the first, as the reference's loop; the index of
    demo.py:150-157's best frame gives that branch's clip in one pass, since every frame depends on the initial one alone).  initial_frame: an index for
    every source, a sequence of B indices (one per source), or "best": find_best_frame(model, source, driving_video) with the same frames_per_call and
    graph, each source measured from its own best frame (relative=False has no initial frame and searches for none).  frames_per_call: that many
    frames of the clip run as one batch against the one cached source (a shorter last group at its own size).  graph=True replays one captured program per
    group size.  One loop over an Animator(relative=relative, ...) in every mode.  Returns (B,3,T,H,W)."""
    fpc = _check_frames_per_call(frames_per_call)
    bs, n = source.shape[0], driving_video.shape[2]
    if isinstance(initial_frame, str) and initial_frame == "best":
        initial_frame = find_best_frame(model, source, driving_video, frames_per_call=fpc, graph=graph) if relative else 0
    per_source = isinstance(initial_frame, (list, tuple))
    indices = list(initial_frame) if per_source else [initial_frame]
    if (per_source and len(indices) != bs) or not all(isinstance(i, int) and 0 <= i < n for i in indices):
        raise ValueError(f"initial_frame must be the index of one of the clip's {n} frames, a sequence of {bs} such indices (one per source) or \"best\", "
                         f"not {initial_frame!r}")
    anim = Animator(model, graph=graph, cache_dtype=cache_dtype, corr=corr, relative=relative, adapt_movement_scale=adapt_movement_scale)
    if per_source:                                            # Animator.set_driving_initial takes one frame per source: frame indices[s] of source s
        initial = torch.stack([driving_video[s, :, i] for s, i in enumerate(indices)], dim=0)
    else:
        initial = driving_video[:, :, initial_frame].contiguous()
    anim.set_source(source, initial if relative else None)
    outs = []
    for t0 in range(0, n, fpc):
        T = min(fpc, n - t0)
        out = anim(_clip_group(driving_video, t0, T))
        out = out.view(bs, T, *out.shape[1:])
        outs.extend(out[:, j].clone() for j in range(T))
    return torch.stack(outs, dim=2)
