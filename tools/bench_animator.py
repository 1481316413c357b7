"""Per-frame time of the streaming animation loop (source-side work cached) vs the full per-pair forward, hipGraph replays.

    python tools/bench_animator.py                                  # 256^2, B = 1 and 8, the volume correlation (the original report)
    python tools/bench_animator.py --corr direct                    # the same with RaftFlow.forward(corr="direct") in the Animator
    python tools/bench_animator.py --corr volume direct --size 512 --batch 1 --rounds 5
                                                                    # alternating rounds of both modes in ONE process: median and spread per mode
    python tools/bench_animator.py --corr volume direct --raft-forward --size 512 --batch 4
                                                                    # the RaftFlow forward of bench.py's 512^2 inference configuration, graphed
    python tools/bench_animator.py --frames 1 2 4 8 --corr volume direct --rounds 7
                                                                    # a clip of ONE source, T frames per call: the clip Animator (one cached source), the
                                                                    # replicated-source batch-T Animator and the per-frame Animator, alternating round by round
    python tools/bench_animator.py --relative --frames 1 8 --corr volume direct --rounds 7
                                                                    # relative motion (normalize_kp against the first driving frame, adapted scale): the graphed
                                                                    # relative Animator, the graphed absolute Animator and the eager torch loop, alternating
    python tools/bench_animator.py --best-frame --frames 8 --rounds 7
                                                                    # the best-frame search (BestFrameSearch.add: keypoint detector + mrfa_kp_pose_dist) per frame,
                                                                    # captured and eager, beside the keypoint detector alone on the same groups, alternating
"""
import argparse
import copy
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfa_amd.graph import GraphedForward  # noqa: E402
from mrfa_amd.infer import Animator  # noqa: E402
from mrfa_amd.train import VOX1, HotPath  # noqa: E402
from mrfa_amd.utils.prng import det_uniform, fill_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--corr", nargs="+", choices=("volume", "direct"), default=["volume"], help="RaftFlow correlation mode(s); two modes alternate round by round")
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
ap.add_argument("--rounds", type=int, default=1, help="timed rounds per mode (20 frames each); > 1 prints median and min-max")
ap.add_argument("--raft-forward", action="store_true", help="time the graphed RaftFlow forward on fixed prior inputs instead of the Animator frame")
ap.add_argument("--no-graph", action="store_true")
ap.add_argument("--frames", type=int, nargs="+", default=None, metavar="T",
                help="frames of one source per call: times Animator calls of T frames against one cached source, against the source replicated T times, and "
                     "per frame (replaces the --batch report)")
ap.add_argument("--relative", action="store_true",
                help="relative motion with an adapted movement scale: times the relative Animator, the absolute Animator and the eager loop that calls "
                     "normalize_kp per group of frames, T = --frames (default 1) frames of one source per call")
ap.add_argument("--best-frame", action="store_true",
                help="the best-frame search of a clip of one source, T = --frames (default 8) frames per call: BestFrameSearch.add captured and eager, and the "
                     "keypoint detector alone on the same groups captured and eager, alternating round by round")
a = ap.parse_args()

dev = torch.device("cuda", 0)
cfg = copy.deepcopy(VOX1)
cfg["raft_flow"]["size"] = a.size


def timed(fn, n=20):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def summary(ts):
    return f"{statistics.median(ts):.3f} ms" + (f" (median of {len(ts)}, {min(ts):.3f} - {max(ts):.3f})" if len(ts) > 1 else "")


def raft_forward_steps(B):
    """the RaftFlow forward of bench.py --inference (same weights, same inputs), one step function per correlation mode"""
    from mrfa_amd.modules import RaftFlow
    size, h = a.size, a.size // 4
    rf = RaftFlow(**cfg["raft_flow"])
    sd = fill_state_dict(rf.state_dict(), tag="decoder.")
    for k in list(sd):
        if k.endswith(("refine.conv2.weight", "refine.convo2.weight")):
            sd[k] = sd[k] * 0.3
    rf.load_state_dict(sd)
    rf.to(dev).eval()
    img_full = det_uniform("c5/img", (B, 3, size, size), 0, 1).to(dev)
    img = torch.nn.functional.avg_pool2d(img_full, 4)
    kp_s, kp_d = det_uniform("c5/ks", (B, 10, 2), -0.8, 0.8).to(dev), det_uniform("c5/kd", (B, 10, 2), -0.8, 0.8).to(dev)
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, h), indexing="ij")
    deform = (torch.stack([xs, ys], dim=-1)[None].expand(B, h, h, 2) + det_uniform("c5/d", (B, h, h, 2), -0.1, 0.1)).contiguous().to(dev)
    dm = {"deformation": deform, "occlusion": det_uniform("c5/o", (B, 1, h, h), -2, 2).to(dev)}

    class _Fwd(torch.nn.Module):
        def __init__(self, corr):
            super().__init__()
            self.rf, self.corr = rf, corr

        def forward(self, full, quarter):
            return self.rf(kp_s, kp_d, dm, quarter, full, corr=self.corr)[0]
    steps, outs = {}, {}
    with torch.no_grad():
        for corr in a.corr:
            m = _Fwd(corr).eval()
            if a.no_graph:
                steps[corr] = lambda m=m: m(img_full, img)
            else:
                gf = GraphedForward(m, img_full, img)
                steps[corr] = lambda gf=gf: gf(gf.src, gf.drv)
            outs[corr] = steps[corr]().clone()
    if len(outs) == 2:
        d = (outs["volume"] - outs["direct"]).abs()
        print(f"  direct vs volume output: max |diff| {d.max().item():.3e} mean {d.mean().item():.3e}")
    return steps


def animator_steps(B):
    model = HotPath(cfg)
    for pfx, mod in (("encoder.", model.encoder), ("dense_motion.", model.dense_motion), ("decoder.", model.decoder)):
        mod.load_state_dict(fill_state_dict(mod.state_dict(), tag=pfx))
    model.to(dev).eval()
    src = det_uniform("ba/src", (B, 3, a.size, a.size), 0, 1).to(dev)
    drv = det_uniform("ba/drv", (B, 3, a.size, a.size), 0, 1).to(dev)
    steps = {}
    if a.corr == ["volume"] and a.rounds == 1 and not a.no_graph:
        gf = GraphedForward(model, src, drv)
        steps["full forward"] = lambda: gf(src, drv)
    for corr in a.corr:
        an = Animator(model, graph=not a.no_graph, corr=corr)
        an.set_source(src)
        steps[corr] = lambda an=an: an(drv)
    return steps


def build_model():
    model = HotPath(cfg)
    for pfx, mod in (("encoder.", model.encoder), ("dense_motion.", model.dense_motion), ("decoder.", model.decoder)):
        mod.load_state_dict(fill_state_dict(mod.state_dict(), tag=pfx))
    return model.to(dev).eval()


def clip_report():
    """one source, T driving frames per call; per corr mode and T three Animators in one process: "clip" (set_source of the ONE source, calls of T frames),
    "replicated" (set_source of the source repeated T times: the same batch-T program on T copies) and "per-frame" (T = 1, the path without this option)"""
    model = build_model()
    src = det_uniform("ba/src", (1, 3, a.size, a.size), 0, 1).to(dev)
    drv = det_uniform("ba/clip", (max(a.frames), 3, a.size, a.size), 0, 1).to(dev)

    def make(source, frames, corr):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        an = Animator(model, graph=not a.no_graph, corr=corr)
        an.set_source(source)
        an(frames)                                            # (graph=True: the capture; its pool stays allocated)
        torch.cuda.synchronize()
        return (lambda: an(frames)), (torch.cuda.memory_allocated() - base) / 1e6
    for corr in a.corr:
        for T in a.frames:
            frames = drv[:T].contiguous()
            steps, mem = {}, {}
            steps["per-frame"], mem["per-frame"] = make(src, frames[:1].contiguous(), corr)
            steps["clip"], mem["clip"] = make(src, frames, corr)
            steps["replicated"], mem["replicated"] = make(src.repeat_interleave(T, dim=0).contiguous(), frames, corr)
            d = (steps["clip"]().clone() - steps["replicated"]()).abs()
            times = {k: [] for k in steps}
            for fn in steps.values():
                for _ in range(3):
                    fn()
            for _ in range(a.rounds):
                for k, fn in steps.items():                   # the three alternate round by round: same box, same minute
                    times[k].append(timed(fn))
            print(f"{a.size}^2 corr={corr} T={T}: clip vs replicated output max |diff| {d.max().item():.3e} mean {d.mean().item():.3e}")
            for k, ts in times.items():
                n = 1 if k == "per-frame" else T
                per = [t / n for t in ts]
                print(f"{a.size}^2 corr={corr} T={T}: {k:10s} per call {summary(ts)}; per frame {statistics.median(per):.3f} ms ({min(per):.3f} - {max(per):.3f}), "
                      f"{1e3 / statistics.median(per):.0f} frames/s; device memory held {mem[k]:.1f} MB")
            del steps


def relative_report():
    """one source, T driving frames per call; per corr mode and T three programs in one process: "relative" (Animator(relative=True,
    adapt_movement_scale=True): the keypoints go through mrfa_kp_relative_fwd inside the frame program), "absolute" (the Animator on the raw driving
    keypoints) and "eager loop" (the loop make_animation ran before it moved onto the Animator, kept here as the yardstick: normalize_kp as torch launches on
    repeated keypoints, nothing captured)"""
    from mrfa_amd.infer import _expand_kp, normalize_kp
    model = build_model()
    frames_list = a.frames or [1]
    src = det_uniform("ba/src", (1, 3, a.size, a.size), 0, 1).to(dev)
    drv = det_uniform("ba/clip", (max(frames_list) + 1, 3, a.size, a.size), 0, 1).to(dev)
    first, drv = drv[:1].contiguous(), drv[1:]
    for corr in a.corr:
        kp_s, img_down, kp_init = model.encoder(src), model.down(src), model.encoder(first)
        cache = model.decoder.encode_source(kp_s["kp"], img_down, src)
        for T in frames_list:
            frames = drv[:T].contiguous()
            rel = Animator(model, graph=not a.no_graph, corr=corr, relative=True, adapt_movement_scale=True)
            rel.set_source(src, first)
            ab = Animator(model, graph=not a.no_graph, corr=corr)
            ab.set_source(src)
            kp_s_T, kp_init_T = _expand_kp(kp_s, T), _expand_kp(kp_init, T)

            def eager_loop():
                kp_n = normalize_kp(kp_s_T, model.encoder(frames), kp_init_T, adapt_movement_scale=True, use_relative_movement=True, use_relative_jacobian=True)
                dm = model.dense_motion(src, kp_n, kp_s_T)
                return model.decoder(kp_s["kp"], kp_n["kp"], dm, img=img_down, img_full=src, source_cache=cache, corr=corr)[0]
            steps = {"relative": lambda: rel(frames), "absolute": lambda: ab(frames), "eager loop": eager_loop}
            d = (steps["relative"]().clone() - eager_loop()).abs()
            times = {k: [] for k in steps}
            for fn in steps.values():
                for _ in range(3):
                    fn()
            for _ in range(a.rounds):
                for k, fn in steps.items():                   # the three alternate round by round: same box, same minute
                    times[k].append(timed(fn))
            print(f"{a.size}^2 corr={corr} T={T}: relative Animator vs eager loop output max |diff| {d.max().item():.3e} mean {d.mean().item():.3e}")
            for k, ts in times.items():
                per = [t / T for t in ts]
                print(f"{a.size}^2 corr={corr} T={T}: {k:10s} per frame {statistics.median(per):.3f} ms (median of {len(per)}, {min(per):.3f} - {max(per):.3f}), "
                      f"{1e3 / statistics.median(per):.0f} frames/s")
            med = {k: statistics.median(ts) / T for k, ts in times.items()}
            spread = (max(times["absolute"]) - min(times["absolute"])) / T
            print(f"{a.size}^2 corr={corr} T={T}: relative - absolute {med['relative'] - med['absolute']:+.3f} ms per frame (the absolute rounds spread over "
                  f"{spread:.3f} ms); eager loop / relative {med['eager loop'] / med['relative']:.2f}x")
            del steps, rel, ab


def best_frame_report():
    """one source, T driving frames per call; four programs in one process: "search graph" / "search eager" (BestFrameSearch.add: the keypoint detector on
    the group plus ONE mrfa_kp_pose_dist launch that keeps the running argmin on the device) and "detector graph" / "detector eager" (the keypoint detector
    alone on the same group: what a search cannot do without).  Nothing reads the device inside a timed window; result() is read once per search, after it."""
    from mrfa_amd.infer import BestFrameSearch
    model = build_model()
    src = det_uniform("ba/src", (1, 3, a.size, a.size), 0, 1).to(dev)
    for T in a.frames or [8]:
        groups = [det_uniform(f"ba/best{g}", (T, 3, a.size, a.size), 0, 1).to(dev) for g in range(4)]
        searches = {}
        for graph in (True, False):
            sr = BestFrameSearch(model, graph=graph)
            sr.set_source(src)
            for g in groups:
                sr.add(g)
            searches[graph] = sr
        found = {graph: (sr.result(), sr.state[:, 2].tolist()) for graph, sr in searches.items()}
        print(f"{a.size}^2 T={T}, {model.prior} keypoint detector: a clip of {4 * T} frames in 4 groups: best frame {found[True][0]} captured, {found[False][0]} eager; frames seen {found[True][1]}")
        assert found[True] == found[False], found
        from mrfa_amd import graph_replay_safe
        graph_replay_safe("bench_animator --best-frame")      # (as every capture of the project; the search legs ask through BestFrameSearch)
        static = groups[0].clone()
        model.encoder(static)
        torch.cuda.synchronize()
        gd = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gd):
            model.encoder(static)
        it = iter(range(1 << 30))
        nxt = lambda: groups[next(it) % 4]

        def detector_graph():
            static.copy_(nxt())
            gd.replay()
        steps = {"search graph": lambda: searches[True].add(nxt()), "search eager": lambda: searches[False].add(nxt()),
                 "detector graph": detector_graph, "detector eager": lambda: model.encoder(nxt())}
        times = {k: [] for k in steps}
        for fn in steps.values():
            for _ in range(3):
                fn()
        for _ in range(a.rounds):
            for k, fn in steps.items():                       # the four alternate round by round: same box, same minute
                times[k].append(timed(fn, n=200))             # a call is under a millisecond: 200 of them per window
        for k, ts in times.items():
            per = [t / T for t in ts]
            print(f"{a.size}^2 T={T}: {k:14s} per call {summary(ts)}; per frame {statistics.median(per):.4f} ms ({min(per):.4f} - {max(per):.4f})")
        med = {k: statistics.median(ts) / T for k, ts in times.items()}
        for mode in ("graph", "eager"):
            spread = (max(times[f"detector {mode}"]) - min(times[f"detector {mode}"])) / T
            print(f"{a.size}^2 T={T}: search - detector, {mode}: {med[f'search {mode}'] - med[f'detector {mode}']:+.4f} ms per frame (the detector rounds spread "
                  f"over {spread:.4f} ms)")


if a.best_frame:
    if a.frames and min(a.frames) < 1:
        ap.error("--frames: T >= 1")
    with torch.no_grad():
        best_frame_report()
    sys.exit(0)

if a.relative:
    if a.frames and min(a.frames) < 1:
        ap.error("--frames: T >= 1")
    with torch.no_grad():
        relative_report()
    sys.exit(0)

if a.frames:
    if min(a.frames) < 1:
        ap.error("--frames: T >= 1")
    with torch.no_grad():
        clip_report()
    sys.exit(0)

for B in a.batch:
    with torch.no_grad():
        steps = raft_forward_steps(B) if a.raft_forward else animator_steps(B)
        times = {k: [] for k in steps}
        for fn in steps.values():
            for _ in range(3):
                fn()
        for _ in range(a.rounds):
            for k, fn in steps.items():                       # the modes alternate round by round: same box, same minute
                times[k].append(timed(fn))
    what = "RaftFlow forward" if a.raft_forward else "animator frame"
    for k, ts in times.items():
        label = k if k == "full forward" else f"{what} corr={k}"
        extra = f" ({B / statistics.median(ts) * 1e3:.0f} frames/s)" if k != "full forward" else ""
        print(f"{a.size}^2 B={B}: {label} {summary(ts)}{extra}")
