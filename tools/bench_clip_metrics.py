"""Per-frame time of a clip's metrics beside the Animator that produces the frames (one source, T frames per call, Animator(graph=True)).

    python tools/bench_clip_metrics.py --size 256 --frames 8 --rounds 7
    python tools/bench_clip_metrics.py --size 512 --frames 4 --corr direct --rounds 7
        four programs alternate round by round in ONE process, a window is --calls groups of T frames and ends in a device synchronise:
          animator        the Animator alone
          host metrics    + L1 and PSNR as reconstruction(metrics="host") computes them: per frame a clone, a copy of the driving frame, torch launches and
                          three host reads
          ClipMetrics     + ClipMetrics.add per group (L1, MSE -> PSNR, SSIM in one entry call), ONE host read (result()) at the end of the window
          torch SSIM      + the host metrics and an SSIM written with F.conv2d on the device (a separable depthwise window: ten launches per group), read
                          per frame: what a user without the entry writes
    python tools/bench_clip_metrics.py --size 256 --frames 8 --kernel-only 50
        mrfa_frame_metrics alone on a group, 50 calls: the program to run under `rocprofv3 --kernel-trace --stats`; prints the algorithmic bytes of a call
"""
import argparse
import copy
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfa_amd.infer import Animator, ClipMetrics, _clip_group, psnr  # noqa: E402
from mrfa_amd.train import VOX1, HotPath  # noqa: E402
from mrfa_amd.utils.prng import det_uniform, fill_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--frames", type=int, default=8, metavar="T", help="frames of the one source per call")
ap.add_argument("--corr", choices=("volume", "direct"), default="volume")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20, help="groups per timed window")
ap.add_argument("--kernel-only", type=int, default=0, metavar="N", help="N calls of mrfa_frame_metrics on one group and nothing else (for a kernel trace)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
T, size = a.frames, a.size

video = det_uniform("bcm/clip", (1, 3, T, size, size), 0, 1).to(dev)          # frame 0 is the source, as in reconstruction()
group = _clip_group(video, 0, T)

if a.kernel_only:
    pred = det_uniform("bcm/pred", (T, 3, size, size), 0, 1).to(dev)
    cm = ClipMetrics()
    for _ in range(a.kernel_only):
        cm.add(pred, group)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.kernel_only):
        cm.add(pred, group)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.kernel_only
    res = cm.result()
    nbytes = 2 * T * 3 * size * size * 4
    print(f"{size}^2 T={T}: mrfa_frame_metrics, {a.kernel_only} calls back to back: {dt * 1e6:.1f} us per call on the host clock (two launches each); "
          f"algorithmic bytes per call 2 N C H W 4 = {nbytes}; ssim of the group {res['ssim'][:T].tolist()}")
    sys.exit(0)

cfg = copy.deepcopy(VOX1)
cfg["raft_flow"]["size"] = size
model = HotPath(cfg)
for pfx, mod in (("encoder.", model.encoder), ("dense_motion.", model.dense_motion), ("decoder.", model.decoder)):
    mod.load_state_dict(fill_state_dict(mod.state_dict(), tag=pfx))
model.to(dev).eval()

_g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / 4.5)
_g = (_g / _g.sum()).float().to(dev)
W_ROW, W_COL = _g.view(1, 1, 1, 11).repeat(3, 1, 1, 1), _g.view(1, 1, 11, 1).repeat(3, 1, 1, 1)


def torch_ssim(x, y):
    """(N,3,H,W) -> (N,): the same definition as mrfa_frame_metrics in fp32 torch, ten depthwise-convolution launches"""
    win = lambda v: F.conv2d(F.conv2d(v, W_ROW, groups=3), W_COL, groups=3)
    mx, my = win(x), win(y)
    sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
    return ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))).mean(dim=(1, 2, 3))


def host_metrics(outs):
    """the loop body of reconstruction(metrics="host") on one group"""
    outs = outs.view(1, T, 3, size, size)
    vals = []
    for j in range(T):
        driving = video[:, :, j].contiguous()
        out = outs[:, j].clone()
        vals.append((float(torch.abs(out - driving).mean()), float(psnr(driving, out))))
    return vals


with torch.no_grad():
    an = Animator(model, graph=True, corr=a.corr)
    an.set_source(video[:, :, 0].contiguous())
    an(group)
    state = {"cm": ClipMetrics()}

    def with_clip_metrics():
        state["cm"].add(an(group), group)

    def with_torch_ssim():
        outs = an(group)
        vals = host_metrics(outs)
        s = torch_ssim(outs, group)
        return vals, [float(s[j]) for j in range(T)]

    steps = {"animator": lambda: an(group), "host metrics": lambda: host_metrics(an(group)), "ClipMetrics": with_clip_metrics, "torch SSIM": with_torch_ssim}

    def window(name):
        fn = steps[name]
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.calls):
            fn()
        if name == "ClipMetrics":                                  # the clip's one host read belongs to the window
            state["last"] = state["cm"].result()
            state["cm"] = ClipMetrics()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.calls * 1e3

    # the three forms agree on the same frames
    host = host_metrics(an(group))
    _, ts = with_torch_ssim()
    cm = ClipMetrics()
    cm.add(an(group), group)
    res = cm.result()
    print(f"{size}^2 T={T} corr={a.corr}: l1 host {[round(v[0], 6) for v in host][:3]} device {[round(float(v), 6) for v in res['l1'][:3]]}; psnr host "
          f"{[round(v[1], 4) for v in host][:3]} device {[round(float(v), 4) for v in res['psnr'][:3]]}; ssim torch fp32 {[round(v, 6) for v in ts][:3]} device "
          f"{[round(float(v), 6) for v in res['ssim'][:3]]}")
    times = {k: [] for k in steps}
    for k in steps:
        window(k)
    for _ in range(a.rounds):
        for k in steps:                                            # the four alternate round by round: same box, same minute
            times[k].append(window(k))
for k, ts in times.items():
    per = [t / T for t in ts]
    print(f"{size}^2 T={T} corr={a.corr}: {k:13s} per call {statistics.median(ts):.3f} ms (median of {len(ts)}, {min(ts):.3f} - {max(ts):.3f}); per frame "
          f"{statistics.median(per):.4f} ms ({min(per):.4f} - {max(per):.4f})")
med = {k: statistics.median(ts) / T for k, ts in times.items()}
spread_b = (max(times["host metrics"]) - min(times["host metrics"])) / T
for k in ("host metrics", "ClipMetrics", "torch SSIM"):
    print(f"{size}^2 T={T} corr={a.corr}: {k} - animator {med[k] - med['animator']:+.4f} ms per frame")
print(f"{size}^2 T={T} corr={a.corr}: ClipMetrics - host metrics {med['ClipMetrics'] - med['host metrics']:+.4f} ms per frame (the host-metrics rounds spread over "
      f"{spread_b:.4f} ms)")
