"""Time of bringing byte frames to the model's size: FrameResizer on the device against Pillow on the same box.  Writes profiles/frame_resize.txt.

    python tools/bench_resize.py [--out profiles/frame_resize.txt] [--rounds 7] [--steps 50] [--frames 8] [--no-animator]
        geometries: 1920 x 1080 cropped to the middle 1080^2 -> 256^2 (bilinear, Lanczos); 512^2 -> 256^2; 256^2 -> 256^2 beside mrfa_frames_from_u8.
          kernel     --steps launches back to back between two device events on resident bytes of ONE frame and of --frames frames; GB/s over the algorithmic
                     bytes (the crop read once, the fp32 output written once)
          Pillow     Image.resize(size, filter, box) on the same frame, one thread, wall time per frame
          animator   Animator(graph=True) at T = --frames from HOST bytes of the large frames, wall time per call that ends in a synchronise:
                       device   upload the bytes (pinned), then the Animator with prepare=FrameResizer
                       host     Pillow per frame, then upload the resized BYTES (or their FLOATS) and the Animator as it was
                       alone    the Animator on resident floats of the model's size
        The three alternate round by round in one process; medians and the spread of each.  No threshold: the file states the numbers.
"""
import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mrfa_amd import FrameResizer  # noqa: E402
from mrfa_amd.infer import Animator, frames_from_uint8  # noqa: E402
from tests import ref_resize as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_resize.txt"))
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=50, help="launches per timed window")
ap.add_argument("--frames", type=int, default=8, help="T: frames per Animator call")
ap.add_argument("--no-animator", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
lines = []

try:
    import PIL
    from PIL import Image
    HOST = f"Pillow {PIL.__version__}"
except ImportError:
    Image, HOST = None, "not measured (Pillow is not importable here)"

BOX_1080 = (420, 0, 1500, 1080)
GEOMETRIES = [("1920x1080 box 1080^2 -> 256^2", (1080, 1920), BOX_1080, "bilinear"), ("1920x1080 box 1080^2 -> 256^2", (1080, 1920), BOX_1080, "lanczos"),
              ("512^2 -> 256^2", (512, 512), None, "bilinear"), ("256^2 -> 256^2", (256, 256), None, "bilinear")]
SIZE = (256, 256)


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(v, unit):
    return f"{statistics.median(v):.3f} {unit} (median of {len(v)}, {min(v):.3f} - {max(v):.3f})"


def events(fn, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n * 1e3                              # us per launch


def wall(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3                        # ms per call


_CLIPS = {}


def clip(hi, wi):
    """--frames frames (T,hi,wi,3): one frame of seeded bytes, shifted along its rows from frame to frame"""
    if (hi, wi) not in _CLIPS:
        first = R.det_bytes(f"bench/resize/{hi}x{wi}", (hi, wi, 3))
        _CLIPS[(hi, wi)] = np.stack([np.roll(first, 37 * t, axis=1) for t in range(a.frames)])
    return _CLIPS[(hi, wi)]


def pillow(frame, box, name):
    return np.array(Image.fromarray(frame).resize((SIZE[1], SIZE[0]), getattr(Image, name.upper()), box=box))


def kernel_report():
    for tag, (hi, wi), box, name in GEOMETRIES:
        host = clip(hi, wi)
        resident = torch.from_numpy(host).to(dev)
        r = FrameResizer(SIZE, box=box, filter=name)
        steps = {}
        for n in (1, a.frames):
            src, out = resident[:n].contiguous(), torch.empty(n, 3, *SIZE, device=dev)
            steps[f"resize N={n}"] = (lambda src=src, out=out: r(src, out=out)), n
            if hi == SIZE[0] and box is None:
                steps[f"frames_from_uint8 N={n}"] = (lambda src=src, out=out: frames_from_uint8(src, out=out)), n
        if Image is not None:
            same = np.array_equal(r(resident[:1]).mul(255).round().byte().cpu().numpy()[0].transpose(1, 2, 0), pillow(host[0], box, name))
            say(f"{tag} {name}: device and {HOST} give the same bytes: {same}")
        times = {k: [] for k in steps}
        for fn, _ in steps.values():
            events(fn, 5)
        for _ in range(a.rounds):
            for k, (fn, _) in steps.items():                          # alternate round by round
                times[k].append(events(fn, a.steps))
        bw, bh = (wi, hi) if box is None else (box[2] - box[0], box[3] - box[1])
        for k, v in times.items():
            n = steps[k][1]
            nbytes = n * (bw * bh * 3 + SIZE[0] * SIZE[1] * 12)
            us = statistics.median(v)
            say(f"{tag} {name}: {k:24s} {spread(v, 'us')} per launch, {a.steps} back to back between device events; algorithmic bytes "
                f"{nbytes / 1e6:.2f} MB, {nbytes / us / 1e3:.0f} GB/s")
        if Image is not None:
            pt = []
            for _ in range(a.rounds):
                t = time.perf_counter()
                pillow(host[0], box, name)
                pt.append((time.perf_counter() - t) * 1e3)
            say(f"{tag} {name}: {HOST}, one thread: {spread(pt, 'ms')} per frame")


def animator_report():
    from mrfa_amd.train import VOX1, HotPath
    from mrfa_amd.utils.prng import det_uniform, fill_state_dict
    cfg = copy.deepcopy(VOX1)
    cfg["raft_flow"]["size"] = SIZE[0]
    model = HotPath(cfg)
    for pfx, mod in (("encoder.", model.encoder), ("dense_motion.", model.dense_motion), ("decoder.", model.decoder)):
        mod.load_state_dict(fill_state_dict(mod.state_dict(), tag=pfx))
    model = model.to(dev).eval()
    T = a.frames
    host = clip(1080, 1920)
    pinned = torch.from_numpy(host).pin_memory()
    source = det_uniform("bench/resize/src", (1, 3, *SIZE), 0, 1).to(dev)
    for name in ("bilinear", "lanczos"):
        r = FrameResizer(SIZE, box=BOX_1080, filter=name)
        floats = r(pinned.to(dev)).clone()
        an = {k: Animator(model, graph=True, prepare=(r if k == "device" else None)) for k in ("device", "host", "alone")}
        for v in an.values():
            v.set_source(source)
        small = torch.empty(T, *SIZE, 3, dtype=torch.uint8).pin_memory()

        def host_bytes():
            for t in range(T):
                small[t] = torch.from_numpy(pillow(host[t], BOX_1080, name))
            return an["host"](small.to(dev, non_blocking=True))

        def host_floats():
            x = np.stack([pillow(host[t], BOX_1080, name) for t in range(T)]).astype(np.float32) * np.float32(1.0 / 255.0)
            return an["host"](torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).to(dev))

        steps = {"device: upload bytes, prepare=": (lambda: an["device"](pinned.to(dev, non_blocking=True)), 10),
                 "alone: resident floats": (lambda: an["alone"](floats), 10)}
        if Image is not None:
            steps["host: Pillow, upload bytes"] = (host_bytes, 2)
            steps["host: Pillow, upload floats"] = (host_floats, 2)
        for fn, _ in steps.values():                                  # captures, warm-up
            fn()
            fn()
        times = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, (fn, n) in steps.items():                          # alternate round by round: same box, same minute
                times[k].append(wall(fn, n))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            say(f"animator T={T} 1920x1080 -> 256^2 {name}: {k:30s} {spread(v, 'ms')} per call wall; per frame {med[k] / T:.3f} ms; "
                f"above the Animator alone {(med[k] - med['alone: resident floats']) / T:+.3f} ms per frame")
        say(f"animator T={T} {name}: uploads per call: {host.nbytes / 1e6:.1f} MB of large bytes (device path) against {T * SIZE[0] * SIZE[1] * 3 / 1e6:.2f} MB of "
            f"resized bytes or {T * SIZE[0] * SIZE[1] * 12 / 1e6:.2f} MB of floats (host path)")


kernel_report()
if not a.no_animator:
    animator_report()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("tools/bench_resize.py on MI355X: medians of %d rounds, with the spread of each; host path: %s\n" % (a.rounds, HOST))
    f.write("\n".join(lines) + "\n")
