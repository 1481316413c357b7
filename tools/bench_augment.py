"""Time of augmenting one training batch: PairAugmenter on the device against the reference's host path on the same box.  Writes profiles/pair_augment.txt.

    python tools/bench_augment.py [--out profiles/pair_augment.txt] [--rounds 7] [--steps 20] [--host-steps 3]
        B = 8 and 16 pairs of 256 x 256 x 3 bytes, the vox1 augmentation_params, parameters drawn anew every step.
          device, resident     the bytes already on the device: the entry calls alone between two device events (--steps back to back), and the wall time
                               of a step that ends in a synchronise
          device, pinned       the bytes in pinned host memory: upload as bytes (3.1 MB at B = 8), then the same call; wall time per step
          host                 the reference's path per frame -- uint8 -> PIL -> the four ops in the drawn order -> numpy -> x 1/255 in float64 -> float32,
                               flips, (B,3,H,W) -- and the upload of the FLOATS (12.6 MB at B = 8); Pillow where it is importable, else the numpy
                               specification tests/ref_augment.py (the line says which); wall time per step, one thread
        No threshold: the file states the numbers and their ratio.
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mrfa_amd.augment import PairAugmenter  # noqa: E402
from tests import ref_augment as R  # noqa: E402

VOX1_AUG = {"flip_param": {"horizontal_flip": True, "time_flip": True}, "jitter_param": {"brightness": 0.1, "contrast": 0.1, "saturation": 0.1, "hue": 0.1}}

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_augment.txt"))
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=20, help="device steps per timed window")
ap.add_argument("--host-steps", type=int, default=3, help="host steps per timed window")
a = ap.parse_args()
dev = torch.device("cuda", 0)
lines = []

try:
    import PIL
    from make_augment_goldens import pil_chain
    HOST = f"Pillow {PIL.__version__}"

    def host_frame(rgb, p):
        return pil_chain(rgb, [(n, getattr(p, n)) for n in p.order])
except ImportError:
    HOST = "the numpy specification tests/ref_augment.py (Pillow is not importable here)"

    def host_frame(rgb, p):
        return R.apply_ops(rgb, *R.ops_of([(n, getattr(p, n)) for n in p.order]))


def say(s):
    print(s, flush=True)
    lines.append(s)


def host_step(u8, params):
    """the reference's path: per frame to bytes' floats, flips, planar, then the float upload"""
    B, _, H, W, _ = u8.shape
    source, driving = np.empty((B, 3, H, W), np.float32), np.empty((B, 3, H, W), np.float32)
    for b, p in enumerate(params.pairs):
        clip = [u8[b, 0], u8[b, 1]]
        if p.time_flip:
            clip = clip[::-1]
        if p.hflip:
            clip = [np.fliplr(f) for f in clip]
        clip = [np.multiply(host_frame(f, p), 1.0 / 255, dtype=np.float64).astype("float32") for f in clip]
        source[b], driving[b] = clip[0].transpose(2, 0, 1), clip[1].transpose(2, 0, 1)
    return torch.from_numpy(source).to(dev), torch.from_numpy(driving).to(dev)


def window(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def batch(B, size=256):
    tag = f"B={B} {size}^2"
    host_u8 = R.det_bytes(f"bench/augment/{B}", (B, 2, size, size, 3))
    pinned = torch.from_numpy(host_u8).pin_memory()
    resident = pinned.to(dev)
    aug = PairAugmenter.from_config(VOX1_AUG, rng=random.Random(0))
    out = (torch.empty(B, 3, size, size, device=dev), torch.empty(B, 3, size, size, device=dev))
    # the two paths agree to the byte
    params = aug.draw(B)
    hs, hd = host_step(host_u8, params)
    ds, dd = aug(resident, params, out=out)
    same = bool((torch.round(hs * 255) == torch.round(ds * 255)).all() and (torch.round(hd * 255) == torch.round(dd * 255)).all())
    say(f"{tag}: host path = {HOST}; host and device outputs are the same bytes: {same}; largest float difference {float((hs - ds).abs().max()):.3e}")

    steps = {"device, resident": lambda: aug(resident, out=out),
             "device, pinned": lambda: aug(pinned.to(dev, non_blocking=True), out=out),
             "host": lambda: host_step(host_u8, aug.draw(B))}
    reps = {"device, resident": a.steps, "device, pinned": a.steps, "host": a.host_steps}
    times = {k: [] for k in steps}
    for k in steps:
        window(steps[k], 2)
    for _ in range(a.rounds):
        for k in steps:                                            # alternate round by round: same machine, same minute
            times[k].append(window(steps[k], reps[k]))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        say(f"{tag}: {k:17s} {med[k]:9.3f} ms per step wall (median of {len(v)} windows of {reps[k]} steps, {min(v):.3f} - {max(v):.3f})")
    # the entry calls alone: back to back between two device events (the draw and the launches overlap the kernels)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fixed = aug.draw(B)
    ev = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.steps):
            aug(resident, fixed, out=out)
        t1.record()
        torch.cuda.synchronize()
        ev.append(t0.elapsed_time(t1) / a.steps * 1e3)
    px = B * size * size
    us = statistics.median(ev)
    say(f"{tag}: entry call (luma sums + apply), resident bytes, fixed parameters: {us:.1f} us per call between device events, {a.steps} back to back "
        f"(median of {len(ev)}, {min(ev):.1f} - {max(ev):.1f}; the rate the Python layer issues them at, an upper bound on the kernels' own time); per pair pixel 2 x 3 bytes in (read twice when contrast is on) and 24 out: "
        f"{px * 30 / 1e6:.1f} MB, {px * 30 / us / 1e3:.0f} GB/s")
    say(f"{tag}: host / device, resident = {med['host'] / med['device, resident']:.0f}x; host / device, pinned = {med['host'] / med['device, pinned']:.0f}x; "
        f"uploads: {host_u8.nbytes / 1e6:.1f} MB of bytes against {px * 24 / 1e6:.1f} MB of floats")


batch(8)
batch(16)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("tools/bench_augment.py on MI355X: medians of %d rounds; vox1 augmentation_params; 256 x 256 x 3 frames\n" % a.rounds)
    f.write("\n".join(lines) + "\n")
