"""Per-frame time of the two ends of an inference loop -- byte frames in, byte frames out -- beside the Animator between them (one source, T frames per
call, Animator(graph=True)).  Writes profiles/frame_io.txt.

    python tools/bench_frame_io.py [--out profiles/frame_io.txt] [--rounds 7] [--calls 20]
        at 256^2, T = 8 (corr="volume") and 512^2, T = 4 (corr="direct"), three programs alternate round by round in ONE process; a window is --calls
        groups of T frames and ends in a device synchronise:
          (a) animator      the Animator alone on device-resident fp32 frames
          (b) host ends     the ends as the reference's callers write them: uint8 host frames -> numpy float32 (x 1/255) -> transpose to planar -> upload
                            as fp32; the Animator; .cpu().numpy() -> transpose -> rint(255 x) as uint8 on the host (demo.py:72,160)
          (c) device ends   the same host bytes uploaded AS BYTES, Animator(bytes) (frames_from_uint8 into the captured program's input), frames_to_uint8,
                            the bytes read back
        then the two public conversions alone, 200 calls back to back between device events: the rate the Python layers issue them at.
    rocprofv3 --kernel-trace --stats -- python tools/bench_frame_io.py --kernel-only 100
        the two entries alone at both shapes, for the kernels' own times; prints the bytes a call must move (3 + 12 or 12 + 3 per pixel)
"""
import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfa_amd.infer import Animator, frames_from_uint8, frames_to_uint8  # noqa: E402
from mrfa_amd.train import VOX1, HotPath  # noqa: E402
from mrfa_amd.utils.prng import det_uniform, fill_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "frame_io.txt"))
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20, help="groups per timed window")
ap.add_argument("--kernel-calls", type=int, default=200)
ap.add_argument("--kernel-only", type=int, default=0, metavar="N", help="N calls of each entry at both shapes and nothing else (for a kernel trace)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
lines = []

if a.kernel_only:
    for size, T in ((256, 8), (512, 4)):
        u8 = (det_uniform("bfio/clip", (T, size, size, 3), 0, 1) * 256).clamp(0, 255).to(torch.uint8).to(dev)
        fl = torch.empty(T, 3, size, size, device=dev)
        for _ in range(a.kernel_only):
            frames_from_uint8(u8, out=fl)
        for rounding in ("nearest", "floor"):
            for _ in range(a.kernel_only):
                frames_to_uint8(fl, rounding)
        torch.cuda.synchronize()
        print(f"{size}^2 T={T}: {a.kernel_only} calls of mrfa_frames_from_u8, then of mrfa_frames_to_u8 nearest and floor; each must move {T * size * size * 15} bytes")
    sys.exit(0)


def say(s):
    print(s, flush=True)
    lines.append(s)


def kernel_time(fn, n):
    for _ in range(10):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n * 1e3                                # us per call


def shape(size, T, corr):
    tag = f"{size}^2 T={T} corr={corr}"
    cfg = copy.deepcopy(VOX1)
    cfg["raft_flow"]["size"] = size
    model = HotPath(cfg)
    for pfx, mod in (("encoder.", model.encoder), ("dense_motion.", model.dense_motion), ("decoder.", model.decoder)):
        mod.load_state_dict(fill_state_dict(mod.state_dict(), tag=pfx))
    model.to(dev).eval()
    host_u8 = (det_uniform("bfio/clip", (T, size, size, 3), 0, 1) * 256).clamp(0, 255).to(torch.uint8).numpy()      # what an image reader returns
    src = det_uniform("bfio/src", (1, 3, size, size), 0, 1).to(dev)
    with torch.no_grad():
        an = Animator(model, graph=True, corr=corr)
        an.set_source(src)
        resident = frames_from_uint8(torch.from_numpy(host_u8).to(dev))
        an(resident)

        def host_ends():
            x = np.multiply(host_u8, 1. / 255, dtype=np.float32)                                    # img_as_float32
            x = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).to(dev)
            out = an(x).cpu().numpy()
            return np.clip(np.rint(np.transpose(out, [0, 2, 3, 1]) * 255.0), 0, 255).astype(np.uint8)   # img_as_ubyte

        def device_ends():
            return frames_to_uint8(an(torch.from_numpy(host_u8).to(dev)), "nearest").cpu().numpy()

        steps = {"(a) animator": lambda: an(resident), "(b) host ends": host_ends, "(c) device ends": device_ends}
        b, c = host_ends(), device_ends()
        d = np.abs(b.astype(np.int32) - c.astype(np.int32))
        say(f"{tag}: (b) and (c) return {b.shape} uint8; they differ in {(d > 0).mean():.2e} of the bytes, by at most {d.max()} (two runs of the Animator)")

        def window(name):
            fn = steps[name]
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / a.calls * 1e3

        times = {k: [] for k in steps}
        for k in steps:
            window(k)
        for _ in range(a.rounds):
            for k in steps:                                         # alternate round by round: same machine, same minute
                times[k].append(window(k))
        med = {}
        for k, ts in times.items():
            per = [t / T for t in ts]
            med[k] = statistics.median(per)
            say(f"{tag}: {k:15s} {T / statistics.median(ts) * 1e3:8.1f} frames/s, per frame {med[k]:.4f} ms (median of {len(ts)}, {min(per):.4f} - {max(per):.4f})")
        for k in ("(b) host ends", "(c) device ends"):
            say(f"{tag}: {k} - (a) animator {med[k] - med['(a) animator']:+.4f} ms per frame")
        say(f"{tag}: (c) - (b) {med['(c) device ends'] - med['(b) host ends']:+.4f} ms per frame")
        # the two kernels alone
        dev_u8 = torch.from_numpy(host_u8).to(dev)
        fl = torch.empty(T, 3, size, size, device=dev)
        px = T * size * size
        t_from = kernel_time(lambda: frames_from_uint8(dev_u8, out=fl), a.kernel_calls)
        note = "the rate the Python layers issue them at, not the kernel's time: that is read from a kernel trace of --kernel-only"
        say(f"{tag}: frames_from_uint8 {t_from:.2f} us per call, {a.kernel_calls} back to back between device events ({note}); the kernel must move "
            f"{px * 15} bytes (3 in, 12 out per pixel)")
        for rounding in ("nearest", "floor"):
            t_to = kernel_time(lambda: frames_to_uint8(fl, rounding), a.kernel_calls)
            say(f"{tag}: frames_to_uint8 ({rounding}) {t_to:.2f} us per call incl. the allocation of its output, likewise; {px * 15} bytes (12 in, 3 out per pixel)")
    del an, model
    torch.cuda.empty_cache()


shape(256, 8, "volume")
shape(512, 4, "direct")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("tools/bench_frame_io.py on MI355X: medians of %d rounds of %d groups, Animator(graph=True), one source\n" % (a.rounds, a.calls))
    f.write("\n".join(lines) + "\n")
