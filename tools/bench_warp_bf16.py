"""What the bf16 source-feature cache buys (RaftFlow.encode_source(feature_dtype=torch.bfloat16), Animator(cache_dtype=torch.bfloat16)).

ONE process, one GPU, HIP events, every shape warmed first, the two variants alternating run by run:
  1. the feature warps from an fp32 pyramid (mrfa_grid_sample_fwd, the kernel of the parent tree, unchanged) and from its bf16 cast
     (mrfa_grid_sample_bf16_fwd) at 512^2 batch 4 (BASELINE config 5) and 256^2 batch 8:
       "bench set"    the six launches bench.py's roofline block times (one flow-in-pixels warp per level; 1.039 GB algorithmic at 512^2 batch 4),
       "program set"  the launches RaftFlow._program issues per frame: per level a context warp and an output warp (flow in pixels) and, for the five levels
                      the decoder reads, a coarse warp (normalised grid) straight into its decode concat slot -- 17 launches;
  2. Animator frames per second, fp32 cache against bf16 cache, eager and graph=True, same two shapes;
  3. the bytes each cache holds;
  4. how far the frames of the two caches sit from the reference's recorded frames (tests/golden/dropin_<prior>.npz, the cases of tests/test_callers.py).
Medians and spreads (min .. max over the runs) are printed and written to --out (default profiles/bf16_cache_warps.txt).

    python tools/bench_warp_bf16.py [--runs 15] [--reps 10] [--skip-animator] [--out FILE]
"""
import argparse
import copy
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mrfa_amd import hip  # noqa: E402
from mrfa_amd.engine import Ctx  # noqa: E402

LEVELS = ((512, 32), (512, 16), (512, 8), (256, 4), (128, 2), (64, 1))            # (channels, size // resolution), coarse first
N_UP = 5                                                                        # levels whose coarse warp the decoder reads
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def flush_file(path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")


def med_spread(v):
    return statistics.median(v), min(v), max(v)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(variants, runs, reps):
    """{name: [ms per call, one per run]}: the variants take turns inside every run"""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(runs):
        for k, fn in variants.items():
            out[k].append(timed(fn, reps))
    return out


def verdict(t32, t16):
    (m32, lo32, hi32), (m16, lo16, hi16) = med_spread(t32), med_spread(t16)
    spread = (hi32 - lo32) + (hi16 - lo16)
    ok = m32 - m16 > spread
    return (f"bf16 / fp32 = {m16 / m32:.3f}; fp32 median - bf16 median = {1e3 * (m32 - m16):.1f} us against a combined run-to-run spread of "
            f"{1e3 * spread:.1f} us: {'FASTER by more than the spread' if ok else 'NOT faster by more than the spread'}"), ok


def warp_sets(dev, size, B, runs, reps):
    e = Ctx(dev, train=False, record=False)
    g = torch.Generator(device=dev).manual_seed(size + B)
    lv = []
    for C_, div in LEVELS:
        r = size // div
        f = e.new(B, r, r, C_)
        f.st.data.normal_(generator=g)
        h = e.to_bf16(f)
        flow = e.new(B, r, r, 2)
        flow.st.data.uniform_(-3, 3, generator=g)                                # (bench.py's roofline grids)
        flow_w = e.new(B, r, r, 2)
        flow_w.tensor().copy_(flow.tensor() + torch.empty(B, r, r, 2, device=dev).uniform_(-0.5, 0.5, generator=g))
        ys, xs = torch.meshgrid(torch.linspace(-1, 1, r, device=dev), torch.linspace(-1, 1, r, device=dev), indexing="ij")
        grid_c = e.new(B, r, r, 2)
        grid_c.tensor().copy_(torch.stack([xs, ys], dim=-1)[None].expand(B, r, r, 2) +
                              torch.empty(B, r, r, 2, device=dev).uniform_(-0.1, 0.1, generator=g))                        # (bench.py's config-5 deformation)
        lv.append(dict(C=C_, r=r, f=f, h=h, flow=flow, flow_w=flow_w, grid_c=grid_c, ctx=e.new(B, r, r, C_), out=e.new(B, r, r, C_),
                       cat=e.new(B, r, r, 2 * C_)))
    elems = sum(B * l["C"] * l["r"] ** 2 for l in lv)
    pix = sum(B * l["r"] ** 2 for l in lv)
    alg32 = 4.0 * (2 * elems + 2 * pix)                                          # bench.py: read C H W, write C H W, read the (x, y) grid
    alg16 = alg32 - 2.0 * elems                                                  # the gathered bytes halve, the written bytes do not
    elems_up = sum(B * l["C"] * l["r"] ** 2 for l in lv[:N_UP])
    pix_up = sum(B * l["r"] ** 2 for l in lv[:N_UP])
    prog32 = 2 * alg32 + 4.0 * (2 * elems_up + 2 * pix_up)
    prog16 = prog32 - 2.0 * (2 * elems + elems_up)

    def bench_set(key):
        def run():
            for l in lv:
                e.grid_sample(l[key], l["flow"], 1, out=l["out"])
        return run

    def program_set(key):
        def run():
            for i, l in enumerate(lv):
                e.grid_sample(l[key], l["flow"], 1, out=l["ctx"])
                e.grid_sample(l[key], l["flow_w"], 1, out=l["out"])
                if i < N_UP:
                    e.grid_sample(l[key], l["grid_c"], 0, out=l["cat"].slice(l["C"], 2 * l["C"]))
        return run

    # the two kernels must agree before their times are compared
    worst = 0.0
    for l in lv:
        a = e.grid_sample(l["h"], l["flow"], 1)
        w = Ctx(dev, train=False, record=False).wrap_nhwc(l["h"].tensor().float().contiguous())
        b = e.grid_sample(w, l["flow"], 1)
        worst = max(worst, (a.tensor() - b.tensor()).abs().max().item())
    say(f"== warps at {size}^2, batch {B}: pyramid {elems} elements = {4 * elems / 1e6:.1f} MB fp32, {2 * elems / 1e6:.1f} MB bf16; "
        f"max |bf16 kernel - fp32 kernel on the widened pyramid| = {worst:.3e}")
    oks = {}
    for name, mk, b32, b16, nl in (("bench set (6 launches)", bench_set, alg32, alg16, 6), ("program set (17 launches)", program_set, prog32, prog16, 17)):
        t = alternate({"fp32": mk("f"), "bf16": mk("h")}, runs, reps)
        for k, byt in (("fp32", b32), ("bf16", b16)):
            m, lo, hi = med_spread(t[k])
            say(f"   {name:26s} {k}: median {1e3 * m:8.1f} us  (min {1e3 * lo:8.1f} .. max {1e3 * hi:8.1f}, {runs} runs x {reps} sets)   "
                f"{byt / 1e9:.3f} GB algorithmic = {byt / m / 1e9:.3f} TB/s = {byt / m / 1e9 / 8.0:.3f} of 8 TB/s")
        txt, ok = verdict(t["fp32"], t["bf16"])
        oks[name.split(" (")[0]] = ok
        say(f"   {name:26s} {txt}")
    # per level, flow-in-pixels warp, each level's launch repeated back to back: a level whose input + output fit the 256 MiB Infinity Cache is then served from it
    # (and more levels fit from bf16), so these lines show where the time goes, the sets above (a whole pyramid between two uses of a line) what a frame pays
    for l in lv:
        t = alternate({"fp32": lambda l=l: e.grid_sample(l["f"], l["flow"], 1, out=l["out"]),
                       "bf16": lambda l=l: e.grid_sample(l["h"], l["flow"], 1, out=l["out"])}, max(5, runs // 2), reps)
        m32, m16 = statistics.median(t["fp32"]), statistics.median(t["bf16"])
        say(f"      level C={l['C']:3d} @{l['r']:3d}^2: fp32 {1e3 * m32:7.1f} us, bf16 {1e3 * m16:7.1f} us ({m16 / m32:.3f})")
    return oks


def cache_bytes(cache):
    return sum(f.st.data.numel() * f.st.data.element_size() for f in cache["feature"])


def animator_fps(dev, size, B, runs, reps):
    from mrfa_amd.infer import Animator
    from mrfa_amd.train import VOX1, HotPath
    from mrfa_amd.utils.prng import det_uniform, fill_state_dict
    cfg = copy.deepcopy(VOX1)
    cfg["raft_flow"]["size"] = size
    model = HotPath(cfg)
    for pfx, mod in (("encoder.", model.encoder), ("dense_motion.", model.dense_motion), ("decoder.", model.decoder)):
        sd = fill_state_dict(mod.state_dict(), tag=pfx)
        for k in list(sd):
            if k.endswith("jacobian.weight"):
                sd[k] = sd[k] * 0.05
            if k.endswith("jacobian.bias"):
                sd[k] = torch.tensor([1.0, 0.0, 0.0, 1.0]) + sd[k] * 0.5
            if k.endswith(("refine.conv2.weight", "refine.convo2.weight")):
                sd[k] = sd[k] * 0.3
        mod.load_state_dict(sd)
    model.to(dev).eval()
    src = det_uniform("wb/src", (B, 3, size, size), 0, 1).to(dev)
    drv = det_uniform("wb/drv", (B, 3, size, size), 0, 1).to(dev)
    say(f"== Animator at {size}^2, batch {B} (HotPath, KPDetector prior, deterministic random weights)")
    for graph in (False, True):
        ans = {}
        for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            an = Animator(model, graph=graph, cache_dtype=dt)
            an.set_source(src)
            an(drv)                                                               # (graph=True: capture + its eager-versus-replay gate)
            ans[name] = an
        if not graph:
            say(f"   source cache, feature pyramid: fp32 {cache_bytes(ans['fp32'].cache) / 1e6:.1f} MB, bf16 {cache_bytes(ans['bf16'].cache) / 1e6:.1f} MB")
            d = (ans["bf16"](drv) - ans["fp32"](drv)).abs()
            say(f"   bf16-cache frame against fp32-cache frame (these weights): max |diff| {d.max().item():.3e}, mean {d.mean().item():.3e}")
        t = alternate({k: (lambda an=an: an(drv)) for k, an in ans.items()}, runs, reps)
        for k in ("fp32", "bf16"):
            m, lo, hi = med_spread(t[k])
            say(f"   {'graph=True' if graph else 'eager     '} {k} cache: median {m:7.3f} ms per call (min {lo:7.3f} .. max {hi:7.3f}) = {B / m * 1e3:7.1f} frames/s")
        say(f"   {'graph=True' if graph else 'eager     '} {verdict(t['fp32'], t['bf16'])[0]}")
        del ans
    del model
    torch.cuda.empty_cache()


def frame_distance(dev):
    """frames of make_animation from an fp32 and from a bf16 cache against the frames the reference recorded for the same inputs and weights"""
    from mrfa_amd.infer import make_animation
    from tests import cases
    from tests.test_callers import _dropin_model
    say("== distance to the reference's recorded animation frames (tests/golden/dropin_<prior>.npz: 3 frames, 256^2, every second pixel)")
    for prior in ("fomm", "mtia"):
        g = np.load(os.path.join(ROOT, "tests", "golden", f"dropin_{prior}.npz"))
        m = _dropin_model(prior, dev)
        src = cases.images("dropin/src", 1, 256).to(dev)
        clip = torch.stack([cases.images(f"dropin/drv{t}", 1, 256).to(dev) for t in range(3)], dim=2)
        for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            anim = make_animation(m, src, clip, relative=True, adapt_movement_scale=True, cache_dtype=dt)
            d = np.abs(anim[0].permute(1, 2, 3, 0)[:, ::2, ::2, :].cpu().numpy() - g["animation"])
            say(f"   prior {prior}, {name} cache: max |frame - reference frame| {d.max():.3e}, mean {d.mean():.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-animator", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_cache_warps.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to measure without one"
    hip.lib()
    dev = torch.device("cuda", 0)
    say(f"tools/bench_warp_bf16.py --runs {a.runs} --reps {a.reps}   ({torch.cuda.get_device_name(0)}; one process, HIP events, variants alternating run by run)")
    oks = {}
    with torch.no_grad():
        for size, B in ((512, 4), (256, 8)):
            for k, v in warp_sets(dev, size, B, a.runs, a.reps).items():
                oks[f"{k} at {size}^2 batch {B}"] = v
            torch.cuda.empty_cache()
            flush_file(a.out)
        if not a.skip_animator:
            for size, B in ((512, 4), (256, 8)):
                animator_fps(dev, size, B, max(5, a.runs // 2), max(3, a.reps // 2))
                flush_file(a.out)
            frame_distance(dev)
    say("== bf16 median below the fp32 median by more than the two variants' combined run-to-run spread (max - min of each):")
    for k, v in oks.items():
        say(f"   {k}: {'yes' if v else 'NO'}")
    flush_file(a.out)
    # the exit status follows the set a frame issues (the program set); the bench set is recorded beside it for the 1.039 GB figure bench.py reports
    return 0 if all(v for k, v in oks.items() if k.startswith("program set")) else 3


if __name__ == "__main__":
    sys.exit(main())
