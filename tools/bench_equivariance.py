"""The equivariance constraint on its two paths -- torch ops (GeneratorFullLoss(equivariance="torch"), the default) and the three launches of
mrfa_amd.equivariance ("library") -- measured in ONE process on one MI355X:

  1. the reference-objective training step (B = 8, 256^2, GraphedTrainStep with the full objective, bench.py's VGG initialisation), both priors: the two
     paths ALTERNATE for ROUNDS rounds of STEPS timed replays each; medians and spread per path, and the per-round differences;
  2. the three pieces alone between device events (frame warp, terms forward, terms backward; B = 8, K = 10, 5 x 5 control points), launched eagerly and --
     warp, and terms forward + backward -- as hipGraph replays, where no host cost is left and only the dependent chain counts;
  3. device launches per piece on either path (torch.profiler's kernel records of one eager pass, in a pass of its own).

    python tools/bench_equivariance.py [OUT]            (default OUT: profiles/equivariance.txt; needs a GPU)"""
import os
import statistics
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from mrfa_amd import graph_replay_safe
from mrfa_amd.equivariance import equivariance_terms, transform_frame
from mrfa_amd.graph import GraphedTrainStep
from mrfa_amd.losses import GeneratorFullLoss, Transform, Vgg19, _inv2x2
from mrfa_amd.train import VOX1, HotPath, make_optimizer, reference_loss, train_step
from mrfa_amd.utils.prng import det_normal, det_uniform, fill_state_dict

ROUNDS, STEPS, WARM = 5, 20, 3
PIECE_REPS = 50
PATHS = ("torch", "library")
TRANSFORM = dict(sigma_affine=0.05, sigma_tps=0.005, points_tps=5)
TRAIN_PARAMS = dict(scales=[1, 0.5, 0.25, 0.125], transform_params=TRANSFORM,
                    loss_weights=dict(perceptual=[10, 10, 10, 10, 10], equivariance=10, equivariance_jacobian=10))
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def spread(xs):
    return f"median {statistics.median(xs):8.3f}  min {min(xs):8.3f}  max {max(xs):8.3f}"


def bench_vgg(dev):
    """bench.py's VGG initialisation (He-uniform, positive biases: dense activations through all 16 layers)"""
    vgg = Vgg19()
    vsd = vgg.state_dict()
    new = fill_state_dict({k: v for k, v in vsd.items() if k not in ("mean", "std")}, tag="vgg")
    new.update({k: v.abs() * 0.5 for k, v in new.items() if k.endswith(".bias")})
    new["mean"], new["std"] = vsd["mean"], vsd["std"]
    vgg.load_state_dict(new)
    return vgg.to(dev)


# ------------------------------------------------------------------------------------------------------------------------------------- 1. the step
def steps(dev):
    vgg = bench_vgg(dev)
    src, drv = det_uniform("bench/src/r0", (8, 3, 256, 256), 0, 1).to(dev), det_uniform("bench/drv/r0", (8, 3, 256, 256), 0, 1).to(dev)
    for prior in ("mtia", "fomm"):
        model = HotPath(VOX1, prior=prior)
        bench.init_weights(model)
        model.to(dev).train(True)
        opt = make_optimizer(model, fused=True)
        train_step(model, opt, src, drv)
        graphed = {}
        for path in PATHS:
            full = GeneratorFullLoss(TRAIN_PARAMS, vgg, equivariance=path).to(dev)
            graphed[path] = GraphedTrainStep(model, opt, src, drv, loss_fn=lambda m, s, d, full=full: reference_loss(m, full, s, d))
        times = {p: [] for p in PATHS}
        for _ in range(ROUNDS):
            for path in PATHS:
                g = graphed[path]
                for _ in range(WARM):
                    g(src, drv)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(STEPS):
                    g(src, drv)
                b.record()
                torch.cuda.synchronize()
                times[path].append(a.elapsed_time(b) / STEPS)
        say(f"reference-objective step, prior {prior}, B = 8, 256^2, hipGraph replay: ms per step, {ROUNDS} alternating rounds of {STEPS} replays")
        for path in PATHS:
            say(f"  {path:8s} {spread(times[path])}   rounds: " + " ".join(f"{t:.3f}" for t in times[path]))
        diffs = [t - l for t, l in zip(times["torch"], times["library"])]
        say(f"  torch - library per round: " + " ".join(f"{d:+.3f}" for d in diffs) + f"   median {statistics.median(diffs):+.3f} ms")
        say()
        del graphed, model, opt
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------------------- 2. the pieces
def torch_terms(t, kp_d, jac_d, kp_t, jac_t):
    value = 10 * torch.abs(kp_d - t.warp_coordinates(kp_t)).mean()
    v = torch.matmul(_inv2x2(jac_d), torch.matmul(t.jacobian(kp_t), jac_t))
    return value, 10 * torch.abs(torch.eye(2, device=v.device).view(1, 1, 2, 2) - v)


def library_terms(t, kp_d, jac_d, kp_t, jac_t):
    out = equivariance_terms(t, {"kp": kp_d, "jacobian": jac_d}, {"kp": kp_t, "jacobian": jac_t}, 10.0, 10.0)
    return out["equivariance"], out["equivariance_jacobian"]


def timed(fn, reps=PIECE_REPS, before=None):
    """fn() between two device events, `reps` times (before() outside the events); milliseconds"""
    out = []
    for i in range(reps + 5):
        state = before() if before else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(state) if before else fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 5:
            out.append(a.elapsed_time(b))
    return out


def replayed(fn, reps=PIECE_REPS):
    """fn() captured into a hipGraph; the replay between two device events"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    res = timed(g.replay, reps)
    del keep
    return res


def pieces(dev):
    B, K = 8, 10
    t = Transform(B, generator=torch.Generator(device=dev).manual_seed(1), device=dev, **TRANSFORM)
    frame = det_uniform("bench/drv/r0", (B, 3, 256, 256), 0, 1).to(dev)
    leaves = [det_uniform("equiv/kp_d", (B, K, 2), -0.8, 0.8), torch.eye(2).view(1, 1, 2, 2) + 0.1 * det_normal("equiv/jac_d", (B, K, 2, 2)),
              det_uniform("equiv/kp_t", (B, K, 2), -0.8, 0.8), torch.eye(2).view(1, 1, 2, 2) + 0.1 * det_normal("equiv/jac_t", (B, K, 2, 2))]
    leaves = [x.to(dev).requires_grad_(True) for x in leaves]
    warp = {"torch": lambda: t.transform_frame(frame), "library": lambda: transform_frame(t, frame)}
    terms = {"torch": torch_terms, "library": library_terms}

    def loss_of(path):
        value, term = terms[path](t, *leaves)
        return value + term.mean()

    def fwd_bwd(path):
        return torch.autograd.grad(loss_of(path), leaves)

    say(f"the pieces alone, B = {B}, K = {K}, 256^2, 25 control points: microseconds between device events, {PIECE_REPS} repetitions")
    rows = [("frame warp, eager", {p: timed(warp[p]) for p in PATHS}),
            ("terms forward, eager", {p: timed(lambda p=p: loss_of(p)) for p in PATHS}),
            ("terms backward, eager", {p: timed(lambda loss: torch.autograd.grad(loss, leaves), before=lambda p=p: loss_of(p)) for p in PATHS}),
            ("frame warp, graph replay", {p: replayed(warp[p]) for p in PATHS}),
            ("terms forward + backward, graph replay", {p: replayed(lambda p=p: fwd_bwd(p)) for p in PATHS})]
    for name, res in rows:
        say(f"  {name}")
        for p in PATHS:
            say(f"    {p:8s} {spread([1e3 * x for x in res[p]])}")
    say()
    # ---- 3. launches: kernel records of one eager pass per piece, the profiler on (a pass of its own: its timings are not used)
    from torch.profiler import ProfilerActivity, profile

    def kernels(fn):
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = prof.events()
        dev_ev = [e for e in ev if str(getattr(e, "device_type", "")).endswith("CUDA")]
        return len(dev_ev), sum(1 for e in ev if e.name.startswith("aten::"))

    say("device launches (kernels and copies the profiler records on the device) and aten:: operator calls of one eager pass")
    for name, fns in (("frame warp", warp), ("terms forward + backward", {p: (lambda p=p: fwd_bwd(p)) for p in PATHS})):
        for p in PATHS:
            n_dev, n_aten = kernels(fns[p])
            say(f"  {name:26s} {p:8s} device launches {n_dev if n_dev else 'not recorded by this build of the profiler':>5}   aten:: calls {n_aten}")
    say()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "equivariance.txt")
    assert torch.cuda.is_available(), "bench_equivariance.py measures on a GPU; there is no CPU figure"
    graph_replay_safe("bench_equivariance")
    dev = torch.device("cuda", 0)
    say(f"tools/bench_equivariance.py on {torch.cuda.get_device_name(0)}: GeneratorFullLoss(equivariance=\"torch\") against \"library\", one process")
    say()
    pieces(dev)
    steps(dev)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
