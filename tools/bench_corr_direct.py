"""One refinement level's correlation, both ways, on RaftFlow's shapes: mrfa_corr_direct_fwd against the two volume GEMMs + mrfa_corr_lookup_fwd it replaces.

    python tools/bench_corr_direct.py --size 512 --batch 1 --rounds 7
    python tools/bench_corr_direct.py --size 256 --batch 8 --key-rep 8      # a clip: 8 frames of ONE source (query image n reads key image n // 8), and
                                                                            # beside it the same queries against the keys physically repeated 8 times

A size^2 frame has h = w = size/4 keys of 256 channels and query levels of h/8 .. h pixels a side; the six refinement iterations look up at h/8, h/4, h/2, h,
h, h, and the volume path correlates every query level ONCE per frame (two GEMMs) however often it is looked up.  Device events around each launch, the two
ways alternating round by round in one process, medians and min-max.  Random features, coordinates = the identity correspondence + up to two pixels."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfa_amd.engine import Ctx  # noqa: E402
from mrfa_amd.modules.raft import _CorrVolume  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--key-rep", type=int, default=1, help="frames per source: --batch query images share --batch / --key-rep key images")
a = ap.parse_args()

dev = torch.device("cuda", 0)
B, h, D, T = a.batch, a.size // 4, a.channels, a.key_rep
if T < 1 or B % T:
    ap.error(f"--key-rep {T} must divide --batch {B}")
scale = D ** -0.5
e = Ctx(dev, train=False, record=False)
g = torch.Generator().manual_seed(0)


def rand(n, hh, ww, c):
    v = e.new(n, hh, ww, c)
    v.tensor().copy_(torch.randn(n, hh, ww, c, generator=g))
    return v


def ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def fmt(ts):
    return f"{statistics.median(ts):8.3f} ms ({min(ts):.3f} - {max(ts):.3f})"


k_s = rand(B // T, h, h, D)
k_pool = e.avgpool2(k_s)
if T > 1:                                                     # the parent's workaround: every frame its own copy of the keys
    k_rep = e.new(B, h, h, D)
    k_rep.tensor().copy_(k_s.tensor().repeat_interleave(T, dim=0))
    k_rep_pool = e.avgpool2(k_rep)
tot = {"gemm": 0.0, "lookup": 0.0, "direct": 0.0, "direct_rep": 0.0}
with torch.no_grad():
    for r, uses in ((h // 8, 1), (h // 4, 1), (h // 2, 1), (h, 3)):
        q = rand(B, r, r, D)
        ys, xs = torch.meshgrid(torch.arange(r, dtype=torch.float32), torch.arange(r, dtype=torch.float32), indexing="ij")
        c = torch.stack([xs, ys], dim=-1)[None].expand(B, r, r, 2) * (h / r) + torch.rand(B, r, r, 2, generator=g) * 4 - 2
        coords = e.new(B, r, r, 2)
        coords.tensor().copy_(c)
        out_v, out_d = e.new(B, r, r, 98, pad32=True), e.new(B, r, r, 98, pad32=True)
        vol = _CorrVolume(e, q, k_s, k_pool, scale)
        t = {"gemm": [], "lookup": [], "direct": [], "direct_rep": []}
        for i in range(3 + a.rounds):
            tg = ms(lambda: _CorrVolume(e, q, k_s, k_pool, scale))
            tl = ms(lambda: e.corr_lookup(vol.vol0, vol.vol1, None, h, h, coords, out=out_v))
            td = ms(lambda: e.corr_direct(q, k_s, k_pool, coords, scale, out=out_d, k_rep=T))
            tr = ms(lambda: e.corr_direct(q, k_rep, k_rep_pool, coords, scale, out=out_v)) if T > 1 else 0.0
            if i >= 3:
                t["gemm"].append(tg), t["lookup"].append(tl), t["direct"].append(td), t["direct_rep"].append(tr)
        same = f"  direct on repeated keys {fmt(t['direct_rep'])} bit-identical {torch.equal(out_v.tensor(), out_d.tensor())}" if T > 1 else ""
        e.corr_lookup(vol.vol0, vol.vol1, None, h, h, coords, out=out_v)
        diff = (out_v.tensor() - out_d.tensor()).abs().max().item()
        print(f"{a.size}^2 B={B} level {r}x{r} ({B * r * r} queries, looked up {uses}x per frame): volume GEMMs {fmt(t['gemm'])}  lookup {fmt(t['lookup'])}  "
              f"direct {fmt(t['direct'])}  max |direct - lookup| {diff:.2e}{same}")
        tot["gemm"] += statistics.median(t["gemm"])
        tot["lookup"] += uses * statistics.median(t["lookup"])
        tot["direct"] += uses * statistics.median(t["direct"])
        tot["direct_rep"] += uses * statistics.median(t["direct_rep"])
        del vol
print(f"{a.size}^2 B={B} per frame (medians; GEMMs once per level, lookups per use): volume GEMMs {tot['gemm']:.3f} + lookups {tot['lookup']:.3f} = "
      f"{tot['gemm'] + tot['lookup']:.3f} ms; direct {tot['direct']:.3f} ms" + (f" (key-rep {T}; on repeated keys {tot['direct_rep']:.3f} ms)" if T > 1 else ""))
