"""The best driving frame on the GPU (-m gpu): mrfa_kp_pose_dist against float64 with bounds counted from its own roundings, its running argmin, the
collinear / duplicate / degenerate cases of tests/test_best_frame_cpu.py, what it refuses, and BestFrameSearch (eager and captured) on the dry model."""
import numpy as np
import pytest
import torch

from mrfa_amd import hip
from mrfa_amd.infer import BestFrameSearch, pose_state
from mrfa_amd.utils.prng import det_uniform
from tests.test_best_frame_cpu import INF_BITS, _lattice, demo_dist, wrap_hull

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
CANARY = -1234.5
ICANARY = -7777
PAD = 64                   # canary words on either side of an output and of the state

SHAPES = [(1, 1, 3), (1, 5, 10), (2, 3, 10), (3, 70, 10), (2, 65, 15), (1, 2, 64)]       # (Bs, T, K): 70 and 65 frames are more than the 64 lanes of a source's wave
TRIANGLE = torch.tensor([[-0.5, -0.5], [0.5, -0.5], [-0.5, 0.5]])                        # area 0.5
SUFFIX = {}                # (Bs, T, K) -> tag suffix, where the first draw left best and second best closer than 1e-3 (none needed)


def hull_area64(p):
    q = p.astype(np.float64)
    h = q[wrap_hull(q)]
    return 0.5 * float(np.sum(h[:, 0] * np.roll(h[:, 1], -1) - np.roll(h[:, 0], -1) * h[:, 1]))


def _inputs(Bs, T, K):
    """exact fp32 numbers in [-0.8, 0.8]; a set whose float64 hull area is below 0.05 is replaced by the fixed triangle of area 0.5 (its K - 3 other points
    on the vertices again).  -> kd (Bs T,K,2), ks (Bs,K,2), number of sets replaced"""
    tag = f"bestgpu/{Bs}x{T}x{K}{SUFFIX.get((Bs, T, K), '')}"
    kd, ks = det_uniform(tag + "/kd", (Bs * T, K, 2), -0.8, 0.8), det_uniform(tag + "/ks", (Bs, K, 2), -0.8, 0.8)
    replaced = 0
    for t in (kd, ks):
        for n in range(t.shape[0]):
            if hull_area64(t[n].numpy()) < 0.05:
                t[n] = TRIANGLE[torch.arange(K) % 3]
                replaced += 1
    assert min(hull_area64(s.numpy()) for t in (kd, ks) for s in t) >= 0.05 and max(kd.abs().max(), ks.abs().max()) <= 1
    return kd, ks, replaced


def _reference(p):
    """float64 on the fp32 numbers of one set p (K,2) -> (q, A, n = q / sqrt(A), e_q (K,2), e_A, e_n (K,2)): the exact values and the bounds of the kernel's
    errors on them, as the docstring of test_kernel_against_float64 counts them"""
    p = p.astype(np.float64)
    K = p.shape[0]
    q = p - p.mean(axis=0, keepdims=True)
    e_q = K * U * np.abs(p).mean(axis=0, keepdims=True) + U * np.abs(q)
    hull = wrap_hull(q)
    h = q[hull]
    nx, ny = np.roll(h[:, 0], -1), np.roll(h[:, 1], -1)
    A = 0.5 * float(np.sum(h[:, 0] * ny - nx * h[:, 1]))
    # general position: every other point lies well inside every hull edge, so the kernel's chains hold these vertices whatever its turn tests round to
    for i, j in zip(hull, hull[1:] + hull[:1]):
        turn = (q[j, 0] - q[i, 0]) * (q[:, 1] - q[i, 1]) - (q[j, 1] - q[i, 1]) * (q[:, 0] - q[i, 0])
        assert np.delete(turn, [i, j]).min(initial=1.0) >= 1e-5, "a point within rounding of a hull edge: the bound below does not cover this draw"
    S = float(np.sum(np.abs(h[:, 0] * ny) + np.abs(nx * h[:, 1])))
    e_A = 2 * e_q.max() * float(np.ptp(q[:, 0]) + np.ptp(q[:, 1])) + 0.5 * (K + 1) * U * S
    n = q / np.sqrt(A)
    e_n = e_q / np.sqrt(A) + np.abs(n) * (e_A / (2 * A) + 2 * U)
    return q, A, n, e_q, e_A, e_n


def _bounds(kd, ks, T):
    """float64 dist and area of every frame and the bounds of the kernel's error on them"""
    kd, ks = kd.numpy(), ks.numpy()
    K = kd.shape[1]
    src = [_reference(s) for s in ks]
    dist, area, e_dist, e_area = (np.empty(kd.shape[0]) for _ in range(4))
    for i, f in enumerate(kd):
        _, A, n, _, e_A, e_n = _reference(f)
        _, _, m, _, _, e_m = src[i // T]
        d = n - m
        dist[i], area[i], e_area[i] = float((d * d).sum()), A, 1.01 * e_A
        e_dist[i] = 1.01 * (2 * float((np.abs(d) * (e_n + e_m)).sum()) + (2 * K + 2) * U * dist[i])
    return dist, area, e_dist, e_area


def _guarded(n, dtype=torch.float32):
    canary = CANARY if dtype == torch.float32 else ICANARY
    buf = torch.full((n + 2 * PAD,), canary, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def _intact(buf, n):
    canary = CANARY if buf.dtype == torch.float32 else ICANARY
    return bool((buf[:PAD] == canary).all() and (buf[PAD + n:] == canary).all())


def _launch(kd, ks, T, state=None, dist=True, area=True):
    """one launch on device tensors -> (dist, area) on the CPU; state (Bs,4) int32 on the device is updated in place"""
    B, K = kd.shape[:2]
    dbuf, d = _guarded(B)
    abuf, a = _guarded(B)
    p = lambda t, on=True: t.data_ptr() if on and t is not None else None
    hip.check(hip.lib().mrfa_kp_pose_dist(hip.stream_ptr(), p(kd), p(ks), B, T, K, p(d, dist), p(a, area), p(state)), "mrfa_kp_pose_dist")
    torch.cuda.synchronize()
    for buf, written in ((dbuf, dist), (abuf, area)):
        assert _intact(buf, B), "wrote outside its output"
        assert bool((buf[PAD:PAD + B] == CANARY).any()) != written
    return d.cpu(), a.cpu()


def _state():
    """a fresh state of up to 3 sources inside canary words: (buffer, its words, lambda Bs: the (Bs,4) view)"""
    sbuf, words = _guarded(12, torch.int32)
    words.copy_(pose_state(3, DEV).view(-1))
    return sbuf, words, lambda Bs: words[:4 * Bs].view(Bs, 4)


@pytest.mark.parametrize("Bs,T,K", SHAPES)
def test_kernel_against_float64(Bs, T, K):
    """u = 2^-24; every input is an exact fp32 number in [-1, 1], the expected values are float64 on the same numbers (tests/test_best_frame_cpu.py's
    demo_dist: gift wrapping, not the kernel's chain).  The kernel's roundings in its own order, first order in u:

    Centre: K - 1 additions and one division per coordinate -> |c' - c| <= (K - 1) u mean|p| + u |c| <= K u mean|p|.  q' = fl(p - c') adds one rounding:
    |q' - q| <= e_q = K u mean|p| + u |q|, K + 1 roundings per coordinate.
    Area: (a) the hull of q' against the hull of q.  With e = max e_q, hull(q') lies in hull(q) + [-e, e]^2 and the other way round, and the area of a convex
    set grown by that square is A + 2 e (w_x + w_y) + 4 e^2 (w: its extents) -> |A(q') - A(q)| <= 2 e (w_x + w_y).  (b) the shoelace sum over the E <= K
    hull edges: a term fl(fl(x_i y_j) - fl(x_j y_i)) is off by at most 2 u a_ij, a_ij = |x_i y_j| + |x_j y_i|; the E - 1 additions by at most (E - 1) u sum a
    (every partial sum is at most sum a); the factor 1/2 is exact -> (E + 1) u sum a / 2 <= (K + 1) u S / 2, S = sum a over the float64 hull (_reference
    asserts that no other point is within 1e-5 of a hull edge, so the kernel's chains end on the same vertices).  e_A = 2 e (w_x + w_y) + (K + 1) u S / 2.
    Normalised points: sqrt rounds once (relative e_A / 2A + u), the division once more -> e_n = e_q / sqrt(A) + |n| (e_A / 2A + 2 u); the same for the source.
    Distance: d = fl(n' - m') is off by e_n + e_m + u |d|, its square by 2 |d| (e_n + e_m) + 3 u d^2, and the 2K - 1 additions of the 2K squares by at most
    (2K - 1) u dist -> e_dist = 2 sum |d| (e_n + e_m) + (2K + 2) u dist.
    Every second-order term is a product of two of these relative errors, each below 1e-3 of its quantity for K <= 64 and A >= 0.05: the factor 1.01 on both
    bounds covers them.  A multiplication and an addition contracted into one fused operation removes a rounding and never adds one.  Nothing is measured.
    Also: two runs are bit-identical (state included), nothing outside the outputs and the state is written, the inputs are not written, the state's index is
    the float64 argmin (best and second best more than 1e-3 apart), and the CPU specification (oracle/capi_emulator.py) lies within the same bounds of the kernel."""
    from oracle.capi_emulator import Emulator
    kd, ks, replaced = _inputs(Bs, T, K)
    assert replaced == 0 or K < 10, "det_uniform(-0.8, 0.8) with K >= 10 needs no replacement"
    dist64, area64, e_dist, e_area = _bounds(kd, ks, T)
    best64 = dist64.reshape(Bs, T).argmin(axis=1).tolist()
    if T > 1:
        two = np.sort(dist64.reshape(Bs, T), axis=1)
        assert ((two[:, 1] - two[:, 0]) > 1e-3 * two[:, 0]).all(), "best and second best too close: add a tag suffix for this shape to SUFFIX"
    dkd, dks = kd.to(DEV), ks.to(DEV)
    runs = []
    for _ in range(2):
        sbuf, words, view = _state()
        d, a = _launch(dkd, dks, T, state=view(Bs))
        assert _intact(sbuf, 12) and torch.equal(words[4 * Bs:].cpu(), pose_state(3, "cpu").view(-1)[4 * Bs:]), "wrote outside its sources' state"
        runs.append((d, a, view(Bs).cpu()))
    assert all(torch.equal(x, y) for x, y in zip(*runs)), "two runs differ"
    d, a, st = runs[0]
    ed, ea = np.abs(d.double().numpy() - dist64) / e_dist, np.abs(a.double().numpy() - area64) / e_area
    print(f"[best] Bs={Bs} T={T} K={K}: dist max err / bound {ed.max():.3f} (bound / dist up to {np.max(e_dist / dist64):.2e}), area max err / bound "
          f"{ea.max():.3f} (bound / area up to {np.max(e_area / area64):.2e}), best {st[:, 1].tolist()}")
    assert ed.max() <= 1.0 and ea.max() <= 1.0
    assert st[:, 1].tolist() == best64 and st[:, 2].tolist() == [T] * Bs and st[:, 3].tolist() == [0] * Bs
    assert torch.equal(st[:, 0].view(torch.float32), d.view(Bs, T).min(dim=1).values)
    # the state alone, and the outputs alone
    sbuf, words, view = _state()
    _launch(dkd, dks, T, state=view(Bs), dist=False, area=False)
    assert torch.equal(view(Bs).cpu(), st)
    d2, a2 = _launch(dkd, dks, T)
    assert torch.equal(d2, d) and torch.equal(a2, a)
    # the specification on the same numbers
    e_d, e_a, e_st = torch.full((Bs * T,), CANARY), torch.full((Bs * T,), CANARY), pose_state(Bs, "cpu")
    assert Emulator().mrfa_kp_pose_dist(0, kd.data_ptr(), ks.data_ptr(), Bs * T, T, K, e_d.data_ptr(), e_a.data_ptr(), e_st.data_ptr()) == 0
    assert (np.abs((d.double() - e_d.double()).numpy()) <= e_dist).all() and (np.abs((a.double() - e_a.double()).numpy()) <= e_area).all()
    assert e_st[:, 1:].tolist() == st[:, 1:].tolist()
    assert torch.equal(dkd.cpu(), kd) and torch.equal(dks.cpu(), ks), "inputs must not be written"


def test_groups_ties_nan_and_degenerate_clips():
    """the running argmin over calls of 3, 3 and 1 frames against one call of 7, and the exact-tie, NaN and degenerate cases of the CPU file"""
    kd, ks = det_uniform("bestgpu/state/kd", (14, 10, 2), -0.8, 0.8), det_uniform("bestgpu/state/ks", (2, 10, 2), -0.8, 0.8)

    def run(frames, sizes, sources=ks):
        sbuf, words, view = _state()
        per, dists, t0 = frames.view(2, 7, 10, 2), [], 0
        for T in sizes:
            d, _ = _launch(per[:, t0:t0 + T].reshape(2 * T, 10, 2).contiguous().to(DEV), sources.to(DEV), T, state=view(2))
            dists.append(d.view(2, T))
            t0 += T
        assert _intact(sbuf, 12)
        return view(2).cpu(), torch.cat(dists, dim=1)
    one, d_one = run(kd, [7])
    three, d_three = run(kd, [3, 3, 1])
    ref = [int(np.argmin(demo_dist(kd[7 * s:7 * s + 7].numpy(), ks[s].numpy())[0])) for s in range(2)]
    assert torch.equal(one, three) and torch.equal(d_one, d_three) and one[:, 1].tolist() == ref and one[:, 2].tolist() == [7, 7]
    tie = kd.clone().view(2, 7, 10, 2)
    tie[:, 2] = ks
    tie[:, 5] = ks
    for sizes in ([7], [3, 3, 1]):
        st, d = run(tie.view(14, 10, 2), sizes)
        assert st[:, 1].tolist() == [2, 2] and (d[:, 2] == 0).all() and (d[:, 5] == 0).all(), sizes
    nan = kd.clone().view(2, 7, 10, 2)
    nan[:, ref[0], 3, 1] = float("nan")
    st, d = run(nan.view(14, 10, 2), [3, 3, 1])
    assert torch.isinf(d[:, ref[0]]).all() and st[0, 1].item() == int(d[0].double().argmin()) != ref[0]
    nan[:] = float("nan")
    line = torch.tensor([[0.0625 * i, 0.125 * i] for i in range(10)]).repeat(14, 1, 1)
    for frames, sources in ((nan.view(14, 10, 2), ks), (line, ks), (kd, line[:2].contiguous())):
        st, d = run(frames, [3, 3, 1], sources)
        assert st[:, 1].tolist() == [0, 0] and st[:, 0].tolist() == [INF_BITS] * 2 and st[:, 2].tolist() == [7, 7] and torch.isinf(d).all()


def test_lattice_midpoints_and_duplicates():
    """hull points on hull edges: every number of the computation is exact, the area within 4 u of the exact value; a line and a single point have no area.
    A point listed twice or a little off its edge makes the centre inexact: with K <= 10 points of |p| <= 1 and mean |p| <= 0.5, test_kernel_against_float64's
    count gives e_q <= (10 x 0.5 + 0.6) u = 5.6 u, extents w_x + w_y <= 2.01 and S <= 5 -> e_A <= 22.6 u + 27.5 u: 64 u"""
    lattice = _lattice()
    square = torch.tensor([[-0.5, -0.5], [0.0, -0.5], [0.5, -0.5], [0.5, 0.0], [0.5, 0.5], [0.0, 0.5], [-0.5, 0.5], [-0.5, 0.0]])

    def area_of(pts, against=None):
        dev = pts[None].contiguous().to(DEV)
        d, a = _launch(dev, dev if against is None else against[None].contiguous().to(DEV), 1)
        return a.item(), d.item()
    for pts in (lattice, lattice.flip(0), lattice[torch.tensor([4, 0, 8, 1, 2, 6, 3, 7, 5])], square, square[torch.tensor([3, 0, 6, 1, 7, 2, 5, 4])]):
        a, d = area_of(pts)
        assert abs(a - 1.0) <= 4 * U and d == 0.0, (pts, a, d)
    for pts in (torch.cat([lattice, lattice[:1]], dim=0), torch.cat([square, square[3:4] * 0.5, square[3:4] * 0.5], dim=0)):
        a, d = area_of(pts)
        assert abs(a - 1.0) <= 64 * U and d == 0.0, (pts, a, d)
    for eps in (1e-3, -1e-3):                                  # a midpoint a little off its edge: its distance times half the edge, not a fan counted twice
        bump = square.clone()
        bump[1, 1] -= eps
        off = -(bump[1, 1].double().item() + 0.5)              # the fp32 number's own distance from the edge
        assert abs(area_of(bump)[0] - (1.0 + max(off, 0.0) * 0.5)) <= 64 * U
    line = torch.tensor([[0.125 * i, 0.25 * i] for i in range(8)])
    for kd, ks, flat in ((line, lattice[:8], True), (lattice[:8], line, False), (line, line, True), (lattice[4:5].repeat(8, 1), lattice[:8], True)):
        a, d = area_of(kd, ks)
        assert d == float("inf") and (a == 0.0 if flat else a > 0.1), (kd, ks, a, d)


def test_kernel_refuses_bad_arguments_and_leaves_outputs_and_state_untouched():
    B, rep, K = 6, 3, 10
    kd, ks = det_uniform("bestgpu/bad/kd", (B, K, 2), -0.8, 0.8).to(DEV), det_uniform("bestgpu/bad/ks", (2, K, 2), -0.8, 0.8).to(DEV)
    dbuf, d = _guarded(B)
    abuf, a = _guarded(B)
    sbuf, words, view = _state()
    before = sbuf.clone()
    p = lambda t: t.data_ptr()
    good = dict(kp_d=p(kd), kp_s=p(ks), B=B, rep=rep, K=K, dist_out=p(d), area_out=p(a), state=p(words))
    L = hip.lib()
    for bad in (dict(kp_d=None), dict(kp_s=None), dict(dist_out=None, area_out=None, state=None), dict(B=0), dict(B=-3), dict(rep=0), dict(rep=-1),
                dict(K=0), dict(K=-1), dict(rep=4), dict(rep=5), dict(B=5), dict(K=2), dict(K=1), dict(K=65), dict(kp_d=p(kd) + 4), dict(kp_s=p(ks) + 4),
                dict(dist_out=p(d) + 2), dict(area_out=p(a) + 2), dict(state=p(words) + 2)):
        rc = L.mrfa_kp_pose_dist(hip.stream_ptr(), *{**good, **bad}.values())
        msg = L.mrfa_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and "kp_pose_dist" in msg and len(msg) > 25, (bad, rc, msg)
        assert (dbuf == CANARY).all() and (abuf == CANARY).all() and torch.equal(sbuf, before), bad               # nothing was launched
    hip.check(L.mrfa_kp_pose_dist(hip.stream_ptr(), *good.values()), "mrfa_kp_pose_dist")
    torch.cuda.synchronize()
    assert torch.isfinite(d).all() and torch.isfinite(a).all() and view(2)[:, 2].tolist() == [3, 3] and _intact(sbuf, 12)


# ------------------------------------------------------------------------------------------------------------- BestFrameSearch
def _groups(clip, frames, sizes):
    """the frames `frames` of a clip (Bs,3,T,H,W) as driving batches of sizes[i] frames per source"""
    out, t0 = [], 0
    for T in sizes:
        g = clip[:, :, frames[t0:t0 + T]]
        out.append(g.permute(0, 2, 1, 3, 4).reshape(g.shape[0] * T, g.shape[1], *g.shape[3:]).contiguous())
        t0 += T
    return out


def test_best_frame_search_eager_and_captured(monkeypatch):
    """the FOMM dry configuration at its own size (64 x 64), Bs = 2, a 7-frame clip in groups of 3, 3 and 1: BestFrameSearch(graph=True) against graph=False
    and against the float64 argmin of the eager detector's keypoints; the capture's own replays leave no trace in the state; a second clip after reset()"""
    from tests.test_bf16_cache import _dry_model
    from tests.test_clip_cpu import _clips
    m = _dry_model().to(DEV)
    src, clip = (t.to(DEV) for t in _clips(7))
    with torch.no_grad():
        ks = m.encoder(src)["kp"].cpu().numpy()
        kd = np.stack([m.encoder(clip[:, :, t].contiguous())["kp"].cpu().numpy() for t in range(7)], axis=1)          # (Bs,T,K,2)
    d64 = np.stack([demo_dist(kd[s], ks[s])[0] for s in range(2)])
    second = [4, 5, 6]                                         # the second clip: three frames of the first, one per call
    for sub in (d64, d64[:, second]):
        two = np.sort(sub, axis=1)
        assert ((two[:, 1] - two[:, 0]) > 1e-3 * two[:, 0]).all(), d64
    ref, ref2 = d64.argmin(axis=1).tolist(), d64[:, second].argmin(axis=1).tolist()
    print(f"[best] dry model on the device: float64 distances {np.round(d64, 4).tolist()}, best {ref}, of frames {second}: {ref2}")
    assert ref != ref2
    replays = []
    real = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(id(self)), real(self))[1])
    results = {}
    for graph in (False, True):
        search = BestFrameSearch(m, graph=graph)
        search.set_source(src)
        seen = []
        for g in _groups(clip, list(range(7)), [3, 3, 1]):
            search.add(g)
            seen.append(search.state[:, 2].tolist())
        assert seen == [[3, 3], [6, 6], [7, 7]], seen        # a capture (T = 3 at the first add, T = 1 at the third) shows only the frames added
        results[graph] = search.result()
        assert sorted(search._graphs) == ([1, 3] if graph else [])
        search.reset()
        del replays[:]
        for g in _groups(clip, second, [1, 1, 1]):
            search.add(g)
        if graph:                                              # T = 1 was captured above: three adds are three replays of that one program
            assert replays == [id(search._graphs[1][0])] * 3, replays
        assert search.state[:, 2].tolist() == [3, 3] and search.result() == ref2
    assert results[False] == results[True] == ref
