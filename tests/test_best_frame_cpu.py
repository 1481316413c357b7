"""The best driving frame from the model's keypoints, on the CPU through the specification of mrfa_kp_pose_dist (oracle/capi_emulator.py on oracle/infer_spec.py): the entry against
scipy's hull and demo.py:78-94 written out in numpy, collinear and duplicate points, rep, the running argmin, what it refuses, find_best_frame and
make_animation(initial_frame="best") on the dry model."""
import numpy as np
import pytest
import torch

from mrfa_amd import engine, hip
from mrfa_amd.infer import Animator, BestFrameSearch, find_best_frame, make_animation, pose_state
from tests import cases
from oracle.capi_emulator import Emulator
from tests.emu import emulated_hip

CANARY = -1234.5
PAD = 8
INF_BITS = 0x7F800000


def wrap_hull(q):
    """the hull vertices (indices, counter-clockwise) of (K,2) float64 points in general position by gift wrapping (an algorithm the specification does not
    use): from the lowest-left point, the next vertex is the one no other point lies to the right of"""
    n = len(q)
    start = min(range(n), key=lambda i: (q[i, 0], q[i, 1]))
    hull, cur = [], start
    while True:
        hull.append(cur)
        nxt = (cur + 1) % n
        for r in range(n):
            if r != cur and (q[nxt, 0] - q[cur, 0]) * (q[r, 1] - q[cur, 1]) - (q[nxt, 1] - q[cur, 1]) * (q[r, 0] - q[cur, 0]) < 0:
                nxt = r
        cur = nxt
        if cur == start:
            return hull
        assert len(hull) <= n


def _wrap_area(q):
    h = q[wrap_hull(q)]
    return 0.5 * float(np.sum(h[:, 0] * np.roll(h[:, 1], -1) - np.roll(h[:, 0], -1) * h[:, 1]))


def demo_dist(kd, ks, area=_wrap_area):
    """demo.py:78-94 in numpy float64 with the landmarks replaced by keypoints: frames kd (T,K,2) against ONE source ks (K,2) -> (dist (T), area (T))"""
    def normalize_kp(kp):
        kp = kp - kp.mean(axis=0, keepdims=True)
        a = area(kp)
        return kp / np.sqrt(a), a
    src, _ = normalize_kp(ks.astype(np.float64))
    out = [normalize_kp(f.astype(np.float64)) for f in kd]
    return np.array([(np.abs(src - n) ** 2).sum() for n, _ in out]), np.array([a for _, a in out])


def _entry(emu, kd, ks, rep=1, state=None, dist=True, area=True, **over):
    """one call of the entry on (B,K,2) / (B/rep,K,2) fp32 tensors -> (rc, dist_out, area_out), the outputs inside canary floats; over: arguments by name"""
    B, K = kd.shape[:2]
    dbuf, abuf = torch.full((B + 2 * PAD,), CANARY), torch.full((B + 2 * PAD,), CANARY)
    p = lambda t: t.data_ptr()
    a = dict(kp_d=p(kd), kp_s=p(ks), B=B, rep=rep, K=K, dist_out=p(dbuf) + 4 * PAD if dist else None, area_out=p(abuf) + 4 * PAD if area else None,
             state=state if state is None or isinstance(state, int) else p(state))
    a.update(over)
    rc = emu.mrfa_kp_pose_dist(0, **a)
    for buf in (dbuf, abuf):
        assert (buf[:PAD] == CANARY).all() and (buf[PAD + B:] == CANARY).all(), "wrote outside its output"
    return rc, dbuf[PAD:PAD + B], abuf[PAD:PAD + B]


def _best(state):
    return state[:, 1].tolist()


def test_specification_against_scipy_and_the_demo_arithmetic():
    ConvexHull = pytest.importorskip("scipy.spatial").ConvexHull
    emu = Emulator()
    for K in (3, 10, 15):
        kd, ks = cases.keypoints(f"best/spec{K}/kd", 20, K)["kp"], cases.keypoints(f"best/spec{K}/ks", 2, K)["kp"]
        rc, dist, area = _entry(emu, kd, ks, rep=10)
        assert rc == 0
        for s in range(2):
            frames = kd[10 * s:10 * s + 10].numpy()
            ref_d, _ = demo_dist(frames, ks[s].numpy(), area=lambda q: ConvexHull(q).volume)
            ref_a = np.array([ConvexHull(f.astype(np.float64)).volume for f in frames])          # (the area does not move with the centring)
            ea = np.abs(area[10 * s:10 * s + 10].double().numpy() - ref_a) / ref_a
            ed = np.abs(dist[10 * s:10 * s + 10].double().numpy() - ref_d) / ref_d
            print(f"[best] K={K} source {s}: area max rel err {ea.max():.3e}, dist max rel err {ed.max():.3e}, smallest area {ref_a.min():.3e}")
            assert ea.max() <= 1e-6 and ed.max() <= 1e-5
            mine_d, mine_a = demo_dist(frames, ks[s].numpy())                                        # the test's own hull agrees with scipy's
            assert np.abs(mine_a - ref_a).max() <= 1e-12 and np.abs(mine_d - ref_d).max() <= 1e-9 * ref_d.max()


def _lattice():
    return torch.tensor([[0.5 * i, 0.5 * j] for i in range(3) for j in range(3)])


def test_collinear_hull_points_and_duplicates():
    emu = Emulator()
    lattice = _lattice()                                                                         # every edge of the hull carries a third point
    square = torch.tensor([[-0.5, -0.5], [0.0, -0.5], [0.5, -0.5], [0.5, 0.0], [0.5, 0.5], [0.0, 0.5], [-0.5, 0.5], [-0.5, 0.0]])
    for pts, exact in ((lattice, 1.0), (lattice.flip(0), 1.0), (lattice[torch.tensor([4, 0, 8, 1, 2, 6, 3, 7, 5])], 1.0), (square, 1.0),
                       (square[torch.tensor([3, 0, 6, 1, 7, 2, 5, 4])], 1.0)):
        rc, dist, area = _entry(emu, pts[None].contiguous(), pts[None].contiguous())
        assert rc == 0 and area.item() == exact and dist.item() == 0.0, (pts, area, dist)
    twice = torch.cat([lattice, lattice[:1]], dim=0)                                             # a corner listed twice: the centre moves, the hull does not
    rc, dist, area = _entry(emu, twice[None].contiguous(), twice[None].contiguous())
    assert rc == 0 and abs(area.item() - 1.0) <= 2.0 ** -23 and dist.item() == 0.0               # (float64 to a few 1e-16, then ONE fp32 rounding: an ulp of 1)
    inner = torch.cat([square, square[3:4] * 0.5, square[3:4] * 0.5], dim=0)                     # an interior point listed twice
    assert abs(_entry(emu, inner[None].contiguous(), inner[None].contiguous())[2].item() - 1.0) <= 2.0 ** -23
    line = torch.tensor([[0.125 * i, 0.25 * i] for i in range(8)])                               # all on one line: no area, no pose
    for kd, ks in ((line, lattice[:8]), (lattice[:8], line), (line, line)):
        rc, dist, area = _entry(emu, kd[None].contiguous(), ks[None].contiguous())
        assert rc == 0 and dist.item() == float("inf")
        assert area.item() == (0.0 if kd is line else area.item()) and torch.isfinite(area).all()
    same = lattice[4:5].repeat(5, 1)                                                             # one point five times
    rc, dist, area = _entry(emu, same[None].contiguous(), lattice[None, :5].contiguous())
    assert rc == 0 and area.item() == 0.0 and dist.item() == float("inf")
    # a point a little off an edge changes the area by its distance times half the edge, not by a fan counted twice
    for eps in (1e-3, -1e-3, 1e-6):
        bump = square.clone()
        bump[1, 1] -= eps                                                                        # the midpoint of the lower edge, outwards for eps > 0
        a = _entry(emu, bump[None].contiguous(), bump[None].contiguous())[2].item()
        assert abs(a - (1.0 + max(eps, 0.0) * 0.5)) <= 2e-7, (eps, a)


def test_rep_reads_source_n_div_rep():
    emu, rep = Emulator(), 3
    kd, ks = cases.keypoints("best/rep/kd", 6, 15)["kp"], cases.keypoints("best/rep/ks", 2, 15)["kp"]
    rc, dist, area = _entry(emu, kd, ks, rep=rep)
    rc1, dist1, area1 = _entry(emu, kd, ks.repeat_interleave(rep, dim=0).contiguous(), rep=1)
    assert rc == 0 and rc1 == 0 and torch.equal(dist, dist1) and torch.equal(area, area1) and torch.isfinite(dist).all()
    _, dist2, _ = _entry(emu, kd, ks.repeat(rep, 1, 1).contiguous(), rep=1)                      # source n % rep
    assert not torch.equal(dist, dist2)


def test_state_one_call_against_three():
    emu = Emulator()
    kd, ks = cases.keypoints("best/state/kd", 14, 10)["kp"], cases.keypoints("best/state/ks", 2, 10)["kp"]

    def run(frames, sizes, sources=ks):
        state, dists, t0 = pose_state(sources.shape[0], "cpu"), [], 0
        view = frames.view(sources.shape[0], -1, *frames.shape[1:])
        for T in sizes:
            rc, dist, _ = _entry(emu, view[:, t0:t0 + T].reshape(-1, *frames.shape[1:]).contiguous(), sources, rep=T, state=state)
            assert rc == 0
            dists.append(dist.view(-1, T))
            t0 += T
        return state, torch.cat(dists, dim=1)
    one, d_one = run(kd, [7])
    three, d_three = run(kd, [3, 3, 1])
    assert torch.equal(one, three) and torch.equal(d_one, d_three)
    ref = [int(np.argmin(demo_dist(kd[7 * s:7 * s + 7].numpy(), ks[s].numpy())[0])) for s in range(2)]
    assert _best(one) == ref == d_one.double().argmin(dim=1).tolist()
    assert one[:, 2].tolist() == [7, 7] and one[:, 3].tolist() == [0, 0]
    assert torch.equal(one[:, 0].view(torch.float32), d_one.min(dim=1).values)
    assert len(set(ref)) == 2 or ref[0] != 0, "the two sources should not both answer 0"
    # state only, no distances: the same answer
    state = pose_state(2, "cpu")
    assert _entry(emu, kd, ks, rep=7, state=state, dist=False, area=False)[0] == 0 and torch.equal(state, one)
    # two bit-identical frames that are both the minimum: the earlier one, within a call and across calls
    tie = kd.clone().view(2, 7, 10, 2)
    tie[:, 2] = ks
    tie[:, 5] = ks
    for sizes in ([7], [3, 3, 1], [1] * 7):
        st, d = run(tie.view(14, 10, 2), sizes)
        assert _best(st) == [2, 2] and (d[:, 2] == 0).all() and (d[:, 5] == 0).all(), sizes
    # a NaN frame never wins; it does not stop the frames behind it from winning either
    nan = kd.clone().view(2, 7, 10, 2)
    nan[:, ref[0], 3, 1] = float("nan")
    st, d = run(nan.view(14, 10, 2), [3, 3, 1])
    assert torch.isinf(d[:, ref[0]]).all() and _best(st)[0] == int(d[0].double().argmin()) != ref[0]
    nan[:] = float("nan")
    st, d = run(nan.view(14, 10, 2), [3, 3, 1])
    assert _best(st) == [0, 0] and st[:, 0].tolist() == [INF_BITS] * 2 and st[:, 2].tolist() == [7, 7] and torch.isinf(d).all()
    # an all-degenerate clip (every frame on one line), and a degenerate source: index 0, as the reference's loop
    line = torch.tensor([[0.0625 * i, 0.125 * i] for i in range(10)]).repeat(14, 1, 1)
    for frames, sources in ((line, ks), (kd, line[:2].contiguous())):
        st, d = run(frames, [3, 3, 1], sources)
        assert _best(st) == [0, 0] and st[:, 0].tolist() == [INF_BITS] * 2 and st[:, 2].tolist() == [7, 7] and torch.isinf(d).all()


def test_entry_refuses_bad_arguments_and_leaves_outputs_and_state_untouched():
    emu = Emulator()
    kd, ks = cases.keypoints("best/bad/kd", 6)["kp"], cases.keypoints("best/bad/ks", 2)["kp"]
    state = pose_state(2, "cpu")
    state[:, 1:] = 77
    before = state.clone()
    rc, dist, area = _entry(emu, kd, ks, rep=3)
    assert rc == 0 and not (dist == CANARY).any() and not (area == CANARY).any()
    p = lambda t: t.data_ptr()
    bads = [dict(kp_d=None), dict(kp_s=None), dict(dist_out=None, area_out=None, state=None),                       # null inputs, nothing to write
            dict(B=0), dict(B=-3), dict(rep=0), dict(rep=-1), dict(K=0), dict(K=-1),                                  # sizes < 1
            dict(rep=4), dict(rep=5), dict(B=5),                                                                      # B % rep != 0
            dict(K=2), dict(K=1), dict(K=65),                                                                         # no hull / more than the kernel holds
            dict(kp_d=p(kd) + 4), dict(kp_s=p(ks) + 4), dict(state=p(state) + 2)]                                     # misaligned
    for bad in bads:
        rc, dist, area = _entry(emu, kd, ks, **{"rep": 3, "state": state, **bad})
        assert rc != 0 and b"kp_pose_dist" in emu.mrfa_last_error() and len(emu.mrfa_last_error()) > 25, bad
        assert (dist == CANARY).all() and (area == CANARY).all() and torch.equal(state, before), bad
    buf = torch.full((16,), CANARY)
    for name in ("dist_out", "area_out"):
        assert emu.mrfa_kp_pose_dist(0, p(kd), p(ks), 6, 3, 10, **{"dist_out": None, "area_out": None, "state": p(state), name: p(buf) + 2}) != 0
        assert (buf == CANARY).all() and torch.equal(state, before)


def test_ctx_checks_shapes_and_a_recording_context():
    kd, ks = cases.keypoints("best/ctx/kd", 6)["kp"], cases.keypoints("best/ctx/ks", 2)["kp"]
    with emulated_hip(counting=True) as lib:
        e = engine.Ctx(torch.device("cpu"), train=False, record=False)
        launches = lambda: [c for c, _ in lib.calls if c != "mrfa_get_mfma_mode"]                # (the host-side mode query of every new context)
        n = len(launches())
        for args, kw in (((kd, ks), dict(rep=2)), ((kd, ks[:, :9]), dict(rep=3)), ((kd[..., :1], ks), dict(rep=3)), ((kd[:, :2], ks[:, :2]), dict(rep=3)),
                         ((kd, ks), dict(rep=3, want_dist=False)), ((kd, ks), dict(rep=3, state=pose_state(3, "cpu"))),
                         ((kd, ks), dict(rep=3, state=torch.zeros(2, 4)))):
            with pytest.raises(ValueError, match="kp_pose_dist"):
                e.kp_pose_dist(*args, **kw)
        with pytest.raises(RuntimeError, match="no backward"):
            engine.Ctx(torch.device("cpu"), train=False, record=True).kp_pose_dist(kd, ks, rep=3)
        assert len(launches()) == n                                                              # refused before anything was launched
        flat = torch.zeros(6 * 10 * 2 + 1)
        odd = flat[1:].view(6, 10, 2).copy_(kd)                                                  # 4 bytes past an 8-byte boundary: copied, not refused
        assert odd.data_ptr() % 8 == 4
        dist, area = e.kp_pose_dist(odd, ks, rep=3, want_area=True)
        ref, _ = e.kp_pose_dist(kd, ks, rep=3)
        assert torch.equal(dist, ref) and area.shape == (6,) and launches()[n:] == ["mrfa_kp_pose_dist"] * 2


_MODEL = []


def _model_and_clips(n):
    """the dry model (built once: filling its weights is most of a test's time; nobody modifies it), the Bs sources and an n-frame clip"""
    from tests.test_bf16_cache import _dry_model
    from tests.test_clip_cpu import _clips
    if not _MODEL:
        _MODEL.append(_dry_model())
    return (_MODEL[0],) + _clips(n)


def test_find_best_frame_on_the_dry_model(monkeypatch):
    with emulated_hip(counting=True) as lib:
        m, src, clip = _model_and_clips(5)
        with torch.no_grad():
            ks = m.encoder(src)["kp"].numpy()
            kd = np.stack([m.encoder(clip[:, :, t].contiguous())["kp"].numpy() for t in range(5)], axis=1)          # (Bs,T,K,2)
        d64 = np.stack([demo_dist(kd[s], ks[s])[0] for s in range(2)])
        ref = d64.argmin(axis=1).tolist()
        two = np.sort(d64, axis=1)
        print(f"[best] dry model, float64 distances {d64.tolist()}")
        assert ((two[:, 1] - two[:, 0]) / two[:, 0] > 1e-3).all()                                 # what separates best from second best is no rounding
        reads = []
        for name in ("tolist", "item", "cpu", "numpy"):                                          # (float() / int() are the emulator's own, on its host memory)
            real = getattr(torch.Tensor, name)
            monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **k: (reads.append(_name), _real(self, *a, **k))[1])
        results = []
        for fpc in (1, 2, 5):
            del lib.calls[:], reads[:]
            search = BestFrameSearch(m)
            search.set_source(src)
            for t0 in range(0, 5, fpc):
                T = min(fpc, 5 - t0)
                search.add(clip[:, :, t0:t0 + T].permute(0, 2, 1, 3, 4).reshape(2 * T, 3, *clip.shape[3:]).contiguous())
            assert not reads, reads                                                              # nothing read the device before result()
            results.append(search.result())
            assert reads == ["tolist"]
            calls = [a for n, a in lib.calls if n == "mrfa_kp_pose_dist"]
            sizes = [min(fpc, 5 - t0) for t0 in range(0, 5, fpc)]
            assert [(a[3], a[4], a[5]) for a in calls] == [(2 * T, T, 10) for T in sizes]        # once per group: (B, rep, K)
            assert all(a[6] is None and a[7] is None and a[8] == search.state.data_ptr() for a in calls)      # the state alone
            assert search.state[:, 2].tolist() == [5, 5]
            del lib.calls[:]
            assert find_best_frame(m, src, clip, frames_per_call=fpc) == results[-1]
            assert [n for n, _ in lib.calls].count("mrfa_kp_pose_dist") == len(sizes)
        assert results == [ref] * 3
        # a second clip on the same object after reset(): its own answer
        search.reset()
        assert search.state[:, 2].tolist() == [0, 0]
        search.add(clip.flip(2).permute(0, 2, 1, 3, 4).reshape(10, 3, *clip.shape[3:]).contiguous())
        assert search.state[:, 2].tolist() == [5, 5] and search.result() == [4 - i for i in ref] != ref
        with pytest.raises(ValueError, match="frames_per_call"):
            find_best_frame(m, src, clip, frames_per_call=0)
        with pytest.raises(ValueError, match=r"3.*2"):
            search.add(clip[:, :, 0][[0, 1, 0]].contiguous())


def test_make_animation_best_equals_the_index_it_found():
    """Bs = 1: "best" is the search plus make_animation(initial_frame=that index), bit for bit; the values refused before still raise"""
    with emulated_hip(counting=True) as lib:
        m, src, clip = _model_and_clips(3)
        one_src, one_clip = src[:1].contiguous(), clip[:1].contiguous()
        best = find_best_frame(m, one_src, one_clip)
        del lib.calls[:]
        a = make_animation(m, one_src, one_clip, initial_frame="best", frames_per_call=2)
        assert [args[4] for n, args in lib.calls if n == "mrfa_kp_pose_dist"] == [2, 1]           # the search ran with the same groups
        assert torch.equal(a, make_animation(m, one_src, one_clip, initial_frame=best[0], frames_per_call=2))
        del lib.calls[:]
        make_animation(m, src, clip[:, :, :1].contiguous(), relative=False, initial_frame="best")  # no initial frame to look for
        assert "mrfa_kp_pose_dist" not in [n for n, _ in lib.calls]
        for bad in (3, -1, 1.0, "worst", [0], [0, 3], [0, 1.0], (0, 1, 2), None):
            with pytest.raises(ValueError, match="initial_frame"):
                make_animation(m, src, clip, initial_frame=bad)


def test_make_animation_best_finds_the_source_in_the_clip():
    """a clip that holds the source as frame 2: that frame is the best, and the animation from it reproduces the source there"""
    from tests.test_clip_cpu import _gate
    with emulated_hip():
        m, src, clip = _model_and_clips(3)
        clip[:, :, 2] = src
        assert find_best_frame(m, src, clip, frames_per_call=3) == [2, 2]
        b = make_animation(m, src, clip, adapt_movement_scale=True, initial_frame="best", frames_per_call=3)
        absolute = Animator(m)
        absolute.set_source(src)
        _gate(b[:, :, 2], absolute(src), "initial_frame='best': frame 2 vs the self-reconstruction")
        assert (b[:, :, 0] - b[:, :, 2]).abs().max().item() > 1e-3


def test_make_animation_takes_one_initial_frame_per_source():
    with emulated_hip():
        m, src, clip = _model_and_clips(2)
        c = make_animation(m, src, clip, initial_frame=[0, 1], frames_per_call=2)
        r = make_animation(m, src, clip, initial_frame=0, frames_per_call=2)
        assert torch.equal(c[0], r[0]) and (c[1] - r[1]).abs().max().item() > 1e-3
        assert (c[1, :, 1] - r[1, :, 0]).abs().max().item() <= 1e-3                               # source 1 measured from ITS frame 1: the self-reconstruction there
