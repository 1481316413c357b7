"""The packed weight layouts of engine.ConvW (engine.LAYOUTS) and their batched refresh (engine.PackPlan), through the ABI emulator.

Sizes, element types and pack modes are restated here from the comment above mrfa_pack_conv_weight in include/mrfa_hip.h, not taken from the
table under test; contents are compared with a fresh pack call of that mode into a zeroed buffer."""
import ctypes as C

import pytest
import torch

from mrfa_amd import engine, hip
from tests.emu import emulated_hip

CPU = torch.device("cpu")
_r = lambda c, m: (c + m - 1) // m * m


def spec(name, cw, padded):
    """(pack mode, dtype, elements) of layout `name` of convolution cw by the header's pack-mode table"""
    T, Co, Ci = cw.R * cw.S, cw.Cout, cw.Cin
    fwd, dg = T * _r(Co, 128) * _r(Ci, 32), T * _r(Ci, 128) * _r(Co, 32)
    if name == "fwd":
        return (0, torch.float32, fwd) if (padded or Ci % 32 == 0) else (1, torch.float32, _r(Co, 128) * _r(T * Ci, 32))
    if name == "dgrad":
        return (2, torch.float32, dg) if (padded or Co % 32 == 0) else (3, torch.float32, _r(Ci, 128) * _r(T * Co, 32))
    return {"fwd_split": (8, torch.int16, 3 * fwd), "dgrad_split": (9, torch.int16, 3 * dg),
            "fwd_rne": (14, torch.int16, fwd), "dgrad_rne": (15, torch.int16, dg),
            "fwd_phase": (12, torch.int16, 3 * 16 * _r(Co, 128) * _r(Ci, 32)), "dgrad_phase": (13, torch.int16, 3 * 16 * _r(Ci, 128) * _r(Co, 32)),
            "fewout": (5, torch.float32, Co * T * Ci), "fewin": (7, torch.float32, Ci * T * Co)}[name]


def fresh_pack(cw, mode, dtype, n):
    ref = torch.zeros(n, dtype=dtype)
    w = cw.conv.weight.detach().contiguous()
    if mode < 8:
        assert hip.lib().mrfa_pack_conv_weight(0, w.data_ptr(), ref.data_ptr(), cw.Cout, cw.Cin, cw.R, cw.S, mode) == 0
    else:
        d = hip.PackDesc()
        d.src, d.Cout, d.Cin, d.R, d.S, d.ndst = w.data_ptr(), cw.Cout, cw.Cin, cw.R, cw.S, 1
        d.dst[0], d.mode[0] = ref.data_ptr(), mode
        assert hip.lib().mrfa_pack_conv_weights_multi(0, C.pointer(d), 1) == 0
    return ref


class CountPacks:
    """the library with every pack destination recorded as (dst pointer, mode)"""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if name == "mrfa_pack_conv_weight":
            def one(stream, src, dst, Cout, Cin, R, S, mode):
                self.calls.append((dst, mode))
                return fn(stream, src, dst, Cout, Cin, R, S, mode)
            return one
        if name == "mrfa_pack_conv_weights_multi":
            def multi(stream, descs, n):
                self.calls += [(descs[i].dst[k], descs[i].mode[k]) for i in range(n) for k in range(descs[i].ndst)]
                return fn(stream, descs, n)
            return multi
        return fn


@pytest.fixture
def counted():
    with emulated_hip():
        hip._lib = CountPacks(hip._lib)
        yield hip._lib


def modules():
    torch.manual_seed(7)
    m = torch.nn.ModuleDict({
        "c33": torch.nn.Conv2d(32, 32, 3, padding=1),
        "flat": torch.nn.Conv2d(3, 32, 7, padding=3),          # flat-K forward
        "fewout": torch.nn.Conv2d(32, 2, 3, padding=1),
        "fewin": torch.nn.Conv2d(2, 32, 7, padding=3),
        "zpad": torch.nn.Conv2d(40, 32, 3, padding=1),         # fed a zpad view: the padded forward case
        "lin": torch.nn.Linear(32, 64),
        "up": torch.nn.Conv2d(32, 32, 3, padding=1),           # UpBlock2d-style ups=True: the phase layouts (split mode)
    })
    return m


def step(conv, *, ups=False, zpad=False):
    """forward + backward of one convolution on a 1 x 8 x 8 input"""
    cw = engine.convw(conv)
    e = engine.Ctx(CPU, train=True, record=True)
    xv = e.from_nchw(torch.randn(1, cw.Cin, 8, 8), out=e.new(1, 8, 8, cw.Cin, pad32=zpad))
    out = e.conv(xv, conv, ups=ups)
    e.seed_grad_nchw(out, torch.ones(1, cw.Cout, out.H, out.W))
    e.run_backward()
    for c in e.touched_convs:
        c.take_grads()
    return cw


def run_all(m, mfma_mode):
    hip.lib().mrfa_set_mfma_mode(mfma_mode)
    return [step(conv, ups=(k == "up"), zpad=(k == "zpad")) for k, conv in m.items()]


def check_contents(cw, names=None):
    for name, (buf, ver, padded) in cw.packs.items():
        if names is not None and name not in names:
            continue
        mode, dtype, n = spec(name, cw, padded)
        assert (buf.dtype, buf.numel()) == (dtype, n), (name, cw.Cin, cw.Cout, buf.dtype, buf.numel(), n)
        assert ver == cw._key()
        assert torch.equal(buf, fresh_pack(cw, mode, dtype, n)), (name, cw.Cin, cw.Cout)


def test_every_layout_has_the_size_type_and_contents_of_its_pack_mode(counted):
    m = modules()
    cws = run_all(m, 1) + run_all(m, 3)                  # bf16x6: the split and phase planes; plain bf16: the rne planes
    assert {n for cw in cws for n in cw.packs} == set(engine.LAYOUTS)
    assert engine.convw(m["zpad"]).packs["fwd"][2] and not engine.convw(m["flat"]).packs["fwd"][2]
    assert list(engine.LAYOUTS) == ["fwd", "dgrad", "fwd_split", "dgrad_split", "fwd_rne", "dgrad_rne", "fwd_phase", "dgrad_phase", "fewout", "fewin"]
    for cw in cws:
        check_contents(cw)


@pytest.mark.parametrize("key,names", [("c33", ["fwd", "dgrad", "fwd_split", "dgrad_split", "fwd_rne", "dgrad_rne", "fwd_phase", "dgrad_phase"]),
                                       ("flat", ["fwd"]), ("fewout", ["fewout", "dgrad"]), ("fewin", ["fewin"])])
def test_a_layout_is_packed_once_per_weight_version(counted, monkeypatch, key, names):
    conv = modules()[key]
    cw = engine.convw(conv)
    for name in names:
        buf = cw.layout(name)
        mode = spec(name, cw, False)[0]
        assert counted.calls == [(buf.data_ptr(), mode)], name
        assert cw.layout(name) is buf and len(counted.calls) == 1, name         # unchanged weights: no pack call
        with torch.no_grad():
            conv.weight.add_(1)
        assert cw.layout(name) is buf and counted.calls[1:] == [(buf.data_ptr(), mode)], name     # one re-pack, into the same buffer
        monkeypatch.setattr(engine, "CAPTURE_KEY", engine.CAPTURE_KEY + 1)
        assert cw.layout(name) is buf and counted.calls[2:] == [(buf.data_ptr(), mode)], name
        check_contents(cw, [name])
        counted.calls.clear()


def test_pack_plan_covers_exactly_the_layouts_that_exist(counted):
    m = modules()
    cws = run_all(m, 1)
    plan = engine.PackPlan(m)
    assert plan.cws == cws
    have = {(buf.data_ptr(), spec(name, cw, padded)[0]) for cw in cws for name, (buf, _, padded) in cw.packs.items()}
    descs = [plan.table[i] for i in range(plan.n)]
    assert {(d.dst[k], d.mode[k]) for d in descs for k in range(d.ndst)} == have
    assert sum(d.ndst for d in descs) == len(have)
    assert plan.n == sum((len(cw.packs) + 2) // 3 for cw in cws)

    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)
    counted.calls.clear()
    plan.run()
    assert set(counted.calls) == have and len(counted.calls) == len(have)
    counted.calls.clear()
    for cw in cws:
        for name, (buf, _, padded) in list(cw.packs.items()):
            assert cw.layout(name, padded) is buf
        check_contents(cw)                                # (its fresh packs go to buffers of their own)
    assert all(dst not in {b for b, _ in have} for dst, _ in counted.calls)


def test_pack_plan_refuses_layouts_created_after_it_was_built(counted):
    m = modules()
    run_all(m, 1)
    plan = engine.PackPlan(m)
    plan.run()
    hip.lib().mrfa_set_mfma_mode(3)                       # a mode switch: the first bf16 step builds the rne planes
    step(m["c33"])
    with pytest.raises(AssertionError, match="PackPlan is stale"):
        plan.run()
    plan = engine.PackPlan(m)
    plan.run()
    cw = engine.convw(m["zpad"])
    old = cw.packs["fwd"][0]
    assert cw.layout("fwd", padded=False) is not old      # the other `padded`: the ONE fp32 forward buffer is replaced ...
    assert list(cw.packs).count("fwd") == 1 and spec("fwd", cw, False)[2] == cw.packs["fwd"][0].numel()
    with pytest.raises(AssertionError, match="PackPlan is stale"):
        plan.run()                                        # ... by one the plan does not write
