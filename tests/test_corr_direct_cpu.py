"""RaftFlow.forward(corr="direct") on the CPU, through the ABI emulator (tests/emu.py; mrfa_corr_direct_fwd = matmul volumes +
mrfa_corr_lookup_fwd): parity with the reference-pinned oracle, which entry points the two modes reach, and what the argument refuses."""
import importlib.util
import os

import pytest
import torch

from mrfa_amd import engine, hip
from mrfa_amd.modules import RaftFlow
from oracle import mrfa_oracle as O
from oracle.capi_emulator import Emulator
from tests import cases
from tests.emu import emulated_hip
from tests.test_oracle_golden import raft_inputs

SIZE, B = 64, 2


def _raft(prior_only=False):
    rf = RaftFlow(**cases.raft_cfg(SIZE, prior_only))
    sd = cases.weights_for(rf.state_dict(), "rf")
    rf.load_state_dict(sd)
    return rf.eval(), sd


def _abi_trace():
    spec = importlib.util.spec_from_file_location("abi_trace", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "abi_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _traced(rf, ins, cache=False, **kw):
    """the ABI calls of one forward as tools/abi_trace.py writes them (entry point, every scalar argument and struct field, weight hashes)"""
    T = _abi_trace()
    lines = []
    with T.traced_hip(lines), torch.no_grad():
        if cache:
            kw["source_cache"] = rf.encode_source(ins[0], ins[3], ins[4])
            del lines[:]
        out = rf(*ins, **kw)
    return lines, out


def test_emulator_reports_the_abi_version_and_refuses_bad_corr_direct_arguments():
    emu = Emulator()
    assert emu.mrfa_version() == hip.ABI_VERSION
    q, k0, k1 = torch.randn(4, 8), torch.randn(16, 8), torch.randn(4, 8)
    c, out = torch.zeros(4, 2), torch.full((4, 98), 7.0)
    args = dict(q=q.data_ptr(), ldq=8, k0=k0.data_ptr(), ldk0=8, k1=k1.data_ptr(), ldk1=8, N=1, h1=2, w1=2, Hs=4, Ws=4, D=8, coords=c.data_ptr(), ldc=2,
                radius=3, scale=0.5, out=out.data_ptr(), ldo=98)
    assert emu.mrfa_corr_direct_fwd(0, **args) == 0 and not (out == 7).any()
    for bad in (dict(radius=4), dict(radius=-1), dict(D=6), dict(ldc=1), dict(ldo=97), dict(Hs=3), dict(Ws=0), dict(ldq=4), dict(q=q.data_ptr() + 4)):
        out.fill_(7.0)
        assert emu.mrfa_corr_direct_fwd(0, **{**args, **bad}) != 0 and len(emu.mrfa_last_error()) > 10, bad
        assert (out == 7).all(), bad


def test_ctx_corr_direct_is_the_lookup_on_matmul_volumes_and_refuses_a_tape():
    with emulated_hip():
        e = engine.Ctx(torch.device("cpu"), train=False, record=False)
        g = torch.Generator().manual_seed(3)
        q, k0, co = e.new(2, 3, 5, 16), e.new(2, 6, 4, 16), e.new(2, 3, 5, 2)
        q.tensor().copy_(torch.randn(2, 3, 5, 16, generator=g))
        k0.tensor().copy_(torch.randn(2, 6, 4, 16, generator=g))
        co.tensor().copy_(torch.rand(2, 3, 5, 2, generator=g) * 8 - 2)
        k1 = e.avgpool2(k0)
        got = e.corr_direct(q, k0, k1, co, 0.25, radius=2)
        assert (got.N, got.H, got.W, got.C) == (2, 3, 5, 50)
        vol0 = (torch.einsum("nic,njc->nij", q.tensor().reshape(2, 15, 16), k0.tensor().reshape(2, 24, 16)) * 0.25).reshape(30, 24).contiguous()
        vol1 = (torch.einsum("nic,njc->nij", q.tensor().reshape(2, 15, 16), k1.tensor().reshape(2, 6, 16)) * 0.25).reshape(30, 6).contiguous()
        ref = e.corr_lookup(vol0, vol1, None, 6, 4, co, radius=2)
        assert torch.allclose(got.tensor(), ref.tensor(), atol=1e-6) and got.tensor().abs().max() > 0.1
        r = engine.Ctx(torch.device("cpu"), train=False, record=True)
        with pytest.raises(RuntimeError, match="no backward"):
            r.corr_direct(q, k0, k1, co, 0.25)


@pytest.mark.parametrize("cache", [False, True])
def test_raft_flow_direct_through_emulator_vs_oracle(cache):
    """the tolerance of the emulator leg tests/test_wiring_cpu.py::test_raft_flow_through_emulator: max |diff| < 1e-4"""
    with emulated_hip():
        rf, sd = _raft()
        ins = raft_inputs(SIZE, B, "g3/raft64")
        kp_s, kp_d, dmo, img, img_full = ins
        with torch.no_grad():
            kw = {"source_cache": rf.encode_source(kp_s, img, img_full)} if cache else {}
            o, w, s = rf(kp_s, kp_d, dmo, img, img_full, corr="direct", **kw)
            oo, ow, os_ = O.raft_flow(kp_s, kp_d, dmo, img, img_full, {k: v.clone() for k, v in sd.items()}, "", size=SIZE)
    for name, got, ref in (("out", o, oo), ("warp", w, ow), ("strip", s, os_)):
        d = (got - ref).abs()
        print(f"[corr direct] emulator vs oracle, cache={cache}, {name}: max |diff| {d.max().item():.3e} mean {d.mean().item():.3e}")
        assert torch.isfinite(got).all() and d.max().item() < 1e-4, name
    assert s.shape == (B, 1, SIZE, 7 * SIZE)


def _is_volume_gemm(line, rf):
    """a batched GEMM launch (gemm_nt is the only caller that sets nbatch > 1) whose output rows are Hs*Ws or Hs*Ws/4 wide: a correlation volume"""
    S0 = rf.h * rf.w
    return line.startswith("mrfa_conv2d_nhwc ") and f" nbatch={B} " in line and (f" Cout={S0} " in line or f" Cout={S0 // 4} " in line)


@pytest.mark.parametrize("cache", [False, True])
def test_direct_builds_no_volume_where_volume_builds_eight(cache):
    """what each mode hands the library.  (That corr="volume" is the PARENT commit's call list is not something one tree can test: it is recorded,
    parent against new, in profiles/corr_direct_identity.txt.)"""
    with emulated_hip():
        rf, _ = _raft()
        ins = raft_inputs(SIZE, B, "g3/raft64")
        ins = (ins[0], ins[1], ins[2], ins[3], ins[4])
        _traced(rf, ins, cache)                                                # (the first forward also packs the weights: not part of the program)
        volume, out_v = _traced(rf, ins, cache, corr="volume")
        direct, out_x = _traced(rf, ins, cache, corr="direct")
    name = lambda l: l.split(" ", 1)[0]
    levels = rf.basic_res_index + 1
    assert len(volume) > 100
    assert sum(_is_volume_gemm(l, rf) for l in volume) == 2 * levels
    assert sum(name(l) == "mrfa_corr_lookup_fwd" for l in volume) == rf.total_iter
    assert not any(name(l) == "mrfa_corr_direct_fwd" for l in volume)
    # "direct": no volume GEMM, no lookup, one direct call per refinement level; everything else is the volume program's call list
    assert not any(_is_volume_gemm(l, rf) for l in direct)
    assert not any(name(l).startswith("mrfa_corr_lookup") for l in direct)
    assert sum(name(l) == "mrfa_corr_direct_fwd" for l in direct) == rf.total_iter == 6
    assert all(l.endswith("-> 0") for l in direct if name(l) == "mrfa_corr_direct_fwd")
    rest_v = [name(l) for l in volume if not _is_volume_gemm(l, rf) and name(l) != "mrfa_corr_lookup_fwd"]
    rest_x = [name(l) for l in direct if name(l) != "mrfa_corr_direct_fwd"]
    assert rest_v == rest_x
    for a, b in zip(out_v, out_x):
        assert (a - b).abs().max().item() < 1e-4


def test_corr_argument_is_checked():
    with emulated_hip(counting=True) as lib:
        rf, _ = _raft()
        kp_s, kp_d, dmo, img, img_full = raft_inputs(SIZE, B, "g3/raft64")
        with torch.no_grad():
            with pytest.raises(ValueError, match="volume.*direct"):
                rf(kp_s, kp_d, dmo, img, img_full, corr="bogus")
            with pytest.raises(ValueError, match="volume.*direct"):
                rf(kp_s, kp_d, dmo, img, img_full, corr=None)
        assert any(p.requires_grad for p in rf.parameters())
        with torch.enable_grad():
            with pytest.raises(ValueError, match="no backward"):
                rf(kp_s, kp_d, dmo, img, img_full, corr="direct")
        rf.train()
        with torch.no_grad():
            with pytest.raises(ValueError, match="inference"):
                rf(kp_s, kp_d, dmo, img, img_full, corr="direct")
        assert not lib.calls                                                   # refused before anything was launched
        rf.eval()
        for p in rf.parameters():
            p.requires_grad_(False)
        with torch.enable_grad():                                              # gradients enabled, nothing asks for one: no tape, legal
            o, _, _ = rf(kp_s, kp_d, dmo, img, img_full, corr="direct")
        assert torch.isfinite(o).all() and sum(n == "mrfa_corr_direct_fwd" for n, _ in lib.calls) == 6


def test_animator_corr_argument():
    from mrfa_amd.infer import Animator, make_animation, reconstruction
    from mrfa_amd.utils.prng import det_uniform
    from tests.test_bf16_cache import _dry_model
    with emulated_hip(counting=True) as lib:
        m = _dry_model()
        for bad in ("bogus", None, "Direct"):
            with pytest.raises(ValueError, match="volume.*direct"):
                Animator(m, corr=bad)
        src = det_uniform("cd/anim/src", (1, 3, 64, 64), 0, 1)
        drv = [det_uniform(f"cd/anim/drv{t}", (1, 3, 64, 64), 0, 1) for t in range(2)]
        clip = torch.stack(drv, dim=2)
        with pytest.raises(ValueError):
            make_animation(m, src, clip, corr="bogus")
        with pytest.raises(ValueError):
            reconstruction(m, clip, corr="bogus")
        a, x = Animator(m), Animator(m, corr="direct", cache_dtype=torch.bfloat16)
        x32 = Animator(m, corr="direct")
        for an in (a, x, x32):
            an.set_source(src)
        direct_model = not m.decoder.prior_only
        for d in drv:
            fa = a(d).clone()
            del lib.calls[:]
            fx = x32(d).clone()
            n_direct = sum(n == "mrfa_corr_direct_fwd" for n, _ in lib.calls)
            assert n_direct == (6 if direct_model else 0)
            assert torch.isfinite(fx).all() and (fx - fa).abs().max().item() < 1e-4
            assert torch.isfinite(x(d)).all()
        r = reconstruction(m, clip, corr="direct")
        x32.set_source(drv[0])
        assert torch.equal(r["prediction"][:, :, 1], x32(drv[1]))
        assert make_animation(m, src, clip, corr="direct").shape == clip.shape


def test_the_rounding_hazard_is_in_the_coordinates():
    """the placed hazard coordinates do what their comment says, in fp32: the sum is an integer, one above floor(c) + offset"""
    e = 2.0 ** -22
    for c, off in ((3.0 - e, 3.0), (1.0 - 2.0 ** -24, 1.0), ((6.0 - 2 * e) * 0.5, 3.0), (-2.0 ** -25, 1.0), (2.0 - 2.0 ** -23, 2.0)):
        c32 = torch.tensor(c, dtype=torch.float32)
        assert c32.item() == c and c32.floor().item() != c                                            # representable and fractional
        s = c32 + torch.tensor(off, dtype=torch.float32)
        assert s.item() == s.floor().item() == c32.floor().item() + off + 1
