"""One line per C-ABI call the engine makes, on the CPU: the ABI emulator (oracle/capi_emulator.py) behind a recording proxy.

    python tools/abi_trace.py OUT.txt            # the programs of main() below, every matrix mode, PROLOGUE_FUSION off and on

A line holds the entry point, every integer / float argument and every non-pointer struct field; a pointer is written as 0 (null) or
a<address % 16>.  The emulator computes from mrfa_conv_params.w alone, so the layouts a launch is HANDED are made visible as hashes of the
bytes the ABI says lie behind them: w / w_split / w_phase of a conv launch, and every destination of a pack call after the call.  Two
commits whose traces are equal line for line hand the library the same calls with the same weights in the same order.
"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mrfa_amd import hip  # noqa: E402
from oracle.capi_emulator import Emulator  # noqa: E402

_r = lambda c, m: (c + m - 1) // m * m


def _hash(ptr, nbytes):
    return hashlib.blake2b(C.string_at(ptr, nbytes), digest_size=8).hexdigest()


def _ptr(v):
    v = v.value if isinstance(v, C.c_void_p) else v
    return "0" if not v else f"a{int(v) % 16}"


def pack_bytes(mode, Cout, Cin, R, S):
    """bytes of a pack destination (the pack-mode table of include/mrfa_hip.h)"""
    T = R * S
    fwd, dg = T * _r(Cout, 128) * _r(Cin, 32), T * _r(Cin, 128) * _r(Cout, 32)
    m = mode & 15
    return {0: 4 * fwd, 1: 4 * _r(Cout, 128) * _r(T * Cin, 32), 2: 4 * dg, 3: 4 * _r(Cin, 128) * _r(T * Cout, 32), 8: 6 * fwd, 9: 6 * dg,
            14: 2 * fwd, 15: 2 * dg, 12: 6 * 16 * _r(Cout, 128) * _r(Cin, 32), 13: 6 * 16 * _r(Cin, 128) * _r(Cout, 32)}.get(m, 4 * T * Cout * Cin)


def _struct(s):
    out = []
    for name, ct in s._fields_:
        v = getattr(s, name)
        if ct is C.c_void_p:
            out.append(f"{name}={_ptr(v)}")
        elif isinstance(v, C.Array):
            out.append(f"{name}=[" + ",".join(_ptr(e) if ct._type_ is C.c_void_p else (_struct(e) if isinstance(e, C.Structure) else repr(e))
                                              for e in v) + "]")
        else:
            out.append(f"{name}={v!r}")
    return "{" + " ".join(out) + "}"


def _structs(a, n):
    """the parameter block(s) behind an argument (byref / pointer / array of n), or None"""
    obj = getattr(a, "_obj", a)
    if isinstance(obj, C.Structure):
        return [obj]
    if isinstance(obj, (C.Array, C._Pointer)) and isinstance(obj[0], C.Structure):
        return [obj[i] for i in range(n)]
    return None


def _conv_weights(p):
    """hashes of the weight layouts a conv launch is handed"""
    T, out = p.R * p.S, []
    if p.w and p.w in (p.w_split, p.w_phase):
        out.append("w=placeholder")
    elif p.w:
        out.append("w=" + _hash(p.w, 4 * ((T - 1) * p.w_tap + (p.w_rows - 1) * p.w_ld + (p.kflat or p.Cin))))
    if p.w_split:
        out.append("w_split=" + _hash(p.w_split, 2 * (3 * p.w_piece if p.w_piece else T * p.w_rows * p.w_ld)))
    if p.w_phase:
        out.append("w_phase=" + _hash(p.w_phase, 2 * 3 * p.w_phase_piece))
    return out


class Tracer:
    def __init__(self, lines):
        self.emu, self.lines = Emulator(), lines

    def __getattr__(self, name):
        fn = getattr(self.emu, name)
        if not name.startswith("mrfa_") or name == "mrfa_last_error":
            return fn
        argtypes = hip._SIGNATURES[name][0]

        def call(*args):
            parts, after = [name], []
            n = args[-1] if "_multi" in name else 1
            for a, ct in zip(args, argtypes):
                structs = _structs(a, n)
                if structs is not None:
                    for s in structs:
                        parts.append(_struct(s))
                        if name == "mrfa_conv2d_nhwc":
                            parts += _conv_weights(s)
                        if isinstance(s, hip.PackDesc):
                            after += [(s.dst[k], pack_bytes(s.mode[k], s.Cout, s.Cin, s.R, s.S)) for k in range(s.ndst)]
                elif isinstance(a, C.Array):
                    parts.append("host")                     # (a host table the call fills: mrfa_build_ktab)
                elif ct is C.c_void_p:
                    parts.append(_ptr(a))
                else:
                    parts.append(repr(a))
            if name == "mrfa_pack_conv_weight":
                after.append((args[2], pack_bytes(args[7], *args[3:7])))
            rc = fn(*args)
            parts += [f"dst={_hash(p, nb)}" for p, nb in after] + [f"-> {rc!r}"]
            self.lines.append(" ".join(parts))
            return rc
        return call


class traced_hip:
    """like tests/emu.py's emulated_hip(), with the recording proxy in the emulator's place"""

    def __init__(self, lines):
        self.lines = lines

    def __enter__(self):
        self.old = hip._lib, hip.stream_ptr
        hip._lib, hip.stream_ptr = Tracer(self.lines), (lambda: 0)
        return hip._lib

    def __exit__(self, *exc):
        hip._lib, hip.stream_ptr = self.old
        return False


def _result(lines, tag, outs, module):
    """outputs and every gradient, bit for bit"""
    for i, t in enumerate(outs):
        lines.append(f"result {tag} out{i} {_hash(t.detach().contiguous().data_ptr(), 4 * t.numel())}")
    for n, p in module.named_parameters():
        g = p.grad
        lines.append(f"result {tag} grad {n} " + ("none" if g is None else _hash(g.contiguous().data_ptr(), 4 * g.numel())))


def programs(lines):
    import contextlib
    from mrfa_amd import engine
    from mrfa_amd.graph import FlatGradients
    from mrfa_amd.modules import DenseMotionNetwork, KPDetector, RaftFlow
    from mrfa_amd.utils.prng import det_uniform
    from tests import cases
    from tests.test_oracle_golden import raft_inputs
    from tests.test_wiring_cpu import small_hrnet

    for direct in (True, False):                     # RaftFlow at 64^2, B = 2, train: forward + backward, then a PackPlan refresh and a second step
        lines.append(f"# program raft direct={direct}")
        rf = RaftFlow(**cases.raft_cfg(64))
        rf.load_state_dict(cases.weights_for(rf.state_dict(), "rf"))
        rf.train(True)
        kp_s, kp_d, dmo, img, img_full = raft_inputs(64, 2, "g4/raft")
        driving = cases.images("g4/drv", 2, 64)
        if direct:
            FlatGradients(rf.parameters()).bind()

        def step(tag, deferred=None):
            leaves = [t.clone().requires_grad_(True) for t in (kp_s, kp_d, dmo["deformation"], dmo["occlusion"])]
            with (engine.direct_param_grads() if direct else contextlib.nullcontext()), engine.defer_wgrads(deferred):
                o, _, _ = rf(leaves[0], leaves[1], {"deformation": leaves[2], "occlusion": leaves[3]}, img, img_full)
                (o - driving).abs().mean().backward()
            if deferred is not None:                 # the weight gradients and their un-packing into .grad are issued by the join
                deferred.join(torch.device("cpu"))
                deferred.reset()
            _result(lines, tag, [o] + [t.grad for t in leaves], rf)
        step("raft/1")
        plan = engine.PackPlan(rf)
        lines.append(f"# PackPlan n={plan.n} convs={len(plan.cws)}")
        with torch.no_grad():
            for p in rf.parameters():
                p.mul_(0.75)
        plan.run()
        step("raft/2")
        if direct:                                   # the same step with its weight gradients deferred: one launch each, then one parameter array
            for batch in (False, True):
                lines.append(f"# program raft deferred batch={batch}")
                step(f"raft/deferred{int(batch)}", engine.DeferredWgrads(batch=batch))

    lines.append("# program small_hrnet stat_groups(2)")
    m = small_hrnet()
    m.train(True)
    with engine.stat_groups(2):
        y = m(det_uniform("sbh/x", (4, 3, 32, 32)))
    (y * det_uniform("sbh/w", (4, 32, 8, 8))).sum().div(4.0).backward()
    _result(lines, "hrnet", [y], m)

    _syncbn_programs(lines)

    lines.append("# program prior stage")
    x = cases.images("g11/x_train", 2, 256)
    kpm = KPDetector(**cases.KP_DETECTOR_CFG)
    kpm.load_state_dict(cases.weights_for(kpm.state_dict(), "kp"))
    kpm.train(True)
    r = kpm(x)
    (r["kp"].sum() + r["jacobian"].sum()).backward()
    _result(lines, "kp", [r["kp"], r["jacobian"]], kpm)
    dmm = DenseMotionNetwork(**cases.DENSE_MOTION_CFG)
    dmm.load_state_dict(cases.weights_for(dmm.state_dict(), "dm"))
    dmm.train(True)
    r = dmm(x, cases.keypoints("g11/kd_train", 2), cases.keypoints("g11/ks_train", 2))
    ((r["deformation"].sum() + r["occlusion"].sum() + r["mask"].square().sum()) / 64.0).backward()
    _result(lines, "dm", [r["deformation"], r["occlusion"], r["mask"]], dmm)


def _syncbn_programs(lines):
    """small_hrnet() under SyncBatchNorm in a one-rank gloo group with the collectives forced (a sum over one rank): depth-batched collectives, one per
    layer and direction, and every layer on the wide-layer path (slot sums first).  Each collective is a trace line of its own."""
    import tempfile
    import torch.distributed as dist
    from mrfa_amd import engine
    from mrfa_amd.utils.prng import det_uniform
    from tests.test_wiring_cpu import small_hrnet

    saved = engine.SYNCBN_FORCE, engine.SYNCBN_LOCKSTEP, engine.SYNCBN_DIRECT_BYTES, engine._syncbn_all_reduce
    reduce_ = engine._syncbn_all_reduce

    def traced_reduce(t, layers=1):
        lines.append(f"collective numel={t.numel()} layers={layers}")
        return reduce_(t, layers)
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "store"), rank=0, world_size=1)
        try:
            engine.SYNCBN_FORCE, engine._syncbn_all_reduce = True, traced_reduce
            for lockstep, direct_bytes, groups in ((True, saved[2], 1), (False, saved[2], 1), (True, 0, 2)):
                lines.append(f"# program small_hrnet SyncBatchNorm lockstep={lockstep} direct_bytes={direct_bytes} stat_groups({groups})")
                engine.SYNCBN_LOCKSTEP, engine.SYNCBN_DIRECT_BYTES = lockstep, direct_bytes
                m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(small_hrnet())
                m.train(True)
                with engine.stat_groups(groups):
                    y = m(det_uniform("sbh/x", (4, 3, 32, 32)))
                (y * det_uniform("sbh/w", (4, 32, 8, 8))).sum().div(4.0).backward()
                _result(lines, f"syncbn/{int(lockstep)}/{direct_bytes}/{groups}", [y], m)
        finally:
            engine.SYNCBN_FORCE, engine.SYNCBN_LOCKSTEP, engine.SYNCBN_DIRECT_BYTES, engine._syncbn_all_reduce = saved
            dist.destroy_process_group()


def main(out_path):
    from mrfa_amd import engine
    lines = []
    for fusion in (False, True):
        engine.PROLOGUE_FUSION = fusion
        for mode in (0, 1, 3):
            lines.append(f"# ==== mrfa_set_mfma_mode({mode}) PROLOGUE_FUSION={fusion}")
            with traced_hip(lines) as lib:
                lib.mrfa_set_mfma_mode(mode)
                programs(lines)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1])
