"""Test helper: tests/emu_clip.py's emulator plus the second additive entry point of ABI version 11, as its CPU specification --
mrfa_kp_relative_fwd is mrfa_amd.infer.normalize_kp(use_relative_movement=True) on the first driving frames and sources repeated rep times
(repeat_interleave: frame n reads entry n // rep), with the movement scale handed in as one float in memory instead of being taken from the hulls,
and with the entry's own argument refusals."""
import contextlib

import torch

from mrfa_amd import hip
from mrfa_amd.infer import normalize_kp
from oracle.capi_emulator import _flat
from tests.emu_clip import EmulatorClip
from tests.emu_corr_direct import Counting


class EmulatorRelative(EmulatorClip):
    def mrfa_version(self):
        return 11             # MRFA_ABI_VERSION of include/mrfa_hip.h: the entry below is additive, the number did not move

    def mrfa_kp_relative_fwd(self, stream, kp_d, jac_d, kp_0, jac_0, kp_s, jac_s, scale, B, rep, K, kp_out, jac_out):
        jacs = [bool(p) for p in (jac_d, jac_0, jac_s, jac_out)]
        bad = None
        if not (kp_d and kp_0 and kp_s and kp_out):
            bad = "null keypoint pointer"
        elif B < 1 or K < 1 or rep < 1:
            bad = f"B, K and rep must be >= 1 (B {B}, K {K}, rep {rep})"
        elif B % rep:
            bad = f"rep must divide B (B {B}, rep {rep})"
        elif any(jacs) and not all(jacs):
            bad = f"the four Jacobian pointers come together or not at all ({sum(jacs)} of 4 given)"
        elif any(p % 8 for p in (kp_d, kp_0, kp_s, kp_out)) or (all(jacs) and any(p % 16 for p in (jac_d, jac_0, jac_s, jac_out))) or (scale and scale % 4):
            bad = "keypoints must be 8-byte aligned and Jacobians 16-byte aligned (vector loads and stores)"
        if bad:
            self._err = ("kp_relative_fwd: " + bad).encode()
            return 1
        Bs = B // rep
        rd = lambda p, n, *shape: _flat(p, n * K * (4 if len(shape) == 2 else 2)).view(n, K, *shape).clone()
        kd, k0, ks = {"kp": rd(kp_d, B, 2)}, {"kp": rd(kp_0, Bs, 2)}, {"kp": rd(kp_s, Bs, 2)}
        if all(jacs):
            kd["jacobian"], k0["jacobian"], ks["jacobian"] = rd(jac_d, B, 2, 2), rd(jac_0, Bs, 2, 2), rd(jac_s, Bs, 2, 2)
        ri = lambda kp: {k: v.repeat_interleave(rep, dim=0) for k, v in kp.items()}
        new = normalize_kp(ri(ks), kd, ri(k0), use_relative_movement=True, use_relative_jacobian=all(jacs))
        if scale:            # normalize_kp's own line with the scale it would have taken from the hulls: difference, times scale, plus source
            new["kp"] = (kd["kp"] - ri(k0)["kp"]) * _flat(scale, 1)[0] + ri(ks)["kp"]
        _flat(kp_out, B * K * 2).view(B, K, 2).copy_(new["kp"])
        if all(jacs):
            _flat(jac_out, B * K * 4).view(B, K, 2, 2).copy_(new["jacobian"])
        return 0


@contextlib.contextmanager
def emulated_hip_relative(counting=False):
    old_lib, old_stream = hip._lib, hip.stream_ptr
    hip._lib = Counting(EmulatorRelative()) if counting else EmulatorRelative()
    hip.stream_ptr = lambda: 0
    try:
        yield hip._lib
    finally:
        hip._lib, hip.stream_ptr = old_lib, old_stream
