"""Test helper: tests/emu_bf16.py's emulator plus the entry point of ABI version 11, as its CPU specification -- mrfa_corr_direct_fwd forms both
correlation volumes with a matmul (vol_l[n Q + i, j] = scale * sum_c q[n, i, c] k_l[n, j, c]) and is then the parent's mrfa_corr_lookup_fwd on them.
Also a counting wrapper for the tests that ask which entry points a program reached."""
import contextlib

import torch

from mrfa_amd import hip
from oracle.capi_emulator import mat
from tests.emu_bf16 import EmulatorBf16


class EmulatorCorrDirect(EmulatorBf16):
    def mrfa_version(self):
        return 11             # MRFA_ABI_VERSION of include/mrfa_hip.h: the version that added the entry below

    def mrfa_corr_direct_fwd(self, stream, q, ldq, k0, ldk0, k1, ldk1, N, h1, w1, Hs, Ws, D, coords, ldc, radius, scale, out, ldo):
        nwin = (2 * radius + 1) ** 2
        bad = None
        if not 0 <= radius <= 3:
            bad = "the window's lattice must fit one wave (0 <= radius <= 3)"
        elif not (q and k0 and k1 and coords and out and N > 0 and h1 > 0 and w1 > 0 and D > 0):
            bad = "null pointer or non-positive size"
        elif Hs < 2 or Ws < 2 or Hs % 2 or Ws % 2:
            bad = "Hs and Ws must be even and >= 2"
        elif ldc < 2 or ldo < 2 * nwin or min(ldq, ldk0, ldk1) < D:
            bad = "a leading dimension is below its channel count"
        elif D % 4 or ldq % 4 or ldk0 % 4 or ldk1 % 4 or q % 16 or k0 % 16 or k1 % 16:
            bad = "needs D % 4 == 0, ldq / ldk0 / ldk1 % 4 == 0 and 16-byte aligned q / k0 / k1"
        if bad:
            self._err = ("corr_direct_fwd: " + bad).encode()
            return 1
        Q, S0, S1 = h1 * w1, Hs * Ws, (Hs // 2) * (Ws // 2)
        qm = mat(q, N * Q, ldq, D).view(N, Q, D)
        vol0 = (torch.matmul(qm, mat(k0, N * S0, ldk0, D).view(N, S0, D).transpose(1, 2)) * scale).contiguous()
        vol1 = (torch.matmul(qm, mat(k1, N * S1, ldk1, D).view(N, S1, D).transpose(1, 2)) * scale).contiguous()
        return self.mrfa_corr_lookup_fwd(stream, vol0.data_ptr(), vol1.data_ptr(), Hs, Ws, coords, ldc, N * Q, radius, out, ldo)


class Counting:
    """an emulator behind a proxy that lists (entry point, arguments) of every mrfa_* call"""

    def __init__(self, emu):
        self.emu, self.calls = emu, []

    def __getattr__(self, name):
        fn = getattr(self.emu, name)
        if not name.startswith("mrfa_") or name == "mrfa_last_error":
            return fn

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


@contextlib.contextmanager
def emulated_hip_corr_direct(counting=False):
    old_lib, old_stream = hip._lib, hip.stream_ptr
    hip._lib = Counting(EmulatorCorrDirect()) if counting else EmulatorCorrDirect()
    hip.stream_ptr = lambda: 0
    try:
        yield hip._lib
    finally:
        hip._lib, hip.stream_ptr = old_lib, old_stream
