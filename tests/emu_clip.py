"""Test helper: tests/emu_corr_direct.py's emulator plus the additive entry point of ABI version 11, as its CPU specification --
mrfa_corr_direct_rep_fwd is the parent's mrfa_corr_direct_fwd on keys repeated k_rep times (repeat_interleave: query image n reads key image n // k_rep),
with the parent's argument refusals and the two of its own."""
import contextlib

from mrfa_amd import hip
from oracle.capi_emulator import mat
from tests.emu_corr_direct import Counting, EmulatorCorrDirect


class EmulatorClip(EmulatorCorrDirect):
    def mrfa_version(self):
        return 11             # MRFA_ABI_VERSION of include/mrfa_hip.h: the entry below is additive, the number did not move

    def mrfa_corr_direct_rep_fwd(self, stream, q, ldq, k0, ldk0, k1, ldk1, N, k_rep, h1, w1, Hs, Ws, D, coords, ldc, radius, scale, out, ldo):
        if k_rep < 1 or N % k_rep:
            self._err = f"corr_direct_rep_fwd: k_rep >= 1 must divide N (N {N}, k_rep {k_rep})".encode()
            return 1
        # the parent's refusals, asked of the caller's own key pointers and leading dimensions before any key is read: the parent's words in the parent's
        # order (radius; null / non-positive; Hs, Ws; leading dimensions; D % 4, ld % 4, alignment)
        if (not 0 <= radius <= 3 or not (q and k0 and k1 and coords and out and N > 0 and h1 > 0 and w1 > 0 and D > 0) or Hs < 2 or Ws < 2 or Hs % 2 or Ws % 2
                or ldc < 2 or ldo < 2 * (2 * radius + 1) ** 2 or min(ldq, ldk0, ldk1) < D or D % 4 or ldq % 4 or ldk0 % 4 or ldk1 % 4
                or q % 16 or k0 % 16 or k1 % 16):
            rc = self.mrfa_corr_direct_fwd(stream, q, ldq, k0, ldk0, k1, ldk1, N, h1, w1, Hs, Ws, D, coords, ldc, radius, scale, out, ldo)
            assert rc != 0                                    # (no key was read: the parent refuses these arguments whatever the keys hold)
            return rc
        Nk, S0, S1 = N // k_rep, Hs * Ws, (Hs // 2) * (Ws // 2)
        r0 = mat(k0, Nk * S0, ldk0, D).view(Nk, S0, D).repeat_interleave(k_rep, dim=0).contiguous()       # dense: ld = D, D % 4 == 0
        r1 = mat(k1, Nk * S1, ldk1, D).view(Nk, S1, D).repeat_interleave(k_rep, dim=0).contiguous()
        assert r0.data_ptr() % 16 == 0 and r1.data_ptr() % 16 == 0
        return self.mrfa_corr_direct_fwd(stream, q, ldq, r0.data_ptr(), D, r1.data_ptr(), D, N, h1, w1, Hs, Ws, D, coords, ldc, radius, scale, out, ldo)


@contextlib.contextmanager
def emulated_hip_clip(counting=False):
    old_lib, old_stream = hip._lib, hip.stream_ptr
    hip._lib = Counting(EmulatorClip()) if counting else EmulatorClip()
    hip.stream_ptr = lambda: 0
    try:
        yield hip._lib
    finally:
        hip._lib, hip.stream_ptr = old_lib, old_stream
