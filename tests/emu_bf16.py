"""Test helper: the C-ABI emulator (oracle/capi_emulator.py) plus the two bf16 entry points of ABI version 10, as their CPU specification --
mrfa_cast_bf16 is `tensor.to(torch.bfloat16)` (round to nearest, ties to even), mrfa_grid_sample_bf16_fwd widens its input (exact) and is then the
parent's mrfa_grid_sample_fwd.  Also the helpers the bf16-cache tests share: reading a cache back, and running the oracle on a given pyramid."""
import contextlib
import ctypes as C

import torch

from mrfa_amd import hip
from oracle.capi_emulator import Emulator, mat


def bf16_mat(ptr: int, rows: int, ld: int, cols: int) -> torch.Tensor:
    """[rows, cols] strided bf16 view (row stride ld, in bf16 elements) of host memory at ptr"""
    n = (rows - 1) * ld + cols
    flat = torch.frombuffer((C.c_int16 * n).from_address(ptr), dtype=torch.int16).view(torch.bfloat16)
    return torch.as_strided(flat, (rows, cols), (ld, 1))


class EmulatorBf16(Emulator):
    def mrfa_version(self):
        return 10             # MRFA_ABI_VERSION of include/mrfa_hip.h: the version that added the two entries below

    def mrfa_cast_bf16(self, stream, x, ldx, rows, Cc, y, ldy):
        if Cc % 8 or ldx % 8 or ldy % 8 or x % 16 or y % 16:
            self._err = b"cast_bf16: needs C % 8 == 0, ldx % 8 == 0, ldy % 8 == 0 and 16-byte aligned pointers"
            return 1
        if rows:
            bf16_mat(y, rows, ldy, Cc).copy_(mat(x, rows, ldx, Cc).to(torch.bfloat16))
        return 0

    def mrfa_grid_sample_bf16_fwd(self, stream, inp, ldi, in_bstride, in_rep, Hi, Wi, Cc, grid, ldg, N, Ho, Wo, out, ldo, mode):
        if Cc % 8 or ldi % 8 or in_bstride % 8 or ldo % 4 or inp % 16 or out % 16:
            self._err = b"grid_sample_bf16_fwd: needs C % 8 == 0, ldi % 8 == 0, in_bstride % 8 == 0, ldo % 4 == 0 and 16-byte aligned in / out"
            return 1
        n_in = (N + in_rep - 1) // in_rep
        assert in_bstride == Hi * Wi * ldi
        wide = torch.zeros((n_in * Hi * Wi, ldi), dtype=torch.float32)            # the widened copy, same geometry (counted in fp32 elements)
        wide[:, :Cc] = bf16_mat(inp, n_in * Hi * Wi, ldi, Cc).float()
        return self.mrfa_grid_sample_fwd(stream, wide.data_ptr(), ldi, in_bstride, in_rep, Hi, Wi, Cc, grid, ldg, N, Ho, Wo, out, ldo, mode)


@contextlib.contextmanager
def emulated_hip_bf16():
    old_lib, old_stream = hip._lib, hip.stream_ptr
    hip._lib = EmulatorBf16()
    hip.stream_ptr = lambda: 0
    try:
        yield
    finally:
        hip._lib, hip.stream_ptr = old_lib, old_stream


def cache_pyramid_nchw(cache) -> list:
    """the cached feature pyramid as the oracle's generator_encode returns it: fp32 NCHW tensors on the CPU, coarse first (bf16 levels widened: exact)"""
    return [f.st.data.view(f.N, f.H, f.W, f.ld)[..., f.coff:f.coff + f.C].float().permute(0, 3, 1, 2).contiguous().cpu() for f in cache["feature"]]


def cache_pyramid_bytes(cache) -> int:
    return sum(f.st.data.numel() * f.st.data.element_size() for f in cache["feature"])


@contextlib.contextmanager
def oracle_pyramid(feats):
    """oracle.mrfa_oracle.generator_encode returns `feats` while the block runs: the oracle's raft_flow then starts from the SAME (rounded) pyramid as the
    device program, and everything downstream is the same program on both sides"""
    from oracle import mrfa_oracle as O
    real = O.generator_encode
    O.generator_encode = lambda x, P, pfx, train: [f.clone() for f in feats]
    try:
        yield
    finally:
        O.generator_encode = real
