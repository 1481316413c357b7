"""Test helper: run the product engine on CPU memory through the C-ABI emulator (oracle/capi_emulator.py), the CPU specification of every entry of
include/mrfa_hip.h.  Also a counting wrapper for the tests that ask which entry points a program reached, and the helpers the bf16-cache tests share:
reading a cache back, and running the oracle on a given pyramid."""
import contextlib

from mrfa_amd import hip
from oracle.capi_emulator import Emulator


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
def emulated_hip(counting=False):
    """installs the emulator as the loaded library and yields it; counting: behind Counting"""
    old_lib, old_stream = hip._lib, hip.stream_ptr
    hip._lib = Counting(Emulator()) if counting else Emulator()
    hip.stream_ptr = lambda: 0
    try:
        yield hip._lib
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
