"""Test helper: the numpy specification of libmrfa_data_hip.so (tests/ref_augment.py) installed as the loaded library of mrfa_amd.data_hip, the way
tests/emu.py installs the emulator of the model library.  PairAugmenter's host logic then runs on CPU tensors."""
import contextlib

from mrfa_amd import data_hip, hip
from tests.ref_augment import Library


@contextlib.contextmanager
def emulated_data_hip():
    old_lib, old_stream = data_hip._lib, hip.stream_ptr
    data_hip._lib = Library()
    hip.stream_ptr = lambda: 0
    try:
        yield data_hip._lib
    finally:
        data_hip._lib, hip.stream_ptr = old_lib, old_stream
