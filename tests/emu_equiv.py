"""Test helper: the numpy specification of the equivariance entries (tests/ref_equiv.py) installed as the loaded library of mrfa_amd.equiv_hip, the way
tests/emu_data.py installs the data library's.  transform_frame and equivariance_terms then run their host logic on CPU tensors."""
import contextlib

from mrfa_amd import equiv_hip, hip
from tests.ref_equiv import Library


@contextlib.contextmanager
def emulated_equiv():
    old_lib, old_stream = equiv_hip._lib, hip.stream_ptr
    equiv_hip._lib = Library()
    hip.stream_ptr = lambda: 0
    try:
        yield equiv_hip._lib
    finally:
        equiv_hip._lib, hip.stream_ptr = old_lib, old_stream
