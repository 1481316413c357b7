"""The ABI emulator (oracle/capi_emulator.py) and the ctypes binding (mrfa_amd/hip.py) describe ONE ABI: the same entry points, the same argument
counts, the same version as include/mrfa_hip.h.  A pull request that adds or changes an entry fails here until the emulator follows."""
import inspect
import os
import re

from mrfa_amd import hip
from oracle.capi_emulator import Emulator
from tests.emu import emulated_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulator_has_every_entry_of_the_binding_with_its_argument_count():
    assert len(hip._SIGNATURES) >= 89                                                    # (the table as it stood when this test was written)
    for name, (argtypes, _) in hip._SIGNATURES.items():
        fn = getattr(Emulator, name, None)
        assert callable(fn), f"{name} is in hip._SIGNATURES but oracle/capi_emulator.py has no such entry"
        params = list(inspect.signature(fn).parameters.values())[1:]                     # without self
        assert all(p.kind is p.POSITIONAL_OR_KEYWORD for p in params), name
        required = sum(p.default is p.empty for p in params)
        assert required <= len(argtypes) <= len(params), f"{name}: the binding passes {len(argtypes)} arguments, the emulator takes {required}..{len(params)}"


def test_emulator_has_no_entry_the_binding_lacks():
    extra = {n for n in dir(Emulator) if n.startswith("mrfa_")} - set(hip._SIGNATURES)
    assert not extra, extra


def test_emulator_binding_and_header_state_one_version():
    header = open(os.path.join(ROOT, "include", "mrfa_hip.h")).read()
    assert Emulator().mrfa_version() == hip.ABI_VERSION == int(re.search(r"#define MRFA_ABI_VERSION (\d+)", header).group(1))


def test_without_hides_an_entry_and_the_block_restores_the_library():
    lib_before, stream_before = hip._lib, hip.stream_ptr
    with emulated_hip(without=("mrfa_kp_relative_fwd",)) as lib:
        assert hip._lib is lib and hip.lib() is lib
        assert getattr(lib, "mrfa_kp_relative_fwd", None) is None
        assert not hip.has("mrfa_kp_relative_fwd") and hip.has("mrfa_corr_direct_rep_fwd")
        assert lib.mrfa_version() == hip.ABI_VERSION
    assert hip._lib is lib_before and hip.stream_ptr is stream_before
    with emulated_hip(counting=True) as lib:
        assert hip.has("mrfa_kp_relative_fwd") and lib.mrfa_version() == hip.ABI_VERSION
        assert [n for n, _ in lib.calls] == ["mrfa_version"]
    assert hip._lib is lib_before and hip.stream_ptr is stream_before
