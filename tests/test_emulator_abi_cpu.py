"""The ABI emulator (oracle/capi_emulator.py) and the ctypes binding (mrfa_amd/hip.py) describe ONE ABI: the same entry points, the same argument
counts, the same version as include/mrfa_hip.h.  A pull request that adds or changes an entry fails here until the emulator follows."""
import inspect
import os
import re

import pytest

from mrfa_amd import hip
from oracle.capi_emulator import Emulator
from tests.emu import emulated_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulator_has_every_entry_of_the_binding_with_its_argument_count():
    assert len(hip._SIGNATURES) >= 94                                                    # (the table as it stood when this test was written)
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


def test_the_emulated_block_restores_the_library():
    lib_before, stream_before = hip._lib, hip.stream_ptr
    with emulated_hip() as lib:
        assert hip._lib is lib and hip.lib() is lib
        assert lib.mrfa_version() == hip.ABI_VERSION
    assert hip._lib is lib_before and hip.stream_ptr is stream_before
    with emulated_hip(counting=True) as lib:
        assert lib.mrfa_version() == hip.ABI_VERSION
        assert [n for n, _ in lib.calls] == ["mrfa_version"]
    assert hip._lib is lib_before and hip.stream_ptr is stream_before


# A library built from an older checkout is refused where it is loaded, by hip.lib(): by its version number, and -- should the number ever fail to move -- by
# the first symbol it lacks.  Both on a stand-in for ctypes.CDLL, without a built library.
FORMERLY_OPTIONAL = ("mrfa_kp_relative_fwd", "mrfa_kp_pose_dist", "mrfa_frame_metrics", "mrfa_frame_metrics_workspace", "mrfa_frames_from_u8",
                     "mrfa_frames_to_u8")


class _Entry:
    """what ctypes hands out for a symbol: callable, with argtypes / restype to assign"""

    def __init__(self, value=0):
        self.value = value

    def __call__(self, *args):
        return self.value


def _stand_in(monkeypatch, version, lacks=()):
    """hip.lib() will load a plain object with every symbol of the binding except `lacks`, whose mrfa_version() returns `version`"""
    L = type("StandIn", (), {})()
    for name in hip._SIGNATURES:
        if name not in lacks:
            setattr(L, name, _Entry(version if name == "mrfa_version" else 0))
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "LIB_PATH", os.path.abspath(__file__))                       # lib() asks that the file exists before it loads it
    monkeypatch.setattr(hip.C, "CDLL", lambda path: L)
    return L


def test_lib_refuses_a_library_of_the_previous_version_and_says_rebuild(monkeypatch):
    _stand_in(monkeypatch, hip.ABI_VERSION - 1)
    with pytest.raises(RuntimeError) as err:
        hip.lib()
    assert f"speaks ABI version {hip.ABI_VERSION - 1}," in str(err.value) and "rebuild the library" in str(err.value)
    assert hip._lib is None


@pytest.mark.parametrize("name", FORMERLY_OPTIONAL)
def test_lib_refuses_a_library_that_lacks_a_formerly_optional_entry(monkeypatch, name):
    assert name in hip.EXPORTED_SYMBOLS
    _stand_in(monkeypatch, hip.ABI_VERSION, lacks=(name,))
    with pytest.raises(AttributeError) as err:
        hip.lib()
    assert name in str(err.value)
    assert hip._lib is None
