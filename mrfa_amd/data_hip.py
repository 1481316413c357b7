"""ctypes binding of libmrfa_data_hip.so (C ABI: include/mrfa_data_hip.h): the input pipeline's device side, a library of its own beside libmrfa_hip.so
with its own version number.  As in mrfa_amd/hip.py the library is the product: there is no CPU or eager fallback, a library of another version or one that
lacks an entry is refused where it is loaded.  Launches go on torch's current HIP stream (hip.stream_ptr)."""
from __future__ import annotations

import ctypes as C
import os

from . import hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRFA_DATA_HIP_LIB") or os.path.join(_HERE, "_lib", "libmrfa_data_hip.so")

ABI_VERSION = 1            # MRFA_DATA_ABI_VERSION of include/mrfa_data_hip.h: PairAug mirrors THAT header
AUG_MAX_PAIRS = 32         # MRFA_AUG_MAX_PAIRS
AUG_NONE, AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE = 0, 1, 2, 3, 4      # MRFA_AUG_*


class PairAug(C.Structure):
    """mrfa_pair_aug: one pair's descriptor"""
    _fields_ = [("factor", C.c_float * 3), ("op", C.c_ubyte * 4), ("hue_shift", C.c_ubyte), ("time_flip", C.c_ubyte), ("hflip", C.c_ubyte),
                ("reserved", C.c_ubyte)]


_V, _I, _L = C.c_void_p, C.c_int, C.c_longlong

_SIGNATURES = {
    "mrfa_data_version": ([], C.c_int),
    "mrfa_data_last_error": ([], C.c_char_p),
    "mrfa_pair_augment_workspace": ([_I, _I, _I], C.c_longlong),
    "mrfa_pair_augment": ([_V, _V, _I, _I, _I, _I, C.POINTER(PairAug), _V, _L, _V, _V], C.c_int),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def lib():
    """Loads libmrfa_data_hip.so once; raises loudly if it is absent, of another version, or lacks an entry."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise hip.HipLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -m mrfa_amd.build` (hipcc --offload-arch=gfx950). mrfa_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.mrfa_data_version.argtypes, L.mrfa_data_version.restype = _SIGNATURES["mrfa_data_version"]
        if L.mrfa_data_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} speaks data ABI version {L.mrfa_data_version()}, this binding was written against {ABI_VERSION} "
                               "(include/mrfa_data_hip.h MRFA_DATA_ABI_VERSION): rebuild the library (`python -m mrfa_amd.build --force`)")
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the library and the header drift apart
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {lib().mrfa_data_last_error().decode()}")


def stream_ptr() -> int:
    return hip.stream_ptr()
