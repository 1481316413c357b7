"""ctypes binding of the equivariance entries of libmrfa_hip.so (C ABI: include/mrfa_equiv_hip.h): a second entry group of the model library with its own
version number, bound apart from mrfa_amd/hip.py, whose table states the first group.  As there, the library is the product: no CPU or eager fallback, a
library of another version or one that lacks an entry is refused where it is loaded.  Launches go on torch's current HIP stream (hip.stream_ptr)."""
from __future__ import annotations

import ctypes as C
import os

from . import hip

ABI_VERSION = 1            # MRFA_EQUIV_ABI_VERSION of include/mrfa_equiv_hip.h
MAX_POINTS = 64            # MRFA_EQUIV_MAX_POINTS
LDS_PARAMS = 2048          # MRFA_EQUIV_LDS_PARAMS

_V, _I, _F = C.c_void_p, C.c_int, C.c_float

_SIGNATURES = {
    "mrfa_equiv_version": ([], C.c_int),
    "mrfa_last_error": ([], C.c_char_p),
    "mrfa_equiv_warp_frame": ([_V, _V, _I, _I, _I, _I, _V, _V, _V, _I, _V], C.c_int),
    "mrfa_equiv_loss_fwd": ([_V, _I, _I, _V, _V, _V, _V, _V, _V, _V, _I, _F, _F, _V, _V], C.c_int),
    "mrfa_equiv_loss_bwd": ([_V, _I, _I, _V, _V, _V, _V, _V, _V, _V, _I, _F, _F, _V, _V, _V, _V, _V, _V], C.c_int),
}

EXPORTED_SYMBOLS = tuple(n for n in _SIGNATURES if n != "mrfa_last_error")      # (the message is hip.py's entry, read here too)

_lib = None


def lib():
    """Loads libmrfa_hip.so once for this entry group; raises loudly if it is absent, of another equivariance version, or lacks an entry."""
    global _lib
    if _lib is None:
        path = hip.LIB_PATH
        if not os.path.exists(path):
            raise hip.HipLibraryMissing(
                f"{path} not found: build it with `python -m mrfa_amd.build` (hipcc --offload-arch=gfx950). mrfa_amd has no CPU fallback.")
        L = C.CDLL(path)
        L.mrfa_equiv_version.argtypes, L.mrfa_equiv_version.restype = _SIGNATURES["mrfa_equiv_version"]     # AttributeError: a library without the group
        if L.mrfa_equiv_version() != ABI_VERSION:
            raise RuntimeError(f"{path} speaks equivariance ABI version {L.mrfa_equiv_version()}, this binding was written against {ABI_VERSION} "
                               "(include/mrfa_equiv_hip.h MRFA_EQUIV_ABI_VERSION): rebuild the library (`python -m mrfa_amd.build --force`)")
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the library and the header drift apart
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = L
    return _lib


def last_error() -> str:
    return lib().mrfa_last_error().decode()


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {last_error()}")


def stream_ptr() -> int:
    return hip.stream_ptr()
