"""ctypes binding of the resize entries of libmrfa_data_hip.so (C ABI: include/mrfa_resize_hip.h): a second entry group of the data library with its own
version number, bound apart from mrfa_amd/data_hip.py, whose table states the first group.  As there, the library is the product: no CPU or eager fallback, a
library of another version or one that lacks an entry is refused where it is loaded.  Launches go on torch's current HIP stream (hip.stream_ptr)."""
from __future__ import annotations

import ctypes as C
import os

from . import data_hip, hip

ABI_VERSION = 1            # MRFA_RESIZE_ABI_VERSION of include/mrfa_resize_hip.h
MAX_TAPS = 383             # MRFA_RESIZE_MAX_TAPS
BOX, BILINEAR, HAMMING, BICUBIC, LANCZOS = 0, 1, 2, 3, 4          # MRFA_RESIZE_*
FILTERS = {"box": BOX, "bilinear": BILINEAR, "hamming": HAMMING, "bicubic": BICUBIC, "lanczos": LANCZOS}

_V, _I, _F = C.c_void_p, C.c_int, C.c_float
_P = C.POINTER(C.c_int)

_SIGNATURES = {
    "mrfa_resize_version": ([], C.c_int),
    "mrfa_data_last_error": ([], C.c_char_p),
    "mrfa_resize_ksize": ([_I, _F, _F, _I, _I], C.c_int),
    "mrfa_resize_coeffs": ([_I, _F, _F, _I, _I, _P, _P], C.c_int),
    "mrfa_frames_resize_u8": ([_V, _V, _I, _I, _I, _I, _V, _V, _I, _V, _V, _I, _I, _I, _V, _V], C.c_int),
}

EXPORTED_SYMBOLS = tuple(n for n in _SIGNATURES if n != "mrfa_data_last_error")      # (the message is data_hip's entry, read here too)

_lib = None


def lib():
    """Loads libmrfa_data_hip.so once for this entry group; raises loudly if it is absent, of another resize version, or lacks an entry."""
    global _lib
    if _lib is None:
        path = data_hip.LIB_PATH
        if not os.path.exists(path):
            raise hip.HipLibraryMissing(
                f"{path} not found: build it with `python -m mrfa_amd.build` (hipcc --offload-arch=gfx950). mrfa_amd has no CPU fallback.")
        L = C.CDLL(path)
        L.mrfa_resize_version.argtypes, L.mrfa_resize_version.restype = _SIGNATURES["mrfa_resize_version"]     # AttributeError: a library without the group
        if L.mrfa_resize_version() != ABI_VERSION:
            raise RuntimeError(f"{path} speaks resize ABI version {L.mrfa_resize_version()}, this binding was written against {ABI_VERSION} "
                               "(include/mrfa_resize_hip.h MRFA_RESIZE_ABI_VERSION): rebuild the library (`python -m mrfa_amd.build --force`)")
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the library and the header drift apart
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = L
    return _lib


def last_error() -> str:
    return lib().mrfa_data_last_error().decode()


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {last_error()}")


def stream_ptr() -> int:
    return hip.stream_ptr()
