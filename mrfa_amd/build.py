"""Builds mrfa_amd/_lib/libmrfa_hip.so (all HIP kernels + the C ABIs of include/mrfa_hip.h and include/mrfa_equiv_hip.h) and mrfa_amd/_lib/libmrfa_data_hip.so (the input pipeline's
kernels, csrc_data/, + the C ABIs of include/mrfa_data_hip.h and include/mrfa_resize_hip.h) for gfx950 with hipcc.

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container; the resulting .so travels to the
GPU box with the repo snapshot (it is git-ignored, not gpurun-ignored)."""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "_lib")
LIB = os.path.join(LIBDIR, "libmrfa_hip.so")
SOURCES = ["error.cpp", "conv_plan.hip", "conv_mfma.hip", "conv_split.hip", "conv_halo.hip", "conv_small.hip", "conv_lean.hip", "wgrad_mfma.hip", "wgrad_split.hip", "wgrad_halo.hip", "wgrad_small.hip", "wgrad_lean.hip", "conv_fewout.hip", "conv_fewout3.hip", "layout.hip", "pack_multi.hip", "norm.hip", "sample.hip", "elementwise.hip", "optim.hip", "tokenpose.hip", "attention_mfma.hip", "losses.hip", "prior.hip", "pose.hip", "metrics.hip", "frames.hip", "equivariance.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
         "-Wno-unused-result"]
# the data library: every kernel of csrc_data/ plus its own error / version file.  Its arithmetic is specified operation by operation (augment_math.h), so no
# contraction into fused multiply-adds and IEEE division, on the host and the device side alike.
CSRC_DATA = os.path.join(HERE, "csrc_data")
DATA_LIB = os.path.join(LIBDIR, "libmrfa_data_hip.so")
DATA_FLAGS = FLAGS + ["-I" + CSRC_DATA, "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def data_sources() -> list:
    return ["error.cpp"] + sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC_DATA, "*.hip")))


def build(force: bool = False, verbose: bool = True) -> str:
    """builds both libraries; returns the model library's path (the data library is DATA_LIB)"""
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    headers = [os.path.join(ROOT, "include", h) for h in ("mrfa_hip.h", "mrfa_equiv_hip.h")] + sorted(glob.glob(os.path.join(CSRC, "*.h")))
    data_headers = headers + [os.path.join(ROOT, "include", h) for h in ("mrfa_data_hip.h", "mrfa_resize_hip.h")] \
        + sorted(glob.glob(os.path.join(CSRC_DATA, "*.h")))
    units = [(CSRC, src, "", FLAGS, headers) for src in SOURCES] + [(CSRC_DATA, src, "data_", DATA_FLAGS, data_headers) for src in data_sources()]
    objs = {LIB: [], DATA_LIB: []}
    procs = []
    for srcdir, src, prefix, flags, deps in units:
        sp = os.path.join(srcdir, src)
        if not os.path.exists(sp):
            raise FileNotFoundError(sp)
        obj = os.path.join(LIBDIR, prefix + os.path.splitext(src)[0] + ".o")
        objs[DATA_LIB if prefix else LIB].append(obj)
        if force or _stale(obj, [sp] + deps):
            cmd = [hipcc] + flags + (["-x", "hip"] if src.endswith(".cpp") else []) + ["-c", sp, "-o", obj]
            if verbose:
                print("[mrfa_amd.build]", " ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd)))
    for src, pr in procs:
        if pr.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    for out, os_ in objs.items():
        if force or _stale(out, os_):
            cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + os_
            if verbose:
                print("[mrfa_amd.build]", " ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
    print(DATA_LIB)
