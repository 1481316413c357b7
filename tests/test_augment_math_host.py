"""mrfa_amd/csrc_data/augment_math.h -- the one text of the jitter's per-pixel rules, which the device kernels compile -- built by g++ ALONE into a plain host
program (tests/augment_math_host.cpp, its own main) and held against tests/ref_augment.py on all 2^24 inputs, per primitive and parameter.  No GPU.

The same program may be built with -fsanitize=address,undefined and run directly: MRFA_AUGMENT_HOST_SANITIZE=1 adds the flags."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import ref_augment as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = [np.float32(x) for x in ("0.0", "0.9", "1.0", "1.1", "2.0", "0.9428090", "1.0471976")]
SHIFTS = [1, 25, 231, 128]
MEANS = [10, 117]
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def program_lines(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/augment_math_host.cpp"
    exe = str(tmp_path_factory.mktemp("augment_math") / "augment_math_host")
    flags = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "mrfa_amd", "csrc_data")]
    if os.environ.get("MRFA_AUGMENT_HOST_SANITIZE"):
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    subprocess.run([gxx] + flags + [os.path.join(ROOT, "tests", "augment_math_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        name, param, s, w = line.split()
        table[(name, float(np.float32(param)) if "/" not in param else param)] = (int(s), int(w))      # (%.9g reads back as the same fp32)
    return table


@pytest.fixture(scope="module")
def colours():
    return R.all_colours()


def _sums(out: np.ndarray) -> tuple:
    """out: (4096,4096,3) bytes or (4096,4096) values -> (sum, index-weighted sum) modulo 2^64, as the program forms them"""
    o = out.astype(np.uint64)
    if o.ndim == 3:
        o = o[..., 0] << np.uint64(16) | o[..., 1] << np.uint64(8) | o[..., 2]
    o = o.reshape(-1)
    with np.errstate(over="ignore"):
        w = (o * (np.arange(o.size, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64)
    return int(o.sum(dtype=np.uint64)) & M64, int(w) & M64


def test_luma(program_lines, colours):
    assert program_lines[("luma", 0.0)] == _sums(R.luma(colours))


@pytest.mark.parametrize("f", FACTORS, ids=lambda f: f"f{float(f):.7g}")
def test_blends(program_lines, colours, f):
    key = float(f)
    assert program_lines[("brightness", key)] == _sums(R.brightness(colours, f))
    assert program_lines[("saturation", key)] == _sums(R.saturation(colours, f))
    for m in MEANS:
        assert program_lines[(f"contrast@{m}", key)] == _sums(R.blend(m, colours, f)), m


def test_hsv_both_ways(program_lines, colours):
    assert program_lines[("rgb_to_hsv", 0.0)] == _sums(R.rgb_to_hsv(colours))
    assert program_lines[("hsv_to_rgb", 0.0)] == _sums(R.hsv_to_rgb(colours))


@pytest.mark.parametrize("shift", SHIFTS)
def test_hue(program_lines, colours, shift):
    assert program_lines[("hue", float(shift))] == _sums(R.hue(colours, shift))


def test_chain_and_its_prefix(program_lines, colours):
    """every op in one order with a fixed contrast mean, and the part before contrast that the luma-sum pass evaluates"""
    f = [np.float32("1.07"), np.float32("0.93"), np.float32("1.05")]
    x = R.hue(R.saturation(colours, f[2]), 231)
    assert program_lines[("chain_prefix", 0.0)] == _sums(x)
    assert program_lines[("chain", 0.0)] == _sums(R.brightness(R.blend(117, x, f[1]), f[0]))


def test_contrast_mean_is_int_of_mean_plus_half(program_lines):
    seen = 0
    for (name, param), (m, _) in program_lines.items():
        if name == "mean":
            S, n = map(int, param.split("/"))
            assert m == int(S / n + 0.5) == (2 * S + n) // (2 * n), param
            seen += 1
    assert seen >= 20
    assert program_lines[("mean", "21/2")][0] == 11 and program_lines[("mean", "52/35")][0] == 1 and program_lines[("mean", "53/35")][0] == 2
