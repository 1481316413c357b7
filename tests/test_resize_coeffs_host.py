"""mrfa_amd/csrc_data/resize_coeffs.h -- the one text of the resize coefficient rules, which the data library compiles -- built by g++ ALONE into a plain host
program (tests/resize_coeffs_host.cpp, its own main) and held against tests/ref_resize.py: every bound and every coefficient of both axes of the geometry
list, all five filters, exactly.  No GPU.

The same program may be built with -fsanitize=address,undefined and run directly: MRFA_RESIZE_HOST_SANITIZE=1 adds the flags."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import ref_resize as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def axes():
    """(in_size, in0, in1, out_size) of both axes of every geometry, and a few more: the refusal case's 751 taps, the caps' geometries"""
    seen = []
    for (hi, wi), (ho, wo), box in R.GEOMETRIES:
        left, upper, right, lower = R.full_box(hi, wi, box)
        for a in ((wi, left, right, wo), (hi, upper, lower, ho)):
            if a not in seen:
                seen.append(a)
    return seen + [(2000, 0.0, 2000.0, 16), (3840, 0.0, 3840.0, 256), (2160, 0.0, 2160.0, 256), (4096, 0.0, 4096.0, 256), (1920, 420.0, 1500.0, 256)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/resize_coeffs_host.cpp"
    exe = str(tmp_path_factory.mktemp("resize_coeffs") / "resize_coeffs_host")
    flags = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "mrfa_amd", "csrc_data")]
    if os.environ.get("MRFA_RESIZE_HOST_SANITIZE"):
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    subprocess.run([gxx] + flags + [os.path.join(ROOT, "tests", "resize_coeffs_host.cpp"), "-o", exe], check=True)

    def run(cases):
        args = []
        for n, a, b, m, f in cases:
            args += [str(n), "%.9g" % np.float32(a), "%.9g" % np.float32(b), str(m), str(f)]
        return subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    return run


@pytest.mark.parametrize("name", list(R.FILTERS))
def test_tables_equal_the_numpy_specification(program, name):
    f = R.FILTERS[name]
    cases = [(n, a, b, m, f) for n, a, b, m in axes()]
    lines = program(cases)
    assert len(lines) == len(cases)
    for (n, a, b, m, _), line in zip(cases, lines):
        got = np.array(line.split(), dtype=np.int64)
        bounds, kk = R.coeffs(n, a, b, m, f)
        k = kk.shape[1]
        assert got[0] == k == R.ksize_of(a, b, m, f), (n, a, b, m)
        assert np.array_equal(got[1:1 + 2 * m].reshape(m, 2), bounds), (n, a, b, m)
        assert np.array_equal(got[1 + 2 * m:].reshape(m, k), kk), (n, a, b, m)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 0).all() and (bounds[:, 1] <= k).all() and (bounds.sum(axis=1) <= n).all()


def test_the_taps_the_cap_is_chosen_for(program):
    lan = R.LANCZOS
    lines = program([(3840, 0, 3840, 256, lan), (2160, 0, 2160, 256, lan), (4096, 0, 4096, 256, lan), (2000, 0, 2000, 16, lan)])
    assert [int(line.split()[0]) for line in lines] == [91, 53, 97, 751]
    assert 361 <= R.MAX_TAPS < 751                                       # (361: 8x300 -> 17x5 of the geometry list under Lanczos)


def test_refused_boxes_and_filters(program):
    bad = [(0, 0, 1, 4, 1), (4, 0, 4, 0, 1), (4, 0, 4, 4, 5), (4, 0, 4, 4, -1), (4, -0.5, 4, 4, 1), (4, 0, 4.5, 4, 1), (4, 2, 2, 4, 1), (4, 3, 1, 4, 1),
           (4, float("nan"), 4, 4, 1), (4, 0, float("inf"), 4, 1)]
    assert program(bad) == ["refused"] * len(bad)
    for n, a, b, m, f in bad:
        assert n < 1 or m < 1 or f not in R.SUPPORT or not R.box_ok(n, a, b)
