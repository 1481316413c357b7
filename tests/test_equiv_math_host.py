"""mrfa_amd/csrc/equiv_math.h -- the one text of U, U', U'' and of the six sums over the control points, which the device kernels compile -- built by g++
ALONE into a plain host program (tests/equiv_math_host.cpp, its own main) and held against tests/ref_equiv.py within the derived bound.  No GPU.

The same program may be built with -fsanitize=address,undefined and run directly: MRFA_EQUIV_HOST_SANITIZE=1 adds the flags."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import ref_equiv as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("s", "gx", "gy", "hxx", "hxy", "hyy")
DISTANCES = np.array([0.0, 1e-7, 1e-6, 3e-5, 1e-3, 0.01, 0.25, 0.5, 1.0, 1.7, 2.0, 3.9], dtype=np.float32)


def _hex(v):
    return float(v).hex()


def _case(P, n, seed):
    rng = np.random.default_rng(seed)
    side = int(round(P ** 0.5))
    if side * side == P and side > 1:                               # the reference's square grid of control points over [-1, 1]^2
        ax = (2.0 * (np.arange(side, dtype=np.float32) / np.float32(side - 1)) - 1.0).astype(np.float32)
        q = np.stack(np.meshgrid(ax, ax), -1).reshape(P, 2)
    else:
        q = rng.uniform(-1, 1, (P, 2)).astype(np.float32)
    c = (rng.standard_normal(P) * 0.005).astype(np.float32)
    pts = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    if P:
        pts[0] = q[P // 2]                                          # on a control point
        pts[1, 0] = q[0, 0]                                         # on a control column
        pts[2, 1] = q[-1, 1]                                        # on a control row
    return q, c, pts


CASES = {(P, seed): _case(P, 40, seed) for P, seed in ((0, 1), (1, 2), (25, 3), (64, 4), (7, 5))}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/equiv_math_host.cpp"
    exe = str(tmp_path_factory.mktemp("equiv_math") / "equiv_math_host")
    flags = ["-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "mrfa_amd", "csrc")]
    if os.environ.get("MRFA_EQUIV_HOST_SANITIZE"):
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    subprocess.run([gxx] + flags + [os.path.join(ROOT, "tests", "equiv_math_host.cpp"), "-o", exe], check=True)

    def run(q, c, pts, ds):
        lines = [str(len(c))] + [f"{_hex(a[0])} {_hex(a[1])} {_hex(b)}" for a, b in zip(q, c)]
        lines += [str(len(pts))] + [f"{_hex(p[0])} {_hex(p[1])}" for p in pts]
        lines += [str(len(ds))] + [_hex(d) for d in ds]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
        rows = [[float.fromhex(t) for t in ln.split()] for ln in out if ln.strip()]
        return np.array(rows[:len(pts)], dtype=np.float64).reshape(len(pts), 6), np.array(rows[len(pts):], dtype=np.float64).reshape(len(ds), 3)
    return run


@pytest.mark.parametrize("key", list(CASES), ids=lambda k: f"P{k[0]}")
def test_six_sums_within_the_bound(program, key):
    q, c, pts = CASES[key]
    got, _ = program(q, c, pts, [])
    ref = R.tps_sums(pts[:, 0], pts[:, 1], q, c[None, :], R.EPS32)
    ratios = []
    for j, k in enumerate(KEYS):
        err, bound = np.abs(got[:, j] - ref[k].v), ref[k].bound
        ratios.append(float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (k, err.max(), bound[np.argmax(err)])
        if key[0] == 0:
            assert (got[:, j] == 0).all()
    print(f"[equiv] host sums P={key[0]}: max err/bound " + "  ".join(f"{k} {r:.3f}" for k, r in zip(KEYS, ratios)))
    if key[0]:
        assert any(np.abs(ref[k].v).max() > 0 for k in KEYS)


def test_u_and_its_derivatives_within_the_bound(program):
    _, got = program(np.zeros((0, 2), np.float32), np.zeros(0, np.float32), np.zeros((0, 2), np.float32), DISTANCES)
    d = R.VM(DISTANCES.astype(np.float64))                         # an input: exact
    for j, f in enumerate((R.u_of, R.du_of, R.ddu_of)):
        ref = f(d, R.EPS32)
        assert (np.abs(got[:, j] - ref.v) <= ref.bound).all(), (j, np.abs(got[:, j] - ref.v), ref.bound)


def test_derivatives_are_the_central_differences_of_the_fp64_functions():
    """U' against (U(d + h) - U(d - h)) / 2h and U'' against the same of U', in fp64: the truncation error of a central difference is h^2 / 6 times the third
    derivative of the differenced function: about 2 / d for U and 2 / d^2 for U' (eps aside), bounded generously below; h = 1e-5 d."""
    d = np.array([1e-3, 0.01, 0.1, 0.25, 0.5, 1.0, 2.0, 3.9])
    h = 1e-5 * d
    for f, df, third in ((R.u_of, R.du_of, lambda x: 2 / x + 4 / x ** 2), (R.du_of, R.ddu_of, lambda x: 4 / x ** 2 + 12 / x ** 3)):
        num = (f(d + h).v - f(d - h).v) / (2 * h)
        tol = h * h / 6 * third(d - h) + 1e-16 * (np.abs(f(d + h).v) + 1) / h          # truncation + fp64 cancellation
        assert (np.abs(num - df(d).v) <= tol).all(), (num - df(d).v, tol)
