"""mrfa_corr_direct_fwd (csrc/sample.hip) against float64, element by element (-m gpu).

REFERENCE.  vol_l[n Q + i, j] = scale * sum_c q[n, i, c] k_l[n, j, c] in float64 from the fp32 operands (scale = the fp32 value the kernel is handed), then
tests/ref_sample.corr_lookup_ref on those volumes: the specification of include/mrfa_hip.h, with nothing of the kernel in it.

THE BOUND, per output element, counted from the kernel's fp32 roundings (u = 2^-24; the style of tests/test_sample_kernels_gpu.py):
  lattice value   the dot product is a sum of D fp32 FMA terms -- in whatever order and however many partial sums (the kernel: four chains per lane, eight
                  lanes, a tree), its error is at most gamma_D S with gamma_D = D u / (1 - D u) and S = sum_c |q_c k_c| -- followed by one rounded
                  multiplication by scale:  E = (D + 2) u / (1 - D u) * scale * S  per lattice point (gamma_D (1 + u) + u <= (D + 2) u / (1 - D u)).
                  E is formed as a volume of its own (|q| . |k|^T in float64) and the bound takes its MAXIMUM over the 4 x 4 neighbourhood of the sample
                  (ref_sample's tap_wide): the blend's weights are non-negative and sum to at most one, on whichever of the neighbouring tap sets the
                  fp32 coordinate selects.
  blend           10 u (S_out + E): the four-term blend of the lookup kernels (six roundings inside a term, four terms), on the computed lattice values.
  coordinate      (delta_x + delta_y) 2 max|tap|: ix = cx / 2^lvl + (a - r) is one fp32 addition where the reference adds in float64; delta = one ulp of the
                  result, the maximum over the 4 x 4 neighbourhood because the fp32 sum may land on the next integer (the case the header names: the value is
                  continuous there, so a kernel that blends the RIGHT lattice points stays inside, one that reads a wrong or missing point is off by O(|v|)).
No term is measured from the kernel.  Dead samples (NaN, +-inf, <= -1, >= W) must be exactly 0.

Every operand sits in a wider buffer (rows longer than the channel count, NaN in the padding and in front of the first row); the output's padding and
surroundings hold a canary that must survive.  Two runs must agree bit for bit (the kernel has no atomics)."""
import pytest
import torch

from mrfa_amd import hip
from tests import ref_sample as R
from tests.kernel_check import CANARY, DEV, F64, NAN, U, Buf, check, note, report

pytestmark = pytest.mark.gpu

WAVES = 2048 * 4                                          # mrfa_corr_direct_fwd launches at most 2048 four-wave workgroups; beyond, a wave walks a run of queries
INF = float("inf")


def special_coords(Hs, Ws):
    e = 2.0 ** -22
    return [(1.75, 0.375), (Ws - 1.5, Hs - 1.25), (0.5 * Ws + 0.3, 0.5 * Hs - 0.6),                  # interior, fractional
            (3.0, 5.0), (4.0, 2.0), (1.0, 1.0), (0.0, 0.0), (Ws - 1.0, 0.0), (0.0, Hs - 1.0), (Ws - 1.0, Hs - 1.0),       # exact integers, the corners
            (-30.0, 1.0), (4.0 * Ws + 9, 1.0), (1.0, -30.0), (1.0, 4.0 * Hs + 9), (1e9, 1e9), (-1e9, 2.0),           # the whole window outside, each side
            (-2.5, 1.25), (Ws + 1.5, 0.75), (0.5, -2.25), (1.25, Hs + 0.5), (-0.5, -0.5), (Ws - 0.5, Hs - 0.5),       # straddling each border
            (-1.0, 1.0), (float(Ws), 1.0), (1.0, -1.0), (1.0, float(Hs)), (-4.0, 0.0), (Ws + 3.0, 0.0),             # integers on / past the selection rule's edges
            (NAN, 1.0), (2.0, NAN), (INF, 3.0), (1.0, -INF), (NAN, NAN),
            # cx + (a - r) rounds UP to an integer in fp32 while cx is fractional (a - r = 3 at 3 - 2^-22; a - r = 1 at 1 - 2^-24), on level 0, on level 1
            # (cx / 2 = 3 - 2^-22), in x, in y and in both; and just below zero (-2^-25 + 1 rounds to 1)
            (3.0 - e, 2.5), (2.5, 3.0 - e), (3.0 - e, 3.0 - e), (6.0 - 2 * e, 1.5), (1.5, 6.0 - 2 * e), (6.0 - 2 * e, 6.0 - 2 * e),
            (1.0 - 2.0 ** -24, 0.5), (0.5, 1.0 - 2.0 ** -24), (1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24), (-2.0 ** -25, -2.0 ** -25), (2.0 - 2.0 ** -23, 2.0 - 2.0 ** -23)]


def make_coords(Q, Hs, Ws, seed, start=0):
    """Q coordinate pairs: the special ones (from `start`, cycling) at the odd positions, uniform over the map and four pixels around it elsewhere"""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(Q, 2, generator=g) * torch.tensor([Ws + 8.0, Hs + 8.0]) - 4
    sp = special_coords(Hs, Ws)
    for j, i in enumerate(range(1 if Q > 1 else 0, Q, 2)):
        c[i] = torch.tensor(sp[(start + j) % len(sp)], dtype=torch.float32)
    return c


def direct(bq, bk0, bk1, bc, bo, N, h1, w1, Hs, Ws, D, radius, scale, over=()):
    a = dict(q=bq.ptr, ldq=bq.ld, k0=bk0.ptr, ldk0=bk0.ld, k1=bk1.ptr, ldk1=bk1.ld, N=N, h1=h1, w1=w1, Hs=Hs, Ws=Ws, D=D, coords=bc.ptr, ldc=bc.ld,
             radius=radius, scale=scale, out=bo.ptr, ldo=bo.ld)
    a.update(over)                                                             # (same keys: the argument order stays the ABI's)
    return hip.lib().mrfa_corr_direct_fwd(hip.stream_ptr(), *a.values())


def run_direct(test, N, h1, w1, Hs, Ws, D, radius, coords, ref_dev="cpu", seed=0):
    QI, Q, nwin, H1, W1 = h1 * w1, N * h1 * w1, (2 * radius + 1) ** 2, Hs // 2, Ws // 2
    assert coords.shape == (Q, 2)
    g = torch.Generator().manual_seed(1000 * D + 10 * Hs + radius + seed)
    q, k0, k1 = torch.randn(Q, D, generator=g), torch.randn(N * Hs * Ws, D, generator=g), torch.randn(N * H1 * W1, D, generator=g)
    scale = torch.tensor(D ** -0.5, dtype=torch.float32).item()               # the fp32 value the kernel is handed
    bq, bk0, bk1 = Buf(q, 1, D + 4, NAN, lead=4), Buf(k0, 1, D + 8, NAN, lead=8), Buf(k1, 1, D + 12, NAN, lead=4)
    bc = Buf(coords, 1, 3, NAN)
    runs = []
    for _ in range(2):
        bo = Buf(torch.full((Q, 2 * nwin), NAN), 1, 2 * nwin + 5, CANARY, lead=3)
        hip.check(direct(bq, bk0, bk1, bc, bo, N, h1, w1, Hs, Ws, D, radius, scale), "mrfa_corr_direct_fwd")
        runs.append(bo)
    out = runs[0].get()
    assert torch.equal(runs[0].bits(), runs[1].bits()), "two runs differ"
    assert bq.untouched() and bk0.untouched() and bk1.untouched() and bc.untouched()
    rd = ref_dev
    qd = q.to(rd, F64).view(N, QI, D)
    vols, errs = [], []
    for k, H, W in ((k0, Hs, Ws), (k1, H1, W1)):
        kd = k.to(rd, F64).view(N, H * W, D)
        vols.append((scale * torch.matmul(qd, kd.transpose(1, 2))).reshape(Q, H, W))
        S = scale * torch.matmul(qd.abs(), kd.abs().transpose(1, 2))
        errs.append(((D + 2) * U / (1 - D * U) * S).reshape(Q, H, W))
    cd = coords.to(rd)
    res, res_e = R.corr_lookup_ref(vols[0], vols[1], cd, radius, full=True), R.corr_lookup_ref(errs[0], errs[1], cd, radius, full=True)
    for lvl, (r, re) in enumerate(zip(res, res_e)):
        o = out[:, lvl * nwin:(lvl + 1) * nwin].reshape(-1, 1)
        assert (o[(~r["live"]).cpu()] == 0).all(), "a dead sample is not exactly 0"
        E = re["tap_wide"]
        bound = E + 10 * U * (r["S_out"] + E) + (r["delta_x"] + r["delta_y"])[:, None] * 2 * r["tap_wide"]
        note(test, f"out{lvl}", check(o, r["out"], bound, f"{test}: level {lvl}"))
    return out


@pytest.mark.parametrize("radius", [0, 1, 3])
@pytest.mark.parametrize("D", [4, 36, 256])
@pytest.mark.parametrize("Hs,Ws", [(2, 2), (8, 8), (6, 10)])
def test_corr_direct(Hs, Ws, D, radius):
    """N = 2 with different keys per sample, 2 x 5 x 9 = 90 queries: every special coordinate once, random ones between"""
    test = f"direct r{radius} D{D} {Hs}x{Ws}"
    out = run_direct(test, 2, 5, 9, Hs, Ws, D, radius, make_coords(90, Hs, Ws, seed=Hs + D))
    assert out.abs().max() > 0.05                                              # (it correlated something)
    report(test, "corr direct")


@pytest.mark.parametrize("Q", [1, 5])
def test_corr_direct_few_queries(Q):
    """N = 1; one and five queries (less than a workgroup's four waves / a partly filled second workgroup), the special coordinates a few at a time"""
    test = f"direct Q{Q}"
    n = len(special_coords(8, 8))
    for start in range(0, n, 2 if Q > 1 else 1):
        run_direct(test, 1, 1, Q, 8, 8, 36, 3, make_coords(Q, 8, 8, seed=start, start=start), seed=start)
    report(test, "corr direct")


def test_corr_direct_more_queries_than_waves():
    """Q above the launched waves: every wave walks a run of two neighbouring queries, the last waves a shorter one or none"""
    N, h1, w1 = 2, 65, 67
    assert WAVES < N * h1 * w1 < 2 * WAVES - 64
    run_direct("direct many", N, h1, w1, 8, 8, 36, 3, make_coords(N * h1 * w1, 8, 8, seed=4), ref_dev=DEV)
    report("direct many", "corr direct")


def test_corr_direct_production_strides():
    """the RaftFlow shape of one 256^2 sample's coarse levels: 64 x 64 keys of 256 channels (the register-resident query path), radius 3"""
    run_direct("direct 64x64", 1, 8, 8, 64, 64, 256, 3, make_coords(64, 64, 64, seed=9))
    report("direct 64x64", "corr direct")


def test_corr_direct_refuses_bad_arguments():
    N, h1, w1, Hs, Ws, D, radius = 1, 2, 2, 4, 4, 8, 3
    g = torch.Generator().manual_seed(1)
    bq, bk0, bk1 = Buf(torch.randn(4, D, generator=g), 1, D + 4, NAN, lead=4), Buf(torch.randn(16, D, generator=g), 1, D + 4, NAN, lead=4), \
        Buf(torch.randn(4, D, generator=g), 1, D + 4, NAN, lead=4)
    bc = Buf(torch.ones(4, 2), 1, 2, NAN)
    bo = Buf(torch.full((4, 98), NAN), 1, 100, CANARY, lead=3)
    L = hip.lib()
    bad = [dict(radius=4), dict(radius=-1), dict(D=6), dict(D=0), dict(ldc=1), dict(ldo=97), dict(ldq=4), dict(ldk0=4), dict(ldk1=4), dict(ldq=D + 2),
           dict(ldk0=D + 2), dict(ldk1=D + 1), dict(Hs=3), dict(Ws=5), dict(Hs=0), dict(Ws=1), dict(q=bq.ptr + 4), dict(k0=bk0.ptr + 8), dict(k1=bk1.ptr + 4),
           dict(q=None), dict(out=None), dict(N=0)]
    for over in bad:
        rc = direct(bq, bk0, bk1, bc, bo, N, h1, w1, Hs, Ws, D, radius, 0.5, over)
        msg = L.mrfa_last_error().decode()
        assert rc != 0 and "corr_direct" in msg and len(msg) > 20, (over, rc, msg)
    assert bo.untouched()                                                      # nothing was launched
    for r in (0, 1, 2, 3):                                                     # what IS legal runs
        hip.check(direct(bq, bk0, bk1, bc, bo, N, h1, w1, Hs, Ws, D, r, 0.5), "mrfa_corr_direct_fwd")
    assert torch.isfinite(bo.get()).all()
