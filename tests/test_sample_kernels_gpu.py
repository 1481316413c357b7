"""Every kernel of csrc/sample.hip on every dispatch path against the float64 reference of tests/ref_sample.py (-m gpu), element by element.

THE BOUND.  No tolerance here is a fraction of a tensor's maximum: each assertion is |got - ref| <= bound per element, and the bound is built from the
reference's companion outputs by counting the fp32 roundings of the ABI's formula.  u = 2^-24 is the unit roundoff (half an ulp, relative).

  rounding term  (k + c) u S.   S is the sum of the absolute values of the contributions to the element (for +=: the old value included), k their number
                 (k - 1 additions, each on a partial sum <= S, plus one for +=), c the roundings inside ONE contribution:
                   forward      w v with w = (1 - fx)(1 - fy): fx, fy, 1 - fx, 1 - fy, the product of the weights, the product with v: c = 6, k = 4  -> 10 u S
                   din / dvol   g w: the same weight, times g: c = 6 (fx and fy are shared), k = k_din + 1 (the old value)              -> (k_din + 7) u S
                   dgrid        g ((v01 - v00)(1 - fy) + (v11 - v10) fy): a difference, 1 - fy, two products, a sum, times g: 6; then the factor
                                W / 2 of mode 0 and the += : c = 8, k = C (one term per channel; a wave's shuffle tree or the <= 8 chunk atomics of a
                                pixel add fewer roundings than a serial sum of C terms)                                                  -> (C + 8) u S
                   resize fwd   ((v00 (1 - fx) + v01 fx)(1 - fy) + (..) fy) mul (+ old): 1 - fx, 1 - fy, four products and the adds are k;
                                mul, += : c = 8, k = 4                                                                                  -> 12 u S
                   resize bwd   g mul w, as din                                                                                         -> (k_din + 7) u S
  coordinate term.  The kernel evaluates the sample coordinate in fp32, the reference in float64 from the same fp32 grid values.  delta = one ulp (twice the
                 rounding error) of the result of each fp32 operation of the formula, carried to the end (ref_sample.gs_coords: mode 0 three operations,
                 mode 1 one; the lookup one; the resize two).  A bilinear weight is Lipschitz-1 in each coordinate and the |d w / d x| of a row of taps sum
                 to 2, so a forward value moves by at most (dx + dy) 2 max|tap|, an input-gradient element by sum |g_p| (dx_p + dy_p) over the points p that
                 can reach it (C_din), and a dgrid component by delta of the OTHER axis times sum_c |g| (|v00| + |v01| + |v10| + |v11|) (T).  A coordinate
                 may round across an integer, which changes the tap set but not the (continuous) value: max|tap| and C_din are taken over the 4 x 4
                 neighbourhood for that reason.
  dgrid / dcoords are discontinuous at integer coordinates: elements whose coordinate lies within delta of an integer are compared only where every fp32
  step of the coordinate formula is exact (the deliberate integer / border coordinates: the kernel then has the reference's coordinate itself); the
  others are left out, and the test asserts that this is at most 0.1 % of the elements.
  Dead samples (NaN, +-inf, <= -1, >= W): out == 0, dgrid / dcoords bit-identical to their old value, nothing in din (the bound there has no term from them).

Every operand sits in a wider buffer: inputs NaN outside their [.., :C] slice, outputs a canary that must survive."""
import pytest
import torch

from mrfa_amd import hip
from tests import ref_sample as R
from tests.kernel_check import CANARY, DEV, F64, NAN, U, Buf, check, note, report
from tests.sample_grids import FLOWS, flow_grid, gs_grid

pytestmark = pytest.mark.gpu

CAP = 256 * 16                                            # stream_grid (csrc/common.h): at most this many 256-thread workgroups, the rest grid-strides
VEC_C = lambda c: c % 256 == 0 or c in (64, 128)


def steps(work_threads):
    """trip count of the busiest thread's grid-stride loop in a stream_grid launch over `work_threads` threads' worth of work"""
    blocks = min(max((work_threads + 255) // 256, 1), CAP)
    return -(-work_threads // (blocks * 256))


def call(name, *args):
    hip.check(getattr(hip.lib(), name)(hip.stream_ptr(), *args), name)


# ================================================================================================================== grid_sample
def gs_family(Cc, aligned, din):
    """the kernel mrfa_grid_sample_fwd / _bwd dispatch to, by construction of the operands"""
    vec = VEC_C(Cc) and aligned
    lpp = 64 if Cc % 256 == 0 else (32 if Cc == 128 else 16)
    return (f"fwd_vec<{lpp}>" if vec else "fwd"), (f"bwd_vec<{lpp}>" if vec and not din else "bwd")


def run_gs(test, Cc, Nin, in_rep, Hi, Wi, Ho, Wo, mode, grid, *, ldg=2, aligned=True, expect=None, ref_dev="cpu", seed=0, min_steps=None,
           variants=("din+dgrid", "din", "dgrid"), exact_only=False, placed=()):
    N = Nin * in_rep
    npix = N * Ho * Wo
    g = torch.Generator().manual_seed(1000 * Cc + 10 * Wo + mode + seed)
    pad = 4 if aligned else 1
    ldi, ldo, lddo, lddi = Cc + pad, Cc + pad + (4 if aligned else 0), Cc + pad, Cc + pad + 4
    x = torch.randn(Nin * Hi * Wi, Cc, generator=g) * 2
    dout = torch.randn(npix, Cc, generator=g)
    din0 = torch.randn(Nin * Hi * Wi, Cc, generator=g)
    dg0 = torch.randn(npix, 2, generator=g)
    lead = 4 if aligned else 1
    bx = Buf(x, Nin, ldi, NAN, lead=lead, gap=8)
    bg = Buf(grid, 1, ldg, NAN)
    bo = Buf(torch.full((npix, Cc), NAN), 1, ldo, CANARY, lead=lead)
    bdo = Buf(dout, 1, lddo, NAN, lead=lead)
    is_aligned = all(v % 4 == 0 for v in (ldi, ldo, lddo, bx.gstride)) and all(p % 16 == 0 for p in (bx.ptr, bo.ptr, bdo.ptr))
    assert is_aligned == aligned or not VEC_C(Cc)
    fam_f, _ = gs_family(Cc, is_aligned, True)
    if expect is not None:
        assert fam_f == expect[0], (fam_f, expect)
    if min_steps:
        work = {"fwd": npix * Cc}.get(fam_f, npix * Cc // 4)
        assert steps(work) >= min_steps, (fam_f, steps(work))

    rd = ref_dev
    x4, g4 = x.view(Nin, Hi, Wi, Cc).to(rd), grid.view(N, Ho, Wo, 2).to(rd)
    r = R.grid_sample_grads_ref(x4, g4, dout.view(N, Ho, Wo, Cc).to(rd), mode, in_rep, full=True, din0=din0.view(Nin, Hi, Wi, Cc).to(rd))
    live, dxy = r["live"], (r["dx"] + r["dy"])
    exact = R.gs_coords_exact(g4, mode, Hi, Wi)
    if exact_only:
        assert exact[live].all(), "this flow is meant to be exact in fp32"

    # ---- forward
    call("mrfa_grid_sample_fwd", bx.ptr, ldi, bx.gstride, in_rep, Hi, Wi, Cc, bg.ptr, ldg, N, Ho, Wo, bo.ptr, ldo, mode)
    out = bo.get()
    assert (out[(~live).cpu()] == 0).all(), "a dead sample's output is not exactly 0"
    note(test, "out", check(out, r["out"], 10 * U * r["S_out"] + dxy[:, None] * 2 * r["tap_wide"], f"out [{fam_f}]"))

    # ---- backward, three ways
    near = live & ((r["dist_x"] <= r["dx"]) | (r["dist_y"] <= r["dy"])) & ~exact
    rnd = near.clone()
    rnd[list(placed)] = False                               # (placed integers that mode 0 cannot reach exactly on a 9 x 7 image are not the random share)
    assert rnd.double().mean().item() <= 1e-3, f"{rnd.sum().item()} of {npix} random dgrid rows left out"
    for var in variants:
        want_din, want_dg = "din" in var, "dgrid" in var
        _, fam_b = gs_family(Cc, is_aligned, want_din)
        if expect is not None:
            assert fam_b == (expect[1] if want_din else expect[2]), (var, fam_b, expect)
        if min_steps:
            work = npix * Cc // 4 if fam_b != "bwd" else N * Ho * -(-Wo // 8) * -(-Cc // 64) * 64
            assert steps(work) >= min_steps, (fam_b, steps(work))
        bdi = Buf(din0, Nin, lddi, CANARY, lead=lead, gap=12) if want_din else None
        bdg = Buf(dg0, 1, 3, CANARY) if want_dg else None
        call("mrfa_grid_sample_bwd", bx.ptr, ldi, bx.gstride, in_rep, Hi, Wi, Cc, bg.ptr, ldg, N, Ho, Wo, bdo.ptr, lddo, mode,
             bdi.ptr if bdi else None, lddi, bdi.gstride if bdi else 0, bdg.ptr if bdg else None, 3)
        if want_din:
            bound = (r["k_din"][..., None] + 7) * U * r["S_din"] + r["C_din"]
            note(test, f"din[{var}]", check(bdi.get(), (r["din"] + din0.view(Nin, Hi, Wi, Cc).to(rd)).view(-1, Cc), bound.view(-1, Cc), f"din [{fam_b}, {var}]"))
        if want_dg:
            dg = bdg.get()
            assert torch.equal(dg[(~live).cpu()], dg0[(~live).cpu()]), "a dead sample changed dgrid"
            ref = r["dgrid"].view(-1, 2) + dg0.to(rd)
            Sx, Sy = r["S_gx"] * r["mx"] + dg0[:, 0].to(rd).abs(), r["S_gy"] * r["my"] + dg0[:, 1].to(rd).abs()
            bound = torch.stack([(Cc + 8) * U * Sx + r["dy"] * r["T"] * r["mx"], (Cc + 8) * U * Sy + r["dx"] * r["T"] * r["my"]], dim=1)
            note(test, f"dgrid[{var}]", check(dg, ref, bound, f"dgrid [{fam_b}, {var}]", mask=(~near)[:, None]))
        bx.get(), bg.get(), bdo.get()                                                # the inputs are untouched


GS_C = {3: ("fwd", "bwd", "bwd"), 2: ("fwd", "bwd", "bwd"), 64: ("fwd_vec<16>", "bwd", "bwd_vec<16>"), 96: ("fwd", "bwd", "bwd"),
        128: ("fwd_vec<32>", "bwd", "bwd_vec<32>"), 130: ("fwd", "bwd", "bwd"), 256: ("fwd_vec<64>", "bwd", "bwd_vec<64>"),
        512: ("fwd_vec<64>", "bwd", "bwd_vec<64>")}
SCALAR = ("fwd", "bwd", "bwd")
PLACED = list(range(3, 29, 2))                            # the rows sample_grids.gs_grid places its `special` coordinates in


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Cc", list(GS_C))
def test_grid_sample_special_and_outside_coordinates(Cc, mode):
    """the coordinate lists of sample_grids.gs_grid (integers, -1, W - 1, W, -0.999, far outside, NaN, inf) among random ones, every channel count of the
    dispatch (scalar forward; vec forward at 16 / 32 / 64 lanes per pixel with one and two chunks; scalar backward with 1 and 3 chunks and a ragged last
    one; vec backward at all three widths), in_rep 1 / 3 / 11, grid rows of 2 and 3 floats, Wo = 13 (a ragged run)"""
    test = f"special C{Cc} m{mode}"
    for in_rep, Nin, ldg in ((1, 2, 2), (3, 1, 3), (11, 1, 2)):
        if in_rep == 11 and Cc > 3:
            continue
        Hi, Wi, Ho, Wo = (8, 16, 11, 13) if in_rep == 3 else (9, 7, 11, 13)             # power-of-two sizes: mode 0 reaches the integers exactly
        grid, outside = gs_grid(Nin * in_rep, Ho, Wo, Hi, Wi, mode, seed=Cc + in_rep)
        run_gs(test, Cc, Nin, in_rep, Hi, Wi, Ho, Wo, mode, grid, ldg=ldg, expect=GS_C[Cc], seed=in_rep, placed=PLACED)
    report(test)


@pytest.mark.parametrize("Cc", [64, 128, 256])
def test_grid_sample_misaligned_operands_take_the_scalar_kernels(Cc):
    """a vec shape with ld = C + 1 and 4-byte aligned bases: the scalar kernels on the operands of the vec case above (same seed, same values)"""
    test = f"misaligned C{Cc}"
    Hi, Wi, Ho, Wo = 9, 7, 11, 13
    for mode in (0, 1):
        grid, _ = gs_grid(2, Ho, Wo, Hi, Wi, mode, seed=Cc + 1)
        run_gs(test, Cc, 2, 1, Hi, Wi, Ho, Wo, mode, grid, aligned=False, expect=SCALAR, seed=1, placed=PLACED)
    report(test)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Wo", [1, 5, 8, 9, 21, 64])
@pytest.mark.parametrize("kind", FLOWS)
def test_grid_sample_flows_and_run_geometry(kind, Wo, mode):
    """the flows the carried-column merge of grid_sample_bwd_kernel is for (shift, identity: a merge on every step) and against (collapse, reverse, stride2,
    sinus: in and out of the image inside a run), on rows of one pixel, a short run, exactly one run, one run and a tail of one, ragged tails and several
    runs; power-of-two input sizes, so that both modes sample the same, fp32-exact pixel coordinates.  C = 3 (the image warp) and C = 96 (a ragged
    second channel chunk) through the scalar kernels, C = 64 through the vec ones."""
    test = f"flow {kind} Wo{Wo} m{mode}"
    Hi, Wi, Ho = 8, 16, 6
    for Cc, Nin, in_rep in ((3, 1, 2), (96, 2, 1), (64, 2, 1)):
        N = Nin * in_rep
        grid = flow_grid(kind, N, Ho, Wo, Hi, Wi, mode)
        run_gs(test, Cc, Nin, in_rep, Hi, Wi, Ho, Wo, mode, grid, expect=GS_C[Cc], exact_only=True)
    report(test)


@pytest.mark.parametrize("Cc,N,Ho,Wo", [(3, 6, 256, 256), (64, 2, 250, 270), (128, 2, 200, 220), (256, 2, 120, 140)])
def test_grid_sample_production_sizes_take_every_grid_stride_loop_twice(Cc, N, Ho, Wo):
    """more work than stream_grid's 4096 x 256 threads in every kernel family: the i += gridDim.x * blockDim.x steps, the iters / live tail of the vec
    backward, the wave loop of the scalar backward (asserted from the launch arithmetic).  Random flows of +-5 pixels, mode 1; reference on the device."""
    test = f"production C{Cc}"
    in_rep = 3 if Cc == 3 else 1
    Hi, Wi = Ho // 2 + 3, Wo // 2 + 5
    g = torch.Generator().manual_seed(Cc)
    grid = torch.rand(N * Ho * Wo, 2, generator=g) * 10 - 5 + torch.tensor([-Wo / 4.0, -Ho / 4.0])
    grid[::1000] = NAN
    run_gs(test, Cc, N // in_rep, in_rep, Hi, Wi, Ho, Wo, 1, grid, expect=GS_C[Cc], ref_dev=DEV, min_steps=2)
    report(test)


# ================================================================================================================== correlation lookup
def corr_coords(Q, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(Q, 2, generator=g) * torch.tensor([Ws + 8.0, Hs + 8.0]) - 4
    placed = [(3.0, 5.0), (4.0, 2.0), (5.0, 3.0), (1.0, 7.0),                      # integers; odd ones are half-integers on level 1
              (0.0, 0.0), (Ws - 1.0, 0.0), (0.0, Hs - 1.0), (Ws - 1.0, Hs - 1.0),  # the four corners
              (-2.5, 1.25), (Ws + 1.5, Hs - 0.75), (0.5, -3.0),                    # a window partly outside
              (-30.0, -30.0), (4.0 * Ws, 2.0), (1e9, 1e9),                         # wholly outside on both levels
              (NAN, 1.0), (2.0, NAN), (float("inf"), 3.0)]
    for i, p in enumerate(placed):
        c[1 + 2 * i] = torch.tensor(p)
    return c


def run_corr(test, Q, Hs, Ws, radius, ldc, coords, ref_dev="cpu", variants=("dvol+dcoords", "dvol", "dcoords")):
    nwin = (2 * radius + 1) ** 2
    g = torch.Generator().manual_seed(Q + Hs + radius)
    H1, W1 = Hs // 2, Ws // 2
    v0, v1 = torch.randn(Q, Hs * Ws, generator=g), torch.randn(Q, H1 * W1, generator=g)
    dout = torch.randn(Q, 2 * nwin, generator=g)
    d00, d10, dc0 = torch.randn(Q, Hs * Ws, generator=g), torch.randn(Q, H1 * W1, generator=g), torch.randn(Q, 2, generator=g)
    ldo = 2 * nwin + 5
    bc = Buf(coords, 1, ldc, NAN)
    bo = Buf(torch.full((Q, 2 * nwin), NAN), 1, ldo, CANARY, lead=3)
    bdo = Buf(dout, 1, ldo + 2, NAN, lead=1)
    v0d, v1d = v0.to(DEV), v1.to(DEV)
    rd = ref_dev
    res, dc = R.corr_lookup_grads_ref(v0.view(Q, Hs, Ws).to(rd), v1.view(Q, H1, W1).to(rd), coords.to(rd), dout.to(rd), radius, full=True,
                                      dvol0=(d00.view(Q, Hs, Ws).to(rd), d10.view(Q, H1, W1).to(rd)))
    call("mrfa_corr_lookup_fwd", v0d.data_ptr(), v1d.data_ptr(), Hs, Ws, bc.ptr, ldc, Q, radius, bo.ptr, ldo)
    out = bo.get()
    for lvl, r in enumerate(res):
        o = out[:, lvl * nwin:(lvl + 1) * nwin].reshape(-1, 1)
        assert (o[(~r["live"]).cpu()] == 0).all()
        bound = 10 * U * r["S_out"] + (r["delta_x"] + r["delta_y"])[:, None] * 2 * r["tap_wide"]
        note(test, f"out{lvl}", check(o, r["out"], bound, f"corr out level {lvl}"))
    exact = R.corr_coords_exact(coords.to(rd), radius)
    near = torch.zeros(Q, dtype=torch.bool, device=rd)
    alive = torch.zeros(Q, dtype=torch.bool, device=rd)
    for r in res:
        near |= (r["live"] & ((r["dist_x"] <= r["delta_x"]) | (r["dist_y"] <= r["delta_y"]))).view(Q, nwin).any(1)
        alive |= r["live"].view(Q, nwin).any(1)
    near &= ~exact
    assert near.double().mean().item() <= 1e-3
    for var in variants:
        want_v, want_c = "dvol" in var, "dcoords" in var
        d0, d1 = (d00.to(DEV), d10.to(DEV)) if want_v else (None, None)
        bdc = Buf(dc0, 1, 3, CANARY) if want_c else None
        call("mrfa_corr_lookup_bwd", v0d.data_ptr(), v1d.data_ptr(), Hs, Ws, bc.ptr, ldc, Q, radius, bdo.ptr, ldo + 2,
             d0.data_ptr() if want_v else None, d1.data_ptr() if want_v else None, bdc.ptr if want_c else None, 3)
        torch.cuda.synchronize()
        if want_v:
            for lvl, (r, got, old) in enumerate(zip(res, (d0, d1), (d00, d10))):
                bound = (r["k_din"][..., None] + 7) * U * r["S_din"] + r["C_din"]
                note(test, f"dvol{lvl}[{var}]", check(got.view(-1, 1), (r["din"].view(-1, 1) + old.view(-1, 1).to(rd)), bound.view(-1, 1), f"dvol{lvl} [{var}]"))
        if want_c:
            got = bdc.get()
            assert torch.equal(got[(~alive).cpu()], dc0[(~alive).cpu()]), "a wholly dead window changed dcoords"
            bx = sum(r["inv"] * ((nwin + 8) * U * r["S_gx"] + r["delta_y"] * r["T"]).view(Q, nwin).sum(1) for r in res) + 3 * U * (dc0[:, 0].abs().to(rd) + dc.abs()[:, 0])
            by = sum(r["inv"] * ((nwin + 8) * U * r["S_gy"] + r["delta_x"] * r["T"]).view(Q, nwin).sum(1) for r in res) + 3 * U * (dc0[:, 1].abs().to(rd) + dc.abs()[:, 1])
            note(test, f"dcoords[{var}]", check(got, dc + dc0.to(rd), torch.stack([bx, by], dim=1), f"dcoords [{var}]", mask=(~near)[:, None]))
        bc.get(), bdo.get()


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("Hs,Ws", [(16, 16), (8, 24), (64, 64)])
def test_corr_lookup(Hs, Ws, radius):
    """radius 1 and 2 (idle lanes >= (2r+1)^2 sample at -2), square / wide / production maps, coordinate rows of 2 and 3 floats, output rows wider than
    2 (2r+1)^2, coordinates placed on purpose (corr_coords), and each of dvol / dcoords absent in turn.  dcoords: the per-lane terms of both levels are
    summed over the wave: k = (2r+1)^2 terms per level, 8 roundings per term, 3 for the level sum and the +=."""
    test = f"corr r{radius} {Hs}x{Ws}"
    for ldc in (2, 3):
        run_corr(test, 60, Hs, Ws, radius, ldc, corr_coords(60, Hs, Ws, seed=ldc))
    report(test)


def test_corr_lookup_more_queries_than_waves():
    """Q > 16 384 (stream_grid's 4096 workgroups x 4 waves): q += nwaves runs"""
    Q = 16384 + 4 * 777 + 1
    assert steps(Q * 64) >= 2
    run_corr("corr many", Q, 8, 8, 3, 2, corr_coords(Q, 8, 8, seed=4), ref_dev=DEV)
    report("corr many")


# ================================================================================================================== resize
def run_resize(test, N, Hi, Wi, Ho, Wo, Cc, mul=1.0, acc=False, ref_dev="cpu", min_steps=None):
    g = torch.Generator().manual_seed(Hi * 100 + Wo + Cc)
    x = torch.randn(N * Hi * Wi, Cc, generator=g)
    y0 = torch.randn(N * Ho * Wo, Cc, generator=g)
    dout = torch.randn(N * Ho * Wo, Cc, generator=g)
    din0 = torch.randn(N * Hi * Wi, Cc, generator=g)
    bx = Buf(x, 1, Cc + 3, NAN, lead=1)
    by = Buf(y0 if acc else torch.full_like(y0, NAN), 1, Cc + 2, CANARY, lead=2)
    bdo = Buf(dout, 1, Cc + 1, NAN)
    bdi = Buf(din0, 1, Cc + 5, CANARY, lead=3)
    rd = ref_dev
    rf = R.resize_ref(x.view(N, Hi, Wi, Cc).to(rd), Ho, Wo, mul, y0.view(N, Ho, Wo, Cc).to(rd) if acc else None, full=True)
    rb = R.resize_grads_ref((N, Hi, Wi, Cc), dout.view(N, Ho, Wo, Cc).to(rd), mul, full=True, din0=din0.view(N, Hi, Wi, Cc).to(rd))
    gather = Ho >= Hi and Wo >= Wi
    if min_steps:
        assert steps(N * Ho * Wo * Cc) >= min_steps and steps(N * (Hi * Wi if gather else Ho * Wo) * Cc) >= min_steps
    call("mrfa_resize_bilinear_fwd", bx.ptr, bx.ld, N, Hi, Wi, Cc, by.ptr, by.ld, Ho, Wo, mul, int(acc))
    call("mrfa_resize_bilinear_bwd", bdo.ptr, bdo.ld, N, Hi, Wi, Cc, bdi.ptr, bdi.ld, Ho, Wo, mul)
    out, din = by.get(), bdi.get()
    b_out = 12 * U * rf["S_out"] + rf["delta"][:, None] * 2 * rf["tap_wide"] * abs(mul)
    b_din = ((rb["k_din"][..., None] + 7) * U * rb["S_din"] + rb["C_din"]).view(-1, Cc)
    kind = "gather" if gather else "scatter"
    note(test, "out", check(out, rf["out"], b_out, "resize out"))
    note(test, f"din[{kind}]", check(din, rb["din"].view(-1, Cc) + din0.to(rd), b_din, f"resize din [{kind}]"))
    if not acc:
        # adjoint identity on the device results, in float64: <resize(x), g> = <x, resize_bwd(g)>, each side within its own element bounds
        lhs = (out.double() * dout.double()).sum().item()
        rhs = (x.double() * (din.double() - din0.double())).sum().item()
        slack = (b_out.cpu() * dout.double().abs()).sum().item() + (x.double().abs() * b_din.cpu()).sum().item()
        note(test, "adjoint", abs(lhs - rhs) / max(slack, 1e-300))
        assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)
    bx.get(), bdo.get()


RESIZES = [(64, 64, 256, 256, 1), (64, 64, 256, 256, 2), (64, 64, 256, 256, 98),    # production (the 98-channel one is past the grid cap)
           (7, 7, 50, 50, 3), (5, 5, 64, 64, 2), (50, 50, 7, 7, 2), (6, 40, 30, 9, 3),    # odd ratios; up in H and down in W together (the scatter path)
           (1, 1, 9, 9, 2), (9, 9, 1, 1, 2), (1, 7, 5, 1, 2), (12, 10, 12, 10, 3)]      # the s = 0 branches; same size


@pytest.mark.parametrize("shape", RESIZES)
def test_resize(shape):
    Hi, Wi, Ho, Wo, Cc = shape
    test = f"resize {Hi}x{Wi}->{Ho}x{Wo} C{Cc}"
    big = Ho * Wo * Cc > 100000
    run_resize(test, 2, Hi, Wi, Ho, Wo, Cc, ref_dev=DEV if big else "cpu")
    run_resize(test, 2, Hi, Wi, Ho, Wo, Cc, mul=-2.5, acc=True, ref_dev=DEV if big else "cpu")
    report(test)


@pytest.mark.parametrize("shape", [(128, 128, 130, 131, 40), (300, 290, 256, 256, 9)])
def test_resize_past_the_grid_cap(shape):
    """more elements than 4096 x 256 threads on the side each kernel loops over: forward and the gather backward (up), forward and the scatter backward (down)"""
    Hi, Wi, Ho, Wo, Cc = shape
    test = f"resize big {Hi}->{Ho}"
    run_resize(test, 2, Hi, Wi, Ho, Wo, Cc, mul=0.5, ref_dev=DEV, min_steps=2)
    report(test)


# ================================================================================================================== resize_sum_multi
def _rec(dst, ldd, N, Hd, Wd, Cc, ow, terms):
    d = hip.ResizeSumDesc()
    d.dst, d.ldd, d.N, d.Hd, d.Wd, d.C, d.nterm, d.overwrite = dst, ldd, N, Hd, Wd, Cc, len(terms), ow
    for k, (src, lds, Hs, Ws, mul) in enumerate(terms):
        d.term[k].src, d.term[k].lds, d.term[k].Hs, d.term[k].Ws, d.term[k].mul = src, lds, Hs, Ws, mul
    return d


@pytest.mark.parametrize("bwd", [False, True])
def test_resize_sum_multi_long_table_and_four_terms(bwd):
    """a table of 53 records (MRFA_RESIZE_SUM_MAX = 48: the base += 48 chunk loop of resize_sum_launch, a second launch with its own prefix table) with one-,
    two- and FOUR-term records on both sides of the chunk boundary, against the separate mrfa_copy_view / mrfa_resize_bilinear_* launches each record
    replaces AND against float64.  The two device forms evaluate the same expression (the compiler may contract different multiply-adds): each errs by at
    most the forward (backward) bound of a single resize per term plus one rounding per term of the chain."""
    N, Cc, nrec = 2, 2, 53
    g = torch.Generator().manual_seed(17 + bwd)
    sizes = [(3, 4), (6, 8), (5, 5), (6, 8), (12, 9)]
    dH, dW = (6, 8) if not bwd else (3, 4)                                             # forward: any source size; backward: sources (output gradients) >= dst
    pool = [s for s in sizes if not bwd or (s[0] >= dH and s[1] >= dW)]
    srcs = [(torch.randn(N * h * w, Cc + 1, generator=g), h, w) for h, w in pool for _ in range(2)]
    srcs_d = [t.to(DEV) for t, _, _ in srcs]
    dst0 = torch.randn(nrec, N * dH * dW, Cc + 2, generator=g)
    table, plan = [], []
    multi, sep = dst0.clone().to(DEV), dst0.clone().to(DEV)
    for i in range(nrec):
        nterm = 4 if i in (5, 50) else 1 + i % 2
        ow = 0 if bwd else i % 3 != 0
        terms = [((i + 3 * k) % len(srcs), (-1.0) ** k * (0.5 + 0.25 * ((i + k) % 4))) for k in range(nterm)]
        plan.append((ow, terms))
        table.append(_rec(multi[i].data_ptr() + 4, Cc + 2, N, dH, dW, Cc, int(ow),
                          [(srcs_d[j].data_ptr(), Cc + 1, srcs[j][1], srcs[j][2], m) for j, m in terms]))
    call("mrfa_resize_sum_multi_bwd" if bwd else "mrfa_resize_sum_multi", (hip.ResizeSumDesc * nrec)(*table), nrec)
    ref = dst0[:, :, 1:1 + Cc].double().clone()
    S = ref.abs()
    coord = torch.zeros_like(ref)
    for i, (ow, terms) in enumerate(plan):
        if ow:
            ref[i], S[i] = 0, 0
        for k, (j, m) in enumerate(terms):
            t, h, w = srcs[j]
            sv = t[:, :Cc].reshape(N, h, w, Cc)
            dptr, sptr = sep[i].data_ptr() + 4, srcs_d[j].data_ptr()
            first = bool(ow) and k == 0
            if (h, w) == (dH, dW):
                call("mrfa_copy_view", sptr, Cc + 1, N * h * w, Cc, dptr, Cc + 2, m, int(not first))
                ref[i] += m * sv.double().view(-1, Cc)
                S[i] += abs(m) * sv.double().abs().view(-1, Cc)
            elif not bwd:
                call("mrfa_resize_bilinear_fwd", sptr, Cc + 1, N, h, w, Cc, dptr, Cc + 2, dH, dW, m, int(not first))
                r = R.resize_ref(sv, dH, dW, m, full=True)
                ref[i] += r["out"]
                S[i] += r["S_out"]
                coord[i] += r["delta"][:, None] * 2 * r["tap_wide"] * abs(m)
            else:
                call("mrfa_resize_bilinear_bwd", sptr, Cc + 1, N, dH, dW, Cc, dptr, Cc + 2, h, w, m)
                r = R.resize_grads_ref((N, dH, dW, Cc), sv, m, full=True)
                ref[i] += r["din"].view(-1, Cc)
                S[i] += r["S_din"].view(-1, Cc) * (1 + r["k_din"].view(-1, 1) / 12)      # ((k_din + 7) + 5 of the chain) u S as 12 u S (1 + k / 12)
                coord[i] += r["C_din"].view(-1, Cc)
    torch.cuda.synchronize()
    multi, sep = multi.cpu(), sep.cpu()
    for t in (multi, sep):
        assert torch.equal(t[:, :, 0], dst0[:, :, 0]) and torch.equal(t[:, :, 1 + Cc:], dst0[:, :, 1 + Cc:]), "wrote outside the channel slice"
    bound = (12 + 4) * U * S + coord
    what = "bwd" if bwd else "fwd"
    note("resize_sum", f"{what} vs fp64", check(multi[:, :, 1:1 + Cc], ref, bound, "resize_sum_multi vs float64"))
    note("resize_sum", f"{what} separate vs fp64", check(sep[:, :, 1:1 + Cc], ref, bound, "separate launches vs float64"))
    note("resize_sum", f"{what} vs separate", check(multi[:, :, 1:1 + Cc], sep[:, :, 1:1 + Cc].double(), 2 * (12 + 4) * U * S, "resize_sum_multi vs separate launches"))
    report("resize_sum")


# ================================================================================================================== argument checks
def test_sampling_kernels_refuse_what_they_do_not_take():
    L = hip.lib()
    s = hip.stream_ptr()
    x = torch.zeros(64, 8, device=DEV)
    grid = torch.zeros(64, 2, device=DEV)
    can = [torch.full((64 * 8 * 4,), 5.0, device=DEV) for _ in range(2)]
    c0, c1 = can[0].data_ptr(), can[1].data_ptr()
    xp, gp = x.data_ptr(), grid.data_ptr()

    def refused(rc, name):
        msg = L.mrfa_last_error().decode()
        assert rc != 0 and len(msg) > 10 and name in msg, (rc, msg)

    def gsf(Hi=8, Wi=8, Cc=8, ldi=8, Ho=8, Wo=8, ldo=8, ldg=2, mode=1):
        return L.mrfa_grid_sample_fwd(s, xp, ldi, 64 * ldi, 1, Hi, Wi, Cc, gp, ldg, 1, Ho, Wo, c0, ldo, mode)

    def gsb(Hi=8, Wi=8, Cc=8, ldi=8, Ho=8, Wo=8, lddo=8, ldg=2, mode=1, lddi=8, lddg=2, din=True, dgrid=True):
        return L.mrfa_grid_sample_bwd(s, xp, ldi, 64 * ldi, 1, Hi, Wi, Cc, gp, ldg, 1, Ho, Wo, xp, lddo, mode, c0 if din else None, lddi, 64 * lddi,
                                      c1 if dgrid else None, lddg)
    for kw in (dict(mode=7), dict(mode=-1), dict(mode=2), dict(Hi=0), dict(Wi=-3), dict(Ho=0), dict(Wo=0), dict(Cc=0), dict(ldi=7), dict(ldo=4), dict(ldg=1)):
        refused(gsf(**kw), "grid_sample_fwd")
    for kw in (dict(mode=7), dict(mode=2), dict(Hi=0), dict(Wi=0), dict(Ho=-1), dict(Wo=0), dict(ldi=7), dict(lddo=7), dict(ldg=1), dict(lddi=7), dict(lddg=1)):
        refused(gsb(**kw), "grid_sample_bwd")
    assert gsb(lddi=0, din=False) == 0 and gsb(lddg=0, dgrid=False) == 0               # an absent gradient's leading dimension is not looked at

    def rsf(Hi=8, Wi=8, Cc=8, ldi=8, Ho=4, Wo=4, ldo=8):
        return L.mrfa_resize_bilinear_fwd(s, xp, ldi, 1, Hi, Wi, Cc, c0, ldo, Ho, Wo, 1.0, 0)

    def rsb(Hi=8, Wi=8, Cc=8, lddo=8, Ho=4, Wo=4, lddi=8):
        return L.mrfa_resize_bilinear_bwd(s, xp, lddo, 1, Hi, Wi, Cc, c0, lddi, Ho, Wo, 1.0)
    for kw in (dict(Hi=0), dict(Wi=0), dict(Ho=0), dict(Wo=-2), dict(Cc=0), dict(ldi=7), dict(ldo=3)):
        refused(rsf(**kw), "resize_fwd")
    for kw in (dict(Hi=0), dict(Wi=0), dict(Ho=0), dict(Wo=0), dict(Cc=-1), dict(lddo=7), dict(lddi=2)):
        refused(rsb(**kw), "resize_bwd")

    def clf(Hs=8, Ws=8, ldc=2, r=1, ldo=18):
        return L.mrfa_corr_lookup_fwd(s, xp, xp, Hs, Ws, gp, ldc, 4, r, c0, ldo)

    def clb(Hs=8, Ws=8, ldc=2, r=1, lddo=18, lddc=2, dc=True):
        return L.mrfa_corr_lookup_bwd(s, xp, xp, Hs, Ws, gp, ldc, 4, r, xp, lddo, c0, c1, c1 if dc else None, lddc)
    for kw in (dict(Hs=0), dict(Hs=1), dict(Ws=-4), dict(ldc=1), dict(r=-1), dict(r=4), dict(ldo=17)):
        refused(clf(**kw), "corr_lookup")
    for kw in (dict(Hs=0), dict(Ws=1), dict(ldc=0), dict(r=-2), dict(r=5), dict(lddo=10), dict(lddc=1)):
        refused(clb(**kw), "corr_lookup")
    torch.cuda.synchronize()
    c0v, c1v = can[0].clone(), can[1].clone()
    # the accepted calls above (absent gradients) wrote zeros' worth of gradient: += 0 on a canary of 5 leaves 5
    assert (c0v == 5).all() and (c1v == 5).all()
