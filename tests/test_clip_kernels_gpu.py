"""The kernels of a clip against one cached source (-m gpu): mrfa_corr_direct_rep_fwd (query image n reads key image n // k_rep) against the existing
mrfa_corr_direct_fwd on physically repeated keys, and mrfa_grid_sample_fwd / mrfa_grid_sample_bf16_fwd with in_rep against the same call on a repeated
input.  Both are the same arithmetic in the same order at another address, so every comparison is bit for bit (torch.equal on the whole output buffer,
padding and canary included); mrfa_corr_direct_fwd itself is held to float64 by tests/test_corr_direct_gpu.py."""
import pytest
import torch

from mrfa_amd import hip
from tests.kernel_check import CANARY, DEV, NAN, Buf
from tests.test_corr_direct_gpu import direct, make_coords

pytestmark = pytest.mark.gpu

N, H1, W1, HS, WS = 6, 4, 6, 8, 4


def rep_direct(bq, bk0, bk1, bc, bo, N, k_rep, h1, w1, Hs, Ws, D, radius, scale, over=()):
    a = dict(q=bq.ptr, ldq=bq.ld, k0=bk0.ptr, ldk0=bk0.ld, k1=bk1.ptr, ldk1=bk1.ld, N=N, k_rep=k_rep, h1=h1, w1=w1, Hs=Hs, Ws=Ws, D=D, coords=bc.ptr, ldc=bc.ld,
             radius=radius, scale=scale, out=bo.ptr, ldo=bo.ld)
    a.update(over)                                                             # (same keys: the argument order stays the ABI's)
    return hip.lib().mrfa_corr_direct_rep_fwd(hip.stream_ptr(), *a.values())


def operands(D, k_rep, seed=0):
    """queries of N images, keys of N / k_rep images and the same keys repeated k_rep times; every operand inside a wider buffer (ld > D, the first row at a
    channel offset, NaN around); centres inside, on the border, more than a window outside on every side, NaN (tests/test_corr_direct_gpu.py's list)"""
    Q, Nk = N * H1 * W1, N // k_rep
    g = torch.Generator().manual_seed(100 * D + k_rep + seed)
    q = torch.randn(Q, D, generator=g)
    k0, k1 = torch.randn(Nk, HS * WS, D, generator=g), torch.randn(Nk, (HS // 2) * (WS // 2), D, generator=g)
    coords = make_coords(Q, HS, WS, seed=D + k_rep)
    assert torch.isnan(coords).any() and (coords[:, 0] > WS + 8).any() and (coords[:, 0] < -8).any() and (coords[:, 1] > HS + 8).any() and (coords[:, 1] < -8).any()
    mk = lambda t, ld, lead: Buf(t.reshape(-1, D).contiguous(), 1, ld, NAN, lead=lead)
    rep = lambda t: t.repeat_interleave(k_rep, dim=0)
    return (Buf(q, 1, D + 4, NAN, lead=4), mk(k0, D + 8, 8), mk(k1, D + 12, 4), mk(rep(k0), D + 8, 8), mk(rep(k1), D + 12, 4), Buf(coords, 1, 3, NAN))


def out_buf(radius):
    nwin = (2 * radius + 1) ** 2
    return Buf(torch.full((N * H1 * W1, 2 * nwin), NAN), 1, 2 * nwin + 5, CANARY, lead=3)


@pytest.mark.parametrize("k_rep", [3, 1, 6])
@pytest.mark.parametrize("radius", [3, 1])
@pytest.mark.parametrize("D", [256, 24])
def test_corr_direct_rep_equals_the_entry_on_repeated_keys(D, radius, k_rep):
    """k_rep = 3: two key images (n // 3, where n % 3 would read the wrong one); k_rep = 1: the existing entry's own case; k_rep = N: one key image.
    D = 256 is the register-resident query path, D = 24 the generic one.  A rerun is bit-identical."""
    bq, bk0, bk1, rk0, rk1, bc = operands(D, k_rep)
    scale = torch.tensor(D ** -0.5, dtype=torch.float32).item()
    got, again, ref = out_buf(radius), out_buf(radius), out_buf(radius)
    hip.check(rep_direct(bq, bk0, bk1, bc, got, N, k_rep, H1, W1, HS, WS, D, radius, scale), "mrfa_corr_direct_rep_fwd")
    hip.check(rep_direct(bq, bk0, bk1, bc, again, N, k_rep, H1, W1, HS, WS, D, radius, scale), "mrfa_corr_direct_rep_fwd")
    hip.check(direct(bq, rk0, rk1, bc, ref, N, H1, W1, HS, WS, D, radius, scale), "mrfa_corr_direct_fwd")
    assert torch.equal(got.bits(), ref.bits()), "differs from mrfa_corr_direct_fwd on repeated keys"
    assert torch.equal(got.bits(), again.bits()), "two runs differ"
    out = got.get()                                                            # (asserts the padding / canary survived)
    assert torch.isfinite(out).all() and out.abs().max() > 0.05               # it correlated something
    assert all(b.untouched() for b in (bq, bk0, bk1, bc))
    if k_rep == 3:                                                             # the two sources' keys really differ: n % k_rep would not pass
        wrong = out_buf(radius)
        mixed = lambda b, S: Buf(b.orig[b.lead:].view(2, S, b.ld)[:, :, :D].repeat(3, 1, 1).reshape(-1, D).contiguous(), 1, b.ld, NAN, lead=b.lead)
        hip.check(direct(bq, mixed(bk0, HS * WS), mixed(bk1, HS * WS // 4), bc, wrong, N, H1, W1, HS, WS, D, radius, scale), "mrfa_corr_direct_fwd")
        assert not torch.equal(got.bits(), wrong.bits())


def test_corr_direct_rep_refuses_bad_arguments_and_leaves_out_untouched():
    D, radius = 24, 3
    bq, bk0, bk1, _, _, bc = operands(D, 3)
    L = hip.lib()
    for over in (dict(k_rep=4), dict(k_rep=0), dict(k_rep=-2), dict(N=7), dict(radius=4), dict(D=6), dict(ldk0=4), dict(Hs=3), dict(out=None), dict(N=0)):
        bo = out_buf(radius)
        rc = rep_direct(bq, bk0, bk1, bc, bo, N, 3, H1, W1, HS, WS, D, radius, 0.5, over)
        msg = L.mrfa_last_error().decode()
        assert rc != 0 and "corr_direct" in msg and len(msg) > 20, (over, rc, msg)
        assert bo.untouched(), over                                            # nothing was launched
    bo = out_buf(radius)
    hip.check(rep_direct(bq, bk0, bk1, bc, bo, N, 3, H1, W1, HS, WS, D, radius, 0.5), "mrfa_corr_direct_rep_fwd")
    assert torch.isfinite(bo.get()).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grid_sample_in_rep_equals_the_call_on_a_repeated_input(dtype, mode):
    """C = 8 at 5 x 7 -> 6 x 4, two input images for six output images (in_rep = 3): bit for bit the same call (in_rep = 1) on the input repeated"""
    Nin, rep, C, Hi, Wi, Ho, Wo = 2, 3, 8, 5, 7, 6, 4
    Nout = Nin * rep
    g = torch.Generator().manual_seed(11 + mode)
    x = torch.randn(Nin, Hi * Wi, C, generator=g)
    if mode == 0:                                                              # normalised coordinates, some outside [-1, 1]
        grid = torch.rand(Nout * Ho * Wo, 2, generator=g) * 2.6 - 1.3
    else:                                                                      # a flow in pixels around the identity, some of it off the map
        grid = torch.randn(Nout * Ho * Wo, 2, generator=g) * 3.0
    grid_d = grid.to(DEV)
    xr = x.repeat_interleave(rep, dim=0)
    outs = []
    for inp, in_rep in ((x, rep), (xr, 1)):
        out = torch.full((Nout * Ho * Wo, C + 4), CANARY, device=DEV)
        if dtype == torch.bfloat16:
            d = inp.to(DEV).to(torch.bfloat16).contiguous()
            fn = hip.lib().mrfa_grid_sample_bf16_fwd
        else:
            d = inp.to(DEV).contiguous()
            fn = hip.lib().mrfa_grid_sample_fwd
        hip.check(fn(hip.stream_ptr(), d.data_ptr(), C, Hi * Wi * C, in_rep, Hi, Wi, C, grid_d.data_ptr(), 2, Nout, Ho, Wo, out.data_ptr(), C + 4, mode),
                  "grid_sample")
        torch.cuda.synchronize()
        outs.append(out.cpu())
    a, b = outs
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert (a[:, C:] == CANARY).all() and torch.isfinite(a).all() and a[:, :C].abs().max() > 0.1
    per = a[:, :C].view(Nin, rep, Ho * Wo, C)
    assert not torch.equal(per[0], per[1])                                     # the two inputs really differ
