"""What the per-element kernel tests share (tests/test_sample_kernels_gpu.py, tests/test_token_kernels_gpu.py, tests/test_norm_kernels_gpu.py,
tests/test_prior_kernels_gpu.py): operands inside wider buffers whose surroundings are
watched, the |got - ref| <= bound assertion, and the err / bound ratios each test prints."""
import torch

DEV = "cuda:0"
U = 2.0 ** -24                                            # unit roundoff of fp32 (half an ulp, relative)
NAN = float("nan")
CANARY = -77.0
F64 = torch.float64


class Buf:
    """values [rows, C] inside a [lead + groups * gstride] buffer of `dtype` (float32; float64 for the BatchNorm statistics blocks) filled with `fill`: row r of
    group j starts at lead + j * gstride + r * ld"""

    def __init__(self, vals, groups, ld, fill, lead=0, gap=0, dev=DEV, dtype=torch.float32):
        rows_all, Cc = vals.shape
        self.rows, self.C, self.ld, self.groups, self.lead = rows_all // groups, Cc, ld, groups, lead
        self.gstride = self.rows * ld + gap
        self.flat = torch.full((lead + groups * self.gstride,), fill, dtype=dtype)
        self.fill = fill
        self._view(self.flat)[..., :Cc] = vals.view(groups, self.rows, Cc)
        self.orig = self.flat.clone()
        self.flat = self.flat.to(dev)

    def _view(self, flat):
        return flat[self.lead:].view(self.groups, self.gstride)[:, :self.rows * self.ld].view(self.groups, self.rows, self.ld)

    @property
    def ptr(self):
        return self.flat.data_ptr() + self.flat.element_size() * self.lead

    def _sync(self):
        if self.flat.is_cuda:
            torch.cuda.synchronize()

    def get(self):
        """the values back ([rows_all, C], cpu) after asserting that nothing outside the slice changed"""
        self._sync()
        now = self.flat.cpu()
        a, b = now.clone(), self.orig.clone()
        self._view(a)[..., :self.C] = 0
        self._view(b)[..., :self.C] = 0
        assert torch.equal(a.nan_to_num(nan=12345.0), b.nan_to_num(nan=12345.0)), "a kernel wrote outside its [.., :C] slice"
        return self._view(now)[..., :self.C].reshape(-1, self.C).clone()

    def bits(self):
        """the whole buffer as int32 (cpu): two of these compare bit by bit, NaN included"""
        self._sync()
        return self.flat.cpu().view(torch.int32).clone()

    def untouched(self):
        """the whole buffer, slice included, is bit-identical to what it was built with"""
        return torch.equal(self.bits(), self.orig.view(torch.int32))


def check(got, ref, bound, what, mask=None):
    """|got - ref| <= bound element by element; returns max(err / bound)"""
    got, ref, bound = got.to(F64).cpu(), ref.to(F64).cpu(), bound.to(F64).cpu()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    if mask is not None:
        m = mask.cpu().expand_as(got)
        got, ref, bound = got[m], ref[m], bound[m]
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    err = (got - ref).abs()
    bad = err > bound
    ratio = (err / bound.clamp(min=1e-300)).max().item() if err.numel() else 0.0
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements beyond the bound; first at flat index {i}: got {got.flatten()[i].item():.9g} "
                             f"ref {ref.flatten()[i].item():.9g} bound {bound.flatten()[i].item():.3e}; max err/bound {ratio:.3g}")
    return ratio


RATIOS = {}


def note(test, what, ratio):
    RATIOS[(test, what)] = max(RATIOS.get((test, what), 0.0), ratio)


def report(test, tag="sample"):
    items = [(w, r) for (t, w), r in RATIOS.items() if t == test]
    print(f"[{tag}] {test}: max err/bound " + "  ".join(f"{w} {r:.3f}" for w, r in items))
