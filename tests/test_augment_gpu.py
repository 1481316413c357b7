"""PairAugmenter on the GPU (-m gpu): the device run equals the same call on CPU memory through the specification (tests/emu_data.py), bit for bit; and its
out= tensors feed one eager training step."""
import random

import pytest
import torch

from mrfa_amd.augment import PairAugmenter
from tests import ref_augment as R
from tests.emu_data import emulated_data_hip
from tests.test_augment_cpu import VOX1_AUG

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("seed", range(4))
def test_device_run_equals_the_specification(seed):
    x = torch.from_numpy(R.det_bytes(f"augment/gpu/module/{seed}", (4, 2, 64, 64, 3)))
    params = PairAugmenter.from_config(VOX1_AUG, rng=random.Random(seed)).draw(4)
    with emulated_data_hip():
        want = PairAugmenter.from_config(VOX1_AUG)(x, params)
    aug = PairAugmenter.from_config(VOX1_AUG, rng=random.Random(seed))
    got = aug(x.to(DEV))                                                       # params=None: the augmenter draws the same four from its generator
    assert got[0].device == DEV and got[0].shape == (4, 3, 64, 64) and got[0].dtype == torch.float32
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
    again = aug(x.to(DEV), params)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])     # two runs, bit for bit


def test_out_feeds_an_eager_train_step():
    """The augmenter writes into given (B,3,256,256) tensors, which go straight into train_step; a twin model at the same weights takes the same floats as
    fresh tensors.  The inputs are the same bits; the two losses are two launches of one program, which the fp32 atomics of the split reductions let differ
    by rounding (tests/test_graph_gpu.py bounds two such launches by 1e-4 on outputs in [0, 1]; an L1 mean of them moves by no more)."""
    from mrfa_amd.train import make_optimizer, train_step
    from tests.test_graph_gpu import _hotpath
    x = torch.from_numpy(R.det_bytes("augment/gpu/step", (2, 2, 256, 256, 3))).to(DEV)
    aug = PairAugmenter.from_config(VOX1_AUG, rng=random.Random(0))
    params = aug.draw(2)
    out = (torch.zeros(2, 3, 256, 256, device=DEV), torch.zeros(2, 3, 256, 256, device=DEV))
    source, driving = aug(x, params, out=out)
    assert source is out[0] and driving is out[1]
    with emulated_data_hip():
        want = PairAugmenter.from_config(VOX1_AUG)(x.cpu(), params)
    assert torch.equal(source.cpu(), want[0]) and torch.equal(driving.cpu(), want[1])
    ma, mb = _hotpath("augstep").train(), _hotpath("augstep").train()
    la = float(train_step(ma, make_optimizer(ma), source, driving))
    lb = float(train_step(mb, make_optimizer(mb), want[0].to(DEV), want[1].to(DEV)))
    assert la == la and abs(la) < float("inf") and abs(la - lb) <= 1e-4, (la, lb)
