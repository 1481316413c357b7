"""PairAugmenter's host logic on CPU memory, through the numpy specification of the data library (tests/emu_data.py): the draw against the reference's own
run (golden augment_reference: seeds 0..15), rng isolation, hand-built parameters, both configs, the split above the per-launch maximum, out=, every
refusal, and the outputs against the reference's.  Then the guards of mrfa_amd.data_hip.lib().  No GPU."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import mrfa_amd
from mrfa_amd import data_hip
from mrfa_amd.augment import PairAugmenter, PairDraw, PairParams, hue_shift_of
from tests import ref_augment as R
from tests.emu_data import emulated_data_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# dataset_params.augmentation_params of the two training configs (vox1.yaml, celebvhq.yaml), as yaml.safe_load returns them
VOX1_AUG = {"flip_param": {"horizontal_flip": True, "time_flip": True}, "jitter_param": {"brightness": 0.1, "contrast": 0.1, "saturation": 0.1, "hue": 0.1}}
CELEBVHQ_AUG = {"flip_param": {"horizontal_flip": True, "time_flip": True},
                "jitter_param": {"brightness": 0.1, "contrast": 0.1, "saturation": 0.1, "hue": 0.1}}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "augment_reference.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "augment_reference.npz"))


def _spec(u8: np.ndarray, params: PairParams):
    """the specification called directly: (source, driving) floats of a whole batch in ONE call"""
    descs = []
    for p in params.pairs:
        d = p.descriptor()
        descs.append((list(d.op), tuple(d.factor), d.hue_shift, d.time_flip, d.hflip))
    s, d = R.pair_augment_bytes(u8, descs)
    return torch.from_numpy(R.unit(s)), torch.from_numpy(R.unit(d))


def _pairs(name, B, H=6, W=8, C=3):
    return torch.from_numpy(R.det_bytes(name, (B, 2, H, W, C)))


# --------------------------------------------------------------------------------------------------------------------------------- the draw
def test_draw_consumes_the_generator_as_the_reference_does(golden):
    meta, _ = golden
    assert meta["augmentation_params"] == VOX1_AUG
    flips = set()
    for clip in meta["clips"]:
        random.seed(clip["seed"])
        p = PairAugmenter.from_config(VOX1_AUG).draw(1).pairs[0]
        assert (p.time_flip, p.hflip) == (clip["time_flip"], clip["hflip"]), clip["seed"]
        assert [[n, getattr(p, n)] for n in p.order] == clip["ops"], clip["seed"]          # order and factors, to the last bit
        flips.add((p.time_flip, p.hflip))
    assert flips == {(False, False), (False, True), (True, False)}                         # a time flip is never followed by a horizontal draw


def test_a_batch_draws_pair_by_pair():
    random.seed(3)
    a = PairAugmenter.from_config(VOX1_AUG).draw(4)
    random.seed(3)
    one = PairAugmenter.from_config(VOX1_AUG)
    assert a == PairParams(tuple(one.draw(1).pairs[0] for _ in range(4)))


def test_rng_keeps_the_module_generator_untouched():
    random.seed(11)
    state = random.getstate()
    a = PairAugmenter.from_config(VOX1_AUG, rng=random.Random(5)).draw(3)
    assert random.getstate() == state
    random.seed(5)
    assert a == PairAugmenter.from_config(VOX1_AUG).draw(3)
    assert a != PairAugmenter.from_config(VOX1_AUG, rng=random.Random(6)).draw(3)


def test_strength_zero_draws_nothing_and_no_params_consume_nothing():
    rng = random.Random(2)
    p = PairAugmenter(jitter_param={"brightness": 0.2, "contrast": 0, "saturation": 0, "hue": 0.05}, rng=rng).draw(1).pairs[0]
    twin = random.Random(2)
    b, h = twin.uniform(0.8, 1.2), twin.uniform(-0.05, 0.05)
    order = ["brightness", "hue"]
    twin.shuffle(order)
    assert (p.brightness, p.hue, p.contrast, p.saturation, p.order, p.time_flip, p.hflip) == (b, h, None, None, tuple(order), False, False)
    state = rng.getstate()
    assert PairAugmenter(rng=rng).draw(2) == PairParams((PairDraw(), PairDraw())) and rng.getstate() == state


def test_from_config_reads_both_training_configs():
    for cfg in (VOX1_AUG, CELEBVHQ_AUG):
        aug = PairAugmenter.from_config(cfg, rng=random.Random(0))
        assert aug.flip == {"time_flip": True, "horizontal_flip": True} and aug.jitter == {n: 0.1 for n in ("brightness", "contrast", "saturation", "hue")}
    assert mrfa_amd.PairAugmenter is PairAugmenter and mrfa_amd.PairParams is PairParams


# --------------------------------------------------------------------------------------------------------------------------------- the call
def test_outputs_equal_the_reference_transform(golden):
    """bytes exact, floats within 2^-24 of the reference's (its b / 255 in float64, cast, against ONE fp32 multiply: two roundings of one number)"""
    meta, arrays = golden
    u8 = np.stack([R.det_bytes(f"augment/reference/{c['seed']}", tuple(meta["shape"])) for c in meta["clips"]])
    params = []
    for c in meta["clips"]:
        random.seed(c["seed"])
        params.append(PairAugmenter.from_config(VOX1_AUG).draw(1).pairs[0])
    with emulated_data_hip():
        source, driving = PairAugmenter.from_config(VOX1_AUG)(torch.from_numpy(u8), PairParams(tuple(params)))
    got = torch.stack([source, driving], 1).permute(0, 1, 3, 4, 2).numpy()                 # (16, 2, H, W, 3)
    assert got.dtype == np.float32
    assert np.array_equal(np.rint(got.astype(np.float64) * 255.0).astype(np.uint8), arrays["out_bytes"])
    assert np.array_equal(got, arrays["out_bytes"].astype(np.float32) * np.float32(1.0 / 255.0))
    assert np.abs(got.astype(np.float64) - arrays["out_float"].astype(np.float64)).max() <= 2.0 ** -24


def test_hand_built_params():
    x = _pairs("augment/cpu/hand", 2)
    params = PairParams((PairDraw(time_flip=True, hflip=True, contrast=1.3, hue=-0.2, order=("hue", "contrast")), PairDraw()))
    assert params.pairs[0].hue_shift == hue_shift_of(-0.2) == 205
    with emulated_data_hip():
        source, driving = PairAugmenter()(x, params)
    u8 = x.numpy()
    want = R.contrast(R.hue(u8[0, 1], 205), 1.3)[:, ::-1]                                   # frame 1 is the source of a time-flipped pair
    assert np.array_equal(source[0].permute(1, 2, 0).numpy(), R.unit(want))
    assert np.array_equal(driving[1].permute(1, 2, 0).numpy(), R.unit(u8[1, 1])) and np.array_equal(source[1].permute(1, 2, 0).numpy(), R.unit(u8[1, 0]))
    for bad in (dict(order=("hue",)), dict(hue=0.1), dict(brightness=1.0, order=("brightness", "brightness")), dict(hue=0.6, order=("hue",)),
                dict(contrast=-0.1, order=("contrast",)), dict(saturation=float("nan"), order=("saturation",))):
        with pytest.raises(ValueError, match="PairDraw"):
            PairDraw(**bad)


def test_params_none_draws_from_the_augmenters_generator():
    x = _pairs("augment/cpu/none", 3)
    with emulated_data_hip():
        got = PairAugmenter.from_config(VOX1_AUG, rng=random.Random(8))(x)
        want = PairAugmenter.from_config(VOX1_AUG)(x, PairAugmenter.from_config(VOX1_AUG, rng=random.Random(8)).draw(3))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_a_batch_above_the_per_launch_maximum_is_split(monkeypatch):
    B = data_hip.AUG_MAX_PAIRS + 3
    x = _pairs("augment/cpu/split", B, H=3, W=4)
    aug = PairAugmenter.from_config(VOX1_AUG, rng=random.Random(1))
    params = aug.draw(B)
    with emulated_data_hip() as lib:
        calls, real = [], lib.mrfa_pair_augment
        monkeypatch.setattr(lib, "mrfa_pair_augment", lambda *a: calls.append(a[2]) or real(*a), raising=False)
        source, driving = aug(x, params)
    assert calls == [data_hip.AUG_MAX_PAIRS, 3]
    want = _spec(x.numpy(), params)
    assert torch.equal(source, want[0]) and torch.equal(driving, want[1])
    assert sorted(k[1] for k in aug._workspace) == [3, data_hip.AUG_MAX_PAIRS]              # one workspace per (B, H, W)


def test_out_is_written_in_place_and_returned():
    x = _pairs("augment/cpu/out", 2)
    aug = PairAugmenter.from_config(VOX1_AUG, rng=random.Random(4))
    params = aug.draw(2)
    out = (torch.full((2, 3, 6, 8), -7.0), torch.full((2, 3, 6, 8), -7.0))
    with emulated_data_hip():
        source, driving = aug(x, params, out=out)
    assert source is out[0] and driving is out[1]
    want = _spec(x.numpy(), params)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


def test_grey_and_alpha_frames():
    params = PairParams((PairDraw(saturation=1.5, brightness=0.8, order=("saturation", "brightness")),))
    for C in (1, 4):
        x = _pairs(f"augment/cpu/c{C}", 1, C=C)
        with emulated_data_hip():
            source, _ = PairAugmenter()(x, params)
        want = R.brightness(R.saturation(R.to_rgb(x[0, 0].numpy()), 1.5), 0.8)
        assert np.array_equal(source[0].permute(1, 2, 0).numpy(), R.unit(want))


# --------------------------------------------------------------------------------------------------------------------------------- refusals
def test_value_errors_name_what_they_got():
    aug, ok = PairAugmenter(), _pairs("augment/cpu/bad", 2)
    p2 = PairParams((PairDraw(), PairDraw()))
    with emulated_data_hip():
        for bad, says in ((ok.float(), "torch.float32"), (ok[0], "(2, 6, 8, 3)"), (ok[:, :1], "(2, 1, 6, 8, 3)"), (ok[..., :2], "(2, 2, 6, 8, 2)"),
                          (ok.numpy(), "ndarray"), (ok[:, :, :0], "(2, 2, 0, 8, 3)")):
            with pytest.raises(ValueError, match=re.escape(says)):
                aug(bad, p2)
        with pytest.raises(ValueError, match="PairParams of 2 pairs, not PairParams of 1"):
            aug(ok, PairParams((PairDraw(),)))
        with pytest.raises(ValueError, match="PairParams of 2 pairs, not dict"):
            aug(ok, {"time_flip": True})
        good = torch.empty(2, 3, 6, 8)
        for bad, says in ((torch.empty(2, 3, 6, 9), "(2, 3, 6, 9)"), (torch.empty(2, 3, 6, 8, dtype=torch.float64), "torch.float64"),
                          (torch.empty(2, 3, 8, 6).transpose(2, 3), "contiguous"), (torch.empty(2, 3, 6, 8, device="meta"), "on meta")):
            with pytest.raises(ValueError, match=re.escape(says)):
                aug(ok, p2, out=(good, bad))
            with pytest.raises(ValueError, match="source"):
                aug(ok, p2, out=(bad, good))
        with pytest.raises(ValueError, match="pair \\(source, driving\\)"):
            aug(ok, p2, out=good)
    with pytest.raises(ValueError, match="draw"):
        aug.draw(0)
    with pytest.raises(ValueError, match="jitter_param"):
        PairAugmenter(jitter_param={"gamma": 0.1})
    with pytest.raises(ValueError, match="hue at most 0.5"):
        PairAugmenter(jitter_param={"hue": 0.6})
    with pytest.raises(ValueError, match="flip_param"):
        PairAugmenter(flip_param={"vertical_flip": True})


@pytest.mark.parametrize("name", ["rotation_param", "resize_param", "crop_param"])
def test_the_other_transforms_are_not_implemented(name):
    with pytest.raises(NotImplementedError, match=name):
        PairAugmenter(**{name: {"degrees": 10}})
    with pytest.raises(NotImplementedError, match=name):
        PairAugmenter.from_config({**VOX1_AUG, name: {"size": 64}})


def test_the_specification_refuses_what_the_header_lists():
    """tests/ref_augment.Library, the CPU side of every refusal of mrfa_pair_augment: nonzero, a message, nothing written"""
    lib = R.Library()
    src = np.zeros((2, 2, 2, 4, 3), np.uint8)
    ws, out = np.zeros(2 * 2 * R.PARTS, np.uint32), [np.full(2 * 3 * 2 * 4 + 1, -7.0, np.float32) for _ in range(2)]
    descs = (R.PairAug * 2)()
    good = dict(src=src.ctypes.data, B=2, H=2, W=4, Cin=3, params=descs, workspace=ws.ctypes.data, workspace_bytes=ws.nbytes, source=out[0].ctypes.data,
                driving=out[1].ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return lib.mrfa_pair_augment(0, a["src"], a["B"], a["H"], a["W"], a["Cin"], a["params"], a["workspace"], a["workspace_bytes"], a["source"],
                                     a["driving"])

    def desc(**kw):
        d = (R.PairAug * 2)()
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                for i, e in enumerate(v):
                    getattr(d[1], k)[i] = e
            else:
                setattr(d[1], k, v)
        return d

    for d in descs:
        d.factor[:] = [1.0, 1.0, 1.0]
    assert call() == 0 and (out[0][:-1] == 0).all()
    for o in out:
        o[:] = -7.0
    bad = [dict(src=0), dict(params=None), dict(workspace=0), dict(source=0), dict(driving=0), dict(B=0), dict(H=0), dict(W=-1), dict(B=R.MAX_PAIRS + 1),
           dict(Cin=2), dict(Cin=5), dict(params=desc(op=[1, 5, 0, 0], factor=[1, 1, 1])), dict(params=desc(op=[2, 0, 2, 0], factor=[1, 1, 1])),
           dict(params=desc(factor=[1, float("inf"), 1])), dict(params=desc(factor=[1, 1, float("nan")])), dict(params=desc(factor=[-0.5, 1, 1])),
           dict(workspace_bytes=ws.nbytes - 1), dict(workspace=ws.ctypes.data + 4), dict(source=out[0].ctypes.data + 2), dict(driving=out[1].ctypes.data + 1)]
    for kw in bad:
        lib.error = b""
        assert call(**kw) != 0 and lib.mrfa_data_last_error().startswith(b"pair_augment: "), kw
        assert all((o == -7.0).all() for o in out), kw
    assert lib.mrfa_pair_augment_workspace(2, 2, 4) == ws.nbytes and lib.mrfa_pair_augment_workspace(0, 2, 4) < 0 \
        and lib.mrfa_pair_augment_workspace(R.MAX_PAIRS + 1, 2, 4) < 0 and lib.mrfa_pair_augment_workspace(1, 1 << 16, 1 << 15) < 0


# --------------------------------------------------------------------------------------------------------------------------------- data_hip.lib()
class _Entry:
    def __init__(self, value=0):
        self.value = value

    def __call__(self, *args):
        return self.value


def _stand_in(monkeypatch, version, lacks=()):
    """data_hip.lib() will load a plain object with every symbol of the binding except `lacks`, whose mrfa_data_version() returns `version`"""
    L = type("StandIn", (), {})()
    for name in data_hip._SIGNATURES:
        if name not in lacks:
            setattr(L, name, _Entry(version if name == "mrfa_data_version" else 0))
    monkeypatch.setattr(data_hip, "_lib", None)
    monkeypatch.setattr(data_hip, "LIB_PATH", os.path.abspath(__file__))
    monkeypatch.setattr(data_hip.C, "CDLL", lambda path: L)
    return L


@pytest.mark.parametrize("version", [data_hip.ABI_VERSION - 1, data_hip.ABI_VERSION + 1])
def test_lib_refuses_a_library_of_another_version(monkeypatch, version):
    _stand_in(monkeypatch, version)
    with pytest.raises(RuntimeError) as err:
        data_hip.lib()
    assert f"speaks data ABI version {version}," in str(err.value) and "rebuild the library" in str(err.value)
    assert data_hip._lib is None


@pytest.mark.parametrize("name", [n for n in data_hip._SIGNATURES if n != "mrfa_data_version"])
def test_lib_refuses_a_library_that_lacks_an_entry(monkeypatch, name):
    _stand_in(monkeypatch, data_hip.ABI_VERSION, lacks=(name,))
    with pytest.raises(AttributeError) as err:
        data_hip.lib()
    assert name in str(err.value) and data_hip._lib is None


def test_lib_accepts_the_matching_stand_in_and_a_missing_file_is_an_error(monkeypatch):
    L = _stand_in(monkeypatch, data_hip.ABI_VERSION)
    assert data_hip.lib() is L
    monkeypatch.setattr(data_hip, "_lib", None)
    monkeypatch.setattr(data_hip, "LIB_PATH", os.path.join(ROOT, "no", "such", "libmrfa_data_hip.so"))
    with pytest.raises(mrfa_amd.hip.HipLibraryMissing, match="no CPU fallback"):
        data_hip.lib()


def test_header_binding_and_specification_state_one_version_and_one_layout():
    header = open(os.path.join(ROOT, "include", "mrfa_data_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", header).group(1))

    assert define("MRFA_DATA_ABI_VERSION") == data_hip.ABI_VERSION == R.VERSION == R.Library().mrfa_data_version()
    assert define("MRFA_AUG_MAX_PAIRS") == data_hip.AUG_MAX_PAIRS == R.MAX_PAIRS and define("MRFA_AUG_PARTS") == R.PARTS
    for n in ("NONE", "BRIGHTNESS", "CONTRAST", "SATURATION", "HUE"):
        assert define("MRFA_AUG_" + n) == getattr(data_hip, "AUG_" + n) == getattr(R, n)
    import ctypes
    assert ctypes.sizeof(data_hip.PairAug) == ctypes.sizeof(R.PairAug) == 20
    assert [f[0] for f in data_hip.PairAug._fields_] == [f[0] for f in R.PairAug._fields_]
    assert set(data_hip._SIGNATURES) == {n for n in dir(R.Library) if n.startswith("mrfa_")}
    model = open(os.path.join(ROOT, "include", "mrfa_hip.h")).read()
    assert not any(re.search(rf"\b{n}\b", model) for n in data_hip._SIGNATURES)             # no name shared with the model library
    assert not set(data_hip._SIGNATURES) & set(mrfa_amd.hip._SIGNATURES)
