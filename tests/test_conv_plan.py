"""The convolution capability queries answer from the launch plan (csrc/conv_plan.hip): a decision table recorded from the library before the plan
existed (tools/conv_plan_table.py -> tests/golden/conv_plan_table.npz) pins every answer.  The queries dereference none of the block's pointers,
so this runs without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from mrfa_amd.hip import ConvParams, WgradParams, tuned

BASE = 1 << 32          # tools/conv_plan_table.py: pointer field i of a block sits at BASE + i * 4 KiB + its stored offset


@pytest.fixture(scope="module")
def table(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "conv_plan_table.npz")))


@pytest.fixture(scope="module")
def lib():
    from mrfa_amd.build import build
    L = C.CDLL(build(verbose=False))
    L.mrfa_set_tuning.argtypes = [C.c_char_p, C.c_int]
    mode = L.mrfa_get_mfma_mode()
    yield L
    L.mrfa_set_mfma_mode(mode)


def _block(struct, ptr_names, ptrs, val_names, vals):
    p = struct()
    all_ptrs = [n for n, t in struct._fields_ if t is C.c_void_p]
    for n, v in zip(ptr_names, ptrs):
        setattr(p, n, None if v < 0 else BASE + all_ptrs.index(n) * 4096 + int(v))
    for n, v in zip(val_names, vals):
        setattr(p, n, float(v) if n in ("alpha", "fin_momentum", "fin_eps") else int(v))
    return p


def _answers(L, t, kind, struct):
    queries = [str(q) for q in t[f"{kind}_queries"]]
    fns = [getattr(L, "mrfa_conv2d_" + q) for q in queries]
    for f in fns:
        f.argtypes = [C.POINTER(struct)]
    ptr_names, val_names = [str(n) for n in t[f"{kind}_ptr_fields"]], [str(n) for n in t[f"{kind}_val_fields"]]
    got = np.zeros_like(t[f"{kind}_answers"])
    for ti, tuning in enumerate(str(s) for s in t["tunings"]):
        key, _, value = tuning.partition("=")
        with tuned(L, **({key: int(value)} if key else {})):
            for mode in range(4):
                assert L.mrfa_set_mfma_mode(mode) == 0
                for i in np.nonzero((t[f"{kind}_tuning"] == ti) & (t[f"{kind}_mode"] == mode))[0]:
                    p = _block(struct, ptr_names, t[f"{kind}_ptrs"][i], val_names, t[f"{kind}_vals"][i])
                    got[i] = [f(C.byref(p)) for f in fns]
    return queries, got


def _mismatches(t, kind, queries, got, want):
    bad = np.argwhere(got != want)
    return [f"row {i} ({queries[j]}, mode {t[f'{kind}_mode'][i]}, tuning {t['tunings'][t[f'{kind}_tuning'][i]]!r}): {got[i, j]} != {want[i, j]}"
            for i, j in bad[:10]]


def test_conv_queries_match_the_table(lib, table):
    queries, got = _answers(lib, table, "conv", ConvParams)
    assert not _mismatches(table, "conv", queries, got, table["conv_answers"])


def test_wgrad_queries_match_the_table(lib, table):
    queries, got = _answers(lib, table, "wgrad", WgradParams)
    want = table["wgrad_answers"].copy()
    # The one recorded answer that changes: with the `conv_small` switch off the weight-gradient dispatch has no strided kernel, but the recorded
    # mrfa_conv2d_wgrad_stride_supported still said yes (it asked the small kernel's eligibility alone) and the launch then refused stride 2.
    drift = (table["wgrad_tuning"] == list(table["tunings"]).index("conv_small=0")) & (want[:, queries.index("wgrad_stride_supported")] == 1)
    assert drift.any()
    want[drift, queries.index("wgrad_stride_supported")] = 0
    assert not _mismatches(table, "wgrad", queries, got, want)


# ---- hip.tuned: the one way to flip a mrfa_set_tuning key and put it back
KEYS = ["conv_small", "conv_halo", "conv_halo_min_tiles", "conv_halo_pr", "conv_halo_phase", "conv_halo_bn256", "conv_halo_bn192", "conv_halo_bn64_fill",
        "conv_lean", "conv_lean_min_wgs", "conv_lean_geo", "gemm_lean", "wgrad_halo", "wgrad_halo_min_wgs", "wgrad_halo_target_wgs", "wgrad_halo_phase",
        "wgrad_lean", "conv_fewout3", "attention_mfma"]


def _state(L):
    """every key's stored value (a key is read by setting it and putting back what the call returned)"""
    out = {}
    for k in KEYS:
        out[k] = L.mrfa_set_tuning(k.encode(), 0)
        L.mrfa_set_tuning(k.encode(), out[k])
    return out


def test_tuning_defaults_are_constants(lib):
    s = _state(lib)
    assert s == {**{k: 1 for k in KEYS}, "conv_halo_min_tiles": 128, "conv_halo_pr": 0, "conv_lean_min_wgs": 128, "conv_lean_geo": -1,
                 "wgrad_halo_min_wgs": 192, "wgrad_halo_target_wgs": 256}


def test_tuned_restores_the_previous_values_after_the_body_raises(lib):
    before = _state(lib)
    lib.mrfa_set_tuning(b"conv_halo_min_tiles", 77)           # (not the default: what is restored is what was there)
    try:
        with pytest.raises(ZeroDivisionError):
            with tuned(lib, conv_halo_min_tiles=3, conv_small=0, gemm_lean=2):
                assert _state(lib) == {**before, "conv_halo_min_tiles": 3, "conv_small": 0, "gemm_lean": 2}
                1 / 0
        assert _state(lib) == {**before, "conv_halo_min_tiles": 77}
    finally:
        lib.mrfa_set_tuning(b"conv_halo_min_tiles", before["conv_halo_min_tiles"])


def test_nested_tuned_blocks_unwind_in_order(lib):
    before = _state(lib)
    with tuned(lib, wgrad_halo_min_wgs=1, wgrad_halo=0):
        with tuned(lib, wgrad_halo_min_wgs=5, wgrad_halo_phase=0):
            assert _state(lib) == {**before, "wgrad_halo_min_wgs": 5, "wgrad_halo": 0, "wgrad_halo_phase": 0}
        assert _state(lib) == {**before, "wgrad_halo_min_wgs": 1, "wgrad_halo": 0}
        with tuned(lib, wgrad_halo_min_wgs=9):                # a second block on a key the outer one holds
            assert _state(lib)["wgrad_halo_min_wgs"] == 9
        assert _state(lib) == {**before, "wgrad_halo_min_wgs": 1, "wgrad_halo": 0}
    assert _state(lib) == before


def test_tuned_refuses_an_unknown_key_and_changes_nothing(lib):
    before = _state(lib)
    ran = []
    with pytest.raises(KeyError, match="conv_hallo"):
        with tuned(lib, conv_small=0, conv_lean_geo=3, conv_hallo=0, conv_lean=0):
            ran.append(1)
    assert not ran and _state(lib) == before


def test_conv_lean_geo_round_trips_through_minus_one(lib):
    assert _state(lib)["conv_lean_geo"] == -1
    with tuned(lib, conv_lean_geo=5):
        assert _state(lib)["conv_lean_geo"] == 5
        with tuned(lib, conv_lean_geo=-1):
            assert _state(lib)["conv_lean_geo"] == -1
        assert _state(lib)["conv_lean_geo"] == 5
    assert _state(lib)["conv_lean_geo"] == -1


def test_the_libraries_read_no_environment():
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mrfa_amd")
    seen = 0
    for sub in ("csrc", "csrc_data"):
        for f in sorted(os.listdir(os.path.join(pkg, sub))):
            seen += 1
            assert "getenv" not in open(os.path.join(pkg, sub, f)).read(), f"{sub}/{f} reads the environment"
    assert seen > 30
