"""The convolution capability queries answer from the launch plan (csrc/conv_plan.hip): a decision table recorded from the library before the plan
existed (tools/conv_plan_table.py -> tests/golden/conv_plan_table.npz) pins every answer.  The queries dereference none of the block's pointers,
so this runs without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from mrfa_amd.hip import ConvParams, WgradParams

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
        prev = L.mrfa_set_tuning(key.encode(), int(value)) if key else None
        try:
            for mode in range(4):
                assert L.mrfa_set_mfma_mode(mode) == 0
                for i in np.nonzero((t[f"{kind}_tuning"] == ti) & (t[f"{kind}_mode"] == mode))[0]:
                    p = _block(struct, ptr_names, t[f"{kind}_ptrs"][i], val_names, t[f"{kind}_vals"][i])
                    got[i] = [f(C.byref(p)) for f in fns]
        finally:
            if key:
                L.mrfa_set_tuning(key.encode(), prev)
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
