"""``coocc_conv_wgrad_h2t`` (csrc/wgrad_h2t.hip, the split-f16 weight gradient over a row table) without a GPU: the entry is
exported and declared the same way in the header and in ``_lib.SIGNATURES``, it refuses bad arguments with COOCC_EINVAL before any
launch or HIP call, and the rule-book generator of tests/test_gpu_sparse_wgrad_h2t.py has the properties that file relies on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from co_occ_amd import _lib

import wgrad_h2t_cases as W

NAME = "coocc_conv_wgrad_h2t"
P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def test_entry_is_exported_and_the_ctypes_row_agrees_with_the_header():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libcoocc_hip.so not built: run __graft_entry__.build()")
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "missing export " + NAME
    src = open(os.path.join(ROOT, "include", "coocc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, src)
    assert m, "include/coocc_hip.h does not declare " + NAME
    want = []
    for arg in m.group(1).split(","):
        arg = arg.strip()
        want.append(P if "*" in arg else (L if arg.startswith("int64_t") else I))
    res, args = _lib.SIGNATURES[NAME]
    assert res is I and list(args) == want, "ctypes row %r, header %r" % (args, want)


def test_entry_validates_before_launching():
    """In the manner of tests/test_abi.py: COOCC_EINVAL (-1) and a message naming the entry, with no GPU present."""
    lib = _lib.load()
    one = ctypes.c_void_p(16)          # a non-null, 16-byte aligned dummy address: validation never dereferences device pointers
    taps, Cin, Cout, M = 27, 32, 64, 100
    per = taps * Cin * Cout

    def rc(in_=one, table=one, M=M, Cin=Cin, Cout=Cout, ws_floats=per, in_rows=120, dacc=one, dw=one, ws=one):
        return lib.coocc_conv_wgrad_h2t(in_, in_rows, Cin, dacc, Cout, table, M, Cin, Cout, taps, None, dw, 0, ws, ws_floats, None)
    for what, kw in [("a null in", dict(in_=None)), ("Cin = 16", dict(Cin=16, ws_floats=1 << 30)), ("Cout = 48", dict(Cout=48, ws_floats=1 << 30)),
                     ("M = 0", dict(M=0)), ("a null table", dict(table=None)), ("a workspace one float short", dict(ws_floats=per - 1)),
                     ("a null dacc", dict(dacc=None)), ("a null dw", dict(dw=None)), ("a null workspace", dict(ws=None)),
                     ("an operand of 4 GB", dict(in_rows=1 << 25))]:
        assert rc(**kw) == -1, what
        assert b"conv_wgrad_h2t" in lib.coocc_last_error(), what


@pytest.mark.parametrize("taps", [1, 27])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 33, 300, 4099, 60000])
def test_rule_book_generator_has_the_cases_it_claims(taps, M):
    in_rows = M + 37
    tb = W.book(taps, M, in_rows, seed=5)
    assert tb.dtype == np.int32 and tb.shape == (taps, M) and tb.min() >= -1 and tb.max() < in_rows
    assert np.array_equal(tb, W.book(taps, M, in_rows, seed=5)), "seeded"
    dt, run = W.dead_tap(taps), W.dead_run(M)
    assert (dt is None) == (taps == 1) and (run is None) == (M < 32)
    if dt is not None:
        assert (tb[dt] == -1).all(), "one tap is all -1"
    if run is not None:
        assert run[0] % 16 == 0 and run[1] == run[0] + 16 and run[1] <= M and (tb[:, run[0]:run[1]] == -1).all(), "an aligned dead 16-row run"
    for t in range(taps):
        if t != dt:
            assert (tb[t] >= 0).any(), "tap %d has live entries" % t
    if M >= 4099:
        live = (np.delete(tb, dt, 0) if dt is not None else tb) >= 0
        assert 0.25 < live.mean() < 0.35, "about 30 %% live: %.3f" % live.mean()
    x = torch.arange(in_rows * 2, dtype=torch.float64).view(in_rows, 2) + 1
    gx = W.gathered(x, tb[0])
    assert ((gx[:, 0] == 0).numpy() == (tb[0] < 0)).all() and (gx[tb[0] >= 0, 0].numpy() == 2 * tb[0][tb[0] >= 0] + 1).all()
