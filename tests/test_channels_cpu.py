"""Host-side halves of tests/test_channels_gpu.py (no GPU needed): every conv plan query over channel counts the model never
makes -- none may fail, whatever the argument tuple --, what the queries answer for shapes the launch entry points refuse, and the
discrimination of the fp64 error bound at ragged channel counts (channel rotations beside the one-pixel shifts)."""
import ctypes
import json
import math
import os

import pytest
import torch

from discogan_modernized_amd import _lib, model, ops
from tests import shape_ref as R

OPS = (0, 1, 2)                                            # forward, input gradient, weight gradient
GEOMS = ((2, 1), (1, 0))                                   # (stride, pad): the stride-2 layers, the 4 x 4 heads
SWEEP_C = (4, 8, 12, 32, 36, 60, 64, 68, 96, 100, 128, 132, 160, 192, 200, 224, 320, 2048)
SWEEP_K = (1, 4, 8, 12, 20, 32, 36, 64, 96, 100, 132, 160, 200, 288, 2048)
SWEEP_N = (1, 3, 13)


def refused(op, C, K, stride):
    """Does the launch entry point of `op` refuse the channel counts?  (include/discogan_hip.h, "Shapes without a plan")"""
    if C % 4 != 0 or not (K == 1 or K % 4 == 0):
        return True
    if K == 1:
        return stride != 1                                 # the K == 1 form exists for the 4 x 4 head only
    return (op == 0 and C % 32 != 0) or (op == 1 and stride == 2 and K % 32 != 0)


def all_queries(L, op, N, H, C, K, stride, pad, prec, pg):
    """Every plan query of one shape: dict name -> answer.  The forms without a precision argument read the process default, which
    the caller has set to `prec`."""
    g = (op, N, H, H, C, K, stride, pad)
    return dict(ws=L.dg_conv_workspace_bytes(*g), ws_p=L.dg_conv_workspace_bytes_p(*g, prec, pg),
                splits=L.dg_conv_plan_splits(*g), splits_p=L.dg_conv_plan_splits_p(*g, prec, pg),
                rows=L.dg_conv_bnstats_rows(*g), rows_p=L.dg_conv_bnstats_rows_p(*g, prec),
                bf16_ok=L.dg_conv_bf16_operands_ok(*g), x3_ok=L.dg_conv_x3_planes_ok(*g), x3_rows=L.dg_conv_x3_bnstats_rows(*g),
                mixed_rows=[L.dg_conv_mixed_bnstats_rows(*g, a16, b16) for a16 in (0, 1) for b16 in (0, 1)])


def sweep(stride, pad, kts=(0, 16, 32), precs=(0, 1, 2), ops_=OPS, Cs=SWEEP_C, Ks=SWEEP_K):
    """Run the queries over the sweep of one geometry; returns the number of shapes asked.  Options are put back however it ends."""
    L = _lib.load()
    asked = 0
    try:
        for kt in kts:
            _lib.set_option("kt", kt)
            for prec in precs:
                _lib.set_option("bf16", prec)
                for op in ops_:
                    for C in Cs:
                        for K in Ks:
                            for N in SWEEP_N:
                                for H in ((2, 8, 64) if stride == 2 else (4,)):
                                    for pg in (1, 4):
                                        q = all_queries(L, op, N, H, C, K, stride, pad, prec, pg)
                                        asked += 1
                                        what = f"op {op} N {N} H {H} C {C} K {K} stride {stride} kt {kt} prec {prec} plan_groups {pg}: {q}"
                                        assert q["splits"] >= 1 and q["splits_p"] >= 1, what
                                        # (the converse does not hold: the workspace covers the bf16-operand and plane forms' plans too)
                                        assert (q["ws"] > 0 or q["splits"] == 1) and (q["ws_p"] > 0 or q["splits_p"] == 1), what
                                        assert min(q["rows"], q["rows_p"], q["x3_rows"], *q["mixed_rows"]) >= 0, what
                                        assert q["bf16_ok"] in (0, 1, 2) and q["x3_ok"] in (0, 1, 2, 3, 4), what
                                        if refused(op, C, K, stride) or K == 1:
                                            # no plan: nothing to allocate, nothing fused, no bf16 / plane kernel
                                            assert (q["ws"], q["ws_p"], q["splits"], q["splits_p"]) == (0, 0, 1, 1), what
                                            assert (q["rows"], q["rows_p"], q["x3_rows"], q["bf16_ok"], q["x3_ok"]) == (0, 0, 0, 0, 0), what
                                            assert q["mixed_rows"] == [0, 0, 0, 0], what
                                        if op == 2 or stride != 2:
                                            assert (q["rows"], q["rows_p"], q["x3_rows"]) == (0, 0, 0) and q["mixed_rows"] == [0, 0, 0, 0], what
    finally:
        _lib.set_option("kt", 0)
        _lib.set_option("bf16", 0)
    return asked


@pytest.mark.parametrize("stride,pad", GEOMS)
def test_plan_queries_return_for_every_channel_count(stride, pad):
    """All nine plan queries over op x C x K x N x H x option kt x arithmetic x plan_groups: every one returns (a stride-2 input
    gradient with K = 4 and C > 64 used to divide by zero in make_plan and kill the process), splits >= 1, a workspace wherever
    K is split, and for a refused shape or the K == 1 head the documented "nothing"."""
    n = sweep(stride, pad)
    assert n == 3 * 3 * 3 * len(SWEEP_C) * len(SWEEP_K) * len(SWEEP_N) * (3 if stride == 2 else 1) * 2


def test_plan_queries_answer_nothing_for_bad_arguments():
    """Arguments no sweep of supported geometry contains: an op outside 0..2, C % 4 != 0, K = 6, a 5 x 5 image, an unknown
    (stride, pad), N = 0."""
    L = _lib.load()
    for op, N, H, C, K, stride, pad in ((3, 2, 8, 64, 64, 2, 1), (-1, 2, 8, 64, 64, 2, 1), (0, 2, 8, 30, 64, 2, 1), (1, 2, 8, 64, 6, 2, 1),
                                        (2, 2, 5, 64, 64, 2, 1), (0, 2, 8, 64, 64, 3, 1), (1, 0, 8, 64, 64, 2, 1), (1, 2, 8, 0, 32, 2, 1),
                                        (1, 2, 8, 96, 0, 2, 1)):
        for prec in (0, 1, 2):
            q = all_queries(L, op, N, H, C, K, stride, pad, prec, 1)
            assert (q["ws"], q["ws_p"], q["splits"], q["splits_p"]) == (0, 0, 1, 1), (op, N, H, C, K, stride, pad, q)
            assert (q["rows"], q["rows_p"], q["x3_rows"], q["bf16_ok"], q["x3_ok"]) == (0, 0, 0, 0, 0), (op, N, H, C, K, stride, pad, q)


def test_refused_input_gradient_is_refused_not_planned():
    """(N 2, 8 x 8, C 96, K 4): the stride-2 input gradient takes K % 32 == 0.  The queries answer "nothing" and the launch entry
    points refuse with a message (non-null dummies: validation fails before they are dereferenced or anything is launched)."""
    L = _lib.load()
    assert L.dg_conv_workspace_bytes_p(1, 2, 8, 8, 96, 4, 2, 1, 0, 1) == 0
    assert L.dg_conv_plan_splits_p(1, 2, 8, 8, 96, 4, 2, 1, 0, 1) == 1
    d = ctypes.c_void_p(8)
    tab = (ctypes.c_void_p * 2)(8, 8)
    assert L.dg_conv_dgrad(d, d, d, 2, 8, 8, 96, 4, 2, 1, None, 0, None) < 0
    assert b"multiple of 32" in L.dg_last_error()
    assert L.dg_conv_dgrad_g(2, tab, tab, tab, 2, 8, 8, 96, 4, 2, 1, 0, 1, None, 0, tab, 0, None) < 0
    assert b"multiple of 32" in L.dg_last_error()
    assert L.dg_conv_dgrad_mixed(d, 0, d, 1, d, 0, 2, 8, 8, 96, 4, 2, 1, None, 0, None, 0, None) < 0
    assert b"multiple of 32" in L.dg_last_error()
    assert L.dg_conv_dgrad_bias_act(d, d, None, d, 2, 8, 8, 96, 4, 2, 1, ops.ACT_RELU, 0.0, None, 0, None) < 0
    assert b"multiple of 32" in L.dg_last_error()
    # the forward's rule, and the plane forms apply the same ones
    assert L.dg_conv_fwd(d, d, d, 2, 8, 8, 48, 64, 2, 1, None, 0, None) < 0 and b"multiple of 32" in L.dg_last_error()
    assert L.dg_conv_fwd_x3(d, 1 << 20, d, 1 << 20, 0, d, 16, 8, 8, 48, 192, 2, 1, None, 0, None, 0, None) < 0
    assert b"multiple of 32" in L.dg_last_error()
    # a bf16 x of the weight gradient: 8-element granules must not straddle a tap
    assert L.dg_conv_wgrad_mixed(d, 0, d, 1, d, 3, 8, 8, 36, 100, 2, 1, 0, None, 0, None) < 0 and b"C % 8" in L.dg_last_error()


PLAN_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_table.json")
PLAN_COLUMNS = ("ws", "ws_p", "splits", "splits_p", "rows", "rows_p", "bf16_ok", "x3_ok", "x3_rows", "mixed_rows")


def plan_table_shapes():
    """(N, H, C, K, stride, pad) of the table: every interior conv layer of the generators and discriminators (model.py: the
    stride-2 stages behind the 3-channel one -- a decoder stage is the input gradient of the same geometry --, the generator's
    100-channel bottleneck and the discriminator's K = 1 head) at 64 px with N 64 and 256 and at 512 px with N 32, and an off-model
    grid."""
    shapes = []
    for size, N in ((64, 64), (64, 256), (512, 32)):
        ch = model.stage_channels(size)
        shapes += [(N, size >> i, ch[i - 1], ch[i], 2, 1) for i in range(1, len(ch))]
        shapes += [(N, 4, ch[-1], 100, 1, 0), (N, 4, ch[-1], 1, 1, 0)]
    for C in (32, 96, 128, 192, 320):
        shapes += [(3, H, C, K, 2, 1) for K in (4, 32, 64, 100, 160, 288) for H in (8, 64)]
        shapes += [(3, 4, C, K, 1, 0) for K in (1, 32)]
    return shapes


def plan_table_rows(L):
    """One row of PLAN_COLUMNS per shape x op x arithmetic x plan_groups, in that order, from the library L (option "kt" 0)."""
    rows = []
    try:
        for N, H, C, K, stride, pad in plan_table_shapes():
            for op in OPS:
                for prec in (0, 1, 2):
                    _lib.set_option("bf16", prec)
                    for pg in (1, 4):
                        q = all_queries(L, op, N, H, C, K, stride, pad, prec, pg)
                        rows.append([q[c] for c in PLAN_COLUMNS])
    finally:
        _lib.set_option("bf16", 0)
    return rows


def test_plans_match_the_recorded_table():
    """tests/golden/conv_plan_table.json holds what every plan query answered before the host layer was given one launch path and one
    query helper (written by tests/golden/make_conv_plan_table.py from the library of the commit before): workspace bytes, K-splits,
    statistics rows and the bf16 / plane kernel codes of the model's layers and of an off-model grid, per op, arithmetic and
    plan_groups.  The planner reads no device property, so the table holds on any machine; a change of plan is a change of
    speed or of summation order and must be made on purpose, with the table regenerated."""
    with open(PLAN_TABLE) as f:
        table = json.load(f)
    assert table["columns"] == list(PLAN_COLUMNS)
    assert [tuple(s) for s in table["shapes"]] == plan_table_shapes()
    rows = plan_table_rows(_lib.load())
    assert len(rows) == len(table["rows"]) == len(plan_table_shapes()) * 3 * 3 * 2
    it = iter(zip(rows, table["rows"]))
    for shape in plan_table_shapes():
        for op in OPS:
            for prec in (0, 1, 2):
                for pg in (1, 4):
                    got, want = next(it)
                    assert got == want, f"(N, H, C, K, stride, pad) {shape} op {op} arithmetic {prec} plan_groups {pg}: {PLAN_COLUMNS}"


OPNAMES = ("fwd", "dgrad", "wgrad")


def test_error_bound_catches_rotated_channels_at_ragged_counts():
    """(N 3, C 96, K 100, 16 x 16): an fp32 evaluation of each op stays inside shape_ref's bound, while the float64 references of the
    wrong problems violate it -- the one-pixel shifts and both channel rotations (output channels: what a kernel that mis-indexes
    the ragged column tile computes; input channels: a K-tile paired with the wrong channels)."""
    N, C, K, H = 3, 96, 100, 16
    x, w, dy = R.rnd(N, C, H, H, seed=1), R.rnd(K, C, 4, 4, seed=2, scale=1.0 / math.sqrt(16 * C)), R.rnd(N, K, H // 2, H // 2, seed=3)
    TF = torch.nn.functional
    got = dict(fwd=TF.conv2d(x, w, stride=2, padding=1), dgrad=TF.conv_transpose2d(dy, w, stride=2, padding=1),
               wgrad=torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=2, padding=1))
    for op, a, b, n in (("fwd", x, w, R.taps("fwd", C, K)), ("dgrad", dy, w, R.taps("dgrad", C, K)), ("wgrad", x, dy, N * (H // 2) ** 2)):
        ref, absref = R.conv_ref(op, a, b, wshape=w.shape)
        R.assert_within(got[op], ref, absref, n, f"fp32 CPU {op}")
        wrongs = R.wrong_problems(op, R.f64(a), R.f64(b))
        assert len(wrongs) == 4
        for wa, wb in wrongs:
            wrong = R.conv_ref(op, wa, wb, wshape=w.shape)[0]
            assert R.violations(wrong, ref, absref, n) > 0.5 * ref.numel(), op
            with pytest.raises(AssertionError, match="past the bound"):
                R.assert_within(wrong, ref, absref, n, "wrong problem")
    # the two rotations of the weight, as named functions
    ref, absref = R.conv_ref("fwd", x, w)
    for rot in (R.rot_out, R.rot_in):
        assert torch.equal(rot(rot(w)), torch.roll(w, 2, dims=0 if rot is R.rot_out else 1))
        R.assert_discriminates(R.conv_ref("fwd", x, rot(w))[0], ref, absref, 16 * C, "rotated weight")
    # the head's input gradient sums K products per element
    assert R.taps("dgrad", 96, 100, stride=1) == 100 and R.taps("dgrad", 96, 160) == 640
