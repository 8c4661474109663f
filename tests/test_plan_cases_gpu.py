"""Every conv plan the model's layers get, at the smallest shape that reaches it, against float64 element by element.

The cases and their signatures are tests/test_plan_cases_cpu.py's PLAN_CASES and MORE_CASES (that module also proves, without a GPU,
that every plan of a model layer is the plan of a case).  Each case is driven through ops.conv_fwd / conv_dgrad / conv_wgrad with its operands in the
case's forms; the library is asked -- under the case's options, before the launch -- for the plan of the request, which must be the
case's signature, and the launch entry points are watched (gpu_util.conv_requests) to see that the wrapper made exactly that
request: a case that silently runs another kernel fails.  The result is held to the elementwise bound of tests/shape_ref.py, the
bound must tell every wrong problem from the right one, fused BatchNorm statistics are checked where the plan emits them, the
weight gradient also in its accumulating form, and every output starts as NaN, so no element may stay unwritten.  A bf16 case
whose feature-map operands are bf16 runs once more the way bf16 feature-map storage hands it over: bf16 tensors in, bf16 out."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import ops  # noqa: E402
from tests import shape_ref as R  # noqa: E402
from tests.gpu_util import conv_operands, conv_requests, krsc, nan_outputs, options  # noqa: E402
from tests.shape_ref import rnd  # noqa: E402
from tests.test_plan_cases_cpu import ALL_CASES, BF16, F32X3, case_id, describe, signature  # noqa: E402

OPS = ("fwd", "dgrad", "wgrad")
NAN = float("nan")


def _run(op, xg, wg, dyg, hw, stride, pad, wshape, want_stats=False):
    """The case's op through its wrapper, on outputs that start as NaN."""
    with nan_outputs():
        if op == 0:
            return ops.conv_fwd(xg, wg, stride, pad, want_stats=want_stats)
        if op == 1:
            return ops.conv_dgrad(dyg, wg, hw, stride, pad, want_stats=want_stats)
        return ops.conv_wgrad(dyg, xg, stride, pad, out=krsc(torch.full(wshape, NAN)))


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_plan_case(case):
    req, opts, want = case
    op, N, H, W, C, K, stride, pad, prec, _, a_form, b_form = req
    Ho, Wo = (H // 2, W // 2) if stride == 2 else (1, 1)
    name = OPS[op]
    what = f"{name} {case_id(case)}"
    x = rnd(N, C, H, W, seed=1) if op != 1 else None
    w = rnd(K, C, 4, 4, seed=2, scale=1.0 / math.sqrt(16 * C)) if op != 2 else None
    dy = rnd(N, K, Ho, Wo, seed=3) if op != 0 else None
    a, b = ((x, w), (dy, w), (x, dy))[op]                        # conv_ref's operand order
    used = want[1]                                               # the arithmetic the plan really runs
    opnd = R.r16 if used == BF16 else R.f64
    mult = 8 if used == F32X3 else 1
    n = R.taps(name, C, K, stride=stride, nz_rows=N * Ho * Wo)
    wshape = (K, C, 4, 4)
    args = ((H, W), stride, pad, wshape)
    # the GEMM's operands: A = x, B = w (forward); A = dy, B = w (input gradient); A = dy, B = x (weight gradient)
    x_form, dy_form, w_form = (a_form if op == 0 else b_form), a_form, b_form
    ctx = ops.Context(prec=prec, shadow=prec == BF16 and bool(a_form or b_form), x3=a_form == 3)
    stats = acc = preset = got16 = None
    with options(**opts), ops.use(ctx):
        f = describe(req)
        assert f is not None and signature(f) == want, f"{what}: the library plans {f}"
        xg, wg, dyg = conv_operands(x, w, dy, shadow_x=x_form == 1, shadow_dy=dy_form == 1, shadow_w=w_form == 1)
        with conv_requests() as asked:
            got = _run(op, xg, wg, dyg, *args)
        assert asked == [req], f"{what}: the wrapper asked for {asked}"
        assert got.dtype == torch.float32
        if f["stat_rows"] > 0:                                   # the trainer asks these forms for fused BatchNorm statistics
            again, st = _run(op, xg, wg, dyg, *args, want_stats=True)
            ch = K if op == 0 else C
            assert st is not None and tuple(st.shape) == (f["stat_rows"], 3 * ch + 4), f"{what}: statistics rows {None if st is None else tuple(st.shape)}"
            stats = ops.bn_stats_from_partials(st, again, None, None, None, 1e-5, 0.1)
            assert torch.equal(again, got), f"{what}: the output changes when statistics are asked for"
        if op == 2:
            preset = rnd(*wshape, seed=4, scale=0.5)
            acc = ops.conv_wgrad(dyg, xg, stride, pad, out=krsc(preset), accumulate=True)
        torch.cuda.synchronize()
    # bf16 feature-map storage: the same request with the feature-map operands as bf16 tensors and (where the output is a feature
    # map of a multiple of 8 channels) a bf16 output
    if prec == BF16 and all(form == 1 for t, form in ((x, x_form), (dy, dy_form)) if t is not None):
        ctx16 = ops.Context(prec=prec, shadow=True, act16=True)
        with options(**opts), ops.use(ctx16):
            xg, wg, dyg = conv_operands(x, w, dy, act16=True, shadow_w=w_form == 1)
            with conv_requests() as asked:
                got16 = _run(op, xg, wg, dyg, *args)
            assert asked == [req], f"{what}: with bf16 feature maps the wrapper asked for {asked}"
            assert (got16.dtype == torch.bfloat16) == (op != 2 and (K, C)[op] % 8 == 0), f"{what}: output type {got16.dtype}"
            torch.cuda.synchronize()
    ref, absref = R.conv_ref(name, opnd(a), opnd(b), stride=stride, pad=pad, wshape=wshape)
    R.assert_within(got, ref, absref, n, what, mult=mult)
    for wa, wb in R.wrong_problems(name, opnd(a), opnd(b)):
        wrong, _ = R.conv_ref(name, wa, wb, stride=stride, pad=pad, wshape=wshape)
        R.assert_discriminates(wrong, ref, absref, n, what, mult=mult)
        if got16 is not None:
            R.assert_discriminates(wrong, ref, absref, n, what + " bf16 maps", mult=mult, out16=got16.dtype == torch.bfloat16)
    if got16 is not None:
        R.assert_within(got16, ref, absref, n, what + " bf16 maps", mult=mult, out16=got16.dtype == torch.bfloat16)
    if acc is not None:
        R.assert_within(acc, ref + R.f64(preset), absref + R.f64(preset).abs(), n + 1, what + " accumulate", mult=mult)
    if stats is not None:
        M = ref.numel() // ref.shape[1]
        mean, var = ref.mean((0, 2, 3)), ref.var((0, 2, 3), unbiased=False)
        sc, tol = mean.abs() + var.sqrt(), R.bn_tol(M)
        assert R.bn_violations(stats[0], mean, sc, tol) == 0, f"{what}: mean"
        assert R.bn_violations(1.0 / stats[1].double() ** 2 - 1e-5, var, var, tol) == 0, f"{what}: variance"
        assert R.bn_violations(torch.roll(mean, 1), mean, sc, tol) > 0 and R.bn_violations(torch.roll(var, 1), var, var, tol) > 0, \
            f"{what}: statistics bound vacuous"
