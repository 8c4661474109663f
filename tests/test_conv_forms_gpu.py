"""The entry-point forms of one conv op agree bitwise.

A forward, input gradient or weight gradient can be asked for through the plain form (dg_conv_fwd / _dgrad / _wgrad), its named
wrappers (dg_conv4x4s2_* / dg_conv4x4_valid_*, and dg_convT4x4s2_* / dg_convT4x4_1to4_* with the roles swapped), the grouped form
with one problem and the default arithmetic, and the bf16-operand form with every bf16 flag off.  All of them are the same
validation, plan and launch, so their outputs are bitwise equal -- under each process arithmetic, with the default split plan and
with K-splitting forced off -- and the fused-statistics form writes the output and the statistics rows that the grouped form
writes when it is handed a statistics buffer.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, ops  # noqa: E402

DEV = "cuda"
# (N, H, C, K, stride, pad): a stride-2 layer, the 4 x 4 head with 32 outputs and with one (plain reductions, no plan)
GEOMS = ((2, 8, 64, 64, 2, 1), (4, 4, 64, 32, 1, 0), (4, 4, 64, 1, 1, 0))
FILL = float("nan")                                        # outputs start as NaN: an element no kernel wrote is never "equal"


def rnd(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, generator=g) * 2 - 1) * scale).to(DEV)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def tab(t):
    return (ctypes.c_void_p * 1)(t.data_ptr() if t is not None else None)


def forms(L, op, geom, a, b, out_numel, ws, wsb, st):
    """name -> output of every form of `op` at `geom`; a / b are the op's operands in the plain form's order."""
    N, H, C, K, stride, pad = geom
    g = (N, H, H, C, K, stride, pad)
    acc = (0,) if op == 2 else ()
    s2 = stride == 2
    plain = ("dg_conv_fwd", "dg_conv_dgrad", "dg_conv_wgrad")[op]
    named = (("dg_conv4x4s2_fwd", "dg_conv4x4s2_dgrad", "dg_conv4x4s2_wgrad") if s2 else
             ("dg_conv4x4_valid_fwd", "dg_conv4x4_valid_dgrad", "dg_conv4x4_valid_wgrad"))[op]
    # ConvTranspose2d(Cin = K, Cout = C): its forward is this input gradient, its input gradient this forward, and its weight
    # gradient this weight gradient with (dy, x) swapped
    transposed = (("dg_convT4x4s2_dgrad", "dg_convT4x4s2_fwd", "dg_convT4x4s2_wgrad") if s2 else
                  ("dg_convT4x4_1to4_dgrad", "dg_convT4x4_1to4_fwd", "dg_convT4x4_1to4_wgrad"))[op]
    ta, tb = (b, a) if op == 2 else (a, b)
    calls = {
        plain: lambda o: getattr(L, plain)(ptr(a), ptr(b), ptr(o), *g, *acc, ptr(ws), wsb, st),
        named: lambda o: getattr(L, named)(ptr(a), ptr(b), ptr(o), *((N, H, H, C, K) if s2 else (N, C, K)), *acc, ptr(ws), wsb, st),
        transposed: lambda o: getattr(L, transposed)(ptr(ta), ptr(tb), ptr(o), *((N, H // 2, H // 2, K, C) if s2 else (N, K, C)), *acc,
                                                      ptr(ws), wsb, st),
        plain + "_g": lambda o: (getattr(L, plain + "_g")(1, 1, tab(a), tab(b), tab(o), *g, ops.PREC_DEFAULT, 1, 0, tab(ws), wsb, st) if op == 2 else
                                 getattr(L, plain + "_g")(1, tab(a), tab(b), tab(o), *g, ops.PREC_DEFAULT, 1, None, 0, tab(ws), wsb, st)),
        plain + "_mixed": lambda o: (getattr(L, plain + "_mixed")(ptr(a), 0, ptr(b), 0, ptr(o), *g, 0, ptr(ws), wsb, st) if op == 2 else
                                     getattr(L, plain + "_mixed")(ptr(a), 0, ptr(b), 0, ptr(o), 0, *g, None, 0, ptr(ws), wsb, st)),
    }
    outs = {}
    for name, call in calls.items():
        o = torch.full((out_numel,), FILL, device=DEV)
        rc = call(o)
        assert rc == 0, (name, geom, L.dg_last_error())
        outs[name] = o
    return outs


@pytest.mark.parametrize("splitk", [0, 1], ids=["default_split", "unsplit"])
@pytest.mark.parametrize("prec", [0, 1, 2], ids=["f32", "bf16", "f32x3"])
def test_forms_of_one_op_agree_bitwise(prec, splitk):
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    try:
        _lib.set_option("bf16", prec)
        _lib.set_option("splitk", splitk)
        for geom in GEOMS:
            N, H, C, K, stride, pad = geom
            Ho = H // 2 if stride == 2 else 1
            x, w, dy = rnd(N * H * H * C, 1), rnd(K * 16 * C, 2, 0.05), rnd(N * Ho * Ho * K, 3)
            for op, (a, b, out_numel) in enumerate(((x, w, dy.numel()), (dy, w, x.numel()), (dy, x, w.numel()))):
                g = (op, N, H, H, C, K, stride, pad)
                wsb = L.dg_conv_workspace_bytes(*g)
                ws = torch.empty(max(wsb, 4) // 4, device=DEV) if wsb else None
                outs = forms(L, op, geom, a, b, out_numel, ws, wsb, st)
                torch.cuda.synchronize()
                names = list(outs)
                assert not torch.isnan(outs[names[0]]).any(), (names[0], geom, "elements left unwritten")
                for name in names[1:]:
                    assert torch.equal(outs[name], outs[names[0]]), f"{name} differs from {names[0]} at {geom}, arithmetic {prec}, splitk {splitk}"
                if op == 2 or stride != 2:
                    continue
                # the fused-statistics form against the grouped form with a statistics buffer
                rows = L.dg_conv_bnstats_rows_p(*g, prec)
                assert rows > 0, (g, prec)
                nstat = rows * (3 * (K if op == 0 else C) + 4)
                fused = ("dg_conv_fwd_bnstats", "dg_conv_dgrad_bnstats")[op]
                grouped = ("dg_conv_fwd_g", "dg_conv_dgrad_g")[op]
                o1, o2 = (torch.full((out_numel,), FILL, device=DEV) for _ in range(2))
                s1, s2 = (torch.full((nstat,), -7.0, device=DEV) for _ in range(2))
                assert getattr(L, fused)(ptr(a), ptr(b), ptr(o1), N, H, H, C, K, ptr(s1), nstat, ptr(ws), wsb, st) == 0, L.dg_last_error()
                assert getattr(L, grouped)(1, tab(a), tab(b), tab(o2), N, H, H, C, K, stride, pad, ops.PREC_DEFAULT, 1, tab(s2), nstat, tab(ws),
                                           wsb, st) == 0, L.dg_last_error()
                torch.cuda.synchronize()
                assert not torch.isnan(o1).any() and torch.equal(o1, o2), f"{fused} output at {geom}, arithmetic {prec}, splitk {splitk}"
                assert torch.equal(s1, s2), f"{fused} statistics rows at {geom}, arithmetic {prec}, splitk {splitk}"
                assert not torch.equal(s1, torch.full_like(s1, -7.0)), f"{fused} wrote no statistics"
    finally:
        _lib.set_option("splitk", 0)
        _lib.set_option("bf16", 0)
