"""The entry-point forms of one 3-channel edge op agree bitwise, and an arithmetic argument wins over the process default.

The first conv of every network and the last transposed conv of every generator can be asked for through a plain form
(dg_conv4x4s2_c3_fwd / _dgrad / _wgrad, process-default arithmetic), a storage-type form (_t), an explicit-arithmetic form (_p), a
fused-activation form (_act / _act_p) and a grouped form (_g) with one problem.  All of them fill one call record and go through the
same validation, form choice and launch, so their outputs are bitwise equal -- under each arithmetic, with the streaming / scatter
kernels and (option "kt" 16) with the tiled / gather ones -- and a form that a kernel does not have is refused with nothing written.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, ops  # noqa: E402

DEV = "cuda"
FILL = float("nan")                                        # outputs start as NaN: an element no kernel wrote is never "equal"
INVALID = -1                                               # DG_ERR_INVALID
SLOPE = 0.2
PRECS = pytest.mark.parametrize("prec", [0, 1, 2], ids=["f32", "bf16", "f32x3"])
KTS = pytest.mark.parametrize("kt", [0, 16], ids=["kt0", "kt16"])


def rnd(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, generator=g) * 2 - 1) * scale).to(DEV)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def tab(t):
    return (ctypes.c_void_p * 1)(t.data_ptr() if t is not None else None)


def stream():
    return torch.cuda.current_stream().cuda_stream


def run(L, calls, numel, preset=None, refused=()):
    """name -> output of every call; each starts from NaN (or a copy of `preset`).  The names in `refused` must return
    DG_ERR_INVALID and leave their output untouched; they are not in the result."""
    outs = {}
    for name, call in calls.items():
        o = torch.full((numel,), FILL, device=DEV) if preset is None else preset.clone()
        rc = call(o)
        torch.cuda.synchronize()
        if name in refused:
            assert rc == INVALID, (name, rc, L.dg_last_error())
            assert torch.isnan(o).all() if preset is None else torch.equal(o, preset), f"{name} was refused but wrote"
            continue
        assert rc == 0, (name, L.dg_last_error())
        assert not torch.isnan(o).any(), (name, "elements left unwritten")
        outs[name] = o
    return outs


def assert_all_equal(outs, what):
    names = list(outs)
    assert len(names) >= 2, (what, names)
    for name in names[1:]:
        assert torch.equal(outs[name], outs[names[0]]), f"{name} differs from {names[0]}: {what}"


def fwd_calls(L, x, w, N, H, W, K, prec, act=ops.ACT_LEAKY):
    g = (N, H, W, K, act, SLOPE)
    return {
        "fwd": lambda o: L.dg_conv4x4s2_c3_fwd(ptr(x), ptr(w), ptr(o), *g, stream()),
        "fwd_t": lambda o: L.dg_conv4x4s2_c3_fwd_t(ptr(x), ptr(w), ptr(o), 0, *g, stream()),
        "fwd_p": lambda o: L.dg_conv4x4s2_c3_fwd_p(ptr(x), ptr(w), ptr(o), 0, *g, prec, stream()),
        "fwd_g": lambda o: L.dg_conv4x4s2_c3_fwd_g(1, tab(x), tab(w), tab(o), *g, prec, stream()),
    }


def wgrad_calls(L, dy, x, ws, wsb, N, H, W, K, prec, acc, io_bf16=0, act=ops.ACT_NONE, out=None):
    g = (N, H, W, K)
    calls = {
        "wgrad_t": lambda o: L.dg_conv4x4s2_c3_wgrad_t(ptr(dy), ptr(out), io_bf16, act, SLOPE, ptr(x), ptr(o), *g, acc, ptr(ws), wsb, stream()),
        "wgrad_p": lambda o: L.dg_conv4x4s2_c3_wgrad_p(ptr(dy), ptr(out), io_bf16, act, SLOPE, ptr(x), ptr(o), *g, prec, acc, ptr(ws), wsb, stream()),
    }
    if not io_bf16:
        calls["wgrad_act"] = lambda o: L.dg_conv4x4s2_c3_wgrad_act(ptr(dy), ptr(out), act, SLOPE, ptr(x), ptr(o), *g, acc, ptr(ws), wsb, stream())
        calls["wgrad_g"] = lambda o: L.dg_conv4x4s2_c3_wgrad_g(1, 1, tab(dy), tab(out), act, SLOPE, tab(x), tab(o), *g, prec, acc, tab(ws), wsb,
                                                               stream())
        if act == ops.ACT_NONE:
            calls["wgrad"] = lambda o: L.dg_conv4x4s2_c3_wgrad(ptr(dy), ptr(x), ptr(o), *g, acc, ptr(ws), wsb, stream())
    return calls


def wgrad_ws(L, N, H, W, K):
    wsb = L.dg_c3_wgrad_workspace_bytes(N, H, W, K)
    return torch.empty(wsb // 4, device=DEV), wsb


@KTS
@PRECS
def test_forward_forms_agree_bitwise(prec, kt):
    """(2,8,8,64): the streaming kernels, under "kt" 16 the tiled one (the grouped form has none and refuses); (2,8,8,128): tiled, two
    N-tiles; (2,8,8,32): tiled, ragged K.  The grouped form exists at K == 64 only."""
    L = _lib.load()
    try:
        _lib.set_option("bf16", prec)
        _lib.set_option("kt", kt)
        for N, H, W, K in ((2, 8, 8, 64), (2, 8, 8, 128), (2, 8, 8, 32)):
            x, w = rnd(N * 3 * H * W, 1), rnd(K * 48, 2, 0.1)
            refused = ("fwd_g",) if (K != 64 or kt == 16) else ()
            outs = run(L, fwd_calls(L, x, w, N, H, W, K, prec), N * (H // 2) * (W // 2) * K, refused=refused)
            assert len(outs) == 4 - len(refused)
            assert_all_equal(outs, f"forward {(N, H, W, K)}, arithmetic {prec}, kt {kt}")
    finally:
        _lib.set_option("kt", 0)
        _lib.set_option("bf16", 0)


@KTS
@PRECS
def test_input_gradient_forms_agree_bitwise(prec, kt):
    """(2,8,8,64): the scatter kernel, under "kt" 16 the gather one (one problem: the grouped form refuses); (2,8,8,32): the VALU
    kernel (no grouped form).  The fused LeakyReLU backward (scatter kernel only) against act_bwd followed by the plain form, with an
    fp32 and a bf16 dy."""
    L = _lib.load()
    try:
        _lib.set_option("bf16", prec)
        _lib.set_option("kt", kt)
        for N, H, W, K in ((2, 8, 8, 64), (2, 8, 8, 32)):
            dy, w = rnd(N * (H // 2) * (W // 2) * K, 3), rnd(K * 48, 2, 0.1)
            wsb = L.dg_c3_dgrad_workspace_bytes(K)
            ws = torch.empty(wsb // 4, device=DEV) if wsb else None
            g = (N, H, W, K, ops.ACT_SIGMOID)
            calls = {
                "dgrad": lambda o: L.dg_conv4x4s2_c3_dgrad(ptr(dy), ptr(w), ptr(o), *g, ptr(ws), wsb, stream()),
                "dgrad_t": lambda o: L.dg_conv4x4s2_c3_dgrad_t(ptr(dy), 0, ptr(w), ptr(o), *g, ptr(ws), wsb, stream()),
                "dgrad_p": lambda o: L.dg_conv4x4s2_c3_dgrad_p(ptr(dy), 0, ptr(w), ptr(o), *g, prec, ptr(ws), wsb, stream()),
                "dgrad_g": lambda o: L.dg_conv4x4s2_c3_dgrad_g(1, tab(dy), tab(w), tab(o), *g, prec, stream()),
            }
            refused = ("dgrad_g",) if (K != 64 or kt == 16) else ()
            outs = run(L, calls, N * 3 * H * W, refused=refused)
            assert len(outs) == 4 - len(refused)
            assert_all_equal(outs, f"input gradient {(N, H, W, K)}, arithmetic {prec}, kt {kt}")
        N, H, W, K = 2, 8, 8, 64
        w = rnd(K * 48, 2, 0.1)
        wsb = L.dg_c3_dgrad_workspace_bytes(K)
        ws = torch.empty(wsb // 4, device=DEV)
        g = (N, H, W, K, ops.ACT_NONE)
        for dtype in (torch.float32, torch.bfloat16):
            i16 = int(dtype == torch.bfloat16)
            dy, out = rnd(N * 16 * K, 3).to(dtype), rnd(N * 16 * K, 4).to(dtype)
            dya = ops.act_bwd(dy, out, ops.ACT_LEAKY, SLOPE)
            calls = {
                "act_bwd + dgrad_p": lambda o: L.dg_conv4x4s2_c3_dgrad_p(ptr(dya), i16, ptr(w), ptr(o), *g, prec, ptr(ws), wsb, stream()),
                "dgrad_act_p": lambda o: L.dg_conv4x4s2_c3_dgrad_act_p(ptr(dy), i16, ptr(out), ops.ACT_LEAKY, SLOPE, ptr(w), ptr(o), *g, prec, ptr(ws),
                                                                       wsb, stream()),
            }
            # the gather kernel ("kt" 16) has no fused form and reads fp32
            refused = () if kt == 0 else (tuple(calls) if i16 else ("dgrad_act_p",))
            outs = run(L, calls, N * 3 * H * W, refused=refused)
            if kt == 0:
                assert_all_equal(outs, f"fused input gradient, dy {dtype}, arithmetic {prec}")
    finally:
        _lib.set_option("kt", 0)
        _lib.set_option("bf16", 0)


@KTS
@PRECS
def test_weight_gradient_forms_agree_bitwise(prec, kt):
    """(2,8,8,64), the same under option "pointer_path" 1 (the 64-bit addressing kernels) and (1,4,256,64), whose rows reach the
    f32x3 LDS kernel: every fp32 form, overwriting and accumulating onto a preset dw, and with a fused LeakyReLU.  (1,2,32,64) with a
    bf16 dy reaches the bf16 LDS kernel: the two forms that take bf16."""
    L = _lib.load()
    try:
        _lib.set_option("bf16", prec)
        _lib.set_option("kt", kt)
        for (N, H, W, K), pointer_path in (((2, 8, 8, 64), 0), ((1, 4, 256, 64), 0), ((2, 8, 8, 64), 1)):
            _lib.set_option("pointer_path", pointer_path)
            dy, x, out = rnd(N * (H // 2) * (W // 2) * K, 3), rnd(N * 3 * H * W, 1), rnd(N * (H // 2) * (W // 2) * K, 4)
            ws, wsb = wgrad_ws(L, N, H, W, K)
            preset = rnd(K * 48, 5)
            for acc in (0, 1):
                what = f"weight gradient {(N, H, W, K)}, arithmetic {prec}, kt {kt}, pointer_path {pointer_path}, accumulate {acc}"
                outs = run(L, wgrad_calls(L, dy, x, ws, wsb, N, H, W, K, prec, acc), K * 48, preset=preset if acc else None)
                assert len(outs) == 5
                assert_all_equal(outs, what)
                if acc:
                    assert not torch.equal(outs["wgrad"], preset)
                fused = run(L, wgrad_calls(L, dy, x, ws, wsb, N, H, W, K, prec, acc, act=ops.ACT_LEAKY, out=out), K * 48,
                            preset=preset if acc else None)
                assert len(fused) == 4
                assert_all_equal(fused, what + ", fused LeakyReLU")
                assert not torch.equal(fused["wgrad_p"], outs["wgrad_p"])
        _lib.set_option("pointer_path", 0)
        N, H, W, K = 1, 2, 32, 64
        dy, x = rnd(N * (H // 2) * (W // 2) * K, 3).to(torch.bfloat16), rnd(N * 3 * H * W, 1)
        ws, wsb = wgrad_ws(L, N, H, W, K)
        preset = rnd(K * 48, 5)
        for acc in (0, 1):
            outs = run(L, wgrad_calls(L, dy, x, ws, wsb, N, H, W, K, prec, acc, io_bf16=1), K * 48, preset=preset if acc else None)
            assert len(outs) == 2
            assert_all_equal(outs, f"weight gradient {(N, H, W, K)} with a bf16 dy, arithmetic {prec}, kt {kt}, accumulate {acc}")
    finally:
        _lib.set_option("pointer_path", 0)
        _lib.set_option("kt", 0)
        _lib.set_option("bf16", 0)


@pytest.mark.parametrize("a,b", [(0, 1), (0, 2), (1, 0), (2, 0)])
def test_the_arithmetic_argument_wins_over_the_process_default(a, b):
    """Process default a, explicit prec b != a: the _p / _g forms give bitwise the plain form's output under process default b, on the
    (2,8,8,64) forward and the (1,4,256,64) weight gradient.  Random inputs make f32 and bf16 products differ, so for (0, 1) the
    forward also differs from the default-0 output: an ignored argument cannot pass.  A plain call right after a _p call runs on the
    process default again."""
    L = _lib.load()
    N, H, W, K = 2, 8, 8, 64
    x, w = rnd(N * 3 * H * W, 1), rnd(K * 48, 2, 0.1)
    wN, wH, wW = 1, 4, 256
    dy, wx = rnd(wN * (wH // 2) * (wW // 2) * K, 3), rnd(wN * 3 * wH * wW, 1)
    ws, wsb = wgrad_ws(L, wN, wH, wW, K)
    try:
        plain = {}
        for d in (a, b):
            _lib.set_option("bf16", d)
            plain[d] = (run(L, {"fwd": fwd_calls(L, x, w, N, H, W, K, d)["fwd"]}, N * 16 * K)["fwd"],
                        run(L, {"wgrad": wgrad_calls(L, dy, wx, ws, wsb, wN, wH, wW, K, d, 0)["wgrad"]}, K * 48)["wgrad"])
        if (a, b) == (0, 1):
            assert not torch.equal(plain[a][0], plain[b][0])
        _lib.set_option("bf16", a)
        calls = fwd_calls(L, x, w, N, H, W, K, b)
        outs = run(L, {n: calls[n] for n in ("fwd_p", "fwd_g", "fwd")}, N * 16 * K)            # in this order: the plain call last
        assert torch.equal(outs["fwd_p"], plain[b][0]) and torch.equal(outs["fwd_g"], plain[b][0]), f"forward: prec {b} under process default {a}"
        assert torch.equal(outs["fwd"], plain[a][0]), f"forward: the plain form after a _p call, process default {a}"
        calls = wgrad_calls(L, dy, wx, ws, wsb, wN, wH, wW, K, b, 0)
        outs = run(L, {n: calls[n] for n in ("wgrad_p", "wgrad_g", "wgrad")}, K * 48)
        assert torch.equal(outs["wgrad_p"], plain[b][1]) and torch.equal(outs["wgrad_g"], plain[b][1]), f"weight gradient: prec {b} under process default {a}"
        assert torch.equal(outs["wgrad"], plain[a][1]), f"weight gradient: the plain form after a _p call, process default {a}"
    finally:
        _lib.set_option("bf16", 0)
