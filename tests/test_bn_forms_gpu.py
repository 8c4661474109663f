"""The entry-point forms of one BatchNorm pass agree bitwise.

Training statistics, the apply pass and the backward pass can each be asked for through a plain form (dg_bn_train_stats / dg_bn_act_fwd /
dg_bn_act_bwd), a storage-type form (_t), a grouped form (_g) with one problem and, for the two apply passes, a form that also writes
a bf16 shadow (_bf16) or a bf16 plane triple in either layout (_x3), with or without the fp32 output.  All of them fill one call
record and go through the same validation, form choice and launch, so what they have in common is bitwise equal -- on the rows
kernels and (option "bn_items" 1) on the item kernels -- and a refused call writes nothing.  The VALUES of the shadow and the planes
are pinned by tests/test_ops_gpu.py; here only that they do not depend on whether the fp32 output is written.

Shapes (M, C), the smallest that reach each branch of the form choice:
    16 x 64     rows kernels, one channel chunk
    24 x 192    rows kernels, ragged channel chunk
    12 x 64     item kernels (M % 8 != 0); quad-chunk planes still allowed (M % 4 == 0)
    6 x 12      item kernels, C no multiple of 64 (nor of 8: fp32 output only)
    16 x 24     bf16 storage at 8 channels per lane
    2560 x 64   more than one row chunk in the reductions (128 rows per chunk at C = 64)
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, ops  # noqa: E402
from tests.gpu_util import options  # noqa: E402

DEV = "cuda"
FILL = float("nan")                                        # outputs start as NaN: an element no kernel wrote is never "equal"
INVALID = -1                                               # DG_ERR_INVALID
SLOPE, EPS, MOMENTUM = 0.2, 1e-5, 0.1
SHAPES = [(16, 64), (24, 192), (12, 64), (6, 12), (16, 24), (2560, 64)]
SHAPE = pytest.mark.parametrize("M,C", SHAPES, ids=[f"{m}x{c}" for m, c in SHAPES])
ITEMS = pytest.mark.parametrize("items", [0, 1], ids=["rows", "items"])


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def tab(t):
    return (ctypes.c_void_p * 1)(t.data_ptr() if t is not None else None)


def stream():
    return torch.cuda.current_stream().cuda_stream


def nans(n, dtype=torch.float32):
    return torch.full((n,), FILL, device=DEV, dtype=dtype)


def workspace(L, M, C):
    wsb = L.dg_bn_workspace_bytes(M, C)
    return torch.empty(wsb // 8 + 1, device=DEV, dtype=torch.float64), wsb


_PROBLEMS = {}


def problem(M, C):
    """The inputs of one shape, made once and never written: y, dz, gamma, beta and saved (the statistics of y)."""
    if (M, C) not in _PROBLEMS:
        g = torch.Generator().manual_seed(1000 * M + C)
        y, dz = (((torch.rand(M * C, generator=g) * 2 - 1) * s).to(DEV) for s in (2.0, 1.0))
        gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.rand(C, generator=g) - 0.5).to(DEV)
        L = _lib.load()
        saved = nans(2 * C)
        ws, wsb = workspace(L, M, C)
        assert L.dg_bn_train_stats(ptr(y), M, C, EPS, MOMENTUM, None, None, None, ptr(saved), ptr(ws), wsb, stream()) == 0, L.dg_last_error()
        torch.cuda.synchronize()
        assert not torch.isnan(saved).any()
        _PROBLEMS[M, C] = (y, dz, gamma, beta, saved)
    return _PROBLEMS[M, C]


def run(L, calls, refused=()):
    """name -> outputs of every call.  A call is (outputs, function of them): the outputs a kernel overwrites start as NaN.  The names in
    `refused` must return DG_ERR_INVALID and leave every output as it was; they are not in the result."""
    outs = {}
    for name, (o, call) in calls.items():
        before = [t.clone() for t in o]
        rc = call(*o)
        torch.cuda.synchronize()
        if name in refused:
            assert rc == INVALID, (name, rc, L.dg_last_error())
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(o, before)), f"{name} was refused but wrote"
            continue
        assert rc == 0, (name, L.dg_last_error())
        assert not any(torch.isnan(t.float()).any() for t in o), (name, "elements left unwritten")
        outs[name] = o
    return outs


def assert_all_equal(outs, what, first=None):
    """every output (or only the first `first` ones) of every call equals the first call's"""
    names = list(outs)
    assert len(names) >= 2, (what, names)
    for name in names[1:]:
        for k, (a, b) in enumerate(zip(outs[name][:first], outs[names[0]][:first])):
            assert torch.equal(a, b), f"{name} differs from {names[0]} in output {k}: {what}"


@ITEMS
@SHAPE
def test_statistics_forms_agree_bitwise(M, C, items):
    """saved (mean, invstd) and the running buffers of the plain, the storage-type and the one-problem grouped form."""
    L = _lib.load()
    y = problem(M, C)[0]

    def outputs():      # saved, running_mean, running_var, num_batches_tracked
        return [nans(2 * C), torch.full((C,), 0.5, device=DEV), torch.full((C,), 2.0, device=DEV), torch.full((1,), 3, device=DEV, dtype=torch.int64)]

    ws, wsb = workspace(L, M, C)
    g = (M, C, EPS, MOMENTUM)
    calls = {
        "stats": (outputs(), lambda s, rm, rv, nbt: L.dg_bn_train_stats(ptr(y), *g, ptr(rm), ptr(rv), ptr(nbt), ptr(s), ptr(ws), wsb, stream())),
        "stats_t": (outputs(), lambda s, rm, rv, nbt: L.dg_bn_train_stats_t(ptr(y), 0, *g, ptr(rm), ptr(rv), ptr(nbt), ptr(s), ptr(ws), wsb, stream())),
        "stats_g": (outputs(), lambda s, rm, rv, nbt: L.dg_bn_train_stats_g(1, 1, tab(y), *g, tab(rm), tab(rv), tab(nbt), tab(s), tab(ws), wsb, stream())),
    }
    with options(bn_items=items):
        outs = run(L, calls)
    assert_all_equal(outs, f"statistics {M}x{C}")
    assert torch.equal(outs["stats"][0], problem(M, C)[4]) and int(outs["stats"][3]) == 4


def plane_layouts(M, C):
    return [0, 1] if (C % 64 == 0 and M % 4 == 0) else [0]


@ITEMS
@SHAPE
def test_forward_forms_agree_bitwise(M, C, items):
    """z of every form with an fp32 output; the planes of the plane-only form equal the planes written next to z."""
    L = _lib.load()
    y, _, gamma, beta, saved = problem(M, C)
    g = (M, C, ptr(saved), ptr(gamma), ptr(beta), ops.ACT_LEAKY, SLOPE)
    n = M * C
    calls = {
        "fwd": ([nans(n)], lambda z: L.dg_bn_act_fwd(ptr(y), ptr(z), *g, stream())),
        "fwd_t": ([nans(n)], lambda z: L.dg_bn_act_fwd_t(ptr(y), ptr(z), 0, *g, stream())),
        "fwd_g": ([nans(n)], lambda z: L.dg_bn_act_fwd_g(1, tab(y), tab(z), M, C, tab(saved), tab(gamma), tab(beta), ops.ACT_LEAKY, SLOPE, stream())),
    }
    only = {}
    if C % 8 == 0:
        calls["fwd_bf16"] = ([nans(n), nans(n, torch.bfloat16)], lambda z, z16: L.dg_bn_act_fwd_bf16(ptr(y), ptr(z), ptr(z16), *g, stream()))
        for lay in plane_layouts(M, C):
            calls[f"fwd_x3 layout {lay}"] = ([nans(n), nans(3 * n, torch.bfloat16)],
                                             lambda z, z3, lay=lay: L.dg_bn_act_fwd_x3(ptr(y), ptr(z), ptr(z3), n, lay, *g, stream()))
            only[lay] = ([nans(3 * n, torch.bfloat16)], lambda z3, lay=lay: L.dg_bn_act_fwd_x3(ptr(y), None, ptr(z3), n, lay, *g, stream()))
    with options(bn_items=items):
        outs = run(L, calls)
        planes = run(L, {lay: c for lay, c in only.items()})
    assert_all_equal(outs, f"forward {M}x{C}", first=1)
    for lay, (z3,) in planes.items():
        assert torch.equal(z3, outs[f"fwd_x3 layout {lay}"][1]), f"plane-only forward, layout {lay}, {M}x{C}"


@pytest.mark.parametrize("accumulate", [0, 1])
@ITEMS
@SHAPE
def test_backward_forms_agree_bitwise(M, C, items, accumulate):
    """dy, dgamma and dbeta of every form with an fp32 output (accumulate: onto the same preset gradients); the plane-only form gives the
    same planes and parameter gradients as the form that also writes dy."""
    L = _lib.load()
    y, dz, gamma, beta, saved = problem(M, C)
    g = (M, C, ptr(saved), ptr(gamma), ptr(beta), ops.ACT_LEAKY, SLOPE)
    n = M * C
    ws, wsb = workspace(L, M, C)
    w = (accumulate, ptr(ws), wsb)

    def grads():        # dgamma, dbeta: overwritten, or accumulated onto
        return [torch.full((C,), 0.25, device=DEV), torch.full((C,), -1.5, device=DEV)] if accumulate else [nans(C), nans(C)]

    calls = {
        "bwd": ([nans(n)] + grads(), lambda dy, dg, db: L.dg_bn_act_bwd(ptr(dz), ptr(y), ptr(dy), *g, ptr(dg), ptr(db), *w, stream())),
        "bwd_t": ([nans(n)] + grads(), lambda dy, dg, db: L.dg_bn_act_bwd_t(ptr(dz), ptr(y), ptr(dy), 0, *g, ptr(dg), ptr(db), *w, stream())),
        "bwd_g": ([nans(n)] + grads(), lambda dy, dg, db: L.dg_bn_act_bwd_g(1, 1, tab(dz), tab(y), tab(dy), M, C, tab(saved), tab(gamma), tab(beta),
                                                                           ops.ACT_LEAKY, SLOPE, tab(dg), tab(db), accumulate, tab(ws), wsb, stream())),
    }
    only = {}
    if C % 8 == 0:
        calls["bwd_bf16"] = ([nans(n)] + grads() + [nans(n, torch.bfloat16)],
                             lambda dy, dg, db, dy16: L.dg_bn_act_bwd_bf16(ptr(dz), ptr(y), ptr(dy), ptr(dy16), *g, ptr(dg), ptr(db), *w, stream()))
        for lay in plane_layouts(M, C):
            calls[f"bwd_x3 layout {lay}"] = ([nans(n)] + grads() + [nans(3 * n, torch.bfloat16)], lambda dy, dg, db, dy3, lay=lay: L.dg_bn_act_bwd_x3(
                ptr(dz), ptr(y), ptr(dy), ptr(dy3), n, lay, *g, ptr(dg), ptr(db), *w, stream()))
            only[lay] = (grads() + [nans(3 * n, torch.bfloat16)], lambda dg, db, dy3, lay=lay: L.dg_bn_act_bwd_x3(
                ptr(dz), ptr(y), None, ptr(dy3), n, lay, *g, ptr(dg), ptr(db), *w, stream()))
    with options(bn_items=items):
        outs = run(L, calls)
        planes = run(L, {lay: c for lay, c in only.items()})
    assert_all_equal(outs, f"backward {M}x{C} accumulate {accumulate}", first=3)
    for lay, got in planes.items():
        for a, b in zip(got, outs[f"bwd_x3 layout {lay}"][1:]):
            assert torch.equal(a, b), f"plane-only backward, layout {lay}, {M}x{C}"


@ITEMS
@SHAPE
def test_bf16_storage_runs_where_c_is_a_multiple_of_8_and_is_refused_elsewhere(M, C, items):
    """io_bf16 = 1 of the three _t forms: every element of every output is written; C = 12 is refused with nothing written."""
    L = _lib.load()
    y, dz, gamma, beta, saved = problem(M, C)
    y16, dz16 = y.to(torch.bfloat16), dz.to(torch.bfloat16)
    g = (M, C, ptr(saved), ptr(gamma), ptr(beta), ops.ACT_LEAKY, SLOPE)
    n = M * C
    ws, wsb = workspace(L, M, C)
    calls = {
        "stats_t": ([nans(2 * C)], lambda s: L.dg_bn_train_stats_t(ptr(y16), 1, M, C, EPS, MOMENTUM, None, None, None, ptr(s), ptr(ws), wsb, stream())),
        "fwd_t": ([nans(n, torch.bfloat16)], lambda z: L.dg_bn_act_fwd_t(ptr(y16), ptr(z), 1, *g, stream())),
        "bwd_t": ([nans(n, torch.bfloat16), nans(C), nans(C)],
                  lambda dy, dg, db: L.dg_bn_act_bwd_t(ptr(dz16), ptr(y16), ptr(dy), 1, *g, ptr(dg), ptr(db), 0, ptr(ws), wsb, stream())),
    }
    with options(bn_items=items):
        outs = run(L, calls, refused=tuple(calls) if C % 8 else ())
    assert len(outs) == (0 if C % 8 else 3)
