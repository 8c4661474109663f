"""Convolutions at channel counts the model never makes: C and K that are not whole 64-column wave tiles or 32-deep K-tiles, on every
entry point that accepts them -- the exact-fp32 implicit-GEMM kernel (buffer and 64-bit pointer form), the 4 x 4 heads, the f32x3 and
bf16 modes (which fall back per op at such counts), the fused BatchNorm statistics of a ragged column tile, the inference forms, the
3-channel edge kernels, grouped launches, and the autograd modules.  Every result is compared with a float64 CPU reference under the
elementwise bound of tests/shape_ref.py (no tolerance of this file's own), every case asserts from the plan queries which kernel family
it reached, and every case shows that the bound would catch a one-pixel shift AND a rotation of the output or input channels."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, functional as F, model, ops  # noqa: E402
from tests import shape_ref as R  # noqa: E402
from tests.gpu_util import DEV, ambient, krsc, nhwc, options, with_shadow  # noqa: E402
from tests.shape_ref import rnd  # noqa: E402

OPI = {"fwd": 0, "dgrad": 1, "wgrad": 2}
TF = torch.nn.functional


# ---- problems, float64 references (cached: the option loops reuse them) ---------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(N, C, K, H, stride=2, biased=False):
    """(x, w, dy) on the CPU from fixed seeds; weights scaled by 1 / sqrt(16 C); biased: offsets that give the statistics a mean."""
    Ho = H // 2 if stride == 2 else 1
    x, w, dy = rnd(N, C, H, H, seed=1), rnd(K, C, 4, 4, seed=2, scale=1.0 / math.sqrt(16 * C)), rnd(N, K, Ho, Ho, seed=3)
    return (x + 0.4, w, dy + 0.2) if biased else (x, w, dy)


def operands(op, N, C, K, H, stride=2, biased=False):
    x, w, dy = problem(N, C, K, H, stride, biased)
    return {"fwd": (x, w), "dgrad": (dy, w), "wgrad": (x, dy)}[op]


@functools.lru_cache(maxsize=None)
def refs(op, N, C, K, H, stride=2, rounded=False, biased=False):
    """(reference, reference on absolute values, references of the wrong problems) in float64; rounded: on bf16-rounded operands."""
    a, b = operands(op, N, C, K, H, stride, biased)
    f = R.r16 if rounded else R.f64
    a, b, pad, ws = f(a), f(b), (1 if stride == 2 else 0), (K, C, 4, 4)
    ref, absref = R.conv_ref(op, a, b, stride, pad, wshape=ws)
    wrongs = [R.conv_ref(op, wa, wb, stride, pad, wshape=ws)[0] for wa, wb in R.wrong_problems(op, a, b)]
    return ref, absref, wrongs


def reduction(op, N, C, K, H, stride=2):
    """Longest reduction of one output element."""
    if op == "wgrad":
        return N * ((H // 2) ** 2 if stride == 2 else 1)
    return R.taps(op, C, K, stride)


def check(op, got, shape, what, stride=2, mult=1, out16=False, rounded=False, biased=False):
    """got against the float64 reference of (op, shape) under shape_ref's bound, and every wrong problem outside it."""
    ref, absref, wrongs = refs(op, *shape, stride, rounded, biased)
    n = reduction(op, *shape, stride)
    R.assert_within(got, ref, absref, n, what, mult=mult, out16=out16)
    assert wrongs, what
    for i, wrong in enumerate(wrongs):
        R.assert_discriminates(wrong, ref, absref, n, f"{what}, wrong problem {i}", mult=mult, out16=out16)
    return ref


def device_operands(shape, stride=2, dtype=torch.float32, biased=False):
    x, w, dy = problem(*shape, stride, biased)
    return nhwc(x, dtype), krsc(w), nhwc(dy, dtype)


def call(op, xg, wg, dyg, H, stride=2, **kw):
    pad = 1 if stride == 2 else 0
    if op == "fwd":
        return ops.conv_fwd(xg, wg, stride, pad, **kw)
    if op == "dgrad":
        return ops.conv_dgrad(dyg, wg, (H, H), stride, pad, **kw)
    return ops.conv_wgrad(dyg, xg, stride, pad, **kw)


def geom(op, shape, stride=2):
    N, C, K, H = shape
    return (OPI[op], N, H, H, C, K, stride, 1 if stride == 2 else 0)


def expected_splits(op, shape, stride, kt, forced, prec=0):
    """The split count a forced split-K option gives (include/discogan_hip.h: at least four K-tiles per split, no empty split)."""
    N, C, K, H = shape
    npix = N * ((H // 2) ** 2 if stride == 2 else 1)
    if prec == 2:
        kt = 16
    if op == "fwd":
        nit = 16 * C // kt
    elif op == "dgrad" and stride == 2:
        nit = 4 * K // (16 if C <= 64 else kt)
    elif op == "dgrad":
        nit = -(-K // kt)
    else:
        nit = -(-npix // kt)
    s = max(1, min(forced, nit // 4, 64))
    per = -(-nit // s)
    return -(-nit // per)


def assert_splits(L, op, shape, stride, kt, forced, prec=0):
    s = L.dg_conv_plan_splits_p(*geom(op, shape, stride), prec, 1)
    if shape[2] == 1:
        assert s == 1
    elif forced > 0:
        assert s == expected_splits(op, shape, stride, kt, forced, prec), (op, shape, kt, forced, s)
    else:
        assert s >= 1
    assert L.dg_conv_workspace_bytes_p(*geom(op, shape, stride), prec, 1) > 0 or s == 1
    return s


# ---- the shape lists -------------------------------------------------------------------------------------------------
S2_FW = [(3, 32, 36, 16), (3, 96, 100, 16), (5, 32, 132, 8), (2, 96, 160, 32), (13, 96, 200, 8), (2, 160, 4, 8)]
S2_DG = [(3, C, K, 16) for C in (4, 12, 36, 60, 64, 68, 100, 132, 200) for K in (32, 96, 160)]       # both tile rules, the flip at 64
# (N 6, 16 x 16: 384 gradient pixels = 24 / 12 K-tiles of 16 / 32, so a forced split-K of three really splits; Ng = 16 C = 64, 192, 576, 1600)
S2_WG = [(6, C, K, 16) for C in (4, 12, 36, 100) for K in (4, 36, 100, 132)]
# weight gradients of the forward list with too few gradient pixels for four K-tiles per slab under either K-tile: they cannot split
FEW_PIXELS = {("wgrad", (5, 32, 132, 8)), ("wgrad", (2, 160, 4, 8))}
S2_CASES = ([(s, ("fwd", "wgrad") + (("dgrad",) if s[2] % 32 == 0 else ())) for s in S2_FW] + [(s, ("dgrad",)) for s in S2_DG] +
            [(s, ("wgrad",)) for s in S2_WG])
HEAD_CASES = ([((13, C, K, 4), ("fwd", "wgrad")) for K in (4, 36, 132) for C in (32, 96, 160)] +
              [((13, C, K, 4), ("dgrad", "wgrad")) for K in (4, 20, 36, 100, 132) for C in (4, 12, 36, 96)] +     # the ragged last K-tile
              [((13, C, 1, 4), ("fwd", "dgrad", "wgrad")) for C in (32, 96, 160)])


def ids(cases):
    return ["x".join(map(str, s)) + "-" + "+".join(o) for s, o in cases]


# ==== 9. Nothing written outside the tensor (run first: a stray store must land in memory the test owns) ============
MARGIN = 256 * 256                 # floats on each side of the output: one 256 x 256 fp32 tile
SENTINEL = -1234.5


@pytest.mark.parametrize("ptr", [0, 1], ids=["buf", "ptr"])
@pytest.mark.parametrize("splitk", [1, 3], ids=["one-slab", "three-slabs"])       # (0 would let the planner split on its own)
@pytest.mark.parametrize("op,shape", [("fwd", (3, 96, 36, 16)), ("fwd", (3, 96, 100, 16)), ("dgrad", (3, 36, 96, 16)), ("wgrad", (6, 36, 100, 16))],
                         ids=["fwd-K36", "fwd-K100", "dgrad-C36", "wgrad-C36-K100"])
def test_a_ragged_last_tile_writes_nothing_outside_its_tensor(op, shape, splitk, ptr):
    """The ragged last column tile stores float4s: the output sits inside a larger buffer filled with a sentinel, and every byte
    before and after it must be untouched (forward and input gradient through the C entry points with a pointer into the buffer, the
    weight gradient through out=)."""
    N, C, K, H = shape
    L = _lib.load()
    xg, wg, dyg = device_operands(shape)
    numel = {"fwd": N * K * (H // 2) ** 2, "dgrad": N * C * H * H, "wgrad": K * C * 16}[op]
    buf = torch.full((2 * MARGIN + numel,), SENTINEL, device=DEV)
    want = torch.full((MARGIN,), SENTINEL).view(torch.int32)
    with options(splitk=splitk, pointer_path=ptr):
        splits = assert_splits(L, op, shape, 2, 16 if op == "wgrad" else 32, splitk)
        assert (splits > 1) == (splitk == 3), f"{op} {shape}: splitk {splitk} plans {splits} split(s)"       # the slab stores and the reduction run
        if op == "wgrad":
            out = buf[MARGIN:MARGIN + numel].view(K, 4, 4, C).permute(0, 3, 1, 2)
            ops.conv_wgrad(dyg, xg, 2, 1, out=out)
        else:
            ws, wsb = ops._ws(L.dg_conv_workspace_bytes(*geom(op, shape)), DEV)
            outp = buf.data_ptr() + 4 * MARGIN
            if op == "fwd":
                _lib.check(L.dg_conv_fwd(xg.data_ptr(), wg.data_ptr(), outp, N, H, H, C, K, 2, 1, ops._ptr(ws), wsb, ops._stream()), "dg_conv_fwd")
                out = buf[MARGIN:MARGIN + numel].view(N, H // 2, H // 2, K).permute(0, 3, 1, 2)
            else:
                _lib.check(L.dg_conv_dgrad(dyg.data_ptr(), wg.data_ptr(), outp, N, H, H, C, K, 2, 1, ops._ptr(ws), wsb, ops._stream()), "dg_conv_dgrad")
                out = buf[MARGIN:MARGIN + numel].view(N, H, H, C).permute(0, 3, 1, 2)
        torch.cuda.synchronize()
    host = buf.cpu()
    assert torch.equal(host[:MARGIN].view(torch.int32), want), f"{op} {shape}: bytes BEFORE the output were written"
    assert torch.equal(host[MARGIN + numel:].view(torch.int32), want), f"{op} {shape}: bytes AFTER the output were written"
    check(op, out, shape, f"{op} {shape} splitk {splitk} ptr {ptr} inside a sentinel buffer")


# ==== 1. Exact fp32 kernel, stride 2 ====================================================================================
@pytest.mark.parametrize("ptr", [0, 1], ids=["buf", "ptr"])
@pytest.mark.parametrize("shape,oplist", S2_CASES, ids=ids(S2_CASES))
def test_exact_fp32_stride2_at_ragged_channels(shape, oplist, ptr):
    """igemm_kernel<.., PREC 0> with a masked last column tile, buffer-descriptor and 64-bit pointer form, K-tile 16 and 32, no split /
    forced one slab / three K-slabs (the split-K reduction over Ng / 4 float4 columns).  Under splitk 3 every op really splits under at
    least one of the two K-tiles (the weight-gradient grid under both), FEW_PIXELS aside."""
    L = _lib.load()
    xg, wg, dyg = device_operands(shape)
    split3 = {op: [] for op in oplist}
    for kt in (16, 32):
        for splitk in (0, 1, 3):
            with options(kt=kt, splitk=splitk, pointer_path=ptr):
                for op in oplist:
                    splits = assert_splits(L, op, shape, 2, kt, splitk)
                    assert splitk == 3 or splitk == 0 or splits == 1
                    if splitk == 3:
                        split3[op].append(splits)
                got = {op: call(op, xg, wg, dyg, shape[3]) for op in oplist}
                torch.cuda.synchronize()
            for op in oplist:
                check(op, got[op], shape, f"f32 {op} {shape} kt {kt} splitk {splitk} ptr {ptr}")
    for op in oplist:
        if (op, shape) not in FEW_PIXELS:
            assert max(split3[op]) > 1, f"{op} {shape}: splitk 3 never split ({split3[op]})"
        if shape in S2_WG:
            assert min(split3[op]) > 1, f"{op} {shape}: splitk 3 must split under both K-tiles ({split3[op]})"


# ==== 2. The 4 x 4 heads ===============================================================================================
@pytest.mark.parametrize("ptr", [0, 1], ids=["buf", "ptr"])
@pytest.mark.parametrize("shape,oplist", HEAD_CASES, ids=ids(HEAD_CASES))
def test_exact_fp32_heads_at_ragged_channels(shape, oplist, ptr):
    """Conv2d(C, K, 4, 1, 0) on a 4 x 4 input: forward, input gradient (K-tile count rounded up: K = 4, 20, 36, 100, 132 leave a ragged
    last K-tile) and weight gradient; K = 1 takes the plain reductions."""
    L = _lib.load()
    xg, wg, dyg = device_operands(shape, stride=1)
    for kt in (16, 32):
        for splitk in (0, 3):
            with options(kt=kt, splitk=splitk, pointer_path=ptr):
                for op in oplist:
                    splits = assert_splits(L, op, shape, 1, kt, splitk)
                    # (16 C / kt K-tiles: the forward splits; the weight gradient has 13 reduction rows, the input gradient K / kt K-tiles)
                    assert op != "fwd" or shape[2] == 1 or splitk != 3 or splits > 1, (op, shape, kt, splitk, splits)
                    assert L.dg_conv_bnstats_rows_p(*geom(op, shape, 1), 0) == 0
                got = {op: call(op, xg, wg, dyg, 4, stride=1) for op in oplist}
                torch.cuda.synchronize()
            for op in oplist:
                check(op, got[op], shape, f"f32 head {op} {shape} kt {kt} splitk {splitk} ptr {ptr}", stride=1)


# ==== 3. The same lists under f32x3 =====================================================================================
def x3_expected(op, shape, stride):
    """dg_conv_x3_planes_ok by the rules of include/discogan_hip.h: 1 the plane kernel (both extents >= 192, or a weight gradient of
    96 rows and more; C and K multiples of 8, the reduction in whole 16-channel chunks), 2 / 1 the window input gradient (C <= 128, image
    rows of 32..128 pixels), 0 the register-staged f32x3 tiles."""
    N, C, K, H = shape
    Ho = H // 2 if stride == 2 else 1
    npix = N * Ho * Ho
    if K == 1 or C % 8 or K % 8 or (op == "fwd" and C % 32) or (op == "dgrad" and (stride != 2 or K % 32)):
        return 0
    M, Ng = {"fwd": (npix, K), "dgrad": (npix, C), "wgrad": (K, 16 * C)}[op]
    if (Ng >= 192 and M >= 192) or (op == "wgrad" and M >= 96 and Ng >= 192):
        return 1
    if op == "dgrad" and C <= 128 and 32 <= Ho <= 128 and Ho * Ho >= 256:
        return 2 if K % 64 == 0 else 1
    return 0


# input gradients with image rows of 32 pixels and C <= 128: the window kernels (f32x3: planes_ok 2 at K % 64 == 0, else 1; bf16: 2)
WINDOW_DG = [(1, 40, 64, 64), (1, 72, 32, 64), (2, 104, 96, 64), (2, 104, 128, 64)]
X3_CASES = [(s, o, 2) for s, o in S2_CASES] + [(s, o, 1) for s, o in HEAD_CASES] + [(s, ("dgrad",), 2) for s in WINDOW_DG]


@pytest.mark.parametrize("shape,oplist,stride", X3_CASES, ids=[i + f"-s{st}" for i, (_, _, st) in zip(ids([c[:2] for c in X3_CASES]), X3_CASES)])
def test_f32x3_at_ragged_channels(shape, oplist, stride):
    """options(bf16=2) with plane operands on: per op the plane kernel where the queries say so, else the register-staged f32x3 tiles
    (the K == 1 head: plain fp32 reductions) -- gamma(8 n) either way."""
    L = _lib.load()
    H = shape[3]
    xg, wg, dyg = device_operands(shape, stride)
    for splitk in (0, 3):
        with options(bf16=2, splitk=splitk), ambient(x3=True):
            for op in oplist:
                code = L.dg_conv_x3_planes_ok(*geom(op, shape, stride))
                assert code == x3_expected(op, shape, stride), (op, shape, code)
                assert shape not in WINDOW_DG or code == (2 if shape[2] % 64 == 0 else 1), (shape, code)
                splits = assert_splits(L, op, shape, stride, 16, splitk if code == 0 else 0, prec=2)
                assert shape not in S2_WG or splitk != 3 or splits > 1, (op, shape, splitk, splits)
            got = {op: call(op, xg, wg, dyg, H, stride) for op in oplist}
            torch.cuda.synchronize()
        for op in oplist:
            check(op, got[op], shape, f"f32x3 {op} {shape} stride {stride} splitk {splitk}", stride=stride, mult=1 if shape[2] == 1 else 8)


# ==== 4. bf16 operands at ragged counts ================================================================================
BF16_YES = ([("dgrad", (2, 36, 64, 16)), ("dgrad", (3, 200, 64, 16)), ("dgrad", (3, 100, 128, 16)), ("fwd", (3, 64, 36, 16)), ("fwd", (3, 64, 200, 16)),
             ("fwd", (5, 128, 132, 8))] + [("wgrad", s) for s in S2_FW] + [("wgrad", s) for s in S2_WG[::3]] +
            [("dgrad", s) for s in WINDOW_DG if s[2] % 64 == 0])
BF16_NO = [("fwd", (3, 96, 100, 16)), ("fwd", (2, 96, 160, 32)), ("fwd", (5, 32, 132, 8)), ("dgrad", (3, 100, 96, 16)), ("dgrad", (3, 36, 160, 16)),
           ("dgrad", (3, 64, 32, 16))]


def _io16_ok(op, shape):
    N, C, K, H = shape
    return (op == "fwd" and C % 8 == 0) or (op == "dgrad" and K % 8 == 0) or (op == "wgrad" and C % 8 == 0 and K % 8 == 0)


BF16_CASES = [(op, s, f) for op, s in BF16_YES for f in ("both", "one", "io16") if f != "io16" or _io16_ok(op, s)]


@pytest.mark.parametrize("op,shape,form", BF16_CASES, ids=[f"{o}-{'x'.join(map(str, s))}-{f}" for o, s, f in BF16_CASES])
def test_bf16_operands_at_ragged_channels(op, shape, form):
    """Shapes where dg_conv_bf16_operands_ok answers 1 or 2 without whole 64-channel tiles on the OTHER extent: bf16 shadows of both
    operands, of one only (the weight; for the weight gradient dy), and bf16 feature maps in and out.  The kernel multiplies bf16-rounded
    operands whichever way they arrive; a bf16 output adds its own rounding."""
    N, C, K, H = shape
    L = _lib.load()
    code = L.dg_conv_bf16_operands_ok(*geom(op, shape))
    assert code >= 1
    if op == "dgrad":
        lds_dma = C >= 192 and N * (H // 2) ** 2 >= 192                # both extents fill 3/4 of the 256 x 256 tile
        assert (code == 2) == (shape in WINDOW_DG or lds_dma), (shape, code)      # 2: with both operands bf16 the window / LDS-DMA kernel runs
    io16 = form == "io16"
    outch = {"fwd": K, "dgrad": C, "wgrad": 0}[op]
    out16 = io16 and op != "wgrad" and outch % 8 == 0
    with options(bf16=1), ambient(shadow=True, act16=io16):
        xg, wg, dyg = device_operands(shape, dtype=torch.bfloat16 if io16 else torch.float32)
        if not io16:
            if op == "wgrad":
                with_shadow(dyg)
                if form == "both":
                    with_shadow(xg)
            else:
                with_shadow(wg)
                if form == "both":
                    with_shadow(xg if op == "fwd" else dyg)
        else:
            with_shadow(wg)
        got = call(op, xg, wg, dyg, H)
        torch.cuda.synchronize()
    assert (got.dtype == torch.bfloat16) == out16
    check(op, got, shape, f"bf16 {form} {op} {shape}", rounded=True, out16=out16)


@pytest.mark.parametrize("op,shape", BF16_NO, ids=[f"{o}-{'x'.join(map(str, s))}" for o, s in BF16_NO])
def test_bf16_context_falls_back_to_exact_fp32(op, shape):
    """dg_conv_bf16_operands_ok answers 0 (forward C % 64 != 0, input gradient K % 64 != 0) while the context asks for bf16 and shadows
    exist: the exact-fp32 kernel runs on the UNROUNDED operands, so the fp32 bound holds."""
    L = _lib.load()
    assert L.dg_conv_bf16_operands_ok(*geom(op, shape)) == 0
    with options(bf16=1), ambient(shadow=True):
        xg, wg, dyg = device_operands(shape)
        with_shadow(wg)
        with_shadow(xg if op == "fwd" else dyg)
        got = call(op, xg, wg, dyg, shape[3])
        torch.cuda.synchronize()
    assert got.dtype == torch.float32
    check(op, got, shape, f"bf16 context, fp32 kernel: {op} {shape}")


# ==== 5. Fused BatchNorm statistics with a ragged column tile ========================================================
STAT_CASES = [(op, mode, ch, how) for op in ("fwd", "dgrad") for mode in ("f32", "f32x3", "bf16") for ch in (36, 100, 132) for how in (True, "split")]


@pytest.mark.parametrize("op,mode,ch,how", STAT_CASES, ids=[f"{o}-{m}-{c}-{'split' if h == 'split' else 'epilogue'}" for o, m, c, h in STAT_CASES])
def test_fused_bn_statistics_of_a_ragged_column_tile(op, mode, ch, how):
    """want_stats from the kernel epilogue (True) and from the split-K reduction ("split", three slabs forced): the statistics row of a
    column tile that is not whole.  Merged with bn_stats_from_partials; mean and biased variance against the float64 statistics of the
    float64 reference, as test_conv_fused_bn_statistics_non_square does; the statistics of rotated channels must fail."""
    red = 128 if mode == "bf16" else 96                # the reduction extent: whole 64-channel tiles where the bf16 kernels need them
    shape = (3, red, ch, 16) if op == "fwd" else (3, ch, red, 16)
    N, C, K, H = shape
    L = _lib.load()
    prec = {"f32": 0, "bf16": 1, "f32x3": 2}[mode]
    rounded = mode == "bf16"
    with options(bf16=prec, splitk=3 if how == "split" else 1), ambient(shadow=rounded, x3=mode == "f32x3"):
        xg, wg, dyg = device_operands(shape, biased=True)
        if rounded:
            assert L.dg_conv_bf16_operands_ok(*geom(op, shape)) >= 1
            with_shadow(wg)
            with_shadow(xg if op == "fwd" else dyg)
            rows = L.dg_conv_mixed_bnstats_rows(*geom(op, shape), 1, 1)
        else:
            assert L.dg_conv_x3_planes_ok(*geom(op, shape)) == 0          # fewer than 192 columns: the register-staged tiles
            rows = L.dg_conv_bnstats_rows_p(*geom(op, shape), prec)
        splits = L.dg_conv_plan_splits_p(*geom(op, shape), prec, 1)
        assert rows > 0 and (splits > 1) == (how == "split"), (rows, splits)
        out, st = call(op, xg, wg, dyg, H, want_stats=how)
        assert st is not None and tuple(st.shape) == (rows, 3 * ch + 4), (None if st is None else tuple(st.shape), rows)
        saved = ops.bn_stats_from_partials(st, out, None, None, None, 1e-5, 0.1)
        torch.cuda.synchronize()
    what = f"want_stats={how} {mode} {op} {shape}"
    ref = check(op, out, shape, what, mult=8 if mode == "f32x3" else 1, rounded=rounded, biased=True)
    mean, var = ref.mean((0, 2, 3)), ref.var((0, 2, 3), unbiased=False)
    sc = mean.abs() + var.sqrt()
    assert R.bn_violations(saved[0], mean, sc) == 0, f"{what}: mean"
    assert R.bn_violations(1.0 / saved[1].double() ** 2 - 1e-5, var, var) == 0, f"{what}: variance"
    assert R.bn_violations(torch.roll(mean, 1), mean, sc) > 0 and R.bn_violations(torch.roll(var, 1), var, var) > 0, f"{what}: bound vacuous"


# ==== 6. Inference forms ================================================================================================
def _act64(v, act):
    return {"none": v, "relu": v.clamp(min=0), "leaky": torch.where(v > 0, v, 0.2 * v)}[act]


@pytest.mark.parametrize("op,shape", [("fwd", (3, 96, 100, 16)), ("fwd", (5, 32, 132, 8)), ("dgrad", (3, 100, 96, 16)), ("dgrad", (3, 36, 32, 16))],
                         ids=["fwd-96-100", "fwd-32-132", "dgrad-100-96", "dgrad-36-32"])
def test_inference_forms_at_ragged_channels(op, shape):
    """act(conv + bias) in one kernel, under shape_ref.with_epilogue's rule for a bias and an activation on top of a sum."""
    N, C, K, H = shape
    acts = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY}
    xg, wg, dyg = device_operands(shape)
    nch = K if op == "fwd" else C
    bias = rnd(nch, seed=7, scale=0.5)
    bg = bias.to(DEV)
    ref, absref, wrongs = refs(op, *shape)
    b64 = bias.double().view(1, -1, 1, 1)
    for name, a in acts.items():
        n, absb = R.with_epilogue(reduction(op, *shape), absref, bias=b64, act=name)
        if op == "fwd":
            got = ops.conv_fwd_bias_act(xg, wg, bg, 2, 1, a, 0.2)
        else:
            got = ops.conv_dgrad_bias_act(dyg, wg, bg, (H, H), 2, 1, a, 0.2)
        torch.cuda.synchronize()
        want = _act64(ref + b64, name)
        R.assert_within(got, want, absb, n, f"{op}_bias_act {name} {shape}")
        for i, wrong in enumerate(wrongs):
            R.assert_discriminates(_act64(wrong + b64, name), want, absb, n, f"{op}_bias_act {name} {shape}, wrong problem {i}")
        R.assert_discriminates(_act64(ref + torch.roll(b64, 1, 1), name), want, absb, n, f"{op}_bias_act {name}: rotated bias")


# ==== 7. Edge kernels (3 image channels) ==============================================================================
C3_MODES = {"f32": 0, "f32x3": 2, "bf16_mfma": 1}


def c3_problem(N, K, H):
    x = torch.rand(N, 3, H, H, generator=torch.Generator().manual_seed(1))
    return x, rnd(K, 3, 4, 4, seed=2, scale=0.2), rnd(N, K, H // 2, H // 2, seed=3)


C3_POST = {"none": lambda v: v, "leaky": lambda v: TF.leaky_relu(v, 0.2), "sigmoid": torch.sigmoid}


def c3_check(op, got, a, b, n, what, wshape=None, mult=1, act="none", scaled=False):
    """n = the reduction of the plain op; a fused activation / a gradient scaled on the way in by shape_ref.with_epilogue's rule."""
    post = C3_POST[act]
    ref, absref = R.conv_ref(op, a, b, wshape=wshape)
    n, absref = R.with_epilogue(n, absref, act=act, scaled=scaled)
    R.assert_within(got, post(ref), absref, n, what, mult=mult)
    wrongs = R.wrong_problems(op, R.f64(a), R.f64(b))
    assert len(wrongs) >= 3
    for i, (wa, wb) in enumerate(wrongs):
        R.assert_discriminates(post(R.conv_ref(op, wa, wb, wshape=wshape)[0]), post(ref), absref, n, f"{what}, wrong problem {i}", mult=mult)


@pytest.mark.parametrize("mode", list(C3_MODES))
@pytest.mark.parametrize("K", [4, 36, 100, 192])
def test_c3_forward_and_input_gradient_off_64_channels(K, mode):
    """conv1 / the last transposed conv at K != 64: the tiled forward and the VALU input gradient (the MFMA forms exist at K = 64 only,
    so every arithmetic mode runs exact fp32 here and the fused activation backward does not exist); with and without the sigmoid.
    Off K = 64 the input gradient has the VALU form only: the gather form (option kt 16) exists at K = 64 and is covered by
    test_shapes_gpu.test_c3_gather_and_valu_forms_non_square."""
    N, H = 2, 16
    x, w, dy = c3_problem(N, K, H)
    mult = 8 if mode == "f32x3" else 1
    with options(bf16=C3_MODES[mode]):
        assert not ops.c3_dgrad_act_ok(K, N, H, H)
        y = ops.c3_fwd(x.to(DEV), w.to(DEV), ops.ACT_NONE)
        dx = ops.c3_dgrad(nhwc(dy), w.to(DEV), ops.ACT_NONE)
        dxs = ops.c3_dgrad(nhwc(dy), w.to(DEV), ops.ACT_SIGMOID)
        torch.cuda.synchronize()
    what = f"c3 {mode} K={K}"
    c3_check("fwd", y, x, w, R.taps("fwd", 3, K), what + " fwd", mult=mult)
    c3_check("dgrad", dx, dy, w, R.taps("dgrad", 3, K), what + " dgrad", mult=mult)
    c3_check("dgrad", dxs, dy, w, R.taps("dgrad", 3, K), what + " dgrad + sigmoid", mult=mult, act="sigmoid")


@pytest.mark.parametrize("mode", list(C3_MODES))
@pytest.mark.parametrize("K", [128, 192, 320])
def test_c3_weight_gradient_and_module_off_64_channels(K, mode):
    """c3_wgrad at K = 128, 192, 320 (K % 64 == 0), and functional.ConvC3Fn (conv1 + LeakyReLU) there: c3_dgrad_act_ok is false off
    K = 64, so the backward takes the stand-alone activation backward and the unfused pair."""
    N, H = 2, 16
    x, w, dy = c3_problem(N, K, H)
    mult = 8 if mode == "f32x3" else 1
    npix = N * (H // 2) ** 2
    with options(bf16=C3_MODES[mode]):
        assert not ops.c3_dgrad_act_ok(K, N, H, H)
        dw = ops.c3_wgrad(nhwc(dy), x.to(DEV))
        xr, wp = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        y = F.ConvC3Fn.apply(xr, wp, ops.ACT_LEAKY, 0.2)
        y.backward(nhwc(dy))
        torch.cuda.synchronize()
    what = f"c3 {mode} K={K}"
    c3_check("wgrad", dw, x, dy, npix, what + " wgrad", wshape=w.shape, mult=mult)
    c3_check("fwd", y, x, w, R.taps("fwd", 3, K), what + " module forward", mult=mult, act="leaky")
    g = R.f64(dy) * torch.where(R.f64(y) > 0, 1.0, 0.2)             # the activation backward on the kernel's own sign of y
    c3_check("dgrad", xr.grad, g, w, R.taps("dgrad", 3, K), what + " module input gradient", mult=mult, scaled=True)
    c3_check("wgrad", wp.grad, x, g, npix, what + " module weight gradient", wshape=w.shape, mult=mult, scaled=True)


# ==== 8. Grouped launches ==============================================================================================
def same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: grouped launch differs from the single-problem call"


@pytest.mark.parametrize("prec", [ops.PREC_F32, ops.PREC_F32X3], ids=["f32", "f32x3"])
@pytest.mark.parametrize("g", [2, 4])
@pytest.mark.parametrize("N,C,K,H", [(3, 96, 100, 16), (2, 160, 36, 8)])
def test_grouped_launches_at_ragged_channels_are_bitwise_the_single_calls(N, C, K, H, g, prec):
    """dg_conv_*_g with 2 and 4 problems (forward, weight gradient, weight gradient with share = 2; the input gradient on the mirrored
    shape, whose K is the multiple of 32 it needs): bitwise the single-problem calls, and those inside the bound."""
    mult = 8 if prec == ops.PREC_F32X3 else 1
    scale = 1.0 / math.sqrt(16 * C)
    xs = [rnd(N, C, H, H, seed=10 + i) for i in range(g)]
    wl = [rnd(K, C, 4, 4, seed=20 + i, scale=scale) for i in range(g)]
    dys = [rnd(N, K, H // 2, H // 2, seed=30 + i) for i in range(g)]
    wm = [rnd(C, K, 4, 4, seed=40 + i, scale=1.0 / math.sqrt(16 * K)) for i in range(g)]          # the mirrored problem: C <-> K
    dm = [rnd(N, C, H // 2, H // 2, seed=50 + i) for i in range(g)]
    xg, wg, dyg, wmg, dmg = [nhwc(t) for t in xs], [krsc(t) for t in wl], [nhwc(t) for t in dys], [krsc(t) for t in wm], [nhwc(t) for t in dm]
    kr = lambda: torch.zeros((K, 4, 4, C), device=DEV).permute(0, 3, 1, 2)
    with ops.use(ops.Context(prec=prec, group_plan="single")):
        y1 = [ops.conv_fwd(x, w, 2, 1) for x, w in zip(xg, wg)]
        yg = ops.conv_fwd_g(xg, wg, 2, 1)
        d1 = [ops.conv_dgrad(d, w, (H, H), 2, 1) for d, w in zip(dmg, wmg)]
        dg = ops.conv_dgrad_g(dmg, wmg, (H, H), 2, 1)
        w1 = [ops.conv_wgrad(d, x, 2, 1) for d, x in zip(dyg, xg)]
        wgr = [kr() for _ in range(g)]
        ops.conv_wgrad_g(dyg, xg, 2, 1, wgr, False)
        sh1 = [kr() for _ in range(g // 2)]
        for z in range(g // 2):
            ops.conv_wgrad(dyg[2 * z], xg[2 * z], 2, 1, out=sh1[z], accumulate=False)
            ops.conv_wgrad(dyg[2 * z + 1], xg[2 * z + 1], 2, 1, out=sh1[z], accumulate=True)
        shg = [kr() for _ in range(g // 2)]
        ops.conv_wgrad_g(dyg, xg, 2, 1, [shg[i // 2] for i in range(g)], False, share=2)
        torch.cuda.synchronize()
    for i in range(g):
        same(yg[i], y1[i], f"forward, problem {i}")
        same(dg[i], d1[i], f"input gradient, problem {i}")
        same(wgr[i], w1[i], f"weight gradient, problem {i}")
    for z in range(g // 2):
        same(shg[z], sh1[z], f"shared weight gradient {z}")
    for op, got, a, b, n, ws in (("fwd", y1[g - 1], xs[g - 1], wl[g - 1], 16 * C, None), ("dgrad", d1[g - 1], dm[g - 1], wm[g - 1], 4 * C, None),
                                 ("wgrad", w1[g - 1], xs[g - 1], dys[g - 1], N * (H // 2) ** 2, wl[0].shape)):
        ref, absref = R.conv_ref(op, a, b, wshape=ws)
        R.assert_within(got, ref, absref, n, f"grouped shapes, single {op}", mult=mult)
        for wa, wb in R.wrong_problems(op, R.f64(a), R.f64(b)):
            R.assert_discriminates(R.conv_ref(op, wa, wb, wshape=ws)[0], ref, absref, n, f"grouped shapes {op}", mult=mult)


# ==== 10. Through the autograd modules ================================================================================
TRAINER_MODES = {"f32": dict(prec=ops.PREC_F32), "f32x3": dict(prec=ops.PREC_F32X3, x3=True), "bf16": dict(prec=ops.PREC_BF16, shadow=True),
                 "bf16_act16": dict(prec=ops.PREC_BF16, shadow=True, act16=True)}
STACK_N, STACK_S = 3, 32
# (kind, Cin, Cout, input height) of 3 -> 64 -> 96 -> 160 and back 160 -> 96 -> 64 -> 3 at 32 x 32
STACK = [("conv", 3, 64, 32), ("bn", 64, 64, 16), ("conv", 64, 96, 16), ("bn", 96, 96, 8), ("conv", 96, 160, 8), ("bn", 160, 160, 4),
         ("convT", 160, 96, 4), ("bn", 96, 96, 8), ("convT", 96, 64, 8), ("bn", 64, 64, 16), ("convT", 64, 3, 16)]


@functools.lru_cache(maxsize=None)
def stack_reference():
    """The float64 stack on the CPU: per layer its parameters, its input and the gradient arriving at its output."""
    torch.manual_seed(77)
    x = torch.rand(STACK_N, 3, STACK_S, STACK_S, dtype=torch.float64).requires_grad_(True)
    recs, h = [], x
    for i, (kind, ci, co, hin) in enumerate(STACK):
        if kind == "bn":
            p = (rnd(co, seed=100 + i).double() + 1.5, rnd(co, seed=200 + i).double())
            out = TF.batch_norm(h, None, None, p[0], p[1], True, 0.1, 1e-5)
        elif kind == "conv":
            p = (rnd(co, ci, 4, 4, seed=100 + i, scale=1.0 / math.sqrt(16 * ci)).double(),)
            out = TF.conv2d(h, p[0], stride=2, padding=1)
        else:
            p = (rnd(ci, co, 4, 4, seed=100 + i, scale=1.0 / math.sqrt(4 * ci)).double(),)
            out = TF.conv_transpose2d(h, p[0], stride=2, padding=1)
        out.retain_grad()
        recs.append([kind, p, h, out])
        h = out
    h.backward(rnd(*h.shape, seed=99).double())
    return [(kind, p, inp.detach(), out.grad.detach()) for kind, p, inp, out in recs]


def _conv_bounds(mode, op, geo, edge):
    """(operands rounded to bf16?, multiplier) of one conv op of the stack, from the plan queries."""
    L = _lib.load()
    if mode == "f32x3":
        return False, 8
    if mode.startswith("bf16") and not edge:
        return L.dg_conv_bf16_operands_ok(OPI[op], *geo, 2, 1) >= 1, 1
    return False, 1


@pytest.mark.parametrize("mode", list(TRAINER_MODES))
def test_module_stack_teacher_forced(mode):
    """model.Conv2d / ConvTranspose2d / BatchNorm2d, forward and backward in each trainer arithmetic, teacher-forced: every layer gets
    the fp32 (bf16 with bf16 feature maps) rounding of the float64 stack's input and upstream gradient, so the per-op bounds apply.
    With bf16 feature maps a layer whose reduction extent is not a multiple of 64 has no bf16 kernel for the bf16 map it is handed
    (forward of 96 -> 160, the transposed 160 -> 96 and 96 -> 64, the input gradient of 64 -> 96): the wrappers raise DiscoganHipError
    before any launch, which is pinned here (module route)."""
    act16 = mode == "bf16_act16"
    L = _lib.load()
    N = STACK_N
    for li, (kind, p, inp64, gout64) in enumerate(stack_reference()):
        _, ci, co, hin = STACK[li]
        edge = 3 in (ci, co)
        in16 = act16 and ci % 8 == 0 and not (kind == "conv" and ci == 3)
        g16 = act16 and co % 8 == 0 and co != 3
        rin = (lambda t: t.bfloat16().float()) if in16 else (lambda t: t.float())
        rg = (lambda t: t.bfloat16().float()) if g16 else (lambda t: t.float())
        inp, gout = rin(inp64), rg(gout64)
        what = f"stack {mode} layer {li} {kind} {ci}->{co}"
        ctx = ops.Context(**TRAINER_MODES[mode])
        with ops.use(ctx):
            if kind == "bn":
                bn = model.BatchNorm2d(co).to(DEV)
                with torch.no_grad():
                    bn.weight.copy_(p[0].float())
                    bn.bias.copy_(p[1].float())
                yg = nhwc(inp, torch.bfloat16 if in16 else torch.float32).requires_grad_(True)
                z = bn(yg)
                z.backward(nhwc(gout, torch.bfloat16 if g16 else torch.float32))
                torch.cuda.synchronize()
                ref = R.bn_ref(inp, p[0].float(), p[1].float(), gout, "none")
                o16 = z.dtype == torch.bfloat16
                assert o16 == (act16 and co % 8 == 0), what
                tol = R.bn_tol(ref["M"], o16)
                assert R.bn_violations(z, ref["z"], ref["sz"], tol, o16) == 0, what + ": z"
                assert R.bn_violations(yg.grad, ref["dx"], ref["sdx"], tol, yg.grad.dtype == torch.bfloat16) == 0, what + ": dx"
                assert R.violations(bn.weight.grad, ref["dgamma"], ref["sg"], ref["M"]) == 0, what + ": dgamma"
                assert R.violations(bn.bias.grad, ref["dbeta"], ref["sb"], ref["M"]) == 0, what + ": dbeta"
                assert R.bn_violations(R.bn_roll_channels(ref["z"]), ref["z"], ref["sz"], tol, o16) > 0, what + ": bound vacuous"
                ctx.clear()
                continue
            layer = (model.Conv2d if kind == "conv" else model.ConvTranspose2d)(ci, co).to(DEV)
            w32 = p[0].float()
            with torch.no_grad():
                layer.weight.copy_(w32.to(DEV))
            xin = (inp.to(DEV) if ci == 3 else nhwc(inp, torch.bfloat16 if in16 else torch.float32)).requires_grad_(True)
            gy = gout.to(DEV).contiguous() if co == 3 else nhwc(gout, torch.bfloat16 if g16 else torch.float32)
            # a bf16 feature map can only be read by a bf16 kernel: where the plan queries say the op has none (forward C % 64 != 0,
            # input gradient K % 64 != 0) the wrapper refuses BEFORE any launch -- in the forward, or in the backward for the gradient
            geo = (N, hin, hin, ci, co) if kind == "conv" else (N, 2 * hin, 2 * hin, co, ci)
            fop, bop = (0, 1) if kind == "conv" else (1, 0)
            if not edge and in16 and L.dg_conv_bf16_operands_ok(fop, *geo, 2, 1) == 0:
                assert (kind, ci, co) in (("conv", 96, 160), ("convT", 160, 96), ("convT", 96, 64)), what
                with pytest.raises(_lib.DiscoganHipError, match="no bf16 kernel for a bf16 (input|gradient)"):
                    layer(xin)
                ctx.clear()
                continue
            y = layer(xin)
            if not edge and g16 and L.dg_conv_bf16_operands_ok(bop, *geo, 2, 1) == 0:
                # the forward ran (bf16 in, bf16 out) and is checked below; the backward's input gradient is the refused op
                assert (kind, ci, co) == ("conv", 64, 96) and y.dtype == torch.bfloat16, what
                with pytest.raises(_lib.DiscoganHipError, match="no bf16 kernel for a bf16 (input|gradient)"):
                    y.backward(gy)
                dx = dw = None
            else:
                y.backward(gy)
                dx, dw = xin.grad, layer.weight.grad
                assert dx is not None and dw is not None, what
            torch.cuda.synchronize()
        ctx.clear()
        # the three ops of the layer in Conv2d geometry: a transposed conv's forward is the input gradient of Conv2d(co, ci) on the output
        if kind == "conv":
            C, K, H = ci, co, hin
            trip = (("fwd", y, inp, w32), ("dgrad", dx, gout, w32), ("wgrad", dw, inp, gout))
        else:
            C, K, H = co, ci, 2 * hin
            trip = (("dgrad", y, inp, w32), ("fwd", dx, gout, w32), ("wgrad", dw, gout, inp))
        assert trip[0][1] is y
        for op, got, a, b in trip:
            if got is None:                            # (the pinned refusal above: nothing was computed)
                continue
            rounded, mult = _conv_bounds(mode, op, (N, H, H, C, K), edge)
            if edge and mode.startswith("bf16"):
                # the 3 <-> 64 streaming forward kernel multiplies bf16 values on the bf16 path; the scatter input gradient and the weight
                # gradient do when their 64-channel operand is a bf16 feature map
                rounded = op == "fwd" or act16
            f = R.r16 if rounded else R.f64
            n = {"fwd": 16 * C, "dgrad": 4 * K, "wgrad": N * (H // 2) ** 2}[op]
            o16 = got.dtype == torch.bfloat16
            ref, absref = R.conv_ref(op, f(a), f(b), wshape=(K, C, 4, 4))
            R.assert_within(got, ref, absref, n, f"{what} {op}", mult=mult, out16=o16)
            for wa, wb in R.wrong_problems(op, f(a), f(b)):
                R.assert_discriminates(R.conv_ref(op, wa, wb, wshape=(K, C, 4, 4))[0], ref, absref, n, f"{what} {op}", mult=mult, out16=o16)
