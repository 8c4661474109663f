"""Kernels at shapes the model never makes: BatchNorm at channel counts that are not powers of two and at row counts on both
sides of the row-geometry rules, every conv family on non-square images, and real tensors on both sides of the 2 GiB
limits where the kernel choice changes.  Every result is compared with a float64 CPU reference of the same operation under
the elementwise bound of tests/shape_ref.py, every case asserts (with the plan queries) that it reached the kernel it is
about, and every case shows that the bound would catch a one-pixel shift or a channel mix-up."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, functional as F, model, ops  # noqa: E402
from tests import shape_ref as R  # noqa: E402
from tests.gpu_util import DEV, ambient, conv_operands, krsc, nhwc, options, with_shadow  # noqa: E402
from tests.shape_ref import rnd  # noqa: E402

ACTS = {"leaky": ops.ACT_LEAKY, "relu": ops.ACT_RELU, "none": ops.ACT_NONE}


# ==== 1. BatchNorm over channels and rows ============================================================================
BN_C = [4, 12, 100, 192, 320, 384, 448, 576, 960]
BN_ROWS = [(3, 5, 1), (1, 2, 6), (2, 4, 8)]          # M = 15 (M % 8 != 0, odd), 12 (M % 4 == 0 only), 64 (row-geometry kernels)


def _bn_forms(C, M):
    forms = ["f32"]
    if C % 8 == 0:
        forms += ["bf16", "shadow", "planes"]
        if C % 64 == 0 and M % 4 == 0:
            forms.append("planes_cm")
    return forms


BN_CASES = [(C, r, f) for C in BN_C for r in BN_ROWS for f in _bn_forms(C, r[0] * r[1] * r[2])]


def _bn_inputs(N, C, H, W, seed=1):
    y = rnd(N, C, H, W, seed=seed, scale=2.0) + 0.3
    return y, rnd(N, C, H, W, seed=seed + 3), rnd(C, seed=seed + 1) + 1.5, rnd(C, seed=seed + 2)


def _bn_check(ref, z, dx, dg, db, what, out16=False):
    tol = R.bn_tol(ref["M"], out16)
    assert R.bn_violations(z, ref["z"], ref["sz"], tol, out16) == 0, f"{what}: z"
    assert R.bn_dx_violations(dx, ref, tol, out16) == 0, f"{what}: dx"
    n = ref["M"]
    assert R.violations(dg, ref["dgamma"], ref["sg"], n) == 0, f"{what}: dgamma"
    assert R.violations(db, ref["dbeta"], ref["sb"], n) == 0, f"{what}: dbeta"
    # the bound tells a channel mix-up from the right answer
    assert R.bn_violations(R.bn_roll_channels(ref["z"]), ref["z"], ref["sz"], tol, out16) > 0, f"{what}: z bound vacuous"
    assert R.bn_violations(R.bn_roll_channels(ref["dx"]), ref["dx"], ref["sdx"], tol, out16) > 0, f"{what}: dx bound vacuous"


def _planes_value(t3, N, C, H, W, cm):
    """fp32 value held by a plane triple (hi + mid + lo), as logical NCHW."""
    v = t3.double().sum(0).cpu()
    M = N * H * W
    if cm:
        v = v.view(M // 4, C // 16, 4, 16).permute(0, 2, 1, 3).reshape(M, C)
    return v.view(N, H, W, C).permute(0, 3, 1, 2)


@pytest.mark.parametrize("C,rows,form", BN_CASES)
def test_batchnorm_channels_rows_forms(C, rows, form):
    """Training-mode BatchNorm + LeakyReLU / ReLU / none against fp64: statistics, running buffers, z, dx, dgamma, dbeta; fp32,
    bf16 storage, the bf16 shadow and plane triples in both layouts.  C = 192 / 320 / 384 / ... give the row-geometry kernels
    a ragged last channel chunk (M % 8 == 0); M % 8 != 0 stays on the item kernels."""
    N, H, W = rows
    M = N * H * W
    y, dz, gm, bt = _bn_inputs(N, C, H, W)
    io16 = form == "bf16"
    if io16:
        y, dz = y.bfloat16().float(), dz.bfloat16().float()
    yg, dzg = nhwc(y, torch.bfloat16 if io16 else torch.float32), nhwc(dz, torch.bfloat16 if io16 else torch.float32)
    gg, bg = gm.to(DEV), bt.to(DEV)
    rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
    saved = ops.bn_train_stats(yg, rm, rv, nbt, 1e-5, 0.1)
    for act in ("leaky", "relu", "none"):
        ref = R.bn_ref(y, gm, bt, dz, act)
        sc = ref["mean"].abs() + ref["var"].sqrt()
        if act == "leaky":
            assert int(nbt) == 1
            assert R.bn_violations(saved[0], ref["mean"], sc) == 0, "mean"
            assert R.bn_violations(rm, ref["rmean"], sc) == 0 and R.bn_violations(rv, ref["rvar"], ref["var"] + 1) == 0, "running stats"
        with ambient(shadow=form == "shadow", x3=form.startswith("planes")):
            cm = form == "planes_cm"
            z = ops.bn_act_fwd(yg, saved, gg, bg, ACTS[act], 0.2, planes_cm=cm)
            dx, dg, db = ops.bn_act_bwd(dzg, yg, saved, gg, bg, ACTS[act], 0.2, planes_cm=cm)
            torch.cuda.synchronize()
            what = f"BN C={C} M={M} {form} {act}"
            _bn_check(ref, z, dx, dg, db, what, out16=io16)
            if form == "shadow":
                z16, dx16 = ops._SHADOW_TAB[z.data_ptr()][1], ops._SHADOW_TAB[dx.data_ptr()][1]
                _bn_check(ref, z16, dx16, dg, db, what + " shadow", out16=True)
            if form.startswith("planes"):
                ez, edx = ops._PLANE_TAB[z.data_ptr()], ops._PLANE_TAB[dx.data_ptr()]
                assert bool(ez[2]) == cm and bool(edx[2]) == cm, "plane layout"
                zp, dxp = _planes_value(ez[1], N, C, H, W, cm), _planes_value(edx[1], N, C, H, W, cm)
                assert torch.equal(zp, R.f64(z)) and torch.equal(dxp, R.f64(dx)), f"{what}: planes hold the fp32 result"


@pytest.mark.parametrize("C", [12, 192, 320, 576])
def test_batchnorm_grouped_forms(C):
    """dg_bn_*_g with two problems (a discriminator's real and fake pass through one module: share = 2)."""
    N, H, W = 2, 4, 8
    ins = [_bn_inputs(N, C, H, W, seed=s) for s in (1, 11)]
    gm, bt = ins[0][2], ins[0][3]
    gg, bg = gm.to(DEV), bt.to(DEV)
    ys, dzs = [nhwc(i[0]) for i in ins], [nhwc(i[1]) for i in ins]
    saved = ops.bn_train_stats_g(ys, [None, None], [None, None], [None, None], 1e-5, 0.1)
    for act in ("leaky", "relu", "none"):
        refs = [R.bn_ref(i[0], gm, bt, i[1], act) for i in ins]
        zs = ops.bn_act_fwd_g(ys, saved, [gg, gg], [bg, bg], ACTS[act], 0.2)
        dgs, dbs = [torch.zeros(C, device=DEV)], [torch.zeros(C, device=DEV)]
        dxs = ops.bn_act_bwd_g(dzs, ys, saved, [gg, gg], [bg, bg], ACTS[act], 0.2, [dgs[0], dgs[0]], [dbs[0], dbs[0]], False, share=2)
        torch.cuda.synchronize()
        for p in range(2):
            assert R.bn_violations(zs[p], refs[p]["z"], refs[p]["sz"]) == 0, f"grouped z {p} C={C} {act}"
            assert R.bn_dx_violations(dxs[p], refs[p]) == 0, f"grouped dx {p} C={C} {act}"
        M = refs[0]["M"]
        assert R.violations(dgs[0], refs[0]["dgamma"] + refs[1]["dgamma"], refs[0]["sg"] + refs[1]["sg"], 2 * M) == 0, "shared dgamma"
        assert R.violations(dbs[0], refs[0]["dbeta"] + refs[1]["dbeta"], refs[0]["sb"] + refs[1]["sb"], 2 * M) == 0, "shared dbeta"


@pytest.mark.parametrize("form", ["f32", "bf16", "planes_cm"])
def test_batchnorm_many_rows(form):
    """M = 10 x 128 x 128 = 163840 rows at C = 192: bn_grid's cap of 512 row chunks and bn_rows' 4096 / cchunks cap both bind,
    with the ragged channel chunk of C = 192."""
    N, C, H, W = 10, 192, 128, 128
    y, dz, gm, bt = _bn_inputs(N, C, H, W, seed=21)
    io16 = form == "bf16"
    if io16:
        y, dz = y.bfloat16().float(), dz.bfloat16().float()
    dt = torch.bfloat16 if io16 else torch.float32
    yg, dzg, gg, bg = nhwc(y, dt), nhwc(dz, dt), gm.to(DEV), bt.to(DEV)
    ref = R.bn_ref(y, gm, bt, dz, "leaky")
    with ambient(x3=form == "planes_cm"):
        saved = ops.bn_train_stats(yg, None, None, None, 1e-5, 0.1)
        z = ops.bn_act_fwd(yg, saved, gg, bg, ops.ACT_LEAKY, 0.2, planes_cm=True)
        dx, dg, db = ops.bn_act_bwd(dzg, yg, saved, gg, bg, ops.ACT_LEAKY, 0.2, planes_cm=True)
        torch.cuda.synchronize()
        _bn_check(ref, z, dx, dg, db, f"BN many rows {form}", out16=io16)
        if form == "planes_cm":
            zp = _planes_value(ops._PLANE_TAB[z.data_ptr()][1], N, C, H, W, True)
            assert torch.equal(zp, R.f64(z))


@pytest.mark.parametrize("C", [192, 320])
def test_batchnorm_module_autograd(C):
    """The public model.BatchNorm2d(C) forward and backward through autograd against torch.nn.BatchNorm2d in float64."""
    N, H, W = 4, 4, 8
    y, dz, gm, bt = _bn_inputs(N, C, H, W, seed=31)
    ref_bn = torch.nn.BatchNorm2d(C).double()
    bn = model.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        ref_bn.weight.copy_(gm)
        ref_bn.bias.copy_(bt)
        bn.weight.copy_(gm)
        bn.bias.copy_(bt)
    yr = y.double().requires_grad_(True)
    zr = ref_bn(yr)
    zr.backward(dz.double())
    yg = nhwc(y).requires_grad_(True)
    z = bn(yg)
    z.backward(nhwc(dz))
    torch.cuda.synchronize()
    ref = R.bn_ref(y, gm, bt, dz, "none")
    assert R.bn_violations(z, zr.detach(), ref["sz"]) == 0
    assert R.bn_violations(yg.grad, yr.grad, ref["sdx"]) == 0          # (no activation: no kink)
    assert R.violations(bn.weight.grad, ref_bn.weight.grad, ref["sg"], ref["M"]) == 0
    assert R.violations(bn.bias.grad, ref_bn.bias.grad, ref["sb"], ref["M"]) == 0
    sc = ref["mean"].abs() + ref["var"].sqrt()
    assert R.bn_violations(bn.running_mean, ref_bn.running_mean, sc) == 0
    assert R.bn_violations(bn.running_var, ref_bn.running_var, ref["var"] + 1) == 0
    assert int(bn.num_batches_tracked) == 1


# ==== 2. Non-square images on every conv path =========================================================================
# form -> (N, C, K, H, W) shapes; each reaches the kernel named in the comment (asserted from the plan queries below)
CONV_CASES = [
    ("f32", (2, 64, 128, 8, 32)), ("f32", (3, 64, 128, 32, 8)), ("f32", (2, 64, 128, 2, 64)), ("f32", (1, 64, 128, 64, 2)),
    ("ptr", (2, 64, 128, 8, 32)), ("ptr", (1, 64, 128, 64, 2)),                       # 64-bit pointer kernels (option pointer_path)
    ("bf16op", (2, 64, 128, 8, 32)), ("bf16op", (1, 64, 128, 64, 2)),                 # register-staged bf16 tiles
    ("dma", (4, 256, 256, 16, 64)), ("dma", (4, 256, 256, 64, 16)),                   # LDS-DMA bf16 kernel, all three ops
    ("bf16dgw", (2, 64, 128, 16, 128)),                                               # bf16 window input gradient (Wo = 64)
    ("bf16io", (3, 128, 256, 8, 32)), ("bf16io", (2, 128, 256, 128, 16)),             # bf16 feature maps in and out
    ("x3", (4, 192, 256, 16, 64)), ("x3", (4, 192, 256, 64, 16)),                     # f32x3 plane kernel, all three ops
    ("x3dgw", (2, 64, 128, 16, 128)),                                                 # f32x3 window input gradient
]


def _conv_kernel_asserts(form, N, C, K, H, W):
    L = _lib.load()
    bq = [L.dg_conv_bf16_operands_ok(op, N, H, W, C, K, 2, 1) for op in range(3)]
    xq = [L.dg_conv_x3_planes_ok(op, N, H, W, C, K, 2, 1) for op in range(3)]
    if form == "bf16op":
        assert min(bq) >= 1, bq
    elif form == "dma":
        assert bq == [2, 2, 2], bq
    elif form == "bf16dgw":
        assert bq[1] == 2 and W // 2 >= 32, bq
    elif form == "bf16io":
        assert bq[0] == 2 and bq[2] == 2, bq
    elif form == "x3":
        assert xq == [1, 1, 1], xq
    elif form == "x3dgw":
        assert xq[1] == 2, xq
    else:
        assert all(L.dg_conv_plan_splits_p(op, N, H, W, C, K, 2, 1, ops.PREC_F32, 1) >= 1 for op in range(3))


@pytest.mark.parametrize("form,shape", CONV_CASES, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in CONV_CASES])
def test_conv_non_square(form, shape):
    N, C, K, H, W = shape
    Ho, Wo = H // 2, W // 2
    x, w, dy = rnd(N, C, H, W, seed=1), rnd(K, C, 4, 4, seed=2, scale=1.0 / math.sqrt(16 * C)), rnd(N, K, Ho, Wo, seed=3)
    _conv_kernel_asserts(form, N, C, K, H, W)
    bf = form in ("bf16op", "dma", "bf16dgw", "bf16io")
    opnd = R.r16 if bf else R.f64
    mult = 8 if form.startswith("x3") else 1
    out16 = form == "bf16io"
    prec = {"x3": 2, "x3dgw": 2}.get(form, 1 if bf else 0)
    with options(bf16=prec, pointer_path=int(form == "ptr")), ambient(shadow=form in ("dma", "bf16dgw", "bf16io"), act16=out16,
                                                                        x3=form.startswith("x3")):
        shadowed = form in ("dma", "bf16dgw")
        xg, wg, dyg = conv_operands(x, w, dy, act16=out16, shadow_x=shadowed, shadow_dy=shadowed, shadow_w=bf)
        y = ops.conv_fwd(xg, wg, 2, 1)
        dx = ops.conv_dgrad(dyg, wg, (H, W), 2, 1)
        dw = ops.conv_wgrad(dyg, xg, 2, 1)
        torch.cuda.synchronize()
        assert (y.dtype == torch.bfloat16) == out16 and (dx.dtype == torch.bfloat16) == out16
    for op, got, a, b, n, o16 in (("fwd", y, x, w, R.taps("fwd", C, K), out16), ("dgrad", dx, dy, w, R.taps("dgrad", C, K), out16),
                                  ("wgrad", dw, x, dy, N * Ho * Wo, False)):
        ref, absref = R.conv_ref(op, opnd(a), opnd(b), wshape=w.shape)
        R.assert_within(got, ref, absref, n, f"{form} {op} {shape}", mult=mult, out16=o16)
        for wa in R.shifted(opnd(a)):
            wrong, _ = R.conv_ref(op, wa, opnd(b), wshape=w.shape)
            R.assert_discriminates(wrong, ref, absref, n, f"{form} {op} {shape}", mult=mult, out16=o16)


@pytest.mark.parametrize("N,Cin,Cout,Hin,Win", [(2, 128, 64, 4, 16), (3, 64, 128, 16, 2), (1, 256, 128, 2, 32)])
def test_conv_transpose_non_square(N, Cin, Cout, Hin, Win):
    """ConvTranspose2d(Cin, Cout, 4, 2, 1) through the autograd Function: forward = the stride-2 input-gradient kernel, input
    gradient = the forward kernel, weight gradient with the roles swapped."""
    x, w, dy = rnd(N, Cin, Hin, Win, seed=1), rnd(Cin, Cout, 4, 4, seed=2, scale=1.0 / math.sqrt(16 * Cout)), rnd(N, Cout, 2 * Hin, 2 * Win, seed=3)
    xg, wg = nhwc(x).requires_grad_(True), krsc(w).requires_grad_(True)
    y = F.ConvTransposeFn.apply(xg, wg, 2, 1)
    y.backward(nhwc(dy))
    torch.cuda.synchronize()
    for op, got, a, b, n in (("dgrad", y, x, w, 4 * Cin), ("fwd", xg.grad, dy, w, 16 * Cout), ("wgrad", wg.grad, dy, x, N * Hin * Win)):
        ref, absref = R.conv_ref(op, a, b, wshape=w.shape)
        R.assert_within(got, ref, absref, n, f"convT {op}")
        wrong, _ = R.conv_ref(op, R.shift_w(R.f64(a)), b, wshape=w.shape)
        R.assert_discriminates(wrong, ref, absref, n, f"convT {op}")


@pytest.mark.parametrize("N,C,K,H,W", [(2, 64, 128, 8, 32), (3, 64, 128, 32, 8), (2, 128, 64, 4, 64)])
def test_conv_fused_bn_statistics_non_square(N, C, K, H, W):
    """want_stats: the BatchNorm statistics from the conv epilogue (forward and stride-2 input gradient) against the fp64
    statistics of the fp64 reference output."""
    x, w, dy = rnd(N, C, H, W, seed=1) + 0.4, rnd(K, C, 4, 4, seed=2, scale=1.0 / math.sqrt(16 * C)), rnd(N, K, H // 2, W // 2, seed=3) + 0.2
    xg, wg, dyg = nhwc(x), krsc(w), nhwc(dy)
    for op, (out, st), a, ch in (("fwd", ops.conv_fwd(xg, wg, 2, 1, want_stats=True), x, K),
                                 ("dgrad", ops.conv_dgrad(dyg, wg, (H, W), 2, 1, want_stats=True), dy, C)):
        assert st is not None and st.shape[1] == 3 * ch + 4, op
        saved = ops.bn_stats_from_partials(st, out, None, None, None, 1e-5, 0.1)
        ref, absref = R.conv_ref(op, a, w)
        R.assert_within(out, ref, absref, R.taps(op, C, K), f"want_stats {op} output")
        mean, var = ref.mean((0, 2, 3)), ref.var((0, 2, 3), unbiased=False)
        sc = mean.abs() + var.sqrt()
        assert R.bn_violations(saved[0], mean, sc) == 0, f"{op} mean"
        assert R.bn_violations(1.0 / saved[1].double() ** 2 - 1e-5, var, var) == 0, f"{op} var"
        assert R.bn_violations(R.conv_ref(op, R.shift_w(R.f64(a)), w)[0].mean((0, 2, 3)), mean, sc) > 0, f"{op}: bound vacuous"


C3_NS = [(2, 8, 32), (2, 32, 8), (1, 2, 64), (1, 64, 2), (1, 16, 128)]
C3_MODES = ["f32", "f32x3", "bf16_mfma", "bf16_storage"]


@pytest.mark.parametrize("N,H,W", C3_NS)
@pytest.mark.parametrize("mode", C3_MODES)
def test_c3_edge_non_square(N, H, W, mode):
    """conv1 (3 -> 64, + LeakyReLU), its input gradient (scatter form; gather form with option kt 16; the VALU form at K = 32)
    and weight gradient (plain and with the LeakyReLU backward fused), and the fused-activation input gradient, in all four
    arithmetic forms."""
    K, Ho, Wo = 64, H // 2, W // 2
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(1))
    w = rnd(K, 3, 4, 4, seed=2, scale=0.2)
    dy = rnd(N, K, Ho, Wo, seed=3)
    b16 = mode.startswith("bf16")
    dt = torch.bfloat16 if b16 else torch.float32
    if b16:
        dy = dy.bfloat16().float()
    mult = 8 if mode == "f32x3" else 1
    rx = R.r16 if mode == "bf16_mfma" else R.f64                 # what the bf16 MFMA multiplies: rounded image and weights
    xg, wg, dyg = x.to(DEV), w.to(DEV), nhwc(dy, dt)
    with options(bf16={"f32": 0, "f32x3": 2, "bf16_mfma": 1, "bf16_storage": 0}[mode]), ambient(act16=b16):
        y = ops.c3_fwd(xg, wg, ops.ACT_LEAKY, 0.2)
        assert (y.dtype == torch.bfloat16) == b16
        assert ops.c3_dgrad_act_ok(K, N, H, W, b16)
        dx = ops.c3_dgrad(dyg, wg, ops.ACT_NONE)
        dxa = ops.c3_dgrad(dyg, wg, ops.ACT_NONE, act_out=y, in_act=ops.ACT_LEAKY, slope=0.2)
        dxu = ops.c3_dgrad(ops.act_bwd(dyg, y, ops.ACT_LEAKY, 0.2), wg, ops.ACT_NONE)
        dw = ops.c3_wgrad(dyg, xg)
        dwa = ops.c3_wgrad(dyg, xg, act_out=y, act=ops.ACT_LEAKY, slope=0.2)
        torch.cuda.synchronize()
    what = f"c3 {mode} {N}x{H}x{W}"
    ref, absref = R.conv_ref("fwd", rx(x), rx(w))
    R.assert_within(y, torch.nn.functional.leaky_relu(ref, 0.2), absref, 49, what + " fwd", out16=b16)
    R.assert_discriminates(torch.nn.functional.leaky_relu(R.conv_ref("fwd", R.shift_w(rx(x)), rx(w))[0], 0.2),
                           torch.nn.functional.leaky_relu(ref, 0.2), absref, 49, what + " fwd", out16=b16)
    ref, absref = R.conv_ref("dgrad", dy, rx(w))
    R.assert_within(dx, ref, absref, R.taps("dgrad", 3, K), what + " dgrad", mult=mult)
    R.assert_discriminates(R.conv_ref("dgrad", R.shifted(R.f64(dy))[0], rx(w))[0], ref, absref, R.taps("dgrad", 3, K), what + " dgrad", mult=mult)
    assert torch.equal(dxa, dxu), what + ": fused activation backward vs act_bwd + input gradient"
    ga = R.f64(dy) * torch.where(R.f64(y) > 0, 1.0, 0.2)
    if b16:
        ga = ga.bfloat16().double()                               # the stand-alone pass stores g in bf16
    ref, absref = R.conv_ref("dgrad", ga, rx(w))
    R.assert_within(dxa, ref, absref, R.taps("dgrad", 3, K) + 1, what + " dgrad act", mult=mult)
    ref, absref = R.conv_ref("wgrad", rx(x), dy, wshape=w.shape)
    R.assert_within(dw, ref, absref, N * Ho * Wo, what + " wgrad", mult=mult)
    R.assert_discriminates(R.conv_ref("wgrad", R.shift_w(rx(x)), dy, wshape=w.shape)[0], ref, absref, N * Ho * Wo, what + " wgrad", mult=mult)
    ga = R.f64(dy) * torch.where(R.f64(y) > 0, 1.0, 0.2)
    ref, absref = R.conv_ref("wgrad", rx(x), ga, wshape=w.shape)
    if b16:
        absref = absref * (1 + R.U16 / R.gamma(mult * (N * Ho * Wo + 1)))   # g = dy * act' may be rounded to bf16 once more
    R.assert_within(dwa, ref, absref, N * Ho * Wo + 1, what + " wgrad act", mult=mult)


@pytest.mark.parametrize("N,H,W", [(2, 8, 32), (1, 64, 2)])
def test_c3_gather_and_valu_forms_non_square(N, H, W):
    """The older gather form (option kt 16) at K = 64, and the VALU form (K = 32: neither MFMA form takes it)."""
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(1))
    for K in (64, 32):
        w, dy = rnd(K, 3, 4, 4, seed=2, scale=0.2), rnd(N, K, H // 2, W // 2, seed=3)
        with options(kt=16 if K == 64 else 0):
            assert not ops.c3_dgrad_act_ok(K, N, H, W)
            dx = ops.c3_dgrad(nhwc(dy), w.to(DEV), ops.ACT_NONE)
            dw = ops.c3_wgrad(nhwc(dy), x.to(DEV)) if K == 64 else None          # (the weight gradient takes K % 64 == 0)
            y = ops.c3_fwd(x.to(DEV), w.to(DEV), ops.ACT_NONE)
            torch.cuda.synchronize()
        ref, absref = R.conv_ref("dgrad", dy, w)
        R.assert_within(dx, ref, absref, 4 * K, f"c3 dgrad K={K}")
        R.assert_discriminates(R.conv_ref("dgrad", R.shifted(R.f64(dy))[0], w)[0], ref, absref, 4 * K, f"c3 dgrad K={K}")
        if dw is not None:
            ref, absref = R.conv_ref("wgrad", x, dy, wshape=w.shape)
            R.assert_within(dw, ref, absref, N * (H // 2) * (W // 2), f"c3 wgrad K={K}")
        ref, absref = R.conv_ref("fwd", x, w)
        R.assert_within(y, ref, absref, 48, f"c3 fwd K={K}")


@pytest.mark.parametrize("prec", [ops.PREC_F32, ops.PREC_F32X3])
def test_grouped_forms_non_square(prec):
    """The _g entry points with two problems of a non-square shape: interior convs and the three edge ops."""
    N, C, K, H, W = 2, 64, 128, 8, 32
    mult = 8 if prec == ops.PREC_F32X3 else 1
    xs = [rnd(N, C, H, W, seed=1 + i) for i in range(2)]
    wl = [rnd(K, C, 4, 4, seed=3 + i, scale=1.0 / math.sqrt(16 * C)) for i in range(2)]
    dys = [rnd(N, K, H // 2, W // 2, seed=5 + i) for i in range(2)]
    ctx = ops.Context(prec=prec)
    with ops.use(ctx):
        ys = ops.conv_fwd_g([nhwc(t) for t in xs], [krsc(t) for t in wl], 2, 1)
        dxs = ops.conv_dgrad_g([nhwc(t) for t in dys], [krsc(t) for t in wl], (H, W), 2, 1)
        dws = [torch.zeros(K, C, 4, 4, device=DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for _ in range(2)]
        ops.conv_wgrad_g([nhwc(t) for t in dys], [nhwc(t) for t in xs], 2, 1, dws, False)
        im = [torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(9 + i)) for i in range(2)]
        w3 = [rnd(64, 3, 4, 4, seed=11 + i, scale=0.2) for i in range(2)]
        d3 = [rnd(N, 64, H // 2, W // 2, seed=13 + i) for i in range(2)]
        y3 = ops.c3_fwd_g([t.to(DEV) for t in im], [t.to(DEV) for t in w3], ops.ACT_NONE)
        dx3 = ops.c3_dgrad_g([nhwc(t) for t in d3], [t.to(DEV) for t in w3], ops.ACT_NONE)
        dw3 = [torch.zeros(64, 3, 4, 4, device=DEV) for _ in range(2)]
        ops.c3_wgrad_g([nhwc(t) for t in d3], [t.to(DEV) for t in im], dw3, False)
        torch.cuda.synchronize()
    for i in range(2):
        for op, got, a, b, n, ws in (("fwd", ys[i], xs[i], wl[i], 16 * C, None), ("dgrad", dxs[i], dys[i], wl[i], 4 * K, None),
                                     ("wgrad", dws[i], xs[i], dys[i], N * (H // 2) * (W // 2), wl[i].shape),
                                     ("fwd", y3[i], im[i], w3[i], 48, None), ("dgrad", dx3[i], d3[i], w3[i], 256, None),
                                     ("wgrad", dw3[i], im[i], d3[i], N * (H // 2) * (W // 2), w3[i].shape)):
            ref, absref = R.conv_ref(op, a, b, wshape=ws)
            R.assert_within(got, ref, absref, n, f"grouped {op} problem {i}", mult=mult)
            R.assert_discriminates(R.conv_ref(op, R.shifted(R.f64(a))[0], b, wshape=ws)[0], ref, absref, n, f"grouped {op} {i}", mult=mult)


# ==== 3. Real sizes on both sides of each threshold ==================================================================
def _filled(N, per_image_bytes):
    """Image 0, the first image whose bytes start at or past 2^31 (or the middle one if there is none), the last image."""
    first = -(-(1 << 31) // per_image_bytes)
    return sorted({0, first if first < N else N // 2, N - 1})


def _big(N, C, H, W, idx, seed, patch):
    """Zeros on the device in NHWC memory, with a random patch of `patch` rows and columns in the listed images."""
    t = torch.zeros((N, H, W, C), device=DEV).permute(0, 3, 1, 2)
    small = torch.zeros(len(idx), C, H, W)
    r0, c0 = H // 4 + 1, W // 4 + 1
    small[:, :, r0:r0 + patch, c0:c0 + patch] = rnd(len(idx), C, patch, patch, seed=seed)
    t[idx] = small.to(DEV)
    return t, small


def _zero_except(t, idx, what):
    per = t.detach().abs().amax(dim=(1, 2, 3)).float().cpu()
    mask = torch.ones(per.numel(), dtype=torch.bool)
    mask[idx] = False
    assert float(per[mask].max()) == 0.0, f"{what}: an image that holds zeros has a nonzero result"


@pytest.mark.parametrize("form,N", [("f32", 32767), ("f32", 32769), ("bf16", 65535), ("bf16", 65537), ("x3", 65535), ("x3", 65537)])
def test_conv_operands_across_2gib(form, N):
    """Interior stride-2 conv at 16 x 16, C = 64, K = 256: x and dy are N x 64 KiB of fp32.  fp32 crosses 2^31 bytes between
    N = 32767 and 32769; the bf16 shadow and the f32x3 planes count bf16 bytes per plane, so they cross between 65535 and
    65537 (4 GiB of fp32), where the plan drops the buffer descriptors and the bf16 / f32x3 kernels for the fp32 pointer
    kernels.  Zero images give exact zeros, the filled images the fp64 result of those images alone."""
    C, K, H, W = 64, 256, 16, 16
    L = _lib.load()
    over = N * H * W * C * 4 >= (1 << 32 if form != "f32" else 1 << 31)
    if form == "bf16":
        assert [L.dg_conv_bf16_operands_ok(op, N, H, W, C, K, 2, 1) for op in range(3)] == ([0, 0, 0] if over else [2, 1, 2])
    if form == "x3":
        assert [L.dg_conv_x3_planes_ok(op, N, H, W, C, K, 2, 1) for op in range(3)] == ([0, 0, 0] if over else [1, 0, 1])
    idx = _filled(N, H * W * C * (2 if form != "f32" else 4))
    w = rnd(K, C, 4, 4, seed=2, scale=1.0 / math.sqrt(16 * C))
    mult = 8 if (form == "x3" and not over) else 1
    opnd = R.r16 if (form == "bf16" and not over) else R.f64
    prec = {"f32": 0, "bf16": 1, "x3": 2}[form]
    with options(bf16=prec), ambient(shadow=form == "bf16", x3=form == "x3"):
        wg = krsc(w)
        if form == "bf16":
            with_shadow(wg)
        for op in ("fwd", "dgrad", "wgrad"):
            if op == "fwd":
                a, a_small = _big(N, C, H, W, idx, 5, 6)
                if form == "bf16":
                    with_shadow(a)
                out = ops.conv_fwd(a, wg, 2, 1)
                got, (ref, absref), n = out[idx], R.conv_ref("fwd", opnd(a_small), opnd(w)), 16 * C
                wrong = R.conv_ref("fwd", R.shift_w(opnd(a_small)), opnd(w))[0]
            elif op == "dgrad":
                a, a_small = _big(N, K, H // 2, W // 2, idx, 6, 3)
                if form == "bf16":
                    with_shadow(a)
                out = ops.conv_dgrad(a, wg, (H, W), 2, 1)
                got, (ref, absref), n = out[idx], R.conv_ref("dgrad", opnd(a_small), opnd(w)), 4 * K
                wrong = R.conv_ref("dgrad", R.shift_w(opnd(a_small)), opnd(w))[0]
            else:
                if form == "x3":      # (x and dy as plane triples would need 20 GB: dy of 64 channels crosses nothing, x does)
                    break
                xb, x_small = _big(N, C, H, W, idx, 5, 6)
                dyb, dy_small = _big(N, K, H // 2, W // 2, idx, 6, 3)
                if form == "bf16":
                    with_shadow(xb)
                    with_shadow(dyb)
                got, a = ops.conv_wgrad(dyb, xb, 2, 1), None
                n = len(idx) * 9
                ref, absref = R.conv_ref("wgrad", opnd(x_small), opnd(dy_small), wshape=w.shape)
                wrong = R.conv_ref("wgrad", R.shift_w(opnd(x_small)), opnd(dy_small), wshape=w.shape)[0]
                del xb, dyb
            torch.cuda.synchronize()
            if op != "wgrad":
                _zero_except(out, idx, f"{form} N={N} {op}")
                del out
            R.assert_within(got, ref, absref, n, f"{form} N={N} {op}", mult=mult)
            R.assert_discriminates(wrong, ref, absref, n, f"{form} N={N} {op}", mult=mult)
            del a, got
            ops.shadow_clear()
            ops.planes_clear()
            torch.cuda.empty_cache()


@pytest.mark.parametrize("mode,N", [("f32", 127), ("f32", 128), ("f32x3", 127), ("f32x3", 128), ("bf16", 255), ("bf16", 256)])
def test_conv1_across_the_scatter_limit(mode, N):
    """functional.ConvC3Fn (conv1 + LeakyReLU) forward and backward at 512 px.  The fp32 dy of N x 16 MiB crosses the scatter
    kernel's 2^31 bytes between N = 127 and 128; a bf16 dy (bf16 feature maps) between 255 and 256.  Past it the input gradient
    takes the stand-alone activation backward and the VALU kernel (a bf16 dy as an fp32 copy).  Both sides: fp64 reference on
    the filled images, exact zeros elsewhere, and the fused result equal to the unfused one."""
    S, K = 512, 64
    b16 = mode == "bf16"
    fused = ops.c3_dgrad_act_ok(K, N, S, S, b16)
    assert fused == (N * (S // 2) ** 2 * K * (2 if b16 else 4) < (1 << 31))
    idx = _filled(N, (S // 2) ** 2 * K * (2 if b16 else 4))
    w = rnd(K, 3, 4, 4, seed=2, scale=0.2)
    ctx = ops.Context(prec=ops.PREC_F32X3 if mode == "f32x3" else ops.PREC_F32, act16=b16)
    mult = 8 if mode == "f32x3" else 1
    x = torch.zeros(N, 3, S, S, device=DEV)
    x_small = torch.zeros(len(idx), 3, S, S)
    x_small[:, :, 200:216, 300:316] = torch.rand(len(idx), 3, 16, 16, generator=torch.Generator().manual_seed(1))
    x[idx] = x_small.to(DEV)
    dy = torch.zeros((N, S // 2, S // 2, K), device=DEV, dtype=torch.bfloat16 if b16 else torch.float32).permute(0, 3, 1, 2)
    dy_small = torch.zeros(len(idx), K, S // 2, S // 2)
    dy_small[:, :, 100:108, 150:158] = rnd(len(idx), K, 8, 8, seed=3)
    if b16:
        dy_small = dy_small.bfloat16().float()
    dy[idx] = dy_small.to(DEV, dy.dtype)
    wp = w.to(DEV).requires_grad_(not b16)       # (the bf16 weight gradient refuses a dy of 1 GiB and more: an explicit limit)
    xr = x.requires_grad_(True)
    with ops.use(ctx):
        y = F.ConvC3Fn.apply(xr, wp, ops.ACT_LEAKY, 0.2)
        assert (y.dtype == torch.bfloat16) == b16
        y.backward(dy)
        torch.cuda.synchronize()
        dx_unfused = ops.c3_dgrad(ops.act_bwd(ops.as_nhwc(dy), y.detach(), ops.ACT_LEAKY, 0.2), wp.detach(), ops.ACT_NONE) if fused else None
        torch.cuda.synchronize()
    what = f"conv1 {mode} N={N}"
    _zero_except(y, idx, what + " forward")
    _zero_except(xr.grad, idx, what + " input gradient")
    if dx_unfused is not None:
        assert torch.equal(xr.grad, dx_unfused), what + ": fused input gradient vs act_bwd + unfused"
        del dx_unfused
    y_small = y.detach()[idx].float().cpu()
    ref, absref = R.conv_ref("fwd", x_small, w)
    R.assert_within(y_small, torch.nn.functional.leaky_relu(ref, 0.2), absref, 49, what + " forward", mult=mult, out16=b16)
    R.assert_discriminates(torch.nn.functional.leaky_relu(R.conv_ref("fwd", R.shift_w(R.f64(x_small)), w)[0], 0.2),
                           torch.nn.functional.leaky_relu(ref, 0.2), absref, 49, what + " forward", mult=mult, out16=b16)
    g = R.f64(dy_small) * torch.where(R.f64(y_small) > 0, 1.0, 0.2)
    if b16:
        g = g.bfloat16().double()                                 # the activation backward of a bf16 gradient stores bf16
    ref, absref = R.conv_ref("dgrad", g, w)
    R.assert_within(xr.grad[idx], ref, absref, 4 * K + 1, what + " input gradient", mult=1 if not fused else mult)
    R.assert_discriminates(R.conv_ref("dgrad", R.shift_w(g), w)[0], ref, absref, 4 * K + 1, what + " input gradient", mult=mult)
    if not b16:
        nz = int((g != 0).any(1).sum())
        ref, absref = R.conv_ref("wgrad", x_small, g, wshape=w.shape)
        if b16:
            absref = absref * (1 + R.U16 / R.gamma(mult * (nz + 1)))     # the fused form may take g = dy * act' unrounded
        R.assert_within(wp.grad, ref, absref, nz + 1, what + " weight gradient", mult=mult)
        R.assert_discriminates(R.conv_ref("wgrad", R.shift_w(R.f64(x_small)), g, wshape=w.shape)[0], ref, absref, nz + 1, what + " weight gradient",
                               mult=mult)
    del x, xr, dy, y, wp
    torch.cuda.empty_cache()
