"""The generators' last group [BatchNorm2d(64)][ReLU][ConvTranspose2d(64, 3)][Sigmoid] with the BatchNorm apply inside the 3-channel
kernels (ops.c3_dgrad_bn / ops.c3_wgrad_bn, functional.BatchNormActConvTransposeC3Fn) against the same group with the apply pass in
front: every comparison is bitwise, on both arithmetics that have the form (exact fp32 and f32x3).

Shapes.  The 3-channel entry points take power-of-two images only (the reference side of each comparison, ops.c3_dgrad / ops.c3_wgrad,
refuses anything else), so the ragged cases are the power-of-two ones that are ragged against the scatter kernel's 6 x 14 pixel tile:
(2, 8, 16) two row tiles and two column tiles, the last of each partly outside; (1, 16, 32) three by three tiles, ragged both ways;
(3, 4, 8) one tile per image (tile index = image index), partly outside on both sides; (9, 32, 64) 1080 tiles on a grid of 512, so
that both register sets and the second trip of the tile loop run.  The weight gradient runs its two kernels: the exact-fp32 MFMA
kernel (rows under 256 pixels, and every row in exact fp32) and the LDS kernel of the f32x3 path in its plain (W = 256) and its deep
(W = 512) loop.  A build with the scatter kernel's padding select taken out fails every forward case on its first border assertion."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, model, ops  # noqa: E402
from tests.gpu_util import DEV, nhwc, options  # noqa: E402
from tests.shape_ref import rnd  # noqa: E402

K = 64
ARITH = {"f32": dict(prec=ops.PREC_F32), "f32x3": dict(prec=ops.PREC_F32X3, x3=True)}


def _ctx(arith):
    return ops.use(ops.Context(**ARITH[arith]))


def _bn_params(seed, big_beta=False):
    """saved = [mean | invstd], gamma, beta on the device.  big_beta: large positive entries -- relu(bn(0)) is then at least 8 on
    every channel, so a padding pixel taken through the transform changes the border outputs."""
    mean, var = rnd(K, seed=seed) * 0.5, rnd(K, seed=seed + 1).abs() + 0.25
    invstd = torch.rsqrt(var + 1e-5)
    gamma = rnd(K, seed=seed + 2) + 1.5
    beta = rnd(K, seed=seed + 3)
    if big_beta:
        beta = beta.abs() * 4.0 + 8.0 + (mean * gamma * invstd).abs()
    return torch.stack([mean, invstd]).to(DEV), gamma.to(DEV), beta.to(DEV)


class _count_calls:
    """Calls of one library entry point inside the block."""

    def __init__(self, name):
        self.name, self.n = name, 0

    def __enter__(self):
        L = _lib.load()
        self.fn = fn = getattr(L, self.name)

        def wrapped(*a):
            self.n += 1
            return fn(*a)

        setattr(L, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(_lib.load(), self.name, self.fn)
        return False


# ==== 1. forward: the scatter kernel ===================================================================================
@pytest.mark.parametrize("arith", list(ARITH))
@pytest.mark.parametrize("shape", [(2, 8, 16), (1, 16, 32), (3, 4, 8), (9, 32, 64)])
def test_forward_bitwise(arith, shape):
    N, Ho, Wo = shape
    y = nhwc(rnd(N, K, Ho, Wo, seed=11, scale=2.0) + 0.3)
    w = (rnd(K, 3, 4, 4, seed=12) * 0.1).to(DEV)
    saved, gamma, beta = _bn_params(13, big_beta=True)
    with _ctx(arith):
        assert ops.c3_tail_bn_ok(y, need_wgrad=False)
        z = ops.bn_act_fwd(y, saved, gamma, beta, ops.ACT_RELU)
        assert float((beta - saved[0] * gamma * saved[1]).min()) >= 7.9, "relu(bn(0)) is not large on every channel"
        ref = ops.c3_dgrad(z, w, ops.ACT_SIGMOID)
        ref_raw = ops.c3_dgrad(z, w, ops.ACT_NONE)
        got = torch.full_like(ref, float("nan"))
        _lib.check(_lib.load().dg_conv4x4s2_c3_dgrad_bn_p(y.data_ptr(), saved.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ops.ACT_RELU,
                                                          w.data_ptr(), got.data_ptr(), N, 2 * Ho, 2 * Wo, K, ops.ACT_SIGMOID,
                                                          ops.current().cprec, torch.cuda.current_stream().cuda_stream),
                   "dg_conv4x4s2_c3_dgrad_bn_p")
        got_raw = ops.c3_dgrad_bn(y, saved, gamma, beta, w, ops.ACT_NONE)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all(), "an output element was not written"
    # the border rows and columns read the zero padding: with bn(0) taken for a padding pixel they would move
    for name, sl in (("top", (..., 0, slice(None))), ("bottom", (..., -1, slice(None))), ("left", (..., slice(None), 0)),
                     ("right", (..., slice(None), -1))):
        assert torch.equal(got[sl], ref[sl]), f"{name} border (sigmoid)"
        assert torch.equal(got_raw[sl], ref_raw[sl]), f"{name} border (no activation)"
    assert torch.equal(got, ref)
    assert torch.equal(got_raw, ref_raw)


# ==== 2. weight gradient ================================================================================================
@pytest.mark.parametrize("arith", list(ARITH))
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("shape", [(2, 32, 32), (1, 16, 64), (1, 4, 256), (1, 2, 512)])
def test_wgrad_bitwise(arith, accumulate, shape):
    N, H, W = shape
    y = nhwc(rnd(N, K, H // 2, W // 2, seed=21, scale=2.0) + 0.3)
    g = rnd(N, 3, H, W, seed=22).to(DEV)
    saved, gamma, beta = _bn_params(23)
    dw0 = rnd(K, 3, 4, 4, seed=24).to(DEV)
    with _ctx(arith):
        assert ops.c3_tail_bn_ok(y, need_wgrad=True)
        z = ops.bn_act_fwd(y, saved, gamma, beta, ops.ACT_RELU)
        ref = ops.c3_wgrad(z, g, out=dw0.clone() if accumulate else None, accumulate=accumulate)
        got = ops.c3_wgrad_bn(y, saved, gamma, beta, g, out=dw0.clone() if accumulate else torch.full_like(dw0, float("nan")),
                              accumulate=accumulate)
    assert torch.isfinite(got).all()
    assert torch.equal(got, ref)


# ==== 3. model level: the group with the switch on against the switch off ===============================================
def _stub(seed):
    torch.manual_seed(seed)
    layers = [model.ConvTranspose2d(128, K), model.BatchNorm2d(K), model.ReLU(True), model.ConvTranspose2d(K, 3), model.Sigmoid()]
    with torch.no_grad():
        layers[1].weight.copy_(rnd(K, seed=seed + 1) + 1.5)
        layers[1].bias.copy_(rnd(K, seed=seed + 2))
    return [m.to(DEV).train() for m in layers]


def _run_stub(onload, arith, size, fuse_stats=False, n=2):
    """One forward + backward of the stub; everything the switch could change."""
    layers = _stub(5)
    x = nhwc(rnd(n, 128, size, size, seed=31)).requires_grad_(True)
    dout = rnd(n, 3, 4 * size, 4 * size, seed=32).to(DEV)
    saved_switch, saved_fuse = model.TAIL_BN_ONLOAD, model.FUSE_BN_STATS
    model.TAIL_BN_ONLOAD, model.FUSE_BN_STATS = onload, (True if fuse_stats else saved_fuse)
    try:
        with _ctx(arith), _count_calls("dg_conv4x4s2_c3_dgrad_bn_p") as fwd_calls, _count_calls("dg_conv4x4s2_c3_wgrad_bn_p") as wg_calls, \
                _count_calls("dg_bn_act_fwd_x3") as x3_apply, _count_calls("dg_bn_act_fwd") as f32_apply:
            out = model._run_fused(layers, x)
            out.backward(dout)
            ops.current().clear()
        torch.cuda.synchronize()
    finally:
        model.TAIL_BN_ONLOAD, model.FUSE_BN_STATS = saved_switch, saved_fuse
    bn = layers[1]
    res = dict(out=out.detach(), dx=x.grad, dw1=layers[0].weight.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, dw2=layers[3].weight.grad,
               running_mean=bn.running_mean, running_var=bn.running_var, nbt=bn.num_batches_tracked)
    return res, (fwd_calls.n, wg_calls.n, x3_apply.n + f32_apply.n)


def _leaf_group(onload, arith):
    """The group alone on a leaf y: the gradient INTO the previous layer (dy) is y.grad itself."""
    layers = _stub(5)
    bn, relu, convT, sig = layers[1:]
    y = nhwc(rnd(2, K, 32, 32, seed=41, scale=2.0) + 0.3).requires_grad_(True)
    dout = rnd(2, 3, 64, 64, seed=42).to(DEV)
    with _ctx(arith):
        if onload:
            out = model._tail_apply(y, bn, ops.ACT_RELU, None, [convT, sig])
        else:
            out = convT(bn(y, ops.ACT_RELU, 0.0), ops.ACT_SIGMOID)
        out.backward(dout)
        ops.current().clear()
    return dict(out=out.detach(), dy=y.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, dw2=convT.weight.grad,
                running_mean=bn.running_mean, running_var=bn.running_var)


def _same(a, b):
    for k in a:
        assert a[k] is not None and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("arith,fuse_stats", [("f32", False), ("f32", True), ("f32x3", False)])
def test_model_switch_bitwise(arith, fuse_stats):
    on, calls_on = _run_stub(True, arith, 16, fuse_stats)
    off, calls_off = _run_stub(False, arith, 16, fuse_stats)
    assert calls_on == (1, 1, 0), f"the group did not take the on-load kernels: {calls_on}"
    assert calls_off == (0, 0, 1), f"the switch did not restore the apply pass: {calls_off}"
    _same(on, off)


@pytest.mark.parametrize("arith", list(ARITH))
def test_group_on_leaf_bitwise(arith):
    _same(_leaf_group(True, arith), _leaf_group(False, arith))


def test_forward_hook_keeps_the_apply_pass():
    """A forward hook on the BatchNorm wants its output: the group keeps the apply pass."""
    layers = _stub(5)
    seen = []
    h = layers[1].register_forward_hook(lambda mod, inp, out: seen.append(tuple(out.shape)))
    x = nhwc(rnd(2, 128, 16, 16, seed=31))
    with _ctx("f32"), _count_calls("dg_conv4x4s2_c3_dgrad_bn_p") as calls, torch.no_grad():
        model._run_fused(layers, x)
    h.remove()
    assert calls.n == 0 and seen == [(2, K, 32, 32)]


# ==== 4. where the form does not exist ==================================================================================
def test_ok_query_refusals():
    L = _lib.load()
    F32, X3, BF16 = ops.PREC_F32, ops.PREC_F32X3, ops.PREC_BF16
    for prec in (F32, X3):
        assert L.dg_c3_dgrad_bn_ok(2, 64, 64, 64, prec) == 1 and L.dg_c3_wgrad_bn_ok(2, 64, 64, 64, prec) == 1
        assert L.dg_c3_dgrad_bn_ok(2, 64, 64, 32, prec) == 0 and L.dg_c3_wgrad_bn_ok(2, 64, 64, 32, prec) == 0        # K = 32
        assert L.dg_c3_wgrad_bn_ok(2, 16, 16, 64, prec) == 0 and L.dg_c3_wgrad_bn_ok(2, 32, 32, 64, prec) == 1        # W = 16 | 32
        assert L.dg_c3_dgrad_bn_ok(64, 1024, 1024, 64, prec) == 0                                                     # y of 2^32 bytes
        assert L.dg_c3_wgrad_bn_ok(32, 512, 512, 64, prec) == 1 and L.dg_c3_wgrad_bn_ok(64, 512, 512, 64, prec) == 0  # y of 2^29 | 2^30 bytes
    assert L.dg_c3_dgrad_bn_ok(2, 64, 64, 64, BF16) == 0 and L.dg_c3_wgrad_bn_ok(2, 64, 64, 64, BF16) == 0
    with options(kt=16):
        assert L.dg_c3_dgrad_bn_ok(2, 64, 64, 64, F32) == 0                  # the gather form has no on-load variant
    y32 = nhwc(rnd(2, K, 32, 32, seed=1))
    y16 = nhwc(rnd(2, K, 32, 32, seed=1), torch.bfloat16)
    with _ctx("f32"):
        assert ops.c3_tail_bn_ok(y32) and not ops.c3_tail_bn_ok(y16)         # bf16 storage
        assert not ops.c3_tail_bn_ok(nhwc(rnd(2, K, 8, 8, seed=1))) and ops.c3_tail_bn_ok(nhwc(rnd(2, K, 8, 8, seed=1)), need_wgrad=False)
    with ops.use(ops.Context(prec=F32, act16=True)):
        assert not ops.c3_tail_bn_ok(y32)
    with ops.use(ops.Context(prec=BF16, shadow=True)):
        assert not ops.c3_tail_bn_ok(y32)
    # the entry points refuse what the queries refuse, and anything but a ReLU
    w = rnd(32, 3, 4, 4, seed=2).to(DEV)
    p = torch.zeros(2, 64, device=DEV)
    out = torch.empty(2, 3, 64, 64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert L.dg_conv4x4s2_c3_dgrad_bn_p(y32.data_ptr(), p.data_ptr(), p.data_ptr(), p.data_ptr(), ops.ACT_RELU, w.data_ptr(), out.data_ptr(), 2, 64, 64, 32,
                                        ops.ACT_NONE, F32, st) == -1
    assert L.dg_conv4x4s2_c3_dgrad_bn_p(y32.data_ptr(), p.data_ptr(), p.data_ptr(), p.data_ptr(), ops.ACT_LEAKY, w.data_ptr(), out.data_ptr(), 2, 64, 64, 64,
                                        ops.ACT_NONE, F32, st) == -1


def test_refused_shape_takes_the_old_group():
    """16 px images: the weight gradient has no on-load form (W = 16), the model keeps the apply pass -- and computes the same."""
    on, calls_on = _run_stub(True, "f32", 4)
    off, calls_off = _run_stub(False, "f32", 4)
    assert calls_on == (0, 0, 1) and calls_off == (0, 0, 1)
    _same(on, off)


def test_grouped_passes_keep_the_apply_pass():
    """The grouped (``_g``) forms used below 256 px have no on-load variant: group_generators does not reach the new entry points."""
    torch.manual_seed(3)
    nets = [model.Generator(image_size=64).to(DEV).train() for _ in range(2)]
    xs = [rnd(2, 3, 64, 64, seed=50 + i).to(DEV) for i in range(2)]
    with _ctx("f32"), _count_calls("dg_conv4x4s2_c3_dgrad_bn_p") as calls, torch.no_grad():
        assert ops.group_ok()
        grouped = model.group_generators(nets, xs)
        assert calls.n == 0
        single = [net(x) for net, x in zip(nets, xs)]
        assert calls.n == 2
    for a, b in zip(grouped, single):
        assert torch.equal(a, b)
