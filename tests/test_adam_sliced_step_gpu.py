"""A step of optim.Adam issued in slices (begin_step, step_ranges per slice, finish_step: what the bucketed and the graph-overlap
exchange of the trainer do) against step() on a twin optimiser: every buffer the group keeps, bit for bit.

The group is small and has every kind of parameter: a KRSC conv weight of one 64 x 64 tile (K = 64, C = 4: J = 64), one of the other
tile width (K = 64, C = 8: J = 128), a 3-channel 4x4 weight (J = 48: no whole tile), two BatchNorm vectors of C = 192 and a 1-element
head bias with 63 elements of padding behind it.  With the f32x3 planes step() takes the fused group path (ops.adam_step_group_x3),
documented as bit-identical to the flat step followed by the transpose pass (tests/test_adam_fused_transpose_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import optim, ops  # noqa: E402

DEV = "cuda"
SHAPES = [(64, 4), 192, (64, 8), 192, (64, 3), 1]          # (K, C) of a [K, C, 4, 4] weight, or a vector
CONFIGS = ["plain", "bf16_shadow", "x3_planes"]
CORE = ("flat_p", "exp_avg", "exp_avg_sq", "state")
DERIVED = {"plain": (), "bf16_shadow": ("flat_p16",), "x3_planes": ("flat_p3", "flat_p3t")}


def _group(config):
    gen = torch.Generator().manual_seed(7)
    params = []
    for s in SHAPES:
        if isinstance(s, int):
            params.append(torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)))
        else:
            params.append(torch.nn.Parameter(ops.krsc_param(torch.randn(s[0], s[1], 4, 4, generator=gen).to(DEV))))
    opt = optim.Adam(params, lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-2)
    if config == "bf16_shadow":
        opt.enable_bf16_shadow()
    elif config == "x3_planes":
        opt.enable_x3_planes()
    return opt


def _random_flat(opt, gen, scale):
    """Random at the parameters, +0 at the padding between them (as the optimiser keeps its flat gradient)."""
    k = torch.zeros(opt.numel, device=DEV)
    for p, off in zip(opt.params, opt.offsets):
        k[off:off + p.numel()] = 1
    return torch.where(k != 0, torch.randn(opt.numel, generator=gen).to(DEV) * scale, 0.0)


def _twins(config):
    """Two optimisers in the same state with random moments, and the gradients of two steps."""
    a, b = _group(config), _group(config)
    gen = torch.Generator().manual_seed(11)
    a.exp_avg.copy_(_random_flat(a, gen, 1e-2))
    a.exp_avg_sq.copy_(_random_flat(a, gen, 1e-2).square())
    for name in CORE:
        getattr(b, name).copy_(getattr(a, name))
    return a, b, [_random_flat(a, gen, 1e-2) for _ in range(2)]


def _bits(t):
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _assert_same_bits(a, b, config, what):
    for name in CORE + DERIVED[config]:
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), (what, name)


def _pieces(opt):
    """[0, numel) in three pieces cut at parameter boundaries: (conv, vector), (conv, vector), (3-channel conv, bias + padding)."""
    cuts = [0, opt.offsets[2], opt.offsets[4], opt.numel]
    return list(zip(cuts, cuts[1:]))


@pytest.mark.parametrize("config", CONFIGS)
def test_sliced_step_is_bitwise_the_whole_step(config):
    a, b, grads = _twins(config)
    first, second, third = _pieces(a)
    assert sum(e - s for s, e in (first, second, third)) == a.numel and a.offsets[5] + 64 == a.numel
    for t, g in enumerate(grads):
        before = a.flat_p.clone()
        a.flat_g.copy_(g)
        b.flat_g.copy_(g)
        a.step(grad_scale=0.5)
        b.begin_step()
        b.step_ranges([third], grad_scale=0.5)               # out of order, one call per slice and one call of two
        b.step_ranges([first, second][::-1], grad_scale=0.5)
        b.finish_step()
        torch.cuda.synchronize()
        assert not torch.equal(a.flat_p, before)
        _assert_same_bits(a, b, config, f"step {t + 1}")
    assert float(a.state[0]) == 2.0
    if config == "x3_planes":                                # (the derived forms are those of the stepped parameters)
        assert torch.equal(a.flat_p3.float().sum(0), a.flat_p)
    if config == "bf16_shadow":
        assert torch.equal(a.flat_p16, a.flat_p.to(torch.bfloat16))


@pytest.mark.parametrize("config", CONFIGS)
def test_active_ranges_gate_the_sliced_step_as_they_gate_step(config):
    a, b, grads = _twins(config)

    def sub(o):                                              # the second conv weight with its vector, and the head bias: two ranges
        return o.ranges_of([torch.nn.ParameterList([o.params[2], o.params[3], o.params[5]])])

    assert sub(a) == [(a.offsets[2], a.offsets[4]), (a.offsets[5], a.numel)]
    kept = {name: getattr(a, name).clone() for name in CORE[:3] + DERIVED[config]}
    for g in grads:
        a.flat_g.copy_(g)
        b.flat_g.copy_(g)
        a.step(active=sub(a))
        b.begin_step()
        b.step_ranges(sub(b))
        b.finish_step()
    torch.cuda.synchronize()
    _assert_same_bits(a, b, config, "active")
    outside = torch.ones(a.numel, dtype=torch.bool, device=DEV)
    for s, e in sub(a):
        outside[s:e] = False
    if config == "x3_planes":                                # the stepped weight's transposed planes are those of its new planes
        w = slice(a.offsets[2], a.offsets[3])
        assert torch.equal(_bits(a.flat_p3t[:, w]), _bits(a.flat_p3[:, w].view(3, 64, 128).transpose(1, 2).reshape(3, -1)))
    for name, t in kept.items():                             # (a transposed image lies at its weight's offsets: one mask for all)
        assert torch.equal(_bits(getattr(a, name))[..., outside], _bits(t)[..., outside]), name
        assert not torch.equal(_bits(getattr(a, name))[..., ~outside], _bits(t)[..., ~outside]), name


def test_a_sliced_step_is_refused_under_gradient_control():
    a, _, grads = _twins("plain")
    a.enable_grad_control(1.0, True)
    with pytest.raises(RuntimeError, match="begin_step"):
        a.begin_step()
    assert float(a.state[0]) == 0.0
    before = a.flat_p.clone()
    a.flat_g.copy_(grads[0])
    a.step()
    torch.cuda.synchronize()
    st = a.grad_stats()
    assert float(a.state[0]) == 1.0 and st["steps"] == 1 and not st["skip"] and not torch.equal(a.flat_p, before)
