"""The f32x3 Adam step of a whole group that writes the transposed weight planes itself (ops.adam_step_group_x3,
csrc/optim.hip adam_step_x3t_kernel + adam_step_ranges_x3_kernel) against the two-kernel form it replaces (adam_step_flat with
planes, then x3_transpose_planes; ops.ADAM_FUSED_T = False): every buffer bit for bit.

The group mixes weights that are whole tiles of their [K][J] image -- J % 128 == 0: 64 x 128 tiles (2 x 1 and 1 x 8 of them); otherwise
64 x 64 tiles (one tile, 3 x 3) -- with everything the tiled kernels do not take: K = 100, J = 48, the K = 1 head and BatchNorm-sized
vectors in between.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import ops, optim  # noqa: E402

DEV = "cuda"
SHAPES = [(64, 4), (128, 8), 100, (64, 64), (192, 12), (100, 8), 24, (64, 3), (1, 64)]      # (K, C) of a [K, C, 4, 4] weight, or a vector
BUFFERS = ("flat_p", "exp_avg", "exp_avg_sq", "flat_p3", "flat_p3t")


def _group(weight_decay):
    gen = torch.Generator().manual_seed(7)
    params = []
    for s in SHAPES:
        if isinstance(s, int):
            params.append(torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)))
        else:
            params.append(torch.nn.Parameter(ops.krsc_param(torch.randn(s[0], s[1], 4, 4, generator=gen).to(DEV))))
    opt = optim.Adam(params, lr=2e-4, betas=(0.5, 0.999), weight_decay=weight_decay)
    opt.enable_x3_planes()
    return opt


def _mask(opt):
    """1 at the parameters, 0 at the padding between them."""
    k = torch.zeros(opt.numel, device=DEV)
    for p, off in zip(opt.params, opt.offsets):
        k[off:off + p.numel()] = 1
    return k


def _randomise(opt, seed):
    """Two warm steps (the step count and the bias corrections move), then random p, g, m, v at the parameters."""
    gen = torch.Generator().manual_seed(seed)
    k = _mask(opt)

    def rnd(scale):
        return torch.where(k != 0, torch.randn(opt.numel, generator=gen).to(DEV) * scale, 0.0)      # (+0 at the padding)

    for _ in range(2):
        opt.flat_g.copy_(rnd(1e-2))
        opt.step()
    opt.flat_p.copy_(rnd(0.05))
    opt.flat_g.copy_(rnd(1e-2))
    opt.exp_avg.copy_(rnd(1e-2))
    opt.exp_avg_sq.copy_(rnd(1e-2).square())
    opt.refresh_derived()


def _pair(weight_decay, seed=11, **control):
    """Two groups in the same state: the first is stepped by the fused form, the second by the two-kernel form."""
    a, b = _group(weight_decay), _group(weight_decay)
    _randomise(a, seed)
    for name in BUFFERS + ("flat_g", "state"):
        getattr(b, name).copy_(getattr(a, name))
    if control:
        a.enable_grad_control(**control)
        b.enable_grad_control(**control)
    return a, b


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _assert_same_bits(a, b):
    for name in BUFFERS:
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name


def _assert_padding_zero(opt):
    pad = _mask(opt) == 0
    assert pad.any()
    for name in BUFFERS:
        t = getattr(opt, name)
        assert not _bits(t)[..., pad].any(), name


def _step(opt, fused, monkeypatch, **kw):
    monkeypatch.setattr(ops, "ADAM_FUSED_T", fused)
    opt.step(**kw)
    torch.cuda.synchronize()


def test_the_group_is_split_as_documented():
    opt = _group(0.0)
    nw, w_off, w_k, w_j, nr, r_off, r_len = opt._adam_group_table
    assert [(w_k[i], w_j[i]) for i in range(nw)] == [(64, 64), (128, 128), (64, 1024), (192, 192)]
    assert opt._x3t_rest_table[0] == 2                                   # K = 100 and J = 48 keep the transpose pass
    covered = sum(w_k[i] * w_j[i] for i in range(nw)) + sum(r_len[i] for i in range(nr))
    assert covered == opt.numel and nr == 2                              # neighbours outside the tiles merge into one range


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
def test_fused_step_is_bitwise_the_two_kernel_step(weight_decay, grad_scale, monkeypatch):
    a, b = _pair(weight_decay)
    before = a.flat_p.clone()
    _step(a, True, monkeypatch, grad_scale=grad_scale)
    _step(b, False, monkeypatch, grad_scale=grad_scale)
    assert not torch.equal(a.flat_p, before)
    _assert_same_bits(a, b)
    _assert_padding_zero(a)
    assert torch.equal(a.state, b.state)
    # the planes are the split of the new parameters, the transposed copy is the transpose of the planes
    assert torch.equal(a.flat_p3.float().sum(0), a.flat_p)
    for p, off in zip(a.params, a.offsets):
        if p._dg_x3[2] is not None:
            k, j = p.shape[0], 16 * p.shape[1]
            src = a.flat_p3[:, off:off + k * j].view(3, k, j).transpose(1, 2).reshape(3, -1)
            assert torch.equal(_bits(a.flat_p3t[:, off:off + k * j]), _bits(src))


def test_a_skipped_step_keeps_every_bit(monkeypatch):
    a, b = _pair(1e-2, guard=True)
    for o in (a, b):
        o.flat_g[o.offsets[3] + 5] = float("inf")
    kept = {name: getattr(a, name).clone() for name in BUFFERS}
    count = a.state.clone()
    _step(a, True, monkeypatch)
    _step(b, False, monkeypatch)
    assert a.grad_stats()["skip"] and b.grad_stats()["skip"]
    for name, t in kept.items():
        assert torch.equal(_bits(getattr(a, name)), _bits(t)), name
    assert torch.equal(a.state, count)
    _assert_same_bits(a, b)


def test_a_clipped_step_is_bitwise_the_two_kernel_step(monkeypatch):
    a, b = _pair(1e-2, max_norm=0.05, guard=True)
    before = a.flat_p.clone()
    _step(a, True, monkeypatch)
    _step(b, False, monkeypatch)
    st = a.grad_stats()
    assert 0.0 < st["scale"] < 1.0 and st["clipped"] == 1 and not st["skip"]
    assert not torch.equal(a.flat_p, before)
    _assert_same_bits(a, b)
    _assert_padding_zero(a)


def test_a_step_of_a_sub_range_is_the_two_kernel_step(monkeypatch):
    a, b = _pair(1e-2)

    def sub(o):
        return o.ranges_of([torch.nn.ParameterList([o.params[1], o.params[2], o.params[5]])])

    before = a.flat_p.clone()
    _step(a, True, monkeypatch, active=sub(a))
    _step(b, False, monkeypatch, active=sub(b))
    _assert_same_bits(a, b)
    _assert_padding_zero(a)
    off0, off3 = a.offsets[0], a.offsets[3]
    assert torch.equal(a.flat_p[off0:a.offsets[1]], before[off0:a.offsets[1]])            # outside the ranges: untouched
    assert torch.equal(a.flat_p[off3:a.offsets[4]], before[off3:a.offsets[4]])
    assert not torch.equal(a.flat_p[a.offsets[1]:off3], before[a.offsets[1]:off3])
