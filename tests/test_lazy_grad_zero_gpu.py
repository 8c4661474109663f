"""optim.Adam.zero_grad(lazy=True) -- the trainer's iteration fills nothing and the first weight-gradient kernel of every parameter
overwrites (functional._flat_grad_of; ops.LAZY_ZERO_GRAD) -- against the zero-fill it replaces: parameters and both moments bit for
bit after every iteration, the flat gradient equal by value (0 + x and x differ for x = -0 only).

Smallest trainer the model builds (16 px, batch 2), on every schedule that writes parameter gradients: the two-chain schedule (exact
fp32, and f32x3 on plane operands: the form the 512 px benchmark runs) and the grouped one (below 256 px by default), which
zero-fills its still-unwritten parameters itself.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import model, ops, optim  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402

DEV = "cuda"
CONFIGS = {
    "f32-two-chain": dict(mfma_dtype="f32", group_launch=False),
    "f32-grouped": dict(mfma_dtype="f32"),
    "f32x3-planes": dict(mfma_dtype="f32x3", x3_planes=True),
    "f32x3-grouped": dict(mfma_dtype="f32x3"),
}


def _bits(t):
    return t.view(torch.int32)


def _run(cfg, lazy, iters, monkeypatch, use_graph=False, arch="discogan"):
    """Snapshots (flat_p, exp_avg, exp_avg_sq, flat_g of the generators' and the discriminators' optimiser) after every iteration."""
    monkeypatch.setattr(ops, "LAZY_ZERO_GRAD", lazy)
    tr = DiscoGANTrainer(default_args(model_arch=arch), device=DEV, image_size=16, seed=1234, use_graph=use_graph, **cfg)
    A, B = synthetic_batch(2, 16, 0, DEV)
    snaps = []
    try:
        for it in range(iters):
            tr.train_iteration(A, B, it)
            tr.finish()
            torch.cuda.synchronize()
            snaps.append([t.clone() for o in (tr.optim_gen, tr.optim_dis) for t in (o.flat_p, o.exp_avg, o.exp_avg_sq, o.flat_g)])
    finally:
        tr.close()
    return tr, snaps


def _assert_same(a, b):
    assert len(a) == len(b)
    for it, (sa, sb) in enumerate(zip(a, b)):
        for i, (x, y) in enumerate(zip(sa, sb)):
            if i % 4 == 3:
                assert torch.equal(x, y), f"flat_g of optimiser {i // 4} after iteration {it}"
            else:
                assert torch.equal(_bits(x), _bits(y)), f"buffer {i % 4} of optimiser {i // 4} after iteration {it}"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_three_iterations_bitwise_with_and_without_the_fill(name, monkeypatch):
    first_writers = []
    wgrad = ops.conv_wgrad

    def spy(*a, out=None, accumulate=False, **k):
        if out is not None:
            first_writers.append(not accumulate)
        return wgrad(*a, out=out, accumulate=accumulate, **k)

    monkeypatch.setattr(ops, "conv_wgrad", spy)
    _, on = _run(CONFIGS[name], True, 3, monkeypatch)
    overwrote = sum(first_writers)
    del first_writers[:]
    _, off = _run(CONFIGS[name], False, 3, monkeypatch)
    _assert_same(on, off)
    assert not any(first_writers)                           # with the fill every writer accumulates
    if name in ("f32-two-chain", "f32x3-planes"):
        assert overwrote > 0                                # (the grouped schedule fills and accumulates: no spy on its launches)
    assert not torch.equal(on[0][0], on[2][0]) and on[0][5].any()      # both sides moved (G-steps 1, 2; the D-step 0 left moments)


@pytest.mark.parametrize("name", ["f32-two-chain", "f32x3-planes", "f32-grouped"])
def test_graph_replay_is_bitwise_the_eager_run(name, monkeypatch):
    _, eager = _run(CONFIGS[name], True, 6, monkeypatch)
    _, graphed = _run(CONFIGS[name], True, 6, monkeypatch, use_graph=True)
    _assert_same(graphed, eager)
    _, filled = _run(CONFIGS[name], False, 6, monkeypatch)
    _assert_same(eager, filled)


def test_networks_outside_the_loss_keep_their_bits_and_read_zero_gradients(monkeypatch):
    """model_arch "gan": G_A and D_A get no gradient -- nothing writes their slices, which are filled before the step reads the buffer."""
    cfg = dict(mfma_dtype="f32")
    tr, on = _run(cfg, True, 3, monkeypatch, arch="gan")
    _, off = _run(cfg, False, 3, monkeypatch, arch="gan")
    _assert_same(on, off)
    fresh = DiscoGANTrainer(default_args(model_arch="gan"), device=DEV, image_size=16, seed=1234, **cfg)
    for opt, opt0, net in ((tr.optim_gen, fresh.optim_gen, tr.generator_A), (tr.optim_dis, fresh.optim_dis, tr.discriminator_A)):
        ranges = opt.ranges_of([net])
        assert ranges
        for b, e in ranges:
            assert torch.equal(_bits(opt.flat_p[b:e]), _bits(opt0.flat_p[b:e]))
            assert not _bits(opt.exp_avg[b:e]).any() and not _bits(opt.exp_avg_sq[b:e]).any()
            assert not opt.flat_g[b:e].any()
        assert not any(getattr(p, "_dg_grad_unwritten", False) for p in opt.params)
    assert not torch.equal(tr.optim_gen.flat_p, fresh.optim_gen.flat_p)      # (G_B did move)


def test_plain_zero_grad_still_fills_and_backward_accumulates(monkeypatch):
    monkeypatch.setattr(ops, "LAZY_ZERO_GRAD", True)
    torch.manual_seed(3)
    g = model.Generator(extra_layers=True, image_size=16).to(DEV)
    opt = optim.Adam(g.parameters(), lr=2e-4)
    x = torch.rand(2, 3, 16, 16, device=DEV)

    def backward():
        g(x).sum().backward()
        torch.cuda.synchronize()

    backward()
    once = opt.flat_g.clone()
    assert once.any()
    backward()                                              # no zero_grad in between: the second pass adds
    twice = opt.flat_g.clone()
    assert torch.allclose(twice, 2 * once, rtol=1e-4, atol=1e-6 * float(once.abs().max())) and not torch.equal(twice, once)
    opt.zero_grad()
    assert not _bits(opt.flat_g).any() and all(p.grad is p._dg_flat_grad and not p.grad.any() for p in opt.params)
    backward()
    assert torch.equal(_bits(opt.flat_g), _bits(once))
    backward()
    assert torch.equal(_bits(opt.flat_g), _bits(twice))
    # the lazy form: nothing is filled, the first pass overwrites, the second accumulates -- the same values
    opt.zero_grad(lazy=True)
    assert torch.equal(_bits(opt.flat_g), _bits(twice))
    backward()
    opt.fill_unwritten_grads()
    assert torch.equal(opt.flat_g, once)
    backward()
    assert torch.equal(opt.flat_g, twice)
    # a parameter nothing writes reads zero once the buffer is read
    opt.zero_grad(lazy=True)
    opt.fill_unwritten_grads()
    assert not opt.flat_g.any()
