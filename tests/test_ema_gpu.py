"""Generator weight EMA on the GPU: dg_ema_update_flat / dg_swap_flat bitwise against tests/ema_ref.py, optim.EMA inside the trainer on
every schedule (eager, hipGraph replay, grouped, other architectures, two ranks), the swap context, exact resume and the three CLIs.
Trainers are 16 px, batch 4, seed 1234.

Why bitwise: subtraction, multiplication and addition are correctly rounded IEEE single operations on the device, the kernel is built
with contraction off, numpy fuses nothing, and no denormal goes in or comes out (asserted on the reference's intermediates)."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import evaluate, inference, ops  # noqa: E402
from discogan_modernized_amd import image_translation as it_cli  # noqa: E402
from discogan_modernized_amd._lib import DiscoganHipError  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tests import ema_ref  # noqa: E402

DEV = "cuda"
S, N = 16, 4
# the kernels' geometry (csrc/optim.hip): at most 4096 blocks x 256 threads x 4 elements per trip of the grid-stride loop
TRIP = 4096 * 256 * 4
N_BIG = 2 * TRIP + 300 * 4 + 3                # two full trips of the capped grid, 300 more vector items, a 3-element tail
assert N_BIG == 8_389_811
SIZES = [1, 3, 4, 5, 1027, N_BIG]
WEIGHTS = [float(1 - 0.999), 0.5, 0.0, 1.0]
FLT_MIN = np.float32(1.17549435e-38)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- 1. the update kernel -----------------------------------------------------------------------------------------------------------
_DATA = {}


def _data(n):
    """p, e ~ N(0, 0.02) (fixed seed) with exact zeros in both and a stretch where p == e; made once per size."""
    if n not in _DATA:
        rng = np.random.default_rng(1234 + n)
        p = (rng.standard_normal(n) * 0.02).astype(np.float32)
        e = (rng.standard_normal(n) * 0.02).astype(np.float32)
        p[2::7] = 0.0
        e[5::11] = 0.0
        lo, hi = n // 3, n // 3 + n // 8
        p[lo:hi] = e[lo:hi]
        refs = {}
        for w in WEIGHTS:
            w32 = np.float32(w)
            d = p - e
            s = d * w32
            out = ema_ref.lerp(e, p, w)
            for name, x in (("p", p), ("e", e), ("p - e", d), ("(p - e) * w", s), ("result", out)):
                tiny = (x != 0) & (np.abs(x) < FLT_MIN)
                assert not tiny.any(), f"n={n} w={w}: denormal in {name}"
            refs[w] = out
        _DATA[n] = (p, e, (lo, hi), refs)
    return _DATA[n]


@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_is_bitwise_the_reference(n, w):
    p, e, (lo, hi), refs = _data(n)
    tp, te = torch.from_numpy(p).to(DEV), torch.from_numpy(e).to(DEV)
    ops.ema_update_flat(te, tp, w)
    got = te.cpu().numpy()
    assert np.array_equal(tp.cpu().numpy().view(np.int32), p.view(np.int32)), "p was written"
    bad = np.flatnonzero(got.view(np.int32) != refs[w].view(np.int32))
    assert bad.size == 0, f"n={n} w={w}: {bad.size} elements differ, first at {bad[:5]}: {got[bad[:5]]} vs {refs[w][bad[:5]]}"
    assert np.array_equal(got[lo:hi].view(np.int32), e[lo:hi].view(np.int32)), "p == e must leave e unchanged for every w"
    if w == 0.0:
        assert np.array_equal(got.view(np.int32), e.view(np.int32))


def test_update_of_a_sliced_range_leaves_its_neighbours_alone():
    n = 1027
    p, e, _, refs = _data(n)
    sentinel = 0x7FC12345                                        # a NaN with a payload: any arithmetic on it would show
    eb = torch.full((64 + n + 64,), sentinel, dtype=torch.int32, device=DEV).view(torch.float32)
    pb = torch.full((64 + n + 64,), sentinel, dtype=torch.int32, device=DEV).view(torch.float32)
    eb[64:64 + n] = torch.from_numpy(e).to(DEV)
    pb[64:64 + n] = torch.from_numpy(p).to(DEV)
    w = WEIGHTS[0]
    ops.ema_update_flat(eb[64:64 + n], pb[64:64 + n], w)
    got = eb.cpu().view(torch.int32).numpy()
    assert np.array_equal(got[64:64 + n], refs[w].view(np.int32))
    assert (got[:64] == sentinel).all() and (got[64 + n:] == sentinel).all()
    pg = pb.cpu().view(torch.int32).numpy()
    assert (pg[:64] == sentinel).all() and (pg[64 + n:] == sentinel).all() and np.array_equal(pg[64:64 + n], p.view(np.int32))


@pytest.mark.parametrize("n,k", [(1027, 515), (1027, 1026), (N_BIG, TRIP + 4 * 77 + 1)])
def test_one_nan_in_p_gives_exactly_one_nan_in_the_ema(n, k):
    p, e, _, refs = _data(n)
    tp, te = torch.from_numpy(p).to(DEV), torch.from_numpy(e).to(DEV)
    tp[k] = float("nan")
    ops.ema_update_flat(te, tp, 0.5)
    nan = torch.isnan(te)
    assert int(nan.sum()) == 1 and bool(nan[k])
    got = te.cpu().numpy()
    keep = np.arange(n) != k
    assert np.array_equal(got[keep].view(np.int32), refs[0.5][keep].view(np.int32))


def test_ops_wrappers_refuse_what_the_kernels_cannot_take():
    a = torch.zeros(64, device=DEV)
    with pytest.raises(DiscoganHipError):
        ops.ema_update_flat(a, torch.zeros(63, device=DEV), 0.5)
    with pytest.raises(DiscoganHipError, match="align"):
        ops.ema_update_flat(a[1:33], a[32:64], 0.5)
    with pytest.raises(DiscoganHipError, match="outside"):
        ops.ema_update_flat(a[:32], a[32:], 1.5)
    with pytest.raises(DiscoganHipError, match="overlap"):
        ops.swap_flat(a[:32], a[16:48])
    with pytest.raises(DiscoganHipError):
        ops.swap_flat(a, torch.zeros(64))                          # a host tensor
    torch.cuda.synchronize()
    assert not a.any()


# ---- 2. swap --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_every_bit_and_twice_restores(n):
    g = torch.Generator().manual_seed(77 + n)
    ia = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    ib = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    ia[0], ib[-1] = 0x7FC00001, -4194303                         # a quiet NaN with a payload, a negative NaN (0xFFC00001)
    a, b = ia.to(DEV).view(torch.float32), ib.to(DEV).view(torch.float32)
    ops.swap_flat(a, b)
    assert torch.equal(_bits(a).cpu(), ib) and torch.equal(_bits(b).cpu(), ia)
    ops.swap_flat(a, b)
    assert torch.equal(_bits(a).cpu(), ia) and torch.equal(_bits(b).cpu(), ib)
    ops.swap_flat(a, a)                                            # the same range: nothing happens
    assert torch.equal(_bits(a).cpu(), ia)


def test_swap_of_sliced_ranges_leaves_the_neighbours_alone():
    n = 1027
    g = torch.Generator().manual_seed(9)
    half = 64 + (n + 63) // 64 * 64 + 64                         # like every flat range, both start on a 64-float boundary
    buf = torch.randint(-2 ** 31, 2 ** 31 - 1, (2 * half,), generator=g, dtype=torch.int64).to(torch.int32)
    dev = buf.to(DEV).view(torch.float32)
    ops.swap_flat(dev[64:64 + n], dev[half + 64:half + 64 + n])
    got = dev.cpu().view(torch.int32)
    want = buf.clone()
    want[64:64 + n], want[half + 64:half + 64 + n] = buf[half + 64:half + 64 + n], buf[64:64 + n]
    assert torch.equal(got, want)


# ---- trainer runs shared by the cases below -------------------------------------------------------------------------------------------
_RUNS = {}


def _gen_buffers(tr):
    return [b.detach().clone() for net in (tr.generator_A, tr.generator_B) for b in net.buffers()]


def _run(key, iters=6, args=None, **kw):
    """`iters` iterations (D, G, G, D, G, G) of one trainer on one fixed batch; after every iteration the generators' flat weights and
    the EMA (None until ready) are kept on the host.  One run per key for the whole module."""
    if key not in _RUNS:
        A, B = synthetic_batch(N, S, 5, DEV)
        tr = DiscoGANTrainer(default_args(**(args or {})), device=DEV, image_size=S, seed=1234, **kw)
        losses, snaps, emas, ready = [], [], [], []
        for i in range(iters):
            losses.append(tr.losses_to_floats(tr.train_iteration(A, B, i)))
            tr.finish()
            snaps.append(tr.optim_gen.flat_p.cpu().numpy().copy())
            on = tr.ema is not None and tr.ema.ready
            ready.append(on)
            emas.append(tr.ema.flat.cpu().numpy().copy() if on else None)
        torch.cuda.synchronize()
        _RUNS[key] = dict(losses=losses, snaps=snaps, emas=emas, ready=ready, updates=None if tr.ema is None else tr.ema.updates,
                          m=tr.optim_gen.exp_avg.cpu(), v=tr.optim_gen.exp_avg_sq.cpu(), dis=tr.optim_dis.flat_p.cpu(),
                          bufs=[b.cpu() for b in _gen_buffers(tr)], has_ema_state="ema" in tr.train_state(iters),
                          grouped=tr.group_launch)
        del tr
    return _RUNS[key]


def _eq(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


# ---- 3. the recursion -------------------------------------------------------------------------------------------------------------------
def test_trainer_ema_is_the_reference_recursion_and_only_observes():
    r = _run("eager", args=dict(ema_decay=0.9))
    assert r["updates"] == 3 and r["ready"] == [False, True, True, True, True, True]
    g_snaps = [r["snaps"][i] for i in (1, 2, 4, 5)]
    assert not _eq(g_snaps[0], g_snaps[1]) and not _eq(g_snaps[2], g_snaps[3])            # the generators do move
    assert _eq(r["emas"][1], g_snaps[0])                                                # the first qualifying step: a copy
    assert _eq(r["emas"][2], ema_ref.recursion(g_snaps[:2], 0.9))
    assert _eq(r["emas"][3], r["emas"][2]) and _eq(r["snaps"][3], r["snaps"][2])        # a D-step touches neither
    assert _eq(r["emas"][4], ema_ref.recursion(g_snaps[:3], 0.9))
    assert _eq(r["emas"][5], ema_ref.recursion(g_snaps, 0.9))                           # a copy, then three lerps
    assert not _eq(r["emas"][5], r["snaps"][5])
    assert r["has_ema_state"]
    off = _run("eager_off")
    assert off["updates"] is None and not off["has_ema_state"]
    assert off["losses"] == r["losses"]
    for i in range(6):
        assert _eq(off["snaps"][i], r["snaps"][i]), i
    assert torch.equal(off["m"], r["m"]) and torch.equal(off["v"], r["v"]) and torch.equal(off["dis"], r["dis"])
    assert len(off["bufs"]) == len(r["bufs"]) > 0 and all(torch.equal(a, b) for a, b in zip(off["bufs"], r["bufs"]))


def test_trainer_without_ema_allocates_nothing():
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=1234)
    assert tr.ema is None and "ema" not in tr.train_state(0)
    with pytest.raises(RuntimeError, match="no EMA"):
        with tr.ema_weights():
            pass
    with pytest.raises(RuntimeError):
        tr.ema_state_dicts()
    with pytest.raises(ValueError, match="ema_decay"):
        DiscoGANTrainer(default_args(ema_decay=1.0), device=DEV, image_size=S, seed=1234)
    with pytest.raises(ValueError, match="ema_decay"):
        DiscoGANTrainer(default_args(ema_decay=-0.5), device=DEV, image_size=S, seed=1234)


# ---- 4. start iteration -----------------------------------------------------------------------------------------------------------------
def test_ema_start_iter_delays_the_copy():
    r = _run("start3", args=dict(ema_decay=0.9, ema_start_iter=3))
    assert r["ready"] == [False, False, False, False, True, True]
    assert _eq(r["emas"][4], r["snaps"][4])
    assert _eq(r["emas"][5], ema_ref.recursion([r["snaps"][4], r["snaps"][5]], 0.9))
    assert r["updates"] == 1
    base = _run("eager", args=dict(ema_decay=0.9))
    assert all(_eq(a, b) for a, b in zip(r["snaps"], base["snaps"]))                      # the training itself is the same
    r4 = _run("start4_five_iterations", iters=5, args=dict(ema_decay=0.9, ema_start_iter=3))
    assert r4["updates"] == 0 and r4["ready"][4] and _eq(r4["emas"][4], r4["snaps"][4])


# ---- 5. schedules -----------------------------------------------------------------------------------------------------------------------
# What is bitwise equal to what today (tests/test_group_gpu.py): hipGraph replay == eager dispatch of the same schedule; the grouped
# schedule with group_plan="single" == the two-chain schedule.  (The default grouped plan sums split-K slabs in another order than the
# two-chain schedule, so those two are compared each with its own replayed form.)
@pytest.mark.parametrize("key,kw,base,base_kw", [
    ("graph", dict(use_graph=True), "eager", dict()),
    ("chain_graph", dict(use_graph=True, group_launch=False), "chain", dict(group_launch=False)),
    ("single", dict(group_launch=True, group_plan="single"), "chain", dict(group_launch=False)),
    ("single_graph", dict(group_launch=True, group_plan="single", use_graph=True), "chain", dict(group_launch=False)),
    ("one_stream", dict(group_launch=False, two_streams=False), "chain", dict(group_launch=False)),
])
def test_ema_is_the_same_on_every_schedule(key, kw, base, base_kw):
    a = dict(ema_decay=0.9)
    ref = _run(base, args=a, **base_kw)
    r = _run(key, args=a, **kw)
    assert ref["grouped"] == (base == "eager") and r["updates"] == ref["updates"] == 3
    assert r["losses"] == ref["losses"]
    for i in range(6):
        assert _eq(r["snaps"][i], ref["snaps"][i]), i
        assert r["ready"][i] == ref["ready"][i]
        if r["ready"][i]:
            assert _eq(r["emas"][i], ref["emas"][i]), i
    g_snaps = [r["snaps"][i] for i in (1, 2, 4, 5)]
    assert _eq(r["emas"][5], ema_ref.recursion(g_snaps, 0.9))
    assert _eq(ref["emas"][5], ema_ref.recursion([ref["snaps"][i] for i in (1, 2, 4, 5)], 0.9))


# ---- 6. other architectures -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["gan", "recongan"])
def test_generator_outside_the_loss_keeps_its_ema_equal_to_itself(arch):
    A, B = synthetic_batch(N, S, 5, DEV)
    tr = DiscoGANTrainer(default_args(model_arch=arch, ema_decay=0.9), device=DEV, image_size=S, seed=1234)
    w0 = tr.optim_gen.flat_p.clone()
    for i in range(5):                                             # D, G, G, D, G
        tr.train_iteration(A, B, i)
    tr.finish()
    assert tr.ema.updates == 2 and tr.ema.ready
    opt = tr.optim_gen
    moved = {}
    for name, net in (("gen_A", tr.generator_A), ("gen_B", tr.generator_B)):
        rng = opt.ranges_of([net])
        assert rng
        moved[name] = any(not same_bits(opt.flat_p[b:e], w0[b:e]) for b, e in rng)
        equal = all(same_bits(tr.ema.flat[b:e], opt.flat_p[b:e]) for b, e in rng)
        assert equal == (not moved[name]), (arch, name, moved[name], equal)
    # gan: G_B alone is in the loss; recongan: the cycle A -> B -> A reaches both
    assert moved == (dict(gen_A=False, gen_B=True) if arch == "gan" else dict(gen_A=True, gen_B=True))


# ---- 7. the swap context ----------------------------------------------------------------------------------------------------------------
MODES = dict(f32=dict(mfma_dtype="f32"), bf16=dict(mfma_dtype="bf16"), f32x3=dict(mfma_dtype="f32x3", x3_planes=True))


def _split(seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(4, 3, S, S, generator=g).to(DEV), torch.rand(4, 3, S, S, generator=g).to(DEV)


def _derived(opt):
    out = {}
    if getattr(opt, "flat_p16", None) is not None:
        out["shadow"] = opt.flat_p16.clone()
    if getattr(opt, "flat_p3", None) is not None:
        out["planes"] = opt.flat_p3.clone()
        if opt.flat_p3t is not None:
            out["planes_t"] = opt.flat_p3t.clone()
    return out


def _fresh_derived(opt):
    """The operand forms split afresh from the optimiser's current flat weights."""
    out = {}
    if getattr(opt, "flat_p16", None) is not None:
        out["shadow"] = torch.empty_like(opt.flat_p16)
        ops.f32_to_bf16(opt.flat_p, out["shadow"])
    if getattr(opt, "flat_p3", None) is not None:
        out["planes"] = torch.empty_like(opt.flat_p3)
        ops.f32_to_bf16x3(opt.flat_p, out["planes"])
        if opt.flat_p3t is not None:
            out["planes_t"] = torch.zeros_like(opt.flat_p3t)
            ops.x3_transpose_planes(out["planes"], out["planes_t"], opt._x3t_table)
    return out


def _same_dict(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)) for k in a)


@pytest.mark.parametrize("mode", list(MODES))
def test_swap_context_computes_with_the_ema_and_restores_everything(mode):
    A, B = synthetic_batch(N, S, 5, DEV)
    tA, tB = _split()
    args = dict(ema_decay=0.9)
    tr = DiscoGANTrainer(default_args(**args), device=DEV, image_size=S, seed=1234, **MODES[mode])
    twin = DiscoGANTrainer(default_args(**args), device=DEV, image_size=S, seed=1234, **MODES[mode])
    with pytest.raises(RuntimeError, match="nothing yet"):
        with tr.ema_weights():
            pass
    for i in range(3):
        tr.train_iteration(A, B, i)
        twin.train_iteration(A, B, i)
    opt = tr.optim_gen
    expect = {"f32": set(), "bf16": {"shadow"}, "f32x3": {"planes", "planes_t"}}[mode]
    before = dict(p=opt.flat_p.clone(), ema=tr.ema.flat.clone(), bufs=_gen_buffers(tr), derived=_derived(opt))
    assert set(before["derived"]) == expect
    assert not same_bits(before["p"], before["ema"])
    sds = tr.ema_state_dicts()
    with tr.ema_weights() as inside:
        assert inside is tr
        assert same_bits(opt.flat_p, before["ema"]) and same_bits(tr.ema.flat, before["p"])
        assert _same_dict(_derived(opt), _fresh_derived(opt))          # refresh_derived ran: the kernels read the EMA's operand forms
        if expect:
            assert not _same_dict(_derived(opt), before["derived"])
        outs = tr.sample(tA, tB)
        assert any(not torch.equal(a, b) for a, b in zip(_gen_buffers(tr), before["bufs"]))      # train-mode passes move the statistics
    # a fresh trainer whose generators are loaded from ema_state_dicts() (EMA weights, the live buffers) computes the same images
    fresh = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=99, **MODES[mode])
    fresh.generator_A.load_state_dict(sds["gen_A"])
    fresh.generator_B.load_state_dict(sds["gen_B"])
    want = fresh.sample(tA, tB)
    for a, b, what in zip(outs, want, ("AB", "BA", "ABA", "BAB")):
        assert torch.equal(a, b), f"{mode}: {what} differs from the fresh trainer's"
    live = twin.sample(tA, tB)
    assert not torch.equal(live[0], outs[0])                            # and not what the live weights give
    del fresh

    def restored():
        assert same_bits(opt.flat_p, before["p"]) and same_bits(tr.ema.flat, before["ema"])
        assert all(torch.equal(a, b) for a, b in zip(_gen_buffers(tr), before["bufs"]))
        assert _same_dict(_derived(opt), before["derived"])

    restored()
    with pytest.raises(KeyError, match="inside"):
        with tr.ema_weights():
            tr.sample(tA, tB)
            raise KeyError("inside")
    restored()
    # training goes on as if nothing had happened (the twin never entered the context; its own sample() above moved its running
    # statistics, which train-mode BatchNorm does not read: put them back for the buffer comparison)
    for b, old in zip([b for net in (twin.generator_A, twin.generator_B) for b in net.buffers()], before["bufs"]):
        b.copy_(old)
    for i in range(3, 5):
        la = tr.losses_to_floats(tr.train_iteration(A, B, i))
        lb = twin.losses_to_floats(twin.train_iteration(A, B, i))
        assert la == lb, i
    tr.finish(), twin.finish()
    assert same_bits(opt.flat_p, twin.optim_gen.flat_p) and same_bits(tr.ema.flat, twin.ema.flat)
    assert same_bits(tr.optim_dis.flat_p, twin.optim_dis.flat_p) and tr.ema.updates == twin.ema.updates == 2
    assert all(torch.equal(a, b) for a, b in zip(_gen_buffers(tr), _gen_buffers(twin)))
    assert _same_dict(_derived(opt), _derived(twin.optim_gen))


def test_view_of_keeps_the_parameters_strides():
    tr = DiscoGANTrainer(default_args(ema_decay=0.5), device=DEV, image_size=S, seed=1234)
    A, B = synthetic_batch(N, S, 5, DEV)
    for i in range(2):
        tr.train_iteration(A, B, i)
    krsc = 0
    for p in tr.optim_gen.params:
        v = tr.ema.view_of(p)
        assert v.shape == p.shape and v.stride() == p.stride()
        assert torch.equal(v, p.detach())                                # right after the copy: the same logical tensor
        krsc += int(p.dim() == 4 and ops.is_krsc(p) and not p.is_contiguous())
    assert krsc > 0                                                      # the case a plain .view(shape) would permute
    with pytest.raises(KeyError):
        tr.ema.view_of(tr.optim_dis.params[0])
    sd = tr.ema_state_dicts()
    live = tr.generator_A.state_dict()
    assert list(sd["gen_A"]) == list(live)
    for k, t in sd["gen_A"].items():
        assert not t.is_cuda and t.is_contiguous() and t.dtype == live[k].dtype and t.shape == live[k].shape
        assert torch.equal(t, live[k].cpu()), k


# ---- 8. exact resume --------------------------------------------------------------------------------------------------------------------
def test_resume_continues_the_ema_exactly():
    A, B = synthetic_batch(N, S, 5, DEV)
    args = dict(ema_decay=0.9)
    tr = DiscoGANTrainer(default_args(**args), device=DEV, image_size=S, seed=1234)
    for i in range(3):
        tr.train_iteration(A, B, i)
    st = tr.train_state(3)
    assert st["ema"]["ready"] is True and st["ema"]["updates"] == 1 and st["ema"]["decay"] == 0.9
    assert same_bits(st["ema"]["flat"], tr.ema.flat) and st["ema"]["flat"].data_ptr() != tr.ema.flat.data_ptr()
    for i in range(3, 6):
        tr.train_iteration(A, B, i)
    tr.finish()
    again = DiscoGANTrainer(default_args(**args), device=DEV, image_size=S, seed=4321)
    assert again.load_train_state(st) == 3
    for i in range(3, 6):
        again.train_iteration(A, B, i)
    again.finish()
    assert same_bits(again.optim_gen.flat_p, tr.optim_gen.flat_p)
    assert same_bits(again.ema.flat, tr.ema.flat) and again.ema.updates == tr.ema.updates == 3
    # a state written without the EMA: the trainer starts not-ready and the next generator step copies
    bare = {k: v for k, v in st.items() if k != "ema"}
    late = DiscoGANTrainer(default_args(**args), device=DEV, image_size=S, seed=4321)
    late.ema.ready, late.ema.updates = True, 7                           # whatever it held before
    late.load_train_state(bare)
    assert late.ema.ready is False and late.ema.updates == 0
    late.train_iteration(A, B, 3)                                        # a D-step
    assert late.ema.ready is False
    late.train_iteration(A, B, 4)
    assert late.ema.ready and late.ema.updates == 0 and same_bits(late.ema.flat, late.optim_gen.flat_p)
    # a state with the entry into a trainer without the EMA: ignored
    plain = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=4321)
    assert plain.load_train_state(st) == 3 and plain.ema is None


# ---- 9. the CLIs ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ema")
    g = torch.Generator().manual_seed(2)
    for name, n in (("tA", 4), ("tB", 6)):
        torch.save(torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8), tmp / f"{name}.pt")
    return dict(tmp=tmp, runs={})


def _cli(work, tag, extra):
    """One run of the training CLI per tag: synthetic source, 16 px, batch 4, 10 iterations."""
    if tag not in work["runs"]:
        tmp = work["tmp"]
        argv = ["--task_name", "edges2shoes", "--image_size", str(S), "--batch_size", "4", "--epochs", "3", "--max_iters", "10",
                "--log_interval", "1", "--synthetic_size", "16", "--results_dir", str(tmp / f"res_{tag}"),
                "--models_dir", str(tmp / f"mod_{tag}")] + extra
        it_cli.train(it_cli.parse_args(argv))
        work["runs"][tag] = it_cli.train.last_paths
    return work["runs"][tag]


SAVE = ["--image_save_interval", "0", "--model_save_interval", "5", "--save_train_state"]


def _split_flags(work):
    return ["--test_A", str(work["tmp"] / "tA.pt"), "--test_B", str(work["tmp"] / "tB.pt"), "--image_save_interval", "0"]


def _is_buffer(k):
    return "running_" in k or k.endswith("num_batches_tracked")


def _same_files(mp_a, mp_b, names):
    for f in names:
        a, b = torch.load(mp_a / f), torch.load(mp_b / f)
        assert list(a) == list(b), f
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (f, k)


LIVE = [f"{net}_{tag}.pth" for net in ("gen_A", "gen_B", "dis_A", "dis_B") for tag in ("0", "5", "final")]


def test_cli_writes_ema_checkpoints_next_to_the_live_ones(work):
    rp, mp = _cli(work, "ema", ["--ema_decay", "0.99"] + SAVE)
    names = sorted(os.listdir(mp))
    assert [f for f in names if "_ema_" in f] == ["gen_A_ema_5.pth", "gen_A_ema_final.pth", "gen_B_ema_5.pth", "gen_B_ema_final.pth"]
    assert set(LIVE) <= set(names)                                   # tag 0 is saved behind a D-step: no EMA yet, no EMA file
    for g in ("gen_A", "gen_B"):
        for tag in ("5", "final"):
            live, ema = torch.load(mp / f"{g}_{tag}.pth"), torch.load(mp / f"{g}_ema_{tag}.pth")
            assert list(live) == list(ema)
            differ = []
            for k in live:
                assert live[k].shape == ema[k].shape and live[k].dtype == ema[k].dtype and ema[k].is_contiguous(), (g, tag, k)
                if _is_buffer(k):
                    assert torch.equal(live[k], ema[k]), (g, tag, k)
                elif not torch.equal(live[k], ema[k]):
                    differ.append(k)
            first_conv = next(k for k in live if live[k].dim() == 4)
            assert first_conv in differ, (g, tag, differ)
    st = torch.load(mp / "train_state_5.pth")
    assert st["iters"] == 6 and st["ema"]["ready"] and st["ema"]["updates"] == 3 and st["ema"]["decay"] == 0.99


def test_cli_without_ema_decay_is_the_same_run_and_writes_nothing_extra(work):
    rp, mp = _cli(work, "ema", ["--ema_decay", "0.99"] + SAVE)
    rp0, mp0 = _cli(work, "off", SAVE)
    assert not [f for f in os.listdir(mp0) if "_ema_" in f]
    assert "ema" not in torch.load(mp0 / "train_state_5.pth")
    assert open(rp / "training_log.txt", "rb").read() == open(rp0 / "training_log.txt", "rb").read()
    _same_files(mp, mp0, LIVE)


def test_cli_resume_reproduces_the_ema_files(work):
    rp, mp = _cli(work, "ema", ["--ema_decay", "0.99"] + SAVE)
    rp2, mp2 = _cli(work, "resumed", ["--ema_decay", "0.99"] + SAVE + ["--resume", str(mp / "train_state_5.pth")])
    _same_files(mp, mp2, ["gen_A_ema_final.pth", "gen_B_ema_final.pth"] + [f for f in LIVE if f.endswith("_final.pth")])
    assert torch.load(mp2 / "train_state_final.pth")["ema"]["updates"] == torch.load(mp / "train_state_final.pth")["ema"]["updates"] == 5


def test_cli_final_save_says_when_the_ema_never_started(work, capsys):
    rp, mp = _cli(work, "never", ["--ema_decay", "0.99", "--ema_start_iter", "1000", "--image_save_interval", "0"])
    out = capsys.readouterr().out
    assert out.count("no gen_*_ema_final.pth is written") == 1
    assert not [f for f in os.listdir(mp) if "_ema_" in f]


def test_evaluate_and_inference_use_ema(work, capsys):
    tmp = work["tmp"]
    _, mp = _cli(work, "ema", ["--ema_decay", "0.99"] + SAVE)
    base = ["--model_path", str(mp), "--test_A", str(tmp / "tA.pt"), "--test_B", str(tmp / "tB.pt"), "--image_size", str(S),
            "--use_extra_layers", "--paired"]
    res = evaluate.main(base + ["--use_ema", "--output", str(tmp / "eval_ema.json")])
    live = evaluate.main(base + ["--output", str(tmp / "eval_live.json")])
    assert json.load(open(tmp / "eval_ema.json")) == res and res != live
    tA = ops.u8hwc_to_f32chw(torch.load(tmp / "tA.pt").to(DEV))
    tB = ops.u8hwc_to_f32chw(torch.load(tmp / "tB.pt").to(DEV))
    g_ab, path_ab = inference.load_generator(mp, "AtoB", S, DEV, True, fold=True, ema=True)
    g_ba, path_ba = inference.load_generator(mp, "BtoA", S, DEV, True, fold=True, ema=True)
    assert path_ab.name == "gen_B_ema_final.pth" and path_ba.name == "gen_A_ema_final.pth"       # the AtoB -> gen_B naming trap, kept
    AB, BA = g_ab(tA), g_ba(tB)
    ABA, BAB = g_ba(AB), g_ab(BA)
    want = dict(recon_A=(tA, ABA), recon_B=(tB, BAB), trans_AB=(tB[:4], AB[:4]), trans_BA=(tA[:4], BA[:4]))
    assert set(res) == set(want)
    for name, (ref, got) in want.items():
        assert res[name] == evaluate.summarise(ops.image_metrics(ref, got).cpu()), name
    # the not-found message names the file that was looked for
    _, mp0 = _cli(work, "off", SAVE)
    with pytest.raises(FileNotFoundError, match="gen_B_ema_final.pth"):
        evaluate.main(["--model_path", str(mp0)] + base[2:] + ["--use_ema"])
    capsys.readouterr()
    inp = tmp / "batch.pt"
    torch.save(torch.load(tmp / "tA.pt"), inp)
    common = ["--input_path", str(inp), "--image_size", str(S), "--use_extra_layers"]
    assert inference.main(["--model_path", str(mp0), "--output_dir", str(tmp / "inf0")] + common + ["--use_ema"]) is None
    assert "gen_B_ema_final.pth not found" in capsys.readouterr().out
    out = inference.main(["--model_path", str(mp), "--output_dir", str(tmp / "inf")] + common + ["--use_ema"])
    assert "gen_B_ema_final.pth" in capsys.readouterr().out
    (_, generated, reconstructed), = out
    assert torch.equal(generated, AB) and torch.equal(reconstructed, ABA)
    (_, gen_live, _), = inference.main(["--model_path", str(mp), "--output_dir", str(tmp / "inf_live")] + common)
    assert not torch.equal(gen_live, generated)


def test_cli_ema_samples_scores_the_ema_and_leaves_the_live_run_alone(work):
    """Events at iterations 0, 4, 8.  The first comes behind a D-step, before any EMA exists: live weights, as without the flag, and like
    every live event it moves the generators' running statistics by two forward calls.  The other two run inside ema_weights() and
    leave nothing behind.  So the checkpoints of this run are, bit for bit and running statistics included, those of a run whose only
    event is the one at iteration 0 (--eval_interval 100); against a run with sampling off altogether everything but the generators'
    running statistics is equal and the counters are ahead by exactly that one event."""
    ema = ["--ema_decay", "0.99"]
    rp, mp = _cli(work, "samples_ema", ema + _split_flags(work) + ["--eval_interval", "4", "--ema_samples"])
    lines = open(rp / "eval_log.txt").read().splitlines()
    assert len(lines) == 3 and [ln.split("]")[0] for ln in lines] == ["Eval [0", "Eval [4", "Eval [8"]
    assert [ln.endswith(" [ema]") for ln in lines] == [False, True, True], lines
    rp_live, mp_live = _cli(work, "samples_live", ema + _split_flags(work) + ["--eval_interval", "4"])
    lines_live = open(rp_live / "eval_log.txt").read().splitlines()
    assert not any(ln.endswith("[ema]") for ln in lines_live)
    assert lines_live[0] == lines[0] and lines_live[1] + " [ema]" != lines[1] and lines_live[2] + " [ema]" != lines[2]
    assert open(rp / "training_log.txt", "rb").read() == open(rp_live / "training_log.txt", "rb").read()
    finals = [f"{net}_final.pth" for net in ("gen_A", "gen_B", "dis_A", "dis_B")]
    ema_finals = ["gen_A_ema_final.pth", "gen_B_ema_final.pth"]
    rp_one, mp_one = _cli(work, "samples_first_only", ema + _split_flags(work) + ["--eval_interval", "100"])
    assert len(open(rp_one / "eval_log.txt").read().splitlines()) == 1
    _same_files(mp, mp_one, finals + ema_finals)
    rp_off, mp_off = _cli(work, "samples_off", ema + ["--eval_interval", "0", "--image_save_interval", "0"])
    assert not (rp_off / "eval_log.txt").exists()
    for f in finals + ema_finals:
        a, off, live = torch.load(mp / f), torch.load(mp_off / f), torch.load(mp_live / f)
        for k in a:
            if not (f.startswith("gen") and _is_buffer(k)):
                assert torch.equal(a[k], off[k]) and torch.equal(a[k], live[k]), (f, k)
            elif k.endswith("num_batches_tracked"):
                assert int(a[k]) - int(off[k]) == 2 and int(live[k]) - int(off[k]) == 2 * 3, (f, k)


# ---- 10. two ranks on one GPU -----------------------------------------------------------------------------------------------------------
W, DP_ITERS = 2, 7
DP_MODES = dict(plain=dict(overlap_comm=False, use_graph=False), overlap=dict(overlap_comm=True, use_graph=False, bucket_mb=0.05),
                seggraph=dict(overlap_comm="graph", use_graph=True))


def _ema_worker(rank, world, initfile, outdir, mode):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    try:
        from discogan_modernized_amd import dp
        from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch
        torch.cuda.set_device(0)
        tr = DiscoGANTrainer(default_args(ema_decay=0.9), device="cuda:0", image_size=S, seed=1234, process_group=dist.group.WORLD,
                             **DP_MODES[mode])
        assert tr.world_size == world and tr.graph_overlap == (mode == "seggraph") and tr.overlap_comm == (mode == "overlap")
        A, B = synthetic_batch(N, S, dp.rank_data_seed(rank), "cuda:0")
        snaps = []
        for i in range(DP_ITERS):
            tr.train_iteration(A, B, i)
            if mode == "plain" and not tr.is_dis_step(i):          # (the other modes are left to their own stream ordering)
                snaps.append(tr.optim_gen.flat_p.cpu())
        tr.finish()
        torch.cuda.synchronize()
        if mode == "overlap":
            assert tr._buckets.launched > 0
        torch.save(dict(ema=tr.ema.flat.cpu(), gen=tr.optim_gen.flat_p.cpu(), updates=tr.ema.updates, ready=tr.ema.ready, snaps=snaps),
                   os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
        tr.close()
    finally:
        dist.destroy_process_group()


_DP = {}


def _dp_run(mode):
    if mode not in _DP:
        import torch.multiprocessing as mp
        with tempfile.TemporaryDirectory() as d:
            mp.spawn(_ema_worker, args=(W, os.path.join(d, "init"), d, mode), nprocs=W, join=True)
            _DP[mode] = [torch.load(os.path.join(d, f"rank{k}.pt")) for k in range(W)]
    return _DP[mode]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", list(DP_MODES))
def test_two_ranks_keep_one_ema(mode):
    r = _dp_run(mode)
    assert r[0]["ready"] and r[1]["ready"] and r[0]["updates"] == r[1]["updates"] == 3         # G-steps 1, 2, 4, 5: a copy, three lerps
    assert same_bits(r[0]["ema"], r[1]["ema"]) and same_bits(r[0]["gen"], r[1]["gen"])
    assert not same_bits(r[0]["ema"], r[0]["gen"])
    if mode == "plain":
        want = ema_ref.recursion([s.numpy() for s in r[0]["snaps"]], 0.9)
        assert len(r[0]["snaps"]) == 4 and _eq(r[0]["ema"].numpy(), want)


@pytest.mark.timeout(900)
def test_two_ranks_ema_is_the_same_in_every_dispatch_mode():
    base = _dp_run("plain")[0]
    for mode in ("overlap", "seggraph"):
        r = _dp_run(mode)[0]
        assert same_bits(r["gen"], base["gen"]), mode
        assert same_bits(r["ema"], base["ema"]), mode
