"""The adversarial objectives on the GPU: dg_gan_loss_* against the float64 reference (tests/ganloss_ref.py) within the BCE kernels'
tolerances, the wrong problems those bounds reject, the cross-check with the BCE kernel, the bitwise equalities (repeat, grouped, dead
problems), NaN locality, the discriminators' logits keyword, the trainer on both schedules and the CLI.

Measured on one MI355X, worst error / bound of test 1 over every kind, role, label and shape: loss 0.06, gradient 0.017 for the hard
targets and 0.20 for the smoothed cross entropy; test 2 (against sigmoid + BCE): 0.11."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, losses, model, ops  # noqa: E402
from discogan_modernized_amd import functional as F_  # noqa: E402
from discogan_modernized_amd import image_translation as it_cli  # noqa: E402
from discogan_modernized_amd import trainer as T  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tests import ganloss_ref as GR  # noqa: E402

DEV = "cuda"
GOUT = GR.f32(0.7)
CANARY = -12345.0
_X = {}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _gout(v=GOUT):
    return torch.tensor(v, device=DEV, dtype=torch.float32)


def _logits(n):
    """The fp32 inputs of shape n, host and device, made once."""
    if n not in _X:
        x = GR.logits(n, 100 + n)
        _X[n] = (x, torch.from_numpy(x).to(DEV))
    return _X[n]


def _codes(kind, role):
    return GR.KIND_CODES[kind], GR.ROLE_CODES[role]


def _fwd(xd, kind, role, label=1.0):
    return ops.gan_loss_fwd(xd, *_codes(kind, role), label, out=torch.full((), float("nan"), device=DEV))[0]


def _bwd(xd, kind, role, label=1.0, gout=GOUT):
    return ops.gan_loss_bwd(xd, *_codes(kind, role), label, _gout(gout))


# ---- 1. value and gradient against float64 -----------------------------------------------------------------------------------------------
def test_value_and_gradient_against_float64():
    worst = {"loss": 0.0, "hard": 0.0, "smooth": 0.0}
    for n in GR.SHAPES:
        x, xd = _logits(n)
        for kind, role, label in GR.cases():
            loss, grad = float(_fwd(xd, kind, role, label)), _bwd(xd, kind, role, label).cpu().numpy()
            want, gr = GR.loss_ref(kind, role, x, label), GR.grad_ref(kind, role, x, label, GOUT)
            lr, gratio = GR.loss_ratio(loss, want), GR.grad_ratio(grad, kind, role, gr, label, GOUT)
            key = "smooth" if (kind == "bce_logits" and role == "d_real" and label != 1.0) else "hard"
            worst["loss"], worst[key] = max(worst["loss"], lr), max(worst[key], gratio)
            assert lr <= 1.0, (kind, role, label, n, loss, want)
            assert gratio <= 1.0, (kind, role, label, n, gratio)
    print("dg_gan_loss worst error / bound:", {k: round(v, 4) for k, v in worst.items()})


def test_the_bounds_reject_a_dropped_element_and_a_swapped_role():
    """What a kernel that skips an element, or reads another problem's role, would return is outside the bounds (bce_check's idea):
    evaluated with the kernels themselves on the shortened vector / the other role."""
    for n in (3, 257, 1000):
        x, xd = _logits(n)
        for kind, role, label in GR.cases():
            want, gr = GR.loss_ref(kind, role, x, label), GR.grad_ref(kind, role, x, label, GOUT)
            drop = int(np.argmax(np.abs(GR.term(kind, role, x, label))))
            keep = torch.tensor([i for i in range(n) if i != drop], device=DEV)
            dropped = float(_fwd(xd[keep], kind, role, label)) * (n - 1) / n
            assert GR.loss_ratio(dropped, want) > 1.0, (kind, role, n)
            other = "d_fake" if role != "d_fake" else "g_fake"       # a role of another target (d_real at label 1 and g_fake share one)
            assert GR.loss_ratio(float(_fwd(xd, kind, other)), want) > 1.0, (kind, role, n)
            assert GR.grad_ratio(_bwd(xd, kind, other).cpu().numpy(), kind, role, gr, label, GOUT) > 1.0, (kind, role, n)


# ---- 2. cross-check with the BCE kernel --------------------------------------------------------------------------------------------------
def test_bce_on_logits_equals_the_bce_kernel_on_the_sigmoid():
    """bce_logits on x against the project's sigmoid + BCE kernels on the same x, within the loss tolerance.  The logits are mild
    (ganloss_ref.mild_logits, inside |x| <= 10): the rounding of sigmoid(x) to fp32 limits this comparison, not the kernels."""
    worst = 0.0
    for n in GR.SHAPES:
        x = GR.mild_logits(n, 200 + n)
        xd = torch.from_numpy(x).to(DEV)
        p = ops.act_fwd(xd, ops.ACT_SIGMOID, 0.0)
        for role, label in (("d_real", 1.0), ("d_real", 0.9), ("d_fake", 1.0), ("g_fake", 1.0)):
            got = float(_fwd(xd, "bce_logits", role, label))
            via = float(ops.bce_fwd(p, GR.target(role, label))[0])
            worst = max(worst, GR.loss_ratio(got, via))
            assert abs(got - via) <= GR.loss_bound(via), (n, role, label, got, via)
    print("bce_logits against sigmoid + bce, worst error / bound:", round(worst, 4))


# ---- 3. determinism and grouping -----------------------------------------------------------------------------------------------------------
def test_repeat_is_bitwise():
    for n in (257, 1000):
        _, xd = _logits(n)
        for kind, role, label in GR.cases():
            assert torch.equal(_bits(_fwd(xd, kind, role, label)), _bits(_fwd(xd, kind, role, label)))
            assert torch.equal(_bits(_bwd(xd, kind, role, label)), _bits(_bwd(xd, kind, role, label)))


@pytest.mark.parametrize("g", [2, 3, 4])
def test_grouped_equals_single_calls_bitwise(g):
    L = _lib.load()
    assert L.dg_gan_loss_fwd_g(5, None, 1, 0, None, 1.0, None, None) < 0 and b"(1..4)" in L.dg_last_error()      # 4 = DG_MAX_GROUPS
    roles = ["d_real", "g_fake", "d_fake", "d_real"][:g]
    for n in (3, 256, 257, 1000):
        xs = [torch.from_numpy(GR.logits(n, 300 + 10 * k + n)).to(DEV) for k in range(g)]
        for kind in GR.KINDS:
            for label in GR.labels_of(kind):
                lv = torch.full((g + 2,), CANARY, device=DEV)
                outs = [lv[1 + k] for k in range(g)]
                ops.gan_loss_fwd_g(xs, GR.KIND_CODES[kind], [GR.ROLE_CODES[r] for r in roles], label, outs)
                gouts = [_gout(GR.f32(0.5 + 0.1 * k)) for k in range(g)]
                dxs = ops.gan_loss_bwd_g(xs, GR.KIND_CODES[kind], [GR.ROLE_CODES[r] for r in roles], label, gouts)
                assert float(lv[0]) == CANARY and float(lv[-1]) == CANARY
                for k in range(g):
                    assert torch.equal(_bits(lv[1 + k]), _bits(_fwd(xs[k], kind, roles[k], label))), (kind, n, k)
                    assert torch.equal(_bits(dxs[k]), _bits(_bwd(xs[k], kind, roles[k], label, GR.f32(0.5 + 0.1 * k)))), (kind, n, k)


def test_group_backward_with_a_dead_problem_writes_only_the_live_ones(monkeypatch):
    """GanLossGroupFn's backward launches the problems that received a gradient; the launch writes n elements per live problem and
    nothing outside (outputs between canaries)."""
    n, pad = 257, 64
    bufs = []
    real_empty = torch.empty_like

    def canaried(t, **kw):
        buf = torch.full((t.numel() + 2 * pad,), CANARY, device=t.device, dtype=t.dtype)
        bufs.append(buf)
        return buf[pad:pad + t.numel()].view(t.shape)

    xs = [torch.from_numpy(GR.logits(n, 400 + k)).to(DEV).requires_grad_(True) for k in range(3)]
    roles = [GR.ROLE_CODES[r] for r in ("d_real", "d_fake", "g_fake")]
    calls = []
    inner = ops.gan_loss_bwd_g
    monkeypatch.setattr(ops, "gan_loss_bwd_g", lambda xs_, kind, roles_, label, gouts: (calls.append(list(roles_)), inner(xs_, kind, roles_, label, gouts))[1])
    for kind in GR.KINDS:
        lv = torch.zeros(3, device=DEV)
        a, b, c = F_.GanLossGroupFn.apply(3, GR.KIND_CODES[kind], roles, 1.0, *xs, lv[0], lv[1], lv[2])
        del calls[:], bufs[:]
        monkeypatch.setattr(torch, "empty_like", canaried)
        try:
            ga, gc = torch.autograd.grad(a * 2.0 + c * 3.0, [xs[0], xs[2]], allow_unused=True)     # the middle problem is dead
        finally:
            monkeypatch.setattr(torch, "empty_like", real_empty)
        assert calls == [[roles[0], roles[2]]]
        assert torch.equal(_bits(ga), _bits(_bwd(xs[0].detach(), kind, "d_real", 1.0, 2.0)))
        assert torch.equal(_bits(gc), _bits(_bwd(xs[2].detach(), kind, "g_fake", 1.0, 3.0)))
        assert len(bufs) == 2
        for buf in bufs:
            assert bool((buf[:pad] == CANARY).all()) and bool((buf[-pad:] == CANARY).all()) and not bool((buf[pad:-pad] == CANARY).any())
        (gb,) = torch.autograd.grad(F_.GanLossGroupFn.apply(3, GR.KIND_CODES[kind], roles, 1.0, *xs, lv[0], lv[1], lv[2])[1], [xs[1]])
        assert torch.equal(_bits(gb), _bits(_bwd(xs[1].detach(), kind, "d_fake", 1.0, 1.0)))


def test_modules_and_autograd_nodes():
    x, xd = _logits(64)
    for kind in GR.KINDS:
        crit = losses.GANLoss(kind, 1.0)
        for role in GR.ROLES:
            xr = xd.clone().reshape(64, 1, 1, 1).requires_grad_(True)
            loss = crit(xr, role)
            (loss * 3.0).backward()
            assert torch.equal(_bits(loss), _bits(_fwd(xd, kind, role))) and xr.grad.shape == xr.shape
            assert torch.equal(_bits(xr.grad.reshape(-1)), _bits(_bwd(xd, kind, role, 1.0, 3.0)))
        real, fake = xd.reshape(64, 1, 1, 1), torch.from_numpy(GR.logits(64, 9)).to(DEV).reshape(64, 1, 1, 1)
        dis, gen = losses.get_gan_loss(real, fake, crit)
        want = (_fwd(real.reshape(-1), kind, "d_real") + _fwd(fake.reshape(-1), kind, "d_fake")) * 0.5
        assert torch.equal(_bits(dis), _bits(want)) and torch.equal(_bits(gen), _bits(_fwd(fake.reshape(-1), kind, "g_fake")))
    with pytest.raises(_lib.DiscoganHipError, match="hinge"):
        ops.gan_loss_fwd(xd, ops.GAN_HINGE, ops.GAN_D_REAL, 0.9)
    with pytest.raises(ValueError, match="sizes"):
        ops.gan_loss_fwd_g([xd, xd[:3]], ops.GAN_LSGAN, [0, 1], 1.0, [torch.empty((), device=DEV)] * 2)


# ---- 4. NaN --------------------------------------------------------------------------------------------------------------------------------
def test_a_nan_logit_reaches_the_loss_and_its_own_gradient_element_only():
    for n, at in ((3, 1), (257, 256), (1000, 511)):
        x, xd = _logits(n)
        bad = xd.clone()
        bad[at] = float("nan")
        for kind in GR.KINDS:
            for role in GR.ROLES:                                      # all three roles of every kind (the hinge's differ in code)
                assert bool(torch.isnan(_fwd(bad, kind, role))), (kind, role, n)
                g = _bwd(bad, kind, role)
                nan = torch.isnan(g)
                assert bool(nan[at]) and int(nan.sum()) == 1, (kind, role, n)
                keep = torch.arange(n, device=DEV) != at
                assert torch.equal(_bits(g[keep]), _bits(_bwd(xd, kind, role)[keep])), (kind, role, n)


# ---- 5. model: 16 px, batch 4 ----------------------------------------------------------------------------------------------------------------
S_T, N_T = 16, 4


def test_discriminator_logits_keyword():
    torch.manual_seed(5)
    dA, dB = model.Discriminator(image_size=S_T).to(DEV), model.Discriminator(image_size=S_T).to(DEV)
    keys = list(dA.state_dict().keys())
    A, B = synthetic_batch(N_T, S_T, 5, DEV)
    with torch.no_grad():
        for d, x in ((dA, A), (dB, B)):
            state = {k: v.clone() for k, v in d.state_dict().items()}
            p, feats_p = d(x)
            d.load_state_dict(state)                                   # the same BatchNorm running statistics for the second pass
            z, feats_z = d(x, logits=True)
            assert z.shape == (N_T, 1, 1, 1) and torch.equal(_bits(ops.act_fwd(z, ops.ACT_SIGMOID, 0.0)), _bits(p))
            assert not torch.equal(_bits(z), _bits(p)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(feats_p, feats_z))
            d.load_state_dict(state)
        ps = model.group_discriminators([dA, dA, dB, dB], [A, B, B, A])
        zs = model.group_discriminators([dA, dA, dB, dB], [A, B, B, A], logits=True)
        for (p, fp), (z, fz) in zip(ps, zs):
            assert torch.equal(_bits(ops.act_fwd(z.contiguous(), ops.ACT_SIGMOID, 0.0)), _bits(p))
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(fp, fz))
    assert list(dA.state_dict().keys()) == keys and hasattr(dA, "sigmoid") and not any("sigmoid" in k for k in keys)
    assert keys == list(model.Discriminator(image_size=S_T).state_dict().keys())


# ---- 6. the trainer: 16 px, batch 4 ------------------------------------------------------------------------------------------------------
_RUNS = {}
SLOTS = ((T.A_REAL1, "A_dis_real", "d_real"), (T.A_FAKE0, "A_dis_fake", "d_fake"), (T.A_FAKE1, "A_dis_fake", "g_fake"),
         (T.B_REAL1, "B_dis_real", "d_real"), (T.B_FAKE0, "B_dis_fake", "d_fake"), (T.B_FAKE1, "B_dis_fake", "g_fake"))
LOGGED = ("dis_loss_A", "dis_loss_B", "gen_loss_A", "gen_loss_B", "gen_loss", "dis_loss")


def _snapshot(tr):
    tr.finish()
    torch.cuda.synchronize()
    snap = {f"{side}.{name}": getattr(opt, name).cpu().clone() for side, opt in (("gen", tr.optim_gen), ("dis", tr.optim_dis))
            for name in ("flat_p", "exp_avg", "exp_avg_sq")}
    for k, net in tr.nets.items():
        for name, buf in net.named_buffers():
            snap[f"{k}.{name}"] = buf.detach().cpu().clone()
    return snap


def _differ(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in sorted(a) if not torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                                    b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])]


def _run(key, kind, iters=6, first=0, state=None, args=None, **kw):
    """Iterations ``first .. iters - 1`` of one trainer on one fixed batch; per iteration the discriminator outputs, the loss vector and
    the logged scalars.  One run per key for the module."""
    key = (key, kind)
    if key not in _RUNS:
        A, B = synthetic_batch(N_T, S_T, 5, DEV)
        tr = DiscoGANTrainer(args if args is not None else default_args(gan_loss=kind), device=DEV, image_size=S_T, seed=1234, **kw)
        if state is not None:
            assert tr.load_train_state(state) == first
        per = {}
        for i in range(first, iters):
            out = tr.train_iteration(A, B, i)
            torch.cuda.synchronize()
            per[i] = {name: getattr(out, name).detach().cpu().clone() for name in ("A_dis_real", "A_dis_fake", "B_dis_real", "B_dis_fake", "lossvec") + LOGGED}
        _RUNS[key] = dict(per=per, last=_snapshot(tr), state=tr.train_state(iters), grouped=bool(tr.group_launch))
        del tr
    return _RUNS[key]


KINDS_T = ("lsgan", "hinge")


@pytest.mark.parametrize("kind", KINDS_T)
@pytest.mark.parametrize("key,kw", [("grouped", {}), ("chain", dict(group_launch=False))])
def test_trainer_slots_are_the_objective_of_the_returned_logits(kind, key, kw):
    run = _run(key, kind, **kw)
    assert run["grouped"] == (key == "grouped")
    half = np.float32(0.5)
    for i, it in run["per"].items():
        lv = it["lossvec"].numpy()
        for slot, name, role in SLOTS:
            x = it[name].numpy().reshape(-1)
            assert x.size == N_T
            want = GR.loss_ref(kind, role, x)
            assert abs(float(lv[slot]) - want) <= GR.loss_bound(want), (i, name, role, float(lv[slot]), want)
        # the mix: get_gan_loss's 0.5 (real + fake) and the G_FAKE term, in fp32
        v = {k: np.float32(it[k].item()) for k in LOGGED}
        assert v["dis_loss_A"] == (lv[T.A_REAL1] + lv[T.A_FAKE0]) * half and v["dis_loss_B"] == (lv[T.B_REAL1] + lv[T.B_FAKE0]) * half
        assert v["gen_loss_A"] == lv[T.A_FAKE1] and v["gen_loss_B"] == lv[T.B_FAKE1]
        assert v["dis_loss"] == v["dis_loss_A"] + v["dis_loss_B"] and np.isfinite(v["gen_loss"])
    assert all(bool(torch.isfinite(v).all()) for v in run["last"].values() if v.dtype == torch.float32)
    assert _differ(run["last"], _run(key, "bce", **kw)["last"])      # the objective trains other weights than the default


@pytest.mark.parametrize("kind", KINDS_T)
def test_graph_replay_equals_eager_dispatch(kind):
    for name, kw in (("grouped", {}), ("chain", dict(group_launch=False))):
        eager, graph = _run(name, kind, **kw), _run(name + "_graph", kind, use_graph=True, **kw)
        assert _differ(graph["last"], eager["last"]) == []
        for i in range(6):
            for k in ("lossvec",) + LOGGED:
                assert torch.equal(_bits(graph["per"][i][k]), _bits(eager["per"][i][k])), (name, i, k)


@pytest.mark.parametrize("kind", KINDS_T)
def test_two_chain_equals_grouped_with_single_plans(kind):
    chain = _run("chain", kind, group_launch=False)
    single = _run("grouped_single", kind, group_launch=True, group_plan="single")
    assert single["grouped"] and not chain["grouped"]
    assert _differ(single["last"], chain["last"]) == []
    for i in range(6):
        for k in ("A_dis_real", "B_dis_fake", "lossvec") + LOGGED:
            assert torch.equal(_bits(single["per"][i][k]), _bits(chain["per"][i][k])), (i, k)


@pytest.mark.parametrize("kind", KINDS_T)
def test_resume_continues_bitwise(kind, tmp_path):
    whole = _run("grouped", kind)
    torch.save(_run("head3", kind, iters=3)["state"], tmp_path / "state.pth")
    st = torch.load(tmp_path / "state.pth")
    assert st["iters"] == 3 and not any("gan" in k for k in st)
    tail = _run("resumed", kind, first=3, state=st)
    assert _differ(tail["last"], whole["last"]) == []
    for i in (3, 4, 5):
        assert torch.equal(_bits(tail["per"][i]["lossvec"]), _bits(whole["per"][i]["lossvec"])), i


def test_explicit_bce_equals_the_defaults_bitwise():
    for name, kw in (("grouped", {}), ("chain", dict(group_launch=False))):
        plain = _run(name + "_defaults", "bce", args=default_args(), **kw)
        explicit = _run(name, "bce", **kw)
        assert _differ(plain["last"], explicit["last"]) == []
        for i in range(6):
            for k in ("A_dis_real", "B_dis_fake", "lossvec") + LOGGED:
                assert torch.equal(_bits(plain["per"][i][k]), _bits(explicit["per"][i][k])), (name, i, k)
            p = explicit["per"][i]["A_dis_real"]
            assert float(p.min()) >= 0.0 and float(p.max()) <= 1.0    # the default still returns the sigmoid outputs


def test_label_smoothing_changes_the_real_terms_only():
    """gan_real_label with "bce": the label of the two *_REAL1 terms of the existing kernel, nothing else (first iteration: same weights)."""
    A, B = synthetic_batch(N_T, S_T, 5, DEV)
    outs = {}
    for lab in (1.0, 0.9):
        tr = DiscoGANTrainer(default_args(gan_real_label=lab), device=DEV, image_size=S_T, seed=1234)
        out = tr.train_iteration(A, B, 0)
        torch.cuda.synchronize()
        outs[lab] = (out.lossvec.detach().cpu().clone(), out.A_dis_real.detach().reshape(-1).clone(), out.B_dis_real.detach().reshape(-1).clone())
        del tr
    lv1, lv9 = outs[1.0][0], outs[0.9][0]
    same = [i for i in range(lv1.numel()) if i not in (T.A_REAL1, T.B_REAL1)]
    assert torch.equal(_bits(lv1[same]), _bits(lv9[same]))
    for slot, p in ((T.A_REAL1, outs[0.9][1]), (T.B_REAL1, outs[0.9][2])):
        assert torch.equal(_bits(lv9[slot]), _bits(ops.bce_fwd(p, 0.9)[0].cpu())) and not torch.equal(_bits(lv9[slot]), _bits(lv1[slot]))


def _count_launches(monkeypatch):
    """Record every dg_gan_loss_* / dg_bce_* call of the library and every stand-alone sigmoid over one logit vector."""
    calls = []
    real = _lib.load()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name.startswith(("dg_gan_loss", "dg_bce")):
                return lambda *a, _f=fn, _n=name: (calls.append(_n), _f(*a))[1]
            return fn

    spy = Spy()
    monkeypatch.setattr(_lib, "load", lambda: spy)
    for name in ("act_fwd", "act_fwd_g"):
        inner = getattr(ops, name)

        def wrapped(x, act, *a, _f=inner, _n=name, **k):
            if act == ops.ACT_SIGMOID and (x[0] if isinstance(x, (list, tuple)) else x).numel() == N_T:
                calls.append("sigmoid:" + _n)
            return _f(x, act, *a, **k)

        monkeypatch.setattr(ops, name, wrapped)
    return calls


def test_which_kernels_each_objective_launches(monkeypatch):
    calls = _count_launches(monkeypatch)
    A, B = synthetic_batch(N_T, S_T, 5, DEV)
    for kw, sig, bce, gan in ((dict(), "sigmoid:act_fwd_g", {"dg_bce_fwd_g", "dg_bce_bwd_g"}, {"dg_gan_loss_fwd_g", "dg_gan_loss_bwd_g"}),
                              (dict(group_launch=False), "sigmoid:act_fwd", {"dg_bce_fwd", "dg_bce_bwd"}, {"dg_gan_loss_fwd", "dg_gan_loss_bwd"})):
        for kind in ("bce", "bce_logits", "lsgan", "hinge"):
            tr = DiscoGANTrainer(default_args(gan_loss=kind), device=DEV, image_size=S_T, seed=1234, **kw)
            del calls[:]
            for i in range(3):                                         # a D-step and two G-steps
                tr.train_iteration(A, B, i)
            torch.cuda.synchronize()
            seen = set(calls)
            if kind == "bce":                                          # the default never reaches a dg_gan_loss_* entry point
                assert seen == bce | {sig}, (kw, kind, seen)
            else:                                                      # the others never launch the discriminators' sigmoid, nor the BCE kernels
                assert seen == gan, (kw, kind, seen)
                if not kw:                                             # the grouped schedule keeps its two forward launches per iteration
                    assert calls.count("dg_gan_loss_fwd_g") == 2 * 3
            del tr


def test_trainer_refuses_a_bad_objective():
    with pytest.raises(ValueError, match="unknown adversarial loss"):
        DiscoGANTrainer(default_args(gan_loss="wgan"), device=DEV, image_size=16, seed=1234)
    with pytest.raises(ValueError, match="gan_real_label must be in"):
        DiscoGANTrainer(default_args(gan_loss="lsgan", gan_real_label=0.5), device=DEV, image_size=16, seed=1234)
    with pytest.raises(ValueError, match="hinge"):
        DiscoGANTrainer(default_args(gan_loss="hinge", gan_real_label=0.9), device=DEV, image_size=16, seed=1234)


# ---- 7. CLI ----------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_with_the_objective(tmp_path, capsys):
    argv = ["--task_name", "edges2shoes", "--batch_size", "4", "--epochs", "3", "--log_interval", "1", "--data_source", "synthetic",
            "--synthetic_size", "16", "--image_save_interval", "0", "--image_size", "16", "--max_iters", "3"]
    dirs = lambda name: ["--results_dir", str(tmp_path / name / "res"), "--models_dir", str(tmp_path / name / "mod")]  # noqa: E731
    tr = it_cli.main(argv + dirs("hinge") + ["--gan_loss", "hinge"])
    out = capsys.readouterr().out
    assert "adversarial loss: hinge (real label 1)" in out
    assert tr.gan_loss == "hinge" and tr.gan_kind == ops.GAN_HINGE
    rp, _ = it_cli.train.last_paths
    lines = [ln for ln in open(rp / "training_log.txt").read().splitlines() if ln.startswith("Iter")]
    assert len(lines) == 3
    for ln in lines:
        m = re.search(r"GEN: (\S+)/(\S+), FM: (\S+)/(\S+), RECON: (\S+)/(\S+), DIS: (\S+)/([^\s,]+)", ln)
        assert m is not None and all(np.isfinite(float(v)) for v in m.groups()), ln
    tr = it_cli.main(argv + dirs("plain"))
    assert tr.gan_loss == "bce" and "adversarial loss" not in capsys.readouterr().out
    it_cli.main(argv + dirs("smooth") + ["--gan_loss", "lsgan", "--gan_real_label", "0.9"])
    assert "adversarial loss: lsgan (real label 0.9)" in capsys.readouterr().out
