"""The adversarial objectives without a GPU: the float64 reference (tests/ganloss_ref.py) against torch autograd, the bounds of the GPU
test against an fp32 evaluation and against wrong problems, argument validation of losses / trainer / CLI (raised before any device
call), and the library's refusals (negative status, message, no launch)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from discogan_modernized_amd import _lib, losses
from discogan_modernized_amd import distributed_image_translation as dit
from discogan_modernized_amd import image_translation as it
from discogan_modernized_amd.trainer import DEFAULTS, DiscoGANTrainer, check_gan_loss, default_args
from tests import ganloss_ref as GR

SPECIAL = np.array([60.0, -60.0, 1.0, -1.0, 0.0])
EPS64 = 2.0 ** -52


def _torch_loss(kind, role, x, real_label):
    tau = GR.target(role, real_label)
    if kind == "bce_logits":
        return TF.binary_cross_entropy_with_logits(x, torch.full_like(x, tau))
    if kind == "lsgan":
        return ((x - tau) ** 2).mean()
    return {"d_real": lambda: torch.relu(1.0 - x).mean(), "d_fake": lambda: torch.relu(1.0 + x).mean(), "g_fake": lambda: -x.mean()}[role]()


@pytest.mark.parametrize("kind,role,label", GR.cases())
def test_reference_equals_torch_autograd_in_float64(kind, role, label):
    """Value and gradient, on random logits and on {+-60, +-1, 0}.  torch forms sigmoid(x) - tau with cancellation, so at a saturated
    logit it is exact to an ABSOLUTE float64 rounding of an O(1) value only: the comparison allows that and nothing else."""
    for data in (np.random.default_rng(7).standard_normal(97) * 5.0, SPECIAL, GR.logits(257, 3).astype(np.float64)):
        x = torch.tensor(data, dtype=torch.float64, requires_grad=True)
        loss = _torch_loss(kind, role, x, label)
        loss.backward()
        want, g = float(loss.detach()), x.grad.numpy()
        assert abs(GR.loss_ref(kind, role, data, label) - want) <= 8 * EPS64 * max(1.0, abs(want))
        gr = GR.grad_ref(kind, role, data, label)
        assert np.all(np.abs(gr - g) <= (4 * EPS64 + 1e-12 * np.abs(g)) / data.size), (kind, role, label)


def test_kink_convention_and_targets():
    assert [GR.target(r, 0.9) for r in GR.ROLES] == [GR.f32(0.9), 0.0, 1.0]
    assert GR.deriv("hinge", "d_real", [1.0, np.nextafter(1.0, 0.0), 2.0]).tolist() == [0.0, -1.0, 0.0]
    assert GR.deriv("hinge", "d_fake", [-1.0, np.nextafter(-1.0, 0.0), -2.0]).tolist() == [0.0, 1.0, 0.0]
    assert GR.deriv("hinge", "g_fake", [-1.0, 1.0, 7.0]).tolist() == [-1.0, -1.0, -1.0]
    assert GR.deriv("bce_logits", "g_fake", 60.0) == pytest.approx(-np.exp(-60.0), rel=1e-14)       # non-zero where 1 - sigmoid rounds to 0
    assert GR.deriv("bce_logits", "d_fake", -60.0) == pytest.approx(np.exp(-60.0), rel=1e-14)
    assert GR.term("bce_logits", "d_fake", 60.0) == pytest.approx(60.0, rel=1e-14)                  # no clamp at 100
    with pytest.raises(ValueError):
        GR.term("hinge", "d_real", 0.0, 0.9)
    assert len(GR.cases()) == 3 + 1 + 3 + 1 + 3


def _fp32_model(kind, role, x, label, gout):
    """The formulas evaluated in plain fp32 numpy (double accumulation of the mean, as the kernel has it)."""
    one, tau = np.float32(1.0), np.float32(GR.target(role, label))
    n = np.float32(x.size)
    if kind == "lsgan":
        f, d = (x - tau) * (x - tau), np.float32(2.0) * (x - tau)
    elif kind == "hinge":
        f = {"d_real": np.maximum(one - x, 0), "d_fake": np.maximum(one + x, 0), "g_fake": -x}[role].astype(np.float32)
        d = {"d_real": -(x < 1).astype(np.float32), "d_fake": (x > -1).astype(np.float32), "g_fake": -np.ones_like(x)}[role]
    else:
        e = np.exp(-np.abs(x)).astype(np.float32)
        f = np.log1p(e).astype(np.float32) + np.where(x > 0, (one - tau) * x, -tau * x).astype(np.float32)
        big, small = one / (one + e), e / (one + e)
        sig = np.where(x >= 0, big, small)
        d = np.where(x >= 0, -small, -big) if tau == 1 else (sig if tau == 0 else sig - tau)
    return np.float32(f.astype(np.float64).sum() / x.size), (np.float32(gout) * d.astype(np.float32) / n).astype(np.float32)


def test_bounds_hold_for_an_fp32_evaluation_and_reject_wrong_problems():
    """The GPU test's bounds at its shapes and inputs: an fp32 evaluation of the formulas sits well inside, a dropped element and a
    swapped role are outside."""
    gout = GR.f32(0.7)
    worst = {"loss": 0.0, "hard": 0.0, "smooth": 0.0}
    for n in GR.SHAPES:
        x = GR.logits(n, 100 + n)
        for kind, role, label in GR.cases():
            loss, grad = _fp32_model(kind, role, x, label, gout)
            want, gr = GR.loss_ref(kind, role, x, label), GR.grad_ref(kind, role, x, label, gout)
            key = "smooth" if (kind == "bce_logits" and role == "d_real" and label != 1.0) else "hard"
            worst["loss"] = max(worst["loss"], GR.loss_ratio(loss, want))
            worst[key] = max(worst[key], GR.grad_ratio(grad, kind, role, gr, label, gout))
            if n >= 3:
                t = GR.term(kind, role, x, label)                      # (from n = 3 on 60 and -60 are planted: one of them is a large term)
                dropped = float((t.sum() - t[np.argmax(np.abs(t))]) / n)    # an element that was never summed
                assert GR.loss_ratio(dropped, want) > 1.0, (kind, role, n)
                other = "d_fake" if role != "d_fake" else "g_fake"           # a role of another target (d_real at label 1 and g_fake share one)
                assert GR.loss_ratio(GR.loss_ref(kind, other, x, 1.0), want) > 1.0, (kind, role, other, n)
                assert GR.grad_ratio(GR.grad_ref(kind, other, x, 1.0, gout), kind, role, gr, label, gout) > 1.0, (kind, role, other, n)
    print("worst ratio of an fp32 evaluation:", worst)
    assert worst["loss"] < 0.5 and worst["hard"] < 0.5 and worst["smooth"] < 0.5


def test_check_and_module_validation():
    assert losses.GAN_KINDS == ("bce", "bce_logits", "lsgan", "hinge")
    assert check_gan_loss("lsgan", 0.9) == ("lsgan", 0.9) and check_gan_loss("hinge") == ("hinge", 1.0) and check_gan_loss("bce", 1) == ("bce", 1.0)
    with pytest.raises(ValueError, match="one of bce, bce_logits, lsgan, hinge"):
        check_gan_loss("wgan")
    for bad in (0.5, 0.0, 1.01, -1.0, float("nan"), float("inf"), "soft", None):
        with pytest.raises(ValueError, match="gan_real_label must be"):
            check_gan_loss("lsgan", bad)
    with pytest.raises(ValueError, match="hinge"):
        check_gan_loss("hinge", 0.9)
    m = losses.GANLoss("lsgan", 0.9)
    assert (m.kind, m.real_label) == ("lsgan", 0.9) and losses.GANLoss("hinge").real_label == 1.0
    for args in (("wgan",), ("hinge", 0.9), ("lsgan", 2.0), ("bce",)):
        with pytest.raises(ValueError):
            losses.GANLoss(*args)
    with pytest.raises(ValueError, match="unknown role"):
        m(torch.zeros(4), "real")                                     # refused before the tensor is looked at
    assert losses.GAN_KIND_CODES == GR.KIND_CODES and losses.GAN_ROLES == GR.ROLE_CODES


def test_trainer_validates_before_any_device_call(monkeypatch):
    assert DEFAULTS["gan_loss"] == "bce" and DEFAULTS["gan_real_label"] == 1.0
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    for over, msg in ((dict(gan_loss="wgan"), "unknown adversarial loss"), (dict(gan_real_label=0.4), "gan_real_label must be"),
                      (dict(gan_loss="lsgan", gan_real_label=float("nan")), "gan_real_label must be"),
                      (dict(gan_loss="hinge", gan_real_label=0.9), "hinge")):
        with pytest.raises(ValueError, match=msg):
            DiscoGANTrainer(default_args(**over), device="cuda", image_size=16, seed=1234)


def test_cli_flags_and_defaults():
    for parse in (lambda argv: it.build_parser().parse_args(argv), dit.parse_args):
        a = parse([])
        assert (a.gan_loss, a.gan_real_label) == ("bce", 1.0)
        a = parse(["--gan_loss", "lsgan", "--gan_real_label", "0.9"])
        assert (a.gan_loss, a.gan_real_label) == ("lsgan", 0.9)
        for kind in losses.GAN_KINDS:
            assert parse(["--gan_loss", kind]).gan_loss == kind
        with pytest.raises(SystemExit):
            parse(["--gan_loss", "wgan"])
    args = it.build_parser().parse_args(["--gan_loss", "hinge", "--gan_real_label", "0.9", "--task_name", "edges2shoes"])
    with pytest.raises(ValueError, match="hinge"):                    # before the device is asked for
        it.train(args)


def test_library_refuses_bad_arguments_without_a_launch():
    """Every refusal of dg_gan_loss_*: a negative status and a message, before anything is dereferenced or launched (the pointers are
    dummies, and this machine may have no device)."""
    L = _lib.load()
    P = C.c_void_p
    tab = (P * 4)(8, 8, 8, 8)
    holed = (P * 4)(8, None, 8, 8)
    roles = (C.c_int * 4)(0, 1, 2, 0)

    def fwd(groups=2, x=tab, n=4, kind=1, role=roles, label=1.0, loss=tab):
        return L.dg_gan_loss_fwd_g(groups, x, n, kind, role, label, loss, None)

    def bwd(groups=2, x=tab, n=4, kind=1, role=roles, label=1.0, gout=tab, dx=tab):
        return L.dg_gan_loss_bwd_g(groups, x, n, kind, role, label, gout, dx, None)

    for call in (fwd, bwd):
        for kw, msg in ((dict(groups=0), b"groups"), (dict(groups=5), b"groups"), (dict(groups=-1), b"groups"),
                        (dict(x=None), b"null pointer table"), (dict(x=holed), b"null pointer (problem 1)"),
                        (dict(role=None), b"null role table"), (dict(n=0), b"n=0"), (dict(n=-3), b"n=-3"),
                        (dict(kind=3), b"unknown kind"), (dict(kind=-1), b"unknown kind"),
                        (dict(role=(C.c_int * 4)(0, 3, 0, 0)), b"unknown role 3 (problem 1)"), (dict(role=(C.c_int * 4)(-1, 0, 0, 0)), b"unknown role"),
                        (dict(label=float("nan")), b"real_label"), (dict(label=float("inf")), b"real_label"), (dict(label=0.5), b"real_label"),
                        (dict(label=1.5), b"real_label"), (dict(label=-0.9), b"real_label"),
                        (dict(kind=2, label=0.9), b"hinge")):
            assert call(**kw) < 0, kw
            assert msg in L.dg_last_error(), (kw, L.dg_last_error())
    assert fwd(loss=None) < 0 and fwd(loss=holed) < 0 and bwd(gout=None) < 0 and bwd(dx=holed) < 0 and bwd(gout=holed) < 0
    # a role beyond `groups` is not read
    assert fwd(groups=1, role=(C.c_int * 4)(0, 9, 9, 9), n=0) < 0 and b"n=0" in L.dg_last_error()
    # the single forms
    assert L.dg_gan_loss_fwd(None, 4, 1, 0, 1.0, 8, None) < 0 and b"null pointer" in L.dg_last_error()
    assert L.dg_gan_loss_fwd(8, 4, 1, 0, 1.0, None, None) < 0
    assert L.dg_gan_loss_fwd(8, 0, 1, 0, 1.0, 8, None) < 0 and L.dg_gan_loss_fwd(8, 4, 7, 0, 1.0, 8, None) < 0
    assert L.dg_gan_loss_fwd(8, 4, 1, 3, 1.0, 8, None) < 0 and L.dg_gan_loss_fwd(8, 4, 2, 0, 0.9, 8, None) < 0
    assert L.dg_gan_loss_bwd(8, 4, 1, 0, 1.0, None, 8, None) < 0 and L.dg_gan_loss_bwd(8, 4, 1, 0, 1.0, 8, None, None) < 0
    assert L.dg_gan_loss_bwd(None, 4, 1, 0, 1.0, 8, 8, None) < 0 and L.dg_gan_loss_bwd(8, 4, 0, 0, 0.3, 8, 8, None) < 0
