"""Loss criteria and helpers with the reference's signatures (image_translation.py:136-168, 267-269).

``get_gan_loss`` / ``get_fm_loss`` keep the argument order ``(…, criterion, device)`` and the return
order ``(dis_loss, gen_loss)``.  Labels are constants (ones / zeros), so they are passed to the BCE
kernel as a scalar instead of being materialised on the host and copied every call
(image_translation.py:157-159 — pure overhead in the reference).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import functional as F
from . import ops


class MSELoss(nn.Module):
    """nn.MSELoss() (mean reduction)."""

    def forward(self, input, target):
        return F.MSELossFn.apply(input, target)


RECON_KINDS = ("mse", "l1", "ssim", "l1_ssim", "ms_ssim", "l1_ms_ssim")
MS_SSIM_KINDS = ("ms_ssim", "l1_ms_ssim")           # the third weight multiplies 1 - MS-SSIM (dg_ms_ssim_loss_fwd), not 1 - SSIM
MS_SSIM_EXPONENTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def ms_ssim_max_scales(image_size):
    """min(5, number of j with image_size >> j >= 11): every scale of the pyramid must hold the 11 x 11 window (dg_ms_ssim_max_scales;
    0 under 11 pixels, 11 -> 1, 22 -> 2, 64 -> 3, 176 and more -> 5)."""
    m = 0
    while m < len(MS_SSIM_EXPONENTS) and (int(image_size) >> m) >= 11:
        m += 1
    return m


def ms_ssim_scales(scales, image_size):
    """The scale count of an MS-SSIM criterion at ``image_size``: ``scales`` itself, or the maximum for 0; ValueError when the size
    cannot carry it."""
    top = ms_ssim_max_scales(image_size)
    if top < 1:
        raise ValueError(f"multi-scale SSIM needs image_size >= 11 (the 11 x 11 SSIM window), got {image_size}")
    M = int(scales)
    if M == 0:
        return top
    if not 1 <= M <= top:
        raise ValueError(f"recon_ms_scales {M} does not fit image_size {image_size}: every scale needs a side >= 11, so 1..{top} "
                         "(0: the maximum)")
    return M


def recon_weights(kind, alpha=0.84):
    """The weights ``(w_mse, w_l1, w_ssim)`` of a reconstruction criterion (``dg_recon_loss_fwd``): ``mse`` -> (1, 0, 0), ``l1`` ->
    (0, 1, 0), ``ssim`` -> (0, 0, 1) (the loss is 1 - SSIM), ``l1_ssim`` -> (0, 1 - alpha, alpha) (Zhao et al. 2017: alpha = 0.84).
    ``ms_ssim`` and ``l1_ms_ssim`` (MS_SSIM_KINDS) have the tables of ``ssim`` and ``l1_ssim``; their third weight is w_ms of
    ``dg_ms_ssim_loss_fwd``."""
    if kind == "mse":
        return (1.0, 0.0, 0.0)
    if kind == "l1":
        return (0.0, 1.0, 0.0)
    if kind in ("ssim", "ms_ssim"):
        return (0.0, 0.0, 1.0)
    if kind in ("l1_ssim", "l1_ms_ssim"):
        alpha = float(alpha)
        if not 0.0 < alpha < 1.0:
            raise ValueError(f"recon_ssim_alpha must be in (0, 1), got {alpha}")
        return (0.0, 1.0 - alpha, alpha)
    raise ValueError(f"unknown reconstruction loss {kind!r} (one of {', '.join(RECON_KINDS)})")


class ReconLoss(nn.Module):
    """``w_mse mean (x - t)^2 + w_l1 mean |x - t| + w_ssim (1 - mean SSIM)`` of an image batch ``input`` [n,3,S,S] against the data
    ``target`` (no gradient flows into it), weights by ``recon_weights(kind, alpha)``.  SSIM: 11 x 11 Gaussian window of sigma 1.5,
    valid windows, data range 1 -- the quantity ``ops.image_metrics`` reports."""

    def __init__(self, kind="l1_ssim", alpha=0.84):
        super().__init__()
        if kind in MS_SSIM_KINDS:
            raise ValueError(f"ReconLoss is the single-scale criterion: {kind!r} is MSSSIMLoss")
        self.kind = kind
        self.weights = recon_weights(kind, alpha)

    def forward(self, input, target):
        return F.ReconLossFn.apply(input, target, self.weights)


class MSSSIMLoss(nn.Module):
    """``w_l1 mean |x - t| + w_ms (1 - mean MS-SSIM)`` of an image batch ``input`` [n,3,S,S] against the data ``target`` (no gradient
    flows into it): kind ``ms_ssim`` (1 - MS-SSIM) or ``l1_ms_ssim`` ((1 - alpha) L1 + alpha (1 - MS-SSIM), Zhao et al. 2017: alpha =
    0.84).  MS-SSIM (Wang, Simoncelli, Bovik 2003) over ``scales`` levels of a 2 x 2 average pyramid (0: as many as the input's size
    carries, at most 5), the quantity ``ops.image_ms_ssim`` reports."""

    def __init__(self, kind="l1_ms_ssim", alpha=0.84, scales=0):
        super().__init__()
        if kind not in MS_SSIM_KINDS:
            raise ValueError(f"MSSSIMLoss takes one of {', '.join(MS_SSIM_KINDS)}, got {kind!r}")
        self.kind = kind
        self.weights = recon_weights(kind, alpha)
        self.scales = int(scales)

    def forward(self, input, target):
        return F.MsSsimLossFn.apply(input, target, ms_ssim_scales(self.scales, input.shape[-1]), self.weights)


class L1Loss(ReconLoss):
    """nn.L1Loss() (mean reduction) of an image batch against data."""

    def __init__(self):
        super().__init__("l1")


class SSIMLoss(ReconLoss):
    """1 - mean SSIM of an image batch against data."""

    def __init__(self):
        super().__init__("ssim")


class BCELoss(nn.Module):
    """nn.BCELoss() (mean reduction, log clamped at -100).  ``target`` is a tensor of the input's size, as in the
    reference (image_translation.py:157-166), or a Python scalar label (1.0 / 0.0), which skips materialising it."""

    def forward(self, input, target):
        if isinstance(target, torch.Tensor):
            label = getattr(target, "_dg_label", None)
            if label is None:
                return F.BCETargetLossFn.apply(input, target.to(input.device))
        else:
            label = float(target)
        return F.BCELossFn.apply(input, label)


GAN_KINDS = ("bce", "bce_logits", "lsgan", "hinge")
GAN_KIND_CODES = {"bce_logits": ops.GAN_BCE_LOGITS, "lsgan": ops.GAN_LSGAN, "hinge": ops.GAN_HINGE}     # ("bce": the reference's sigmoid + BCELoss)
GAN_ROLES = {"d_real": ops.GAN_D_REAL, "d_fake": ops.GAN_D_FAKE, "g_fake": ops.GAN_G_FAKE}


def check_gan_loss(kind, real_label=1.0):
    """The adversarial objective ``kind`` (one of GAN_KINDS) and the target ``real_label`` of a discriminator's real batch (one-sided
    label smoothing: finite, in (0.5, 1]; the hinge has no target and takes 1 only).  Returns ``(kind, real_label as a float)``."""
    if kind not in GAN_KINDS:
        raise ValueError(f"unknown adversarial loss {kind!r} (one of {', '.join(GAN_KINDS)})")
    try:
        label = float(real_label)
    except (TypeError, ValueError):
        raise ValueError(f"gan_real_label must be a number in (0.5, 1], got {real_label!r}") from None
    if not 0.5 < label <= 1.0:                              # (a NaN fails both comparisons)
        raise ValueError(f"gan_real_label must be in (0.5, 1], got {real_label!r}")
    if kind == "hinge" and label != 1.0:
        raise ValueError(f"the hinge objective has no target to smooth: gan_real_label must be 1 with gan_loss 'hinge', got {real_label!r}")
    return kind, label


class GANLoss(nn.Module):
    """An adversarial objective on a discriminator's LOGITS (``Discriminator(x, logits=True)``), called as ``(logits, role)`` with role
    ``"d_real"`` (target ``real_label``), ``"d_fake"`` (target 0) or ``"g_fake"`` (target 1): ``bce_logits`` = binary cross entropy of
    sigmoid(x) in its stable form, ``lsgan`` = mean (x - target)^2, ``hinge`` = mean max(0, 1 -+ x) for the discriminator and -mean x for
    the generator (dg_gan_loss_fwd).  ``bce`` is not a kind of this module: it is ``BCELoss`` on the sigmoid output."""

    def __init__(self, kind, real_label=1.0):
        super().__init__()
        kind, self.real_label = check_gan_loss(kind, real_label)
        if kind == "bce":
            raise ValueError("GANLoss works on logits: 'bce' is BCELoss() on the discriminator's sigmoid output (use 'bce_logits' here)")
        self.kind = kind

    def forward(self, logits, role):
        if role not in GAN_ROLES:
            raise ValueError(f"unknown role {role!r} (one of {', '.join(GAN_ROLES)})")
        return F.GanLossFn.apply(logits, GAN_KIND_CODES[self.kind], GAN_ROLES[role], self.real_label)


class HingeEmbeddingLoss(nn.Module):
    """nn.HingeEmbeddingLoss(margin=1.0) (mean reduction), targets in {+1, -1}.  The reference only calls it with
    all-ones targets (image_translation.py:141-142), where it is ``input.mean()``;
    ``get_fm_loss`` below fuses that whole layer term into one kernel and does not go through this module."""

    def __init__(self, margin: float = 1.0):
        super().__init__()
        self.margin = float(margin)

    def forward(self, input, target):
        return F.HingeEmbeddingLossFn.apply(input, target.to(input.device), self.margin)


def label_like(batch_size, value, device):
    t = torch.full((batch_size, 1), float(value), device=device)
    t._dg_label = float(value)
    return t


def get_fm_loss(real_feats, fake_feats, criterion=None, device=None):
    """image_translation.py:136-144: sum over layers of mean_{chw}((mean_n real - mean_n fake)^2)."""
    losses = 0
    for real_feat, fake_feat in zip(real_feats, fake_feats):
        losses = losses + F.FeatureMatchFn.apply(real_feat, fake_feat)
    return losses


def get_gan_loss(dis_real, dis_fake, criterion, device=None):
    """image_translation.py:146-168.  With a ``GANLoss`` criterion ``dis_real`` / ``dis_fake`` are the discriminator's LOGITS, and the
    pair is ``(0.5 (D_REAL + D_FAKE), G_FAKE)``."""
    batch_size = dis_real.size(0)
    if len(dis_real.size()) > 2:
        dis_real = dis_real.view(batch_size, -1)
    if len(dis_fake.size()) > 2:
        dis_fake = dis_fake.view(batch_size, -1)
    if isinstance(criterion, GANLoss):
        return (criterion(dis_real, "d_real") + criterion(dis_fake, "d_fake")) * 0.5, criterion(dis_fake, "g_fake")
    dis_loss = (criterion(dis_real, 1.0) + criterion(dis_fake, 0.0)) * 0.5
    gen_loss = criterion(dis_fake, 1.0)
    return dis_loss, gen_loss
