"""Differentiable augmentation of what a discriminator sees (Zhao et al., NeurIPS 2020, "Differentiable Augmentation for Data-Efficient GAN
Training"), policy ``color,translation,cutout``, on the device.

One random transform per sample on every discriminator input -- reals and fakes, in D-steps and in G-steps, where the gradient flows back
through it into the generator.  Images here live in [0, 1]; the published ops are defined on [-1, 1], so they are implemented conjugated
(brightness amplitude halved, padding and cutout fill 0.5) -- include/discogan_hip.h ("differentiable augmentation") has the exact transform,
its adjoint and the draw.

Two steps per batch, like the image pool's, so that the second can sit inside a captured hipGraph:

  ``draw(iteration, n)``   eager, outside any capture: dg_diffaug_draw writes the batch's records into this object's persistent table -- a
                           pure function of (seed, rank, iteration, domain, role, position), no generator state, no host round trip;
  ``apply(x) -> z``        the transform as an autograd node (functional.DiffAugFn): launches that read only device memory at fixed
                           addresses.  Under graph replay the same nodes apply whatever table the draw in front of the replay left there.

There is no state to checkpoint: a resumed run draws the same records because the draw is keyed on the iteration.
"""
from __future__ import annotations

import torch

from . import ops

POLICIES = dict(color=ops.DIFFAUG_COLOR, translation=ops.DIFFAUG_TRANSLATION, cutout=ops.DIFFAUG_CUTOUT)


def parse_policy(policy):
    """``"color,translation,cutout"`` -> the DG_DIFFAUG_* flags: any subset in any order; ``""`` / ``"none"`` / None -> 0 (off)."""
    if policy is None:
        return 0
    if not isinstance(policy, str):
        raise ValueError(f"diffaug: a comma-separated policy string expected, got {policy!r}")
    names = [p.strip() for p in policy.split(",") if p.strip()]
    if names == ["none"]:
        return 0
    flags = 0
    for p in names:
        if p not in POLICIES:
            raise ValueError(f"diffaug: unknown policy {p!r} (known: color, translation, cutout; '' or 'none' = off)")
        flags |= POLICIES[p]
    return flags


def policy_names(flags):
    return ",".join(k for k, v in POLICIES.items() if flags & v)


class DiffAugment:
    """The transform of one (domain, role) stream of discriminator inputs: domain 0 = A | 1 = B, role 0 = real batch | 1 = fake batch."""

    def __init__(self, flags, image_size, seed, rank, domain, role, device="cuda"):
        if isinstance(flags, bool) or not isinstance(flags, int) or not 0 < flags <= 7:
            raise ValueError(f"DiffAugment needs policy flags in 1..7 (parse_policy), got {flags!r}")
        if domain not in (0, 1) or role not in (0, 1):
            raise ValueError(f"DiffAugment: domain 0 (A) or 1 (B) and role 0 (real) or 1 (fake), got {domain!r}, {role!r}")
        self.flags, self.image_size = flags, int(image_size)
        self.seed, self.rank, self.domain, self.role = int(seed), int(rank), int(domain), int(role)
        self.device = torch.device(device)
        # allocated once for the largest batch the kernels take (32 bytes a row = 128 KiB): its address never changes under a graph
        self.recs = torch.zeros((ops.DIFFAUG_MAX_BATCH, 8), device=self.device, dtype=torch.int32)
        self.drawn = 0                      # samples of the batch the table was last drawn for (0: none yet)

    def draw(self, iteration, n):
        """Draw the records of the batch of ``n`` images that iteration ``iteration`` shows the discriminator.  Eager: call it outside any
        graph capture, before the ``apply`` (or the replay of the graph that holds it)."""
        n = int(n)
        if not 1 <= n <= ops.DIFFAUG_MAX_BATCH:
            raise ValueError(f"DiffAugment.draw: a batch of 1..{ops.DIFFAUG_MAX_BATCH} images, got {n}")
        ops.diffaug_draw(self.seed, self.rank, iteration, self.domain, self.role, n, self.image_size, self.flags, out=self.recs)
        self.drawn = n
        return self.recs[:n]

    def check(self, x):
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, self.image_size, self.image_size):
            raise ValueError(f"DiffAugment: a batch [n,3,{self.image_size},{self.image_size}] expected, got {tuple(x.shape)}")
        if int(x.shape[0]) != self.drawn:
            raise RuntimeError(f"DiffAugment: the record table was drawn for {self.drawn} images, the batch has {x.shape[0]} "
                               "(draw(iteration, n) comes first)")

    def apply(self, x):
        """``x`` [n,3,S,S] -> the batch the discriminator sees, by the records of the last ``draw``; differentiable in x.  Safe to capture."""
        from . import functional as F_
        self.check(x)
        return F_.DiffAugFn.apply(x, self.recs, self.flags)


def apply_group(augs, xs):
    """``augs[i].apply(xs[i])`` for up to ops.MAX_GROUPS batches of one shape in one launch per pass (functional.DiffAugGroupFn)."""
    from . import functional as F_
    flags = augs[0].flags
    for a, x in zip(augs, xs):
        a.check(x)
        if a.flags != flags:
            raise ValueError("apply_group: the transforms of one grouped launch share one policy")
    return F_.DiffAugGroupFn.apply(len(xs), flags, *[a.recs for a in augs], *xs)
