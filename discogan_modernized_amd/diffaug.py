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

``DiffAugment(..., p=...)`` applies every stage to a sample with a probability that the draw kernel reads from device memory
(dg_diffaug_draw_p): a constant (``fixed_p``), or the first field of an ``AdaController``'s control block, which the controller moves on the
device by the discriminator's overfitting measure (Karras et al., NeurIPS 2020, "ADA").  A stage that is gated off writes its neutral record
fields, so the apply kernels and whatever captured them stay as they are.  The controller's ten numbers per domain ARE state: they travel in
``train_state()`` (key ``ada``).
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

    def __init__(self, flags, image_size, seed, rank, domain, role, device="cuda", p=None):
        """``p``: None = every stage on every sample (dg_diffaug_draw), or a float64 tensor ON THE DEVICE whose first element is the
        probability each stage is kept with per sample (dg_diffaug_draw_p): a view of an AdaController's control block, or a constant.
        The draw kernel reads it; the host never does."""
        if isinstance(flags, bool) or not isinstance(flags, int) or not 0 < flags <= 7:
            raise ValueError(f"DiffAugment needs policy flags in 1..7 (parse_policy), got {flags!r}")
        if domain not in (0, 1) or role not in (0, 1):
            raise ValueError(f"DiffAugment: domain 0 (A) or 1 (B) and role 0 (real) or 1 (fake), got {domain!r}, {role!r}")
        if p is not None and not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float64 and p.numel() >= 1):
            raise ValueError("DiffAugment: p is None or a float64 tensor on the device (AdaController.p_view / fixed_p)")
        self.p = p
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
        if self.p is None:
            ops.diffaug_draw(self.seed, self.rank, iteration, self.domain, self.role, n, self.image_size, self.flags, out=self.recs)
        else:
            ops.diffaug_draw_p(self.seed, self.rank, iteration, self.domain, self.role, n, self.image_size, self.flags, self.p, out=self.recs)
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


def fixed_p(p, device="cuda"):
    """A constant probability as the device tensor ``DiffAugment(p=...)`` takes."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"diffaug: a probability in [0, 1] expected, got {p}")
    return torch.full((1,), p, device=device, dtype=torch.float64)


class AdaController:
    """Adaptive discriminator augmentation (Karras et al., NeurIPS 2020): the probability p of both domains' augmentation, the
    overfitting measure r_t = E[sign(D(real) - threshold)] of each discriminator and the controller that moves p, all in device memory
    (include/discogan_hip.h, "adaptive discriminator augmentation").

      ``ctl``   float64 [2, 8], one control block per domain (0 = A, 1 = B): p, r_t of the last closed window (NaN before the first),
                updates done, real outputs counted in total, the last adjustment, 0, 0, 0;  ``p_view(domain)`` is what DiffAugment reads;
      ``acc``   float32 [4]: both domains' windows (sum of signs, count) in one tensor, so that data-parallel ranks exchange them in ONE
                16-byte all-reduce.  Integer-valued: exact below 2^24 and independent of the order of the sum.

    ``accumulate`` after every discriminator step, ``step`` behind it: every ``interval``-th call closes the windows with ``update``,
    which moves p by (real outputs in the window) / (1000 kimg) up when r_t > target, down when below, within [0, p_max].  Every call
    is an eager launch on the current stream that reads only device memory: nothing waits for the host.  ``stats()`` does."""

    def __init__(self, target, interval=4, kimg=500.0, p_max=1.0, p0=0.0, device="cuda"):
        target, kimg, p_max, p0 = float(target), float(kimg), float(p_max), float(p0)
        if not 0.0 < target < 1.0:
            raise ValueError(f"ada_target must lie in (0, 1) (0.6 is customary), got {target}")
        if isinstance(interval, bool) or not isinstance(interval, int) or interval < 1:
            raise ValueError(f"ada_interval must be an integer >= 1 (discriminator steps per update), got {interval!r}")
        if not 1e-3 <= kimg < float("inf"):
            raise ValueError(f"ada_kimg must be >= 0.001 (thousands of real images for p to travel from 0 to 1), got {kimg}")
        if not 0.0 < p_max <= 1.0:
            raise ValueError(f"ada_p_max must lie in (0, 1], got {p_max}")
        if not 0.0 <= p0 <= 1.0:
            raise ValueError(f"diffaug_p (the initial p) must lie in [0, 1], got {p0}")
        self.target, self.interval, self.kimg, self.p_max, self.p0 = target, interval, kimg, p_max, p0
        self.step_per_image = 1.0 / (1000.0 * kimg)
        self.device = torch.device(device)
        self.ctl = torch.zeros((2, 8), device=self.device, dtype=torch.float64)
        self.acc = torch.zeros(4, device=self.device, dtype=torch.float32)
        self.reset()

    def reset(self):
        """Back to p0 with empty windows (also the start of a run whose loaded state holds no controller)."""
        ctl = torch.zeros((2, 8), dtype=torch.float64)
        ctl[:, 0], ctl[:, 1] = self.p0, float("nan")
        self.ctl.copy_(ctl)
        self.acc.zero_()
        self.dsteps = 0                     # discriminator steps accumulated so far: every interval-th closes the windows

    def p_view(self, domain):
        return self.ctl[domain]

    def acc_view(self, domain):
        return self.acc[2 * domain:2 * domain + 2]

    def accumulate(self, domain, d_out, threshold):
        """Add the signs of discriminator ``domain``'s outputs on a real batch to its window (dg_ada_accumulate)."""
        ops.ada_accumulate(d_out.detach().reshape(-1), threshold, self.acc_view(domain))

    def update(self, xg=None):
        """Close both windows (dg_ada_update).  ``xg`` (dp.ExchangeGroup): the windows are summed over the ranks first, so every rank
        computes the same p from all ranks' outputs."""
        if xg is not None:
            xg.all_reduce_sum_(self.acc)
        for d in (0, 1):
            ops.ada_update(self.ctl[d], self.acc_view(d), self.target, self.step_per_image, self.p_max)

    def step(self, xg=None):
        """Behind the ``accumulate`` calls of one discriminator step; returns whether the windows were closed."""
        self.dsteps += 1
        if self.dsteps % self.interval:
            return False
        self.update(xg)
        return True

    def stats(self):
        """Both control blocks as host numbers (waits for the device): dict(p=, rt=, updates=, images=, adjust=) of pairs (A, B)."""
        c = self.ctl.cpu()
        return dict(p=(float(c[0, 0]), float(c[1, 0])), rt=(float(c[0, 1]), float(c[1, 1])), updates=(int(c[0, 2]), int(c[1, 2])),
                    images=(int(c[0, 3]), int(c[1, 3])), adjust=(float(c[0, 4]), float(c[1, 4])))

    def state_dict(self):
        return dict(ctl=self.ctl.cpu(), acc=self.acc.cpu(), dsteps=int(self.dsteps))

    def load_state_dict(self, st):
        ctl, acc = torch.as_tensor(st["ctl"]), torch.as_tensor(st["acc"])
        if tuple(ctl.shape) != (2, 8) or ctl.dtype != torch.float64 or tuple(acc.shape) != (4,) or acc.dtype != torch.float32:
            raise ValueError("AdaController: a state of ctl float64 [2, 8] and acc float32 [4] expected")
        self.ctl.copy_(ctl)
        self.acc.copy_(acc)
        self.dsteps = int(st["dsteps"])


def format_ada_suffix(stats):
    """The log suffix of the controller from ``AdaController.stats()``."""
    return f" ADA: p {stats['p'][0]:.4f}/{stats['p'][1]:.4f} rt {stats['rt'][0]:.3f}/{stats['rt'][1]:.3f}"


def apply_group(augs, xs):
    """``augs[i].apply(xs[i])`` for up to ops.MAX_GROUPS batches of one shape in one launch per pass (functional.DiffAugGroupFn)."""
    from . import functional as F_
    flags = augs[0].flags
    for a, x in zip(augs, xs):
        a.check(x)
        if a.flags != flags:
            raise ValueError("apply_group: the transforms of one grouped launch share one policy")
    return F_.DiffAugGroupFn.apply(len(xs), flags, *[a.recs for a in augs], *xs)
