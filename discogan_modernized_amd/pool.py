"""Image history pool of one domain's generated images (Shrivastava et al. 2017; CycleGAN's ``ImagePool``) on the device.

A discriminator that is trained on ``pool.exchange(fakes)`` instead of the newest fakes sees a mix of current and earlier ones: while
the pool fills, every fake is stored and passed on; afterwards each sample is, with probability 1/2, exchanged for a uniformly drawn
stored image (which it replaces), in batch order -- include/discogan_hip.h ("image history pool") has the exact semantics.

Two steps per batch, so that the second can sit inside a captured hipGraph:

  ``draw(iteration, n)``   eager, outside any capture: dg_pool_draw resolves the batch's in-order semantics into the pool's persistent
                           record table -- a pure function of (seed, rank, iteration, domain, position) and of ``filled``, no generator
                           state, no host round trip -- and advances ``filled``;
  ``exchange(x) -> out``   one launch (dg_pool_exchange) that reads only device memory at fixed addresses: the record table, the slots and
                           ``x``.  Under graph replay the same node applies whatever table the draw in front of the replay left there.

The record table is allocated once for the largest batch the kernels take (ops.POOL_MAX_BATCH rows of 16 bytes = 64 KiB), so its address
never changes under a captured graph however the batch size varies.
"""
from __future__ import annotations

import torch

from . import ops


class ImagePool:
    def __init__(self, size, image_size, seed, rank, domain, device="cuda"):
        if isinstance(size, bool) or not isinstance(size, int) or size < 1:
            raise ValueError(f"ImagePool needs an integer number of slots >= 1, got {size!r}")
        if domain not in (0, 1):
            raise ValueError(f"ImagePool: domain 0 (A) or 1 (B), got {domain!r}")
        self.size, self.image_size = size, int(image_size)
        self.seed, self.rank, self.domain = int(seed), int(rank), int(domain)
        self.device = torch.device(device)
        # zeros, not empty: slots that were never written travel in state_dict()
        self.slots = torch.zeros((size, 3, self.image_size, self.image_size), device=self.device, dtype=torch.float32)
        self.recs = torch.zeros((ops.POOL_MAX_BATCH, 4), device=self.device, dtype=torch.int32)
        self.filled = 0
        self.drawn = 0                      # samples of the batch the table was last drawn for (0: none yet)

    def draw(self, iteration, n):
        """Draw the records of the batch of ``n`` images that iteration ``iteration`` exchanges, and advance ``filled``.  Eager: call it
        outside any graph capture, once per exchanged batch, before the ``exchange`` (or the replay of the graph that holds it)."""
        n = int(n)
        if not 1 <= n <= ops.POOL_MAX_BATCH:
            raise ValueError(f"ImagePool.draw: a batch of 1..{ops.POOL_MAX_BATCH} images, got {n}")
        ops.pool_draw(self.seed, self.rank, iteration, self.domain, n, self.size, self.filled, out=self.recs)
        self.filled = min(self.size, self.filled + n)
        self.drawn = n
        return self.recs[:n]

    def exchange(self, x):
        """``x`` [n,3,S,S] -> the batch the discriminator sees, by the records of the last ``draw``; the slots are updated in place.  The
        result is a new tensor without an autograd history (the pool is a data source, not a layer).  Safe to capture."""
        if x.dim() != 4 or tuple(x.shape[1:]) != tuple(self.slots.shape[1:]):
            raise ValueError(f"ImagePool.exchange: a batch [n,3,{self.image_size},{self.image_size}] expected, got {tuple(x.shape)}")
        if int(x.shape[0]) != self.drawn:
            raise RuntimeError(f"ImagePool.exchange: the record table was drawn for {self.drawn} images, the batch has {x.shape[0]} "
                               "(draw(iteration, n) comes first)")
        return ops.pool_exchange(x.detach().contiguous(), self.slots, self.recs)

    def state_dict(self):
        return dict(size=self.size, image_size=self.image_size, filled=self.filled, seed=self.seed, rank=self.rank, domain=self.domain,
                    slots=self.slots.detach().cpu().clone())

    def load_state_dict(self, st):
        """The slots and the fill count of a saved pool of the same geometry.  Seed, rank and domain stay this pool's own (they come from
        the run's configuration, like the augmentation's)."""
        slots = st["slots"]
        if int(st["size"]) != self.size or tuple(slots.shape) != tuple(self.slots.shape):
            raise ValueError(f"ImagePool.load_state_dict: saved pool {tuple(slots.shape)} does not fit this pool {tuple(self.slots.shape)}")
        filled = int(st["filled"])
        if not 0 <= filled <= self.size:
            raise ValueError(f"ImagePool.load_state_dict: filled = {filled} outside [0, {self.size}]")
        self.slots.copy_(slots.to(self.device, torch.float32))
        self.filled, self.drawn = filled, 0

    def clear(self):
        self.slots.zero_()
        self.filled, self.drawn = 0, 0
