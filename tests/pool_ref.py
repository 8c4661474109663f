"""numpy restatement of the image history pool (include/discogan_hip.h, "image history pool") -- TEST INFRASTRUCTURE ONLY.

Three independent pieces:
  * ``draws`` / ``records``: the draw and the record rule of dg_pool_draw.  Key chain of the augmentation draw (tests/augment_ref.py) with one
    more link, all arithmetic modulo 2^64:
        k = mix(seed + G);  k = mix(k ^ (uint32(rank) << 32 | uint32(domain)));  k = mix(k ^ iteration);  k = mix(k ^ 0x706F6F6C)
        a = mix(k + G (j + 1));  swap = a >> 63;  s = ((a & 0xFFFFFFFF) P) >> 32
    record of sample j (touch = insert or swap; prev = last earlier toucher of j's slot, last = last toucher of it from j on):
        pass (j, -1, j, 0);  insert (j, s, last, 0);  swap, prev < 0: (-1, s, last, 0);  swap, prev >= 0: (prev, -1, j, 0)
  * ``apply_records``: what dg_pool_exchange does with a table -- every ``out`` from the pool as it was BEFORE, then the stores; records
    with a field out of range count as the pass record.
  * ``SequentialPool``: CycleGAN's ImagePool.query, sample by sample, with no records at all (it only shares ``draws``).
"""
import numpy as np

from tests.augment_ref import _G, _M, mix

LINK = 0x706F6F6C


def key(seed, rank, iteration, domain):
    k = mix((seed & _M) + _G)
    k = mix(k ^ (((rank & 0xFFFFFFFF) << 32) | (domain & 0xFFFFFFFF)))
    k = mix(k ^ (iteration & _M))
    return mix(k ^ LINK)


def draws(seed, rank, iteration, domain, n, P):
    """[(swap bit, slot)] of the n batch positions (meaningful for the samples that do not insert)."""
    k = key(seed, rank, iteration, domain)
    out = []
    for j in range(n):
        a = mix(k + _G * (j + 1))
        out.append((a >> 63, ((a & 0xFFFFFFFF) * P) >> 32))
    return out


def touches(seed, rank, iteration, domain, n, P, filled):
    """Per sample: ('insert' | 'swap' | 'pass', slot or -1)."""
    d = draws(seed, rank, iteration, domain, n, P)
    out = []
    for j in range(n):
        if filled + j < P:
            out.append(("insert", filled + j))
        elif d[j][0]:
            out.append(("swap", d[j][1]))
        else:
            out.append(("pass", -1))
    return out


def records(seed, rank, iteration, domain, n, P, filled):
    """int32 [n, 4] = (src, slot, st_src, 0): the table dg_pool_draw writes."""
    t = touches(seed, rank, iteration, domain, n, P, filled)
    recs = np.zeros((n, 4), dtype=np.int32)
    for j, (kind, s) in enumerate(t):
        if kind == "pass":
            recs[j] = (j, -1, j, 0)
            continue
        same = [i for i in range(n) if t[i][1] == s]
        prev = max([i for i in same if i < j], default=-1)
        last = max(i for i in same if i >= j)
        if kind == "insert":
            assert prev < 0
            recs[j] = (j, s, last, 0)
        elif prev < 0:
            recs[j] = (-1, s, last, 0)
        else:
            recs[j] = (prev, -1, j, 0)
    return recs


def apply_records(x, pool, recs):
    """(out, pool after) of dg_pool_exchange; x [n, ...], pool [P, ...] of any dtype, recs [>= n, 4].  Inputs are not modified."""
    n, P = len(x), len(pool)
    out, after = np.empty_like(x), pool.copy()
    for j in range(n):
        src, slot, st = (int(v) for v in recs[j, :3])
        if not (-1 <= src < n and -1 <= slot < P and 0 <= st < n) or (src == -1 and slot == -1):
            src, slot, st = j, -1, j
        out[j] = pool[slot] if src == -1 else x[src]
        if slot >= 0:
            after[slot] = x[st]
    return out, after


class SequentialPool:
    """ImagePool.query of CycleGAN, one sample after the other, on the shared draw."""

    def __init__(self, P, shape, dtype, seed, rank, domain):
        self.P, self.filled = P, 0
        self.seed, self.rank, self.domain = seed, rank, domain
        self.slots = np.zeros((P,) + tuple(shape), dtype=dtype)

    def query(self, x, iteration):
        n = len(x)
        d = draws(self.seed, self.rank, iteration, self.domain, n, self.P)
        out = np.empty_like(x)
        filled = self.filled
        for j in range(n):
            if filled + j < self.P:
                self.slots[filled + j] = x[j]
                out[j] = x[j]
            elif d[j][0]:
                s = d[j][1]
                out[j] = self.slots[s]
                self.slots[s] = x[j]
            else:
                out[j] = x[j]
        self.filled = min(self.P, filled + n)
        return out
