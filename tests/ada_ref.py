"""numpy restatement of the adaptive discriminator augmentation (include/discogan_hip.h, "adaptive discriminator augmentation") -- TEST
INFRASTRUCTURE ONLY.  Built on tests/diffaug_ref.py, which stays as it is.

  * ``gates`` / ``draw_p``: the table of dg_diffaug_draw_p.  One more link of diffaug_ref.key, all arithmetic modulo 2^64:
        k2 = mix(k ^ 0x6164610000000000);  g_1 = mix(k2 + G (2j + 1));  g_2 = mix(k2 + G (2j + 2))
        u_color = unit(hi g_1);  u_translation = unit(lo g_1);  u_cutout = unit(hi g_2);    a stage is kept iff u < float32(p)
    A stage of the policy that is not kept holds its neutral fields: colour (0.0f, 1.0f, 1.0f), translation (0, 0), cutout (S, S).
  * ``accumulate``: a window (sum of signs, count) as float32, the sign from two comparisons.
  * ``update``: the controller in float64, one operation per line in the order of the header.
"""
import numpy as np

from tests import diffaug_ref as DR
from tests.augment_ref import _G, _M, mix

GATE_LINK = 0x6164610000000000
THRESHOLDS = dict(bce=0.5, bce_logits=0.0, hinge=0.0)          # lsgan: real label / 2


def gates(seed, rank, iteration, domain, role, n):
    """float32 [n, 3]: the uniforms of (colour, translation, cutout) per batch position."""
    k2 = mix(DR.key(seed, rank, iteration, domain, role) ^ GATE_LINK)
    out = np.zeros((n, 3), dtype=np.float32)
    for j in range(n):
        g1, g2 = mix((k2 + _G * (2 * j + 1)) & _M), mix((k2 + _G * (2 * j + 2)) & _M)
        out[j] = (DR._unit(g1 >> 32), DR._unit(g1 & 0xFFFFFFFF), DR._unit(g2 >> 32))
    return out


def keep_mask(seed, rank, iteration, domain, role, n, p):
    """bool [n, 3]: which of (colour, translation, cutout) a sample keeps at probability p (one rounding to float32)."""
    return gates(seed, rank, iteration, domain, role, n) < np.float32(p)


def gate(recs, keep, S, flags):
    """The ungated table ``recs`` with the stages of ``flags`` that ``keep`` [n, 3] drops set to their neutral fields."""
    out = recs.copy()
    neutral = DR.make_record()
    if flags & DR.COLOR:
        out[~keep[:, 0], 4:7] = neutral[4:7]
    if flags & DR.TRANSLATION:
        out[~keep[:, 1], 0:2] = 0
    if flags & DR.CUTOUT:
        out[~keep[:, 2], 2:4] = S
    return out


def draw_p(seed, rank, iteration, domain, role, n, S, flags, p):
    """int32 [n, 8]: the table of dg_diffaug_draw_p."""
    return gate(DR.draw(seed, rank, iteration, domain, role, n, S, flags), keep_mask(seed, rank, iteration, domain, role, n, p), S, flags)


def new_ctl(p0=0.0):
    """float64 [8]: p, r_t (NaN before the first update), updates, images, last adjustment, 0, 0, 0."""
    ctl = np.zeros(8, dtype=np.float64)
    ctl[0], ctl[1] = p0, np.nan
    return ctl


def new_acc():
    return np.zeros(2, dtype=np.float32)


def accumulate(acc, d_out, threshold):
    """acc (float32 [2]) += (sum of signs against the threshold, count) of d_out; in place."""
    v, thr = np.asarray(d_out, dtype=np.float32).reshape(-1), np.float32(threshold)
    s = int(np.count_nonzero(v > thr)) - int(np.count_nonzero(v < thr))          # a NaN and v == thr: neither
    acc[0] = np.float32(acc[0] + np.float32(s))
    acc[1] = np.float32(acc[1] + np.float32(v.size))
    return acc


def update(ctl, acc, target, step_per_image, p_max=1.0):
    """Close the window into the control block, both in place; every line is one float64 operation."""
    if acc[1] == 0:
        return ctl
    target, step, p_max = np.float64(target), np.float64(step_per_image), np.float64(p_max)
    rt = np.float64(acc[0]) / np.float64(acc[1])
    adj = np.float64(acc[1]) * step
    applied = adj if rt > target else (-adj if rt < target else np.float64(0.0))
    p = ctl[0] + applied
    if not p >= 0.0:
        p = np.float64(0.0)
    if p > p_max:
        p = p_max
    ctl[0] = p
    ctl[1] = rt
    ctl[2] = ctl[2] + 1.0
    ctl[3] = ctl[3] + np.float64(acc[1])
    ctl[4] = applied
    acc[0] = acc[1] = 0
    return ctl


def step_per_image(kimg):
    return 1.0 / (1000.0 * kimg)
