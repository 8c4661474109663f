"""numpy float64 reference of gradient control (include/discogan_hip.h, "Gradient norm, clipping by it and the non-finite guard"):
the sum of squares of the stepped flat ranges, the norm of the pre-scaled gradient, the clip coefficient of
``torch.nn.utils.clip_grad_norm_`` (``error_if_nonfinite=False``), the guard, the counters of the control block, and the log suffix."""
import math
import re

import numpy as np

EPS = 1e-6                       # torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6)


def sumsq(*ranges):
    """Sum of squares over flat fp32 ranges in float64 (every product exact; numpy sums pairwise)."""
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for g in ranges:
            g64 = np.asarray(g).astype(np.float64)
            total = total + np.sum(g64 * g64, dtype=np.float64)
    return float(total)


def norm(ss, pre_scale=1.0):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(ss)) * np.float64(pre_scale))


def scale(nrm, max_norm, pre_scale=1.0):
    """pre_scale * min(1, max_norm / (norm + 1e-6)); max_norm <= 0: pre_scale.  A NaN norm gives NaN, an infinite one 0."""
    if not max_norm > 0.0:
        return float(pre_scale)
    with np.errstate(all="ignore"):
        coef = np.float64(max_norm) / (np.float64(nrm) + np.float64(EPS))
        if coef >= 1.0:
            return float(pre_scale)
        return float(np.float64(pre_scale) * coef)


def is_clipped(nrm, max_norm):
    return bool(max_norm > 0.0 and np.float64(max_norm) / (np.float64(nrm) + np.float64(EPS)) < 1.0)


def skip(ss, guard):
    return bool(guard) and not math.isfinite(ss)


class Control:
    """Host model of the control block ctl[8] over a sequence of steps."""

    def __init__(self, max_norm=0.0, guard=False):
        self.max_norm, self.guard = float(max_norm), bool(guard)
        self.ctl = [0.0] * 8

    def step(self, ranges, pre_scale=1.0):
        ss = sumsq(*ranges)
        n = norm(ss, pre_scale)
        sk = skip(ss, self.guard)
        c = self.ctl
        c[0], c[1], c[2], c[3] = ss, n, scale(n, self.max_norm, pre_scale), float(sk)
        c[4] += 1.0
        if is_clipped(n, self.max_norm) and not sk:
            c[5] += 1.0
        if sk:
            c[6] += 1.0
        if math.isfinite(n) and n > c[7]:
            c[7] = n
        return list(c)


# ---- the log suffix: " GRAD: D {norm:.4e} G {norm:.4e} clipped {c}/{n} skipped {s}" -----------------------------------------------
_NUM = r"([-+]?(?:\d\.\d{4}e[-+]\d{2,3}|nan|inf))"
_SUFFIX = re.compile(r" GRAD: D " + _NUM + " G " + _NUM + r" clipped (\d+)/(\d+) skipped (\d+)$")


def format_suffix(norm_d, norm_g, clipped, steps, skipped):
    return f" GRAD: D {norm_d:.4e} G {norm_g:.4e} clipped {int(clipped)}/{int(steps)} skipped {int(skipped)}"


def parse(line):
    """dict(norm_d, norm_g, clipped, steps, skipped, head) of a log line that ends in the suffix; None when it has none."""
    m = _SUFFIX.search(line)
    if m is None:
        return None
    return dict(norm_d=float(m.group(1)), norm_g=float(m.group(2)), clipped=int(m.group(3)), steps=int(m.group(4)),
                skipped=int(m.group(5)), head=line[:m.start()])
