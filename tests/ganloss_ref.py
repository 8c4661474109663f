"""Float64 reference of the adversarial objectives on logits (csrc/ganloss.hip, include/discogan_hip.h: dg_gan_loss_*).  Pure numpy,
imported by nothing in the package.

Per problem  loss = mean_i f(x_i),  dlogit_i = gout f'(x_i) / n,  with the target tau by role (D_REAL: real_label, D_FAKE: 0,
G_FAKE: 1):
    bce_logits  f = tau sp(-x) + (1 - tau) sp(x)   f' = sigmoid(x) - tau     sp(x) = max(x, 0) + log1p(exp(-|x|))
    lsgan       f = (x - tau)^2                    f' = 2 (x - tau)
    hinge       D_REAL max(0, 1 - x) | D_FAKE max(0, 1 + x) | G_FAKE -x      f' = -[x < 1] | +[x > -1] | -1   (0 at the kink: relu'(0))
The derivative of the cross entropy is evaluated without cancellation where the target is hard (tau = 1: -sigmoid(-x), tau = 0:
sigmoid(x), both from exp(-|x|)), so the reference itself is accurate to float64 rounding at x = +-60.

Tolerances: the project's own for the BCE kernels (tests/test_ops_gpu.py::test_bce_including_saturation,
tests/test_reductions_gpu.py::bce_check) -- loss rtol 1e-6 + atol 1e-7, gradient 1e-5 |g_ref| elementwise, purely relative for every
hard target; smoothed BCE alone, where sigmoid(x) - 0.9 cancels near x = 2.2, adds 4 * 2^-24 |gout| / n (the rounding of its two O(1)
operands)."""
import numpy as np

KINDS = ("bce_logits", "lsgan", "hinge")
KIND_CODES = {"bce_logits": 0, "lsgan": 1, "hinge": 2}                 # DG_GAN_BCE_LOGITS / LSGAN / HINGE
ROLES = ("d_real", "d_fake", "g_fake")
ROLE_CODES = {"d_real": 0, "d_fake": 1, "g_fake": 2}                   # DG_GAN_D_REAL / D_FAKE / G_FAKE
SHAPES = (1, 3, 64, 255, 256, 257, 1000)
LOSS_RTOL, LOSS_ATOL, GRAD_RTOL = 1e-6, 1e-7, 1e-5
U24 = 2.0 ** -24


def f32(v):
    """The value the library receives for a host float argument."""
    return float(np.float32(v))


def target(role, real_label=1.0):
    """tau of a role; ``real_label`` as the fp32 value the kernel is handed."""
    return {"d_real": f32(real_label), "d_fake": 0.0, "g_fake": 1.0}[role]


def labels_of(kind):
    """The real labels a kind is tested with: the hinge has no target to smooth."""
    return (1.0,) if kind == "hinge" else (1.0, 0.9)


def cases():
    """Every (kind, role, real_label) that is a problem of its own (the label matters to D_REAL only)."""
    return [(k, r, lab) for k in KINDS for r in ROLES for lab in labels_of(k) if lab == 1.0 or r == "d_real"]


def softplus(x):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    """sigmoid(x) from exp(-|x|): relatively accurate on both tails."""
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def term(kind, role, x, real_label=1.0):
    """f(x_i), float64, elementwise."""
    x = np.asarray(x, np.float64)
    tau = target(role, real_label)
    if kind == "bce_logits":
        return tau * softplus(-x) + (1.0 - tau) * softplus(x)
    if kind == "lsgan":
        return (x - tau) ** 2
    if kind == "hinge":
        if real_label != 1.0:
            raise ValueError("the hinge takes real_label 1")
        return {"d_real": np.maximum(0.0, 1.0 - x), "d_fake": np.maximum(0.0, 1.0 + x), "g_fake": -x}[role]
    raise ValueError(kind)


def deriv(kind, role, x, real_label=1.0):
    """f'(x_i), float64, elementwise; 0 at a hinge kink."""
    x = np.asarray(x, np.float64)
    tau = target(role, real_label)
    if kind == "bce_logits":
        if tau == 1.0:
            return -sigmoid(-x)
        return sigmoid(x) if tau == 0.0 else sigmoid(x) - tau
    if kind == "lsgan":
        return 2.0 * (x - tau)
    if kind == "hinge":
        return {"d_real": -(x < 1.0).astype(np.float64), "d_fake": (x > -1.0).astype(np.float64), "g_fake": -np.ones_like(x)}[role]
    raise ValueError(kind)


def loss_ref(kind, role, x, real_label=1.0):
    return float(np.mean(term(kind, role, x, real_label)))


def grad_ref(kind, role, x, real_label=1.0, gout=1.0):
    x = np.asarray(x, np.float64)
    return float(gout) * deriv(kind, role, x, real_label) / x.size


def loss_bound(want):
    return LOSS_RTOL * abs(want) + LOSS_ATOL


def grad_bound(kind, role, g_ref, real_label, gout, n):
    """Elementwise bound of the gradient: relative, plus the cancellation allowance of the smoothed cross entropy alone."""
    b = GRAD_RTOL * np.abs(np.asarray(g_ref, np.float64))
    if kind == "bce_logits" and role == "d_real" and real_label != 1.0:
        b = b + 4.0 * U24 * abs(float(gout)) / n
    return b


def loss_ratio(got, want):
    return abs(float(got) - want) / loss_bound(want)


def grad_ratio(got, kind, role, g_ref, real_label, gout):
    """max_i |got_i - ref_i| / bound_i (an element whose reference and bound are 0 must be 0 exactly: ratio 0 or inf)."""
    g_ref = np.asarray(g_ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - g_ref)
    b = grad_bound(kind, role, g_ref, real_label, gout, g_ref.size)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / b)
    return float(r.max())


def logits(n, seed):
    """fp32 test logits: normal draws at scales 1, 8 and 60 in turn, clipped to +-60, with 60, -60, 1, -1 planted where they fit."""
    rng = np.random.default_rng(seed)
    scale = np.array([1.0, 8.0, 60.0])[np.arange(n) % 3]
    x = np.clip(rng.standard_normal(n) * scale, -60.0, 60.0).astype(np.float32)
    plant = np.array([60.0, -60.0, 1.0, -1.0], np.float32)
    at = rng.permutation(n)[:min(n, 4)]
    x[at] = plant[:at.size]
    return x


def mild_logits(n, seed):
    """fp32 logits for the comparison with the BCE kernel on sigmoid(x): uniform in [-3, 3].  That comparison is limited by the rounding
    of p = sigmoid(x) to fp32, which no kernel behind it can undo: log(1 - p) moves by 2^-25 (1 + e^x).  Against the loss tolerance
    (1e-6 relative) this alone is 17 to 45 times the bound for logits spread over [-10, 10], 0.35 of it on [-4, 4] and 0.19 on [-3, 3]
    (float64 evaluation on correctly rounded p, 50 seeds per shape) -- [-3, 3] leaves the rest of the bound to the three kernels."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-3.0, 3.0, n).astype(np.float32)
