"""CPU references of the held-out image metrics (checker of tests/test_metrics_*.py and tests/test_evaluate_gpu.py).

``ssim_ref(dtype=float64)`` is THE reference: SSIM of Wang et al. 2004 as include/discogan_hip.h states it (11 x 11 Gaussian window of
sigma 1.5 normalised in double, valid windows, C1 = 0.01^2, C2 = 0.03^2, data range 1, mean over channels and windows), evaluated with
``torch.nn.functional.conv2d``.  ``dtype=float32`` is the project's usual yardstick "a plain fp32 evaluation of the same formula" (the
window rounded to fp32 once, every operation in fp32): its distance from the float64 form is the error a sound fp32 kernel may have.
The keyword arguments build deliberately WRONG problems for the discrimination tests."""
import torch
import torch.nn.functional as TF

U32 = 2.0 ** -24


def gaussian(k=11, sigma=1.5):
    """g[i] = exp(-(i - k//2)^2 / (2 sigma^2)) / sum, float64."""
    d = torch.arange(k, dtype=torch.float64) - (k // 2)
    g = torch.exp(-(d * d) / (2.0 * sigma * sigma))
    return g / g.sum()


def ssim_ref(x, y, dtype=torch.float64, sigma=1.5, k=11, K1=.01, K2=.03, pad=False):
    """Per-image SSIM [n] (in ``dtype``) of two [n,C,S,S] batches.  pad=True: zero-padded "same" windows (a wrong problem)."""
    x, y = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    n, C = x.shape[:2]
    g = gaussian(k, sigma)
    if dtype == torch.float32:
        g = g.float()                                             # rounded once; the 2-D weight is the fp32 product
    w = (g[:, None] * g[None, :]).to(dtype).expand(C, 1, k, k).contiguous()
    p = k // 2 if pad else 0
    f = lambda t: TF.conv2d(t, w, padding=p, groups=C)
    mx, my = f(x), f(y)
    sx, sy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    C1, C2 = torch.tensor(K1 ** 2, dtype=dtype), torch.tensor(K2 ** 2, dtype=dtype)
    m = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2))
    return m.reshape(n, -1).mean(1)


def ssim_brute(x, y, k=11, sigma=1.5, K1=.01, K2=.03):
    """The same quantity by a double loop over windows (float64), for one small batch: what ssim_ref is checked against."""
    x, y = x.detach().cpu().double(), y.detach().cpu().double()
    n, C, S, _ = x.shape
    g = gaussian(k, sigma)
    w = g[:, None] * g[None, :]
    out = torch.zeros(n, dtype=torch.float64)
    for i in range(n):
        tot = 0.0
        for c in range(C):
            for r in range(S - k + 1):
                for q in range(S - k + 1):
                    a, b = x[i, c, r:r + k, q:q + k], y[i, c, r:r + k, q:q + k]
                    mx, my = (w * a).sum(), (w * b).sum()
                    sx, sy, sxy = (w * a * a).sum() - mx * mx, (w * b * b).sum() - my * my, (w * a * b).sum() - mx * my
                    tot += ((2 * mx * my + K1 ** 2) * (2 * sxy + K2 ** 2)) / ((mx * mx + my * my + K1 ** 2) * (sx + sy + K2 ** 2))
        out[i] = tot / (C * (S - k + 1) ** 2)
    return out


def mse_mae_ref(x, y, crop=0):
    """(mse [n], mae [n]) in float64.  crop=1: taken over (S-1)^2 pixels per channel (a wrong problem)."""
    x, y = x.detach().cpu().double(), y.detach().cpu().double()
    if crop:
        x, y = x[..., :-crop, :-crop], y[..., :-crop, :-crop]
    d = (x - y).reshape(x.shape[0], -1)
    return (d * d).mean(1), d.abs().mean(1)


def psnr_ref(mse):
    return torch.where(mse == 0, torch.full_like(mse, float("inf")), 10.0 * torch.log10(1.0 / mse))


def gamma(k):
    return k * U32 / (1.0 - k * U32)


# the kernel's fp32 chain before its fp64 hand-over (csrc/metrics.hip header): 4 terms per thread summed pairwise, + 2 for the
# subtraction and the square
K_CHAIN = 4 + 2
SSIM_M = 8                  # bound = SSIM_M * e32 + SSIM_FLOOR
SSIM_FLOOR = 2.0 ** -20     # a few ulp of a value <= 1: the final mean's rounding and the division


def ssim_bound(x, y):
    """SSIM_M x (largest distance over the batch between the plain fp32 evaluation and the float64 reference) + the floor.
    Returns (bound, ref64 [n])."""
    r64 = ssim_ref(x, y, torch.float64)
    e32 = float((ssim_ref(x, y, torch.float32).double() - r64).abs().max())
    return SSIM_M * e32 + SSIM_FLOOR, r64


def make_pair(kind, n, S, seed):
    """The data kinds of the kernel tests, (x, y) float32 [n,3,S,S] on the CPU."""
    g = torch.Generator().manual_seed(seed)
    if kind == "indep":
        return torch.rand(n, 3, S, S, generator=g), torch.rand(n, 3, S, S, generator=g)
    if kind == "noisy":
        x = torch.rand(n, 3, S, S, generator=g)
        return x, (x + 0.05 * torch.randn(n, 3, S, S, generator=g)).clamp(0, 1)
    if kind == "smooth":
        up = lambda: TF.interpolate(torch.rand(n, 3, 4, 4, generator=g), size=(S, S), mode="bilinear", align_corners=False)
        return up().contiguous(), up().contiguous()
    if kind == "flat":
        return 0.5 + 1e-3 * torch.randn(n, 3, S, S, generator=g), 0.5 + 1e-3 * torch.randn(n, 3, S, S, generator=g)
    raise ValueError(kind)


KINDS = ("indep", "noisy", "smooth", "flat")
