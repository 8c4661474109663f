"""CPU references of the reconstruction criterion (checker of tests/test_recon_cpu.py and tests/test_recon_gpu.py).

``loss_ref`` restates the definition of include/discogan_hip.h ("reconstruction loss") with ``torch.nn.functional.conv2d``,
differentiably, in float64 (THE reference) or float32 (the yardstick "a plain fp32 evaluation of the same formula": the window rounded
to fp32 once, every operation and autograd's backward in fp32).  ``grad_analytic`` evaluates the gather form of the SSIM gradient the
header states -- coefficient maps a, b, c over the window corners and the adjoint separable pass -- as a second, independent
evaluation.  The keyword arguments of ``loss_ref`` build deliberately WRONG problems for the discrimination tests.  Data:
``tests.metrics_ref.make_pair``."""
import torch
import torch.nn.functional as TF

from tests import metrics_ref as MR

K = 11
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _window(dtype, C, sigma=1.5):
    g = MR.gaussian(K, sigma)
    if dtype == torch.float32:
        g = g.float()                                             # rounded once; the 2-D weight is the fp32 product
    return (g[:, None] * g[None, :]).to(dtype).expand(C, 1, K, K).contiguous()


def ssim_mean(x, t, sigma=1.5, pad=False, norm_s2=False):
    """Mean SSIM over all n C (S - 10)^2 valid windows, differentiable, in x's dtype.  pad: zero-padded "same" windows (S^2 of them);
    norm_s2: the valid windows' sum divided by n C S^2 -- wrong problems both."""
    n, C, S, _ = x.shape
    w = _window(x.dtype, C, sigma)
    f = lambda v: TF.conv2d(v, w, padding=K // 2 if pad else 0, groups=C)   # noqa: E731
    mx, my = f(x), f(t)
    sx, sy, sxy = f(x * x) - mx * mx, f(t * t) - my * my, f(x * t) - mx * my
    m = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2))
    return m.sum() / (n * C * S * S) if norm_s2 else m.mean()


def parts_ref(x, t, dtype=torch.float64, **wrong):
    """(mse, l1, 1 - mean SSIM) as 0-d tensors of ``dtype``; x may require grad (it must then have ``dtype`` already)."""
    x = x if x.dtype == dtype else x.detach().cpu().to(dtype)
    t = t.detach().cpu().to(dtype)
    d = x - t
    ssim = 1.0 - ssim_mean(x, t, **wrong) if x.shape[-1] >= K else torch.zeros((), dtype=dtype)
    return (d * d).mean(), d.abs().mean(), ssim


def loss_ref(x, t, w, dtype=torch.float64, **wrong):
    """w_mse mse + w_l1 l1 + w_ssim (1 - mean SSIM); a term of weight 0 is left out."""
    parts = parts_ref(x, t, dtype, **wrong)
    return sum(float(wi) * p for wi, p in zip(w, parts) if wi > 0)


def grad_ref(x, t, w, gout=1.0, dtype=torch.float64, **wrong):
    """gout * d loss / d x by autograd of ``loss_ref`` in ``dtype`` (returned in ``dtype``)."""
    xr = x.detach().cpu().to(dtype).requires_grad_(True)
    (loss_ref(xr, t, w, dtype, **wrong) * gout).backward()
    return xr.grad.detach()


def grad_analytic(x, t, w, gout=1.0):
    """The same gradient from the formulas of the header, float64: no autograd."""
    x, t = x.detach().cpu().double(), t.detach().cpu().double()
    n, C, S, _ = x.shape
    N = x.numel()
    d = x - t
    out = torch.zeros_like(x)
    if w[0] > 0:
        out += w[0] * 2.0 * d / N
    if w[1] > 0:
        out += w[1] * torch.sign(d) / N
    if w[2] > 0:
        win = _window(torch.float64, C)
        f = lambda v: TF.conv2d(v, win, groups=C)                           # noqa: E731
        adj = lambda v: TF.conv_transpose2d(v, win, groups=C)               # noqa: E731  the "full" pass: every window that holds q
        mx, my = f(x), f(t)
        sx, sy, sxy = f(x * x) - mx * mx, f(t * t) - my * my, f(x * t) - mx * my
        A1, A2, B1, B2 = 2 * mx * my + C1, 2 * sxy + C2, mx * mx + my * my + C1, sx + sy + C2
        dmu = 2 * my * A2 / (B1 * B2) - 2 * mx * A1 * A2 / (B1 * B1 * B2)
        dsig = -A1 * A2 / (B1 * B2 * B2)
        dc = 2 * A1 / (B1 * B2)
        a, b, c = dmu - 2 * mx * dsig - my * dc, 2 * dsig, dc
        g = (adj(a) + x * adj(b) + t * adj(c)) / (n * C * (S - K + 1) ** 2)
        out -= w[2] * g
    return gout * out


def grad_bound(x, t, w, gout, r64=None):
    """The gradient criterion: SSIM_M x (distance of the plain fp32 autograd from float64) + 2^-20 max |ref|.  Returns (bound, ref64,
    e32)."""
    r64 = grad_ref(x, t, w, gout) if r64 is None else r64
    e32 = float((grad_ref(x, t, w, gout, torch.float32).double() - r64).abs().max())
    return MR.SSIM_M * e32 + 2.0 ** -20 * float(r64.abs().max()), r64, e32


# ---- shapes past the grid caps (tests/test_recon_cpu.py states the arithmetic, tests/test_recon_gpu.py runs them) ----------------------
RC_MAX_BLOCKS = 8192        # csrc/recon.hip: both tile kernels launch at most this many blocks per problem and stride over the items
RC_STREAM_BLOCKS = 1024     # csrc/recon.hip: the forward stream kernel's cap; the backward's is twice that
TILE = 32                   # RT
FINAL_THREADS = 256         # recon_final_kernel: thread t sums the partials t, t + 256, ...
TILE_PAST_CAP = ((5470, 11), (690, 43), (690, 44))      # three trips at one tile per plane; four tiles per plane, scalar and 16-byte loads
FINAL_PAST_256 = ((30, 43, "triple"), (2, 256, "l1"))   # the final kernel's second trip alone: 360 tile partials, 384 stream partials
STREAM_PAST_CAP = ((11, 256), (125, 75))                # 16-byte loads; scalar loads with a three-element tail


def tile_items(n, S):
    """(items, P): work items of the tile kernels (dg_recon_loss_fwd_g: items = n P, P = 3 T^2, T = ceil(S / 32))."""
    T = (S + TILE - 1) // TILE
    return n * 3 * T * T, 3 * T * T


def stream_blocks(n, S):
    """(blocks wanted, quads, tail elements) of the stream kernels: g = (count / 4 + 255) / 256 before the cap."""
    count = n * 3 * S * S
    return max(1, (count // 4 + 255) // 256), count // 4, count % 4


def planted_images(n, S):
    """Image 0, the images that hold the items either side of every multiple of the grid cap (and the image after), the last image."""
    items, P = tile_items(n, S)
    at = {0, n - 1}
    for k in range(1, (items - 1) // RC_MAX_BLOCKS + 1):
        at |= {(k * RC_MAX_BLOCKS - 1) // P, (k * RC_MAX_BLOCKS) // P, (k * RC_MAX_BLOCKS) // P + 1}
    return sorted(i for i in at if i < n)


def planted_pair(n, S, seed):
    """x = t everywhere but in the planted images, where x and t are independent: there one item's share of the loss is far above the
    forward bound, so a dropped or misdecoded item at a trip boundary cannot hide (test_recon_cpu states the margin)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, 3, S, S, generator=g)
    x = t.clone()
    at = planted_images(n, S)
    px, pt = MR.make_pair("indep", len(at), S, seed + 1)
    x[at], t[at] = px, pt
    return x, t, at


def fwd_bound(x, t, w):
    """The forward criterion: each part within its own bound -- MSE and L1 gamma(K_CHAIN) of their values, the SSIM part
    ``metrics_ref.ssim_bound`` -- weighted, plus one rounding of the sum to fp32.  Returns (bound, loss64)."""
    parts = parts_ref(x, t)
    mse, l1, _ = (float(v) for v in parts)
    loss = float(sum(float(wi) * p for wi, p in zip(w, parts) if wi > 0))       # loss_ref's sum, the parts evaluated once
    fb = w[0] * MR.gamma(MR.K_CHAIN) * mse + w[1] * MR.gamma(MR.K_CHAIN) * l1 + MR.U32 * abs(loss)
    if w[2] > 0:
        fb += w[2] * MR.ssim_bound(x, t)[0]
    return fb, loss
