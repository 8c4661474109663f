"""CPU references of multi-scale SSIM (checker of tests/test_msssim_cpu.py and tests/test_msssim_gpu.py).

``values`` / ``ms_channels`` / ``per_image`` / ``loss_ref`` restate the definition of include/discogan_hip.h ("multi-scale SSIM") with
slicing (the 2 x 2 average pyramid) and ``torch.nn.functional.conv2d`` (the windows), differentiably, in float64 (THE reference) or in
float32 (the yardstick "a plain fp32 evaluation of the same formula": window and exponents rounded to fp32 once, the pyramid's
0.25 ((a + b) + (c + d)) in that order, every operation and autograd's backward in fp32).  ``grad_analytic`` evaluates the header's
gradient formulas -- the table k_j = beta_j ms / V_j, per scale the gather form with the derivatives of A2 / B2 (of the whole quotient at
the last scale), and g_j(q >> j) / 4^j -- as a second, independent evaluation.  The keyword arguments build deliberately WRONG problems
for the discrimination tests.  Data: ``tests.metrics_ref.make_pair``."""
import numpy as np
import torch
import torch.nn.functional as TF

from tests import metrics_ref as MR
from tests import recon_ref as RR

K = RR.K
C1, C2 = RR.C1, RR.C2
EXPONENTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_SCALES = len(EXPONENTS)
V_MIN = 5e-4                          # the data condition of the GPU bounds: every float64 |V_j(i, c)| of a GPU case is at least this

# ---- the GPU cases (tests/test_msssim_cpu.py asserts the data condition on exactly these) ------------------------------------------------
SHAPES = ((1, 22, 2), (2, 23, 2), (1, 44, 3), (2, 45, 3), (2, 64, 3), (1, 88, 4), (1, 176, 5))
BELOW_MAX = (2, 64, 2)

# ---- shapes past the grid caps (csrc/msssim.hip) ------------------------------------------------------------------------------------------
MS_MAX_BLOCKS = 8192                  # every tile kernel launches at most this many blocks per problem and strides over its items
FINAL_THREADS = 256                   # ms_final_kernel: thread t takes the (image, channel) pairs t, t + 256, ...
TILE = 32
TILE_PAST_CAP = (2800, 24, 2)         # 8400 items per scale: pyramid 16800, forward 16800, coarse backward 8400, level-0 backward 8400
FINAL_PAST_256 = (90, 23, 2)          # 270 pairs: the final kernel's second trip alone (540 forward items)


KINDS = MR.KINDS + ("dimmed",)


def make_pair(kind, n, S, seed):
    """``metrics_ref.make_pair`` plus "dimmed": the noisy pair with t -> 0.6 t + 0.1, a brightness and contrast change.  On the other
    kinds x and t have equal local means, where the luminance factor A1 / B1 is 1 to a few 1e-4 and "the full SSIM at the last scale"
    cannot be told from "cs at the last scale"; here it is about 0.97, every channel is alive and every V_j >= 0.84."""
    if kind == "dimmed":
        x, t = MR.make_pair("noisy", n, S, seed)
        return x, 0.6 * t + 0.1
    return MR.make_pair(kind, n, S, seed)


def max_scales(S):
    """min(5, number of j with S >> j >= 11); 0: refused."""
    m = 0
    while m < MAX_SCALES and (S >> m) >= K:
        m += 1
    return m


def exponents(M, normalise=True):
    """The first M exponents over their sum: the division in double, rounded once to fp32 (returned as Python floats).
    normalise=False: the raw table (a wrong problem for M < 5)."""
    e = EXPONENTS[:M]
    s = 0.0
    for v in e:
        s += v
    return [float(np.float32(v / s)) if normalise else float(np.float32(v)) for v in e]


def down(v, pool="avg"):
    """Level j -> level j + 1: 0.25 ((a + b) + (c + d)) of the 2 x 2 blocks, a last odd row / column dropped.  pool="max": a wrong problem."""
    h = v.shape[-1] // 2
    a, b = v[..., 0:2 * h:2, 0:2 * h:2], v[..., 0:2 * h:2, 1:2 * h:2]
    c, d = v[..., 1:2 * h:2, 0:2 * h:2], v[..., 1:2 * h:2, 1:2 * h:2]
    if pool == "max":
        return torch.maximum(torch.maximum(a, b), torch.maximum(c, d))
    return 0.25 * ((a + b) + (c + d))


def _factors(x, t, pad=False):
    n, C, S, _ = x.shape
    w = RR._window(x.dtype, C)
    f = lambda v: TF.conv2d(v, w, padding=K // 2 if pad else 0, groups=C)   # noqa: E731
    mx, my = f(x), f(t)
    sx, sy, sxy = f(x * x) - mx * mx, f(t * t) - my * my, f(x * t) - mx * my
    return mx, my, 2 * mx * my + C1, 2 * sxy + C2, mx * mx + my * my + C1, sx + sy + C2


def values(x, t, M, pad=False, pool="avg", last_cs=False):
    """V [M][n][C] in x's dtype (a list of [n, C] tensors), differentiable.  pad: zero-padded "same" windows; pool: the pyramid's
    reduction; last_cs: the contrast-structure term at the last scale too -- wrong problems all."""
    out = []
    for j in range(M):
        _, _, A1, A2, B1, B2 = _factors(x, t, pad)
        q = A2 / B2 if (j < M - 1 or last_cs) else (A1 * A2) / (B1 * B2)
        out.append(q.mean(dim=(2, 3)))
        if j < M - 1:
            x, t = down(x, pool), down(t, pool)
    return out


def ms_channels(x, t, M, normalise=True, **wrong):
    """ms [n][C]: prod_j V_j^beta_j where every V_j > 0, else 0 with gradient 0; a NaN V_j gives NaN."""
    V = values(x, t, M, **wrong)
    beta = exponents(M, normalise)
    alive = torch.ones_like(V[0], dtype=torch.bool)
    nan = torch.zeros_like(alive)
    for v in V:
        alive = alive & (v > 0)
        nan = nan | torch.isnan(v)
    ms = torch.ones_like(V[0])
    for v, b in zip(V, beta):
        ms = ms * torch.where(alive, v, torch.ones_like(v)) ** b
    ms = torch.where(alive, ms, torch.zeros_like(ms))
    return torch.where(nan, torch.full_like(ms, float("nan")), ms)


def _cast(x, t, dtype):
    x = x if x.dtype == dtype else x.detach().cpu().to(dtype)
    return x, t.detach().cpu().to(dtype)


def per_image(x, t, M, dtype=torch.float64, **wrong):
    """The metric: [n] means of ms over the channels, in ``dtype``."""
    x, t = _cast(x, t, dtype)
    return ms_channels(x, t, M, **wrong).mean(dim=1)


def parts_ref(x, t, M, dtype=torch.float64, **wrong):
    """(mse, l1, 1 - mean MS-SSIM) as 0-d tensors of ``dtype``; x may require grad (it must then have ``dtype`` already)."""
    x, t = _cast(x, t, dtype)
    d = x - t
    return (d * d).mean(), d.abs().mean(), 1.0 - ms_channels(x, t, M, **wrong).mean()


def loss_ref(x, t, M, w, dtype=torch.float64, **wrong):
    """w_mse mse + w_l1 l1 + w_ms (1 - mean MS-SSIM); a term of weight 0 is left out."""
    parts = parts_ref(x, t, M, dtype, **wrong)
    return sum(float(wi) * p for wi, p in zip(w, parts) if wi > 0)


def grad_ref(x, t, M, w, gout=1.0, dtype=torch.float64, **wrong):
    """gout * d loss / d x by autograd of ``loss_ref`` in ``dtype`` (returned in ``dtype``)."""
    xr = x.detach().cpu().to(dtype).requires_grad_(True)
    (loss_ref(xr, t, M, w, dtype, **wrong) * gout).backward()
    return xr.grad.detach()


def grad_analytic(x, t, M, w, gout=1.0):
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
        ms = ms_channels(x, t, M)
        V = values(x, t, M)
        beta = exponents(M)
        win = RR._window(torch.float64, C)
        adj = lambda v: TF.conv_transpose2d(v, win, groups=C)               # noqa: E731  the "full" pass: every window that holds q
        xj, tj = x, t
        for j in range(M):
            Sj = xj.shape[-1]
            kj = torch.where(ms > 0, beta[j] * ms / V[j], torch.zeros_like(ms))
            mx, my, A1, A2, B1, B2 = _factors(xj, tj)
            if j == M - 1:
                dmu = 2 * my * A2 / (B1 * B2) - 2 * mx * A1 * A2 / (B1 * B1 * B2)
                dsig = -A1 * A2 / (B1 * B2 * B2)
                dc = 2 * A1 / (B1 * B2)
            else:
                dmu, dsig, dc = torch.zeros_like(A2), -A2 / (B2 * B2), 2 / B2
            a, b, c = dmu - 2 * mx * dsig - my * dc, 2 * dsig, dc
            gj = -w[2] * kj[:, :, None, None] / (C * n * (Sj - K + 1) ** 2) * (adj(a) + xj * adj(b) + tj * adj(c))
            up = gj.repeat_interleave(2 ** j, dim=2).repeat_interleave(2 ** j, dim=3) / 4.0 ** j
            out[:, :, :up.shape[2], :up.shape[3]] += up
            if j < M - 1:
                xj, tj = down(xj), down(tj)
    return gout * out


def fwd_bound(x, t, M, w):
    """The forward criterion: MSE and L1 gamma(K_CHAIN) of their values, the MS-SSIM part SSIM_M x (the largest distance over the batch
    between the fp32 yardstick's per-image value and float64's) + SSIM_FLOOR -- weighted, plus one rounding of the sum to fp32.  Returns
    (bound, loss64, e32, per-image float64 values)."""
    parts = parts_ref(x, t, M)
    mse, l1, _ = (float(v) for v in parts)
    loss = float(sum(float(wi) * p for wi, p in zip(w, parts) if wi > 0))
    r64 = per_image(x, t, M)
    e32 = float((per_image(x, t, M, torch.float32).double() - r64).abs().max())
    fb = w[0] * MR.gamma(MR.K_CHAIN) * mse + w[1] * MR.gamma(MR.K_CHAIN) * l1 + MR.U32 * abs(loss)
    if w[2] > 0:
        fb += w[2] * (MR.SSIM_M * e32 + MR.SSIM_FLOOR)
    return fb, loss, e32, r64


def grad_bound(x, t, M, w, gout, r64=None):
    """The gradient criterion: SSIM_M x (distance of the plain fp32 autograd from float64) + 2^-20 max |ref|.  Returns (bound, ref64,
    e32)."""
    r64 = grad_ref(x, t, M, w, gout) if r64 is None else r64
    e32 = float((grad_ref(x, t, M, w, gout, torch.float32).double() - r64).abs().max())
    return MR.SSIM_M * e32 + 2.0 ** -20 * float(r64.abs().max()), r64, e32


def brute(x, t, M):
    """ms [n][C] by double loops over windows and 2 x 2 blocks (float64), for one small batch: what the functions above are checked
    against."""
    x, t = x.detach().cpu().double(), t.detach().cpu().double()
    n, C, S, _ = x.shape
    g = MR.gaussian(K, 1.5)
    w = g[:, None] * g[None, :]
    beta = exponents(M)
    out = torch.zeros(n, C, dtype=torch.float64)
    for i in range(n):
        for c in range(C):
            a, b = x[i, c], t[i, c]
            ms, alive = 1.0, True
            for j in range(M):
                Sj = a.shape[0]
                tot = 0.0
                for r in range(Sj - K + 1):
                    for q in range(Sj - K + 1):
                        pa, pb = a[r:r + K, q:q + K], b[r:r + K, q:q + K]
                        mx, my = float((w * pa).sum()), float((w * pb).sum())
                        sx, sy = float((w * pa * pa).sum()) - mx * mx, float((w * pb * pb).sum()) - my * my
                        sxy = float((w * pa * pb).sum()) - mx * my
                        cs = (2 * sxy + C2) / (sx + sy + C2)
                        tot += cs if j < M - 1 else cs * (2 * mx * my + C1) / (mx * mx + my * my + C1)
                V = tot / (Sj - K + 1) ** 2
                alive = alive and V > 0
                if alive:
                    ms *= V ** beta[j]
                if j < M - 1:
                    h = Sj // 2
                    na, nb = torch.zeros(h, h, dtype=torch.float64), torch.zeros(h, h, dtype=torch.float64)
                    for r in range(h):
                        for q in range(h):
                            na[r, q] = 0.25 * ((a[2 * r, 2 * q] + a[2 * r, 2 * q + 1]) + (a[2 * r + 1, 2 * q] + a[2 * r + 1, 2 * q + 1]))
                            nb[r, q] = 0.25 * ((b[2 * r, 2 * q] + b[2 * r, 2 * q + 1]) + (b[2 * r + 1, 2 * q] + b[2 * r + 1, 2 * q + 1]))
                    a, b = na, nb
            out[i, c] = ms if alive else 0.0
    return out


# ---- past the grid caps -------------------------------------------------------------------------------------------------------------------
def tile_items(n, S, M):
    """Items per scale of the forward tile launch: n 3 T_j^2, T_j = ceil((S >> j) / 32)."""
    return [n * 3 * (((S >> j) + TILE - 1) // TILE) ** 2 for j in range(M)]


def planted_images(n, S, M):
    """Image 0, the images that hold the items either side of every multiple of the grid cap in the forward launch (whose items run
    over the scales in turn) and in the pyramid launch (two items per level-0 tile), the image after each, and the last image."""
    per = tile_items(1, S, M)
    at = {0, n - 1}
    start = 0
    for p in per:                                                   # forward (and, scale by scale, both backward launches)
        for k in range(1, (start + n * p) // MS_MAX_BLOCKS + 1):
            local = k * MS_MAX_BLOCKS - start
            if 0 < local < n * p:
                at |= {(local - 1) // p, local // p, local // p + 1}
        start += n * p
    for k in range(1, (2 * n * per[0]) // MS_MAX_BLOCKS + 1):       # pyramid
        local = k * MS_MAX_BLOCKS // 2
        at |= {(local - 1) // per[0], local // per[0], local // per[0] + 1}
    for k in range(1, (n * per[0]) // MS_MAX_BLOCKS + 1):           # the backward launches start their own counts at each scale group
        at |= {(k * MS_MAX_BLOCKS - 1) // per[0], k * MS_MAX_BLOCKS // per[0], k * MS_MAX_BLOCKS // per[0] + 1}
    for k in range(1, (3 * n) // FINAL_THREADS + 1):                # the final kernel's pairs
        at |= {(k * FINAL_THREADS - 1) // 3, k * FINAL_THREADS // 3, k * FINAL_THREADS // 3 + 1}
    return sorted(i for i in at if 0 <= i < n)


def planted_pair(n, S, M, seed):
    """x = t everywhere (ms = 1, loss share 0) but in the planted images, which hold a noisy pair with t -> 0.25 t + 0.4 (every channel
    alive, a quarter of the contrast: 1 - ms about 0.5): there one image's share of the loss, (1 - ms) w_ms / n, is several times the
    forward bound (the GPU test asserts the margin), so a dropped or misdecoded item at a trip boundary cannot hide."""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, 3, S, S, generator=g)
    x = t.clone()
    at = planted_images(n, S, M)
    px, pt = MR.make_pair("noisy", len(at), S, seed + 1)
    x[at], t[at] = px, 0.25 * pt + 0.4
    return x, t, at
