"""fp64 CPU references and the elementwise error bound of tests/test_shapes_gpu.py (imported by the CPU tests too).

Convolutions: a sum of n products evaluated in fp32 in ANY order (split-K, trees, MFMA blocks) is within
    gamma(n) * sum |a_i * b_i|,   gamma(n) = n u / (1 - n u),  u = 2^-24
of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, 3.1), products' own rounding included.  The
sum of absolute products is the same convolution on |a| and |b|, computed here in fp64.  A product with a zero factor
is exactly zero and adding it is exact, so n counts the NONZERO products only.  The f32x3 form drops the three smallest
of the nine plane products (<= 2^-23 of |a_i b_i|) and sums six terms per product: gamma(8 n).  A bf16 output adds its
own rounding, u16 = 2^-8 of the value.

Every test also shows the bound is sharp enough to matter: the fp64 reference of the input shifted by one pixel must
violate it somewhere (`assert_discriminates`), so an H / W mix-up or an off-by-one offset in a kernel could not pass.
"""
import torch
import torch.nn.functional as TF

U32 = 2.0 ** -24
U16 = 2.0 ** -8
TINY = 2.0 ** -120


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def r16(t):
    """Round to bf16 (RNE) and return fp64: the operand values a bf16 path multiplies."""
    return t.detach().cpu().bfloat16().double()


def f64(t):
    return t.detach().cpu().double()


def conv_ref(op, a, b, stride=2, pad=1, wshape=None):
    """(reference, reference on absolute values) in fp64 on the CPU.
    op "fwd": a = x, b = w (Conv2d);  "dgrad": a = dy, b = w (its input gradient = ConvTranspose2d);
    "wgrad": a = x, b = dy, wshape = the weight's shape."""
    a, b = f64(a), f64(b)
    if op == "fwd":
        f = lambda p, q: TF.conv2d(p, q, stride=stride, padding=pad)
    elif op == "dgrad":
        f = lambda p, q: TF.conv_transpose2d(p, q, stride=stride, padding=pad)
    else:
        f = lambda p, q: torch.nn.grad.conv2d_weight(p, wshape, q, stride=stride, padding=pad)
    return f(a, b), f(a.abs(), b.abs())


def taps(op, C, K, stride=2, nz_rows=None):
    """Longest reduction of one output element: forward 16 C; stride-2 input gradient 4 K (four of the sixteen taps land on a
    pixel); the 4 x 4 head's input gradient K (its gradient has one pixel: one tap per input pixel); weight gradient = the number of
    nonzero gradient pixels (nz_rows)."""
    if op == "fwd":
        return 16 * C
    if op == "dgrad":
        return (4 if stride == 2 else 1) * K
    return nz_rows


SIGMOID_TERMS = 8


def with_epilogue(n, absref, bias=None, act="none", scaled=False):
    """(terms, absolute reference) of a sum of n products with a fused epilogue or prologue, for `bound`:
      bias    one more term of every sum; |bias| (broadcastable to absref) joins the absolute reference;
      scaled  one factor of every product is itself a rounded product (a gradient taken through an activation's derivative on the
              way in, dy * act'): one more rounding per product, counted as one more term;
      act     "relu" / "leaky": slope <= 1, so the bound of the sum holds for the activated value; leaky's multiplication by the slope
              is one more rounding (one more term).  "sigmoid": slope <= 1/4, and its own evaluation 1 / (1 + exp(-v)) -- exp, add,
              divide, each a few roundings of values <= 1 -- is covered by SIGMOID_TERMS more terms on an absolute reference raised by 1."""
    if bias is not None:
        n, absref = n + 1, absref + bias.abs()
    if scaled:
        n = n + 1
    if act == "leaky":
        n = n + 1
    elif act == "sigmoid":
        n, absref = n + SIGMOID_TERMS, absref + 1.0
    else:
        assert act in ("none", "relu"), act
    return n, absref


def bound(ref, absref, n, mult=1, out16=False):
    b = gamma(mult * n) * absref + TINY
    if out16:
        b = b * (1 + U16) + U16 * ref.abs()
    return b


def violations(got, ref, absref, n, **kw):
    return int((f64(got) - ref).abs().gt(bound(ref, absref, n, **kw)).sum())


def assert_within(got, ref, absref, n, what, **kw):
    got = f64(got)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    b = bound(ref, absref, n, **kw)
    bad = err.gt(b)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements past the bound; first at flat index {i}: "
                             f"got {got.flatten()[i].item():.9g} ref {ref.flatten()[i].item():.9g} bound {b.flatten()[i].item():.3e}")


def assert_discriminates(wrong, ref, absref, n, what, **kw):
    """The bound is not vacuous: a reference computed from a wrongly indexed input violates it."""
    assert violations(wrong, ref, absref, n, **kw) > 0, f"{what}: the bound does not tell a shifted input from the right one"


def shift_w(t):
    return torch.roll(t, 1, dims=-1)


def shift_h(t):
    return torch.roll(t, 1, dims=-2)


def shifted(t):
    """The input moved by one pixel along each spatial axis that has more than one pixel."""
    return [torch.roll(t, 1, dims=d) for d in (-1, -2) if t.shape[d] > 1]


def rot_out(w):
    """A weight [K, C, 4, 4] with its OUTPUT channels rotated by one: what a kernel that mis-indexes a ragged column tile computes."""
    return torch.roll(w, 1, dims=0)


def rot_in(w):
    """The same weight with its INPUT channels rotated by one: a K-tile (reduction chunk) paired with the wrong channels."""
    return torch.roll(w, 1, dims=1)


def wrong_problems(op, a, b):
    """(a', b') operand pairs of wrongly indexed problems of conv_ref(op, a, b): the first operand moved by one pixel along each
    spatial axis (`shifted`), and both channel rotations -- of the weight for "fwd" / "dgrad"; for "wgrad", whose operands are x and dy,
    x with its channels rotated (= the result's input channels) and dy with its channels rotated (= the result's output channels).
    A rotation over an axis of one element would be the right problem and is left out."""
    out = [(s, b) for s in shifted(a)]
    if op == "wgrad":
        if a.shape[1] > 1:
            out.append((torch.roll(a, 1, dims=1), b))
        if b.shape[1] > 1:
            out.append((a, torch.roll(b, 1, dims=1)))
    else:
        if b.shape[0] > 1:
            out.append((a, rot_out(b)))
        if b.shape[1] > 1:
            out.append((a, rot_in(b)))
    return out


def rnd(*shape, seed=0, scale=1.0):
    """Uniform in [-scale, scale) from a fixed seed (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


# ---- BatchNorm (training mode) + activation -------------------------------------------------------------------------
# Not a dot product: the kernels' statistics come from fp32 partial sums over row runs, finalised in fp64.  The fp64
# reference is held to BN_TOL of each channel's output scale S_c (z: |gamma| istd max|y - mean| + |beta|; dx: |gamma| istd
# (max|g| + |dbeta| / M + max|xhat| |dgamma| / M)), plus u16 |ref| where the output is stored as bf16.  Past 512 row chunks
# (bn_grid's cap) a thread's fp32 partial sums run over up to M / 512 rows: bn_tol(M) adds gamma(M / 512 + 64) for them.
BN_TOL = 2.0 ** -16
BN_TOL16 = 2.0 ** -12


def bn_ref(y, gamma_, beta, dz, act, slope=0.2, eps=1e-5, momentum=0.1):
    """fp64 training-mode BatchNorm2d + activation on logical NCHW tensors: dict of z, dx, dgamma, dbeta, mean, var (biased),
    running_mean / running_var after one step from (0, 1), and the per-channel scales of z and dx."""
    y, g_, b_, dz = f64(y), f64(gamma_).view(1, -1, 1, 1), f64(beta).view(1, -1, 1, 1), f64(dz)
    M = y.numel() // y.shape[1]
    mean = y.mean((0, 2, 3), keepdim=True)
    var = ((y - mean) ** 2).mean((0, 2, 3), keepdim=True)
    istd = 1.0 / torch.sqrt(var + eps)
    xhat = (y - mean) * istd
    u = xhat * g_ + b_
    if act == "leaky":
        z, d = torch.where(u > 0, u, slope * u), torch.where(u > 0, 1.0, slope)
    elif act == "relu":
        z, d = torch.where(u > 0, u, 0.0 * u), torch.where(u > 0, 1.0, 0.0)
    else:
        z, d = u, torch.ones_like(u)
    g = dz * d
    dbeta = g.sum((0, 2, 3), keepdim=True)
    dgamma = (g * xhat).sum((0, 2, 3), keepdim=True)
    dx = g_ * istd * (g - dbeta / M - xhat * dgamma / M)
    amax = lambda t: t.abs().amax((0, 2, 3), keepdim=True)
    sz = g_.abs() * istd * amax(y - mean) + b_.abs()
    # at the activation's kink the kernel's fp32 u may have the other sign: there dx with the other derivative is right too
    kink = u.abs() <= 2.0 ** -18 * sz
    d_alt = torch.where(kink, torch.where(u > 0, slope if act == "leaky" else 0.0, 1.0), d) if act != "none" else d
    dx_alt = g_ * istd * (dz * d_alt - dbeta / M - xhat * dgamma / M)
    return dict(z=z, dx=dx, dx_alt=dx_alt, dgamma=dgamma.flatten(), dbeta=dbeta.flatten(), mean=mean.flatten(), var=var.flatten(),
                rmean=momentum * mean.flatten(), rvar=(1 - momentum) + momentum * var.flatten() * M / (M - 1),
                sz=sz,
                sdx=g_.abs() * istd * (amax(g) + dbeta.abs() / M + amax(xhat) * dgamma.abs() / M),
                sg=(g * xhat).abs().sum((0, 2, 3)), sb=g.abs().sum((0, 2, 3)), M=M)


def bn_tol(M, out16=False):
    return (BN_TOL16 if out16 else BN_TOL) + gamma(M // 512 + 64)


def bn_violations(got, ref, scale, tol=BN_TOL, out16=False):
    b = tol * scale + TINY
    if out16:
        b = b + U16 * ref.abs()
    return int((f64(got) - ref).abs().gt(b).sum())


def bn_dx_violations(got, ref, tol=BN_TOL, out16=False):
    """dx against the reference, either derivative accepted where u sits on the activation's kink."""
    b = tol * ref["sdx"] + TINY
    if out16:
        b = b + U16 * ref["dx"].abs()
    got = f64(got)
    return int(torch.minimum((got - ref["dx"]).abs(), (got - ref["dx_alt"]).abs()).gt(b).sum())


def bn_roll_channels(t, k=1):
    """The same tensor with its channels rotated by k: what a kernel that reads the parameters of the wrong channel block writes."""
    return torch.roll(t, k, dims=1)
