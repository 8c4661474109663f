"""fp64 CPU references and the elementwise error bound of tests/test_shapes_gpu.py, tests/test_channels_gpu.py and
tests/test_reductions_gpu.py (imported by the CPU tests too).

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


# ---- reductions past their grid caps and second stages (tests/test_reductions_*.py) ------------------------------------
def exceeds(err, b):
    """Number of elements of err past the bound b; a non-finite error counts as past it (NaN compares false both ways)."""
    return int((~err.le(b)).sum())


# BatchNorm statistics from partial rows (include/discogan_hip.h, csrc/norm_act.hip "Finalize from the conv kernels' partial rows"):
# a row is {count, -, -, -, shift[C], sum(y - shift)[C], sum((y - shift)^2)[C]}; row 0 has count > 0; rows with count 0 are skipped
# and their other fields are never written by the producers.
def partial_rows(y, counts, sentinel=float("nan")):
    """fp32 rows [P, 3 C + 4] of y [M, C] (fp32) cut into consecutive runs of counts[p] samples: sums in fp64 about the run's first
    sample, rounded to fp32 once.  A count-0 row holds `sentinel` in every other field -- what an uninitialised buffer may hold there."""
    y64 = f64(y)
    M, C = y64.shape
    cnt = torch.as_tensor(counts, dtype=torch.long)
    P = cnt.numel()
    assert int(cnt.sum()) == M and int(cnt[0]) > 0
    ne = cnt > 0
    first = torch.cumsum(cnt, 0) - cnt
    rid = torch.repeat_interleave(torch.arange(P), cnt)
    shift = torch.zeros(P, C, dtype=torch.float64)
    shift[ne] = y64[first[ne]]
    d = y64 - shift[rid]
    rows = torch.full((P, 3 * C + 4), sentinel, dtype=torch.float64)
    rows[:, 0] = cnt.double()
    rows[ne, 1:4] = 0.0
    rows[:, 4:4 + C] = torch.where(ne[:, None], shift, rows[:, 4:4 + C])
    s = torch.zeros(P, C, dtype=torch.float64).index_add_(0, rid, d)
    q = torch.zeros(P, C, dtype=torch.float64).index_add_(0, rid, d * d)
    rows[:, 4 + C:4 + 2 * C] = torch.where(ne[:, None], s, rows[:, 4 + C:4 + 2 * C])
    rows[:, 4 + 2 * C:] = torch.where(ne[:, None], q, rows[:, 4 + 2 * C:])
    return rows.float()


def stats_dict(mean, var, M, momentum=0.1):
    """mean, biased var (fp64 [C]) -> also the running buffers after one step from (0, 1) with the unbiased M / (M - 1)."""
    return dict(mean=mean, var=var, rmean=momentum * mean, rvar=(1 - momentum) + momentum * var * M / (M - 1))


def partial_rows_merge(rows, M, drop=None, count_empty=None, rotate_shift=False):
    """fp64 merge of partial rows, every row re-referenced to row 0's shift as the kernels do.  The wrong problems: `drop` leaves one
    row out, `count_empty` takes a count-0 row's fields as data, `rotate_shift` pairs every row's sums with the shifts of the
    neighbouring channel."""
    r = f64(rows)
    C = (r.shape[1] - 4) // 3
    use = r[:, 0] > 0
    if drop is not None:
        use[drop] = False
    if count_empty is not None:
        use[count_empty] = True
    n, sh, s, q = r[use, 0:1], r[use, 4:4 + C], r[use, 4 + C:4 + 2 * C], r[use, 4 + 2 * C:]
    if rotate_shift:
        sh = torch.roll(sh, 1, dims=1)
    G = sh[0] if rotate_shift else r[0, 4:4 + C]
    d = sh - G
    S, Q = (s + n * d).sum(0), (q + d * (2.0 * s + n * d)).sum(0)
    dm = S / M
    return stats_dict(G + dm, (Q / M - dm * dm).clamp_min(0.0), M)


# (P, C, data): "plain" y in [-1, 1); "offset" y + 100 (a mean far larger than the deviation); "ramp" y + 0.01 * row index (the rows'
# shifts differ by far more than the deviation within a row: the re-referencing term d * (2 s + n d) carries the variance)
PARTIALS_CASES = [(1, 4, "plain"), (2, 4, "plain"), (255, 12, "plain"), (256, 12, "plain"), (257, 12, "plain"), (4095, 64, "plain"),
                  (4096, 192, "plain"), (4097, 100, "offset"), (5119, 12, "ramp"), (5120, 12, "ramp"), (33000, 8, "offset")]
PARTIALS_TWO_LEVEL_FROM = 4096        # dg_bn_partials_workspace_bytes(P, C) > 0 exactly from here
PARTIALS_TOL = 2.0 ** -20             # GPU results against the fp64 statistics of y (see stats_violations)
PARTIALS_REF_TOL = 2.0 ** -22         # fp64 merge of the once-rounded rows against the same

_PARTIALS = {}


def partials_case(P, C, data):
    """One case, built once: counts in 1..7, about a tenth of the rows empty (never row 0), one run of 260 empty rows and an empty
    last row wherever P allows; sentinel NaN / 3e38 by turns.  dict: y, M, rows, ref (fp64 statistics of y), merged, wrong (list of
    (name, merge of a wrong problem))."""
    key = (P, C, data)
    if key in _PARTIALS:
        return _PARTIALS[key]
    g = torch.Generator().manual_seed(1000 + P)
    cnt = torch.randint(1, 8, (P,), generator=g)
    empty = torch.rand(P, generator=g) < 0.1
    if P >= 600:
        empty[P // 3:P // 3 + 260] = True
    if P >= 3:
        empty[-1] = True
    if P < 16:
        empty[:-1] = False
    empty[0] = False
    cnt[empty] = 0
    if P == 1:
        cnt[0] = max(int(cnt[0]), 2)                   # training-mode statistics take M >= 2
    M = int(cnt.sum())
    y = rnd(M, C, seed=2000 + P)
    rid = torch.repeat_interleave(torch.arange(P), cnt)
    if data == "offset":
        y = y + 100.0
    elif data == "ramp":
        y = y + 0.01 * rid[:, None].float()
    else:
        assert data == "plain"
    sentinel = float("nan") if PARTIALS_CASES.index(key) % 2 == 0 else 3e38
    rows = partial_rows(y, cnt, sentinel)
    y64 = f64(y)
    mean = y64.mean(0)
    ref = stats_dict(mean, ((y64 - mean) ** 2).mean(0), M)
    nonempty = (cnt > 0).nonzero().flatten()
    wrong = []
    if nonempty.numel() > 1:
        wrong.append(("row dropped", partial_rows_merge(rows, M, drop=int(nonempty[nonempty.numel() // 2]))))
    wrong.append(("shifts rotated", partial_rows_merge(rows, M, rotate_shift=True)))
    if bool(empty.any()):
        wrong.append(("empty row counted", partial_rows_merge(rows, M, count_empty=int(empty.nonzero()[0]))))
    out = dict(y=y, M=M, counts=cnt, rows=rows, ref=ref, merged=partial_rows_merge(rows, M), wrong=wrong, sentinel=sentinel)
    _PARTIALS[key] = out
    return out


def stats_violations(got, ref, tol, eps=1e-5):
    """got: dict of mean, var, rmean, rvar (fp64 [C]).  mean and running_mean within tol of (|mean| + std), var within tol of
    (var + eps), running_var within tol of (var + 1) -- the scales of test_batchnorm_channels_rows_forms.  Number of violations."""
    sc = ref["mean"].abs() + ref["var"].sqrt()
    return (exceeds((got["mean"] - ref["mean"]).abs(), tol * sc) + exceeds((got["var"] - ref["var"]).abs(), tol * (ref["var"] + eps))
            + exceeds((got["rmean"] - ref["rmean"]).abs(), tol * sc) + exceeds((got["rvar"] - ref["rvar"]).abs(), tol * (ref["var"] + 1.0)))


def stats_worst(got, ref, tol, eps=1e-5):
    """Largest error / bound ratio of stats_violations' four comparisons."""
    sc = ref["mean"].abs() + ref["var"].sqrt()
    return max(float(((got["mean"] - ref["mean"]).abs() / (tol * sc)).max()), float(((got["var"] - ref["var"]).abs() / (tol * (ref["var"] + eps))).max()),
               float(((got["rmean"] - ref["rmean"]).abs() / (tol * sc)).max()), float(((got["rvar"] - ref["rvar"]).abs() / (tol * (ref["var"] + 1.0))).max()))


# Feature matching, one layer: loss = mean_j (mean_n real - mean_n fake)^2 (csrc/loss.hip).
def fm_ref(real, fake, drop_last=False, swap=0):
    """fp64 reference on logical [N, C, H, W] tensors: dict of diff [C, H, W], absdiff (= mean_n |real| + mean_n |fake|), loss.
    Wrong problems: drop_last leaves the last image out of real's sum (still divided by N: what a dropped batch chunk computes);
    swap > 0 exchanges real and fake in the first `swap` images."""
    r, f = f64(real), f64(fake)
    N = r.shape[0]
    if swap:
        r, f = torch.cat([f[:swap], r[swap:]]), torch.cat([r[:swap], f[swap:]])
    rsum = r[:-1].sum(0) if drop_last else r.sum(0)
    diff = rsum / N - f.sum(0) / N
    return dict(diff=diff, absdiff=r.abs().sum(0) / N + f.abs().sum(0) / N, loss=(diff * diff).mean(), N=N, J=diff.numel())


def fm_diff_bound(ref):
    """N - 1 additions per mean in any order (batch chunks, then chunks), the rounded 1 / N and the product with it, the subtraction."""
    return gamma(ref["N"] + 2) * ref["absdiff"] + TINY


def fm_loss_bound(ref, terms):
    """`terms` squares per fp32 thread sum (fp64 above that): each square one rounding, terms - 1 additions, the result's rounding to
    fp32 and the scale 1 / J -> gamma(terms + 4) on the fp64 mean of squares; plus what the error b of diff moves it by:
    |(d + e)^2 - d^2| <= 2 |d| b + b^2."""
    b = fm_diff_bound(ref)
    return gamma(terms + 4) * float(ref["loss"]) * (1 + gamma(terms + 4)) + float((2 * ref["diff"].abs() * b + b * b).mean()) * (1 + gamma(terms + 4))


def capped_grid(work, cap, per_block=256):
    """Blocks of a capped streaming launch over `work` items, and the most trips any thread takes."""
    g = max(1, min((work + per_block - 1) // per_block, cap))
    return g, (work + g * per_block - 1) // (g * per_block)
