"""The reconstruction criterion on the GPU: forward values and gradients of dg_recon_loss_* against the float64 reference
(tests/recon_ref.py) within the bounds of the metrics tests, the wrong problems those bounds reject, the bitwise equalities (repeat,
grouped, alignment class, NaN locality), the wrappers' refusals, the trainer and the CLI.

Bounds.  Forward: each part within its own -- MSE and L1 gamma(K_CHAIN) of their values (the kernel's fp32 chain), the SSIM part
``metrics_ref.ssim_bound`` -- weighted, plus one rounding of the sum to fp32.  Gradient: SSIM_M x (the distance of the reference's own
plain-fp32 autograd from float64 on that case) + 2^-20 max |ref|.  References are computed once per case and shared."""
import ctypes
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, losses, ops  # noqa: E402
from discogan_modernized_amd import functional as F_  # noqa: E402
from discogan_modernized_amd import image_translation as it_cli  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tests import metrics_ref as MR  # noqa: E402
from tests import recon_ref as RR  # noqa: E402

DEV = "cuda"
SHAPES = ((1, 11), (2, 12), (1, 43), (2, 64), (3, 75))
f32 = lambda v: float(np.float32(v))  # noqa: E731
WEIGHTS = {"l1": losses.recon_weights("l1"), "ssim": losses.recon_weights("ssim"),
           "l1_ssim": tuple(f32(v) for v in losses.recon_weights("l1_ssim", 0.84)), "triple": (f32(0.3), f32(0.3), f32(0.4))}
GOUT = f32(0.7)
_REF = {}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _gout():
    return torch.tensor(GOUT, device=DEV, dtype=torch.float32)


def _case(n, S, kind, wname):
    """One case's data and float64 references, computed once: loss, its bound, gradient, its bound."""
    key = (n, S, kind, wname)
    if key not in _REF:
        w = WEIGHTS[wname]
        sel = None
        if kind == "planted":                                  # x = t but in the images at the trip boundaries (recon_ref.planted_pair)
            x, t, at = RR.planted_pair(n, S, 100 * S + n)
            if _halves(n, S):                                  # dx is held to its halves' launches bit for bit: float64 for chosen images
                sel = sorted({j for i in at + [n // 2] for j in (i - 1, i, i + 1) if 0 <= j < n})
        else:
            x, t = MR.make_pair(kind, n, S, 100 * S + n)
        fb, loss = RR.fwd_bound(x, t, w)
        if sel is None:
            gb, g64, e32 = RR.grad_bound(x, t, w, GOUT)
        else:       # the loss is a mean over images of per-image terms: rows ``sel`` of the whole batch's gradient are the sub-batch's x m / n
            gb, g64, e32 = RR.grad_bound(x[sel], t[sel], w, GOUT * len(sel) / n)
        _REF[key] = dict(x=x, t=t, w=w, loss=loss, fbound=fb, grad=g64, gbound=gb, e32=e32, sel=sel)
    return _REF[key]


def _halves(n, S):
    """The batch splits into two launches that do not stride."""
    return n % 2 == 0 and RR.tile_items(n // 2, S)[0] <= RR.RC_MAX_BLOCKS


def _gpu(c):
    x, t = c["x"].to(DEV), c["t"].to(DEV)
    return x, t, ops.recon_loss_fwd(x, t, c["w"]), ops.recon_loss_bwd(x, t, c["w"], _gout())


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", SHAPES)
@pytest.mark.parametrize("wname", list(WEIGHTS))
def test_forward_and_gradient_against_float64(n, S, wname):
    for kind in MR.KINDS:
        c = _case(n, S, kind, wname)
        _, _, loss, dx = _gpu(c)
        ferr = abs(float(loss) - c["loss"])
        gerr = float((dx.cpu().double() - c["grad"]).abs().max())
        print(f"n {n} S {S} {kind} {wname}: loss {c['loss']:.6f} err {ferr:.3e} bound {c['fbound']:.3e} | grad max {float(c['grad'].abs().max()):.3e} "
              f"err {gerr:.3e} e32 {c['e32']:.3e} bound {c['gbound']:.3e}")
        assert ferr <= c["fbound"], (kind, ferr, c["fbound"])
        assert gerr <= c["gbound"], (kind, gerr, c["gbound"])


@pytest.mark.parametrize("n,S", SHAPES + ((2, 8),))
def test_mse_and_l1_parts_alone_are_one_rounding_from_their_formulas(n, S):
    """Weights (1, 0, 0) and (0, 1, 0): the streaming kernels, any S.  Forward within gamma(K_CHAIN); dx within one fp32 rounding of
    gout 2 (x - t) / N and gout sign(x - t) / N, sign(0) = 0."""
    x, t = MR.make_pair("noisy", n, S, 5 * S + n)
    _stream_check(x, t)


def _stream_check(x, t, share=None):
    """The criteria of the stream kernels on one pair; loss slot and dx start as NaN.  share(values [N] float64) -> the smallest
    share of the sum that one block's trip (or the tail) holds: it must exceed the forward bound, or a dropped trip could hide."""
    x[0, 1, 2, 3] = t[0, 1, 2, 3]                           # a zero difference
    x64, t64, N = x.double(), t.double(), x.numel()
    xg, tg = x.to(DEV), t.to(DEV)
    for w, terms, ref in (((1.0, 0.0, 0.0), (x64 - t64) ** 2, GOUT * 2.0 * (x64 - t64) / N),
                          ((0.0, 1.0, 0.0), (x64 - t64).abs(), GOUT * torch.sign(x64 - t64) / N)):
        val = float(terms.mean())
        if share is not None:
            least = share(terms.reshape(-1)) / N
            print(f"w {w}: value {val:.6e} bound {MR.gamma(MR.K_CHAIN) * val:.3e} smallest trip's share {least:.3e}")
            assert least > MR.gamma(MR.K_CHAIN) * val, (w, least)
        loss = float(_fwd_nan(xg, tg, w))
        assert abs(loss - val) <= MR.gamma(MR.K_CHAIN) * val, (w, loss, val)
        dx = _bwd_nan(xg, tg, w).cpu().double()
        assert bool(((dx - ref).abs() <= MR.U32 * (1 + 2.0 ** -20) * ref.abs()).all()), w
        assert float(dx[0, 1, 2, 3]) == 0.0


def _fwd_nan(x, t, w):
    """ops.recon_loss_fwd into a slot that starts as NaN."""
    return ops.recon_loss_fwd(x, t, w, out=torch.full((), float("nan"), device=DEV))


def _bwd_nan(x, t, w, gout=GOUT):
    """dg_recon_loss_bwd into a dx that starts as NaN: a value no trip wrote is not "equal"."""
    assert x.is_contiguous() and t.is_contiguous() and x.shape == t.shape
    dx = torch.full_like(x, float("nan"))
    g = torch.tensor(gout, device=DEV, dtype=torch.float32)
    _lib.check(_lib.load().dg_recon_loss_bwd(x.data_ptr(), t.data_ptr(), x.shape[0], x.shape[-1], (ctypes.c_float * 3)(*w), g.data_ptr(), dx.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "dg_recon_loss_bwd")
    return dx


@pytest.mark.parametrize("n,S", SHAPES)
def test_bound_rejects_wrong_problems(n, S):
    """Zero-padded "same" windows, sigma = 1.0, and the normalisation by S^2: each is further from the kernel's gradient than the bound
    allows, on every kind of data."""
    for wname in ("ssim", "l1_ssim"):
        for kind in MR.KINDS:
            c = _case(n, S, kind, wname)
            dx = _gpu(c)[3].cpu().double()
            for wrong in (dict(pad=True), dict(sigma=1.0), dict(norm_s2=True)):
                err = float((dx - RR.grad_ref(c["x"], c["t"], c["w"], GOUT, **wrong)).abs().max())
                print(f"n {n} S {S} {kind} {wname} {wrong}: distance {err:.3e} bound {c['gbound']:.3e}")
                assert err > c["gbound"], (kind, wrong, err, c["gbound"])


@pytest.mark.parametrize("S", (11, 43, 64))
def test_the_ssim_term_is_the_ssim_of_image_metrics(S):
    """recon.hip's promise "SSIM exactly the quantity of dg_image_metrics": one image (S = 11: one window; 43: ragged tiles, scalar
    loads; 64: 16-byte loads), weights (0, 0, 1).  Both tile kernels run one stencil (csrc/ssim_tile.h) and, with one image, both final
    kernels add the same partials in the same order and form the same double D = ss / windows.  dg_image_metrics returns fl32(D): off
    by at most 2^-24 |D|, |D| <= 1.  dg_recon_loss_fwd returns fl32(1 - D): off by at most 2^-24 |1 - D|, |1 - D| <= 2.  Together
    3 x 2^-24 -- derived, not measured; a miss means the two kernels no longer share a stencil."""
    g = torch.Generator().manual_seed(1000 + S)
    x, t = (torch.rand((1, 3, S, S), generator=g, dtype=torch.float32).to(DEV) for _ in range(2))
    loss = float(ops.recon_loss_fwd(x, t, (0.0, 0.0, 1.0)))
    ssim = float(ops.image_metrics(x, t)[0, 2].double())
    err = abs(loss - (1.0 - ssim))
    print(f"S {S}: recon loss {loss!r} 1 - SSIM {1.0 - ssim!r} distance {err:.3e} bound {3 * 2.0 ** -24:.3e}")
    assert err <= 3 * 2.0 ** -24, (S, loss, ssim, err)


# ---- 2. bitwise equalities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", SHAPES)
def test_repeat_grouped_and_alignment_are_bitwise(n, S):
    for wname in ("l1", "l1_ssim"):
        ca, cb = _case(n, S, "noisy", wname), _case(n, S, "smooth", wname)
        w = ca["w"]
        xa, ta, la, da = _gpu(ca)
        xb, tb, lb, db = _gpu(cb)
        _, _, la2, da2 = _gpu(ca)
        assert torch.equal(_bits(la), _bits(la2)) and torch.equal(_bits(da), _bits(da2))
        outs = torch.full((2,), 7.0, device=DEV)
        ops.recon_loss_fwd_g([xa, xb], [ta, tb], w, [outs[0], outs[1]])
        ga, gb = ops.recon_loss_bwd_g([xa, xb], [ta, tb], w, [_gout(), _gout()])
        assert torch.equal(_bits(outs), _bits(torch.stack([la, lb])))
        assert torch.equal(_bits(ga), _bits(da)) and torch.equal(_bits(gb), _bits(db))
        assert not torch.equal(_bits(da), _bits(db))
        # a view one float off the 16-byte boundary: the scalar-load path, the same bits
        numel = xa.numel()
        bx, bt = torch.zeros(numel + 4, device=DEV), torch.zeros(numel + 4, device=DEV)
        xo, to = bx[1:1 + numel].view_as(xa), bt[1:1 + numel].view_as(ta)
        xo.copy_(xa)
        to.copy_(ta)
        assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
        assert torch.equal(_bits(ops.recon_loss_fwd(xo, to, w)), _bits(la))
        assert torch.equal(_bits(ops.recon_loss_bwd(xo, to, w, _gout())), _bits(da))


@pytest.mark.parametrize("n,S", SHAPES)
def test_backward_writes_inside_its_buffer_only(n, S):
    """dg_recon_loss_bwd on a dx between two sentinel bands, 16-byte aligned and one float off: every value written, the bands intact,
    the bits of the wrapper's result."""
    L = _lib.load()
    band, sentinel = 64, -12345.0
    for wname in ("l1", "ssim"):
        c = _case(n, S, "indep", wname)
        x, t, _, dx = _gpu(c)
        cw = (ctypes.c_float * 3)(*c["w"])
        g = _gout()
        for shift in (0, 1):
            buf = torch.full((band + shift + x.numel() + band,), sentinel, device=DEV)
            lo = band + shift
            _lib.check(L.dg_recon_loss_bwd(x.data_ptr(), t.data_ptr(), n, S, cw, g.data_ptr(), buf[lo:].data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "dg_recon_loss_bwd")
            assert torch.equal(_bits(buf[lo:lo + x.numel()]), _bits(dx).reshape(-1)), (wname, shift)
            assert bool((buf[:lo] == sentinel).all()) and bool((buf[lo + x.numel():] == sentinel).all()), (wname, shift)


@pytest.mark.parametrize("S", [64, 75])
def test_a_nan_stays_in_its_own_image(S):
    for wname in ("l1", "l1_ssim"):
        c = _case(3, S, "noisy", wname)
        x, t, _, clean = _gpu(c)
        for where in ((1, 0, 0, 0), (1, 2, S - 1, S - 1), (1, 1, S // 2, 31)):
            bad = x.clone()
            bad[where] = float("nan")
            got = ops.recon_loss_bwd(bad, t, c["w"], _gout())
            assert torch.equal(_bits(got[0]), _bits(clean[0])) and torch.equal(_bits(got[2]), _bits(clean[2])), (wname, where)
            assert bool(torch.isnan(got[1][where[1:]])) and bool(torch.isnan(ops.recon_loss_fwd(bad, t, c["w"])))


# ---- 2b. past the grid caps: the stride loops of the tile, stream and final kernels ---------------------------------------------------
@pytest.mark.parametrize("n,S", RR.TILE_PAST_CAP)
def test_tile_kernels_past_the_grid_cap(n, S):
    """More items than RC_MAX_BLOCKS: every block of both tile kernels takes a second (at S = 11 some a third) item, and the final
    kernel many trips.  Data: recon_ref.planted_pair, whose sensitivity test_recon_cpu states.  The forward against float64 of the whole
    batch under the bound of ``_case``.  The gradient, n = 690: dx equals, bit for bit, the launches of the two halves (which do not
    stride) with gout / 2 -- gout / 2 is exact and both normalisers of half the batch are exactly twice the whole batch's, so the three
    factors gout w / N are the same doubles -- and the planted images, the last of the first and the first of the second half and
    their neighbours are held to float64 under the bound of ``_case`` taken on those images.  n = 5470 has no power-of-two split into
    sub-cap chunks, and another ratio changes the factors' roundings: float64 of the whole batch there, which is cheap at 11 px."""
    items, P = RR.tile_items(n, S)
    assert items > RR.RC_MAX_BLOCKS and items > RR.FINAL_THREADS                    # a second trip in the tile and the final kernels
    if S == 11:
        assert P == 3 and 0 < items - 2 * RR.RC_MAX_BLOCKS < RR.RC_MAX_BLOCKS      # some blocks take three items, the rest two
    else:
        assert P == 12 and RR.RC_MAX_BLOCKS % P != 0                               # four tiles per plane; the second trip starts inside an image
    assert (S % 4 == 0) == (S == 44)                                                # 16-byte loads at 44 alone
    c = _case(n, S, "planted", "triple")
    x, t = c["x"].to(DEV), c["t"].to(DEV)
    assert x.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
    loss, dx = _fwd_nan(x, t, c["w"]), _bwd_nan(x, t, c["w"])
    ferr = abs(float(loss) - c["loss"])
    gerr = float(((dx if c["sel"] is None else dx[c["sel"]]).cpu().double() - c["grad"]).abs().max())
    print(f"n {n} S {S} planted: loss {c['loss']:.6f} err {ferr:.3e} bound {c['fbound']:.3e} | grad max {float(c['grad'].abs().max()):.3e} "
          f"err {gerr:.3e} e32 {c['e32']:.3e} bound {c['gbound']:.3e}")
    assert ferr <= c["fbound"], (ferr, c["fbound"])
    assert gerr <= c["gbound"], (gerr, c["gbound"])
    if _halves(n, S):
        h = n // 2
        assert len(c["sel"]) >= 8 and {0, h - 1, h, n - 1} <= set(c["sel"])
        for lo in (0, h):
            half = _bwd_nan(x[lo:lo + h], t[lo:lo + h], c["w"], gout=GOUT / 2)
            assert torch.equal(_bits(half), _bits(dx[lo:lo + h])), lo
    else:
        assert (n, S) == (5470, 11) and c["sel"] is None


@pytest.mark.parametrize("n,S,wname", RR.FINAL_PAST_256)
def test_final_kernel_second_trip(n, S, wname):
    """More partials than the final kernel has threads, fewer than any grid cap: its stride loop alone."""
    if WEIGHTS[wname][2] > 0:
        parts = RR.tile_items(n, S)[0]
        assert RR.FINAL_THREADS < parts <= RR.RC_MAX_BLOCKS
        for kind in ("indep", "noisy"):
            c = _case(n, S, kind, wname)
            ferr = abs(float(_fwd_nan(c["x"].to(DEV), c["t"].to(DEV), c["w"])) - c["loss"])
            print(f"n {n} S {S} {kind} {wname}: {parts} partials, err {ferr:.3e} bound {c['fbound']:.3e}")
            assert ferr <= c["fbound"], (kind, ferr, c["fbound"])
    else:
        parts = RR.stream_blocks(n, S)[0]
        assert RR.FINAL_THREADS < parts <= RR.RC_STREAM_BLOCKS
        x, t = MR.make_pair("noisy", n, S, 5 * S + n)
        _stream_check(x, t, share=lambda v: float(v.reshape(-1, 1024).sum(1).min()))


@pytest.mark.parametrize("n,S", RR.STREAM_PAST_CAP)
def test_stream_kernels_past_both_caps(n, S):
    """More blocks wanted than the forward's 1024 and the backward's 2048: the stride loops of both stream kernels, with 16-byte and
    with scalar loads and a three-element tail.  One block's trip is 256 quads; the tail's differences are set to 1 so that its share,
    like every trip's, is above the bound."""
    blocks, quads, tail = RR.stream_blocks(n, S)
    assert blocks > 2 * RR.RC_STREAM_BLOCKS and (S % 4 == 0 or tail == 3)
    x, t = MR.make_pair("noisy", n, S, 5 * S + n)
    if tail:
        x.view(-1)[-tail:], t.view(-1)[-tail:] = 1.0, 0.0

    def share(v):
        body = v[:4 * quads]
        full = body[:body.numel() // 1024 * 1024].reshape(-1, 1024).sum(1)
        rest = [float(body[full.numel() * 1024:].sum())] if body.numel() % 1024 else []
        return min([float(full.min())] + rest + ([float(v[4 * quads:].sum())] if tail else []))

    _stream_check(x, t, share)


# ---- 3. refusals and the autograd nodes ------------------------------------------------------------------------------------------------
def test_ops_wrappers_refuse_what_the_kernels_cannot_take():
    x, t = torch.rand(2, 3, 16, 16, device=DEV), torch.rand(2, 3, 16, 16, device=DEV)
    w = WEIGHTS["l1_ssim"]
    small = torch.rand(2, 3, 10, 10, device=DEV)
    with pytest.raises(_lib.DiscoganHipError, match="S >= 11"):
        ops.recon_loss_fwd(small, small.clone(), w)
    with pytest.raises(_lib.DiscoganHipError, match="S >= 11"):
        ops.recon_loss_bwd(small, small.clone(), (0.0, 0.0, 1.0), _gout())
    assert float(ops.recon_loss_fwd(small, small.clone(), (0.0, 1.0, 0.0))) == 0.0        # L1 alone takes any size
    four = torch.rand(2, 4, 16, 16, device=DEV)
    with pytest.raises(_lib.DiscoganHipError, match=r"\[n,3,S,S\]"):
        ops.recon_loss_fwd(four, four.clone(), w)
    with pytest.raises(_lib.DiscoganHipError, match="fp32"):
        ops.recon_loss_fwd(x.bfloat16(), t.bfloat16(), w)
    with pytest.raises(_lib.DiscoganHipError, match="target is data"):
        ops.recon_loss_fwd(x, t.clone().requires_grad_(True), w)
    with pytest.raises(_lib.DiscoganHipError, match="target is data"):
        losses.ReconLoss("l1_ssim")(x.clone().requires_grad_(True), t.clone().requires_grad_(True))
    with pytest.raises(_lib.DiscoganHipError, match="one shape"):
        ops.recon_loss_fwd(x, t[:1], w)
    with pytest.raises(_lib.DiscoganHipError, match="contiguous"):
        ops.recon_loss_fwd(x.transpose(2, 3), t.transpose(2, 3), w)
    for bad in ((0.0, 0.0, 0.0), (0.0, -1.0, 1.0), (float("nan"), 0.0, 1.0), (float("inf"), 0.0, 0.0), (1.0, 0.0)):
        with pytest.raises(_lib.DiscoganHipError, match="weights"):
            ops.recon_loss_fwd(x, t, bad)
    with pytest.raises(_lib.DiscoganHipError, match="one shape"):
        ops.recon_loss_fwd_g([x, x[:1]], [t, t[:1]], w, [torch.empty((), device=DEV)] * 2)
    torch.cuda.synchronize()


def test_modules_and_autograd_nodes():
    """L1Loss / SSIMLoss / ReconLoss through autograd: the gradient of 3 x loss is the kernel's at gout = 3; the out= slot is written;
    the grouped node returns its slots and takes gradients for all problems or none."""
    c = _case(2, 64, "noisy", "l1_ssim")
    x, t = c["x"].to(DEV), c["t"].to(DEV)
    three = torch.tensor(3.0, device=DEV)
    for mod, w in ((losses.L1Loss(), (0.0, 1.0, 0.0)), (losses.SSIMLoss(), (0.0, 0.0, 1.0)), (losses.ReconLoss("l1_ssim", 0.84), (0.0, 1.0 - 0.84, 0.84))):
        xr = x.clone().requires_grad_(True)
        loss = mod(xr, t)
        (loss * 3.0).backward()
        assert torch.equal(_bits(loss), _bits(ops.recon_loss_fwd(x, t, w)))
        assert torch.equal(_bits(xr.grad), _bits(ops.recon_loss_bwd(x, t, w, three)))
    lv = torch.zeros(4, device=DEV)
    xr, yr = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
    a, b = F_.ReconLossGroupFn.apply(2, c["w"], xr, yr, t, x, lv[1], lv[2])
    assert a.data_ptr() == lv[1].data_ptr() and float(lv[0]) == 0.0 and float(lv[3]) == 0.0
    assert torch.equal(_bits(lv[1]), _bits(ops.recon_loss_fwd(x, t, c["w"]))) and torch.equal(_bits(lv[2]), _bits(ops.recon_loss_fwd(t, x, c["w"])))
    (a * 3.0 + b * 3.0).backward()
    assert torch.equal(_bits(xr.grad), _bits(ops.recon_loss_bwd(x, t, c["w"], three)))
    assert torch.equal(_bits(yr.grad), _bits(ops.recon_loss_bwd(t, x, c["w"], three)))
    with torch.no_grad():
        assert not losses.ReconLoss("ssim")(x, t).requires_grad


# ---- 4. the trainer: 16 px, batch 4 ------------------------------------------------------------------------------------------------------
S_T, N_T = 16, 4
_RUNS = {}


def _snapshot(tr):
    tr.finish()
    torch.cuda.synchronize()
    snap = {f"{side}.{name}": getattr(opt, name).cpu().clone() for side, opt in (("gen", tr.optim_gen), ("dis", tr.optim_dis))
            for name in ("flat_p", "exp_avg", "exp_avg_sq")}
    for k, net in tr.nets.items():
        for name, buf in net.named_buffers():
            snap[f"{k}.{name}"] = buf.detach().cpu().clone()
    return snap


def _differ(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in sorted(a) if not torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                                    b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])]


def _run(key, iters=6, kind="l1_ssim", first=0, state=None, **kw):
    """Iterations ``first .. iters - 1`` of one trainer on one fixed batch; per iteration the reconstruction, its loss values and (G-steps
    of an eager run) the gradient that arrived at ABA.  One run per key for the module."""
    if key not in _RUNS:
        A, B = synthetic_batch(N_T, S_T, 5, DEV)
        tr = DiscoGANTrainer(default_args(recon_loss=kind), device=DEV, image_size=S_T, seed=1234, **kw)
        if state is not None:
            assert tr.load_train_state(state) == first
        grads, inner = {}, tr.forward_losses

        def forward_losses(A_, B_, it, need_losses=True):
            out = inner(A_, B_, it, need_losses)
            if out.ABA is not None and out.ABA.requires_grad:
                out.ABA.register_hook(lambda g: grads.__setitem__(it, g.detach().clone()))
            return out

        if not kw.get("use_graph"):
            tr.forward_losses = forward_losses
        per = {}
        for i in range(first, iters):
            out = tr.train_iteration(A, B, i)
            torch.cuda.synchronize()
            per[i] = dict(ABA=out.ABA.detach().cpu().clone(), BAB=out.BAB.detach().cpu().clone(),
                          recon=(out.recon_loss_A.detach().cpu().clone(), out.recon_loss_B.detach().cpu().clone()))
        _RUNS[key] = dict(per=per, grads={i: g.cpu() for i, g in grads.items()}, last=_snapshot(tr), state=tr.train_state(iters),
                          grouped=bool(tr.group_launch), A=A.cpu(), B=B.cpu(), rate=tr.rate(1), w=tr.recon_w)
        del tr
    return _RUNS[key]


@pytest.mark.parametrize("key,kw", [("grouped", {}), ("chain", dict(group_launch=False))])
def test_trainer_loss_values_and_the_gradient_at_the_reconstruction(key, kw):
    run = _run(key, **kw)
    assert run["grouped"] == (key == "grouped")
    w = tuple(f32(v) for v in run["w"])
    assert w == WEIGHTS["l1_ssim"]
    for i, it in run["per"].items():
        for x, t, got in ((it["ABA"], run["A"], it["recon"][0]), (it["BAB"], run["B"], it["recon"][1])):
            mse, l1, ssim = (float(v) for v in RR.parts_ref(x, t))
            want = float(RR.loss_ref(x, t, w))
            bound = w[1] * MR.gamma(MR.K_CHAIN) * l1 + w[2] * MR.ssim_bound(x, t)[0] + MR.U32 * abs(want)
            assert abs(float(got) - want) <= bound, (i, float(got), want, bound)
    assert sorted(run["grads"]) == [1, 2, 4, 5]                    # G-steps; the D-steps' generators run without a graph
    rate = f32(run["rate"])
    for i in (1, 4):
        x = run["per"][i]["ABA"]
        bound, ref, e32 = RR.grad_bound(x, run["A"], w, rate)
        err = float((run["grads"][i].double() - ref).abs().max())
        print(f"{key} iteration {i}: grad max {float(ref.abs().max()):.3e} err {err:.3e} e32 {e32:.3e} bound {bound:.3e}")
        assert err <= bound, (i, err, bound)
    assert all(bool(torch.isfinite(v).all()) for v in run["last"].values() if v.dtype == torch.float32)
    assert _differ(run["last"], _run("mse", kind="mse")["last"])    # the criterion trains other weights than the default


def test_graph_replay_equals_eager_dispatch():
    for name, kw in (("grouped", {}), ("chain", dict(group_launch=False))):
        eager, graph = _run(name, **kw), _run(name + "_graph", use_graph=True, **kw)
        assert _differ(graph["last"], eager["last"]) == []
        for i in range(6):
            for a, b in zip(graph["per"][i]["recon"], eager["per"][i]["recon"]):
                assert torch.equal(_bits(a), _bits(b)), (name, i)


def test_two_chain_equals_grouped_with_single_plans():
    chain = _run("chain", group_launch=False)
    single = _run("grouped_single", group_launch=True, group_plan="single")
    assert single["grouped"] and not chain["grouped"]
    assert _differ(single["last"], chain["last"]) == []
    for i in range(6):
        assert torch.equal(_bits(single["per"][i]["ABA"]), _bits(chain["per"][i]["ABA"]))
        for a, b in zip(single["per"][i]["recon"], chain["per"][i]["recon"]):
            assert torch.equal(_bits(a), _bits(b)), i


def test_d_step_without_losses_launches_no_recon_kernel(monkeypatch):
    calls = []
    for name in ("recon_loss_fwd", "recon_loss_fwd_g", "recon_loss_bwd", "recon_loss_bwd_g"):
        inner = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _f=inner, _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    A, B = synthetic_batch(N_T, S_T, 5, DEV)
    for kw, fwd, bwd in ((dict(), "recon_loss_fwd_g", "recon_loss_bwd_g"), (dict(group_launch=False), "recon_loss_fwd", "recon_loss_bwd")):
        tr = DiscoGANTrainer(default_args(recon_loss="l1_ssim"), device=DEV, image_size=S_T, seed=1234, **kw)
        del calls[:]
        out = tr.train_iteration(A, B, 0, need_losses=False)
        torch.cuda.synchronize()
        assert calls == [] and out.ABA is None
        assert bool(torch.isnan(out.recon_loss_A)) and bool(torch.isnan(out.recon_loss_B)) and bool(torch.isnan(out.lossvec[:2]).all())
        out = tr.train_iteration(A, B, 3)                            # a D-step that logs: forward only
        torch.cuda.synchronize()
        assert set(calls) == {fwd} and bool(torch.isfinite(out.lossvec[:2]).all())
        del calls[:]
        tr.train_iteration(A, B, 4)                                  # a G-step: forward and backward
        torch.cuda.synchronize()
        assert set(calls) == {fwd, bwd}
        del tr


def test_resume_continues_bitwise(tmp_path):
    whole = _run("grouped")
    torch.save(_run("head3", iters=3)["state"], tmp_path / "state.pth")
    st = torch.load(tmp_path / "state.pth")
    assert st["iters"] == 3 and not any("recon" in k for k in st)
    tail = _run("resumed", first=3, state=st)
    assert _differ(tail["last"], whole["last"]) == []
    for i in (3, 4, 5):
        for a, b in zip(tail["per"][i]["recon"], whole["per"][i]["recon"]):
            assert torch.equal(_bits(a), _bits(b)), i


def test_trainer_refuses_a_bad_criterion():
    with pytest.raises(ValueError, match="needs image_size >= 11"):
        DiscoGANTrainer(default_args(recon_loss="ssim"), device=DEV, image_size=8, seed=1234)
    with pytest.raises(ValueError, match="unknown reconstruction loss"):
        DiscoGANTrainer(default_args(recon_loss="huber"), device=DEV, image_size=16, seed=1234)
    with pytest.raises(ValueError, match="recon_ssim_alpha must be in"):
        DiscoGANTrainer(default_args(recon_loss="l1_ssim", recon_ssim_alpha=1.0), device=DEV, image_size=16, seed=1234)


# ---- 5. CLI ----------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_with_the_criterion(tmp_path, capsys):
    argv = ["--task_name", "edges2shoes", "--batch_size", "4", "--epochs", "3", "--log_interval", "1", "--data_source", "synthetic",
            "--synthetic_size", "16", "--image_save_interval", "0", "--results_dir", str(tmp_path / "res"), "--models_dir", str(tmp_path / "mod")]
    tr = it_cli.main(argv + ["--recon_loss", "l1_ssim", "--image_size", "16", "--max_iters", "3"])
    out = capsys.readouterr().out
    assert "reconstruction loss: l1_ssim = 0 MSE + 0.16 L1 + 0.84 (1 - SSIM)" in out
    assert tr.recon_loss == "l1_ssim"
    rp, _ = it_cli.train.last_paths
    lines = [ln for ln in open(rp / "training_log.txt").read().splitlines() if ln.startswith("Iter")]
    assert len(lines) == 3
    for ln in lines:
        vals = [float(v) for v in re.search(r"RECON: ([^/,\s]+)/([^/,\s]+),", ln).groups()]
        assert len(vals) == 2 and all(np.isfinite(v) and 0.0 < v < 1.0 for v in vals), ln
    with pytest.raises(ValueError, match="recon_loss 'ssim' needs image_size >= 11"):
        it_cli.main(argv + ["--recon_loss", "ssim", "--image_size", "8", "--max_iters", "3"])
    assert "reconstruction loss" not in capsys.readouterr().out
