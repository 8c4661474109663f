"""Multi-scale SSIM on the GPU: forward values and gradients of dg_ms_ssim_loss_* and the rows of dg_image_ms_ssim against the float64
reference (tests/msssim_ref.py), the wrong problems the bounds reject, metric / criterion consistency, the bitwise equalities (repeat,
grouped, alignment class, graph replay), buffer discipline (NaN-filled dx, guard bands, NaN locality, dead channels), the refusals, the
shapes past the grid caps, the trainer and the CLI.

Bounds (the project's constants, tests/metrics_ref.py).  Forward: SSIM_M x (the fp32 yardstick's distance from float64 on that case,
per image) + SSIM_FLOOR for the MS-SSIM part, gamma(K_CHAIN) of their values for the MSE and L1 parts, weighted, plus one rounding of
the sum.  Gradient: SSIM_M x (the distance of the yardstick's fp32 autograd from float64) + 2^-20 max |ref|.  They rest on the data
condition tests/test_msssim_cpu.py asserts for exactly these cases.  References are computed once per case and shared."""
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
from tests import msssim_ref as MS  # noqa: E402

DEV = "cuda"
SHAPES = MS.SHAPES + (MS.BELOW_MAX,)
f32 = lambda v: float(np.float32(v))  # noqa: E731
WEIGHTS = {"ms": (0.0, 0.0, 1.0), "l1_ms": tuple(f32(v) for v in losses.recon_weights("l1_ms_ssim", 0.84)), "triple": (f32(0.3), f32(0.3), f32(0.4))}
GOUT = f32(0.7)
_REF = {}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _gout(v=GOUT):
    return torch.tensor(v, device=DEV, dtype=torch.float32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _case(n, S, M, kind, wname):
    """One case's data and float64 references, computed once: loss, per-image values, gradient, and their bounds."""
    key = (n, S, M, kind, wname)
    if key not in _REF:
        w = WEIGHTS[wname]
        at = sel = None
        if kind == "planted":
            x, t, at = MS.planted_pair(n, S, M, 100 * S + n)
            sel = sorted({j for i in at for j in (i - 1, i, i + 1) if 0 <= j < n})
        else:
            x, t = MS.make_pair(kind, n, S, 100 * S + n)
        fb, loss, fe32, rows = MS.fwd_bound(x, t, M, w)
        if sel is None:
            gb, g64, e32 = MS.grad_bound(x, t, M, w, GOUT)
        else:       # the loss is a mean over images of per-image terms: rows ``sel`` of the whole batch's gradient are the sub-batch's x m / n
            gb, g64, e32 = MS.grad_bound(x[sel], t[sel], M, w, GOUT * len(sel) / n)
        _REF[key] = dict(x=x, t=t, M=M, w=w, loss=loss, fbound=fb, fe32=fe32, rows=rows, grad=g64, gbound=gb, e32=e32, at=at, sel=sel)
    return _REF[key]


def _gpu(c):
    x, t = c["x"].to(DEV), c["t"].to(DEV)
    loss, save = ops.ms_ssim_loss_fwd(x, t, c["M"], c["w"])
    return x, t, loss, ops.ms_ssim_loss_bwd(x, t, c["M"], c["w"], _gout(), save)


def _raw(x, t, M, w, gout=GOUT, shift=0, band=64, sentinel=-12345.0):
    """The C ABI on buffers of the library's own sizes between sentinel bands, loss slot and dx pre-filled with NaN.  shift: floats by
    which dx is moved off its 16-byte boundary.  Returns (loss, dx, the three buffers with their payload ranges)."""
    L = _lib.load()
    n, S = x.shape[0], x.shape[-1]
    cw = (ctypes.c_float * 3)(*w)
    wsb, svb, bwb = L.dg_ms_ssim_workspace_bytes(n, S, M), L.dg_ms_ssim_save_bytes(n, S, M), L.dg_ms_ssim_bwd_workspace_bytes(n, S, M)
    assert 0 < bwb < wsb and svb > 0 and wsb % 4 == 0 and svb % 4 == 0 and bwb % 4 == 0
    bufs = {}
    for name, floats, off in (("ws", wsb // 4, 0), ("bws", bwb // 4, 0), ("save", svb // 4, 0), ("dx", x.numel(), shift)):
        b = torch.full((band + off + floats + band,), sentinel, device=DEV)
        assert b.data_ptr() % 16 == 0 and band % 4 == 0
        bufs[name] = (b, band + off, band + off + floats)
    dxb, lo, hi = bufs["dx"]
    dxb[lo:hi] = float("nan")
    loss = torch.full((), float("nan"), device=DEV)
    ws, sv, bws = bufs["ws"][0][band:], bufs["save"][0][band:], bufs["bws"][0][band:]
    _lib.check(L.dg_ms_ssim_loss_fwd(x.data_ptr(), t.data_ptr(), n, S, M, cw, loss.data_ptr(), sv.data_ptr(), svb, ws.data_ptr(), wsb, _stream()),
               "dg_ms_ssim_loss_fwd")
    _lib.check(L.dg_ms_ssim_loss_bwd(x.data_ptr(), t.data_ptr(), n, S, M, cw, _gout(gout).data_ptr(), sv.data_ptr(), svb, dxb[lo:].data_ptr(),
                                     bws.data_ptr(), bwb, _stream()), "dg_ms_ssim_loss_bwd")
    for name, (b, lo_, hi_) in bufs.items():
        assert bool((b[:lo_] == sentinel).all()) and bool((b[hi_:] == sentinel).all()), name
    return loss, dxb[lo:hi].view_as(x), bufs


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S,M", SHAPES)
@pytest.mark.parametrize("wname", list(WEIGHTS))
def test_forward_and_gradient_against_float64(n, S, M, wname):
    for kind in MS.KINDS:
        c = _case(n, S, M, kind, wname)
        _, _, loss, dx = _gpu(c)
        ferr = abs(float(loss) - c["loss"])
        gerr = float((dx.cpu().double() - c["grad"]).abs().max())
        print(f"n {n} S {S} M {M} {kind} {wname}: loss {c['loss']:.6f} err {ferr:.3e} e32 {c['fe32']:.3e} bound {c['fbound']:.3e} | grad max "
              f"{float(c['grad'].abs().max()):.3e} err {gerr:.3e} e32 {c['e32']:.3e} bound {c['gbound']:.3e}")
        assert ferr <= c["fbound"], (kind, ferr, c["fbound"])
        assert gerr <= c["gbound"], (kind, gerr, c["gbound"])


@pytest.mark.parametrize("n,S,M", SHAPES)
def test_metric_rows_against_float64_and_the_criterion(n, S, M):
    """dg_image_ms_ssim: every row within the forward bound of its case; row i is the per-image value of the loss (the criterion on
    image i alone is 1 - row i, each one fp32 rounding of the same double: 3 x 2^-24 as in test_recon_gpu); the criterion on the
    batch is 1 - the mean of the rows (n + 2 roundings of values <= 1)."""
    for kind in MS.KINDS:
        c = _case(n, S, M, kind, "ms")
        x, t = c["x"].to(DEV), c["t"].to(DEV)
        rows = ops.image_ms_ssim(x, t, M)
        err = float((rows.cpu().double() - c["rows"]).abs().max())
        bound = MR.SSIM_M * c["fe32"] + MR.SSIM_FLOOR
        print(f"n {n} S {S} M {M} {kind}: rows {[round(float(v), 6) for v in c['rows']]} err {err:.3e} e32 {c['fe32']:.3e} bound {bound:.3e}")
        assert err <= bound, (kind, err, bound)
        assert torch.equal(_bits(rows), _bits(ops.image_ms_ssim(x, t, M)))
        for i in range(n):
            alone = ops.image_ms_ssim(x[i:i + 1], t[i:i + 1], M)
            assert torch.equal(_bits(alone), _bits(rows[i:i + 1])), (kind, i)         # row i does not depend on n or on the other pairs
            li = float(ops.ms_ssim_loss_fwd(x[i:i + 1], t[i:i + 1], M, (0.0, 0.0, 1.0))[0])
            assert abs(li - (1.0 - float(rows[i]))) <= 3 * 2.0 ** -24, (kind, i, li, float(rows[i]))
        whole = float(ops.ms_ssim_loss_fwd(x, t, M, (0.0, 0.0, 1.0))[0])
        assert abs(whole - (1.0 - float(rows.double().mean()))) <= (n + 2) * 2.0 ** -24, (kind, whole)
        if M == ops.ms_ssim_max_scales(S):
            assert torch.equal(_bits(ops.image_ms_ssim(x, t)), _bits(rows))                # M = 0: the maximum


@pytest.mark.parametrize("n,S", [(1, 22), (2, 23), (2, 64)])
def test_one_scale_is_the_ssim_column_of_image_metrics(n, S):
    """M = 1: V_0 is the full SSIM per channel, beta_0 = 1, so a row is the mean of the channels' SSIM -- the third column of
    dg_image_metrics within that column's own bound (metrics_ref.ssim_bound) when no channel is clamped."""
    for kind in ("noisy", "flat", "dimmed"):
        x, t = MS.make_pair(kind, n, S, 100 * S + n)
        bound, ref = MR.ssim_bound(x, t)
        got = ops.image_ms_ssim(x.to(DEV), t.to(DEV), 1).cpu().double()
        col = ops.image_metrics(x.to(DEV), t.to(DEV))[:, 2].cpu().double()
        print(f"n {n} S {S} {kind}: ms {got.tolist()} ssim column {col.tolist()} bound {bound:.3e}")
        assert float((got - ref).abs().max()) <= bound and float((got - col).abs().max()) <= bound, kind


@pytest.mark.parametrize("n,S,M", SHAPES)
def test_bound_rejects_wrong_problems(n, S, M):
    """Zero-padded "same" windows, unnormalised exponents (M < 5), cs at the last scale, a 2 x 2 max-pool pyramid: each is further from
    the kernel's gradient than the bound allows.  "dimmed" for all four; "noisy" for all but cs-at-the-last-scale, which equal local
    means cannot tell from the right problem (msssim_ref.make_pair)."""
    wrongs = [dict(pad=True), dict(pool="max"), dict(last_cs=True)] + ([dict(normalise=False)] if M < MS.MAX_SCALES else [])
    for kind in ("dimmed", "noisy"):
        c = _case(n, S, M, kind, "ms")
        dx = _gpu(c)[3].cpu().double()
        for wrong in wrongs:
            if kind == "noisy" and "last_cs" in wrong:
                continue
            err = float((dx - MS.grad_ref(c["x"], c["t"], M, c["w"], GOUT, **wrong)).abs().max())
            print(f"n {n} S {S} M {M} {kind} {wrong}: distance {err:.3e} bound {c['gbound']:.3e}")
            assert err > c["gbound"], (kind, wrong, err, c["gbound"])


# ---- 2. bitwise equalities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S,M", SHAPES)
def test_repeat_grouped_and_alignment_are_bitwise(n, S, M):
    for wname in ("ms", "triple"):
        ca, cb = _case(n, S, M, "noisy", wname), _case(n, S, M, "indep", wname)
        w = ca["w"]
        xa, ta, la, da = _gpu(ca)
        xb, tb, lb, db = _gpu(cb)
        _, _, la2, da2 = _gpu(ca)
        assert torch.equal(_bits(la), _bits(la2)) and torch.equal(_bits(da), _bits(da2))
        outs = torch.full((2,), 7.0, device=DEV)
        saves = ops.ms_ssim_loss_fwd_g([xa, xb], [ta, tb], M, w, [outs[0], outs[1]])
        ga, gb = ops.ms_ssim_loss_bwd_g([xa, xb], [ta, tb], M, w, [_gout(), _gout()], saves)
        assert torch.equal(_bits(outs), _bits(torch.stack([la, lb])))
        assert torch.equal(_bits(ga), _bits(da)) and torch.equal(_bits(gb), _bits(db))
        assert not torch.equal(_bits(da), _bits(db))
        # a view one float off the 16-byte boundary: the scalar-load class, the same bits
        numel = xa.numel()
        bx, bt = torch.zeros(numel + 4, device=DEV), torch.zeros(numel + 4, device=DEV)
        xo, to = bx[1:1 + numel].view_as(xa), bt[1:1 + numel].view_as(ta)
        xo.copy_(xa)
        to.copy_(ta)
        assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
        lo, so = ops.ms_ssim_loss_fwd(xo, to, M, w)
        assert torch.equal(_bits(lo), _bits(la))
        assert torch.equal(_bits(ops.ms_ssim_loss_bwd(xo, to, M, w, _gout(), so)), _bits(da))
        assert torch.equal(_bits(ops.image_ms_ssim(xo, to, M)), _bits(ops.image_ms_ssim(xa, ta, M)))


@pytest.mark.parametrize("n,S,M", [(2, 45, 3), (2, 64, 3)])
def test_graph_replay_equals_eager(n, S, M):
    """No host synchronisation and no allocation inside the library: forward, backward and the metric are captured and replayed."""
    c = _case(n, S, M, "noisy", "triple")
    x, t, loss, dx = _gpu(c)
    rows = ops.image_ms_ssim(x, t, M)
    xs, ts = x.clone(), t.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ms_ssim_loss_fwd(xs, ts, M, c["w"])                                  # the library is loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph, go = torch.cuda.CUDAGraph(), _gout()
    with torch.cuda.graph(graph):
        gl, save = ops.ms_ssim_loss_fwd(xs, ts, M, c["w"])
        gd = ops.ms_ssim_loss_bwd(xs, ts, M, c["w"], go, save)
        gr = ops.image_ms_ssim(xs, ts, M)
    for _ in range(2):
        gl.fill_(float("nan"))
        gd.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(gl), _bits(loss)) and torch.equal(_bits(gd), _bits(dx)) and torch.equal(_bits(gr), _bits(rows))


# ---- 3. buffer discipline ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S,M", SHAPES)
def test_every_value_is_written_and_nothing_outside_the_buffers(n, S, M):
    """The C ABI on buffers of exactly the library's sizes between sentinel bands (``_raw`` checks the bands of dx, save and ws), dx
    pre-filled with NaN, 16-byte aligned and one float off: the bits of the wrapper's result."""
    for wname in ("ms", "triple"):
        c = _case(n, S, M, "indep", wname)
        x, t, loss, dx = _gpu(c)
        for shift in (0, 1):
            rl, rdx, _ = _raw(x, t, M, c["w"], shift=shift)
            assert torch.equal(_bits(rl), _bits(loss)), (wname, shift)
            assert torch.equal(_bits(rdx), _bits(dx)), (wname, shift)


@pytest.mark.parametrize("S,M", [(45, 3), (64, 3)])
def test_a_nan_stays_in_its_own_image(S, M):
    for wname in ("ms", "triple"):
        c = _case(3, S, M, "noisy", wname)
        x, t, _, clean = _gpu(c)
        rows = ops.image_ms_ssim(x, t, M)
        for where in ((1, 0, 0, 0), (1, 2, S - 1, S - 1), (1, 1, S // 2, 31)):
            bad = x.clone()
            bad[where] = float("nan")
            loss, save = ops.ms_ssim_loss_fwd(bad, t, M, c["w"])
            got = ops.ms_ssim_loss_bwd(bad, t, M, c["w"], _gout(), save)
            assert torch.equal(_bits(got[0]), _bits(clean[0])) and torch.equal(_bits(got[2]), _bits(clean[2])), (wname, where)
            assert bool(torch.isnan(got[1][where[1:]])) and bool(torch.isnan(loss))
            brow = ops.image_ms_ssim(bad, t, M)
            assert torch.equal(_bits(brow[[0, 2]]), _bits(rows[[0, 2]])) and bool(torch.isnan(brow[1])), (wname, where)


def test_a_dead_channel_has_exactly_the_gradient_of_the_other_parts():
    """smooth at n 1, S 22: every channel is clamped (tests/test_msssim_cpu.py), the MS-SSIM part is 1 with gradient exactly 0.  So dx is
    gout x (the MSE + L1 parts), the bits of dg_recon_loss_bwd with the third weight 0 (the same double combination, rounded once), and
    with the MS-SSIM weight alone dx is +0 everywhere.  indep at n 2, S 64 has dead and alive channels side by side."""
    c = _case(1, 22, 2, "smooth", "triple")
    x, t, loss, dx = _gpu(c)
    w = c["w"]
    assert torch.equal(_bits(dx), _bits(ops.recon_loss_bwd(x, t, (w[0], w[1], 0.0), _gout())))
    want = float(ops.recon_loss_fwd(x, t, (w[0], w[1], 0.0)).double()) + w[2]     # (another summation order: gamma(K_CHAIN) each)
    assert abs(float(loss) - want) <= 2 * MR.gamma(MR.K_CHAIN) * want + 2 * MR.U32 * want
    _, _, l1, d1 = _gpu(_case(1, 22, 2, "smooth", "ms"))
    assert float(l1) == 1.0 and bool((_bits(d1) == 0).all())
    assert bool((ops.image_ms_ssim(x, t, 2) == 0).all())
    c = _case(2, 64, 3, "indep", "triple")
    x, t, _, dx = _gpu(c)
    ms = MS.ms_channels(c["x"].double(), c["t"].double(), 3)
    plain = ops.recon_loss_bwd(x, t, (c["w"][0], c["w"][1], 0.0), _gout())
    assert bool((ms == 0).any()) and bool((ms > 0).any())
    for i in range(2):
        for ch in range(3):
            assert torch.equal(_bits(dx[i, ch]), _bits(plain[i, ch])) == (float(ms[i, ch]) == 0.0), (i, ch)


@pytest.mark.parametrize("n,S,M", [(2, 23, 2), (2, 64, 3)])
def test_a_zero_ms_ssim_weight_evaluates_no_stencil(n, S, M):
    """w_ms == 0: the term is not evaluated.  The save buffer keeps its sentinel (no pyramid, no k table), dx is the bits of
    dg_recon_loss_bwd under the same weights (the same double combination), the loss is within the MSE / L1 chains' gamma(K_CHAIN) of
    float64."""
    x, t = (v.to(DEV) for v in MS.make_pair("noisy", n, S, 100 * S + n))
    for w in ((0.0, 1.0, 0.0), (f32(0.5), f32(0.5), 0.0)):
        loss, dx, bufs = _raw(x, t, M, w)
        b, lo, hi = bufs["save"]
        assert bool((b[lo:hi] == -12345.0).all()), w
        assert torch.equal(_bits(dx), _bits(ops.recon_loss_bwd(x, t, w, _gout()))), w
        want = float(MS.loss_ref(x, t, M, w))
        assert abs(float(loss) - want) <= (MR.gamma(MR.K_CHAIN) + MR.U32) * want, (w, float(loss), want)


# ---- 4. past the grid caps ------------------------------------------------------------------------------------------------------------------
def _past_cap(n, S, M):
    c = _case(n, S, M, "planted", "triple")
    x, t = c["x"].to(DEV), c["t"].to(DEV)
    loss, dx, _ = _raw(x, t, M, c["w"])
    ferr = abs(float(loss) - c["loss"])
    assert bool(torch.isfinite(dx).all())                                        # dx started as NaN: every value was written
    gerr = float((dx[c["sel"]].cpu().double() - c["grad"]).abs().max())         # the planted images and their neighbours against float64
    rows = ops.image_ms_ssim(x, t, M).cpu().double()
    rerr = float((rows - c["rows"]).abs().max())
    rbound = MR.SSIM_M * c["fe32"] + MR.SSIM_FLOOR
    share = float((1.0 - c["rows"][c["at"]]).min()) * c["w"][2] / n          # the smallest planted image's share of the loss
    print(f"n {n} S {S} M {M} planted {c['at']}: loss {c['loss']:.6e} err {ferr:.3e} bound {c['fbound']:.3e} smallest share {share:.3e} | rows err "
          f"{rerr:.3e} bound {rbound:.3e} | grad max {float(c['grad'].abs().max()):.3e} err {gerr:.3e} e32 {c['e32']:.3e} bound {c['gbound']:.3e}")
    assert share > 3 * c["fbound"]                                               # a dropped planted image could not hide
    assert ferr <= c["fbound"] and rerr <= rbound and gerr <= c["gbound"]
    return c


def test_tile_kernels_past_the_grid_cap():
    """More items than MS_MAX_BLOCKS at BOTH scales: the pyramid, the forward, the coarse and the level-0 backward kernels all take a
    second trip (the pyramid and the forward a third), and the final kernel many.  16-byte loads at both levels."""
    n, S, M = MS.TILE_PAST_CAP
    assert all(p > MS.MS_MAX_BLOCKS for p in MS.tile_items(n, S, M)) and S % 8 == 0
    _past_cap(n, S, M)


def test_final_kernel_second_trip():
    """More (image, channel) pairs than the final kernel has threads, fewer items than any grid cap: its stride loop alone."""
    n, S, M = MS.FINAL_PAST_256
    assert MS.FINAL_THREADS < 3 * n and sum(MS.tile_items(n, S, M)) <= MS.MS_MAX_BLOCKS
    c = _past_cap(n, S, M)
    assert {(MS.FINAL_THREADS - 1) // 3, MS.FINAL_THREADS // 3 + 1} <= set(c["at"])


# ---- 5. refusals and the autograd nodes ------------------------------------------------------------------------------------------------
def pyramid_floats(n, S, M):
    return sum((n * 3 * (S >> j) ** 2 + 3) // 4 * 4 for j in range(1, M))


def test_c_abi_refuses_without_launching():
    L = _lib.load()
    assert [L.dg_ms_ssim_max_scales(S) for S in (10, 11, 21, 22, 64, 175, 176, 512)] == [0, 1, 1, 2, 3, 4, 5, 5]
    assert all(L.dg_ms_ssim_max_scales(S) == MS.max_scales(S) for S in range(1, 600))
    n, S, M = 2, 64, 3
    x, t = torch.rand(n, 3, S, S, device=DEV), torch.rand(n, 3, S, S, device=DEV)
    wsb, svb, bwb = L.dg_ms_ssim_workspace_bytes(n, S, M), L.dg_ms_ssim_save_bytes(n, S, M), L.dg_ms_ssim_bwd_workspace_bytes(n, S, M)
    assert bwb == pyramid_floats(n, S, M) * 4 and L.dg_ms_ssim_bwd_workspace_bytes(n, S, 4) == 0      # one float per pixel of levels 1 .. M-1
    assert L.dg_ms_ssim_workspace_bytes(n, S, 4) == 0 and L.dg_ms_ssim_save_bytes(n, 10, 1) == 0 and L.dg_ms_ssim_workspace_bytes(0, S, M) == 0
    assert svb == 2 * pyramid_floats(n, S, M) * 4 + n * 3 * M * 8                         # both pyramids and the k table
    ws, sv = torch.zeros(wsb // 4 + 4, device=DEV), torch.zeros(svb // 4 + 4, device=DEV)
    loss, dx, out, g = torch.full((), 5.0, device=DEV), torch.full_like(x, 5.0), torch.full((n,), 5.0, device=DEV), _gout()
    good = (ctypes.c_float * 3)(0.0, 0.16, 0.84)
    st = _stream()

    def fwd(x_=x.data_ptr(), t_=t.data_ptr(), n_=n, S_=S, M_=M, w_=good, l_=loss.data_ptr(), sv_=sv.data_ptr(), svb_=svb, ws_=ws.data_ptr(), wsb_=wsb):
        return L.dg_ms_ssim_loss_fwd(x_, t_, n_, S_, M_, w_, l_, sv_, svb_, ws_, wsb_, st)

    def bwd(x_=x.data_ptr(), n_=n, S_=S, M_=M, w_=good, g_=g.data_ptr(), sv_=sv.data_ptr(), svb_=svb, dx_=dx.data_ptr(), ws_=ws.data_ptr(), wsb_=wsb):
        return L.dg_ms_ssim_loss_bwd(x_, t.data_ptr(), n_, S_, M_, w_, g_, sv_, svb_, dx_, ws_, wsb_, st)

    def met(x_=x.data_ptr(), n_=n, S_=S, M_=M, o_=out.data_ptr(), ws_=ws.data_ptr(), wsb_=wsb):
        return L.dg_image_ms_ssim(x_, t.data_ptr(), n_, S_, M_, o_, ws_, wsb_, st)

    bad_w = [(ctypes.c_float * 3)(*v) for v in ((0.0, 0.0, 0.0), (0.0, -1.0, 1.0), (float("nan"), 0.0, 1.0), (float("inf"), 0.0, 0.0))]
    refused = [fwd(x_=None), fwd(t_=None), fwd(l_=None), fwd(sv_=None), fwd(ws_=None), fwd(w_=None), fwd(x_=x.data_ptr() + 2),
               fwd(sv_=sv.data_ptr() + 4), fwd(ws_=ws.data_ptr() + 8), fwd(n_=0), fwd(M_=0), fwd(M_=4), fwd(S_=10, M_=1), fwd(wsb_=wsb - 1),
               fwd(svb_=svb - 1)] + [fwd(w_=w) for w in bad_w]
    refused += [bwd(x_=None), bwd(g_=None), bwd(dx_=None), bwd(sv_=None), bwd(ws_=None), bwd(dx_=dx.data_ptr() + 1), bwd(n_=0), bwd(M_=4),
                bwd(S_=10, M_=1), bwd(wsb_=bwb - 1), bwd(svb_=svb - 1), bwd(w_=bad_w[0])]
    refused += [met(x_=None), met(o_=None), met(ws_=None), met(ws_=ws.data_ptr() + 4), met(n_=0), met(M_=0), met(M_=4), met(S_=10, M_=1),
                met(wsb_=wsb - 1)]
    assert all(rc < 0 for rc in refused), refused
    assert b"M 4 scales" in L.dg_last_error() or b"workspace" in L.dg_last_error()
    tabs = (ctypes.c_void_p * 2)(x.data_ptr(), None)
    assert L.dg_ms_ssim_loss_fwd_g(2, tabs, tabs, n, S, M, good, tabs, tabs, svb, tabs, wsb, st) < 0
    assert L.dg_ms_ssim_loss_fwd_g(5, tabs, tabs, n, S, M, good, tabs, tabs, svb, tabs, wsb, st) < 0
    torch.cuda.synchronize()
    assert float(loss) == 5.0 and bool((dx == 5.0).all()) and bool((out == 5.0).all()) and bool((sv == 0).all())       # nothing ran
    assert fwd() == 0 and bwd() == 0 and met() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx).all()) and 0.0 < float(loss) < 1.0


def test_ops_wrappers_refuse_what_the_kernels_cannot_take():
    x, t = torch.rand(2, 3, 64, 64, device=DEV), torch.rand(2, 3, 64, 64, device=DEV)
    w = WEIGHTS["l1_ms"]
    small = torch.rand(2, 3, 10, 10, device=DEV)
    with pytest.raises(_lib.DiscoganHipError, match="S >= 11"):
        ops.ms_ssim_loss_fwd(small, small.clone(), 1, (0.0, 1.0, 0.0))                # also with the MS-SSIM weight 0: the C ABI takes S >= 11
    with pytest.raises(_lib.DiscoganHipError, match="S >= 11"):
        ops.image_ms_ssim(small, small.clone())
    for M in (4, -1, 6):
        with pytest.raises(_lib.DiscoganHipError, match="scales at S=64"):
            ops.ms_ssim_loss_fwd(x, t, M, w)
        with pytest.raises(_lib.DiscoganHipError, match="scales at S=64"):
            ops.image_ms_ssim(x, t, M)
    four = torch.rand(2, 4, 64, 64, device=DEV)
    with pytest.raises(_lib.DiscoganHipError, match=r"\[n,3,S,S\]"):
        ops.ms_ssim_loss_fwd(four, four.clone(), 0, w)
    with pytest.raises(_lib.DiscoganHipError, match="fp32"):
        ops.ms_ssim_loss_fwd(x.bfloat16(), t.bfloat16(), 0, w)
    with pytest.raises(_lib.DiscoganHipError, match="target is data"):
        losses.MSSSIMLoss()(x.clone().requires_grad_(True), t.clone().requires_grad_(True))
    with pytest.raises(_lib.DiscoganHipError, match="one shape"):
        ops.ms_ssim_loss_fwd(x, t[:1], 0, w)
    with pytest.raises(_lib.DiscoganHipError, match="contiguous"):
        ops.ms_ssim_loss_fwd(x.transpose(2, 3), t.transpose(2, 3), 0, w)
    for bad in ((0.0, 0.0, 0.0), (0.0, -1.0, 1.0), (float("nan"), 0.0, 1.0), (1.0, 0.0)):
        with pytest.raises(_lib.DiscoganHipError, match="weights"):
            ops.ms_ssim_loss_fwd(x, t, 0, bad)
    with pytest.raises(_lib.DiscoganHipError, match="one shape"):
        ops.ms_ssim_loss_fwd_g([x, x[:1]], [t, t[:1]], 0, w, [torch.empty((), device=DEV)] * 2)
    torch.cuda.synchronize()


def test_modules_and_autograd_nodes():
    c = _case(2, 64, 3, "noisy", "l1_ms")
    x, t = c["x"].to(DEV), c["t"].to(DEV)
    three = torch.tensor(3.0, device=DEV)
    for mod, M, w in ((losses.MSSSIMLoss("ms_ssim"), 3, (0.0, 0.0, 1.0)), (losses.MSSSIMLoss("l1_ms_ssim", 0.84), 3, (0.0, 1.0 - 0.84, 0.84)),
                      (losses.MSSSIMLoss("l1_ms_ssim", 0.84, scales=2), 2, (0.0, 1.0 - 0.84, 0.84))):
        xr = x.clone().requires_grad_(True)
        loss = mod(xr, t)
        (loss * 3.0).backward()
        want, save = ops.ms_ssim_loss_fwd(x, t, M, w)
        assert torch.equal(_bits(loss), _bits(want))
        assert torch.equal(_bits(xr.grad), _bits(ops.ms_ssim_loss_bwd(x, t, M, w, three, save)))
    lv = torch.zeros(4, device=DEV)
    xr, yr = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
    a, b = F_.MsSsimLossGroupFn.apply(2, 3, c["w"], xr, yr, t, x, lv[1], lv[2])
    assert a.data_ptr() == lv[1].data_ptr() and float(lv[0]) == 0.0 and float(lv[3]) == 0.0
    (l_xt, s_xt), (l_tx, s_tx) = ops.ms_ssim_loss_fwd(x, t, 3, c["w"]), ops.ms_ssim_loss_fwd(t, x, 3, c["w"])
    assert torch.equal(_bits(lv[1]), _bits(l_xt)) and torch.equal(_bits(lv[2]), _bits(l_tx))
    (a * 3.0 + b * 3.0).backward()
    assert torch.equal(_bits(xr.grad), _bits(ops.ms_ssim_loss_bwd(x, t, 3, c["w"], three, s_xt)))
    assert torch.equal(_bits(yr.grad), _bits(ops.ms_ssim_loss_bwd(t, x, 3, c["w"], three, s_tx)))
    with torch.no_grad():
        assert not losses.MSSSIMLoss("ms_ssim")(x, t).requires_grad


# ---- 6. the trainer: 64 px, batch 4 -----------------------------------------------------------------------------------------------------
S_T, N_T, M_T = 64, 4, 3
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


def _run(key, iters=6, first=0, state=None, **kw):
    """Iterations ``first .. iters - 1`` of one trainer on one fixed batch; per iteration the reconstructions, their loss values and (G-steps)
    the gradient that arrived at ABA.  One run per key for the module."""
    if key not in _RUNS:
        A, B = synthetic_batch(N_T, S_T, 5, DEV)
        tr = DiscoGANTrainer(default_args(recon_loss="l1_ms_ssim"), device=DEV, image_size=S_T, seed=1234, **kw)
        assert tr.recon_ms == M_T
        if state is not None:
            assert tr.load_train_state(state) == first
        grads, inner = {}, tr.forward_losses

        def forward_losses(A_, B_, it, need_losses=True):
            out = inner(A_, B_, it, need_losses)
            if out.ABA is not None and out.ABA.requires_grad:
                out.ABA.register_hook(lambda g: grads.__setitem__(it, g.detach().clone()))
            return out

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
    assert w == WEIGHTS["l1_ms"]
    for i, it in run["per"].items():
        for x, t, got in ((it["ABA"], run["A"], it["recon"][0]), (it["BAB"], run["B"], it["recon"][1])):
            bound, want, e32, _ = MS.fwd_bound(x, t, M_T, w)
            print(f"{key} iteration {i}: loss {want:.6f} err {abs(float(got) - want):.3e} e32 {e32:.3e} bound {bound:.3e}")
            assert abs(float(got) - want) <= bound, (i, float(got), want, bound)
    assert sorted(run["grads"]) == [1, 2, 4, 5]                    # G-steps; the D-steps' generators run without a graph
    rate = f32(run["rate"])
    for i in (1, 4):
        x = run["per"][i]["ABA"]
        bound, ref, e32 = MS.grad_bound(x, run["A"], M_T, w, rate)
        err = float((run["grads"][i].double() - ref).abs().max())
        print(f"{key} iteration {i}: grad max {float(ref.abs().max()):.3e} err {err:.3e} e32 {e32:.3e} bound {bound:.3e}")
        assert err <= bound, (i, err, bound)
    assert all(bool(torch.isfinite(v).all()) for v in run["last"].values() if v.dtype == torch.float32)


def test_two_chain_equals_grouped_with_single_plans():
    chain = _run("chain", group_launch=False)
    single = _run("grouped_single", group_launch=True, group_plan="single")
    assert single["grouped"] and not chain["grouped"]
    assert _differ(single["last"], chain["last"]) == []
    for i in range(6):
        assert torch.equal(_bits(single["per"][i]["ABA"]), _bits(chain["per"][i]["ABA"]))
        for a, b in zip(single["per"][i]["recon"], chain["per"][i]["recon"]):
            assert torch.equal(_bits(a), _bits(b)), i


def test_d_step_without_losses_launches_none_of_the_kernels(monkeypatch):
    calls = []
    for name in ("ms_ssim_loss_fwd", "ms_ssim_loss_fwd_g", "ms_ssim_loss_bwd", "ms_ssim_loss_bwd_g"):
        inner = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _f=inner, _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    A, B = synthetic_batch(N_T, S_T, 5, DEV)
    for kw, fwd, bwd in ((dict(), "ms_ssim_loss_fwd_g", "ms_ssim_loss_bwd_g"), (dict(group_launch=False), "ms_ssim_loss_fwd", "ms_ssim_loss_bwd")):
        tr = DiscoGANTrainer(default_args(recon_loss="l1_ms_ssim"), device=DEV, image_size=S_T, seed=1234, **kw)
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
    assert st["iters"] == 3 and not any("recon" in k or "ssim" in k for k in st)      # nothing to checkpoint
    tail = _run("resumed", first=3, state=st)
    assert _differ(tail["last"], whole["last"]) == []
    for i in (3, 4, 5):
        for a, b in zip(tail["per"][i]["recon"], whole["per"][i]["recon"]):
            assert torch.equal(_bits(a), _bits(b)), i


def test_trainer_refuses_scales_the_size_cannot_carry():
    with pytest.raises(ValueError, match="recon_ms_scales 4 does not fit image_size 64"):
        DiscoGANTrainer(default_args(recon_loss="l1_ms_ssim", recon_ms_scales=4), device=DEV, image_size=64, seed=1234)
    with pytest.raises(ValueError, match="needs image_size >= 11"):
        DiscoGANTrainer(default_args(recon_loss="ms_ssim"), device=DEV, image_size=8, seed=1234)


# ---- 7. CLI ----------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_and_evaluates_with_the_criterion(tmp_path, capsys):
    g = torch.Generator().manual_seed(2)
    for name in ("tA", "tB"):
        torch.save(torch.randint(0, 256, (4, 64, 64, 3), generator=g, dtype=torch.uint8), tmp_path / f"{name}.pt")
    argv = ["--task_name", "edges2shoes", "--batch_size", "4", "--epochs", "6", "--log_interval", "1", "--data_source", "synthetic",
            "--synthetic_size", "16", "--image_save_interval", "0", "--results_dir", str(tmp_path / "res"), "--models_dir", str(tmp_path / "mod"),
            "--image_size", "64", "--test_A", str(tmp_path / "tA.pt"), "--test_B", str(tmp_path / "tB.pt")]
    tr = it_cli.main(argv + ["--recon_loss", "l1_ms_ssim", "--max_iters", "6", "--eval_interval", "3", "--eval_ms_ssim"])
    out = capsys.readouterr().out
    assert "reconstruction loss: l1_ms_ssim = 0 MSE + 0.16 L1 + 0.84 (1 - MS-SSIM over 3 scales)" in out
    assert tr.recon_loss == "l1_ms_ssim" and tr.recon_ms == 3
    rp, _ = it_cli.train.last_paths
    lines = [ln for ln in open(rp / "training_log.txt").read().splitlines() if ln.startswith("Iter")]
    assert len(lines) == 6
    for ln in lines:
        vals = [float(v) for v in re.search(r"RECON: ([^/,\s]+)/([^/,\s]+),", ln).groups()]
        assert len(vals) == 2 and all(np.isfinite(v) and 0.0 < v < 1.0 for v in vals), ln
    ev = open(rp / "eval_log.txt").read().splitlines()
    assert len(ev) == 2
    for ln in ev:
        m = re.search(r", RECON_MSSSIM: ([0-9.]+)/([0-9.]+) \(n=4/4\)$", ln)
        assert m and all(0.0 <= float(v) <= 1.0 for v in m.groups()), ln
    with pytest.raises(ValueError, match="recon_ms_scales 4 does not fit image_size 64"):
        it_cli.main(argv + ["--recon_loss", "l1_ms_ssim", "--recon_ms_scales", "4", "--max_iters", "3"])
    assert "reconstruction loss" not in capsys.readouterr().out
