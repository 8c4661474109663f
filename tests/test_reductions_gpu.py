"""Reduction and streaming kernels past their grid caps and second stages: the BatchNorm partial-row merge on synthetic rows (one
launch and two-level), feature matching with chunked batches and capped grids, the scalar losses (two-stage MSE, hinge, BCE against
a tensor target), and the activations, Adam and the plane split where every thread takes a second trip.  Every result is held to a
float64 CPU reference under a bound from the rounding model (tests/shape_ref.py), every size-driven case asserts from a host query
or the documented caps that it is in the regime it is about, and every bound is shown to tell a wrong problem from the right one.
Each test prints its worst error / bound ratio (pytest -s)."""
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, losses, ops  # noqa: E402
from tests import shape_ref as R  # noqa: E402
from tests import test_ops_gpu as T  # noqa: E402
from tests.gpu_util import DEV, nhwc  # noqa: E402
from tests.adam_ref import hyper, split3  # noqa: E402
from tests.adam_ref import one_step as adam_one_step  # noqa: E402
from tests.shape_ref import assert_within, f64, gamma, rnd, violations  # noqa: E402

EPS = 1e-5


def loss_cap():
    """Block cap of the two-stage loss sums: one fp64 partial per block in the loss workspace."""
    return _lib.load().dg_loss_workspace_bytes() // 8


def worst(err, b):
    return float((err / b).max())


# ==== A. BatchNorm statistics from partial rows =======================================================================
PARTIALS_RUNS = [(P, C, data, form) for P, C, data in R.PARTIALS_CASES
                 for form in (("one_launch", "two_level") if P >= R.PARTIALS_TWO_LEVEL_FROM else ("one_launch",))]


@pytest.mark.parametrize("P,C,data,form", PARTIALS_RUNS)
def test_bn_stats_from_partial_rows(P, C, data, form, monkeypatch):
    k = R.partials_case(P, C, data)
    M, ref = k["M"], k["ref"]
    L = _lib.load()
    wsb = L.dg_bn_partials_workspace_bytes(P, C)
    assert (wsb > 0) == (P >= R.PARTIALS_TWO_LEVEL_FROM)
    if form == "two_level":
        rb = wsb // (2 * ((C + 3) // 4 * 4) * 8)
        assert rb >= 2 and (P < 33000 or (rb == 64 and P > 2 * rb * 256)), "row blocks: a second stage, and at 33000 rows several trips"
    else:
        monkeypatch.setattr(ops, "_PARTIALS_ONE_LAUNCH", P >= R.PARTIALS_TWO_LEVEL_FROM)
        assert ops._PARTIALS_ONE_LAUNCH or wsb == 0       # the one-launch form (256 rows per trip: from P = 257 a second trip)
    rows = k["rows"].to(DEV)
    y = torch.empty(1, device=DEV).expand(M, C, 1, 1)     # the wrapper reads y's shape and device only
    rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
    saved = ops.bn_stats_from_partials(rows, y, rm, rv, nbt, EPS, 0.1)
    torch.cuda.synchronize()
    assert int(nbt) == 1 and saved.shape == (2, C)
    got = dict(mean=f64(saved[0]), var=1.0 / f64(saved[1]) ** 2 - EPS, rmean=f64(rm), rvar=f64(rv))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    print(f"RATIO partials P={P} C={C} {data} {form}: {R.stats_worst(got, ref, R.PARTIALS_TOL):.3f}")
    assert R.stats_violations(got, ref, R.PARTIALS_TOL) == 0
    for name, wrong in k["wrong"]:
        assert R.stats_violations(wrong, ref, R.PARTIALS_TOL) > 0, name


# ==== B. Feature matching ================================================================================================
def fm_geometry(N, J):
    """(batch chunks, images per chunk, squares per fp32 thread sum of the diff stage) from the host queries: the workspace holds the
    loss partials and [2][chunks][J] floats; the diff stage runs J / 4 vector items on at most loss_cap() blocks."""
    L = _lib.load()
    nch = (L.dg_fm_workspace_bytes(N, J) - L.dg_loss_workspace_bytes()) // (2 * J * 4)
    _, trips = R.capped_grid(J // 4, loss_cap())
    return nch, (N + nch - 1) // nch, 4 * trips


def mem_to_logical(flat, like, shape):
    """A [J] vector in `like`'s memory order -> logical [C, H, W]."""
    C, H, W = shape
    return flat.view(H, W, C).permute(2, 0, 1) if ops.is_nhwc(like) else flat.view(C, H, W)


def fm_check(real, fake, loss, diff, rd, dreal, dfake, g, what, io16=False):
    """loss, diff and the gradients of one feature-matching problem against float64; returns the reference."""
    ref = R.fm_ref(real, fake)
    N, J = ref["N"], ref["J"]
    nch, per, terms = fm_geometry(N, J)
    b = R.fm_diff_bound(ref)
    d = f64(mem_to_logical(diff, rd, real.shape[1:]))
    assert bool(torch.isfinite(d).all())
    ed = (d - ref["diff"]).abs()
    lb = R.fm_loss_bound(ref, terms)
    el = abs(float(loss) - float(ref["loss"]))
    print(f"RATIO fm {what}: diff {worst(ed, b):.3f} loss {el / lb:.3f}")
    assert R.exceeds(ed, b) == 0, f"{what}: diff"
    assert el <= lb, f"{what}: loss {float(loss):.9g} ref {float(ref['loss']):.9g} bound {lb:.3e}"
    # gradients: 2 g diff / (N J) for every image.  diff's own bound (relative to mean|real| + mean|fake|, not to |diff|: the two
    # means cancel) and three more roundings for the scale -> gamma(N + 5) on the reference evaluated on absolute values; a bf16
    # gradient adds its own rounding.  Against the kernel's own diff only the scale's roundings remain.
    sc = 2.0 * float(g) / (float(N) * float(J))
    gref, gabs = sc * ref["diff"], abs(sc) * ref["absdiff"]
    gb = gamma(N + 5) * gabs + R.TINY
    own = sc * d
    ob = gamma(5) * own.abs() + R.TINY
    if io16:
        gb, ob = gb * (1 + R.U16) + R.U16 * gref.abs(), ob * (1 + R.U16) + R.U16 * own.abs()
    for name, got, sign in (("dreal", dreal, 1.0), ("dfake", dfake, -1.0)):
        if got is None:
            continue
        assert got.shape == real.shape and got.dtype == (torch.bfloat16 if io16 else torch.float32)
        gg = f64(got) * sign
        assert bool(torch.isfinite(gg).all())
        e1, e2 = (gg - gref).abs().amax(0), (gg - own).abs().amax(0)
        print(f"RATIO fm {what} {name}: vs float64 {worst(e1, gb):.3f} vs own diff {worst(e2, ob):.3f}")
        assert R.exceeds(e1, gb) == 0, f"{what}: {name}"
        assert R.exceeds(e2, ob) == 0, f"{what}: {name} against the kernel's own diff"
    # the bounds tell the wrong problems from the right one
    swap = per if nch > 1 else (N + 1) // 2      # (one chunk: exchanging the whole batch only negates diff, so half of it)
    for wrong in (R.fm_ref(real, fake, drop_last=True), R.fm_ref(real, fake, swap=swap)):
        assert R.exceeds((wrong["diff"] - ref["diff"]).abs(), b) > 0, f"{what}: diff bound vacuous"
        assert abs(float(wrong["loss"]) - float(ref["loss"])) > lb, f"{what}: loss bound vacuous"
    return ref


# (N, C, H, W) -> batch chunks fm_chunks picks
FM_CASES = [((8, 128, 8, 8), 2), ((9, 128, 8, 8), 2), ((13, 128, 8, 8), 3), ((17, 128, 8, 8), 4), ((260, 128, 8, 8), 64),
            ((9, 64, 129, 128), 1)]


@pytest.mark.parametrize("shape,chunks", FM_CASES, ids=["x".join(map(str, s)) for s, _ in FM_CASES])
def test_feature_matching_chunks_and_caps(shape, chunks):
    N, J = shape[0], shape[1] * shape[2] * shape[3]
    nch, per, terms = fm_geometry(N, J)
    assert nch == chunks
    if N == 9 and chunks == 2:
        assert (per, N - per) == (5, 4)                                   # ragged last chunk
    if N == 260:
        assert (N + per - 1) // per == 52 and N * (J // 4) > 2048 * 256   # twelve empty chunks; the backward's grid cap binds
    if chunks == 1:
        assert J // 4 > loss_cap() * 256 and terms == 8                   # the diff stage takes a second trip
    real, fake = rnd(*shape, seed=1), rnd(*shape, seed=2)
    rg, fg = nhwc(real), nhwc(fake)
    g = torch.tensor(0.9, device=DEV)
    loss, diff, rd, fd = ops.fm_fwd(rg, fg)
    dreal, dfake = ops.fm_bwd(diff, rd, fd, g, True, True)
    torch.cuda.synchronize()
    fm_check(real, fake, loss, diff, rd, dreal, dfake, g, f"{shape}")
    if J <= 1 << 16:
        only_r, none_f = ops.fm_bwd(diff, rd, fd, g, True, False)
        none_r, only_f = ops.fm_bwd(diff, rd, fd, g, False, True)
        assert none_f is None and none_r is None and torch.equal(only_r, dreal) and torch.equal(only_f, dfake)


@pytest.mark.parametrize("N", [9, 17])
def test_feature_matching_bf16_storage_chunks(N):
    shape = (N, 128, 8, 8)
    real, fake = rnd(*shape, seed=1).bfloat16().float(), rnd(*shape, seed=2).bfloat16().float()      # the reference sees the rounded inputs
    assert fm_geometry(N, 128 * 64)[0] == N // 4
    rg, fg = nhwc(real, torch.bfloat16), nhwc(fake, torch.bfloat16)
    g = torch.tensor(0.9, device=DEV)
    loss, diff, rd, fd = ops.fm_fwd(rg, fg)
    dreal, dfake = ops.fm_bwd(diff, rd, fd, g, True, True)
    torch.cuda.synchronize()
    fm_check(real, fake, loss, diff, rd, dreal, dfake, g, f"bf16 {shape}", io16=True)


def test_feature_matching_grouped_against_float64():
    shape = (9, 128, 8, 8)
    reals, fakes = [rnd(*shape, seed=1 + 10 * i) for i in range(2)], [rnd(*shape, seed=2 + 10 * i) for i in range(2)]
    outs = [torch.empty((), device=DEV) for _ in range(2)]
    gouts = [torch.tensor(0.9 - 0.4 * i, device=DEV) for i in range(2)]
    diffs, rd, fd = ops.fm_fwd_g([nhwc(r) for r in reals], [nhwc(f) for f in fakes], outs)
    dreals, dfakes = ops.fm_bwd_g(diffs, rd, fd, gouts, True, True)
    torch.cuda.synchronize()
    for i in range(2):
        fm_check(reals[i], fakes[i], outs[i], diffs[i], rd[i], dreals[i], dfakes[i], gouts[i], f"grouped {i}")


@pytest.mark.parametrize("real_nhwc", [True, False])
def test_feature_matching_mixed_layouts(real_nhwc):
    """A contiguous-NCHW tensor against an NHWC-memory one: the wrapper brings both to one layout."""
    shape = (9, 128, 8, 8)
    real, fake = rnd(*shape, seed=1), rnd(*shape, seed=2)
    rg, fg = (nhwc(real), fake.to(DEV)) if real_nhwc else (real.to(DEV), nhwc(fake))
    assert ops.is_nhwc(rg) != ops.is_nhwc(fg)
    g = torch.tensor(0.9, device=DEV)
    loss, diff, rd, fd = ops.fm_fwd(rg, fg)
    assert rd.stride() == fd.stride()
    dreal, dfake = ops.fm_bwd(diff, rd, fd, g, True, True)
    torch.cuda.synchronize()
    fm_check(real, fake, loss, diff, rd, dreal, dfake, g, f"mixed layouts, real nhwc {real_nhwc}")


# ==== C. Scalar losses ===================================================================================================
GOUT = 0.37


def scalar_loss_check(got, ref, b, what):
    got = float(got.detach()) if torch.is_tensor(got) else float(got)
    e = abs(got - float(ref))
    print(f"RATIO {what}: {e / b:.3f}")
    assert e <= b, f"{what}: got {got:.9g} ref {float(ref):.9g} bound {b:.3e}"


MSE_CASES = [((2097159,), False), ((1048577,), False), ((3, 8, 5, 7), True)]


@pytest.mark.parametrize("shape,nhwc_in", MSE_CASES, ids=["2097159", "1048577", "nhwc-3x8x5x7"])
def test_mse_two_stage_sum(shape, nhwc_in):
    x, t = torch.rand(shape, generator=torch.Generator().manual_seed(1)), torch.rand(shape, generator=torch.Generator().manual_seed(2))
    n = x.numel()
    if n % 4:
        x.view(-1)[n - n % 4:], t.view(-1)[n - n % 4:] = 1.0, 0.0        # the tail's squares are 1: one of them dropped or taken twice shows
    cap = loss_cap()
    blocks, trips = R.capped_grid(n // 4, cap)
    if n > 1 << 20:
        assert (n // 4 + 1 + 255) // 256 > cap                    # the grid cap binds
    if n > 1 << 21:
        assert trips >= 2 and n % 4 == 3                          # every thread a second trip, and a three-element tail
    # a thread's fp32 sum: four squares per trip (+ the tail on one thread); every square carries the subtraction's rounding twice and
    # its own, the additions one each -> gamma(terms + 3); the fp32 result one more rounding
    terms = 4 * trips + n % 4
    x64, t64 = f64(x), f64(t)
    sq = (x64 - t64) ** 2
    ref = float(sq.mean())
    lb = gamma(terms + 3) * ref + R.U32 * ref
    g32 = torch.tensor(GOUT, dtype=torch.float32)
    gref = 2.0 * float(g32) * (x64 - t64) / n
    xg, tg = (nhwc(x) if nhwc_in else x.to(DEV)), t.to(DEV)
    loss, xd, td = ops.mse_fwd(xg, tg)
    dx = ops.mse_bwd(xd, td, g32.to(DEV))
    xa, ta = xg.clone().requires_grad_(True), tg.clone().requires_grad_(True)
    la = losses.MSELoss()(xa, ta)
    (la * GOUT).backward()
    torch.cuda.synchronize()
    scalar_loss_check(loss, ref, lb, f"mse {shape} ops")
    scalar_loss_check(la, ref, lb, f"mse {shape} module")
    for name, got, r in (("ops dx", dx, gref), ("autograd dx", xa.grad, gref), ("autograd dtarget", ta.grad, -gref)):
        assert_within(got, r, r.abs(), 4, f"mse {shape} {name}")
    assert violations(torch.roll(gref, 1, dims=-1), gref, gref.abs(), 4) > 0
    # wrong problems: one block's share of the elements left out of the sum (one element where that is more than the bound)
    share = n // blocks if n > 1000 else 1
    wrong = float(sq.flatten()[:share].sum()) if share > 1 else float(sq.max())
    assert wrong / n > lb, "mse: the loss bound does not see a dropped share"
    assert n % 4 == 0 or 1.0 / n > lb, "mse: the loss bound does not see one tail element"


def hinge_inputs(n, margin, seed=3):
    x = rnd(n, seed=seed, scale=2.0)
    y = torch.where(torch.rand(n, generator=torch.Generator().manual_seed(seed + 1)) < 0.5, 1.0, -1.0)
    y[0] = 1.0
    if n >= 7:
        x[3::5] = margin                                           # exactly on the margin, under both targets
        y[3] = -1.0
    if n >= 10:
        y[8] = 1.0
    return x, y


def hinge_check(x, y, margin, xg, yg, what):
    n = x.numel()
    x64, y64 = f64(x).requires_grad_(True), f64(y)
    ref = TF.hinge_embedding_loss(x64, y64, margin=margin)
    g32 = torch.tensor(GOUT, dtype=torch.float32)
    (ref * float(g32)).backward()
    ref, gref = ref.detach(), x64.grad
    onkink = (f64(x) == margin) & (y64 == -1.0)
    galt = torch.where(onkink, -float(g32) / n - gref, gref)       # at x == margin either one-sided derivative (0 or -g / n)
    terms_each = torch.where(y64 == 1.0, f64(x), (margin - f64(x)).clamp_min(0.0))
    _, trips = R.capped_grid(n, loss_cap())
    # one term per element and trip: margin - x rounds once, each addition once; the fp32 result once more
    lb = gamma(trips + 3) * float(terms_each.abs().mean()) + R.U32 * abs(float(ref)) + R.TINY
    loss, xd, yd = ops.hinge_fwd(xg, yg, margin)
    dx = ops.hinge_bwd(xd, yd, margin, g32.to(DEV))
    xa = xg.clone().requires_grad_(True)
    la = losses.HingeEmbeddingLoss(margin)(xa, yg)
    (la * GOUT).backward()
    torch.cuda.synchronize()
    scalar_loss_check(loss, ref, lb, f"hinge {what} ops")
    scalar_loss_check(la, ref, lb, f"hinge {what} module")
    gb = gamma(2) * gref.abs() + R.TINY                            # g / n rounds once
    for name, got in (("ops", dx), ("autograd", xa.grad)):
        got = f64(got)
        assert got.shape == gref.shape
        e = torch.minimum((got - gref).abs(), (got - galt).abs())
        assert R.exceeds(e, torch.maximum(gb, gamma(2) * galt.abs() + R.TINY)) == 0, f"hinge {what}: {name} gradient"
    assert bool(onkink.any()) == (n >= 7)
    # wrong problems
    if n <= 1000:
        i = int(terms_each.abs().argmax())
        assert abs(float(terms_each.flatten()[i])) / n > lb, "hinge: one element dropped"
        flipped = torch.where(y64 == 1.0, (margin - f64(x)).clamp_min(0.0), f64(x))
        assert float((flipped - terms_each).abs().max()) / n > lb, "hinge: one target flipped"
    else:
        blocks, _ = R.capped_grid(n, loss_cap())
        assert abs(float(terms_each.flatten()[:n // blocks].sum())) / n > lb, "hinge: one block's share dropped"


@pytest.mark.parametrize("margin", [1.0, 0.25])
@pytest.mark.parametrize("n", [1, 7, 1000, 300001])
def test_hinge_embedding_loss(n, margin):
    if n > 1000:
        assert n > loss_cap() * 256                                # past the block cap: a second trip
    x, y = hinge_inputs(n, margin)
    hinge_check(x, y, margin, x.to(DEV), y.to(DEV), f"n={n} margin={margin}")


def test_hinge_embedding_loss_nhwc_input():
    x, y = hinge_inputs(2 * 6 * 5 * 3, 0.25, seed=7)
    x, y = x.view(2, 6, 5, 3), y.view(2, 6, 5, 3)
    xg = nhwc(x)
    assert ops.is_nhwc(xg) and not xg.is_contiguous()
    hinge_check(x, y, 0.25, xg, y.to(DEV), "nhwc input, contiguous target")


BCE_SPECIAL = [0.0, 1.0, 1e-30, 4e-18, 0.9999999, 0.3, 0.9, 0.5]


def bce_terms(p64, t64):
    return -(t64 * torch.log(p64).clamp_min(-100.0) + (1.0 - t64) * torch.log1p(-p64).clamp_min(-100.0))


def bce_check(p, t, loss, dp, what):
    """Project tolerances of test_bce_including_saturation: loss rtol 1e-6 / atol 1e-7, gradient rtol 1e-5 elementwise."""
    n = p.numel()
    p64, t64 = f64(p), f64(t)
    ref = TF.binary_cross_entropy(p64, t64)
    g = float(torch.tensor(GOUT, dtype=torch.float32))
    gref = g * (p64 - t64) / ((1.0 - p64) * p64).clamp_min(1e-12) / n
    lb = 1e-6 * abs(float(ref)) + 1e-7
    scalar_loss_check(loss, ref, lb, f"bce {what}")
    got = f64(dp).reshape(-1)
    assert bool(torch.isfinite(got).all())
    e = (got - gref).abs()
    print(f"RATIO bce {what} gradient: {float((e / (1e-5 * gref.abs()).clamp_min(1e-300)).max()):.3f}")
    assert R.exceeds(e, 1e-5 * gref.abs()) == 0, f"bce {what}: gradient"
    terms = bce_terms(p64, t64)
    assert abs(float(terms.mean()) - float(ref)) <= 1e-12 * abs(float(ref))
    assert float(terms.max()) / n > lb, "bce: one element dropped"
    assert float((bce_terms(p64, 1.0 - t64) - terms).abs().max()) / n > lb, "bce: one target flipped"


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("n", [8, 256, 257, 1000])
def test_bce_against_tensor_target(n, soft):
    p = torch.rand(n, generator=torch.Generator().manual_seed(5))
    p[:8] = torch.tensor(BCE_SPECIAL)
    u = torch.rand(n, generator=torch.Generator().manual_seed(6))
    t = u if soft else (u < 0.5).float()
    if not soft:
        t[0], t[1] = 1.0, 0.0                                      # log(0) under the weight 1: the -100 clamp, both sides
    pg, tg, gout = p.to(DEV), t.to(DEV), torch.tensor(GOUT, device=DEV)
    loss, pc, tc = ops.bce_target_fwd(pg, tg)
    dp = ops.bce_target_bwd(pc, tc, gout)
    pa = pg.clone().view(-1, 1).requires_grad_(True)
    target = tg.view(-1, 1)
    assert getattr(target, "_dg_label", None) is None
    la = losses.BCELoss()(pa, target)
    (la * GOUT).backward()
    torch.cuda.synchronize()
    bce_check(p, t, loss, dp, f"n={n} {'soft' if soft else 'hard'} ops")
    bce_check(p, t, la, pa.grad, f"n={n} {'soft' if soft else 'hard'} module")


@pytest.mark.parametrize("label", [1.0, 0.0])
@pytest.mark.parametrize("n", [257, 1000])
def test_bce_scalar_label_second_trip(n, label):
    assert n > 256                                                 # dg_bce_fwd: one block, stride 256
    p = torch.rand(n, generator=torch.Generator().manual_seed(5))
    p[:8] = torch.tensor(BCE_SPECIAL)
    loss, pc = ops.bce_fwd(p.to(DEV), label)
    dp = ops.bce_bwd(pc, label, torch.tensor(GOUT, device=DEV))
    torch.cuda.synchronize()
    bce_check(p, torch.full((n,), label), loss, dp, f"n={n} label={label}")


# ==== D. Activations, Adam and the plane split past their caps ===========================================================
def close64(got, ref, rtol, atol, what):
    """tests/test_ops_gpu.py `close` against a float64 reference: max error <= rtol max|ref| + atol.  Returns error / bound."""
    got = f64(got)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    err, b = float((got - ref).abs().max()), rtol * float(ref.abs().max()) + atol
    print(f"RATIO {what}: {err / b:.3f}")
    assert err <= b, f"{what}: max err {err:.3e} > {b:.3e}"


@pytest.mark.parametrize("act", ["leaky", "relu", "sigmoid"])
def test_activations_past_the_grid_cap(act):
    n = 2 * 2048 * 256 * 4 + 5
    assert (n + 3) // 4 > 2 * 2048 * 256                           # 2048 blocks of 256 four-element items: a third trip with the tail
    x, dy = rnd(n, seed=1, scale=20.0), rnd(n, seed=2)
    x64, dy64 = f64(x), f64(dy)
    if act == "sigmoid":
        yr = torch.sigmoid(x64)
        gr = dy64 * (1.0 - yr) * yr
    else:
        s = 0.2 if act == "leaky" else 0.0
        yr, gr = torch.where(x64 > 0, x64, s * x64), torch.where(x64 > 0, dy64, s * dy64)
    code = {"leaky": ops.ACT_LEAKY, "relu": ops.ACT_RELU, "sigmoid": ops.ACT_SIGMOID}[act]
    yg = ops.act_fwd(x.to(DEV), code, 0.2)
    dx = ops.act_bwd(dy.to(DEV), yg, code, 0.2)
    torch.cuda.synchronize()
    close64(yg, yr, 1e-6, 1e-7, f"act {act} fwd")                  # (tolerances of test_activations)
    close64(dx, gr, 1e-5, 1e-7, f"act {act} bwd")
    for got, ref, rtol in ((yg, yr, 1e-6), (dx, gr, 1e-5)):
        assert float((torch.roll(ref, 1) - ref).abs().max()) > rtol * float(ref.abs().max()) + 1e-7
        # ... and the far end really was written from its own inputs
        assert float((f64(got)[-5:] - ref[-5:]).abs().max()) <= rtol * float(ref.abs().max()) + 1e-7


@pytest.mark.parametrize("n,off", [(4194304 + 4 * 256 + 3, 4), (8388608 + 8 * 1000 + 5, 0)])
def test_adam_forms_past_the_grid_cap(n, off):
    """test_adam_forms_agree's assertions at sizes where every thread takes a second trip (4096 blocks of 256 threads: four
    parameters per trip on a range that starts 8 bytes into a plane granule, eight on an aligned one), and one step of the
    op-by-op formula of csrc/optim.hip in float64."""
    assert n // 4 > 4096 * 256 and (off % 8 != 0 or n // 8 > 4096 * 256)
    lr, b1, b2, eps, wd = 2e-4, 0.5, 0.999, 1e-8, 1e-5
    base, runs, state = T.adam_forms(n, off)
    step, bc2 = lr / (1.0 - b1 ** 1), (1.0 - b2 ** 1) ** 0.5            # dg_adam_advance at t = 1
    st = state.cpu()
    assert float(st[0]) == 1.0 and abs(float(st[1]) - step) <= 1e-15 * step and abs(float(st[2]) - bc2) <= 1e-15 * bc2
    # the kernel takes its hyper-parameters as fp32: the reference uses those values (tests/adam_ref.py), and the device's own state
    hp = hyper(b1, b2, eps, wd)
    b2f, wdf, omb1, omb2 = hp["b2"], hp["wd"], hp["omb1"], hp["omb2"]
    sl = slice(off, off + n)

    def one_step(p0, g0, m0, v0):
        return adam_one_step(p0, g0, m0, v0, hp, float(st[1]), float(st[2]))

    p0, g0, m0, v0 = (f64(t[sl]) for t in base)
    pr, mr, vr = one_step(p0, g0, m0, v0)
    pg, mg, vg = (runs[0][i][sl].cpu() for i in range(3))
    ep = (pg.double() - pr).abs()
    print(f"RATIO adam n={n} p: {float(ep.max()) / 2e-7:.3f}")
    assert float(ep.max()) <= 2e-7                                        # test_adam_flat_matches_torch's bound, same scale and hyper-parameters
    # m = m + (g' - m) (1 - b1) and g' = g + wd p cancel: four roundings relative to the reference on absolute values
    absg = g0.abs() + wdf * p0.abs()
    mabs = m0.abs() + (absg + m0.abs()) * omb1
    vabs = v0 * b2f + omb2 * absg * absg
    em, ev = (mg.double() - mr).abs(), (vg.double() - vr).abs()
    print(f"RATIO adam n={n} m: {worst(em, gamma(4) * mabs + R.TINY):.3f} (against |m| itself {worst(em, gamma(4) * mr.abs() + R.TINY):.3f}) "
          f"v: {worst(ev, gamma(4) * vabs + R.TINY):.3f}")
    assert R.exceeds(em, gamma(4) * mabs + R.TINY) == 0 and R.exceeds(ev, gamma(4) * vabs + R.TINY) == 0
    # a gradient moved by one element fails the parameter bound
    assert float((one_step(p0, torch.roll(g0, 1), m0, v0)[0] - pr).abs().max()) > 2e-7
    # shadow and planes: torch's own rounding and split, bitwise; the planes add up to the parameter exactly
    assert torch.equal(runs[1][3][sl].cpu(), pg.bfloat16())
    ref3 = split3(pg)
    assert torch.equal(runs[2][4][:, sl].cpu(), ref3)
    assert torch.equal(ref3.double().sum(0), pg.double())


def test_plane_split_past_the_grid_cap():
    n = 8388608 + 2053
    assert n // 4 > 8192 * 256 and n % 4 == 1                             # 8192 blocks of 256 four-element items, and a tail
    p = rnd(n, seed=9, scale=0.05)
    out = torch.zeros((3, (n + 7) // 8 * 8), device=DEV, dtype=torch.bfloat16)
    ops.f32_to_bf16x3(p.to(DEV), out)
    torch.cuda.synchronize()
    ref3 = split3(p)
    assert torch.equal(out[:, :n].cpu(), ref3) and not bool(out[:, n:].float().any())
    assert torch.equal(ref3.double().sum(0), p.double())
    assert not torch.equal(split3(torch.roll(p, 1)), ref3)
