"""dg_image_metrics / ops.image_metrics against float64 (tests/metrics_ref.py).

Bounds.  MSE / MAE: ``gamma(k) * ref`` with k = 6, the kernel's fp32 chain (4 terms per thread summed pairwise, + 2 for the subtraction
and the square; csrc/metrics.hip header).  SSIM: ``8 * e32 + 2^-20`` per case, e32 = the largest distance over the batch between the
plain fp32 evaluation of the formula and the float64 reference on the same inputs; the floor is a few ulp of a value <= 1.  The same
bounds tell wrong problems from the right one (test_bounds_tell_a_wrong_problem_from_the_right_one).

Worst err / bound ratios measured on an MI355X (``pytest -s`` prints them), S in {11 .. 128} x n in {1, 2, 5}:
    SSIM   indep 0.014   noisy 0.10   smooth 0.052   flat 0.007
    MSE    0.16   MAE 0.16   (all kinds; 0.18 / 0.16 on the 8200-image case past the grid caps, SSIM 0.04 there, 0.012 at 512 px)
The kernel takes its moments about a per-tile constant, so on ``flat`` (the cancellation case of sigma^2) it is far inside the plain
fp32 evaluation's error, and elsewhere its error is below the floor."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, ops  # noqa: E402
from tests import metrics_ref as MR  # noqa: E402

DEV = "cuda"
TINY = 2.0 ** -120
GRID_CAP = 8192             # METRICS_MAX_BLOCKS, csrc/metrics.hip header
TILE = 32
SIZES = (11, 12, 16, 21, 33, 42, 43, 64, 75, 128)       # 42 / 43: one window corner either side of the 32-wide tile (corners 0..S-11)
WORST = {}


def run(x, y):
    out = ops.image_metrics(x.to(DEV), y.to(DEV))
    assert out.dtype == torch.float32 and tuple(out.shape) == (x.shape[0], 3) and out.is_cuda
    return out.cpu()


def note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def check(got, x, y, what, kind=None):
    """All three columns of `got` against float64 under the module's bounds; records the worst err / bound ratios."""
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    mse, mae = MR.mse_mae_ref(x, y)
    for name, col, ref in (("MSE", 0, mse), ("MAE", 1, mae)):
        err, b = (g[:, col] - ref).abs(), MR.gamma(MR.K_CHAIN) * ref + TINY
        note(name, (err / b).max())
        print(f"{what} {name}: worst err / bound {float((err / b).max()):.3f}")
        assert bool((err <= b).all()), f"{what} {name}: err {float(err.max()):.3e} > bound, ref {ref.tolist()[:3]}"
    bound, r64 = MR.ssim_bound(x, y)
    err = (g[:, 2] - r64).abs()
    note(f"SSIM {kind}", err.max() / bound)
    print(f"{what} SSIM: max err {float(err.max()):.3e}, bound {bound:.3e}, ratio {float(err.max()) / bound:.3f}")
    assert bool((err <= bound).all()), f"{what} SSIM: err {float(err.max()):.3e} > bound {bound:.3e}"
    return bound, r64


@pytest.mark.parametrize("S", SIZES)
def test_metrics_match_float64(S):
    for n in (1, 2, 5):
        for i, kind in enumerate(MR.KINDS):
            x, y = MR.make_pair(kind, n, S, seed=1000 * S + 10 * n + i)
            check(run(x, y), x, y, f"S={S} n={n} {kind}", kind)
    print("worst err / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})


def test_identical_images():
    x, _ = MR.make_pair("indep", 3, 33, seed=5)
    got = run(x, x.clone())
    assert torch.equal(got[:, :2], torch.zeros(3, 2))
    assert float((got[:, 2].double() - 1).abs().max()) <= MR.SSIM_FLOOR


@pytest.mark.parametrize("S", [16, 64])
@pytest.mark.parametrize("kind", ["indep", "smooth"])
def test_bounds_tell_a_wrong_problem_from_the_right_one(S, kind):
    x, y = MR.make_pair(kind, 5, S, seed=77 + S)
    got = run(x, y)
    bound, _ = check(got, x, y, f"S={S} {kind}", kind)
    g = got.double()
    wrong = dict(sigma=MR.ssim_ref(x, y, sigma=1.4), window9=MR.ssim_ref(x, y, k=9), K2=MR.ssim_ref(x, y, K2=.02),
                 padded=MR.ssim_ref(x, y, pad=True), channels=MR.ssim_ref(x, torch.roll(y, 1, dims=1)),
                 shifted=MR.ssim_ref(x, torch.roll(y, 1, dims=-1)))
    for name, w in wrong.items():
        err = (g[:, 2] - w).abs()
        print(f"S={S} {kind} wrong problem {name}: max err / bound {float(err.max()) / bound:.1f}")
        assert bool((err > bound).any()), f"the SSIM bound {bound:.3e} does not tell '{name}' from the right problem"
    mse, mae = MR.mse_mae_ref(x, y, crop=1)
    for col, ref, name in ((0, mse, "MSE"), (1, mae, "MAE")):
        assert bool(((g[:, col] - ref).abs() > MR.gamma(MR.K_CHAIN) * ref + TINY).any()), f"{name}: (S-1)^2 pixels pass for S^2"


@pytest.mark.parametrize("S", [12, 43, 64])
def test_rows_are_repeatable_and_independent_of_the_batch(S):
    x, y = MR.make_pair("noisy", 5, S, seed=S)
    xd, yd = x.to(DEV), y.to(DEV)
    a = ops.image_metrics(xd, yd)
    assert torch.equal(a, ops.image_metrics(xd, yd))
    for i in range(5):
        assert torch.equal(ops.image_metrics(xd[i:i + 1], yd[i:i + 1])[0], a[i]), i
    assert torch.equal(ops.image_metrics(xd.flip(0), yd.flip(0)), a.flip(0))


@pytest.mark.parametrize("S", [16, 21])
def test_any_float_alignment_and_layout(S):
    x, y = MR.make_pair("indep", 3, S, seed=S)
    want = ops.image_metrics(x.to(DEV), y.to(DEV))
    check(want.cpu(), x, y, f"S={S} aligned", "indep")
    views = []
    for b in (x, y):
        flat = torch.empty(b.numel() + 1, device=DEV, dtype=torch.float32)
        v = flat[1:].view(b.shape)
        v.copy_(b)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        views.append(v)
    assert torch.equal(ops.image_metrics(*views), want)
    assert torch.equal(ops.image_metrics(views[0], y.to(DEV)), want)            # one batch off the 16-byte line is enough
    nc = [b.to(DEV).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2) for b in (x, y)]
    assert not nc[0].is_contiguous()
    assert torch.equal(ops.image_metrics(*nc), want)


def test_bad_inputs_raise():
    x, y = (t.to(DEV) for t in MR.make_pair("indep", 2, 16, seed=1))
    with pytest.raises(_lib.DiscoganHipError):
        ops.image_metrics(x.cpu(), y.cpu())
    with pytest.raises(_lib.DiscoganHipError):
        ops.image_metrics(x, y[:1])
    with pytest.raises(_lib.DiscoganHipError):
        ops.image_metrics(x, y[:, :, :12, :12])
    with pytest.raises(_lib.DiscoganHipError):
        ops.image_metrics(x[:, :, :10, :10], y[:, :, :10, :10])
    with pytest.raises(_lib.DiscoganHipError):
        ops.image_metrics(x.double(), y.double())


@pytest.mark.parametrize("S,pos", [(16, (1, 7, 9)), (75, (2, 40, 70)), (64, (0, 0, 63))])
def test_a_nan_stays_in_its_row(S, pos):
    x, y = MR.make_pair("noisy", 4, S, seed=3 * S)
    xd, yd = x.to(DEV), y.to(DEV)
    clean = ops.image_metrics(xd, yd)
    for j, bad in ((2, float("nan")), (0, float("inf"))):
        xb = xd.clone()
        xb[(j,) + pos] = bad
        got = ops.image_metrics(xb, yd)
        assert not bool(torch.isfinite(got[j]).any()), (bad, got[j])
        if bad != bad:
            assert bool(torch.isnan(got[j]).all())
        keep = [i for i in range(4) if i != j]
        assert torch.equal(got[keep], clean[keep])


def test_512px_against_float64():
    x, y = MR.make_pair("noisy", 2, 512, seed=512)
    check(run(x, y), x, y, "S=512 n=2 noisy", "noisy")


def test_past_both_grid_caps():
    """More work items than the tile kernel's grid and more images than the final kernel's: the stride loops of both."""
    n, S = GRID_CAP + 8, 11
    T = (S + TILE - 1) // TILE
    assert n * 3 * T * T > GRID_CAP and n > GRID_CAP
    x, y = MR.make_pair("noisy", n, S, seed=11)
    got = run(x, y)
    check(got, x, y, f"S={S} n={n} noisy", "noisy")
    sel = [0, 1, GRID_CAP - 1, GRID_CAP, n - 1]
    assert torch.equal(run(x[sel], y[sel]), got[sel])
