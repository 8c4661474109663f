"""The sliced Wasserstein distance kernels (csrc/swd.hip) stage by stage against tests/swd_ref.py, and evaluate.SWD as a whole.
Bounds: gamma(k) with the k counted in the header of csrc/swd.hip times the magnitude the reference computes; the whole chain against
2 eps, eps = 8 x the reference's own plain-fp32 error (tests/swd_ref.py: chain_bound).  Every test prints err / bound before it asserts."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, evaluate, ops  # noqa: E402
from tests import swd_ref as R  # noqa: E402

DEV = "cuda"
U64 = 2.0 ** -53


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- pyramid -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("S", [16, 32, 34, 36, 64, 96])
def test_pyramid_against_float64(S, n):
    x = R.make_set("mixed", n, S, seed=S + n)
    got = ops.lap_pyramid(_dev(x))
    want, bound = R.pyramid(x.astype(np.float64)), R.pyramid_bound(x)
    wrong = R.pyramid(x.astype(np.float64), "reflect")
    assert [tuple(g.shape) for g in got] == [(n, 3, r, r) for r in R.levels(S)]
    for l, (g, w, b) in enumerate(zip(got, want, bound)):
        g = g.cpu().numpy().astype(np.float64)
        err = np.abs(g - w)
        print(f"S={S} n={n} level {l}: max err {err.max():.3e}, max err/bound {(err / np.maximum(b, 1e-300)).max():.3f}")
        assert (err <= b).all()
        # the mirror rule, where it acts: the four corners and the border rows and columns
        for sl in ((..., 0, 0), (..., 0, -1), (..., -1, 0), (..., -1, -1), (..., 0, slice(None)), (..., -1, slice(None)),
                   (..., slice(None), 0), (..., slice(None), -1)):
            assert (np.abs(g[sl] - w[sl]) <= b[sl]).all()
        if len(want) > 1:                         # and an edge-repeating border is far outside the bound there
            assert np.abs(wrong[l][..., 0, 0] - w[..., 0, 0]).max() > 100 * b[..., 0, 0].max()
            assert np.abs(g[..., 0, 0] - wrong[l][..., 0, 0]).max() > 100 * b[..., 0, 0].max()
    if len(want) == 1:
        assert torch.equal(_bits(got[0]), _bits(_dev(x)))             # a one-level pyramid is a bit copy


@pytest.mark.parametrize("S", [32, 34, 64])
def test_pyramid_bits_do_not_depend_on_alignment_or_strides(S):
    x = _dev(R.make_set("indep", 3, S, seed=5))
    base = ops.lap_pyramid(x)
    buf = torch.empty(x.numel() + 1, device=DEV)
    off = buf[1:].view_as(x)
    off.copy_(x)
    assert off.data_ptr() % 16 == 4
    view = x.transpose(2, 3).contiguous().transpose(2, 3)
    assert not view.is_contiguous() and torch.equal(view, x)
    for other in (ops.lap_pyramid(off), ops.lap_pyramid(view), ops.lap_pyramid(x)):
        for a, b in zip(base, other):
            assert torch.equal(_bits(a), _bits(b))


def _pyramid_nan(x):
    """dg_lap_pyramid into a buffer that starts as NaN (ops.lap_pyramid's is uninitialised): the list of levels."""
    n, S = int(x.shape[0]), int(x.shape[3])
    L = _lib.load()
    out = torch.full((int(L.dg_lap_pyramid_elems(n, S)),), float("nan"), device=DEV)
    assert x.is_contiguous() and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    _lib.check(L.dg_lap_pyramid(x.data_ptr(), n, S, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "dg_lap_pyramid")
    levels, at = [], 0
    for r in R.levels(S):
        levels.append(out[at:at + n * 3 * r * r].view(n, 3, r, r))
        at += n * 3 * r * r
    return levels


@pytest.mark.parametrize("n,S", R.PYRAMID_PAST_CAP)
def test_pyramid_past_the_grid_cap(n, S):
    """More items than SWD_PYR_MAX_BLOCKS x 256: the stride loops of swd_lap_kernel<4> (1366 x 64), swd_lap_kernel<1> and
    swd_down_kernel<1> (4840 x 34), swd_down_kernel<4> (5462 x 64).  Every level equals, bit for bit, the pyramids of chunks of at most
    512 images (which do not stride); the first and last image and the images either side of every trip boundary are held to float64."""
    cap = R.PYR_MAX_BLOCKS * R.PYR_THREADS
    strided = {(k, v) for k, v, _, items, _ in R.pyramid_launches(n, S) if items > cap}
    assert strided == {(1366, 64): {("lap", 4)}, (4840, 34): {("lap", 1), ("down", 1)}, (5462, 64): {("lap", 4), ("down", 4)}}[(n, S)]
    assert all(items <= cap for _, _, _, items, _ in R.pyramid_launches(R.PYRAMID_CHUNK, S))
    sel = R.pyramid_boundary_images(n, S)
    assert len(sel) >= 6 and sel[0] == 0 and sel[-1] == n - 1
    x = torch.rand((n, 3, S, S), device=DEV, generator=torch.Generator(device=DEV).manual_seed(n + S))
    x[sel] = _dev(R.make_set("mixed", len(sel), S, seed=S + n))
    got = _pyramid_nan(x)
    assert [tuple(g.shape) for g in got] == [(n, 3, r, r) for r in R.levels(S)]
    for lo in range(0, n, R.PYRAMID_CHUNK):
        part = _pyramid_nan(x[lo:lo + R.PYRAMID_CHUNK])
        for l, (g, p) in enumerate(zip(got, part)):
            assert torch.equal(_bits(g[lo:lo + R.PYRAMID_CHUNK]), _bits(p)), (lo, l)
    xs = x[sel].cpu().numpy()
    want, bound = R.pyramid(xs.astype(np.float64)), R.pyramid_bound(xs)
    for l, (g, w, b) in enumerate(zip(got, want, bound)):
        err = np.abs(g[sel].cpu().numpy().astype(np.float64) - w)
        print(f"S={S} n={n} level {l}: {len(sel)} images, max err {err.max():.3e}, max err/bound {(err / np.maximum(b, 1e-300)).max():.3f}")
        assert (err <= b).all()


# ---- draw --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("P", [1, 128])
@pytest.mark.parametrize("Rl", [16, 17, 24, 512])
def test_draw_is_the_python_restatement(Rl, P, n):
    table = torch.full((n + 2, P, 2), -7, device=DEV, dtype=torch.int32)
    got = ops.swd_draw(11, 3, n, Rl, P, out=table)
    assert np.array_equal(got.cpu().numpy(), R.draw(11, 3, n, Rl, P))
    assert (table[n:] == -7).all()
    assert np.array_equal(ops.swd_draw(2 ** 64 - 1, 0, n, Rl, P).cpu().numpy(), R.draw(2 ** 64 - 1, 0, n, Rl, P))


# ---- descriptors ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _level(S=64, n=8, which=1):
    """One device level [n,3,R,R] (a Laplacian level of a 'mixed' set), shared by the tests below and never written."""
    return ops.lap_pyramid(_dev(R.make_set("mixed", n, S, seed=3)))[which].contiguous()


def _stats_check(desc, stats):
    d = desc.astype(np.float64).reshape(-1, 3, R.CH)
    N = d.shape[0] * R.CH
    mean, std = d.mean(axis=(0, 2)), d.std(axis=(0, 2))
    mag = np.abs(d).mean(axis=(0, 2))
    # fp64 sums of N terms: the mean within gamma64(N) mean|v|; the variance is a sum of N non-negative terms about a mean that is
    # itself that close, so the deviation is within gamma64(2 N + 8) (std + mean|v|)
    em, es = np.abs(stats[:, 0] - mean), np.abs(stats[:, 1] - std)
    bm, bs = R.gamma(N, U64) * mag, R.gamma(2 * N + 8, U64) * (std + mag)
    print(f"stats: mean err/bound {(em / np.maximum(bm, 1e-300)).max():.3e}, std err/bound {(es / np.maximum(bs, 1e-300)).max():.3e}")
    assert (em <= bm).all() and (es <= bs).all()


def test_descriptors_gather_bitwise_and_statistics():
    lev = _level()
    n, Rl = lev.shape[0], lev.shape[-1]
    recs = ops.swd_draw(0, 1, n, Rl, 16, device=DEV)
    recs[0, 0] = torch.tensor([0, 0])
    recs[0, 1] = torch.tensor([Rl - 7, Rl - 7])
    recs[1, 0] = torch.tensor([0, Rl - 7])
    desc, stats = ops.swd_descriptors(lev, recs)
    want = R.gather(lev.cpu().numpy(), recs.cpu().numpy())
    assert desc.dtype == torch.float32 and tuple(desc.shape) == (n * 16, 147)
    assert np.array_equal(desc.cpu().numpy().view(np.int32), want.view(np.int32))
    _stats_check(want, stats.cpu().numpy())
    again = ops.swd_descriptors(lev, recs)
    assert torch.equal(again[1], stats) and torch.equal(_bits(again[0]), _bits(desc))


def test_descriptors_clamp_hand_made_records():
    """Memory safety by construction: any int32 in a record is clamped to [0, R - 7] before it addresses anything."""
    lev = _level()
    n, Rl = lev.shape[0], lev.shape[-1]
    vals = [-1, -5, Rl - 6, Rl, 2 ** 31 - 1, -2 ** 31, 3, 0]
    recs = torch.tensor([[[vals[(j + p) % 8], vals[(j + 3 * p + 1) % 8]] for p in range(4)] for j in range(n)], device=DEV, dtype=torch.int32)
    desc, stats = ops.swd_descriptors(lev, recs)
    want = R.gather(lev.cpu().numpy(), recs.cpu().numpy())
    assert np.array_equal(desc.cpu().numpy().view(np.int32), want.view(np.int32))
    _stats_check(want, stats.cpu().numpy())


@pytest.mark.parametrize("n,P", R.STATS_PAST_256)
def test_statistics_with_more_partials_than_threads(n, P):
    """nb = ceil(M / 32) > 256 block partials: the second (at M = DG_SWD_MAX_ROW the fourth) trip of swd_sum_parts, in every block of
    swd_var_kernel and in swd_stats_kernel.  The last 32 descriptors -- the last partial, read on the last trip -- alone see a large
    offset in channel 1: leaving them out moves the float64 mean and deviation by far more than the bounds, so a missed partial
    cannot hide.  desc and stats start as NaN."""
    Rl, M = 16, n * P
    nb = -(-M // R.DESC_PER_BLOCK)
    assert nb > R.SUM_THREADS and M <= MAX_ROW and nb == {257 * 32: 257, 256 * 128: 1024}[M] and (M == MAX_ROW) == (P == 128)
    lev = R.make_set("mixed", n, Rl, seed=n + P)
    lev[-1, 1, 9:] += 100.0                                          # rows 9 .. 15 of the last image's channel 1 ...
    recs = ops.swd_draw(5, 2, n, Rl, P, device=DEV)
    last = torch.arange(M - 32, M, device=DEV)
    assert int(last[0]) // P == n - 1                                # ... which the last 32 descriptors read, and no other does
    recs[-1, :, 0] = 0
    recs.view(M, 2)[last, 0] = 9
    desc = torch.full((M, 147), float("nan"), device=DEV)
    stats = torch.full((3, 2), float("nan"), device=DEV, dtype=torch.float64)
    ops.swd_descriptors(_dev(lev), recs, desc=desc, stats=stats)
    want = R.gather(lev, recs.cpu().numpy())
    assert np.array_equal(desc.cpu().numpy().view(np.int32), want.view(np.int32))
    assert (want[:M - 32, 49:98] < 2).all() and (want[M - 32:, 49:98] > 99).all()
    st = stats.cpu().numpy()
    _stats_check(want, st)
    d = want.astype(np.float64).reshape(-1, 3, R.CH)
    N = M * R.CH
    mean, std, mag = d[:, 1].mean(), d[:, 1].std(), np.abs(d[:, 1]).mean()
    without = d[:M - 32, 1].sum() / N, np.sqrt(((d[:M - 32, 1] - mean) ** 2).sum() / N)
    print(f"n={n} P={P}: without the last partial the mean moves by {abs(without[0] - mean):.3e} (bound {R.gamma(N, U64) * mag:.3e}), "
          f"the deviation by {abs(without[1] - std):.3e} (bound {R.gamma(2 * N + 8, U64) * (std + mag):.3e})")
    assert abs(without[0] - mean) > R.gamma(N, U64) * mag and abs(without[1] - std) > R.gamma(2 * N + 8, U64) * (std + mag)


def test_flat_channel_gives_zeros():
    x = R.make_set("mixed", 2, 16, seed=9)
    x[:, 1] = 0.5                                                    # one flat channel between two live ones
    lev = _dev(x)
    recs = ops.swd_draw(0, 0, 2, 16, 8, device=DEV)
    desc, stats = ops.swd_descriptors(lev, recs)
    st = stats.cpu().numpy()
    assert st[1, 0] == 0.5 and st[1, 1] == 0.0 and st[0, 1] > 0 and st[2, 1] > 0
    dirs = np.zeros((2, 147), dtype=np.float32)
    dirs[0, 49:98] = 1.0                                             # sees the flat channel only
    dirs[1, :] = 1.0
    proj = ops.swd_project(desc, stats, _dev(dirs)).cpu().numpy()
    assert np.array_equal(proj[0].view(np.int32), np.zeros(16, dtype=np.int32))          # +0, bit for bit
    assert np.isfinite(proj[1]).all() and np.abs(proj[1]).max() > 0
    flat = _dev(R.make_set("flat", 2, 16, seed=0))
    d2, s2 = ops.swd_descriptors(flat, recs)
    assert np.array_equal(s2.cpu().numpy(), np.array([[0.25, 0], [0.5, 0], [0.75, 0]]))
    assert not ops.swd_project(d2, s2, _dev(R.directions(0, 5))).any()


# ---- projection ---------------------------------------------------------------------------------------------------------------------------
SHAPES_M = {1: (1, 1), 7: (7, 1), 128: (1, 128), 129: (3, 43), 1000: (8, 125)}


@pytest.mark.parametrize("D", [1, 5, 512])
@pytest.mark.parametrize("M", sorted(SHAPES_M))
def test_projection_against_float64(M, D):
    n, P = SHAPES_M[M]
    lev = _level()[:n].contiguous()
    recs = ops.swd_draw(1, 1, n, lev.shape[-1], P, device=DEV)
    desc, stats = ops.swd_descriptors(lev, recs)
    dirs = R.directions(0, 512)[:D]
    got = ops.swd_project(desc, stats, _dev(dirs)).cpu().numpy().astype(np.float64)
    assert got.shape == (D, M)
    d64 = desc.cpu().numpy().astype(np.float64)
    if M == 1:
        # one descriptor: per-channel std of 49 values, still live
        assert (stats.cpu().numpy()[:, 1] > 0).all()
    xhat = R.normalise(d64)
    want, bound = R.project(xhat, dirs), R.project_bound(xhat, dirs)
    err = np.abs(got - want)
    print(f"M={M} D={D}: max err {err.max():.3e}, max err/bound {(err / bound).max():.4f}")
    assert (err <= bound).all()


# ---- sort and distance ----------------------------------------------------------------------------------------------------------------------
MAX_ROW = ops.swd_max_row()


def _rows(D, M, seed):
    """[D,M] float32 on the device; row r is of kind r % 6: random, sorted, reversed, all equal, heavy duplicates, +-inf at the ends."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn((D, M), device=DEV, generator=g)
    for r in range(D):
        k = r % 6
        if k == 1:
            a[r] = torch.sort(a[r])[0]
        elif k == 2:
            a[r] = torch.sort(a[r], descending=True)[0]
        elif k == 3:
            a[r] = 1.25
        elif k == 4:
            a[r] = torch.round(a[r] * 2) / 2 + 0.0      # + 0.0: no -0 (np.sort leaves -0 / +0 in input order; the kernel puts -0 first)
        elif k == 5:
            a[r, 0] = float("inf")
            a[r, -1] = float("-inf")
    return a


@pytest.mark.parametrize("D", [1, 5, 512])
@pytest.mark.parametrize("M", [1, 2, 3, 127, 128, 129, 1000, 4097, MAX_ROW - 1, MAX_ROW])
def test_sort_and_distance(M, D):
    a, b = _rows(D, M, seed=M + D), torch.randn((D, M), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    a_np, b_np = a.cpu().numpy(), b.cpu().numpy()
    a_keep = a.clone()
    b_sorted = ops.swd_sort_rows(b.clone())
    want_b = np.sort(b_np, axis=1)
    assert np.array_equal(b_sorted.cpu().numpy().view(np.int32), want_b.view(np.int32))
    a_sorted = torch.empty_like(a)
    d1 = ops.swd_row_distance(a, b_sorted, sorted_out=a_sorted)
    assert torch.equal(_bits(a), _bits(a_keep))                                        # the input is only read
    want_a = np.sort(a_np, axis=1)
    assert np.array_equal(a_sorted.cpu().numpy().view(np.int32), want_a.view(np.int32))
    assert np.array_equal(ops.swd_sort_rows(a.clone()).cpu().numpy().view(np.int32), want_a.view(np.int32))
    got = d1.cpu().numpy()
    with np.errstate(invalid="ignore"):
        want = np.abs(want_a.astype(np.float64) - want_b.astype(np.float64)).mean(axis=1)
    fin = np.isfinite(want)
    assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any()
    err = np.abs(got[fin] - want[fin])
    bound = R.distance_gamma(M) * want[fin]
    print(f"M={M} D={D}: max err {err.max():.3e}, max err/bound {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert (err <= bound).all()
    # repeatable and symmetric, bit for bit
    assert torch.equal(ops.swd_row_distance(a, b_sorted).view(torch.int64), d1.view(torch.int64))
    d2 = ops.swd_row_distance(b, a_sorted)
    assert torch.equal(d2.view(torch.int64), d1.view(torch.int64))


def test_distance_of_inf_rows_against_themselves_is_nan_in_their_rows_only():
    a = _rows(12, 1000, seed=1)
    s = ops.swd_sort_rows(a.clone())
    d = ops.swd_row_distance(a, s).cpu().numpy()
    assert np.isnan(d[[5, 11]]).all() and not d[[0, 1, 2, 3, 4, 6, 7, 8, 9, 10]].any()          # inf - inf


def test_a_nan_poisons_its_own_row_only():
    D, M = 5, 1000
    a = torch.randn((D, M), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    b = ops.swd_sort_rows(torch.randn((D, M), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)))
    clean = ops.swd_row_distance(a, b)
    a[2, 5] = float("nan")
    a[3, 7] = -float("nan")
    srt = torch.empty_like(a)
    d = ops.swd_row_distance(a, b, sorted_out=srt)
    assert torch.isnan(d[2]) and torch.isnan(d[3])
    keep = [0, 1, 4]
    assert torch.equal(d[keep].view(torch.int64), clean[keep].view(torch.int64))
    assert torch.isnan(srt[2]).sum() == 1 and torch.isnan(srt[3]).sum() == 1 and not torch.isnan(srt[keep]).any()


def test_rows_longer_than_one_workgroup_are_refused():
    big = torch.zeros((2, MAX_ROW + 1), device=DEV)
    with pytest.raises(_lib.DiscoganHipError):
        ops.swd_sort_rows(big)
    with pytest.raises(_lib.DiscoganHipError):
        ops.swd_row_distance(big, big.clone())
    with pytest.raises(_lib.DiscoganHipError):
        ops.swd_sort_rows(torch.zeros((0, 4), device=DEV))


# ---- the whole chain --------------------------------------------------------------------------------------------------------------------------
CHAIN = [(16, 2), (32, 4), (64, 4)]
P_CHAIN = 128


@functools.lru_cache(maxsize=None)
def _chain(S, n):
    x, y = R.make_set("indep", n, S, seed=100 + S), R.make_set("mixed", n, S, seed=200 + S)
    dirs = R.directions(0)
    return x, y, dirs, R.swd(x, y, 0, P_CHAIN, dirs), R.chain_bound(x, y, 0, P_CHAIN, dirs)


@pytest.mark.parametrize("S,n", CHAIN)
def test_whole_chain_against_float64(S, n):
    """evaluate.SWD against the float64 reference, every level within 2 eps (tests/swd_ref.py: chain_bound).
    Measured on an MI355X: worst err / bound over all levels 2.2e-5 at (16, 2), 3.1e-5 at (32, 4), 1.9e-5 at (64, 4) -- errors of
    0.4e-6 to 3.0e-6 on distances of 77 to 229 against bounds of 0.039 to 0.18 (a mean over 512 x M absolute differences averages the
    projection errors the sup-norm bound adds up).  The stages below the chain: pyramid err / bound <= 0.33, projection <= 0.05,
    distance <= 0.32 (M = 1: one term, gamma(3))."""
    x, y, dirs, want, bound = _chain(S, n)
    sw = evaluate.SWD(n, S, DEV, seed=0)
    assert sw.patches == P_CHAIN and sw.M == n * P_CHAIN and sw.D == 512 and sw.sizes == R.levels(S)
    assert np.array_equal(sw.dirs.cpu().numpy(), dirs)
    sw.set_reference(_dev(x))
    res = sw.score(_dev(y))
    assert res["n"] == n and res["patches"] == P_CHAIN and len(res["levels"]) == len(want)
    for l, (g, w, b) in enumerate(zip(res["levels"], want, bound)):
        print(f"S={S} n={n} level {l}: SWD {g:.6f} ref {w:.6f} err {abs(g - w):.3e} bound {b:.3e} err/bound {abs(g - w) / b:.4f}")
    assert all(abs(g - w) <= b for g, w, b in zip(res["levels"], want, bound))
    assert res["mean"] == sum(res["levels"]) / len(res["levels"])
    assert sw.score(_dev(y)) == res                                   # the same input gives the same bits
    same = sw.score(_dev(x))
    assert same["levels"] == [0.0] * len(want) and same["mean"] == 0.0                # SWD(x, x) is exactly 0
    # symmetric in its two sets, bit for bit
    other = evaluate.SWD(n, S, DEV, seed=0).set_reference(_dev(y)).score(_dev(x))
    assert other == res
    # more images than n: the first n are scored
    more = torch.cat([_dev(y), _dev(x)])
    assert sw.score(more) == res


@pytest.mark.parametrize("variant", ["reflect", "shift", "roll", "nonorm", "fewer"])
@pytest.mark.parametrize("S,n", CHAIN[1:])
def test_the_bound_tells_a_wrong_problem_from_the_right_one(S, n, variant):
    x, y, dirs, want, bound = _chain(S, n)
    wrong = R.swd(x, y, 0, P_CHAIN, dirs, variant=variant)
    ratios = [abs(a - b) / c for a, b, c in zip(wrong, want, bound)]
    print(f"S={S} n={n} {variant}: |wrong - right| / bound per level {[f'{r:.1f}' for r in ratios]}")
    assert max(ratios) > 1
