"""Host-side halves of tests/test_reductions_gpu.py (no GPU needed): the float64 builder and merge of BatchNorm partial rows against
the float64 statistics of the data, the refusals of dg_bn_stats_from_partials, the host queries the GPU cases read their regime
from, and the discrimination of the feature-matching bounds."""
import ctypes

import pytest
import torch

from discogan_modernized_amd import _lib
from tests import shape_ref as R


@pytest.mark.parametrize("P,C,data", R.PARTIALS_CASES)
def test_partial_rows_merge_reproduces_statistics(P, C, data):
    """The rows are rounded to fp32 once; their float64 merge gives the float64 statistics of y: mean within 2^-22 (|mean| + std),
    variance within 2^-22 relative (measured: 2^-24 and 2^-22).  The GPU test's bound of 2^-20 is left a factor of four."""
    k = R.partials_case(P, C, data)
    rows, cnt, ref, got = k["rows"], k["counts"], k["ref"], k["merged"]
    assert rows.dtype == torch.float32 and rows.shape == (P, 3 * C + 4) and int(cnt[0]) > 0 and k["M"] >= 2
    empty = cnt == 0
    assert torch.isfinite(rows[~empty]).all() and torch.equal(rows[:, 0], cnt.float())
    if bool(empty.any()):
        rest = rows[empty][:, 1:]
        assert bool(torch.isnan(rest).all()) if k["sentinel"] != k["sentinel"] else bool((rest == 3e38).all())
    if P >= 3:
        assert bool(empty[-1])
    if P >= 600:
        assert bool(empty[P // 3:P // 3 + 260].all())
    sc = ref["mean"].abs() + ref["var"].sqrt()
    em, ev = (got["mean"] - ref["mean"]).abs() / sc, (got["var"] - ref["var"]).abs() / ref["var"]
    print(f"P {P} C {C} {data}: mean error / scale {float(em.max()):.3e}, var relative {float(ev.max()):.3e} (2^-22 = {R.PARTIALS_REF_TOL:.3e})")
    assert R.exceeds(em, R.PARTIALS_REF_TOL) == 0 and R.exceeds(ev, R.PARTIALS_REF_TOL) == 0
    assert R.stats_violations(got, ref, R.PARTIALS_REF_TOL) == 0
    # the bound the GPU results are held to tells every wrong merge from the right one
    assert len(k["wrong"]) == (3 if P > 2 else 1 if P == 1 else 2)
    for name, wrong in k["wrong"]:
        assert R.stats_violations(wrong, ref, R.PARTIALS_TOL) > 0, f"P {P} C {C} {data}: {name} passes the bound"


def test_partials_merge_refusals_and_workspace_rule():
    """M < 2, C = 6 and P = 0 are refused with the entry point's own words before anything is dereferenced or launched (non-null
    dummies); the two-level form's workspace exists exactly from 4096 rows and its row-block count stops at 64."""
    L = _lib.load()
    d = ctypes.c_void_p(8)
    call = lambda P, M, C: L.dg_bn_stats_from_partials(d, P, M, C, 1e-5, 0.1, d, d, d, d, None, 0, None)
    assert call(4, 1, 8) < 0 and b"Expected more than 1 value per channel when training (M=1)" in L.dg_last_error()
    assert call(4, 16, 6) < 0 and b"C=6 must be a multiple of 4" in L.dg_last_error()
    assert call(0, 16, 8) < 0 and b"dg_bn_stats_from_partials: bad argument" in L.dg_last_error()
    for P in (1, 257, 4095, 4096, 4097, 33000, 1 << 20):
        for C in (4, 12, 100, 192):
            b = L.dg_bn_partials_workspace_bytes(P, C)
            assert (b > 0) == (P >= R.PARTIALS_TWO_LEVEL_FROM), (P, C, b)
            if b:
                assert b == min(max(P // 512, 2), 64) * 2 * C * 8, (P, C, b)


def test_capped_grid_arithmetic():
    assert R.capped_grid(1, 1024) == (1, 1) and R.capped_grid(256 * 1024, 1024) == (1024, 1)
    assert R.capped_grid(256 * 1024 + 1, 1024) == (1024, 2) and R.capped_grid(300001, 1024) == (1024, 2)


@pytest.mark.parametrize("N", [9, 260])
def test_feature_matching_bounds_discriminate(N):
    """An fp32 evaluation (chunked the way the kernel chunks the batch) stays inside the diff and loss bounds; the float64 references
    of the wrong problems -- the last image left out of one mean, real and fake exchanged in one chunk's worth of images -- do not."""
    real, fake = R.rnd(N, 32, 4, 4, seed=1), R.rnd(N, 32, 4, 4, seed=2)
    ref = R.fm_ref(real, fake)
    b, lb = R.fm_diff_bound(ref), R.fm_loss_bound(ref, 4)
    chunks = lambda t: sum(c.sum(0) for c in t.split(5)) * (torch.tensor(1.0) / N)
    d32 = chunks(real) - chunks(fake)
    assert R.exceeds((R.f64(d32) - ref["diff"]).abs(), b) == 0
    assert abs(float((R.f64(d32) ** 2).mean()) - float(ref["loss"])) <= lb
    for wrong in (R.fm_ref(real, fake, drop_last=True), R.fm_ref(real, fake, swap=5)):
        assert R.exceeds((wrong["diff"] - ref["diff"]).abs(), b) > 0
        assert abs(float(wrong["loss"]) - float(ref["loss"])) > lb
