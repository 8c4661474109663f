"""Sliced Wasserstein distance, the parts that need no GPU: the levels table, the reference's mirror filter against scipy, the draw's
range and its independence from the other key chains, the patches-per-image rule, the CLI flags and the evaluation line."""
import os
import re

import numpy as np
import pytest
import torch

from discogan_modernized_amd import _lib, evaluate, ops
from discogan_modernized_amd import distributed_image_translation as dit
from discogan_modernized_amd import image_translation as it_cli
from tests import swd_ref as R

LEVELS = {15: [], 16: [16], 24: [24], 32: [32, 16], 34: [34, 17], 48: [48, 24], 64: [64, 32, 16], 96: [96, 48, 24],
          512: [512, 256, 128, 64, 32, 16]}


@pytest.mark.parametrize("S", sorted(LEVELS))
def test_levels_table(S):
    assert ops.swd_levels(S) == LEVELS[S] == R.levels(S)
    assert _lib.load().dg_swd_levels(S) == len(LEVELS[S])
    n = 3
    assert _lib.load().dg_lap_pyramid_elems(n, S) == sum(n * 3 * r * r for r in LEVELS[S])


def test_shapes_past_the_grid_caps_reach_every_stride_loop():
    """The launch arithmetic of dg_lap_pyramid and dg_swd_descriptors (csrc/swd.hip) at the shapes the GPU tests run past the caps, and
    the constants swd_ref copies against the source."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "discogan_modernized_amd", "csrc", "swd.hip")).read()
    assert int(re.search(r"#define SWD_PYR_MAX_BLOCKS (\d+)", src).group(1)) == R.PYR_MAX_BLOCKS
    assert int(re.search(r"#define SWD_DESC_PER_BLOCK (\d+)", src).group(1)) == R.DESC_PER_BLOCK
    assert "for (int i = threadIdx.x; i < nb; i += 256)" in src and R.SUM_THREADS == 256 and "const long b = (items + 255) / 256;" in src
    cap = R.PYR_MAX_BLOCKS * R.PYR_THREADS
    strided = [[(k, v, l, items) for k, v, l, items, _ in R.pyramid_launches(n, S) if items > cap] for n, S in R.PYRAMID_PAST_CAP]
    assert strided == [[("lap", 4, 0, 4196352)], [("down", 1, 0, 4196280), ("lap", 1, 0, 16785120)],
                       [("down", 4, 0, 4194816), ("lap", 4, 0, 16779264), ("lap", 4, 1, 4194816)]]
    for n, S in R.PYRAMID_PAST_CAP:
        assert all(items <= cap for _, _, _, items, _ in R.pyramid_launches(R.PYRAMID_CHUNK, S))      # the chunks do not stride
        sel = R.pyramid_boundary_images(n, S)
        assert 6 <= len(sel) <= 24 and sel[0] == 0 and sel[-1] == n - 1
        for _, _, _, items, per in R.pyramid_launches(n, S):
            for k in range(1, (items - 1) // cap + 1):
                assert (k * cap - 1) // per in sel and (k * cap) // per in sel
    assert R.pyramid_boundary_images(1366, 64) == [0, 1, 2, 683, 1363, 1364, 1365]
    assert all(items <= cap for S in (16, 32, 34, 36, 64, 96) for _, _, _, items, _ in R.pyramid_launches(3, S))   # the older tests: one trip
    max_row = _lib.load().dg_swd_max_row()
    assert [(-(-n * P // R.DESC_PER_BLOCK), n * P <= max_row) for n, P in R.STATS_PAST_256] == [(257, True), (1024, True)]
    assert 256 * 128 == max_row and -(-8 * 16 // R.DESC_PER_BLOCK) <= 16                   # the longest row; the older tests' 4 .. 16 partials


def test_reference_filter_is_scipy_mirror():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for shape in ((16, 16), (17, 17), (34, 34)):
        a = rng.standard_normal(shape)
        want = ndi.convolve(a, np.outer(R.W, R.W), mode="mirror")
        got = R.filt(R.filt(a, R.W, -1), R.W, -2)
        assert np.abs(got - want).max() <= 1e-14
        wrong = R.filt(R.filt(a, R.W, -1, "reflect"), R.W, -2, "reflect")
        assert np.abs(wrong - want).max() > 1e-3                    # the two border rules are not the same filter
        assert np.abs(wrong - ndi.convolve(a, np.outer(R.W, R.W), mode="reflect")).max() <= 1e-14
    # down / up: the pyramid of a constant image is zero below its last level (the filters sum to 1, and up's to 1 at every parity)
    lv = R.pyramid(np.full((1, 3, 64, 64), 0.75))
    assert [v.shape[-1] for v in lv] == [64, 32, 16]
    assert all(np.abs(v).max() <= 1e-15 for v in lv[:-1]) and np.abs(lv[-1] - 0.75).max() <= 1e-15


def _diffaug_key(seed, rank, domain, iteration, role):
    k = R.mix((seed + R.G) & R.MASK)
    k = R.mix(k ^ ((rank << 32) | domain))
    k = R.mix(k ^ iteration)
    return R.mix(k ^ (0x6469666600000000 | role))


def _augment_key(seed, rank, domain, iteration):
    k = R.mix((seed + R.G) & R.MASK)
    k = R.mix(k ^ ((rank << 32) | domain))
    return R.mix(k ^ iteration)


@pytest.mark.parametrize("Rl", [16, 17, 24, 512])
def test_draw_range_and_uniformity(Rl):
    recs = R.draw(7, 2, 40, Rl, 128)
    assert recs.min() >= 0 and recs.max() <= Rl - 7
    assert recs.min() == 0 and recs.max() == Rl - 7                  # 10240 draws over at most 506 values reach both ends
    assert not np.array_equal(recs[..., 0], recs[..., 1])
    assert abs(recs.mean() - (Rl - 7) / 2) < 0.05 * (Rl - 6)


def test_draw_keys_differ_by_seed_level_and_from_the_other_chains():
    keys = {R.level_key(s, l) for s in range(4) for l in range(6)}
    assert len(keys) == 24
    others = {_augment_key(s, 0, d, i) for s in range(4) for d in (0, 1) for i in range(6)}
    others |= {R.mix(_augment_key(s, 0, d, i) ^ 0x706F6F6C) for s in range(4) for d in (0, 1) for i in range(6)}
    others |= {_diffaug_key(s, 0, d, i, r) for s in range(4) for d in (0, 1) for i in range(6) for r in (0, 1)}
    assert not keys & others
    a, b = R.draw(0, 0, 2, 32, 16), R.draw(0, 1, 2, 32, 16)
    assert not np.array_equal(a, b) and np.array_equal(a, R.draw(0, 0, 2, 32, 16))
    assert not np.array_equal(a, R.draw(1, 0, 2, 32, 16))
    # image j, patch p is record j P + p of one sequence: a longer table starts with the shorter one only at equal P
    assert np.array_equal(R.draw(0, 0, 5, 32, 16)[:2], a)


def test_patches_rule():
    mr = ops.swd_max_row()
    assert mr == _lib.load().dg_swd_max_row() and mr in (16384, 32768)
    for n in (1, 4, 200, 256, 257, 1000, mr):
        P = ops.swd_patches(n)
        assert P == min(128, mr // n) == R.patches_per_image(n, mr) and 1 <= P and n * P <= mr
    assert ops.swd_patches(200) == (128 if mr == 32768 else 81)
    assert ops.swd_patches(mr + 1) == 0
    with pytest.raises(ValueError):
        evaluate.SWD(mr + 1, 16, "cpu")
    with pytest.raises(ValueError):
        evaluate.SWD(4, 15, "cpu")


def test_directions_are_unit_vectors_keyed_on_the_seed():
    d = evaluate.make_swd_directions(3)
    assert d.dtype == torch.float32 and tuple(d.shape) == (512, 147)
    assert np.array_equal(d.numpy(), R.directions(3)) and not np.array_equal(d.numpy(), R.directions(4))
    assert np.abs(np.linalg.norm(d.numpy().astype(np.float64), axis=1) - 1).max() <= 147 * R.U


def test_ops_refuse_cpu_tensors_and_wrong_shapes():
    E = _lib.DiscoganHipError
    with pytest.raises(E):
        ops.lap_pyramid(torch.zeros(2, 3, 16, 16))
    with pytest.raises(E):
        ops.swd_sort_rows(torch.zeros(4, 8))
    with pytest.raises(E):
        ops.swd_row_distance(torch.zeros(4, 8), torch.zeros(4, 8))
    with pytest.raises(E):
        ops.swd_project(torch.zeros(4, 147), torch.zeros(3, 2, dtype=torch.float64), torch.zeros(5, 147))
    with pytest.raises(E):
        ops.swd_descriptors(torch.zeros(2, 3, 16, 16), torch.zeros(2, 4, 2, dtype=torch.int32))
    with pytest.raises(E):
        ops.swd_draw(0, 0, 2, 16, 4, out=torch.zeros(2, 4, 2, dtype=torch.int32))
    # the library refuses bad sizes before it launches anything
    L = _lib.load()
    mr = ops.swd_max_row()
    assert L.dg_swd_sort_rows(8, 4, mr + 1, None) < 0 and b"M" in L.dg_last_error()
    assert L.dg_swd_sort_rows(8, 4, 0, None) < 0 and L.dg_swd_sort_rows(8, 0, 4, None) < 0
    assert L.dg_swd_row_distance(8, 8, 4, mr + 1, 8, None, None) < 0
    assert L.dg_swd_project(8, 8, mr + 1, 8, 4, 8, None) < 0
    assert L.dg_lap_pyramid(8, 1, 15, 8, None) < 0
    assert L.dg_swd_draw(0, 0, 1, 6, 1, 8, None) < 0


def test_cli_flags():
    a = it_cli.parse_args(["--eval_interval", "5", "--eval_swd"])
    assert a.eval_swd is True and a.eval_swd_seed == 0 and it_cli.check_eval_swd(a) is True
    d = it_cli.parse_args([])
    assert d.eval_swd is False and it_cli.check_eval_swd(d) is False
    assert dit.parse_args(["--eval_interval", "5", "--eval_swd", "--eval_swd_seed", "9"]).eval_swd_seed == 9
    bad = it_cli.parse_args(["--eval_swd", "--task_name", "edges2shoes"])
    with pytest.raises(ValueError, match="eval_interval"):
        it_cli.check_eval_swd(bad)
    with pytest.raises(ValueError, match="eval_interval"):
        it_cli.train(bad)                                          # before any device is touched
    small = it_cli.parse_args(["--eval_swd", "--eval_interval", "2", "--image_size", "12", "--task_name", "edges2shoes"])
    with pytest.raises(ValueError, match="16"):
        it_cli.train(small)
    e = evaluate.parse_args(["--model_path", "m", "--test_A", "a", "--test_B", "b", "--swd"])
    assert e.swd is True and e.swd_seed == 0
    assert evaluate.parse_args(["--model_path", "m", "--test_A", "a", "--test_B", "b"]).swd is False
    evaluate.check_size(12)
    with pytest.raises(ValueError):
        evaluate.check_size(12, swd=True)


def test_format_eval_with_and_without_swd():
    def m(v):
        return dict(n=4, mse=v, mae=v / 2, ssim=v / 3, psnr=10 * v)
    res = dict(recon_A=m(0.1), recon_B=m(0.2))
    base = evaluate.format_eval(7, res)
    assert base == ("Eval [7] RECON_PSNR: 1.000/2.000, RECON_SSIM: 0.0333/0.0667, RECON_MAE: 0.05000/0.10000 (n=4/4)")
    paired = dict(res, trans_AB=m(0.3), trans_BA=m(0.4))
    base_p = evaluate.format_eval(7, paired)
    assert base_p.startswith(base[:-len(" (n=4/4)")] + ", TRANS_PSNR: 3.000/4.000") and base_p.endswith(" (n=4/4)")
    s = dict(swd_AB=dict(levels=[1.0, 2.5], mean=1.75, n=4, patches=128), swd_BA=dict(levels=[10.0, 0.12345], mean=5.061725, n=4, patches=128))
    tail = ", SWD_AB: 1.000/2.500=1.750, SWD_BA: 10.000/0.123=5.062 (n=4/4)"
    assert evaluate.format_eval(7, dict(res, **s)) == base[:-len(" (n=4/4)")] + tail
    assert evaluate.format_eval(7, dict(paired, **s)) == base_p[:-len(" (n=4/4)")] + tail


def test_reference_chain_properties():
    """SWD(x, x) is exactly 0 and a flat channel normalises to zeros in the reference itself."""
    x = R.make_set("indep", 2, 32, 1)
    dirs = R.directions(0, 16)
    assert R.swd(x, x, 0, 8, dirs) == [0.0, 0.0]
    f = R.make_set("flat", 2, 16, 2).astype(np.float64)
    d = R.gather(f, R.draw(0, 0, 2, 16, 4))
    assert np.array_equal(R.normalise(d), np.zeros_like(d))
