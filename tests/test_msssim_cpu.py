"""Multi-scale SSIM without a GPU: the reference of tests/msssim_ref.py against a brute-force double loop, its limits (M = 1 is the SSIM of
recon_ref, x = t, the exponents), autograd against the header's gradient formulas, the scale arithmetic and the host-side refusals, and
the DATA CONDITION the GPU bounds rest on.

Data condition.  ms = prod V_j^beta_j has derivative beta_j ms / V_j: a V_j near 0 amplifies any error in it without limit, and a V_j
whose sign the fp32 yardstick and float64 disagree on flips a channel between "alive" and "dead" (value 0, gradient 0).  The GPU
bounds (SSIM_M x the yardstick's distance from float64 + a floor) mean something only away from both, so for every GPU case this file
asserts: each float64 |V_j(i, c)| >= 5e-4, and the yardstick puts every one on the same side of 0.  Found for
``metrics_ref.make_pair(kind, n, S, 100 * S + n)`` over the four kinds: the smallest |V| is 9e-4 (indep, n 2, S 64), no sign differs;
several cases (indep and smooth) have dead channels, and smooth at n 1, S 22 has every channel dead (loss 1, gradient 0), which covers
the clamp.  One value of all cases lies under 5e-4: V_1 = -3.9e-5 of channel 0 of that all-dead case (a single window at 11 px), in a
channel that V_0 = -0.099 kills whatever V_1 is; the test pins it as the only one, and asserts what the condition is for on every
channel -- alive: every V_j >= 5e-4; dead: some V_j <= -5e-4.  If a seed is changed, re-check this condition; do not widen a bound."""
import pytest
import torch

from discogan_modernized_amd import losses, trainer
from tests import metrics_ref as MR
from tests import msssim_ref as MS
from tests import recon_ref as RR


def test_reference_against_brute_force():
    for kind in ("indep", "noisy"):
        x, t = MR.make_pair(kind, 1, 22, 7)
        want = MS.brute(x, t, 2)
        got = MS.ms_channels(x.double(), t.double(), 2)
        assert float((got - want).abs().max()) <= 1e-13, kind
        assert float((MS.per_image(x, t, 2) - want.mean(1)).abs().max()) <= 1e-13


def test_one_scale_is_the_ssim_of_the_reconstruction_loss():
    compared = []
    for kind in MR.KINDS:
        x, t = MR.make_pair(kind, 2, 24, 11)
        if float(MS.values(x.double(), t.double(), 1)[0].min()) <= 0:
            continue                                            # a clamped channel: SSIM itself has no clamp
        compared.append(kind)
        ms = MS.ms_channels(x.double(), t.double(), 1).mean()
        assert abs(float(ms) - float(RR.ssim_mean(x.double(), t.double()))) <= 1e-14, kind
        assert float((MS.per_image(x, t, 1) - MR.ssim_ref(x, t)).abs().max()) <= 1e-14, kind
        w = (0.3, 0.3, 0.4)
        assert abs(float(MS.loss_ref(x, t, 1, w)) - float(RR.loss_ref(x, t, w))) <= 1e-14
        assert float((MS.grad_ref(x, t, 1, w) - RR.grad_ref(x, t, w)).abs().max()) <= 1e-15
    assert len(compared) >= 2, compared                         # the loop above compared something


def test_identical_images_give_exactly_one_and_loss_zero():
    x, _ = MR.make_pair("indep", 2, 45, 3)
    for M in (1, 2, 3):
        for dtype in (torch.float64, torch.float32):
            assert bool((MS.per_image(x, x, M, dtype) == 1.0).all()), (M, dtype)
            assert float(MS.loss_ref(x, x, M, (0.0, 0.16, 0.84), dtype)) == 0.0


def test_exponents_sum_to_one_and_are_rounded_once():
    for M in range(1, 6):
        e = MS.exponents(M)
        assert len(e) == M and abs(sum(e) - 1.0) <= M * 2.0 ** -24
        s = sum(MS.EXPONENTS[:M])
        assert all(v == float(torch.tensor(b / s, dtype=torch.float64).float()) for v, b in zip(e, MS.EXPONENTS))
    assert MS.exponents(1) == [1.0]
    assert abs(sum(MS.exponents(3, normalise=False)) - 0.6305) < 1e-6          # the wrong problem differs


def test_autograd_equals_the_analytic_gradient():
    for n, S, M in ((1, 22, 2), (2, 23, 2), (1, 45, 3)):
        for kind in MR.KINDS:
            x, t = MR.make_pair(kind, n, S, 100 * S + n)
            for w in ((0.0, 0.0, 1.0), (0.0, 0.16, 0.84), (0.3, 0.3, 0.4)):
                a, b = MS.grad_ref(x, t, M, w, 0.7), MS.grad_analytic(x, t, M, w, 0.7)
                assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max())), (n, S, M, kind, w)


def test_scale_arithmetic():
    table = {10: 0, 11: 1, 21: 1, 22: 2, 43: 2, 44: 3, 64: 3, 87: 3, 88: 4, 175: 4, 176: 5, 512: 5, 4096: 5}
    for S, m in table.items():
        assert MS.max_scales(S) == m and losses.ms_ssim_max_scales(S) == m, S
    with pytest.raises(ValueError, match="image_size >= 11"):
        losses.ms_ssim_scales(0, 10)
    assert [losses.ms_ssim_scales(0, S) for S in (11, 22, 64, 176, 512)] == [1, 2, 3, 5, 5]
    assert losses.ms_ssim_scales(2, 64) == 2
    for bad, S in ((4, 64), (2, 21), (6, 512), (-1, 64)):
        with pytest.raises(ValueError, match="recon_ms_scales"):
            losses.ms_ssim_scales(bad, S)


def test_kinds_weights_and_host_side_refusals():
    assert losses.recon_weights("ms_ssim") == (0.0, 0.0, 1.0)
    assert losses.recon_weights("l1_ms_ssim", 0.84) == (0.0, 1.0 - 0.84, 0.84)
    assert losses.recon_weights("l1_ms_ssim") == losses.recon_weights("l1_ssim")
    assert trainer.DEFAULTS["recon_ms_scales"] == 0 and trainer.DEFAULTS["recon_loss"] == "mse"
    assert trainer.check_recon_loss("l1_ms_ssim", 0.84, 64) == (0.0, 1.0 - 0.84, 0.84)
    assert trainer.recon_ms_scales("l1_ms_ssim", 64) == 3 and trainer.recon_ms_scales("ms_ssim", 512, 4) == 4
    assert trainer.recon_ms_scales("l1_ssim", 64, 9) == 0                        # read by the multi-scale kinds only
    with pytest.raises(ValueError, match="needs image_size >= 11"):
        trainer.check_recon_loss("ms_ssim", 0.84, 10)
    with pytest.raises(ValueError, match="recon_ms_scales 4 does not fit image_size 64"):
        trainer.check_recon_loss("l1_ms_ssim", 0.84, 64, 4)
    with pytest.raises(ValueError, match="recon_ssim_alpha must be in"):
        trainer.check_recon_loss("l1_ms_ssim", 1.0, 64)
    with pytest.raises(ValueError, match="MSSSIMLoss takes"):
        losses.MSSSIMLoss("l1_ssim")
    with pytest.raises(ValueError, match="single-scale"):
        losses.ReconLoss("ms_ssim")


def test_cli_and_evaluation_surface():
    from discogan_modernized_amd import evaluate
    from discogan_modernized_amd import image_translation as it_cli
    a = it_cli.parse_args([])
    assert a.recon_loss == "mse" and a.recon_ms_scales == 0 and a.eval_ms_ssim is False
    a = it_cli.parse_args(["--recon_loss", "l1_ms_ssim", "--recon_ms_scales", "2", "--eval_ms_ssim"])
    assert (a.recon_loss, a.recon_ms_scales, a.eval_ms_ssim) == ("l1_ms_ssim", 2, True)
    rows = torch.tensor([[0.01, 0.05, 0.8, 0.9], [0.04, 0.1, 0.6, 0.7]])
    plain, more = evaluate.summarise(rows[:, :3]), evaluate.summarise(rows)
    assert "ms_ssim" not in plain and abs(more["ms_ssim"] - 0.8) < 1e-6 and {k: more[k] for k in plain} == plain
    line = evaluate.format_eval(3, dict(recon_A=plain, recon_B=plain))
    assert "MSSSIM" not in line
    line = evaluate.format_eval(3, dict(recon_A=more, recon_B=more, trans_AB=more, trans_BA=more))
    assert ", RECON_MSSSIM: 0.8000/0.8000, TRANS_MSSSIM: 0.8000/0.8000 (n=2/2)" in line
    assert ", RECON_MSSSIM: 0.8000/0.8000 (n=2/2)" in evaluate.format_eval(3, dict(recon_A=more, recon_B=more))


def test_data_condition_of_the_gpu_cases():
    smallest, dead, all_dead = None, [], []
    for n, S, M in MS.SHAPES + (MS.BELOW_MAX,):
        for kind in MS.KINDS:
            x, t = MS.make_pair(kind, n, S, 100 * S + n)
            v64 = torch.stack(MS.values(x.double(), t.double(), M))
            v32 = torch.stack(MS.values(x, t, M))
            assert bool(((v64 > 0) == (v32 > 0)).all()), (kind, n, S, M)
            gone = (v64 <= 0).any(dim=0)
            # an alive channel: every V_j >= V_MIN; a dead one: some V_j <= -V_MIN, so no fp32 error brings it back
            assert bool(torch.where(gone, (v64 <= -MS.V_MIN).any(dim=0), (v64 >= MS.V_MIN).all(dim=0)).all()), (kind, n, S, M)
            if (kind, n, S, M) == ("smooth", 1, 22, 2):
                # THE one value of all cases under V_MIN: V_1(0, 0) = -3.9e-5, one window at 11 px, in a channel V_0 = -0.099 kills anyway
                assert int((v64.abs() < MS.V_MIN).sum()) == 1 and abs(float(v64[1, 0, 0]) + 3.86e-5) < 1e-6 and float(v64[0, 0, 0]) < -0.09
                v64 = torch.cat([v64[:1].reshape(-1), v64[1].reshape(-1)[1:]])
            low = float(v64.abs().min())
            if smallest is None or low < smallest[0]:
                smallest = (low, kind, n, S, M)
            assert low >= MS.V_MIN, (kind, n, S, M, low)
            if bool(gone.any()):
                dead.append((kind, n, S, M))
            if bool(gone.all()):
                all_dead.append((kind, n, S, M))
                assert float(MS.loss_ref(x, t, M, (0.0, 0.0, 1.0))) == 1.0
                assert float(MS.grad_ref(x, t, M, (0.0, 0.0, 1.0)).abs().max()) == 0.0
    print(f"smallest |V| {smallest}; cases with dead channels {dead}; all dead {all_dead}")
    assert dead and all_dead                                       # the clamp is covered by the GPU cases


def test_shapes_past_the_caps_do_what_their_names_say():
    n, S, M = MS.TILE_PAST_CAP
    per = MS.tile_items(n, S, M)
    assert M == 2 and all(p > MS.MS_MAX_BLOCKS for p in per)        # every tile launch strides: forward, pyramid, both backward launches
    assert 3 * n > MS.FINAL_THREADS
    n, S, M = MS.FINAL_PAST_256
    assert MS.FINAL_THREADS < 3 * n <= 2 * MS.FINAL_THREADS and sum(MS.tile_items(n, S, M)) <= MS.MS_MAX_BLOCKS
    assert S % 4 != 0 and MS.TILE_PAST_CAP[1] % 8 == 0              # scalar loads here, 16-byte loads at both levels there
    x, t, at = MS.planted_pair(*MS.FINAL_PAST_256, 5)
    assert 0 in at and n - 1 in at and {85, 86} <= set(at)          # the images either side of pair 256
    assert bool((x[1] == t[1]).all()) and not bool((x[0] == t[0]).all())
