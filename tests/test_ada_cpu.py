"""Adaptive discriminator augmentation without a GPU: the numpy gate and draw against diffaug_ref, the gate's statistics, the float64
controller reference, the trainer's check and both parsers, and the three launchers' argument checks."""
import ctypes as C
import itertools

import numpy as np
import pytest

from discogan_modernized_amd import _lib, trainer
from discogan_modernized_amd import distributed_image_translation as dit
from discogan_modernized_amd import image_translation as it
from tests import ada_ref as AR
from tests import diffaug_ref as DR

SIZES = (8, 9, 64)
KEY = (1234, 0, 6, 0, 1)              # seed, rank, iteration, domain, role


@pytest.mark.parametrize("S", SIZES)
def test_draw_p_at_one_is_the_ungated_draw_and_at_zero_all_neutral(S):
    n = 64
    for flags in range(8):
        want = DR.draw(*KEY, n, S, flags)
        assert np.array_equal(AR.draw_p(*KEY, n, S, flags, 1.0), want), flags
        zero = AR.draw_p(*KEY, n, S, flags, 0.0)
        neutral = DR.make_record()
        neutral[2:4] = S if flags & DR.CUTOUT else 0
        assert np.array_equal(zero, np.tile(neutral, (n, 1))), flags
    # the ends of float32's grid below 1: 1 - 2^-24 is the largest uniform's successor, 2^-24 keeps u = 0 only
    u = AR.gates(*KEY, 4096)
    assert u.max() < 1.0 and u.min() >= 0.0
    assert np.array_equal(AR.keep_mask(*KEY, 4096, 2.0 ** -24), u == 0.0)
    assert np.array_equal(AR.keep_mask(*KEY, 4096, 1.0 - 2.0 ** -24), u < np.float32(1.0 - 2.0 ** -24))


@pytest.mark.parametrize("S", SIZES)
def test_every_stage_is_the_ungated_draws_or_neutral(S):
    n, p = 512, 0.3
    full, got, keep = DR.draw(*KEY, n, S, DR.ALL), AR.draw_p(*KEY, n, S, DR.ALL, p), AR.keep_mask(*KEY, n, p)
    neutral = DR.make_record()
    for j in range(n):
        assert np.array_equal(got[j, 4:7], full[j, 4:7] if keep[j, 0] else neutral[4:7])
        assert np.array_equal(got[j, 0:2], full[j, 0:2] if keep[j, 1] else (0, 0))
        assert np.array_equal(got[j, 2:4], full[j, 2:4] if keep[j, 2] else (S, S))
    assert not got[:, 7].any()
    assert 0 < keep[:, 0].sum() < n and 0 < keep[:, 1].sum() < n and 0 < keep[:, 2].sum() < n
    # a stage outside the policy is neutral whatever its gate says, and the other stages do not move
    for flags in range(8):
        part = AR.draw_p(*KEY, n, S, flags, p)
        for cols, bit in (((4, 5, 6), DR.COLOR), ((0, 1), DR.TRANSLATION), ((2, 3), DR.CUTOUT)):
            for col in cols:
                assert np.array_equal(part[:, col], got[:, col] if flags & bit else np.full(n, neutral[col])), (flags, col)


def test_gate_frequency_and_independence_at_p_03():
    """n = 4096 samples x 8 iterations of one fixed seed: every stage's frequency within 5 binomial standard deviations of 0.3
    (5 sqrt(0.3 0.7 / 32768) = 0.0127), and every pair's joint frequency within the same margin of the product of the two."""
    p, n, iters = 0.3, 4096, 8
    keep = np.concatenate([AR.keep_mask(1234, 0, i, 0, 0, n, p) for i in range(iters)])
    margin = 5.0 * np.sqrt(p * (1.0 - p) / (n * iters))
    assert 0.0126 < margin < 0.0127
    freq = keep.mean(axis=0)
    print("gate frequencies", freq)
    assert np.all(np.abs(freq - p) <= margin), freq
    for a, b in itertools.combinations(range(3), 2):
        joint = np.mean(keep[:, a] & keep[:, b])
        assert abs(joint - freq[a] * freq[b]) <= margin, (a, b, joint)
    # the gate words are not the draw's words: the kept samples' fields are spread like everyone's
    u = AR.gates(1234, 0, 0, 0, 0, n)
    f = DR.factors(DR.draw(1234, 0, 0, 0, 0, n, 64, DR.ALL))
    assert abs(np.corrcoef(u[:, 0], f[:, 0])[0, 1]) < 5.0 / np.sqrt(n)
    # other keys, other gates
    base = AR.gates(1234, 0, 6, 0, 0, 256)
    for other in ((1234, 0, 6, 0, 1), (1234, 0, 6, 1, 0), (1234, 0, 7, 0, 0), (1234, 1, 6, 0, 0), (1235, 0, 6, 0, 0)):
        assert np.mean(AR.gates(*other, 256) != base) > 0.99


@pytest.mark.parametrize("S", SIZES)
def test_geometry_policy_on_p_zero_records_is_the_bitwise_identity(S):
    rng = np.random.default_rng(S)
    flags = DR.TRANSLATION | DR.CUTOUT
    recs = AR.draw_p(*KEY, 5, S, flags, 0.0)
    x = rng.integers(-2 ** 31, 2 ** 31 - 1, size=(5, 3, S, S), dtype=np.int64).astype(np.int32)      # any bit pattern
    assert np.array_equal(DR.forward(x, recs, flags), x)
    assert np.array_equal(DR.backward(x, recs, flags), x)
    xf = rng.random((5, 3, S, S), dtype=np.float32)
    recs7 = AR.draw_p(*KEY, 5, S, DR.ALL, 0.0)                                                      # neutral colour: b = 0, s = c = 1
    assert np.abs(DR.forward(xf.astype(np.float64), recs7, DR.ALL) - xf).max() <= 1e-12


def _run(windows, target, step, p_max, p0):
    ctl, acc = AR.new_ctl(p0), AR.new_acc()
    trace = []
    for batches in windows:
        for b in batches:
            AR.accumulate(acc, b, 0.0)
        AR.update(ctl, acc, target, step, p_max)
        trace.append(ctl.copy())
    return ctl, acc, trace


def test_controller_reference_moves_holds_and_clamps():
    up, down = np.ones(8, dtype=np.float32), -np.ones(8, dtype=np.float32)
    half = np.array([1, 1, 1, -1, 0, 0, 0, 0], dtype=np.float32)              # sum 2 of 8: r_t = 0.25
    step = 1.0 / 64
    ctl, acc, tr = _run([[up], [up, up], [down], [half], [], [down] * 4, [up] * 9], 0.25, step, 0.5, 0.25)
    assert np.isnan(AR.new_ctl(0.25)[1]) and AR.new_ctl(0.25)[0] == 0.25
    assert tr[0][0] == 0.25 + 8 * step and tr[0][1] == 1.0 and tr[0][4] == 8 * step                 # above: up by count x step
    assert tr[1][0] == 0.5 and tr[1][4] == 16 * step and tr[1][2] == 2 and tr[1][3] == 24            # clamps at p_max; the adjustment is unclamped
    assert tr[2][0] == 0.5 - 8 * step and tr[2][1] == -1.0 and tr[2][4] == -8 * step               # below: down
    assert tr[3][0] == tr[2][0] and tr[3][1] == 0.25 and tr[3][4] == 0.0 and tr[3][2] == 4         # equal: holds, still an update
    assert np.array_equal(tr[4], tr[3])                                                            # an empty window changes nothing
    assert tr[5][0] == 0.0 and tr[5][4] == -32 * step                                              # clamps at 0
    assert tr[6][0] == 0.5 and tr[6][3] == 8 * (1 + 2 + 1 + 1 + 4 + 9)
    assert not acc.any() and not ctl[5:].any()
    # NaN, +-0 and the threshold itself count in the window, not in the sum
    acc = AR.accumulate(AR.new_acc(), np.array([np.nan, 0.0, -0.0, 1e-45, -1e-45, np.inf, -np.inf, 2.0], dtype=np.float32), 0.0)
    assert acc.tolist() == [1.0, 8.0]
    assert AR.accumulate(AR.new_acc(), np.array([0.5, 0.4, 0.6, 0.6], dtype=np.float32), 0.5).tolist() == [1.0, 4.0]


def test_two_ranks_windows_sum_to_one_ranks_window():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(37).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    acc_a, acc_b = AR.accumulate(AR.new_acc(), a, 0.0), AR.accumulate(AR.new_acc(), b, 0.0)
    both = AR.accumulate(AR.accumulate(AR.new_acc(), a, 0.0), b, 0.0)
    assert np.array_equal(acc_a + acc_b, both) and np.array_equal(acc_b + acc_a, both)
    one = AR.update(AR.new_ctl(0.1), both.copy(), 0.6, 1e-3)
    summed = AR.update(AR.new_ctl(0.1), (acc_a + acc_b).astype(np.float32), 0.6, 1e-3)
    assert np.array_equal(one.view(np.int64), summed.view(np.int64))


def test_check_ada_ranges_and_what_it_returns():
    chk = trainer.check_ada
    assert chk(0) == (None, None) and chk(7) == (None, None) and chk(7, 1.0) == (None, None)
    assert chk(7, 0.25) == (0.25, None) and chk(7, 0.0) == (0.0, None)
    assert chk(7, None, 0.6) == (0.0, dict(target=0.6, interval=4, kimg=500.0, p_max=1.0))
    assert chk(3, 0.5, 0.6, 2, 0.1, 0.8) == (0.5, dict(target=0.6, interval=2, kimg=0.1, p_max=0.8))
    for bad in (dict(diffaug_p=-0.1), dict(diffaug_p=1.5), dict(diffaug_p=float("nan")), dict(ada_target=1.0), dict(ada_target=-0.2),
                dict(ada_target=0.6, ada_interval=0), dict(ada_target=0.6, ada_interval=2.5), dict(ada_target=0.6, ada_kimg=0.0),
                dict(ada_target=0.6, ada_p_max=0.0), dict(ada_target=0.6, ada_p_max=1.5),
                dict(ada_target=0.6, ada_interval=2 ** 12, batch=2 ** 10, world=4)):
        with pytest.raises(ValueError, match="ada_|diffaug_p"):
            chk(7, **bad)
    assert chk(7, None, 0.6, 2 ** 12, batch=2 ** 10, world=3)[1]["interval"] == 2 ** 12           # 3 x 2^22 < 2^24
    with pytest.raises(ValueError, match="needs a diffaug policy"):
        chk(0, None, 0.6)
    with pytest.raises(ValueError, match="needs a diffaug policy"):
        chk(0, 0.5)
    d = trainer.DEFAULTS
    assert (d["diffaug_p"], d["ada_target"], d["ada_interval"], d["ada_kimg"], d["ada_p_max"]) == (None, 0.0, 4, 500.0, 1.0)
    assert trainer.ada_threshold("bce") == 0.5 and trainer.ada_threshold("lsgan", 0.9) == 0.45
    assert trainer.ada_threshold("bce_logits") == 0.0 == trainer.ada_threshold("hinge")


def test_parsers_gain_the_flags_off_by_default():
    for mod in (it, dit):
        a = mod.parse_args([])
        assert (a.diffaug_p, a.ada_target, a.ada_interval, a.ada_kimg, a.ada_p_max) == (None, 0.0, 4, 500.0, 1.0)
        a = mod.parse_args(["--diffaug", "color", "--diffaug_p", "0.25", "--ada_target", "0.6", "--ada_interval", "8", "--ada_kimg", "100",
                            "--ada_p_max", "0.8"])
        assert (a.diffaug_p, a.ada_target, a.ada_interval, a.ada_kimg, a.ada_p_max) == (0.25, 0.6, 8, 100.0, 0.8)


@pytest.mark.parametrize("argv, match", [
    (["--ada_target", "0.6"], "needs a diffaug policy"),
    (["--diffaug_p", "0.5"], "needs a diffaug policy"),
    (["--diffaug", "none", "--ada_target", "0.6"], "needs a diffaug policy"),
    (["--diffaug", "color", "--diffaug_p", "1.5"], "diffaug_p"),
    (["--diffaug", "color", "--ada_target", "1.0"], "ada_target"),
    (["--diffaug", "color", "--ada_target", "0.6", "--ada_interval", "0"], "ada_interval"),
    (["--diffaug", "color", "--ada_target", "0.6", "--ada_p_max", "0"], "ada_p_max"),
    (["--diffaug", "color", "--ada_target", "0.6", "--ada_interval", "65536", "--batch_size", "256"], "2\\^24"),
])
def test_bad_flags_are_refused_before_the_device_check(argv, match):
    for mod in (it, dit):
        with pytest.raises(ValueError, match=match):
            it.train(mod.parse_args(["--task_name", "edges2shoes"] + argv))
    with pytest.raises(ValueError, match=match):                # the data-parallel entry: before the device and the process group
        dit.main(["--task_name", "edges2shoes"] + argv)


def test_launchers_refuse_bad_arguments_before_any_launch():
    """Negative status and a message, nothing launched (no GPU needed); the addresses are non-null dummies, never dereferenced."""
    lib = _lib.load()
    p = C.c_void_p
    t, prob, x, acc, ctl = p(8192), p(1 << 20), p(2 << 20), p(3 << 20), p(4 << 20)

    def err():
        return lib.dg_last_error()

    draw = lib.dg_diffaug_draw_p
    assert draw(1, 0, 0, 0, 0, 4, 64, 7, None, t, None) == -1 and b"null probability" in err()
    assert draw(1, 0, 0, 0, 0, 4, 64, 7, p((1 << 20) + 4), t, None) == -1 and b"8-byte aligned" in err()
    assert draw(1, 0, 0, 0, 0, 4, 64, 7, prob, None, None) == -1 and b"null record table" in err()
    assert draw(1, 0, 0, 0, 0, 4, 64, 7, prob, p(8196), None) == -1 and b"16-byte aligned" in err()
    assert draw(1, 0, 0, 0, 0, 0, 64, 7, prob, t, None) == -1 and b"4096" in err()
    assert draw(1, 0, 0, 0, 0, 4097, 64, 7, prob, t, None) == -1 and b"4096" in err()
    assert draw(1, 0, 0, 0, 0, 4, 1, 7, prob, t, None) == -1 and b"S" in err()
    assert draw(1, 0, 0, 0, 0, 4, 64, 8, prob, t, None) == -1 and b"flags" in err()
    assert draw(1, 0, 0, 2, 0, 4, 64, 7, prob, t, None) == -1 and b"domain" in err()
    assert draw(1, 0, 0, 0, 2, 4, 64, 7, prob, t, None) == -1 and b"role" in err()
    assert draw(1, -1, 0, 0, 0, 4, 64, 7, prob, t, None) == -1 and draw(1, 0, -1, 0, 0, 4, 64, 7, prob, t, None) == -1
    accum = lib.dg_ada_accumulate
    assert accum(None, 4, 0.0, acc, None) == -1 and b"null pointer" in err()
    assert accum(x, 4, 0.0, None, None) == -1 and b"null pointer" in err()
    assert accum(p((2 << 20) + 2), 4, 0.0, acc, None) == -1 and b"aligned" in err()
    assert accum(x, 4, 0.0, p((3 << 20) + 1), None) == -1 and b"aligned" in err()
    assert accum(x, 0, 0.0, acc, None) == -1 and b"65536" in err()
    assert accum(x, 65537, 0.0, acc, None) == -1 and b"65536" in err()
    assert accum(x, 4, float("nan"), acc, None) == -1 and b"NaN" in err()
    upd = lib.dg_ada_update
    assert upd(None, acc, 0.6, 1e-6, 1.0, None) == -1 and b"null pointer" in err()
    assert upd(ctl, None, 0.6, 1e-6, 1.0, None) == -1 and b"null pointer" in err()
    assert upd(p((4 << 20) + 4), acc, 0.6, 1e-6, 1.0, None) == -1 and b"8-byte aligned" in err()
    assert upd(ctl, p((3 << 20) + 2), 0.6, 1e-6, 1.0, None) == -1 and b"4-byte aligned" in err()
    assert upd(ctl, acc, 1.0, 1e-6, 1.0, None) == -1 and b"target" in err()
    assert upd(ctl, acc, float("nan"), 1e-6, 1.0, None) == -1 and b"target" in err()
    assert upd(ctl, acc, 0.6, -1e-6, 1.0, None) == -1 and b"step_per_image" in err()
    assert upd(ctl, acc, 0.6, float("nan"), 1.0, None) == -1 and b"step_per_image" in err()
    assert upd(ctl, acc, 0.6, 1e-6, 1.5, None) == -1 and b"p_max" in err()
    assert upd(ctl, acc, 0.6, 1e-6, -0.5, None) == -1 and b"p_max" in err()
