"""Differentiable augmentation without a GPU: the policy parser and the trainer's check, the CLI flag, the numpy reference against the
published function and against its own adjoint, the statistics of the draw with a few pinned rows, and the launchers' argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from discogan_modernized_amd import _lib, diffaug, trainer
from discogan_modernized_amd import distributed_image_translation as dit
from discogan_modernized_amd import image_translation as it
from tests import diffaug_ref as DR

SIZES = (8, 9, 64)


def test_parse_policy_accepts_subsets_in_any_order_and_refuses_unknown_names():
    c, t, k = DR.COLOR, DR.TRANSLATION, DR.CUTOUT
    assert (diffaug.POLICIES["color"], diffaug.POLICIES["translation"], diffaug.POLICIES["cutout"]) == (c, t, k) == (1, 2, 4)
    for text, flags in (("", 0), ("none", 0), (None, 0), (" ", 0), ("color", c), ("translation", t), ("cutout", k),
                        ("color,translation,cutout", 7), ("cutout,color", c | k), ("translation, cutout", t | k),
                        ("cutout,translation,color", 7), ("color,color", c)):
        assert diffaug.parse_policy(text) == flags == trainer.check_diffaug(text), text
    for bad in ("colour", "color,flip", "none,color", "color;cutout", "Color", 7, ["color"]):
        with pytest.raises(ValueError, match="diffaug"):
            diffaug.parse_policy(bad)
        with pytest.raises(ValueError, match="diffaug"):
            trainer.check_diffaug(bad)
    assert trainer.DEFAULTS["diffaug"] == ""
    assert diffaug.policy_names(7) == "color,translation,cutout" and diffaug.policy_names(4) == "cutout"


def test_parsers_gain_diffaug_off_by_default():
    for mod in (it, dit):
        assert mod.parse_args([]).diffaug == ""
        assert mod.parse_args(["--diffaug", "color,translation,cutout"]).diffaug == "color,translation,cutout"


def test_an_unknown_policy_is_refused_before_the_device_check():
    with pytest.raises(ValueError, match="unknown policy 'blur'"):
        it.train(it.parse_args(["--task_name", "edges2shoes", "--diffaug", "color,blur"]))


def test_shapes_past_the_grid_caps_reach_every_stride_loop():
    """The launch arithmetic of da_run / da_parts / da_chunk (csrc/diffaug.hip) at the shapes the GPU tests run past the caps, and the
    constants diffaug_ref copies against the source."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "discogan_modernized_amd", "csrc", "diffaug.hip")).read()
    assert int(re.search(r"#define DA_MAX_PARTS (\d+)", src).group(1)) == DR.DA_MAX_PARTS
    assert int(re.search(r"#define DA_PART_ELEMS (\d+)", src).group(1)) == DR.DA_PART_ELEMS
    assert f"cap = {DR.DA_APPLY_BLOCKS} / ((long)groups * n)" in src and "gx = (a.units + 255) / 256" in src
    assert [DR.apply_grid(g, n, S) for g, n, S in DR.APPLY_PAST_CAP] == [(5, 3), (4, 2), (4, 3), (2, 1)]
    assert [S % 4 == 0 for _, _, S in DR.APPLY_PAST_CAP] == [False, True, True, True]
    assert DR.DA_APPLY_BLOCKS // (2 * 2049) == 0                                            # the floor of one block per sample
    for g, n, S in DR.APPLY_PAST_CAP:                                                      # the chunks compared against do not stride,
        for vec in (S % 4 == 0, False):                                                    # nor in the scalar form
            want, got = DR.apply_grid(1, DR.APPLY_CHUNK, S, vec)
            assert want == got
    assert [DR.stats_partition(S) for _, S in DR.STATS_PARTITIONS] == [(4, 7500), (6, 8192), (64, 8112), (64, 8192), (64, 8272), (64, 12288)]
    assert [-(-3 * S * S // DR.DA_PART_ELEMS) for _, S in DR.STATS_PARTITIONS] == [4, 6, 64, 64, 65, 96]
    for S in SIZES + (16, 34, 40):                                                         # what the older tests reach
        assert DR.stats_partition(S)[0] <= 2 and DR.apply_grid(4, 5, S, vec=False) == (-(-S * S // 256),) * 2
    for S in (2, 9, 64, 100, 418, 420, 512, 4097):                                         # the partition covers the sample, in whole quads
        parts, chunk = DR.stats_partition(S)
        assert chunk % 4 == 0 and (parts - 1) * chunk < 3 * S * S <= parts * chunk and 1 <= parts <= DR.DA_MAX_PARTS


@pytest.mark.parametrize("S", SIZES)
def test_reference_equals_the_published_function(S):
    """float64, every subset of the policy, drawn records: 1e-12 (the two differ by a few roundings of the conjugation)."""
    rng = np.random.default_rng(S)
    x = rng.random((5, 3, S, S))
    for flags in range(8):
        recs = DR.draw(1234, 0, 6, 0, 1, 5, S, flags)
        got, want = DR.forward(x, recs, flags), DR.published(torch.from_numpy(x), recs, flags).numpy()
        assert np.abs(got - want).max() <= 1e-12, flags
        if flags == 0:
            assert np.array_equal(got, x)
    # records drawn for the whole policy, applied under a smaller one: the fields of the other stages are not read
    full = DR.draw(1234, 0, 6, 0, 1, 5, S, DR.ALL)
    for flags in range(8):
        assert np.array_equal(DR.forward(x, full, flags), DR.forward(x, DR.draw(1234, 0, 6, 0, 1, 5, S, flags), flags)), flags


@pytest.mark.parametrize("S", SIZES)
def test_reference_backward_is_the_adjoint_of_the_linear_part(S):
    """<L u, v> = <u, L^T v> in float64 to 1e-12 (relative to the products' size), L = forward minus its value at 0; drawn records and
    hand-made ones at the ends of the ranges, with the cut square clipped, outside, and with wild offsets."""
    rng = np.random.default_rng(100 + S)
    T, cs, big = DR.T_of(S), DR.cs_of(S), 2 ** 31 - 1
    hand = np.stack([DR.make_record(T, -T, -cs // 2, S - cs // 2, 0.2, 1.7, 0.6), DR.make_record(-T, T, S - 1, -cs + 1, -0.25, 0.0, 1.5),
                     DR.make_record(0, 0, S, S, 0.1, 2.0, 0.5), DR.make_record(big, -big - 1, -big - 1, big, 0.0, 0.3, 1.0),
                     DR.make_record(1, 0, big, 0, 0.0, 1.0, 1.0)])
    for recs in (DR.draw(99, 1, 4, 1, 0, 5, S, DR.ALL), hand):
        n = len(recs)
        u, v = rng.standard_normal((n, 3, S, S)), rng.standard_normal((n, 3, S, S))
        for flags in range(8):
            Lu = DR.forward(u, recs, flags) - DR.forward(np.zeros_like(u), recs, flags)
            lhs, rhs = float((Lu * v).sum()), float((u * DR.backward(v, recs, flags)).sum())
            assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (flags, lhs, rhs)


def test_reference_backward_is_autograd_through_the_published_function():
    S, n = 9, 3
    rng = np.random.default_rng(5)
    recs = DR.draw(7, 0, 2, 1, 1, n, S, DR.ALL)
    x = torch.from_numpy(rng.random((n, 3, S, S))).requires_grad_(True)
    dz = rng.standard_normal((n, 3, S, S))
    DR.published(x, recs, DR.ALL).backward(torch.from_numpy(dz))
    assert np.abs(x.grad.numpy() - DR.backward(dz, recs, DR.ALL)).max() <= 1e-12


@pytest.mark.parametrize("S", SIZES)
def test_the_draw_covers_its_ranges_and_never_leaves_them(S):
    n, T, cs = 4096, DR.T_of(S), DR.cs_of(S)
    assert (T, cs) == {8: (1, 4), 9: (1, 5), 64: (8, 32)}[S]
    recs = DR.draw(1234, 0, 6, 0, 0, n, S, DR.ALL)
    for col in (0, 1):
        assert recs[:, col].min() == -T and recs[:, col].max() == T
        assert set(np.unique(recs[:, col])) == set(range(-T, T + 1))
    count = S + 1 - cs % 2
    for col in (2, 3):
        assert set(np.unique(recs[:, col])) == set(range(-(cs // 2), count - cs // 2))
    f = DR.factors(recs)
    assert f[:, 0].min() >= -0.25 and f[:, 0].max() < 0.25 and f[:, 0].min() < -0.24 and f[:, 0].max() > 0.24
    assert f[:, 1].min() >= 0.0 and f[:, 1].max() < 2.0 and f[:, 1].min() < 0.01 and f[:, 1].max() > 1.99
    assert f[:, 2].min() >= 0.5 and f[:, 2].max() <= 1.5 and f[:, 2].min() < 0.51 and f[:, 2].max() > 1.49
    assert not recs[:, 7].any()
    assert np.array_equal(recs, DR.draw(1234, 0, 6, 0, 0, n, S, DR.ALL))
    assert np.array_equal(recs[:17], DR.draw(1234, 0, 6, 0, 0, 17, S, DR.ALL))            # a record depends on its position, not on n
    for other in (DR.draw(1234, 0, 6, 0, 1, n, S, DR.ALL), DR.draw(1234, 0, 6, 1, 0, n, S, DR.ALL), DR.draw(1234, 0, 7, 0, 0, n, S, DR.ALL),
                  DR.draw(1234, 0, 5, 0, 0, n, S, DR.ALL), DR.draw(1234, 1, 6, 0, 0, n, S, DR.ALL), DR.draw(1235, 0, 6, 0, 0, n, S, DR.ALL)):
        assert np.mean((other[:, 4:7] != recs[:, 4:7]).any(axis=1)) > 0.99                # 72 fresh bits per sample
        assert not np.array_equal(other[:, :4], recs[:, :4])
    # stages outside the policy hold their neutral values, the others are unchanged
    neutral = DR.make_record()
    for flags in range(8):
        part = DR.draw(1234, 0, 6, 0, 0, 64, S, flags)
        for cols, bit in (((4, 5, 6), DR.COLOR), ((0, 1), DR.TRANSLATION), ((2, 3), DR.CUTOUT)):
            for col in cols:
                assert np.array_equal(part[:, col], recs[:64, col] if flags & bit else np.full(64, neutral[col]))


def test_pinned_records():
    """Rows computed once from the formula in include/discogan_hip.h."""
    assert DR.draw(1234, 0, 6, 0, 0, 3, 64, 7).tolist() == [
        [6, 5, 35, -16, -1102978266, 1071873116, 1060103314, 0],
        [-7, -3, 25, 48, -1103349170, 1072000197, 1068646161, 0],
        [-3, -3, 15, 40, 1043659914, 1057025070, 1068167600, 0]]
    assert DR.draw(1234, 3, 7, 1, 1, 3, 9, 7).tolist() == [
        [1, -1, 2, -2, 1040119508, 1059808362, 1060342589, 0],
        [-1, 1, 4, -1, -1128099504, 1065190172, 1060777702, 0],
        [-1, 0, 0, 0, 1042826564, 1073211157, 1061691690, 0]]
    assert DR.draw((1 << 63) + 5, 1, (1 << 33) + 1, 1, 0, 2, 8, 6).tolist() == [
        [0, -1, 1, 5, 0, 1065353216, 1065353216, 0],
        [-1, 1, 3, -1, 0, 1065353216, 1065353216, 0]]


def test_diffaug_key_is_not_the_augmentation_or_the_pool_key():
    from tests import augment_ref as AR
    from tests import pool_ref as PR
    k = AR.mix(AR.mix(AR.mix(1234 + AR._G) ^ ((3 << 32) | 1)) ^ 7)
    assert DR.key(1234, 3, 7, 1, 0) == AR.mix(k ^ 0x6469666600000000) != DR.key(1234, 3, 7, 1, 1) == AR.mix(k ^ 0x6469666600000001)
    assert len({k, PR.key(1234, 3, 7, 1), DR.key(1234, 3, 7, 1, 0), DR.key(1234, 3, 7, 1, 1)}) == 4


def test_launchers_refuse_bad_arguments_before_any_launch():
    """Negative status and a message, nothing launched (no GPU needed); the addresses are non-null dummies, never dereferenced."""
    lib = _lib.load()
    p = C.c_void_p
    x, z, t, ws = p(1 << 20), p(2 << 20), p(8192), p(3 << 20)

    def err():
        return lib.dg_last_error()

    assert lib.dg_diffaug_workspace_bytes(4, 64, 6) == 0 and lib.dg_diffaug_workspace_bytes(4, 64, 7) == 4 * 2 * 8
    assert lib.dg_diffaug_workspace_bytes(32, 512, 1) == 32 * 64 * 8 and lib.dg_diffaug_workspace_bytes(1, 8, 1) == 8
    assert lib.dg_diffaug_draw(1, 0, 0, 0, 0, 4, 64, 7, None, None) == -1 and b"null record table" in err()
    assert lib.dg_diffaug_draw(1, 0, 0, 0, 0, 4, 64, 7, p(8196), None) == -1 and b"aligned" in err()
    assert lib.dg_diffaug_draw(1, 0, 0, 0, 0, 0, 64, 7, t, None) == -1 and b"4096" in err()
    assert lib.dg_diffaug_draw(1, 0, 0, 0, 0, 4097, 64, 7, t, None) == -1 and b"4096" in err()
    assert lib.dg_diffaug_draw(1, 0, 0, 0, 0, 4, 1, 7, t, None) == -1 and b"S" in err()
    assert lib.dg_diffaug_draw(1, 0, 0, 0, 0, 4, 64, 8, t, None) == -1 and b"flags" in err()
    assert lib.dg_diffaug_draw(1, 0, 0, 2, 0, 4, 64, 7, t, None) == -1 and b"domain" in err()
    assert lib.dg_diffaug_draw(1, 0, 0, 0, 2, 4, 64, 7, t, None) == -1 and b"role" in err()
    assert lib.dg_diffaug_draw(1, -1, 0, 0, 0, 4, 64, 7, t, None) == -1
    for f in (lib.dg_diffaug_fwd, lib.dg_diffaug_bwd):
        assert f(None, z, 4, 8, 6, t, None, 0, None) == -1 and b"null pointer" in err()
        assert f(x, z, 4, 8, 6, None, None, 0, None) == -1 and b"null pointer" in err()
        assert f(x, z, 4, 8, 6, p(8196), None, 0, None) == -1 and b"aligned" in err()
        assert f(x, z, 0, 8, 6, t, None, 0, None) == -1 and b"4096" in err()
        assert f(x, z, 4097, 8, 6, t, None, 0, None) == -1 and b"4096" in err()
        assert f(x, z, 4, 1, 6, t, None, 0, None) == -1 and b"S" in err()
        assert f(x, z, 4, 8, 16, t, None, 0, None) == -1 and b"flags" in err()
        assert f(x, z, 4, 8, 7, t, None, 0, None) == -1 and b"workspace" in err()
        assert f(x, z, 4, 8, 7, t, ws, 8, None) == -1 and b"workspace" in err()
        assert f(x, x, 4, 8, 6, t, None, 0, None) == -1 and b"overlap" in err()
        assert f(x, p((1 << 20) + 4 * 192 * 4 - 4), 4, 8, 6, t, None, 0, None) == -1 and b"overlap" in err()
    tab = (C.c_void_p * 2)
    for f in (lib.dg_diffaug_fwd_g, lib.dg_diffaug_bwd_g):
        assert f(0, tab(x, z), tab(z, x), 4, 8, 6, tab(t, t), None, 0, None) == -1 and b"groups" in err()
        assert f(5, tab(x, z), tab(z, x), 4, 8, 6, tab(t, t), None, 0, None) == -1 and b"groups" in err()
        assert f(2, tab(x, ws), tab(z, z), 4, 8, 6, tab(t, t), None, 0, None) == -1 and b"overlap" in err()        # two outputs alike
        assert f(2, tab(x, z), tab(ws, x), 4, 8, 6, tab(t, t), None, 0, None) == -1 and b"overlap" in err()        # an output on an input
        assert f(2, tab(x, None), tab(z, ws), 4, 8, 6, tab(t, t), None, 0, None) == -1 and b"null pointer" in err()
