"""Gradient control without a GPU: tests/clip_ref.py against ``torch.nn.utils.clip_grad_norm_`` in float64, argument validation, the
log suffix and the CLI surface."""
import math

import numpy as np
import pytest
import torch

from discogan_modernized_amd import distributed_image_translation as dit
from discogan_modernized_amd import image_translation as it
from discogan_modernized_amd import trainer as T
from tests import clip_ref

SHAPES = [(7,), (64,), (3, 43)]


def _grads(seed, mag=1.0):
    """fp32-valued gradients (what the device holds) as numpy arrays."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(s) * mag).astype(np.float32) for s in SHAPES]


def _torch_clip(grads, max_norm):
    params = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.astype(np.float64))
    total = torch.nn.utils.clip_grad_norm_(params, max_norm, error_if_nonfinite=False)
    return float(total), [p.grad.numpy() for p in params]


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("seed,mag", [(0, 1.0), (1, 1e-3), (2, 37.0)])
def test_reference_is_torchs_clip_grad_norm(seed, mag):
    grads = _grads(seed, mag)
    ss = clip_ref.sumsq(*[g.reshape(-1) for g in grads])
    nrm = clip_ref.norm(ss)
    max_norm = 0.25 * nrm                                            # clipped: the coefficient is about 1/4
    total, clipped = _torch_clip(grads, max_norm)
    assert _ulps(nrm, total) <= 2, (nrm, total)
    sc = clip_ref.scale(nrm, max_norm)
    assert 0.24 < sc < 0.26 and clip_ref.is_clipped(nrm, max_norm)
    for g, want in zip(grads, clipped):
        got = g.astype(np.float64) * np.float64(sc)
        assert (_ulps(got, want) <= 1).all()
    # pre_scale rides in front: the norm of the scaled gradient, and the factor the update multiplies by
    assert clip_ref.norm(ss, 0.5) == 0.5 * nrm
    assert clip_ref.scale(0.5 * nrm, max_norm, 0.5) == 0.5 * clip_ref.scale(0.5 * nrm, max_norm)


def test_coefficient_is_clamped_to_one_below_the_bound():
    grads = _grads(3)
    nrm = clip_ref.norm(clip_ref.sumsq(*[g.reshape(-1) for g in grads]))
    for max_norm in (2.0 * nrm, 1e30):
        total, kept = _torch_clip(grads, max_norm)
        assert clip_ref.scale(nrm, max_norm) == 1.0 and not clip_ref.is_clipped(nrm, max_norm)
        assert clip_ref.scale(nrm, max_norm, 0.5) == 0.5
        for g, k in zip(grads, kept):
            assert np.array_equal(g.astype(np.float64), k)            # torch multiplies by exactly 1
    assert clip_ref.scale(nrm, 0.0) == 1.0 and clip_ref.scale(nrm, -1.0, 0.25) == 0.25         # off
    # non-finite norms behave as torch's error_if_nonfinite=False: inf -> 0, NaN -> NaN
    assert clip_ref.scale(math.inf, 1.0) == 0.0 and math.isnan(clip_ref.scale(math.nan, 1.0))
    g = [np.array([1.0, np.inf], dtype=np.float32)]
    total, out = _torch_clip(g, 1.0)
    assert math.isinf(total) and out[0][0] == 0.0
    assert clip_ref.skip(clip_ref.sumsq(g[0]), True) and not clip_ref.skip(clip_ref.sumsq(g[0]), False)
    assert clip_ref.skip(clip_ref.sumsq(np.array([np.nan, 1.0], dtype=np.float32)), True)
    assert not clip_ref.skip(clip_ref.sumsq(np.array([3e38, 3e38], dtype=np.float32)), True)    # finite in float64


def test_control_model_counts_steps():
    c = clip_ref.Control(max_norm=1.0, guard=True)
    a = c.step([np.array([3.0, 4.0], dtype=np.float32)])
    assert a[0] == 25.0 and a[1] == 5.0 and a[2] == 1.0 / (5.0 + 1e-6) and a[3:] == [0.0, 1.0, 1.0, 0.0, 5.0]
    b = c.step([np.array([0.3], dtype=np.float32), np.array([0.4], dtype=np.float32)])
    assert b[2] == 1.0 and b[3:] == [0.0, 2.0, 1.0, 0.0, 5.0]
    d = c.step([np.array([np.nan], dtype=np.float32)])
    assert d[3:7] == [1.0, 3.0, 1.0, 1.0] and d[7] == 5.0 and math.isnan(d[1])


@pytest.mark.parametrize("bad", [-1.0, -1e-9, float("nan")])
def test_negative_grad_clip_is_refused(bad):
    with pytest.raises(ValueError, match="grad_clip"):
        T.check_grad_clip(bad)
    assert T.check_grad_clip(0) == 0.0 and T.check_grad_clip("2.5") == 2.5


def test_suffix_round_trip():
    for vals in [(1.2345e-3, 6.789e2, 3, 7, 0), (0.0, 1.0e30, 0, 1, 0), (float("nan"), float("inf"), 12, 345, 6)]:
        sfx = clip_ref.format_suffix(*vals)
        line = "Iter [3/100] GEN: 0.1/0.2, FM: 0.3/0.4, RECON: 0.5/0.6, DIS: 0.7/0.8" + sfx
        got = clip_ref.parse(line)
        assert got["head"] + sfx == line
        for k, v in zip(("norm_d", "norm_g"), vals[:2]):
            assert (math.isnan(got[k]) and math.isnan(v)) or got[k] == float(f"{v:.4e}")
        assert (got["clipped"], got["steps"], got["skipped"]) == vals[2:]
        # the trainer writes the same text
        d = dict(norm=vals[0], clipped=0, steps=1, skipped=vals[4])
        g = dict(norm=vals[1], clipped=vals[2], steps=vals[3] - 1, skipped=0)
        assert T.format_grad_suffix(d, g) == sfx
    assert clip_ref.parse("Iter [3/100] GEN: 0.1/0.2, FM: 0.3/0.4, RECON: 0.5/0.6, DIS: 0.7/0.8") is None


def test_flags_default_to_off():
    for mod in (it, dit):
        a = mod.parse_args([])
        assert a.grad_clip == 0.0 and a.nonfinite_guard is False and a.log_grad_norm is False
        b = mod.parse_args(["--grad_clip", "2.5", "--nonfinite_guard", "--log_grad_norm"])
        assert b.grad_clip == 2.5 and b.nonfinite_guard is True and b.log_grad_norm is True
    d = T.default_args()
    assert d.grad_clip == 0.0 and d.nonfinite_guard is False and d.log_grad_norm is False
