"""Generator weight EMA, the parts that need no GPU: the CLI surface, the trainer defaults and their validation, argument validation
of dg_ema_update_flat / dg_swap_flat, and the host reference itself."""
import ctypes as C

import numpy as np
import pytest

from discogan_modernized_amd import _lib, evaluate, inference
from discogan_modernized_amd import distributed_image_translation as dit
from discogan_modernized_amd import image_translation as it
from discogan_modernized_amd import trainer as T
from tests import ema_ref


def test_training_parsers_gain_the_ema_flags_off_by_default():
    for mod in (it, dit):
        a = mod.parse_args([])
        assert a.ema_decay == 0.0 and isinstance(a.ema_decay, float)
        assert a.ema_start_iter == 0 and a.ema_samples is False
        b = mod.parse_args(["--ema_decay", "0.999", "--ema_start_iter", "500", "--ema_samples"])
        assert (b.ema_decay, b.ema_start_iter, b.ema_samples) == (0.999, 500, True)


def test_inference_and_evaluate_parsers_gain_use_ema():
    base = ["--model_path", "m", "--input_path", "x.pt"]
    assert inference.parse_args(base).use_ema is False
    assert inference.parse_args(base + ["--use_ema"]).use_ema is True
    base = ["--model_path", "m", "--test_A", "a.pt", "--test_B", "b.pt"]
    assert evaluate.parse_args(base).use_ema is False
    assert evaluate.parse_args(base + ["--use_ema"]).use_ema is True


def test_load_generator_names_the_ema_file_it_looked_for(tmp_path):
    """Nothing is there: the returned path is the file that was looked for -- same AtoB -> gen_B trap as the live files."""
    for direction, ema, reverse, name in (("AtoB", False, False, "gen_B_final.pth"), ("AtoB", True, False, "gen_B_ema_final.pth"),
                                          ("BtoA", True, False, "gen_A_ema_final.pth"), ("AtoB", True, True, "gen_A_ema_final.pth"),
                                          ("BtoA", True, True, "gen_B_ema_final.pth")):
        g, path = inference.load_generator(tmp_path, direction, 16, "cpu", reverse=reverse, ema=ema)
        assert g is None and path == tmp_path / name


def test_defaults_carry_the_ema_keys_and_bad_decays_raise():
    assert T.DEFAULTS["ema_decay"] == 0.0 and T.DEFAULTS["ema_start_iter"] == 0
    a = T.default_args()
    assert a.ema_decay == 0.0 and a.ema_start_iter == 0
    assert T.check_ema_decay(0) == 0.0 and T.check_ema_decay(0.999) == 0.999
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            T.check_ema_decay(bad)
        with pytest.raises(ValueError, match="ema_decay"):         # raised before the constructor touches a device
            T.DiscoGANTrainer(T.default_args(ema_decay=bad), device="cuda", image_size=16)


def test_entry_points_validate_their_arguments():
    """Refused before anything is launched (no GPU needed): negative status, message from dg_last_error.  The addresses are non-null
    dummies that are never dereferenced."""
    L = _lib.load()
    P = C.c_void_p
    a, b = P(4096), P(8192)

    def err():
        return L.dg_last_error()

    # ---- dg_ema_update_flat
    assert L.dg_ema_update_flat(None, b, 8, 0.5, None) == -1 and b"null pointer" in err()
    assert L.dg_ema_update_flat(a, None, 8, 0.5, None) == -1 and b"null pointer" in err()
    assert L.dg_ema_update_flat(P(20), P(16), 8, 0.5, None) == -1 and b"align" in err()
    assert L.dg_ema_update_flat(P(16), P(20), 8, 0.5, None) == -1 and b"align" in err()
    for w in (-0.1, 1.5, float("nan")):
        assert L.dg_ema_update_flat(a, b, 8, w, None) == -1, w
        assert b"outside [0, 1]" in err(), (w, err())
    assert L.dg_ema_update_flat(a, b, 0, 0.5, None) == 0
    # ---- dg_swap_flat
    assert L.dg_swap_flat(None, b, 8, None) == -1 and b"null pointer" in err()
    assert L.dg_swap_flat(a, None, 8, None) == -1 and b"null pointer" in err()
    assert L.dg_swap_flat(P(20), P(16), 8, None) == -1 and b"align" in err()
    assert L.dg_swap_flat(P(16), P(20), 8, None) == -1 and b"align" in err()
    assert L.dg_swap_flat(a, P(4096 + 16), 8, None) == -1 and b"overlap" in err()           # 4 floats apart, 8 long
    assert L.dg_swap_flat(P(4096 + 16), a, 8, None) == -1 and b"overlap" in err()
    assert L.dg_swap_flat(a, P(4096 + 16), 5, None) == -1 and b"overlap" in err()
    assert L.dg_swap_flat(a, a, 8, None) == 0                                                 # the same range: nothing to do
    assert L.dg_swap_flat(a, b, 0, None) == 0
    assert L.dg_swap_flat(a, P(4096 + 16), 0, None) == 0


def test_reference_lerp_properties():
    """What the GPU tests lean on: p == e is a fixed point for every w, w == 0 is the identity, every step is float32."""
    rng = np.random.default_rng(0)
    e = (rng.standard_normal(4099) * 0.02).astype(np.float32)
    p = (rng.standard_normal(4099) * 0.02).astype(np.float32)
    p[100:200] = e[100:200]
    for w in (float(1 - 0.999), 0.5, 0.0, 1.0):
        out = ema_ref.lerp(e, p, w)
        assert out.dtype == np.float32
        assert np.array_equal(ema_ref.bits(out[100:200]), ema_ref.bits(e[100:200]))
        # against float64: each of the three roundings is within half an ulp of its own result
        d = np.float32(p - e).astype(np.float64)
        s = (d * np.float64(np.float32(w))).astype(np.float32)
        assert np.array_equal(out, (e.astype(np.float64) + s.astype(np.float64)).astype(np.float32))
    assert np.array_equal(ema_ref.bits(ema_ref.lerp(e, p, 0.0)), ema_ref.bits(e))
    snaps = [p, e, p]
    r = ema_ref.recursion(snaps, 0.9)
    assert np.array_equal(r, ema_ref.lerp(ema_ref.lerp(p, e, np.float32(float(1.0 - 0.9))), p, np.float32(float(1.0 - 0.9))))
    assert np.array_equal(ema_ref.recursion([p], 0.9), p)
