"""Training augmentation, the parts that need no GPU: the CLI surface and the L rule, the numpy draw's statistics (the device draw is
compared with it exactly in test_augment_gpu.py), the reference image's own definition, and the launchers' argument checks."""
import ctypes as C

import numpy as np
import pytest

from discogan_modernized_amd import _lib
from discogan_modernized_amd import dataset as ds
from discogan_modernized_amd import distributed_image_translation as dit
from discogan_modernized_amd import image_translation as it
from oracle import image_prep_ref as R
from tests import augment_ref as AR

S, L, N = 16, 24, 4096


def test_parsers_gain_the_augment_flags_off_by_default():
    for mod in (it, dit):
        a = mod.parse_args([])
        assert a.augment == "" and a.augment_scale == 1.125
        assert it.augment_of(a) is None
        b = mod.parse_args(["--augment", "flip,crop", "--augment_scale", "1.5", "--image_size", "16", "--seed", "7"])
        rec = it.augment_of(b, rank=3)
        assert rec == ds.Augment(seed=7, rank=3, flags=3, scale=1.5, first_iteration=0) and rec.size(16) == 24


def test_flag_parsing_and_the_L_rule():
    assert ds.parse_augment("") == 0 and ds.parse_augment(None) == 0
    assert ds.parse_augment("flip") == AR.FLIP and ds.parse_augment("crop") == AR.CROP
    assert ds.parse_augment("flip,crop") == ds.parse_augment(" crop , flip ") == AR.FLIP | AR.CROP
    assert ds.augment_name(3) == "flip,crop" and ds.augment_name(0) == "off"
    with pytest.raises(ValueError, match="cutout"):
        ds.parse_augment("flip,cutout")
    assert ds.augment_size(64, AR.CROP) == 72 and ds.augment_size(64, AR.FLIP | AR.CROP, 1.125) == 72
    assert ds.augment_size(256, AR.CROP, 286 / 256) == 286 and ds.augment_size(16, AR.CROP, 1.5) == 24
    assert ds.augment_size(64, AR.FLIP) == 64 and ds.augment_size(64, 0) == 64         # no crop: L = S
    assert ds.augment_size(16, AR.CROP, 1.0) == 16
    for bad in (0.99, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="augment_scale"):
            ds.augment_size(64, AR.CROP, bad)
    with pytest.raises(ValueError, match="augment_scale"):
        it.augment_of(it.parse_args(["--augment", "crop", "--augment_scale", "0.9"]))
    with pytest.raises(ValueError, match="rotate"):
        it.augment_of(it.parse_args(["--augment", "rotate"]))


def test_draw_statistics():
    """Bounds from the binomial, not from the generator: 4096 fair coins have sd 32, so [1856, 2240] is 6 sd; each of the 9 offsets expects
    455 with sd ~20, so 300 is more than 7 sd below."""
    t = AR.draw(1234, 0, 5, 0, N, S, L, AR.FLIP | AR.CROP)
    assert t.dtype == np.int32 and t.shape == (N, 4) and not t[:, 3].any()
    assert 1856 <= int(t[:, 2].sum()) <= 2240 and set(np.unique(t[:, 2])) == {0, 1}
    for col in (0, 1):
        counts = np.bincount(t[:, col], minlength=L - S + 1)
        assert len(counts) == L - S + 1 and counts.min() >= 300, (col, counts)
    assert not np.array_equal(t[:, 0], t[:, 1])
    assert np.array_equal(t, AR.draw(1234, 0, 5, 0, N, S, L, AR.FLIP | AR.CROP))       # a pure function of its key
    assert np.array_equal(t[:100], AR.draw(1234, 0, 5, 0, 100, S, L, AR.FLIP | AR.CROP))   # position j does not depend on n


def test_draw_differs_by_domain_iteration_rank_and_seed():
    base = AR.draw(1234, 0, 5, 0, N, S, L, 3)
    for other in (AR.draw(1234, 0, 5, 1, N, S, L, 3), AR.draw(1234, 0, 6, 0, N, S, L, 3), AR.draw(1234, 1, 5, 0, N, S, L, 3),
                  AR.draw(1235, 0, 5, 0, N, S, L, 3)):
        for col in range(3):                              # as different as two independent sequences: nowhere near equal column by column
            assert (base[:, col] != other[:, col]).mean() > 0.4, col


def test_flags_switch_the_parts_off():
    crop_off = AR.draw(1234, 0, 5, 0, N, S, L, AR.FLIP)
    assert not crop_off[:, :2].any() and crop_off[:, 2].any()
    flip_off = AR.draw(1234, 0, 5, 0, N, S, L, AR.CROP)
    assert not flip_off[:, 2].any() and flip_off[:, :2].any()
    assert not AR.draw(1234, 0, 5, 0, N, S, L, 0).any()
    both = AR.draw(1234, 0, 5, 0, N, S, L, 3)              # a flag masks its part and leaves the other part's words alone
    assert np.array_equal(both[:, 2], crop_off[:, 2]) and np.array_equal(both[:, :2], flip_off[:, :2])


def test_reference_image_is_the_sliced_flipped_preparation():
    img = np.random.default_rng(2).integers(0, 256, (20, 24, 3), dtype=np.uint8)
    full = R.prepare_image(img, None, 18)
    assert np.array_equal(AR.augment_image(img, None, 16, 18, 0, 0, 0), full[:, :16, :16])
    assert np.array_equal(AR.augment_image(img, None, 16, 18, 2, 1, 1), full[:, 1:17, 2:18][:, :, ::-1])
    assert np.array_equal(AR.augment_image(img, None, 16, 16, 0, 0, 0), R.prepare_image(img, None, 16))
    recs = AR.corner_records(16, 24)
    assert recs[:, :2].max() == 8 and recs[:, :2].min() == 0 and set(recs[:, 2]) == {0, 1}


def test_launchers_refuse_bad_arguments_before_any_launch():
    """Negative status and a message, nothing launched (no GPU needed); the addresses are non-null dummies, never dereferenced."""
    lib = _lib.load()
    P = C.c_void_p
    a, b, t = P(4096), P(1 << 20), P(8192)

    def err():
        return lib.dg_last_error()

    assert lib.dg_augment_draw(1, 0, 0, 0, 4, 16, 12, 3, t, None) == -1 and b"smaller than" in err()
    assert lib.dg_augment_draw(1, 0, 0, 0, 4, 16, 24, 3, None, None) == -1 and b"null record table" in err()
    assert lib.dg_augment_draw(1, 0, 0, 0, 4, 0, 24, 3, t, None) == -1
    assert lib.dg_augment_draw(1, 0, 0, 2, 4, 16, 24, 3, t, None) == -1 and b"domain" in err()
    assert lib.dg_augment_draw(1, 0, 0, 0, 4, 16, 24, 4, t, None) == -1 and b"flags" in err()
    assert lib.dg_augment_draw(1, 0, 0, 0, 4, 16, 24, 3, P(8196), None) == -1 and b"aligned" in err()
    assert lib.dg_augment_draw(1, 0, 0, 0, 0, 16, 24, 3, t, None) == 0                                  # nothing to draw
    assert lib.dg_image_prep_aug(a, b, 2, 8, 8, 0, 8, 0, 1, 16, 12, t, None, None) == -1 and b"smaller than" in err()
    assert lib.dg_image_prep_aug(a, b, 2, 8, 8, 0, 8, 0, 1, 16, 24, None, None, None) == -1 and b"null record table" in err()
    assert lib.dg_image_prep_aug(a, b, 2, 8, 8, 0, 8, 0, 1, 0, 24, t, None, None) == -1
    assert lib.dg_image_prep_aug(a, b, 2, 8, 8, 4, 8, 0, 1, 16, 24, t, None, None) == -1 and b"outside the 8-pixel rows" in err()
    assert lib.dg_image_prep_aug(a, b, 2, 8, 8, 0, 8, 0, 2, 16, 24, t, None, None) == -1 and b"mode" in err()
    assert lib.dg_augment_f32(a, b, 2, 16, 12, t, None) == -1 and b"smaller than" in err()
    assert lib.dg_augment_f32(a, b, 2, 16, 24, None, None) == -1 and b"null record table" in err()
    assert lib.dg_augment_f32(a, b, 2, 0, 24, t, None) == -1
    assert lib.dg_augment_f32(a, a, 2, 16, 24, t, None) == -1 and b"overlap" in err()
