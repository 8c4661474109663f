"""Sample grids, the parts that need no GPU: argument validation of dg_sample_grid_u8, the CLI surface, the PNG writer and the
rounding rule the kernel is built on."""
import ctypes as C
import os

import numpy as np
import pytest

from discogan_modernized_amd import _lib, samples
from discogan_modernized_amd import distributed_image_translation as dit
from discogan_modernized_amd import image_translation as it


def test_sample_grid_entry_point_validates_its_arguments():
    """Bad tables / shapes are refused before anything is launched (no GPU needed): negative status, message from dg_last_error."""
    L = _lib.load()
    P = C.c_void_p
    tab8 = (P * 8)(*([8] * 8))                     # non-null dummies: validation fails before they are dereferenced
    canvas = P(8)
    ok = dict(cols=6, rows=5, S=16, gap=2, bg=255)

    def call(src=tab8, canvas=canvas, **over):
        a = dict(ok, **over)
        return L.dg_sample_grid_u8(src, a["cols"], a["rows"], a["S"], a["gap"], a["bg"], canvas, None)

    assert call(src=None) == -1 and b"null pointer table" in L.dg_last_error()
    holed = (P * 8)(8, 8, None, 8, 8, 8, 8, 8)
    assert call(src=holed) == -1 and b"null batch pointer in column 2" in L.dg_last_error()
    assert call(canvas=None) == -1 and b"null canvas" in L.dg_last_error()
    for over, word in ((dict(cols=0), b"cols"), (dict(cols=9), b"cols"), (dict(rows=0), b"rows"), (dict(S=0), b"S 0"),
                       (dict(gap=-1), b"gap"), (dict(bg=256), b"bg"), (dict(bg=-1), b"bg")):
        assert call(**over) == -1, over
        assert word in L.dg_last_error(), (over, L.dg_last_error())
    # a canvas whose rows do not fit 32-bit byte offsets
    assert call(S=2 ** 30, cols=8) == -1 and b"too large" in L.dg_last_error()


GRID_MAX_BLOCKS, GRID_THREADS = 8192, 256      # csrc/export.hip, dg_sample_grid_u8: "if (g > 8192) g = 8192", 256 units per block and trip
# (rows, cols, S): 16-byte loads and scalar quads; at both the cell units alone outnumber the grid, so every gutter unit is written on a later trip
GRID_PAST_CAP = ((65, 8, 128), (8800, 8, 10))


def grid_units(rows, cols, S, gap):
    """(cell, band, strip) units of sample_grid_kernel's one index space, as dg_sample_grid_u8 counts them."""
    Wc = cols * (S + gap) + gap
    band = (rows + 1) * (gap * Wc * 3 // 4 + 2) if gap > 0 else 0
    return cols * rows * S * ((S + 3) // 4), band, rows * S * (cols + 1) if gap > 0 else 0


def test_grid_shapes_past_the_grid_cap():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "discogan_modernized_amd", "csrc", "export.hip")).read()
    assert f"if (g > {GRID_MAX_BLOCKS}) g = {GRID_MAX_BLOCKS};" in src and f"dim3({GRID_THREADS}), 0, (hipStream_t)s, a);" in src
    assert "a.band_dwords = gap > 0 ? a.band_bytes / 4 + 2 : 0;" in src and "a.n_strip = gap > 0 ? (long)rows * S * (cols + 1) : 0;" in src
    cap = GRID_MAX_BLOCKS * GRID_THREADS
    assert [grid_units(r, c, S, 3)[0] for r, c, S in GRID_PAST_CAP] == [2129920, 2112000]
    for r, c, S in GRID_PAST_CAP:
        for gap in (0, 3):
            cell, band, strip = grid_units(r, c, S, gap)
            assert cell > cap and (gap == 0) == (band + strip == 0)
    # the largest older case, the 5 x 6 grid at 512 px, stays under the cap at every gap it runs: no older test strides
    assert [sum(grid_units(5, 6, 512, gap)) for gap in (0, 2, 3)] == [1966080, 2011786, 2025766]
    assert all(sum(grid_units(r, c, S, 3)) <= cap for r, c in ((1, 1), (2, 3), (5, 6), (3, 8)) for S in (10, 16, 64, 512))


def test_parser_gains_the_test_split_flags_and_keeps_every_default():
    a = it.parse_args([])
    assert a.test_A is None and a.test_B is None
    expect = dict(device="cuda", task_name="facescrub", results_dir="./results/", models_dir="./models/",
                  model_arch="discogan", epochs=100, batch_size=64, learning_rate=0.0002, beta1=0.5, beta2=0.999,
                  image_size=64, gan_curriculum=10000, starting_rate=0.01, default_rate=0.5, style_A=None,
                  style_B=None, constraint=None, constraint_type=None, n_test=200, update_interval=3,
                  log_interval=50, image_save_interval=1000, model_save_interval=10000)
    for k, v in expect.items():
        assert getattr(a, k) == v, k
    b = it.parse_args(["--test_A", "a.pt", "--test_B", "b.pt", "--image_save_interval", "0"])
    assert (b.test_A, b.test_B, b.image_save_interval) == ("a.pt", "b.pt", 0)
    d = dit.parse_args([])
    assert d.test_A is None and d.test_B is None and d.image_save_interval == 1000


def test_load_split_is_off_without_a_split_or_with_interval_zero():
    a = it.parse_args(["--image_save_interval", "0", "--test_A", "nowhere.pt", "--test_B", "nowhere.pt"])
    assert samples.load_split(a, "tensors", "cpu") is None            # interval 0: the files are not even opened
    for kind in ("tensors", "shards", "synthetic"):
        assert samples.load_split(it.parse_args([]), kind, "cpu") is None


def test_canvas_shape_and_png_round_trip(tmp_path):
    from PIL import Image
    assert samples.canvas_shape(5, 6, 16, 2) == (92, 110, 3)
    assert samples.canvas_shape(3, 1, 10, 0) == (30, 10, 3)
    assert samples.TITLES == ("A", "B", "A->B", "B->A", "A->B->A", "B->A->B")
    canvas = np.random.default_rng(5).integers(0, 256, samples.canvas_shape(5, 6, 16, 2), dtype=np.uint8)
    path = samples.write_png(canvas, tmp_path / "samples_iter_0.png")
    with Image.open(path) as im:
        assert im.format == "PNG" and im.mode == "RGB"
        back = np.asarray(im)
    assert back.dtype == np.uint8 and np.array_equal(back, canvas)
    import torch
    samples.write_png(torch.from_numpy(canvas), tmp_path / "t.png")    # a host tensor goes the same way
    assert np.array_equal(np.asarray(Image.open(tmp_path / "t.png")), canvas)
    with pytest.raises(ValueError):
        samples.write_png(canvas.astype(np.float32), tmp_path / "bad.png")


def test_rounding_rule_inverts_the_ingest_for_all_256_values():
    """pixel = rint(fl32(k / 255) * 255) == k for every k: what makes u8 -> / 255 -> grid kernel the identity."""
    k = np.arange(256, dtype=np.float32)
    x = k / np.float32(255)
    assert x.dtype == np.float32
    assert np.array_equal(np.rint(x * np.float32(255)), k)
