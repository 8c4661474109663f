"""Host-side halves of tests/test_layout_ingest_gpu.py (no GPU needed): what the four entry points -- dg_nchw_to_nhwc,
dg_nhwc_to_nchw, dg_u8hwc_to_f32chw, dg_image_prep -- refuse before any launch, the agreement of tests/ingest_ref.py's composition
with the oracle, and the proof that every wrong problem of the GPU file differs from its right problem under the comparison used
there, so that no discrimination claim rests on a GPU run."""
import ctypes

import numpy as np
import pytest

from discogan_modernized_amd import _lib
from oracle import image_prep_ref as R
from tests import ingest_ref as I

INVALID = -1                                               # DG_ERR_INVALID


def _refused(rc, *needles):
    assert rc == INVALID, rc
    msg = _lib.load().dg_last_error()
    for n in needles:
        assert n in msg, (n, msg)


# ==== 1. refusals that return before any launch (non-null dummies are never dereferenced) ===============================
@pytest.mark.parametrize("entry", ["dg_nchw_to_nhwc", "dg_nhwc_to_nchw"])
def test_layout_entries_refuse_bad_arguments(entry):
    """Nulls, empty dimensions, N past grid.z, and the grid rules of launch_transpose: one image's C*H*W must fit an int, and its
    ceil(C/32) * ceil(H*W/32) tiles, which lie along grid.x, must keep grid.x * 256 threads under 2^32."""
    fn = getattr(_lib.load(), entry)
    d = ctypes.c_void_p(64)
    for x, y, N, C, H, W in ((None, d, 1, 4, 4, 4), (d, None, 1, 4, 4, 4), (d, d, 0, 4, 4, 4), (d, d, 1, 0, 4, 4), (d, d, 1, 4, 0, 4),
                             (d, d, 1, 4, 4, 0), (d, d, -1, 4, 4, 4), (d, d, 65536, 4, 4, 4)):
        _refused(fn(x, y, N, C, H, W, None), entry.encode(), b"bad argument")
    # H*W alone past an int; C*H*W past an int; 2^30 single-channel pixels = 2^25 tiles
    for C, H, W in ((1, 46341, 46341), (1, 65536, 65536), (3, 32768, 32768), (2147483647, 2, 1)):
        _refused(fn(d, d, 1, C, H, W, None), entry.encode(), b"2^31 - 1")
    assert (1 << 30) // I.TILE > I.transpose_max_tiles() == (1 << 32) // I.BLOCK - 1
    for C, H, W in ((1, 32768, 32768), (1 << 30, 1, 1), (1, 1, 32 * I.transpose_max_tiles() + 1)):
        _refused(fn(d, d, 1, C, H, W, None), entry.encode(), b"tiles of 32 x 32")


def test_byte_ingest_refuses_bad_arguments():
    fn = _lib.load().dg_u8hwc_to_f32chw
    d = ctypes.c_void_p(64)
    for src, dst, N, H, W in ((None, d, 1, 4, 4), (d, None, 1, 4, 4), (d, d, 0, 4, 4), (d, d, 1, 0, 4), (d, d, 1, 4, 0), (d, d, 1, 3, 3),
                              (d, d, 2, 1, 2), (d, d, 1, 5, 7), (d, d, 1, 2, 3)):
        for bgr in (0, 1):
            _refused(fn(src, dst, N, H, W, bgr, None), b"dg_u8hwc_to_f32chw", b"multiple of 4")


def test_image_prep_refuses_bad_arguments():
    fn = _lib.load().dg_image_prep
    d = ctypes.c_void_p(64)
    ok = dict(src=d, dst=d, N=2, H=8, W=10, x0=1, cw=5, erode=0, mode=1, S=4)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["src"], a["dst"], a["N"], a["H"], a["W"], a["x0"], a["cw"], a["erode"], a["mode"], a["S"], None)

    for kw in (dict(src=None), dict(dst=None), dict(N=0), dict(H=0), dict(W=0), dict(S=0), dict(N=-3)):
        _refused(call(**kw), b"dg_image_prep: bad argument")
    for kw in (dict(x0=-1), dict(cw=0), dict(x0=6), dict(x0=0, cw=11), dict(x0=10, cw=1), dict(cw=-2)):
        _refused(call(**kw), b"outside the 10-pixel rows")
    for kw in (dict(mode=2), dict(mode=-1), dict(mode=3, erode=1)):
        _refused(call(**kw), b"mode 0 (float) or 1")


# ==== 2. the constants the GPU file asserts its regimes from =============================================================
def test_launch_constants_and_regimes():
    """The caps the GPU cases are sized against, read from the launchers, and each case on the side of its threshold it is meant
    for."""
    assert I.launcher_cap("misc.hip", "dg_u8hwc_to_f32chw") == 4096
    assert I.launcher_cap("ingest.hip", "dg_image_prep") == 8192
    N, H, W = I.U8_BIG
    assert N * H * W // 4 > I.launcher_cap("misc.hip", "dg_u8hwc_to_f32chw") * I.BLOCK
    g = I.PREP_BIG
    assert g["N"] * g["S"] ** 2 > I.launcher_cap("ingest.hip", "dg_image_prep") * I.BLOCK
    for N, C, H, W in I.BIG_PLANES:
        tiles_r, tiles_c = -(-H * W // I.TILE), -(-C // I.TILE)
        assert tiles_r > I.OLD_GRID_Y_LIMIT and (H * W - 1) // I.TILE <= I.OLD_GRID_Y_LIMIT + 100     # just past the old limit
        assert tiles_r * tiles_c <= I.transpose_max_tiles()
    for N, H, W in I.U8_SHAPES:
        assert H * W % 4 == 0
    assert any(W % 4 != 0 for _, _, W in I.U8_SHAPES)                  # quads that straddle two rows
    for H, W, x0, cw, S in I.PREP_ABI_CASES:
        assert 0 <= x0 and x0 + cw <= W and H != cw
    assert {(x0 % 2, cw == 1, cw == W, x0 + cw == W and x0 > 0) for _, W, x0, cw, _ in I.PREP_ABI_CASES} >= {
        (1, False, False, False), (1, True, False, False), (0, False, True, False), (1, False, False, True)}


def test_byte_sweep_puts_every_value_in_every_position():
    """(4, 16, 16): all 256 byte values in each of the 12 byte positions of a pixel quad; (1, 16, 16) alone reaches 64 per
    position -- all 256 in every CHANNEL, a quarter of them in every position."""
    for shape, per_position in (((4, 16, 16), 256), ((1, 16, 16), 64)):
        src = I.u8_source(shape)
        quads = src.reshape(-1, 12)
        for j in range(12):
            assert len(np.unique(quads[:, j])) == per_position, (shape, j)
        for c in range(3):
            assert len(np.unique(src[0, :, :, c])) == 256


# ==== 3. tests/ingest_ref.py against the oracle =============================================================================
@pytest.mark.parametrize("domain,x0,cw,erode,mode", [("A", 0, 256, 1, 0), ("B", 256, 256, 0, 1), (None, 0, 512, 0, 1)])
@pytest.mark.parametrize("S", [64, 100])
def test_prep_ref_is_the_oracle_on_the_three_domains(domain, x0, cw, erode, mode, S):
    src = I.prep_source(2, 40, 512, seed=3)
    assert np.array_equal(I.bits(I.prep_ref(src, x0, cw, erode, mode, S)), I.bits(R.read_images(list(src), domain, S)))


def test_border_expectation_is_the_oracle_and_the_leak_is_not():
    """The hand-written expectation of the erosion border rule equals the oracle's composition in both modes (an identity-size
    resize is exact in both), and eroding before the crop gives another image: black first and last columns."""
    g, src, want = I.BORDER, I.border_source(), I.border_expected()
    assert g["S"] == g["cw"] == g["H"] and g["x0"] % 2 == 1
    assert np.all(src[:, :, g["x0"] - 1] == 0) and np.all(src[:, :, g["x0"] + g["cw"]] == 0)
    assert np.all(want[0, :, :, 0] == 1.0) and np.all(want[0, :, :, -1] == 1.0) and np.all(want[1, :, 2:-2, (0, -1)] == 1.0)
    assert int((want[0, 0] == 0).sum()) == 25 and int((want[1, 0] == 0).sum()) == 16
    for mode in (0, 1):
        assert np.array_equal(I.bits(I.prep_ref(src, g["x0"], g["cw"], 1, mode, g["S"])), I.bits(want))
        leak = I.prep_leaky_ref(src, g["x0"], g["cw"], mode, g["S"])
        assert np.all(leak[:, :, :, 0] == 0.0) and np.all(leak[:, :, :, -1] == 0.0)
        assert I.rejected(mode, leak, want)
        for name, wrong in I.prep_wrongs(src, g["x0"], g["cw"], 1, mode, g["S"]).items():
            assert I.rejected(mode, wrong, want), (mode, name)


# ==== 4. every wrong problem differs from its right problem ==================================================================
@pytest.mark.parametrize("direction", I.DIRECTIONS)
@pytest.mark.parametrize("shape", I.LAYOUT_SHAPES + I.BIG_PLANES)
def test_layout_wrong_problems_differ(direction, shape):
    src, want = I.layout_problem(direction, shape)
    assert len(np.unique(src)) == src.size and I.SENTINEL not in src and I.GUARD not in src
    assert np.isin(np.array(I.SPECIALS[:src.size], dtype=np.uint32).view(np.int32), src).all()
    assert np.isnan(src.view(np.float32)).sum() == min(2, src.size)
    wrongs = I.layout_wrongs(direction, shape, src)
    assert wrongs, shape
    for name, wrong in wrongs.items():
        assert wrong.shape == want.shape and not np.array_equal(wrong, want), (shape, name)
    # what is left out is left out because it IS the right problem: nothing a comparison could tell apart
    N, C, H, W = shape
    assert ("hw_swapped" in wrongs) == (H != W and min(H, W) > 1)
    assert ("other_direction" in wrongs) == (C > 1 and H * W > 1 and C != H * W)
    if C == 1 or H * W == 1:
        assert np.array_equal(want, src)                               # this direction, like the other, is the identity
    if C == H * W:                                                     # both directions transpose the same square matrix per image
        assert np.array_equal(want, src.reshape(N, C, C).transpose(0, 2, 1).reshape(-1))
    if min(H, W) == 1 and H != W:
        assert np.array_equal(I.layout_problem(direction, (N, C, W, H))[1], want)      # same payload, H and W exchanged


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("shape", I.U8_SHAPES + [I.U8_BIG])
def test_byte_ingest_wrong_problems_differ(shape, bgr):
    src = I.u8_source(shape)
    want = I.u8_ref(src, bgr)
    assert want.dtype == np.float32 and want.shape == (shape[0], 3, shape[1], shape[2])
    for name, wrong in I.u8_wrongs(src, bgr).items():
        assert not np.array_equal(I.bits(wrong), I.bits(want)), (shape, name)


def test_byte_ingest_reference_divides():
    """The reference is the correctly rounded division: a multiply by the fp32 reciprocal differs from it for some byte values, so
    a kernel that multiplied would fail the sweep."""
    v = np.arange(256, dtype=np.float32)
    assert np.any(v / np.float32(255.0) != v * (np.float32(1.0) / np.float32(255.0)))


@pytest.mark.parametrize("case", I.PREP_BATCH_CASES)
def test_prepare_batch_wrong_problems_differ(case):
    (h, w), S = case
    src = I.prep_source(3, h, w)
    want = I.prep_ref(src, 0, w, 0, 1, S)
    assert np.array_equal(I.bits(want), I.bits(R.read_images(list(src), None, S)))
    assert I.rejected(1, I.prep_ref(I.shift_one_pixel(src), 0, w, 0, 1, S), want)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("erode", [0, 1])
@pytest.mark.parametrize("case", I.PREP_ABI_CASES)
def test_image_prep_abi_wrong_problems_differ(case, erode, mode):
    H, W, x0, cw, S = case
    src = I.prep_source(2, H, W)
    want = I.prep_ref(src, x0, cw, erode, mode, S)
    for name, wrong in I.prep_wrongs(src, x0, cw, erode, mode, S).items():
        assert I.rejected(mode, wrong, want), (case, name)
        if mode == 0:                                                  # far outside the bar, not at its edge
            assert np.abs(wrong - want).max() > 1000 * I.MODE0_BAR, (case, name)


@pytest.mark.parametrize("mode", [0, 1])
def test_image_prep_big_wrong_problems_differ(mode):
    g = I.PREP_BIG
    src = I.prep_source(g["N"], g["H"], g["W"])
    want = I.prep_ref(src, 0, g["W"], 1 - mode, mode, g["S"])
    for name, wrong in I.prep_wrongs(src, 0, g["W"], 1 - mode, mode, g["S"]).items():
        assert I.rejected(mode, wrong, want), name


def test_mode0_bar_holds_an_fp32_evaluation():
    """The 2e-6 bar against the fp64 oracle leaves room for an fp32 evaluation of the same expression (horizontal pass, vertical
    pass, division, each rounded to fp32): outputs lie in [0, 1], three roundings of the 255-scale sums and one of the quotient are
    about 4 * 2^-24 = 2.4e-7 relative.  Evaluated here in numpy fp32 over the C-ABI cases."""
    worst = 0.0
    for H, W, x0, cw, S in I.PREP_ABI_CASES:
        src = I.prep_source(2, H, W)
        for erode in (0, 1):
            want = I.prep_ref(src, x0, cw, erode, 0, S)
            for n, img in enumerate(src):
                crop = img[:, x0:x0 + cw, :]
                crop = (R.erode3x3(crop) if erode else crop).astype(np.float32)
                sx, fx = R._axis(cw, S)
                sy, fy = R._axis(H, S)
                x1, y1 = np.minimum(sx + 1, cw - 1), np.minimum(sy + 1, H - 1)
                a1, b1 = fx[None, :, None], fy[:, None, None]
                a0, b0 = np.float32(1.0) - a1, np.float32(1.0) - b1
                rows = crop[:, sx, :] * a0 + crop[:, x1, :] * a1
                got = ((rows[sy] * b0 + rows[y1] * b1) / np.float32(255.0)).transpose(2, 0, 1)
                assert got.dtype == np.float32
                worst = max(worst, float(np.abs(got.astype(np.float64) - want[n]).max()))
    print(f"fp32 numpy evaluation of mode 0: worst error {worst:.3e} (bar {I.MODE0_BAR:.0e})")
    assert worst <= I.MODE0_BAR / 4
