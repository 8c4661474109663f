"""The kernels at the boundary where users' tensors and image files enter, off the model's shapes: the layout transposes
(dg_nchw_to_nhwc / dg_nhwc_to_nchw), the byte ingest (dg_u8hwc_to_f32chw) and the image preparation (dg_image_prep), each against a
CPU reference (torch.permute, numpy, oracle/image_prep_ref.py) built in tests/ingest_ref.py.  Every comparison comes with wrong
problems it rejects; that those differ from the right problem is shown without a GPU in tests/test_layout_ingest_cpu.py.

Layout shapes against the 32 x 32 tile (R x Cn is C x H*W one way, H*W x C the other): (1,1,1,1) one element of one tile; (2,3,5,7)
R < 32 and Cn in two tiles (35), the last 3 wide; (1,31,1,33) and (1,33,1,31) one short of / one past the tile on either axis;
(3,32,4,8) exactly one full tile per image; (2,33,3,11) 33 x 33: four tiles, three of them one element wide or high; (1,64,1,1) and
(4,1,9,9) a one-wide axis (H*W = 1, C = 1); (2,100,6,6) 100 x 36: ragged last tile on both axes; (1,3,64,64) the image case,
3 x 4096.  Direct calls write into the middle of a larger allocation: the destination starts as a NaN of a known payload, 64 guard
floats of another pattern lie on each side, all inside one allocation.

Byte ingest: shapes whose pixel quads straddle image rows (W = 6, 7 with H*W % 4 == 0), the byte sweep, a batch past the
launcher's 4096-block cap.  Image preparation: mode 1 (cv2's 8-bit fixed point) bit-exact, mode 0 (float) within the existing 2e-6
of the fp64 oracle with the worst error printed (pytest -s); crops no domain rule makes; the crop edge as the erosion's image border,
on a built image; a batch past the launcher's 8192-block cap."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, dataset as ds, ops  # noqa: E402
from tests import ingest_ref as I  # noqa: E402

DEV = "cuda"
G = I.GUARD_FLOATS


class Guarded:
    """n destination floats in the middle of one allocation of G + n + G: destination = SENTINEL NaNs, guards = GUARD."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((G + n + G,), I.GUARD, dtype=torch.int32, device=DEV)
        self.buf[G:G + n] = I.SENTINEL
        self.ptr = self.buf.data_ptr() + 4 * G
        assert self.ptr % 16 == 0

    def read(self, written=True):
        """Destination bits after the call; the guards must be untouched, and every element written (or, written=False, none)."""
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert np.all(b[:G] == I.GUARD), "the guard band in front of the destination was written"
        assert np.all(b[G + self.n:] == I.GUARD), "the guard band behind the destination was written"
        dst = b[G:G + self.n]
        left = int((dst == I.SENTINEL).sum())
        if written:
            assert left == 0, f"{left} of {self.n} destination elements were not written"
        else:
            assert left == self.n, f"{self.n - left} destination elements were written by a refused call"
        return dst


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _reject_all(got, wrongs):
    for name, wrong in wrongs.items():
        assert not np.array_equal(got, wrong), f"the comparison does not tell the right problem from '{name}'"


# ==== 1. layout transposes =====================================================================================================
@pytest.mark.parametrize("direction", I.DIRECTIONS)
@pytest.mark.parametrize("shape", I.LAYOUT_SHAPES)
def test_layout_c_abi_bitwise(shape, direction):
    """One direction, called directly, against torch.permute on the CPU as int32 bit patterns (NaN payloads, +-inf, -0.0 among
    distinct values)."""
    N, C, H, W = shape
    src, want = I.layout_problem(direction, shape)
    x, dst = _dev_bits(src), Guarded(src.size)
    _lib.check(getattr(_lib.load(), "dg_" + direction)(x.data_ptr(), dst.ptr, N, C, H, W, _stream()), direction)
    got = dst.read()
    assert np.array_equal(got, want)
    _reject_all(got, I.layout_wrongs(direction, shape, src))


@pytest.mark.parametrize("shape", I.LAYOUT_SHAPES)
def test_as_nhwc_bitwise(shape):
    """ops.as_nhwc on a plain contiguous tensor: the result is the same logical tensor with NHWC memory."""
    N, C, H, W = shape
    src, want = I.layout_problem("nchw_to_nhwc", shape)
    x = _dev_bits(src).view(torch.float32).view(N, C, H, W)
    y = ops.as_nhwc(x)
    assert y.shape == x.shape and ops.is_nhwc(y)
    got = y.permute(0, 2, 3, 1).contiguous().view(torch.int32).reshape(-1).cpu().numpy()     # NHWC memory order: a plain copy
    assert y.permute(0, 2, 3, 1).is_contiguous()
    assert np.array_equal(got, want)
    _reject_all(got, I.layout_wrongs("nchw_to_nhwc", shape, src))
    assert np.array_equal(x.view(torch.int32).reshape(-1).cpu().numpy(), src), "the source was changed"


@pytest.mark.parametrize("shape", I.LAYOUT_SHAPES)
def test_to_nchw_contiguous_bitwise(shape):
    """ops.to_nchw_contiguous on a tensor with NHWC memory: plain contiguous memory, same logical tensor."""
    N, C, H, W = shape
    src, want = I.layout_problem("nhwc_to_nchw", shape)
    x = _dev_bits(src).view(torch.float32).view(N, H, W, C).permute(0, 3, 1, 2)
    y = ops.to_nchw_contiguous(x)
    assert y.shape == (N, C, H, W) and y.is_contiguous()
    got = y.view(torch.int32).reshape(-1).cpu().numpy()
    assert np.array_equal(got, want)
    _reject_all(got, I.layout_wrongs("nhwc_to_nchw", shape, src))


@pytest.mark.parametrize("direction", I.DIRECTIONS)
@pytest.mark.parametrize("shape", I.BIG_PLANES)
def test_layout_plane_past_the_old_grid_limit(shape, direction):
    """Grid limits.  An MI355X reports hipDeviceAttributeMaxGridDimX / Y / Z = 2 147 483 647 / 65 536 / 65 536.
    launch_transpose used to put ceil(R / 32) row tiles in grid.y with R = H*W for dg_nhwc_to_nchw (and R = C for dg_nchw_to_nhwc)
    and no host check: a single-channel plane of 1449 x 1449 = 2 099 601 pixels, 8.4 MB, asks for 65 613 > 65 536.  The tiles of
    one image now lie along grid.x, and what grid.x cannot hold (more than 16 777 215 tiles: 256-thread blocks, under 2^32 threads)
    is refused on the host (tests/test_layout_ingest_cpu.py).  Bitwise on planes just past the old limit, one channel and three."""
    N, C, H, W = shape
    assert -(-H * W // I.TILE) > I.OLD_GRID_Y_LIMIT and -(-H * W // I.TILE) * -(-C // I.TILE) <= I.transpose_max_tiles()
    src, want = I.layout_problem(direction, shape)
    x, dst = _dev_bits(src), Guarded(src.size)
    _lib.check(getattr(_lib.load(), "dg_" + direction)(x.data_ptr(), dst.ptr, N, C, H, W, _stream()), direction)
    got = dst.read()
    assert np.array_equal(got, want)
    _reject_all(got, I.layout_wrongs(direction, shape, src))


# ==== 2. byte ingest ===============================================================================================================
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("shape", I.U8_SHAPES)
def test_byte_ingest_bitwise(shape, bgr):
    """Wrapper and direct call against src.astype(np.float32) / 255. transposed, bit for bit; guards and sentinel on the direct
    call.  (2,2,6) and (2,4,7): quads straddle rows.  (1,16,16), (4,16,16): the byte sweep (ingest_ref.u8_source)."""
    N, H, W = shape
    src = I.u8_source(shape)
    want = I.bits(I.u8_ref(src, bgr)).reshape(-1)
    x = torch.from_numpy(src).to(DEV)
    y = ops.u8hwc_to_f32chw(x, bgr=bgr)
    assert y.shape == (N, 3, H, W) and y.dtype == torch.float32 and y.is_contiguous()
    got_w = y.view(torch.int32).reshape(-1).cpu().numpy()
    dst = Guarded(want.size)
    _lib.check(_lib.load().dg_u8hwc_to_f32chw(x.data_ptr(), dst.ptr, N, H, W, int(bgr), _stream()), "dg_u8hwc_to_f32chw")
    got = dst.read()
    wrongs = {k: I.bits(v).reshape(-1) for k, v in I.u8_wrongs(src, bgr).items()}
    for g in (got_w, got):
        assert np.array_equal(g, want), f"{int((g != want).sum())} of {want.size} elements differ"
        _reject_all(g, wrongs)
    assert np.array_equal(x.cpu().numpy(), src), "the source was changed"


@pytest.mark.parametrize("bgr", [False, True])
def test_byte_ingest_past_the_grid_cap(bgr):
    """(17, 512, 512): 1 114 112 pixel quads on a grid capped at 4096 blocks of 256, so 65 536 quads (a whole image) take the
    second trip of the grid-stride loop."""
    N, H, W = I.U8_BIG
    cap = I.launcher_cap("misc.hip", "dg_u8hwc_to_f32chw")
    assert N * H * W // 4 > cap * I.BLOCK
    src = I.u8_source(I.U8_BIG)
    want = I.bits(I.u8_ref(src, bgr))
    got = ops.u8hwc_to_f32chw(torch.from_numpy(src).to(DEV), bgr=bgr).view(torch.int32).cpu().numpy()
    first_trip = cap * I.BLOCK * 4 // (H * W)                          # images wholly inside the first trip
    assert first_trip == N - 1
    assert np.array_equal(got[first_trip:], want[first_trip:]), "the second trip of the grid-stride loop"
    assert np.array_equal(got, want)
    for name, wrong in I.u8_wrongs(src[first_trip:], bgr).items():
        assert not np.array_equal(got[first_trip:], I.bits(wrong)), name


def test_byte_ingest_takes_a_non_contiguous_view():
    wide = torch.from_numpy(I.u8_source((3, 6, 10), seed=9)).to(DEV)
    view = wide[:, :, 1:-1]
    assert not view.is_contiguous() and view.shape == (3, 6, 8, 3)
    src = wide.cpu().numpy()[:, :, 1:-1]
    for bgr in (False, True):
        got = ops.u8hwc_to_f32chw(view, bgr=bgr)
        assert torch.equal(got, ops.u8hwc_to_f32chw(view.contiguous(), bgr=bgr))
        got = got.view(torch.int32).cpu().numpy()
        assert np.array_equal(got, I.bits(I.u8_ref(src, bgr)))
        for name, wrong in I.u8_wrongs(np.ascontiguousarray(src), bgr).items():
            assert not np.array_equal(got, I.bits(wrong)), name


@pytest.mark.parametrize("shape", [(1, 3, 3), (2, 1, 2), (1, 5, 7)])
def test_byte_ingest_refuses_ragged_quads(shape):
    """H*W % 4 != 0 is refused -- through the wrapper as an exception -- and nothing is written."""
    N, H, W = shape
    x = torch.from_numpy(I.u8_source(shape)).to(DEV)
    with pytest.raises(_lib.DiscoganHipError, match="multiple of 4"):
        ops.u8hwc_to_f32chw(x)
    dst = Guarded(N * 3 * H * W + 8)
    with pytest.raises(_lib.DiscoganHipError, match="multiple of 4"):
        _lib.check(_lib.load().dg_u8hwc_to_f32chw(x.data_ptr(), dst.ptr, N, H, W, 0, _stream()), "dg_u8hwc_to_f32chw")
    dst.read(written=False)


# ==== 3. image preparation =====================================================================================================
def _compare_prep(got, want, wrongs, mode, what):
    """Mode 1: bits.  Mode 0: the 2e-6 bar, worst error printed.  Either way every wrong problem is rejected by the same rule."""
    assert got.shape == want.shape and got.dtype == np.float32
    if mode == 1:
        assert np.array_equal(I.bits(got), I.bits(want)), f"{what}: max diff {np.abs(got - want).max():.3e}"
        worst = 0.0
    else:
        worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print(f"dg_image_prep mode 0, {what}: worst error {worst:.3e} (bar {I.MODE0_BAR:.0e})")
        assert worst <= I.MODE0_BAR, f"{what}: {worst:.3e}"
    for name, wrong in wrongs.items():
        assert I.rejected(mode, got, wrong), f"{what}: the comparison does not tell the right problem from '{name}'"
    return worst


def _prep_abi(src, x0, cw, erode, mode, S):
    n, H, W, _ = src.shape
    x, dst = torch.from_numpy(src).to(DEV), Guarded(n * 3 * S * S)
    _lib.check(_lib.load().dg_image_prep(x.data_ptr(), dst.ptr, n, H, W, x0, cw, erode, mode, S, _stream()), "dg_image_prep")
    return dst.read().view(np.float32).reshape(n, 3, S, S)


@pytest.mark.parametrize("case", I.PREP_BATCH_CASES)
def test_prepare_batch_uint8_path_bit_exact(case):
    """dataset.prepare_batch, domain None (mode 1): different non-integer ratios on the two axes, up and down, one-pixel axes, one
    and two output pixels, exact 2x both ways."""
    (h, w), S = case
    src = I.prep_source(3, h, w)
    got = ds.prepare_batch(torch.from_numpy(src).to(DEV), None, S).cpu().numpy()
    _compare_prep(got, I.prep_ref(src, 0, w, 0, 1, S), {"shifted": I.prep_ref(I.shift_one_pixel(src), 0, w, 0, 1, S)}, 1, f"{case}")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("erode", [0, 1])
@pytest.mark.parametrize("case", I.PREP_ABI_CASES)
def test_image_prep_abi_every_combination(case, erode, mode):
    """(erode, mode) in all four combinations -- the domain rules make three -- on crops they never make: odd x0 (unaligned byte
    offsets), cw = 1, cw = W, a crop ending at the last column; H != cw throughout.  Guarded destination."""
    H, W, x0, cw, S = case
    src = I.prep_source(2, H, W)
    got = _prep_abi(src, x0, cw, erode, mode, S)
    _compare_prep(got, I.prep_ref(src, x0, cw, erode, mode, S), I.prep_wrongs(src, x0, cw, erode, mode, S), mode,
                  f"(H, W, x0, cw, S) {case} erode {erode}")


@pytest.mark.parametrize("mode", [0, 1])
def test_erosion_treats_the_crop_edge_as_the_image_border(mode):
    """White images with black columns x0 - 1 and x0 + cw, identity-size resize (exact in both modes): the first and last output
    columns stay white, a black 3 x 3 block inside grows to exactly 5 x 5, and black pixels in the crop's four corners darken
    exactly the 2 x 2 corner neighbourhoods.  A kernel that took neighbours beside the crop would give ingest_ref.prep_leaky_ref."""
    g, src, want = I.BORDER, I.border_source(), I.border_expected()
    got = _prep_abi(src, g["x0"], g["cw"], 1, mode, g["S"])
    assert np.all(got[0, :, :, 0] == 1.0) and np.all(got[0, :, :, -1] == 1.0), "a black column beside the crop leaked in"
    by, bx = g["block"]
    assert np.all(got[0, :, by - 1:by + 4, bx - 1:bx + 4] == 0.0) and int((got[0] == 0.0).sum()) == 3 * 25
    assert int((got[1] == 0.0).sum()) == 3 * 16 and np.all(got[1, :, 2:-2, :] == 1.0) and np.all(got[1, :, :, 2:-2] == 1.0)
    wrongs = dict(I.prep_wrongs(src, g["x0"], g["cw"], 1, mode, g["S"]), leak=I.prep_leaky_ref(src, g["x0"], g["cw"], mode, g["S"]))
    worst = _compare_prep(got, want, wrongs, mode, "border rule")
    assert worst == 0.0 and np.array_equal(I.bits(got), I.bits(want))


@pytest.mark.parametrize("mode", [0, 1])
def test_image_prep_past_the_grid_cap(mode):
    """N = 9 images of 8 x 8 to S = 512: 2 359 296 output pixels on a grid capped at 8192 blocks of 256, so the last image takes the
    second trip of the grid-stride loop; a 64x enlargement spreads the clamped half-pixel bands over 32 output rows and columns at
    each edge.  Mode 1 without erosion, mode 0 with it (the pairs the domain rules use)."""
    g = I.PREP_BIG
    cap = I.launcher_cap("ingest.hip", "dg_image_prep")
    assert g["N"] * g["S"] ** 2 > cap * I.BLOCK and (g["N"] - 1) * g["S"] ** 2 == cap * I.BLOCK
    src = I.prep_source(g["N"], g["H"], g["W"])
    erode = 1 - mode
    got = _prep_abi(src, 0, g["W"], erode, mode, g["S"])
    want = I.prep_ref(src, 0, g["W"], erode, mode, g["S"])
    _compare_prep(got, want, I.prep_wrongs(src, 0, g["W"], erode, mode, g["S"]), mode, f"past the cap, erode {erode}")
    last = slice(g["N"] - 1, g["N"])
    _compare_prep(got[last], want[last], {k: v[last] for k, v in I.prep_wrongs(src, 0, g["W"], erode, mode, g["S"]).items()}, mode,
                  "second trip")
    # the clamped bands: output rows / columns 0..31 and 480..511 repeat the (eroded) border pixels
    assert np.array_equal(got[:, :, :32, :], np.broadcast_to(got[:, :, :1, :], got[:, :, :32, :].shape))
    assert np.array_equal(got[:, :, :, -32:], np.broadcast_to(got[:, :, :, -1:], got[:, :, :, -32:].shape))


def test_image_prep_refusals_write_nothing():
    """A crop outside the row, mode 2 and a null pointer arrive as exceptions, and the destination is untouched."""
    src = I.prep_source(2, 8, 10)
    x, S = torch.from_numpy(src).to(DEV), 4
    L = _lib.load()
    for args, text in (((x.data_ptr(), 2, 8, 10, 6, 5, 0, 1), "outside the 10-pixel rows"), ((x.data_ptr(), 2, 8, 10, 1, 5, 0, 2), "mode 0"),
                       ((None, 2, 8, 10, 1, 5, 0, 1), "bad argument")):
        dst = Guarded(2 * 3 * S * S)
        with pytest.raises(_lib.DiscoganHipError, match=text):
            _lib.check(L.dg_image_prep(args[0], dst.ptr, *args[1:], S, _stream()), "dg_image_prep")
        dst.read(written=False)
    with pytest.raises(_lib.DiscoganHipError, match="bad argument"):
        _lib.check(L.dg_image_prep(x.data_ptr(), None, 2, 8, 10, 1, 5, 0, 1, S, _stream()), "dg_image_prep")
    with pytest.raises(ValueError):
        ds.prepare_batch(x, "B", S)                                     # no columns from 256 on
