"""CPU side of tests/test_layout_ingest_gpu.py, shared with tests/test_layout_ingest_cpu.py: the case tables, the payloads, the right
problem and the wrong problems of every comparison, and the launch constants read out of the kernel sources.  Numpy only (torch for
the CPU `permute` the layout kernels are held to); nothing here touches a device.

The image preparation is NOT restated: oracle/image_prep_ref.py exposes the erosion and both resizes, and `prep_ref` composes them for
any (x0, cw, erode, mode), the four combinations of which the oracle's own `prepare_image` covers three."""
import os
import re

import numpy as np
import torch

from oracle import image_prep_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "discogan_modernized_amd", "csrc")

# ---- constants of the kernels, read from their sources ---------------------------------------------------------------
TILE = 32                       # transpose_kernel: 32 x 32 LDS tile
OLD_GRID_Y_LIMIT = 65536        # hipDeviceAttributeMaxGridDimY: the row tiles of one image used to lie along grid.y
BLOCK = 256


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def launcher_cap(source, entry):
    """The grid cap `if (g > CAP) g = CAP;` of the launcher `entry` in csrc/`source`."""
    text = _source(source)
    body = text[text.index(f'extern "C" int {entry}('):]
    m = re.search(r"if \(g > (\d+)\) g = (\d+);", body)
    assert m and m.group(1) == m.group(2), f"{entry}: no grid cap found"
    return int(m.group(1))


def transpose_max_tiles():
    m = re.search(r"#define TRANSPOSE_MAX_TILES (\d+)L", _source("misc.hip"))
    assert m, "TRANSPOSE_MAX_TILES not found"
    return int(m.group(1))


# ---- bit patterns -------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC0BEEF           # the NaN every destination element starts as
GUARD = 0x4B1D4B1D              # the (finite) pattern of the guard bands
GUARD_FLOATS = 64
# quiet NaNs of both signs with payloads, +-inf, -0.0, +0.0, the smallest denormal, the largest finite
SPECIALS = (0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x7F7FFFFF)


def layout_payload(n, seed):
    """n distinct int32 bit patterns in a seeded order: floats of [1, 2) numbered by a permutation of the indices, with the
    SPECIALS in the first places of a second permutation (as many as fit).  None equals SENTINEL or GUARD."""
    assert n < (1 << 23)
    rng = np.random.default_rng(seed)
    bits = (np.uint32(0x3F800000) + rng.permutation(n).astype(np.uint32))
    where = rng.permutation(n)[:len(SPECIALS)]
    bits[where] = np.array(SPECIALS[:len(where)], dtype=np.uint32)
    return bits.view(np.int32)


# ---- 1. layout transposes ---------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 31, 1, 33), (1, 33, 1, 31), (3, 32, 4, 8), (2, 33, 3, 11), (1, 64, 1, 1), (2, 100, 6, 6),
                 (1, 3, 64, 64), (4, 1, 9, 9)]
DIRECTIONS = ("nchw_to_nhwc", "nhwc_to_nchw")
# planes whose H*W / 32 row tiles do not fit grid.y: single channel (the issue's case) and three channels (a real transposition)
BIG_PLANES = [(1, 1, 1449, 1449), (1, 3, 1449, 1449)]


def layout_problem(direction, shape, seed=0):
    """(source bits, flat, as the kernel reads them; expected destination bits, flat) with torch.permute on the CPU."""
    N, C, H, W = shape
    src = layout_payload(N * C * H * W, seed + (0 if direction == DIRECTIONS[0] else 1))
    t = torch.from_numpy(src)
    if direction == "nchw_to_nhwc":
        want = t.view(N, C, H, W).permute(0, 2, 3, 1).contiguous()
    else:
        want = t.view(N, H, W, C).permute(0, 3, 1, 2).contiguous()
    return src, want.reshape(-1).numpy()


def layout_wrongs(direction, shape, src):
    """name -> flat destination bits of the wrong problems.  'hw_swapped': H and W exchanged; 'other_direction': the source read as
    the other layout and permuted the other way; 'rolled': the right answer moved on by one element.  A wrong problem that IS the
    right one is left out, and `layout_degenerate` says which those are: with H or W equal to 1 exchanging them moves nothing,
    with C = 1 or H*W = 1 both directions are the identity, and with C = H*W both are the transpose of the same square matrix."""
    N, C, H, W = shape
    t = torch.from_numpy(src)
    out = {}
    if direction == "nchw_to_nhwc":
        right = t.view(N, C, H, W).permute(0, 2, 3, 1)
        swapped = t.view(N, C, H, W).permute(0, 3, 2, 1)
        other = t.view(N, H, W, C).permute(0, 3, 1, 2)
    else:
        right = t.view(N, H, W, C).permute(0, 3, 1, 2)
        swapped = t.view(N, H, W, C).permute(0, 3, 2, 1)
        other = t.view(N, C, H, W).permute(0, 2, 3, 1)
    deg = layout_degenerate(shape)
    if H != W and "hw_swapped" not in deg:
        out["hw_swapped"] = swapped.contiguous().reshape(-1).numpy()
    if "other_direction" not in deg:
        out["other_direction"] = other.contiguous().reshape(-1).numpy()
    if src.size > 1:
        out["rolled"] = np.roll(right.contiguous().reshape(-1).numpy(), 1)
    else:
        out["untouched"] = np.full(1, SENTINEL, dtype=np.int32)
    return out


def layout_degenerate(shape):
    N, C, H, W = shape
    deg = set()
    if H == W or min(H, W) == 1:
        deg.add("hw_swapped")
    if C == 1 or H * W == 1 or C == H * W:
        deg.add("other_direction")
    return deg


# ---- 2. byte ingest ---------------------------------------------------------------------------------------------------------
U8_SHAPES = [(1, 2, 2), (3, 1, 4), (2, 2, 6), (2, 4, 7), (5, 16, 24), (1, 16, 16), (4, 16, 16)]
U8_SWEEPS = {(1, 16, 16), (4, 16, 16)}
U8_BIG = (17, 512, 512)


def u8_source(shape, seed=5):
    """uint8 [N, H, W, 3].  The 16 x 16 shapes are the byte sweep: pixel index p = 16 y + x, image k, channel c holds (p + k + 85 c) mod
    256.  In one image a position j of the 12-byte group (pixel p % 4, channel c) sees the 64 values congruent to j + c mod 4; the
    four images of (4, 16, 16) shift that residue through all four, so every byte value passes every position."""
    N, H, W = shape
    if shape in U8_SWEEPS:
        p = np.arange(H * W).reshape(1, H, W, 1)
        k = np.arange(N).reshape(N, 1, 1, 1)
        c = np.array([0, 85, 170]).reshape(1, 1, 1, 3)
        return ((p + k + c) % 256).astype(np.uint8)
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


def u8_ref(src, bgr):
    """src.astype(np.float32) / 255. transposed to [N, 3, H, W] (channels reversed first with bgr)."""
    s = src[..., ::-1] if bgr else src
    return np.ascontiguousarray((s.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))


def u8_wrongs(src, bgr):
    return {"other_bgr": u8_ref(src, not bgr), "shifted": u8_ref(shift_one_pixel(src), bgr)}


def shift_one_pixel(src):
    """The batch [N, H, W, 3] moved on by one source pixel: along the rows, or down the columns where a row has one pixel."""
    return np.roll(src, 1, axis=2 if src.shape[2] > 1 else 1)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- 3. image preparation ---------------------------------------------------------------------------------------------------
MODE0_BAR = 2e-6                # tests/test_ingest_gpu.py: fp32 against the oracle's fp64 accumulation

# (h, w) -> S through dataset.prepare_batch, domain None (x0 = 0, cw = w, no erosion, mode 1)
PREP_BATCH_CASES = [((33, 47), 20), ((47, 33), 20), ((7, 200), 64), ((200, 7), 64), ((1, 9), 8), ((9, 1), 8), ((5, 5), 1), ((5, 5), 2),
                    ((64, 64), 128), ((128, 128), 64)]
# (H, W, x0, cw, S) through the C ABI: odd x0 up-scaling; cw = 1; cw = W; an odd x0 whose crop ends at the last column, down-scaling.
# H differs from cw in all of them.
PREP_ABI_CASES = [(9, 20, 3, 11, 16), (6, 13, 5, 1, 7), (10, 7, 0, 7, 12), (5, 16, 7, 9, 6)]
PREP_BIG = dict(N=9, H=8, W=8, S=512)


def prep_source(n, h, w, seed=21):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def prep_ref(src, x0, cw, erode, mode, S):
    """dg_image_prep's contract from the oracle's pieces: crop, erosion inside the crop, one of the two resizes, / 255, CHW."""
    out = []
    for img in src:
        crop = img[:, x0:x0 + cw, :]
        if erode:
            crop = R.erode3x3(crop)                                  # integer-valued float64
        if mode == 1:
            v = R.resize_linear_u8(np.asarray(crop).astype(np.uint8), S)
        else:
            v = R.resize_linear_float(np.asarray(crop).astype(np.float64), S)
        out.append(np.ascontiguousarray((v.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)))
    return np.stack(out)


def prep_wrongs(src, x0, cw, erode, mode, S):
    """The reference of the source moved by one pixel, and the reference with the erosion switched the other way."""
    return {"shifted": prep_ref(shift_one_pixel(src), x0, cw, erode, mode, S), "erosion_switched": prep_ref(src, x0, cw, 1 - erode, mode, S)}


def prep_leaky_ref(src, x0, cw, mode, S):
    """The wrong problem of the border rule: the erosion taken over the whole rows and cropped afterwards, so that pixels beside
    the crop count as neighbours."""
    out = []
    for img in src:
        crop = R.erode3x3(img)[:, x0:x0 + cw, :]
        v = R.resize_linear_u8(crop.astype(np.uint8), S) if mode == 1 else R.resize_linear_float(crop, S)
        out.append(np.ascontiguousarray((v.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)))
    return np.stack(out)


def rejected(mode, a, b):
    """Does the comparison of `mode` tell a from b?  Mode 1 compares bits; mode 0 allows MODE0_BAR."""
    if mode == 1:
        return not np.array_equal(bits(a), bits(b))
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) > MODE0_BAR


BORDER = dict(H=12, W=20, x0=5, cw=12, S=12, block=(5, 5))           # identity-size resize: S == cw == H


def border_source():
    """Two all-white images [2, H, W, 3] with black columns x0 - 1 and x0 + cw just outside the crop.  Image 0: a black 3 x 3 block
    inside the crop (crop rows / columns 5..7).  Image 1: black pixels in the crop's own four corners."""
    g = BORDER
    src = np.full((2, g["H"], g["W"], 3), 255, dtype=np.uint8)
    src[:, :, g["x0"] - 1] = 0
    src[:, :, g["x0"] + g["cw"]] = 0
    by, bx = g["block"]
    src[0, by:by + 3, g["x0"] + bx:g["x0"] + bx + 3] = 0
    for y in (0, g["H"] - 1):
        for x in (g["x0"], g["x0"] + g["cw"] - 1):
            src[1, y, x] = 0
    return src


def border_expected():
    """What the rule gives, written down by hand: [2, 3, S, S] of 0.0 / 1.0."""
    g = BORDER
    S = g["S"]
    want = np.ones((2, 3, S, S), dtype=np.float32)
    by, bx = g["block"]
    want[0, :, by - 1:by + 4, bx - 1:bx + 4] = 0.0                   # 3 x 3 grows to 5 x 5
    for ys in (slice(0, 2), slice(S - 2, S)):
        for xs in (slice(0, 2), slice(S - 2, S)):
            want[1, :, ys, xs] = 0.0                                  # a corner pixel darkens its 2 x 2 neighbourhood
    return want
