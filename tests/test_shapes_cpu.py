"""Host-side halves of tests/test_shapes_gpu.py (no GPU needed): the plan queries on both sides of the 2 GiB limits, the
c3 input gradient's argument checks past the scatter kernel's limit, and the discrimination of the fp64 error bound."""
import ctypes

import pytest
import torch

from discogan_modernized_amd import _lib, ops
from tests import shape_ref as R


def test_c3_dgrad_fused_form_depends_on_size_and_dy_type():
    """conv1 at 512 px: the scatter kernel takes dy up to 2^31 bytes, so an fp32 dy leaves it between batch 127 and 128, a bf16
    dy between 255 and 256; the fused activation backward exists only there."""
    L = _lib.load()
    assert [L.dg_c3_dgrad_act_ok(n, 512, 512, 64, 0) for n in (127, 128)] == [1, 0]
    assert [L.dg_c3_dgrad_act_ok(n, 512, 512, 64, 1) for n in (255, 256)] == [1, 0]
    assert L.dg_c3_dgrad_act_ok(1, 16, 16, 32, 0) == 0                       # K != 64: no scatter form
    assert ops.c3_dgrad_act_ok(64) and ops.c3_dgrad_act_ok(64, 127, 512, 512) and not ops.c3_dgrad_act_ok(64, 128, 512, 512)
    assert ops.c3_dgrad_act_ok(64, 255, 512, 512, dy_bf16=True) and not ops.c3_dgrad_act_ok(64, 256, 512, 512, dy_bf16=True)
    _lib.set_option("kt", 16)
    try:
        assert L.dg_c3_dgrad_act_ok(2, 16, 16, 64, 0) == 0
    finally:
        _lib.set_option("kt", 0)


def test_c3_dgrad_refuses_a_bf16_dy_on_the_fp32_kernels():
    """Past the scatter kernel's limit a bf16 dy is refused before anything is launched (the VALU and gather kernels read fp32),
    and so is the fused form (non-null dummies: validation fails before they are dereferenced)."""
    L = _lib.load()
    P = ctypes.c_void_p
    d = P(8)
    assert L.dg_conv4x4s2_c3_dgrad_t(d, 1, d, d, 256, 512, 512, 64, ops.ACT_NONE, None, 0, None) < 0
    assert b"VALU form reads an fp32 dy" in L.dg_last_error()
    assert L.dg_conv4x4s2_c3_dgrad_act_p(d, 1, d, ops.ACT_LEAKY, 0.2, d, d, 256, 512, 512, 64, ops.ACT_NONE, 0, None, 0, None) < 0
    assert b"scatter kernel" in L.dg_last_error()
    assert L.dg_conv4x4s2_c3_dgrad_act_p(d, 0, d, ops.ACT_LEAKY, 0.2, d, d, 128, 512, 512, 64, ops.ACT_NONE, 0, None, 0, None) < 0
    assert b"scatter kernel" in L.dg_last_error()


@pytest.mark.parametrize("N,fits", [(65535, True), (65536, False)])
def test_plans_drop_bf16_and_plane_kernels_at_2gib_per_plane(N, fits):
    """16 x 16 x 64 fp32 images with K = 256: a bf16 shadow / plane of x and dy reaches 2^31 bytes at N = 65536, and the plan then
    leaves the bf16 and f32x3 kernels for the fp32 pointer kernels (the plan queries report 0)."""
    L = _lib.load()
    bq = [L.dg_conv_bf16_operands_ok(op, N, 16, 16, 64, 256, 2, 1) for op in range(3)]
    xq = [L.dg_conv_x3_planes_ok(op, N, 16, 16, 64, 256, 2, 1) for op in range(3)]
    assert bq == ([2, 1, 2] if fits else [0, 0, 0]) and xq == ([1, 0, 1] if fits else [0, 0, 0])


def test_error_bound_catches_a_transposed_or_shifted_problem():
    """The bound of the GPU shape tests, evaluated on CPU against fp64 references of WRONG problems: the H <-> W transposed
    problem (re-transposed to the right shape) and the input shifted by one pixel both violate it, while an fp32 evaluation of
    the right problem stays inside."""
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 64, 16, 16, generator=g) * 2 - 1
    w = (torch.rand(128, 64, 4, 4, generator=g) * 2 - 1) / 32
    ref, absref = R.conv_ref("fwd", x, w)
    n = R.taps("fwd", 64, 128)
    R.assert_within(torch.nn.functional.conv2d(x, w, stride=2, padding=1), ref, absref, n, "fp32 CPU conv")
    transposed = R.conv_ref("fwd", x.transpose(2, 3), w)[0].transpose(2, 3)
    shifted = R.conv_ref("fwd", R.shift_w(x), w)[0]
    for wrong in (transposed, shifted):
        assert R.violations(wrong, ref, absref, n) > 0.5 * ref.numel()
        with pytest.raises(AssertionError, match="past the bound"):
            R.assert_within(wrong, ref, absref, n, "wrong problem")
