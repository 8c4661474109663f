"""Device-side helpers shared by tests/test_shapes_gpu.py and tests/test_channels_gpu.py (the CPU-side ones, `rnd` among them, live
in tests/shape_ref.py)."""
import torch

from discogan_modernized_amd import _lib, ops

DEV = "cuda"


def nhwc(t, dtype=torch.float32):
    """CPU logical NCHW -> GPU tensor with NHWC memory."""
    return t.to(DEV).to(dtype).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def krsc(w):
    return ops.krsc_param(w.to(DEV))


def with_shadow(t):
    t16 = torch.empty_like(t, dtype=torch.bfloat16, memory_format=torch.preserve_format)
    ops.f32_to_bf16(t, t16)
    ops.shadow_put(t, t16)
    t._dg_bf16, t._dg_bf16_ver = t16, t._version
    return t


class options:
    """Library options for the duration of a block, put back to 0 however it ends."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            _lib.set_option(k, 0)
        return False


class ambient:
    """ops.SHADOW / ops.ACT16 / ops.X3 for a block; derived copies cleared afterwards."""

    def __init__(self, shadow=False, act16=False, x3=False):
        self.v = (shadow, act16, x3)

    def __enter__(self):
        ops.SHADOW, ops.ACT16, ops.X3 = self.v

    def __exit__(self, *exc):
        ops.SHADOW = ops.ACT16 = ops.X3 = False
        ops.shadow_clear()
        ops.planes_clear()
        return False
