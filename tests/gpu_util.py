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


def conv_operands(x, w, dy, act16=False, shadow_x=False, shadow_dy=False, shadow_w=False):
    """Device operands of the three conv ops from CPU logical tensors (any may be None), in the forms a context hands over: x and dy
    with NHWC memory -- as bf16 tensors (act16: bf16 feature maps), or fp32, with a bf16 shadow where asked -- and w in KRSC memory,
    with a shadow where asked.  Call it inside the context the ops will run under: activation shadows live in its table."""
    if act16:
        xg, dyg = (None if t is None else nhwc(t, torch.bfloat16) for t in (x, dy))
    else:
        xg, dyg = (None if t is None else nhwc(t) for t in (x, dy))
        if shadow_x and xg is not None:
            with_shadow(xg)
        if shadow_dy and dyg is not None:
            with_shadow(dyg)
    wg = None if w is None else krsc(w)
    if shadow_w and wg is not None:
        with_shadow(wg)
    return xg, wg, dyg


# name -> (op, where the geometry starts in the argument list, kind) of the interior-conv launch entry points
_CONV_ENTRY = {"dg_conv_fwd_g": (0, 4, "g"), "dg_conv_dgrad_g": (1, 4, "g"), "dg_conv_wgrad_g": (2, 5, "g"),
               "dg_conv_fwd_mixed": (0, 6, "mixed"), "dg_conv_dgrad_mixed": (1, 6, "mixed"), "dg_conv_wgrad_mixed": (2, 5, "mixed"),
               "dg_conv_fwd_x3": (0, 6, "x3"), "dg_conv_dgrad_x3": (1, 6, "x3"), "dg_conv_wgrad_x3": (2, 6, "x3")}


class conv_requests:
    """Records what the conv wrappers really ask the library for: inside the block every interior-conv launch entry point is
    wrapped, and the list the block yields receives, per launch, the plan request (op, N, H, W, C, K, stride, pad, prec,
    plan_groups, a_form, b_form) that the entry point builds from its arguments (csrc/igemm.hip conv_g / conv_mixed / conv_x3)."""

    def __enter__(self):
        L = _lib.load()
        self.saved, calls = {}, []
        for name, (op, g0, kind) in _CONV_ENTRY.items():
            fn = getattr(L, name)
            self.saved[name] = fn

            def wrapped(*a, _fn=fn, _op=op, _g0=g0, _kind=kind):
                geom = tuple(int(v) for v in a[_g0:_g0 + 7])
                if _kind == "g":
                    form = (int(a[_g0 + 7]), int(a[_g0 + 8]), 0, 0)
                elif _kind == "mixed":        # bf16 operands or a bf16 output imply the bf16 arithmetic, else the process default
                    any16 = a[1] or a[3] or (_op != 2 and a[5])
                    form = (ops.PREC_BF16 if any16 else ops.PREC_DEFAULT, 1, int(a[1]), int(a[3]))
                else:
                    form = (ops.PREC_F32X3, 1, 3, 3)
                calls.append((_op,) + geom + form)
                return _fn(*a)

            setattr(L, name, wrapped)
        return calls

    def __exit__(self, *exc):
        L = _lib.load()
        for name, fn in self.saved.items():
            setattr(L, name, fn)
        return False


class nan_outputs:
    """Inside the block every activation tensor the op wrappers allocate (ops.empty_nhwc: conv outputs among them) starts as NaN
    instead of whatever the allocator's block held, so an element a kernel leaves unwritten shows as a non-finite value."""

    def __enter__(self):
        self.orig = orig = ops.empty_nhwc
        ops.empty_nhwc = lambda *a, **kw: orig(*a, **kw).fill_(float("nan"))

    def __exit__(self, *exc):
        ops.empty_nhwc = self.orig
        return False


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
