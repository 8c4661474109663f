"""One element-wise check per conv plan the model's layers get (the cases; tests/test_plan_cases_gpu.py runs them).

The planner (csrc/igemm.hip make_plan) picks the code a convolution runs from the GEMM mode, the arithmetic, the operand forms, the
tile, the kernel family, whether K is split and the blockIdx-to-tile order.  `dg_conv_plan_describe` reports that plan from the
library itself (no planner is restated here).  This module
  * lists every conv request the networks make (`model_requests`) at 64 px / batch 64, 64 px / batch 256 and 512 px / batch 32,
  * keeps committed lists of small shapes, each with the signature it must reach: `PLAN_CASES`, one per signature, and `MORE_CASES`,
    further shapes of the same signatures with more tiles, ragged edges and longer reductions, and
  * asserts that the library gives each case its signature, that every signature of a model layer is the signature of a case of
    `PLAN_CASES`, and that no case checks a plan no layer gets.
No GPU is needed: the query makes no device call."""
import ctypes
import itertools

import pytest

from discogan_modernized_amd import _lib, model, ops

FIELDS = ("mode", "prec", "wm", "wn", "kt", "dma", "ncls", "M", "Ng", "BM", "BN", "tilesM", "tilesN", "zmul", "nIt", "splits", "itPerSplit",
          "xcd_group", "stat_rows", "addressing")
F32, BF16, F32X3 = ops.PREC_F32, ops.PREC_BF16, ops.PREC_F32X3
WINDOW_KERNELS = (3, 4)           # kernel families that ignore xcd_group: the f32x3 and the bf16 window input-gradient kernels
CASE_OPTIONS = ("splitk", "pointer_path")        # the only library options a case may set


def describe(req, opts=None):
    """dg_conv_plan_describe of req = (op, N, H, W, C, K, stride, pad, prec, plan_groups, a_form, b_form) under the library options
    `opts` (put back to 0 afterwards): dict of FIELDS plus the request's operand forms, or None where the request has no plan."""
    L = _lib.load()
    opts = opts or {}
    for k, v in opts.items():
        _lib.set_option(k, v)
    try:
        out = (ctypes.c_int * len(FIELDS))()
        n = L.dg_conv_plan_describe(*req, out, len(FIELDS))
    finally:
        for k in opts:
            _lib.set_option(k, 0)
    if n == 0:
        return None
    assert n == len(FIELDS), f"the library knows {n} plan fields, this module {len(FIELDS)}"
    d = dict(zip(FIELDS, out))
    d["a_form"], d["b_form"] = req[10], req[11]
    return d


def signature(f):
    """The fields that select code: (mode, arithmetic actually used, a_form, b_form, wm, wn, kt, kernel family, ncls, split?, tile order,
    addressing)."""
    return (f["mode"], f["prec"], f["a_form"], f["b_form"], f["wm"], f["wn"], f["kt"], f["dma"], f["ncls"], f["splits"] > 1,
            "n/a" if f["dma"] in WINDOW_KERNELS else f["xcd_group"], f["addressing"])


# ---- what the networks ask for ----------------------------------------------------------------------------------------------
CONFIGS = [(64, 64), (64, 256), (512, 32)]             # (image size, batch)
# (arithmetic, a_form, b_form) the three mfma_dtype settings can hand over: "f32"; "bf16" without shadows and with a bf16 tensor (a
# shadow, or bf16 feature maps) on either side or both; "f32x3" with fp32 tensors (register-staged split) and with plane triples
FORMS = [(F32, 0, 0), (BF16, 0, 0), (BF16, 1, 0), (BF16, 0, 1), (BF16, 1, 1), (F32X3, 0, 0), (F32X3, 3, 3)]
GROUPED_FORMS = [(F32, 0, 0), (F32X3, 0, 0)]           # trainer.py can_group: fp32 tensors on exact fp32 or register-staged f32x3
GROUPED_BELOW_PX = 256                                 # trainer.py: group_launch defaults to image_size < 256
GROUPS = 4                                             # a D-step's real and fake pass of both sides


def interior_layers(image_size):
    """(name, H, C, K, stride, pad) of every interior conv geometry of Generator and Discriminator: the stride-2 layers between the stages
    (encoder / discriminator Conv2d; the decoder's ConvTranspose2d is the same geometry with forward and input gradient swapped) and the
    100-channel bottleneck on the 4 x 4 map (encoder Conv2d(ch, 100, 4, 1, 0); decoder ConvTranspose2d(100, ch, 4, 1, 0)).  The
    3-channel edge layers have kernels of their own and the discriminator's K == 1 head has no plan."""
    ch = model.stage_channels(image_size)
    out = [(f"{image_size}px {ch[i - 1]}->{ch[i]} @{image_size >> i}", image_size >> i, ch[i - 1], ch[i], 2, 1) for i in range(1, len(ch))]
    out.append((f"{image_size}px {ch[-1]}->100 bottleneck", 4, ch[-1], 100, 1, 0))
    return out


def refused(op, C, K, stride, prec, a_form, b_form, plan):
    """Why the launch entry points refuse a combination (csrc/igemm.hip), or None:
      check_channels     a forward needs C % 32 == 0, a stride-2 input gradient K % 32 == 0 (such a request has no plan either);
      mixed_plan_rules   a bf16 gradient operand (a_form 1 of op 1 / 2) needs K % 8 == 0; a bf16 x of the weight gradient C % 8 == 0;
                         bf16 operands need the bf16 tile kernels (the plan's arithmetic is bf16);
      x3_plan_rules      plane operands need a plane kernel (family 2 or 3)."""
    if plan is None:
        return "no plan (channel rules)"
    if prec == BF16 and a_form == 1 and op != 0 and K % 8 != 0:
        return "bf16 gradient operand with K % 8 != 0"
    if prec == BF16 and b_form == 1 and op == 2 and C % 8 != 0:
        return "bf16 x of a weight gradient with C % 8 != 0"
    if prec == BF16 and (a_form or b_form) and plan["prec"] != BF16:
        return "bf16 operands without a bf16 tile kernel"
    if a_form == 3 and plan["dma"] not in (2, 3):
        return "plane operands without a plane kernel"
    return None


def model_requests():
    """(layer name, request, plan fields) of every conv launch the networks can make, refused combinations dropped."""
    for size, batch in CONFIGS:
        for name, H, C, K, stride, pad in interior_layers(size):
            for op, (prec, af, bf) in itertools.product(range(3), FORMS):
                groups = [1] + ([GROUPS] if size < GROUPED_BELOW_PX and (prec, af, bf) in GROUPED_FORMS else [])
                for pg in groups:
                    req = (op, batch, H, H, C, K, stride, pad, prec, pg, af, bf)
                    plan = describe(req)
                    if refused(op, C, K, stride, prec, af, bf, plan) is None:
                        yield f"{name} batch {batch} op {op} groups {pg}", req, plan


def conv_work(f, req):
    """2 M Ng R of the request's GEMM (the four parity classes of a stride-2 input gradient together)."""
    op, N, H, W, C, K, stride = req[:7]
    npix = N * (H // 2) * (W // 2) if stride == 2 else N
    R = 16 * C if op == 0 else (npix if op == 2 else (4 * K if stride == 2 else K))
    return 2 * f["M"] * f["Ng"] * R * f["zmul"]


def case_bytes(f, req, opts):
    """fp32 operands + output + the split-K workspace the wrappers allocate for the request's arithmetic."""
    op, N, H, W, C, K, stride, pad, prec, pg = req[:10]
    Ho, Wo = (H // 2, W // 2) if stride == 2 else (1, 1)
    L = _lib.load()
    for k, v in opts.items():
        _lib.set_option(k, v)
    try:
        ws = L.dg_conv_workspace_bytes_p(op, N, H, W, C, K, stride, pad, prec, pg)
    finally:
        for k in opts:
            _lib.set_option(k, 0)
    return 4 * (N * H * W * C + N * Ho * Wo * K + 16 * C * K) + ws


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# (request, options, signature).  PLAN_CASES holds exactly one case per signature of model_requests(): the shape of least conv work
# that a search over the query found for it (N from 2, power-of-two H <= W from 4, channel counts 32 .. 2048, option splitk 0 .. 3)
# -- two images and a 2 x 2 output at the least (the 4 x 4 bottleneck aside), so that shape_ref.wrong_problems has its shifts.
# Take any one of them away and test_every_model_signature_has_a_case names the layers that lost their check.
PLAN_CASES = [
    ((0, 2, 8, 256, 32, 160, 2, 1, 0, 1, 0, 0), {"splitk": 1}, (0, 0, 0, 0, 2, 2, 32, 0, 0, False, 1, 0)),
    ((0, 2, 8, 256, 32, 32, 2, 1, 0, 1, 0, 0), {"splitk": 1}, (0, 0, 0, 0, 2, 2, 32, 0, 0, False, 3, 0)),
    ((0, 2, 4, 4, 64, 100, 1, 0, 0, 1, 0, 0), {}, (0, 0, 0, 0, 2, 2, 32, 0, 0, True, 1, 0)),
    ((0, 9, 4, 16, 32, 160, 2, 1, 0, 1, 0, 0), {}, (0, 0, 0, 0, 2, 2, 32, 0, 0, True, 2, 0)),
    ((0, 2, 8, 256, 32, 32, 2, 1, 0, 1, 0, 0), {}, (0, 0, 0, 0, 2, 2, 32, 0, 0, True, 3, 0)),
    ((0, 2, 8, 256, 64, 160, 2, 1, 1, 1, 0, 0), {"splitk": 1}, (0, 1, 0, 0, 2, 2, 64, 0, 0, False, 1, 0)),
    ((0, 2, 8, 256, 64, 32, 2, 1, 1, 1, 0, 0), {"splitk": 1}, (0, 1, 0, 0, 2, 2, 64, 0, 0, False, 3, 0)),
    ((0, 2, 4, 4, 128, 100, 1, 0, 1, 1, 0, 0), {}, (0, 1, 0, 0, 2, 2, 64, 0, 0, True, 1, 0)),
    ((0, 9, 4, 16, 64, 160, 2, 1, 1, 1, 0, 0), {}, (0, 1, 0, 0, 2, 2, 64, 0, 0, True, 2, 0)),
    ((0, 2, 8, 256, 64, 32, 2, 1, 1, 1, 0, 0), {}, (0, 1, 0, 0, 2, 2, 64, 0, 0, True, 3, 0)),
    ((0, 2, 8, 256, 64, 160, 2, 1, 1, 1, 0, 1), {"splitk": 1}, (0, 1, 0, 1, 2, 2, 64, 0, 0, False, 1, 0)),
    ((0, 2, 8, 256, 64, 32, 2, 1, 1, 1, 0, 1), {"splitk": 1}, (0, 1, 0, 1, 2, 2, 64, 0, 0, False, 3, 0)),
    ((0, 2, 4, 4, 128, 100, 1, 0, 1, 1, 0, 1), {}, (0, 1, 0, 1, 2, 2, 64, 0, 0, True, 1, 0)),
    ((0, 9, 4, 16, 64, 160, 2, 1, 1, 1, 0, 1), {}, (0, 1, 0, 1, 2, 2, 64, 0, 0, True, 2, 0)),
    ((0, 2, 8, 256, 64, 32, 2, 1, 1, 1, 0, 1), {}, (0, 1, 0, 1, 2, 2, 64, 0, 0, True, 3, 0)),
    ((0, 2, 8, 256, 64, 160, 2, 1, 1, 1, 1, 0), {"splitk": 1}, (0, 1, 1, 0, 2, 2, 64, 0, 0, False, 1, 0)),
    ((0, 2, 8, 256, 64, 32, 2, 1, 1, 1, 1, 0), {"splitk": 1}, (0, 1, 1, 0, 2, 2, 64, 0, 0, False, 3, 0)),
    ((0, 2, 4, 4, 128, 100, 1, 0, 1, 1, 1, 0), {}, (0, 1, 1, 0, 2, 2, 64, 0, 0, True, 1, 0)),
    ((0, 9, 4, 16, 64, 160, 2, 1, 1, 1, 1, 0), {}, (0, 1, 1, 0, 2, 2, 64, 0, 0, True, 2, 0)),
    ((0, 2, 8, 256, 64, 32, 2, 1, 1, 1, 1, 0), {}, (0, 1, 1, 0, 2, 2, 64, 0, 0, True, 3, 0)),
    ((0, 2, 8, 256, 64, 32, 2, 1, 1, 1, 1, 1), {"splitk": 1}, (0, 1, 1, 1, 2, 2, 64, 0, 0, False, 3, 0)),
    ((0, 2, 4, 4, 128, 100, 1, 0, 1, 1, 1, 1), {}, (0, 1, 1, 1, 2, 2, 64, 0, 0, True, 1, 0)),
    ((0, 2, 8, 256, 64, 32, 2, 1, 1, 1, 1, 1), {}, (0, 1, 1, 1, 2, 2, 64, 0, 0, True, 3, 0)),
    ((0, 2, 16, 256, 64, 192, 2, 1, 1, 1, 1, 1), {"splitk": 1}, (0, 1, 1, 1, 2, 2, 64, 1, 0, False, 1, 0)),
    ((0, 9, 4, 32, 64, 192, 2, 1, 1, 1, 1, 1), {}, (0, 1, 1, 1, 2, 2, 64, 1, 0, True, 1, 0)),
    ((0, 9, 4, 32, 64, 320, 2, 1, 1, 1, 1, 1), {}, (0, 1, 1, 1, 2, 2, 64, 1, 0, True, 2, 0)),
    ((0, 2, 8, 256, 32, 160, 2, 1, 2, 1, 0, 0), {"splitk": 1}, (0, 2, 0, 0, 2, 2, 16, 0, 0, False, 1, 0)),
    ((0, 2, 8, 256, 32, 32, 2, 1, 2, 1, 0, 0), {"splitk": 1}, (0, 2, 0, 0, 2, 2, 16, 0, 0, False, 3, 0)),
    ((0, 2, 4, 4, 32, 100, 1, 0, 2, 1, 0, 0), {}, (0, 2, 0, 0, 2, 2, 16, 0, 0, True, 1, 0)),
    ((0, 9, 4, 16, 32, 160, 2, 1, 2, 1, 0, 0), {}, (0, 2, 0, 0, 2, 2, 16, 0, 0, True, 2, 0)),
    ((0, 2, 8, 256, 32, 32, 2, 1, 2, 1, 0, 0), {}, (0, 2, 0, 0, 2, 2, 16, 0, 0, True, 3, 0)),
    ((0, 2, 16, 256, 32, 192, 2, 1, 2, 1, 3, 3), {"splitk": 1}, (0, 2, 3, 3, 2, 4, 16, 2, 0, False, 1, 0)),
    ((0, 3, 4, 64, 32, 192, 2, 1, 2, 1, 3, 3), {}, (0, 2, 3, 3, 2, 4, 16, 2, 0, True, 1, 0)),
    ((0, 9, 4, 32, 32, 320, 2, 1, 2, 1, 3, 3), {}, (0, 2, 3, 3, 2, 4, 16, 2, 0, True, 2, 0)),
    ((1, 2, 4, 4, 96, 32, 2, 1, 0, 1, 0, 0), {}, (1, 0, 0, 0, 2, 2, 32, 0, 0, False, 0, 0)),
    ((1, 9, 4, 16, 160, 32, 2, 1, 0, 1, 0, 0), {}, (1, 0, 0, 0, 2, 2, 32, 0, 0, False, 2, 0)),
    ((1, 2, 4, 4, 96, 64, 2, 1, 0, 1, 0, 0), {}, (1, 0, 0, 0, 2, 2, 32, 0, 0, True, 0, 0)),
    ((1, 2, 16, 256, 32, 32, 2, 1, 0, 1, 0, 0), {"splitk": 1}, (1, 0, 0, 0, 4, 1, 16, 0, 0, False, 1, 0)),
    ((1, 2, 4, 4, 96, 64, 2, 1, 1, 1, 0, 0), {}, (1, 1, 0, 0, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 9, 4, 16, 160, 64, 2, 1, 1, 1, 0, 0), {}, (1, 1, 0, 0, 2, 2, 64, 0, 0, False, 2, 0)),
    ((1, 2, 4, 4, 96, 128, 2, 1, 1, 1, 0, 0), {}, (1, 1, 0, 0, 2, 2, 64, 0, 0, True, 0, 0)),
    ((1, 2, 16, 256, 32, 64, 2, 1, 1, 1, 0, 0), {"splitk": 1}, (1, 1, 0, 0, 4, 1, 32, 0, 0, False, 1, 0)),
    ((1, 2, 4, 4, 96, 64, 2, 1, 1, 1, 0, 1), {}, (1, 1, 0, 1, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 9, 4, 16, 160, 64, 2, 1, 1, 1, 0, 1), {}, (1, 1, 0, 1, 2, 2, 64, 0, 0, False, 2, 0)),
    ((1, 2, 4, 4, 96, 128, 2, 1, 1, 1, 0, 1), {}, (1, 1, 0, 1, 2, 2, 64, 0, 0, True, 0, 0)),
    ((1, 2, 16, 256, 32, 64, 2, 1, 1, 1, 0, 1), {"splitk": 1}, (1, 1, 0, 1, 4, 1, 32, 0, 0, False, 1, 0)),
    ((1, 2, 4, 4, 96, 64, 2, 1, 1, 1, 1, 0), {}, (1, 1, 1, 0, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 9, 4, 16, 160, 64, 2, 1, 1, 1, 1, 0), {}, (1, 1, 1, 0, 2, 2, 64, 0, 0, False, 2, 0)),
    ((1, 2, 4, 4, 96, 128, 2, 1, 1, 1, 1, 0), {}, (1, 1, 1, 0, 2, 2, 64, 0, 0, True, 0, 0)),
    ((1, 2, 16, 256, 32, 64, 2, 1, 1, 1, 1, 0), {"splitk": 1}, (1, 1, 1, 0, 4, 1, 32, 0, 0, False, 1, 0)),
    ((1, 2, 4, 4, 96, 64, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 2, 4, 4, 96, 128, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 2, 2, 64, 0, 0, True, 0, 0)),
    ((1, 3, 4, 64, 192, 64, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 2, 2, 64, 1, 0, False, 0, 0)),
    ((1, 3, 4, 64, 192, 128, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 2, 2, 64, 1, 0, True, 0, 0)),
    ((1, 9, 4, 32, 320, 128, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 2, 2, 64, 1, 0, True, 2, 0)),
    ((1, 2, 4, 256, 96, 64, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 2, 2, 64, 4, 2, False, "n/a", 0)),
    ((1, 8, 32, 32, 32, 64, 2, 1, 1, 1, 1, 1), {"splitk": 1}, (1, 1, 1, 1, 4, 1, 32, 0, 0, False, 1, 0)),
    ((1, 2, 4, 256, 32, 64, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 4, 1, 32, 4, 4, False, "n/a", 0)),
    ((1, 2, 4, 4, 96, 32, 2, 1, 2, 1, 0, 0), {"splitk": 1}, (1, 2, 0, 0, 2, 2, 16, 0, 0, False, 0, 0)),
    ((1, 9, 4, 16, 160, 32, 2, 1, 2, 1, 0, 0), {"splitk": 1}, (1, 2, 0, 0, 2, 2, 16, 0, 0, False, 2, 0)),
    ((1, 2, 4, 4, 96, 32, 2, 1, 2, 1, 0, 0), {}, (1, 2, 0, 0, 2, 2, 16, 0, 0, True, 0, 0)),
    ((1, 2, 16, 256, 32, 32, 2, 1, 2, 1, 0, 0), {"splitk": 1}, (1, 2, 0, 0, 4, 1, 16, 0, 0, False, 1, 0)),
    ((1, 2, 4, 256, 96, 32, 2, 1, 2, 1, 3, 3), {}, (1, 2, 3, 3, 2, 2, 16, 3, 2, False, "n/a", 0)),
    ((1, 3, 4, 64, 192, 32, 2, 1, 2, 1, 3, 3), {"splitk": 1}, (1, 2, 3, 3, 2, 4, 16, 2, 0, False, 0, 0)),
    ((1, 3, 4, 64, 192, 32, 2, 1, 2, 1, 3, 3), {}, (1, 2, 3, 3, 2, 4, 16, 2, 0, True, 0, 0)),
    ((1, 9, 4, 32, 320, 32, 2, 1, 2, 1, 3, 3), {}, (1, 2, 3, 3, 2, 4, 16, 2, 0, True, 2, 0)),
    ((1, 2, 4, 256, 32, 32, 2, 1, 2, 1, 3, 3), {}, (1, 2, 3, 3, 4, 1, 16, 3, 4, False, "n/a", 0)),
    ((1, 2, 4, 4, 32, 100, 1, 0, 0, 1, 0, 0), {}, (2, 0, 0, 0, 2, 2, 32, 0, 0, False, 0, 0)),
    ((1, 2, 4, 4, 32, 100, 1, 0, 1, 1, 0, 0), {}, (2, 1, 0, 0, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 2, 4, 4, 32, 100, 1, 0, 1, 1, 0, 1), {}, (2, 1, 0, 1, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 2, 4, 4, 32, 100, 1, 0, 2, 1, 0, 0), {}, (2, 2, 0, 0, 2, 2, 16, 0, 0, False, 0, 0)),
    ((2, 2, 4, 4, 32, 100, 1, 0, 0, 1, 0, 0), {}, (3, 0, 0, 0, 2, 2, 16, 0, 0, False, 0, 0)),
    ((2, 2, 4, 4, 32, 1024, 2, 1, 0, 1, 0, 0), {}, (3, 0, 0, 0, 2, 2, 16, 0, 0, False, 1, 0)),
    ((2, 2, 4, 64, 32, 32, 2, 1, 0, 1, 0, 0), {}, (3, 0, 0, 0, 2, 2, 16, 0, 0, True, 0, 0)),
    ((2, 2, 4, 256, 32, 32, 2, 1, 0, 1, 0, 0), {}, (3, 0, 0, 0, 2, 2, 16, 0, 0, True, 1, 0)),
    ((2, 2, 4, 4, 32, 100, 1, 0, 1, 1, 0, 0), {}, (3, 1, 0, 0, 2, 2, 64, 0, 0, False, 0, 0)),
    ((2, 2, 4, 4, 32, 1024, 2, 1, 1, 1, 0, 0), {}, (3, 1, 0, 0, 2, 2, 64, 0, 0, False, 1, 0)),
    ((2, 2, 16, 256, 32, 32, 2, 1, 1, 1, 0, 0), {}, (3, 1, 0, 0, 2, 2, 64, 0, 0, True, 1, 0)),
    ((2, 2, 4, 4, 32, 100, 1, 0, 1, 1, 0, 1), {}, (3, 1, 0, 1, 2, 2, 64, 0, 0, False, 0, 0)),
    ((2, 2, 4, 4, 32, 1024, 2, 1, 1, 1, 0, 1), {}, (3, 1, 0, 1, 2, 2, 64, 0, 0, False, 1, 0)),
    ((2, 2, 16, 256, 32, 32, 2, 1, 1, 1, 0, 1), {}, (3, 1, 0, 1, 2, 2, 64, 0, 0, True, 1, 0)),
    ((2, 2, 4, 4, 32, 1024, 2, 1, 1, 1, 1, 0), {}, (3, 1, 1, 0, 2, 2, 64, 0, 0, False, 1, 0)),
    ((2, 2, 16, 256, 32, 32, 2, 1, 1, 1, 1, 0), {}, (3, 1, 1, 0, 2, 2, 64, 0, 0, True, 1, 0)),
    ((2, 2, 16, 256, 32, 32, 2, 1, 1, 1, 1, 1), {}, (3, 1, 1, 1, 2, 2, 64, 0, 0, True, 1, 0)),
    ((2, 2, 4, 4, 32, 2048, 2, 1, 1, 1, 1, 1), {}, (3, 1, 1, 1, 2, 2, 64, 1, 0, False, 1, 0)),
    ((2, 2, 8, 256, 32, 320, 2, 1, 1, 1, 1, 1), {}, (3, 1, 1, 1, 2, 2, 64, 1, 0, True, 1, 0)),
    ((2, 2, 4, 4, 32, 100, 1, 0, 2, 1, 0, 0), {}, (3, 2, 0, 0, 2, 2, 16, 0, 0, False, 0, 0)),
    ((2, 2, 4, 4, 32, 1024, 2, 1, 2, 1, 0, 0), {}, (3, 2, 0, 0, 2, 2, 16, 0, 0, False, 1, 0)),
    ((2, 2, 4, 64, 32, 32, 2, 1, 2, 1, 0, 0), {}, (3, 2, 0, 0, 2, 2, 16, 0, 0, True, 0, 0)),
    ((2, 2, 4, 256, 32, 32, 2, 1, 2, 1, 0, 0), {}, (3, 2, 0, 0, 2, 2, 16, 0, 0, True, 1, 0)),
    ((2, 2, 4, 128, 32, 160, 2, 1, 2, 1, 3, 3), {}, (3, 2, 3, 3, 1, 4, 16, 2, 0, True, 1, 0)),
    ((2, 2, 4, 4, 32, 2048, 2, 1, 2, 1, 3, 3), {}, (3, 2, 3, 3, 2, 4, 16, 2, 0, False, 1, 0)),
    ((2, 2, 4, 128, 32, 320, 2, 1, 2, 1, 3, 3), {}, (3, 2, 3, 3, 2, 4, 16, 2, 0, True, 1, 0)),
]

# MORE_CASES: further cases of the same signatures (three per signature at the most, PLAN_CASES' one included).
# The weight-dominated tile order with split-K (xcd_group 2) at five images of 16 x 16: two or three row tiles, two to four column tiles.
MORE_CASES = [
    ((0, 5, 16, 16, 64, 384, 2, 1, 0, 1, 0, 0), {}, (0, 0, 0, 0, 2, 2, 32, 0, 0, True, 2, 0)),
    ((0, 5, 16, 16, 64, 384, 2, 1, 2, 1, 0, 0), {}, (0, 2, 0, 0, 2, 2, 16, 0, 0, True, 2, 0)),
    ((0, 5, 16, 16, 64, 384, 2, 1, 2, 1, 3, 3), {}, (0, 2, 3, 3, 2, 4, 16, 2, 0, True, 2, 0)),
    ((0, 5, 16, 16, 64, 384, 2, 1, 1, 1, 1, 1), {}, (0, 1, 1, 1, 2, 2, 64, 1, 0, True, 2, 0)),
    ((1, 5, 16, 16, 512, 64, 2, 1, 2, 1, 3, 3), {}, (1, 2, 3, 3, 2, 4, 16, 2, 0, True, 2, 0)),
    ((1, 5, 16, 16, 512, 128, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 2, 2, 64, 1, 0, True, 2, 0)),
]

# A second case per signature, from the same search with another aim: among the shapes of at most the largest first case's work, the
# one that leaves the fewest of these untouched -- two or more row tiles (sixteen where each XCD takes a block of them: xcd_group 3)
# and column tiles, a ragged last row tile and column tile, four or more K-tiles per split, a ragged last split, an odd batch, and
# two or more rounds of eight (row tile, split) pairs where the order deals them out (xcd_group 1) -- and of those the least work.
# A first case is often one tile, one K-tile or one image row, which reaches the code and little of its indexing.
MORE_CASES += [
    ((0, 3, 16, 256, 32, 160, 2, 1, 0, 1, 0, 0), {"splitk": 1}, (0, 0, 0, 0, 2, 2, 32, 0, 0, False, 1, 0)),
    ((0, 3, 16, 256, 32, 32, 2, 1, 0, 1, 0, 0), {"splitk": 1}, (0, 0, 0, 0, 2, 2, 32, 0, 0, False, 3, 0)),
    ((0, 5, 4, 32, 64, 160, 2, 1, 0, 1, 0, 0), {}, (0, 0, 0, 0, 2, 2, 32, 0, 0, True, 1, 0)),
    ((0, 33, 4, 4, 32, 160, 2, 1, 0, 1, 0, 0), {}, (0, 0, 0, 0, 2, 2, 32, 0, 0, True, 2, 0)),
    ((0, 3, 16, 256, 32, 32, 2, 1, 0, 1, 0, 0), {"splitk": 3}, (0, 0, 0, 0, 2, 2, 32, 0, 0, True, 3, 0)),
    ((0, 2, 16, 256, 64, 160, 2, 1, 1, 1, 0, 0), {"splitk": 1}, (0, 1, 0, 0, 2, 2, 64, 0, 0, False, 1, 0)),
    ((0, 3, 16, 256, 64, 32, 2, 1, 1, 1, 0, 0), {"splitk": 1}, (0, 1, 0, 0, 2, 2, 64, 0, 0, False, 3, 0)),
    ((0, 5, 4, 32, 128, 160, 2, 1, 1, 1, 0, 0), {}, (0, 1, 0, 0, 2, 2, 64, 0, 0, True, 1, 0)),
    ((0, 33, 4, 4, 64, 160, 2, 1, 1, 1, 0, 0), {}, (0, 1, 0, 0, 2, 2, 64, 0, 0, True, 2, 0)),
    ((0, 3, 16, 256, 64, 32, 2, 1, 1, 1, 0, 0), {"splitk": 3}, (0, 1, 0, 0, 2, 2, 64, 0, 0, True, 3, 0)),
    ((0, 2, 16, 256, 64, 160, 2, 1, 1, 1, 0, 1), {"splitk": 1}, (0, 1, 0, 1, 2, 2, 64, 0, 0, False, 1, 0)),
    ((0, 3, 16, 256, 64, 32, 2, 1, 1, 1, 0, 1), {"splitk": 1}, (0, 1, 0, 1, 2, 2, 64, 0, 0, False, 3, 0)),
    ((0, 5, 4, 32, 128, 160, 2, 1, 1, 1, 0, 1), {}, (0, 1, 0, 1, 2, 2, 64, 0, 0, True, 1, 0)),
    ((0, 33, 4, 4, 64, 160, 2, 1, 1, 1, 0, 1), {}, (0, 1, 0, 1, 2, 2, 64, 0, 0, True, 2, 0)),
    ((0, 3, 16, 256, 64, 32, 2, 1, 1, 1, 0, 1), {"splitk": 3}, (0, 1, 0, 1, 2, 2, 64, 0, 0, True, 3, 0)),
    ((0, 2, 16, 256, 64, 160, 2, 1, 1, 1, 1, 0), {"splitk": 1}, (0, 1, 1, 0, 2, 2, 64, 0, 0, False, 1, 0)),
    ((0, 3, 16, 256, 64, 32, 2, 1, 1, 1, 1, 0), {"splitk": 1}, (0, 1, 1, 0, 2, 2, 64, 0, 0, False, 3, 0)),
    ((0, 5, 4, 32, 128, 160, 2, 1, 1, 1, 1, 0), {}, (0, 1, 1, 0, 2, 2, 64, 0, 0, True, 1, 0)),
    ((0, 33, 4, 4, 64, 160, 2, 1, 1, 1, 1, 0), {}, (0, 1, 1, 0, 2, 2, 64, 0, 0, True, 2, 0)),
    ((0, 3, 16, 256, 64, 32, 2, 1, 1, 1, 1, 0), {"splitk": 3}, (0, 1, 1, 0, 2, 2, 64, 0, 0, True, 3, 0)),
    ((0, 3, 16, 256, 64, 32, 2, 1, 1, 1, 1, 1), {"splitk": 1}, (0, 1, 1, 1, 2, 2, 64, 0, 0, False, 3, 0)),
    ((0, 5, 4, 32, 128, 160, 2, 1, 1, 1, 1, 1), {}, (0, 1, 1, 1, 2, 2, 64, 0, 0, True, 1, 0)),
    ((0, 3, 16, 256, 64, 32, 2, 1, 1, 1, 1, 1), {"splitk": 3}, (0, 1, 1, 1, 2, 2, 64, 0, 0, True, 3, 0)),
    ((0, 9, 4, 32, 128, 288, 2, 1, 1, 1, 1, 1), {}, (0, 1, 1, 1, 2, 2, 64, 1, 0, True, 1, 0)),
    ((0, 33, 4, 8, 64, 288, 2, 1, 1, 1, 1, 1), {}, (0, 1, 1, 1, 2, 2, 64, 1, 0, True, 2, 0)),
    ((0, 3, 16, 256, 32, 160, 2, 1, 2, 1, 0, 0), {"splitk": 1}, (0, 2, 0, 0, 2, 2, 16, 0, 0, False, 1, 0)),
    ((0, 3, 16, 256, 32, 32, 2, 1, 2, 1, 0, 0), {"splitk": 1}, (0, 2, 0, 0, 2, 2, 16, 0, 0, False, 3, 0)),
    ((0, 25, 4, 16, 288, 160, 2, 1, 2, 1, 0, 0), {}, (0, 2, 0, 0, 2, 2, 16, 0, 0, True, 1, 0)),
    ((0, 33, 4, 4, 288, 448, 2, 1, 2, 1, 0, 0), {}, (0, 2, 0, 0, 2, 2, 16, 0, 0, True, 2, 0)),
    ((0, 3, 16, 256, 32, 32, 2, 1, 2, 1, 0, 0), {"splitk": 3}, (0, 2, 0, 0, 2, 2, 16, 0, 0, True, 3, 0)),
    ((0, 2, 16, 256, 32, 288, 2, 1, 2, 1, 3, 3), {"splitk": 1}, (0, 2, 3, 3, 2, 4, 16, 2, 0, False, 1, 0)),
    ((0, 9, 4, 32, 32, 288, 2, 1, 2, 1, 3, 3), {}, (0, 2, 3, 3, 2, 4, 16, 2, 0, True, 1, 0)),
    ((0, 33, 4, 8, 32, 288, 2, 1, 2, 1, 3, 3), {}, (0, 2, 3, 3, 2, 4, 16, 2, 0, True, 2, 0)),
    ((1, 5, 4, 32, 160, 32, 2, 1, 0, 1, 0, 0), {}, (1, 0, 0, 0, 2, 2, 32, 0, 0, False, 0, 0)),
    ((1, 33, 4, 4, 160, 32, 2, 1, 0, 1, 0, 0), {}, (1, 0, 0, 0, 2, 2, 32, 0, 0, False, 2, 0)),
    ((1, 5, 4, 32, 160, 128, 2, 1, 0, 1, 0, 0), {"splitk": 3}, (1, 0, 0, 0, 2, 2, 32, 0, 0, True, 0, 0)),
    ((1, 3, 32, 256, 32, 32, 2, 1, 0, 1, 0, 0), {"splitk": 1}, (1, 0, 0, 0, 4, 1, 16, 0, 0, False, 1, 0)),
    ((1, 5, 4, 32, 160, 64, 2, 1, 1, 1, 0, 0), {}, (1, 1, 0, 0, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 33, 4, 4, 160, 64, 2, 1, 1, 1, 0, 0), {}, (1, 1, 0, 0, 2, 2, 64, 0, 0, False, 2, 0)),
    ((1, 5, 4, 32, 160, 256, 2, 1, 1, 1, 0, 0), {"splitk": 3}, (1, 1, 0, 0, 2, 2, 64, 0, 0, True, 0, 0)),
    ((1, 3, 32, 256, 32, 64, 2, 1, 1, 1, 0, 0), {"splitk": 1}, (1, 1, 0, 0, 4, 1, 32, 0, 0, False, 1, 0)),
    ((1, 5, 4, 32, 160, 64, 2, 1, 1, 1, 0, 1), {}, (1, 1, 0, 1, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 33, 4, 4, 160, 64, 2, 1, 1, 1, 0, 1), {}, (1, 1, 0, 1, 2, 2, 64, 0, 0, False, 2, 0)),
    ((1, 5, 4, 32, 160, 256, 2, 1, 1, 1, 0, 1), {"splitk": 3}, (1, 1, 0, 1, 2, 2, 64, 0, 0, True, 0, 0)),
    ((1, 3, 32, 256, 32, 64, 2, 1, 1, 1, 0, 1), {"splitk": 1}, (1, 1, 0, 1, 4, 1, 32, 0, 0, False, 1, 0)),
    ((1, 5, 4, 32, 160, 64, 2, 1, 1, 1, 1, 0), {}, (1, 1, 1, 0, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 33, 4, 4, 160, 64, 2, 1, 1, 1, 1, 0), {}, (1, 1, 1, 0, 2, 2, 64, 0, 0, False, 2, 0)),
    ((1, 5, 4, 32, 160, 256, 2, 1, 1, 1, 1, 0), {"splitk": 3}, (1, 1, 1, 0, 2, 2, 64, 0, 0, True, 0, 0)),
    ((1, 3, 32, 256, 32, 64, 2, 1, 1, 1, 1, 0), {"splitk": 1}, (1, 1, 1, 0, 4, 1, 32, 0, 0, False, 1, 0)),
    ((1, 5, 4, 32, 160, 64, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 5, 4, 32, 160, 256, 2, 1, 1, 1, 1, 1), {"splitk": 3}, (1, 1, 1, 1, 2, 2, 64, 0, 0, True, 0, 0)),
    ((1, 9, 4, 32, 288, 64, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 2, 2, 64, 1, 0, False, 0, 0)),
    ((1, 9, 4, 32, 288, 256, 2, 1, 1, 1, 1, 1), {"splitk": 3}, (1, 1, 1, 1, 2, 2, 64, 1, 0, True, 0, 0)),
    ((1, 33, 4, 8, 288, 256, 2, 1, 1, 1, 1, 1), {"splitk": 3}, (1, 1, 1, 1, 2, 2, 64, 1, 0, True, 2, 0)),
    ((1, 3, 4, 256, 96, 128, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 2, 2, 64, 4, 2, False, "n/a", 0)),
    ((1, 16, 32, 32, 32, 64, 2, 1, 1, 1, 1, 1), {"splitk": 1}, (1, 1, 1, 1, 4, 1, 32, 0, 0, False, 1, 0)),
    ((1, 3, 4, 256, 32, 128, 2, 1, 1, 1, 1, 1), {}, (1, 1, 1, 1, 4, 1, 32, 4, 4, False, "n/a", 0)),
    ((1, 5, 4, 32, 160, 32, 2, 1, 2, 1, 0, 0), {"splitk": 1}, (1, 2, 0, 0, 2, 2, 16, 0, 0, False, 0, 0)),
    ((1, 33, 4, 4, 160, 32, 2, 1, 2, 1, 0, 0), {"splitk": 1}, (1, 2, 0, 0, 2, 2, 16, 0, 0, False, 2, 0)),
    ((1, 5, 4, 32, 160, 64, 2, 1, 2, 1, 0, 0), {"splitk": 3}, (1, 2, 0, 0, 2, 2, 16, 0, 0, True, 0, 0)),
    ((1, 3, 32, 256, 32, 32, 2, 1, 2, 1, 0, 0), {"splitk": 1}, (1, 2, 0, 0, 4, 1, 16, 0, 0, False, 1, 0)),
    ((1, 3, 4, 256, 96, 64, 2, 1, 2, 1, 3, 3), {}, (1, 2, 3, 3, 2, 2, 16, 3, 2, False, "n/a", 0)),
    ((1, 9, 4, 32, 288, 32, 2, 1, 2, 1, 3, 3), {"splitk": 1}, (1, 2, 3, 3, 2, 4, 16, 2, 0, False, 0, 0)),
    ((1, 9, 4, 32, 288, 64, 2, 1, 2, 1, 3, 3), {"splitk": 3}, (1, 2, 3, 3, 2, 4, 16, 2, 0, True, 0, 0)),
    ((1, 33, 4, 8, 288, 64, 2, 1, 2, 1, 3, 3), {"splitk": 3}, (1, 2, 3, 3, 2, 4, 16, 2, 0, True, 2, 0)),
    ((1, 3, 4, 256, 32, 64, 2, 1, 2, 1, 3, 3), {}, (1, 2, 3, 3, 4, 1, 16, 3, 4, False, "n/a", 0)),
    ((1, 3, 4, 4, 32, 100, 1, 0, 0, 1, 0, 0), {}, (2, 0, 0, 0, 2, 2, 32, 0, 0, False, 0, 0)),
    ((1, 3, 4, 4, 32, 100, 1, 0, 1, 1, 0, 0), {}, (2, 1, 0, 0, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 3, 4, 4, 32, 100, 1, 0, 1, 1, 0, 1), {}, (2, 1, 0, 1, 2, 2, 64, 0, 0, False, 0, 0)),
    ((1, 3, 4, 4, 32, 100, 1, 0, 2, 1, 0, 0), {}, (2, 2, 0, 0, 2, 2, 16, 0, 0, False, 0, 0)),
    ((2, 13, 4, 4, 32, 160, 2, 1, 0, 1, 0, 0), {}, (3, 0, 0, 0, 2, 2, 16, 0, 0, False, 0, 0)),
    ((2, 13, 4, 4, 32, 2048, 2, 1, 0, 1, 0, 0), {}, (3, 0, 0, 0, 2, 2, 16, 0, 0, False, 1, 0)),
    ((2, 33, 4, 4, 32, 160, 2, 1, 0, 1, 0, 0), {}, (3, 0, 0, 0, 2, 2, 16, 0, 0, True, 0, 0)),
    ((2, 33, 4, 8, 32, 448, 2, 1, 0, 1, 0, 0), {}, (3, 0, 0, 0, 2, 2, 16, 0, 0, True, 1, 0)),
    ((2, 25, 4, 8, 32, 160, 2, 1, 1, 1, 0, 0), {}, (3, 1, 0, 0, 2, 2, 64, 0, 0, False, 0, 0)),
    ((2, 25, 4, 8, 32, 2048, 2, 1, 1, 1, 0, 0), {}, (3, 1, 0, 0, 2, 2, 64, 0, 0, False, 1, 0)),
    ((2, 33, 4, 32, 32, 448, 2, 1, 1, 1, 0, 0), {}, (3, 1, 0, 0, 2, 2, 64, 0, 0, True, 1, 0)),
    ((2, 25, 4, 8, 32, 160, 2, 1, 1, 1, 0, 1), {}, (3, 1, 0, 1, 2, 2, 64, 0, 0, False, 0, 0)),
    ((2, 25, 4, 8, 32, 2048, 2, 1, 1, 1, 0, 1), {}, (3, 1, 0, 1, 2, 2, 64, 0, 0, False, 1, 0)),
    ((2, 33, 4, 32, 32, 448, 2, 1, 1, 1, 0, 1), {}, (3, 1, 0, 1, 2, 2, 64, 0, 0, True, 1, 0)),
    ((2, 25, 4, 8, 32, 2048, 2, 1, 1, 1, 1, 0), {}, (3, 1, 1, 0, 2, 2, 64, 0, 0, False, 1, 0)),
    ((2, 33, 4, 32, 32, 448, 2, 1, 1, 1, 1, 0), {}, (3, 1, 1, 0, 2, 2, 64, 0, 0, True, 1, 0)),
    ((2, 33, 4, 32, 32, 160, 2, 1, 1, 1, 1, 1), {}, (3, 1, 1, 1, 2, 2, 64, 0, 0, True, 1, 0)),
    ((2, 25, 4, 8, 32, 2048, 2, 1, 1, 1, 1, 1), {}, (3, 1, 1, 1, 2, 2, 64, 1, 0, False, 1, 0)),
    ((2, 33, 4, 32, 32, 288, 2, 1, 1, 1, 1, 1), {}, (3, 1, 1, 1, 2, 2, 64, 1, 0, True, 1, 0)),
    ((2, 13, 4, 4, 32, 160, 2, 1, 2, 1, 0, 0), {}, (3, 2, 0, 0, 2, 2, 16, 0, 0, False, 0, 0)),
    ((2, 13, 4, 4, 32, 2048, 2, 1, 2, 1, 0, 0), {}, (3, 2, 0, 0, 2, 2, 16, 0, 0, False, 1, 0)),
    ((2, 33, 4, 4, 32, 160, 2, 1, 2, 1, 0, 0), {}, (3, 2, 0, 0, 2, 2, 16, 0, 0, True, 0, 0)),
    ((2, 33, 4, 8, 32, 448, 2, 1, 2, 1, 0, 0), {}, (3, 2, 0, 0, 2, 2, 16, 0, 0, True, 1, 0)),
    ((2, 33, 4, 8, 32, 160, 2, 1, 2, 1, 3, 3), {}, (3, 2, 3, 3, 1, 4, 16, 2, 0, True, 1, 0)),
    ((2, 13, 4, 4, 32, 2048, 2, 1, 2, 1, 3, 3), {}, (3, 2, 3, 3, 2, 4, 16, 2, 0, False, 1, 0)),
    ((2, 33, 4, 8, 32, 288, 2, 1, 2, 1, 3, 3), {}, (3, 2, 3, 3, 2, 4, 16, 2, 0, True, 1, 0)),
]

# The smallest case of a finding these cases made: a forward cut into more than sixteen K-slabs (24 here) whose output is small enough
# for the lane-order reduction kernel.  Asked for fused statistics, the same call went through the statistics reduction, which sums
# in slab order: the output's last bits depended on whether statistics were asked for (csrc/igemm.hip run_plan: one order per such plan now).
MORE_CASES += [
    ((0, 2, 4, 4, 192, 32, 2, 1, 0, 1, 0, 0), {}, (0, 0, 0, 0, 2, 2, 32, 0, 0, True, 1, 0)),
]

# conditions on a case, not measurements: twice the largest case of the list (0.81 GFLOP, 21.8 MiB)
MAX_WORK = 2 * 805306368
MAX_BYTES = 2 * 22821888
ALL_CASES = PLAN_CASES + MORE_CASES


def case_id(case):
    req, opts, _ = case
    return "op{}-n{}-{}x{}-c{}-k{}-s{}-p{}a{}b{}".format(*req[:7], *req[8:9], *req[10:]) + "".join(f"-{k}{v}" for k, v in sorted(opts.items()))


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_case_reaches_its_signature(case):
    req, opts, want = case
    assert set(opts) <= set(CASE_OPTIONS), f"a case may set {CASE_OPTIONS} only"
    f = describe(req, opts)
    assert f is not None, "no plan"
    assert signature(f) == want, dict(f)
    assert refused(req[0], req[4], req[5], req[6], req[8], req[10], req[11], f) is None


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_case_is_small(case):
    req, opts, _ = case
    f = describe(req, opts)
    assert conv_work(f, req) <= MAX_WORK, conv_work(f, req)
    assert case_bytes(f, req, opts) <= MAX_BYTES, case_bytes(f, req, opts)


def test_every_model_signature_has_a_case():
    """PLAN_CASES: one case for every signature a model layer gets and for nothing else.  MORE_CASES: signatures of model layers only."""
    sigs = [c[2] for c in PLAN_CASES]
    assert len(set(sigs)) == len(sigs), "PLAN_CASES holds one case per signature; further ones belong in MORE_CASES"
    layers = {}
    for name, req, plan in model_requests():
        layers.setdefault(signature(plan), []).append(name)
    missing = {s: n for s, n in layers.items() if s not in set(sigs)}
    assert not missing, "model layers whose plan no case checks:\n" + "\n".join(
        f"  {s}: {len(n)} launches, e.g. {'; '.join(n[:4])}" for s, n in sorted(missing.items(), key=str))
    idle = [case_id(c) for c in ALL_CASES if c[2] not in layers]
    assert not idle, f"cases whose plan no model layer gets: {idle}"


def test_no_signature_has_more_than_three_cases():
    count = {}
    for _, _, s in ALL_CASES:
        count[s] = count.get(s, 0) + 1
    assert all(v <= 3 for v in count.values()), {s: v for s, v in count.items() if v > 3}
