"""Tensor-level wrappers over the C ABI (device pointers + sizes; torch only supplies memory/streams).

Layout conventions (see include/discogan_hip.h):
  * interior activations: logical [N,C,H,W] tensors whose MEMORY is NHWC (torch channels_last);
  * image side (3 channels): plain contiguous NCHW;
  * Conv2d weight logical [K,C,4,4] stored KRSC; ConvTranspose2d weight logical [Cin,Cout,4,4] stored
    [Cin,4,4,Cout]; 3-channel edge weights stay logically contiguous.
"""
from __future__ import annotations

import collections
import ctypes
import os

import torch

from . import _lib

ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3
PREC_DEFAULT, PREC_F32, PREC_BF16, PREC_F32X3 = -1, 0, 1, 2      # include/discogan_hip.h DG_PREC_*


class Context:
    """The arithmetic and operand-form settings ONE caller (a trainer, a test) runs its ops under -- a per-caller object instead
    of process-wide switches ("dtype enum" per call, "no global mutable state").

      prec    arithmetic of the conv products, passed to the C ABI with EVERY call (DG_PREC_F32 | _BF16 | _F32X3); None = the
              library's process default (dg_set_option("bf16"): tools and op tests that flip it around single calls)
      shadow  bf16 path: conv kernels read bf16 shadows written by the producers (see "bf16 shadow operands" below)
      act16   bf16 path: feature maps and their gradients exist only as bf16
      x3      f32x3 path: conv kernels read plane triples written once per tensor
      shadow_tab / plane_tab: the derived copies of this caller's live activations

    ``with ops.use(ctx):`` makes it the ambient context of the forward calls issued inside; every autograd Function remembers the
    context of its forward and runs its backward under it (functional._fwd / _bwd), so two trainers with different arithmetic can be
    interleaved call by call in one process."""

    def __init__(self, prec=None, shadow=False, act16=False, x3=False, group_plan="launch"):
        self.prec = prec
        self.group_plan = group_plan           # grouped conv launches: split-K planned for the whole "launch" or per "single" problem
        self.shadow, self.act16, self.x3 = bool(shadow), bool(act16), bool(x3)
        self.shadow_tab, self.plane_tab = {}, {}

    @property
    def cprec(self):
        return PREC_DEFAULT if self.prec is None else int(self.prec)

    def clear(self):
        self.shadow_tab.clear()
        self.plane_tab.clear()


_AMBIENT = Context()          # what module-level ops.SHADOW / ops.ACT16 / ops.X3 read and write outside any ``use`` block
_CUR = _AMBIENT


def current():
    return _CUR


class use:
    """Context manager: run the ops issued inside under ``ctx``."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        global _CUR
        self.prev = _CUR
        _CUR = self.ctx
        return self.ctx

    def __exit__(self, *exc):
        global _CUR
        _CUR = self.prev
        return False

# bench.py's roofline leg sets this to a list: every launch of the MFMA implicit-GEMM family then
# appends (op, algorithmic FLOPs, start event, end event), recorded on the launch stream.
PROFILE = None
# Same hook for the HBM-bound kernel families: (family, algorithmic bytes, start event, end event).
PROFILE_HBM = None


class _timed:
    """``with _prof(name, flops):`` / ``with _hbm(name, nbytes):`` -- one record per block into the sink, when the sink is a list."""

    def __init__(self, sink, name, amount):
        self.sink = sink
        if sink is not None:
            self.name, self.amount = name, amount
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        if self.sink is not None:
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.sink is not None:
            self.e1.record()
            self.sink.append((self.name, self.amount, self.e0, self.e1))
        return False


_UNTIMED = _timed(None, None, None)                   # (the hooks are off in training: no object per launch then)


def _prof(name, flops):
    return _UNTIMED if PROFILE is None else _timed(PROFILE, name, flops)


def _hbm(name, nbytes):
    return _UNTIMED if PROFILE_HBM is None else _timed(PROFILE_HBM, name, nbytes)


def _env_flag(name, default):
    """A switch from the environment: one that is on by default is turned off by "0", one that is off by default is turned on by "1"."""
    v = os.environ.get(name)
    return v != "0" if default else v == "1"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


_TAB_TYPES = {}


def _tab(ts):
    """Pointer table of a grouped C-ABI call: one device pointer per problem (None entries allowed)."""
    if ts is None:
        return None
    n = len(ts)
    table = _TAB_TYPES.get(n) or _TAB_TYPES.setdefault(n, ctypes.c_void_p * n)
    return table(*[(t.data_ptr() if t is not None else None) for t in ts])


def _check_dev(*ts, allow16=False, planes_ok=False):
    """fp32 HIP tensors only.  allow16: the wrapper dispatches on the storage type itself (bf16 activation storage: the
    ``*_t`` / ``*_mixed`` entry points); every other wrapper calls an fp32-only kernel with numel() elements, where a bf16
    tensor would be read as floats past its end -- refused here instead."""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.DiscoganHipError(
                "discogan_modernized_amd ops need CUDA/HIP tensors (no CPU fallback exists); got a CPU tensor")
        if t.dtype != torch.float32 and not (allow16 and t.dtype == torch.bfloat16):
            raise _lib.DiscoganHipError(("fp32 or bf16" if allow16 else "fp32") + f" tensors required, got {t.dtype}")
        if not planes_ok and getattr(t, "_dg_planes_only", False):
            raise _lib.DiscoganHipError("this tensor exists only as its plane triple (ops.X3_PLANES_ONLY): its fp32 memory was never "
                                        "written and this op would read it")


# ---- layout helpers -------------------------------------------------------------------------------------
def empty_nhwc(n, c, h, w, device, dtype=torch.float32):
    """Logical [n,c,h,w] tensor backed by NHWC memory."""
    return torch.empty((n, h, w, c), device=device, dtype=dtype).permute(0, 3, 1, 2)


# bf16 ACTIVATION STORAGE (DiscoGANTrainer(mfma_dtype="bf16", act_dtype="bf16")): with ACT16 on, every feature map and
# feature-map gradient an op produces is a bf16 tensor (channel counts that are multiples of 8; the [N,100] bottleneck and
# everything image-shaped stay fp32), and the ops take bf16 tensors as they come -- there is no fp32 copy to shadow.
def _is16(t):
    return t is not None and t.dtype == torch.bfloat16


def _act_dtype(channels):
    return torch.bfloat16 if (_CUR.act16 and channels % 8 == 0) else torch.float32


def is_nhwc(x):
    """Is the memory of the logical [N,C,H,W] tensor NHWC?  (x.permute(0, 2, 3, 1).is_contiguous() without building the view: every
    conv call asks twice.  An empty tensor counts as it does there.)"""
    return x.dim() == 4 and (x.is_contiguous(memory_format=torch.channels_last) or x.numel() == 0)


def as_nhwc(x):
    """Return x (logical NCHW) with NHWC memory; converts with the library's own transpose kernel."""
    if is_nhwc(x):
        return x
    _check_dev(x)
    if x.dtype != torch.float32:
        raise _lib.DiscoganHipError("bf16 activations must already have NHWC memory")
    xc = x.contiguous()
    n, c, h, w = xc.shape
    y = empty_nhwc(n, c, h, w, x.device)
    _lib.check(_lib.load().dg_nchw_to_nhwc(_ptr(xc), _ptr(y), n, c, h, w, _stream()), "dg_nchw_to_nhwc")
    return y


def to_nchw_contiguous(x):
    """Logical NCHW tensor with plain contiguous memory (for export / comparisons)."""
    if x.is_contiguous():
        return x
    if is_nhwc(x):
        n, c, h, w = x.shape
        y = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
        _lib.check(_lib.load().dg_nhwc_to_nchw(_ptr(x), _ptr(y), n, c, h, w, _stream()), "dg_nhwc_to_nchw")
        return y
    return x.contiguous()


def u8hwc_to_f32chw(x_u8, bgr=False):
    """uint8 [N,H,W,3] (decoded image rows) -> float32 contiguous NCHW [N,3,H,W] = pixel / 255 (dataset.py:65-66)."""
    if not x_u8.is_cuda or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3:
        raise _lib.DiscoganHipError("u8hwc_to_f32chw needs a uint8 HIP tensor of shape [N,H,W,3]")
    x = x_u8.contiguous()
    n, h, w, _ = x.shape
    y = torch.empty((n, 3, h, w), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().dg_u8hwc_to_f32chw(_ptr(x), _ptr(y), n, h, w, int(bool(bgr)), _stream()), "dg_u8hwc_to_f32chw")
    return y


AUG_FLIP, AUG_CROP = 1, 2      # DG_AUG_* of include/discogan_hip.h


def check_aug_table(recs, n, who):
    """A record table as the augmentation kernels take it: int32 [m, 4] (ox, oy, flip, 0) on the device, contiguous, m >= n."""
    if not (recs.is_cuda and recs.dtype == torch.int32 and recs.dim() == 2 and recs.shape[1] == 4 and recs.is_contiguous()):
        raise _lib.DiscoganHipError(f"{who} needs a contiguous int32 HIP record table of shape [n, 4]")
    if recs.shape[0] < n:
        raise _lib.DiscoganHipError(f"{who}: the record table has {recs.shape[0]} rows for {n} samples")


def augment_draw(seed, rank, iteration, domain, n, S, L, flags, out=None, device="cuda"):
    """The augmentation records of one batch: int32 [n, 4] = (ox, oy, flip, 0) per position, drawn ON THE DEVICE as a pure function of
    (seed, rank, iteration, domain 0 = A | 1 = B, position) -- dg_augment_draw; include/discogan_hip.h defines the generator.
    ``out``: a table of at least n rows to fill (rows from n on stay as they are)."""
    if out is None:
        out = torch.empty((n, 4), device=device, dtype=torch.int32)
    check_aug_table(out, n, "augment_draw")
    _lib.check(_lib.load().dg_augment_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank), int(iteration), int(domain), int(n), int(S), int(L),
                                           int(flags), _ptr(out), _stream()), "dg_augment_draw")
    return out[:n]


def augment_f32(x, L, recs):
    """Float NCHW batch [n,3,S,S] -> [n,3,S,S]: bilinear resize to L x L (dg_image_prep's sampling, float arithmetic), the S x S window at
    the record's (ox, oy), mirrored when its flip is set -- one launch (dg_augment_f32).  L = S with zero records returns x bitwise."""
    _check_dev(x)
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or not x.is_contiguous():
        raise _lib.DiscoganHipError(f"augment_f32 needs a contiguous [n,3,S,S] batch, got {tuple(x.shape)}")
    n, S = int(x.shape[0]), int(x.shape[3])
    check_aug_table(recs, n, "augment_f32")
    out = torch.empty_like(x)
    _lib.check(_lib.load().dg_augment_f32(_ptr(x), _ptr(out), n, S, int(L), _ptr(recs), _stream()), "dg_augment_f32")
    return out


POOL_MAX_BATCH = 4096          # samples per pool batch (dg_pool_draw scans the batch in every thread)


def check_pool_table(recs, n, who):
    """A record table as the pool kernels take it: int32 [m, 4] (src, slot, st_src, 0) on the device, contiguous, m >= n."""
    if not (recs.is_cuda and recs.dtype == torch.int32 and recs.dim() == 2 and recs.shape[1] == 4 and recs.is_contiguous()):
        raise _lib.DiscoganHipError(f"{who} needs a contiguous int32 HIP record table of shape [n, 4]")
    if recs.shape[0] < n:
        raise _lib.DiscoganHipError(f"{who}: the record table has {recs.shape[0]} rows for {n} samples")


def pool_draw(seed, rank, iteration, domain, n, P, filled, out=None, device="cuda"):
    """The image-pool records of one batch: int32 [n, 4] = (src, slot, st_src, 0) per position, the in-order semantics of a pool of P slots
    with ``filled`` in use resolved ON THE DEVICE as a pure function of (seed, rank, iteration, domain 0 = A | 1 = B, position) --
    dg_pool_draw; include/discogan_hip.h defines the draw and the record rule.  ``out``: a table of at least n rows to fill (rows from n on
    stay as they are).  The caller advances ``filled`` to min(P, filled + n)."""
    if out is None:
        out = torch.empty((n, 4), device=device, dtype=torch.int32)
    check_pool_table(out, n, "pool_draw")
    _lib.check(_lib.load().dg_pool_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank), int(iteration), int(domain), int(n), int(P), int(filled),
                                        _ptr(out), _stream()), "dg_pool_draw")
    return out[:n]


def pool_exchange(x, pool, recs, out=None):
    """Apply a record table to a batch ``x`` [n, ...] and a pool [P, ...] of images of the same shape, in ONE launch (dg_pool_exchange):
    ``out[j] = pool[slot] if src == -1 else x[src]``, and where ``slot >= 0`` then ``pool[slot] = x[st_src]``.  Returns ``out`` (a new
    tensor like x unless given); the pool is updated in place, x is only read.  A copy: every bit pattern survives."""
    _check_dev(x, pool, out)
    if x.dim() < 2 or pool.dim() != x.dim() or tuple(pool.shape[1:]) != tuple(x.shape[1:]) or not (x.is_contiguous() and pool.is_contiguous()):
        raise _lib.DiscoganHipError(f"pool_exchange needs a contiguous batch [n, ...] and pool [P, ...] of one image shape, got "
                                    f"{tuple(x.shape)} and {tuple(pool.shape)}")
    n, P = int(x.shape[0]), int(pool.shape[0])
    if n < 1 or P < 1 or x[0].numel() < 1:
        raise _lib.DiscoganHipError(f"pool_exchange: empty batch, pool or image ({tuple(x.shape)}, {tuple(pool.shape)})")
    check_pool_table(recs, n, "pool_exchange")
    if out is None:
        out = torch.empty_like(x)
    elif tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
        raise _lib.DiscoganHipError(f"pool_exchange: out must be contiguous and shaped like x, got {tuple(out.shape)}")
    elems = x[0].numel()
    _lib.check(_lib.load().dg_pool_exchange(_ptr(x), _ptr(pool), _ptr(out), n, P, elems, _ptr(recs), _stream()), "dg_pool_exchange")
    return out


DIFFAUG_COLOR, DIFFAUG_TRANSLATION, DIFFAUG_CUTOUT = 1, 2, 4      # DG_DIFFAUG_* of include/discogan_hip.h
DIFFAUG_MAX_BATCH = 4096       # samples per batch of the differentiable-augmentation kernels


def check_diffaug_table(recs, n, who):
    """A record table as the differentiable-augmentation kernels take it: int32 [m, 8] (tx, ty, cx0, cy0, bits(b), bits(s), bits(c), 0)
    on the device, contiguous, m >= n."""
    if not (recs.is_cuda and recs.dtype == torch.int32 and recs.dim() == 2 and recs.shape[1] == 8 and recs.is_contiguous()):
        raise _lib.DiscoganHipError(f"{who} needs a contiguous int32 HIP record table of shape [n, 8]")
    if recs.shape[0] < n:
        raise _lib.DiscoganHipError(f"{who}: the record table has {recs.shape[0]} rows for {n} samples")


def diffaug_draw(seed, rank, iteration, domain, role, n, S, flags, out=None, device="cuda"):
    """The differentiable-augmentation records of one batch: int32 [n, 8] per position, drawn ON THE DEVICE as a pure function of
    (seed, rank, iteration, domain 0 = A | 1 = B, role 0 = real | 1 = fake, position) -- dg_diffaug_draw; include/discogan_hip.h defines
    the generator.  ``out``: a table of at least n rows to fill (rows from n on stay as they are)."""
    if out is None:
        out = torch.empty((n, 8), device=device, dtype=torch.int32)
    check_diffaug_table(out, n, "diffaug_draw")
    _lib.check(_lib.load().dg_diffaug_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank), int(iteration), int(domain), int(role), int(n), int(S),
                                           int(flags), _ptr(out), _stream()), "dg_diffaug_draw")
    return out[:n]


ADA_MAX_OUTPUTS = 65536        # discriminator outputs per dg_ada_accumulate call


def _check_ada_state(t, dtype, n, who, what):
    if not (t.is_cuda and t.dtype == dtype and t.dim() == 1 and t.numel() == n and t.is_contiguous()):
        raise _lib.DiscoganHipError(f"{who} needs {what}")


def diffaug_draw_p(seed, rank, iteration, domain, role, n, S, flags, p, out=None):
    """diffaug_draw with every stage of the policy kept per sample with probability ``p[0]``: ``p`` is a float64 tensor ON THE DEVICE (a
    view of an ADA control block, or any 1-element tensor) that the kernel reads -- the host never does (dg_diffaug_draw_p;
    include/discogan_hip.h, "adaptive discriminator augmentation", defines the gate).  p = 1 gives diffaug_draw's table bit for bit."""
    if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float64 and p.numel() >= 1 and p.is_contiguous()):
        raise _lib.DiscoganHipError("diffaug_draw_p needs the probability as a contiguous float64 HIP tensor")
    if out is None:
        out = torch.empty((n, 8), device=p.device, dtype=torch.int32)
    check_diffaug_table(out, n, "diffaug_draw_p")
    _lib.check(_lib.load().dg_diffaug_draw_p(int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank), int(iteration), int(domain), int(role), int(n), int(S),
                                             int(flags), _ptr(p), _ptr(out), _stream()), "dg_diffaug_draw_p")
    return out[:n]


def ada_accumulate(d_out, threshold, acc):
    """Add the signs of one batch of discriminator outputs ``d_out`` (float32, any shape, 1..65536 values) against ``threshold`` to the
    window ``acc`` = float32 [2] (sum of signs, count) on the device, in place (dg_ada_accumulate)."""
    _check_dev(d_out, acc)
    if not (d_out.dtype == torch.float32 and d_out.is_contiguous() and 1 <= d_out.numel() <= ADA_MAX_OUTPUTS):
        raise _lib.DiscoganHipError(f"ada_accumulate needs 1..{ADA_MAX_OUTPUTS} contiguous float32 values, got {tuple(d_out.shape)} {d_out.dtype}")
    _check_ada_state(acc, torch.float32, 2, "ada_accumulate", "the window as a contiguous float32 HIP tensor [2]")
    _lib.check(_lib.load().dg_ada_accumulate(_ptr(d_out), int(d_out.numel()), float(threshold), _ptr(acc), _stream()), "dg_ada_accumulate")
    return acc


def ada_update(ctl, acc, target, step_per_image, p_max=1.0):
    """Close the window ``acc`` (float32 [2]) into the control block ``ctl`` (float64 [8]: p, r_t, updates, images, last adjustment, 0, 0,
    0), both on the device, in place: p moves by count x ``step_per_image`` towards more augmentation when r_t > ``target``, towards less
    when below, clamped to [0, ``p_max``]; the window is zeroed.  An empty window changes nothing (dg_ada_update)."""
    _check_ada_state(ctl, torch.float64, 8, "ada_update", "the control block as a contiguous float64 HIP tensor [8]")
    _check_ada_state(acc, torch.float32, 2, "ada_update", "the window as a contiguous float32 HIP tensor [2]")
    _lib.check(_lib.load().dg_ada_update(_ptr(ctl), _ptr(acc), float(target), float(step_per_image), float(p_max), _stream()), "dg_ada_update")
    return ctl


def _diffaug_g(name, xs, flags, recs, outs):
    """``len(xs)`` batches [n,3,S,S] of one shape through dg_diffaug_{fwd,bwd}[_g]: one launch per pass for all of them."""
    g = len(xs)
    _check_dev(*xs, *(outs or ()))
    x0 = xs[0]
    if x0.dim() != 4 or x0.shape[1] != 3 or x0.shape[2] != x0.shape[3]:
        raise _lib.DiscoganHipError(f"{name} needs [n,3,S,S] batches, got {tuple(x0.shape)}")
    if len(recs) != g or any(tuple(x.shape) != tuple(x0.shape) or not x.is_contiguous() for x in xs):
        raise _lib.DiscoganHipError(f"{name}: one record table per batch, and contiguous batches of one shape, expected")
    n, S = int(x0.shape[0]), int(x0.shape[3])
    for r in recs:
        check_diffaug_table(r, n, name)
    if outs is None:
        outs = [torch.empty_like(x) for x in xs]
    elif len(outs) != g or any(tuple(o.shape) != tuple(x0.shape) or not o.is_contiguous() for o in outs):
        raise _lib.DiscoganHipError(f"{name}: outputs must be contiguous and shaped like the inputs")
    L = _lib.load()
    wsl, wsb = _ws_g(L.dg_diffaug_workspace_bytes(n, S, int(flags)), g, x0.device)
    with _hbm("diffaug", 8.0 * g * x0.numel()):
        if g == 1:
            _lib.check(getattr(L, name)(_ptr(xs[0]), _ptr(outs[0]), n, S, int(flags), _ptr(recs[0]), _ptr(wsl[0]), wsb, _stream()), name)
        else:
            _lib.check(getattr(L, name + "_g")(g, _tab(xs), _tab(outs), n, S, int(flags), _tab(recs), _tab(wsl), wsb, _stream()), name + "_g")
    return outs


def diffaug_fwd(x, flags, recs, out=None):
    """The differentiable augmentation of a batch ``x`` [n,3,S,S] by a record table (dg_diffaug_fwd; include/discogan_hip.h defines the
    transform): a new tensor like x unless ``out`` is given.  x is only read; x and out may not overlap."""
    return _diffaug_g("dg_diffaug_fwd", [x], flags, [recs], None if out is None else [out])[0]


def diffaug_bwd(dz, flags, recs, out=None):
    """The adjoint of diffaug_fwd's linear part applied to ``dz`` [n,3,S,S] (dg_diffaug_bwd): the gradient of the input."""
    return _diffaug_g("dg_diffaug_bwd", [dz], flags, [recs], None if out is None else [out])[0]


def diffaug_fwd_g(xs, flags, recs, outs=None):
    """diffaug_fwd of up to MAX_GROUPS batches of one shape, each by its own table, in one launch per pass; bitwise the single calls."""
    return _diffaug_g("dg_diffaug_fwd", list(xs), flags, list(recs), outs)


def diffaug_bwd_g(dzs, flags, recs, outs=None):
    """diffaug_bwd of up to MAX_GROUPS gradients of one shape, each by its own table, in one launch per pass."""
    return _diffaug_g("dg_diffaug_bwd", list(dzs), flags, list(recs), outs)


def sample_grid(batches, rows, gap=2, bg=255):
    """1..8 float32 NCHW batches [n_c,3,S,S] (n_c >= rows) -> ONE uint8 canvas [rows*(S+gap)+gap, cols*(S+gap)+gap, 3] on the device:
    cell (r, c) = image r of batches[c], pixel = rint(clamp(x, 0, 1) * 255) (half to even, NaN -> 0), every other byte ``bg``
    (image_translation.py:170-209).  One launch writes the whole canvas (dg_sample_grid_u8)."""
    import ctypes as C
    batches = list(batches)
    if not batches:
        raise _lib.DiscoganHipError("sample_grid needs at least one batch")
    _check_dev(*batches)
    xs = [b.contiguous() for b in batches]
    S = xs[0].shape[-1]
    for x in xs:
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != S or x.shape[3] != S or x.device != xs[0].device:
            raise _lib.DiscoganHipError(f"sample_grid needs [n,3,S,S] batches of one S on one device, got {tuple(x.shape)}")
        if x.shape[0] < rows:
            raise _lib.DiscoganHipError(f"sample_grid: a batch of {x.shape[0]} images cannot fill {rows} rows")
    cols, pitch = len(xs), S + int(gap)
    canvas = torch.empty((max(rows, 0) * pitch + int(gap), cols * pitch + int(gap), 3), device=xs[0].device, dtype=torch.uint8)
    tab = (C.c_void_p * cols)(*[x.data_ptr() for x in xs])
    _lib.check(_lib.load().dg_sample_grid_u8(tab, cols, int(rows), S, int(gap), int(bg), _ptr(canvas), _stream()), "dg_sample_grid_u8")
    return canvas


def f32chw_to_u8hwc(x):
    """float32 NCHW [n,3,S,S] -> uint8 [n,S,S,3] = rint(clamp(x, 0, 1) * 255): the inverse of ``u8hwc_to_f32chw`` (a one-column
    grid without gutters is exactly the images one under the other)."""
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise _lib.DiscoganHipError(f"f32chw_to_u8hwc needs a square [n,3,S,S] batch, got {tuple(x.shape)}")
    n, S = x.shape[0], x.shape[3]
    return sample_grid([x], n, gap=0, bg=0).view(n, S, S, 3)


def image_metrics(x, y):
    """Two float32 NCHW batches [n,3,S,S] (S >= 11) -> float32 [n,3] on the device: row i = (MSE, MAE, SSIM) of the pair (x[i], y[i]),
    values taken as they are (data range 1; SSIM: 11 x 11 Gaussian window, sigma 1.5, valid windows).  Row i depends on pair i alone
    and is bitwise repeatable (dg_image_metrics)."""
    _check_dev(x, y)
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or tuple(y.shape) != tuple(x.shape) or y.device != x.device:
        raise _lib.DiscoganHipError(f"image_metrics needs two [n,3,S,S] batches of one shape on one device, got {tuple(x.shape)} and "
                                    f"{tuple(y.shape)}")
    n, S = int(x.shape[0]), int(x.shape[3])
    if n < 1 or S < 11:
        raise _lib.DiscoganHipError(f"image_metrics needs n >= 1 images of S >= 11 pixels (the 11 x 11 window), got n={n}, S={S}")
    xc, yc = x.contiguous(), y.contiguous()
    out = torch.empty((n, 3), device=x.device, dtype=torch.float32)
    L = _lib.load()
    ws, ws_bytes = _ws(L.dg_image_metrics_workspace_bytes(n, S), x.device)
    _lib.check(L.dg_image_metrics(_ptr(xc), _ptr(yc), n, S, _ptr(out), _ptr(ws), ws_bytes, _stream()), "dg_image_metrics")
    return out


# ---- sliced Wasserstein distance on Laplacian-pyramid patches (include/discogan_hip.h defines every stage) -----------------------
SWD_DESC = 147                 # floats per descriptor: 3 x 7 x 7, [channel][dy][dx]
SWD_PATCH = 7


def swd_max_row():
    """DG_SWD_MAX_ROW of the loaded library: the longest row (descriptors per set and level) one workgroup sorts in LDS."""
    return int(_lib.load().dg_swd_max_row())


def swd_levels(S):
    """The pyramid's resolutions for images of S pixels: [S, S/2, ...] while the size is even and its half is at least 16; [] for S < 16."""
    L = int(_lib.load().dg_swd_levels(int(S)))
    return [int(S) >> l for l in range(L)]


def swd_patches(n, patches=128):
    """Patches per image for a set of n images: min(patches, DG_SWD_MAX_ROW // n), so that a row of n P values fits one workgroup."""
    return min(int(patches), swd_max_row() // max(int(n), 1))


def _swd_fail(msg):
    raise _lib.DiscoganHipError(msg)


def _swd_buf(t, shape, dtype, who, what):
    if not (t.is_cuda and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        _swd_fail(f"{who} needs {what} as a contiguous {dtype} HIP tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def lap_pyramid(x):
    """float32 NCHW batch [n,3,S,S] (S >= 16) -> the list of its Laplacian-pyramid levels [n,3,R_l,R_l], views of one buffer
    (dg_lap_pyramid: [1 4 6 4 1] / 16, mirror border; the last level is the Gaussian level itself)."""
    _check_dev(x)
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        _swd_fail(f"lap_pyramid needs a [n,3,S,S] batch, got {tuple(x.shape)}")
    n, S = int(x.shape[0]), int(x.shape[3])
    Rs = swd_levels(S)
    if n < 1 or not Rs:
        _swd_fail(f"lap_pyramid needs n >= 1 images of S >= 16 pixels, got n={n}, S={S}")
    xc = x.contiguous()
    L = _lib.load()
    out = torch.empty(int(L.dg_lap_pyramid_elems(n, S)), device=x.device, dtype=torch.float32)
    _lib.check(L.dg_lap_pyramid(_ptr(xc), n, S, _ptr(out), _stream()), "dg_lap_pyramid")
    levels, at = [], 0
    for R in Rs:
        levels.append(out[at:at + n * 3 * R * R].view(n, 3, R, R))
        at += n * 3 * R * R
    return levels


def swd_draw(seed, level, n, R, P, out=None, device="cuda"):
    """The patch positions of one level: int32 [n, P, 2] = (oy, ox) in [0, R - 7], drawn on the device as a pure function of
    (seed, level, image, patch) -- dg_swd_draw.  ``out``: a table of at least n images to fill (rows from n on stay as they are)."""
    if out is None:
        out = torch.empty((int(n), int(P), 2), device=device, dtype=torch.int32)
    if not (out.is_cuda and out.dtype == torch.int32 and out.dim() == 3 and out.shape[1] == P and out.shape[2] == 2 and out.is_contiguous()
            and out.shape[0] >= n):
        _swd_fail(f"swd_draw needs a contiguous int32 HIP record table of shape [>= {n}, {P}, 2]")
    _lib.check(_lib.load().dg_swd_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, int(level), int(n), int(R), int(P), _ptr(out), _stream()), "dg_swd_draw")
    return out[:n]


def swd_descriptors(level, recs, desc=None, stats=None):
    """One pyramid level [n,3,R,R] and its record table int32 [n,P,2] -> (desc float32 [n P, 147], stats float64 [3, 2] = per channel mean
    and population standard deviation of the descriptor values) -- dg_swd_descriptors.  Offsets are clamped into the image."""
    _check_dev(level)
    if level.dim() != 4 or level.shape[1] != 3 or level.shape[2] != level.shape[3] or not level.is_contiguous():
        _swd_fail(f"swd_descriptors needs a contiguous [n,3,R,R] level, got {tuple(level.shape)}")
    n, R = int(level.shape[0]), int(level.shape[3])
    if not (recs.is_cuda and recs.dtype == torch.int32 and recs.dim() == 3 and recs.shape[0] == n and recs.shape[2] == 2 and recs.is_contiguous()):
        _swd_fail(f"swd_descriptors needs a contiguous int32 HIP record table of shape [{n}, P, 2]")
    P = int(recs.shape[1])
    M = n * P
    if n < 1 or P < 1 or M > swd_max_row() or R < SWD_PATCH:
        _swd_fail(f"swd_descriptors needs 1 <= n P <= {swd_max_row()} and R >= {SWD_PATCH}, got n={n}, P={P}, R={R}")
    desc = torch.empty((M, SWD_DESC), device=level.device, dtype=torch.float32) if desc is None else \
        _swd_buf(desc, (M, SWD_DESC), torch.float32, "swd_descriptors", "desc")
    stats = torch.empty((3, 2), device=level.device, dtype=torch.float64) if stats is None else \
        _swd_buf(stats, (3, 2), torch.float64, "swd_descriptors", "stats")
    L = _lib.load()
    nbytes = int(L.dg_swd_descriptors_workspace_bytes(M))
    ws = torch.empty(nbytes // 8, device=level.device, dtype=torch.float64)
    _lib.check(L.dg_swd_descriptors(_ptr(level), n, R, P, _ptr(recs), _ptr(desc), _ptr(stats), _ptr(ws), nbytes, _stream()), "dg_swd_descriptors")
    return desc, stats


def swd_project(desc, stats, dirs, out=None):
    """desc float32 [M,147], stats float64 [3,2], dirs float32 [D,147] -> proj float32 [D,M]: the normalised descriptors on every
    direction (dg_swd_project: fp32 fma chain, a channel of standard deviation 0 contributes zeros)."""
    _check_dev(desc, dirs)
    if desc.dim() != 2 or desc.shape[1] != SWD_DESC or dirs.dim() != 2 or dirs.shape[1] != SWD_DESC or not desc.is_contiguous() \
            or not dirs.is_contiguous():
        _swd_fail(f"swd_project needs contiguous desc [M,{SWD_DESC}] and dirs [D,{SWD_DESC}], got {tuple(desc.shape)} and {tuple(dirs.shape)}")
    _swd_buf(stats, (3, 2), torch.float64, "swd_project", "stats")
    M, D = int(desc.shape[0]), int(dirs.shape[0])
    if M < 1 or D < 1 or M > swd_max_row():
        _swd_fail(f"swd_project needs 1 <= M <= {swd_max_row()} and D >= 1, got M={M}, D={D}")
    out = torch.empty((D, M), device=desc.device, dtype=torch.float32) if out is None else _swd_buf(out, (D, M), torch.float32, "swd_project", "out")
    _lib.check(_lib.load().dg_swd_project(_ptr(desc), _ptr(stats), M, _ptr(dirs), D, _ptr(out), _stream()), "dg_swd_project")
    return out


def _swd_rows(proj, who):
    _check_dev(proj)
    if proj.dim() != 2 or not proj.is_contiguous():
        _swd_fail(f"{who} needs a contiguous [D,M] tensor, got {tuple(proj.shape)}")
    D, M = int(proj.shape[0]), int(proj.shape[1])
    if D < 1 or M < 1 or M > swd_max_row():
        _swd_fail(f"{who} needs D >= 1 rows of 1 <= M <= {swd_max_row()} values (one workgroup sorts a row in LDS), got D={D}, M={M}")
    return D, M


def swd_sort_rows(proj):
    """Sorts every row of float32 [D,M] ascending IN PLACE (dg_swd_sort_rows; total order on the bits: -inf first, +inf last, NaNs beyond)."""
    D, M = _swd_rows(proj, "swd_sort_rows")
    _lib.check(_lib.load().dg_swd_sort_rows(_ptr(proj), D, M, _stream()), "dg_swd_sort_rows")
    return proj


def swd_row_distance(proj, ref_sorted, out=None, sorted_out=None):
    """float32 [D,M] and sorted rows [D,M] -> float64 [D]: out[d] = mean_i |sort(proj[d])_i - ref_sorted[d][i]| (dg_swd_row_distance).
    ``proj`` is only read; its sorted rows are written to ``sorted_out`` when given."""
    D, M = _swd_rows(proj, "swd_row_distance")
    _check_dev(ref_sorted, sorted_out)
    _swd_buf(ref_sorted, (D, M), torch.float32, "swd_row_distance", "ref_sorted")
    if sorted_out is not None:
        _swd_buf(sorted_out, (D, M), torch.float32, "swd_row_distance", "sorted_out")
    out = torch.empty(D, device=proj.device, dtype=torch.float64) if out is None else _swd_buf(out, (D,), torch.float64, "swd_row_distance", "out")
    _lib.check(_lib.load().dg_swd_row_distance(_ptr(proj), _ptr(ref_sorted), D, M, _ptr(out), _ptr(sorted_out), _stream()), "dg_swd_row_distance")
    return out


def krsc_param(w_logical):
    """[K,C,4,4] contiguous -> same logical tensor whose memory is [K,4,4,C] (dim 1 innermost)."""
    return w_logical.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def is_krsc(w):
    return is_nhwc(w)


def _krsc(w):
    return w if is_krsc(w) else krsc_param(w)


def empty_krsc(k, c, device):
    return torch.empty((k, 4, 4, c), device=device, dtype=torch.float32).permute(0, 3, 1, 2)


def _ws(nbytes, device):
    if nbytes == 0:
        return None, 0
    t = torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
    return t, t.numel() * 4


# ---- bf16 shadow operands (mfma_dtype="bf16") -------------------------------------------------------------------
# A shadow is a bf16 (RNE) copy of an fp32 tensor in the same memory layout, written by the tensor's producer (Adam for
# weights, the BatchNorm kernels / first conv for activations and gradients).  With SHADOW on, the conv wrappers hand the
# shadows to dg_conv_*_mixed: half the operand bytes, no conversion in the conv kernel, bit-identical results.
#   weights    : ``param._dg_bf16`` (a view of optim.Adam's flat bf16 buffer), valid while ``param._version`` is unchanged
#   activations: side table keyed by the fp32 tensor's storage address; the entry holds the fp32 tensor, so the address
#                cannot be recycled while the entry lives; the trainer clears the table every iteration.
def shadow_clear():
    _CUR.shadow_tab.clear()


def shadow_put(t, t16):
    _CUR.shadow_tab[t.data_ptr()] = (t, t16)


def derived_release(*tensors):
    """Drop the bf16 shadow / plane triple of tensors whose conv consumers have all been issued (functional.py calls this
    after a layer's input-grad and weight-grad): the fp32 tensor and its copies then die with autograd's own references
    instead of living to the end of the iteration (or, under hipGraph capture, forever in the graph's pool)."""
    for t in tensors:
        if t is None:
            continue
        key = t.data_ptr()
        for tab in (_CUR.shadow_tab, _CUR.plane_tab):
            e = tab.get(key)
            if e is not None and e[0].shape == t.shape:
                del tab[key]


def shadow_get(t):
    if not _CUR.shadow:
        return None
    e = _CUR.shadow_tab.get(t.data_ptr())
    if e is None or e[0].shape != t.shape or e[0].stride() != t.stride():
        return None
    return e[1]


def weight_shadow(w):
    """bf16 shadow of a conv weight Parameter (None when shadows are off or the parameter is not in a flat Adam group)."""
    if not _CUR.shadow:
        return None
    w16 = getattr(w, "_dg_bf16", None)
    if w16 is None:
        return None
    if getattr(w, "_dg_bf16_ver", None) != w._version:          # e.g. load_state_dict wrote the fp32 weights
        f32_to_bf16(w, w16)
        w._dg_bf16_ver = w._version
    return w16


def f32_to_bf16(x, out):
    """out (bf16, same memory layout / numel as x) <- RNE(x)."""
    assert out.dtype == torch.bfloat16 and out.stride() == x.stride() and out.shape == x.shape
    _lib.check(_lib.load().dg_f32_to_bf16(_ptr(x), _ptr(out), x.numel(), _stream()), "dg_f32_to_bf16")
    return out


def empty_nhwc_bf16(n, c, h, w, device):
    return torch.empty((n, h, w, c), device=device, dtype=torch.bfloat16).permute(0, 3, 1, 2)


def _bf16_ok(op, n, h, wd, c, k, stride, pad):
    return _CUR.shadow and _lib.load().dg_conv_bf16_operands_ok(op, n, h, wd, c, k, stride, pad) >= 1


# ---- f32x3 plane operands (mfma_dtype="f32x3") -----------------------------------------------------------------
# A plane triple is three bf16 tensors hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid) of an fp32 tensor,
# plane-major ([3, numel] bf16).  With X3 on, the conv wrappers hand plane triples of BOTH operands to dg_conv_*_x3 where the
# shape has the plane kernel (csrc/igemm_dma_x3.hip); everything else keeps the fp32 tensors (register-staged f32x3 tiles).
#   weights    : ``param._dg_x3`` = (flat [3, P] bf16 buffer of optim.Adam, element offset), refreshed by the Adam kernel;
#                valid while ``param._version`` is unchanged (a foreign write re-splits the one weight)
#   activations: side table like the bf16 shadows; filled by the producers (BatchNorm kernels) or, for a tensor nobody has
#                split yet, by dg_f32_to_bf16x3 at its first use (the triple then serves the forward AND the weight gradient)
# X3_CM: the BatchNorm kernels write the plane triples that a WINDOW input-grad kernel will read (dy of the conv layers with
# <= 128 input channels, the input of the transposed convs with <= 128 output channels) in the QUAD-CHUNK layout
# ([pixels/4][C/16][4][16], include/discogan_hip.h "plane_layout"): the window kernel then uses every byte of the 128-byte lines
# it fetches instead of 32.  Bit-identical results; DG_X3_CM=0 keeps every triple pixel-major (A/B).
X3_CM = _env_flag("DG_X3_CM", True)
# X3_PLANES_ONLY: a BatchNorm output whose every reader is a plane kernel (the next conv's forward and weight-grad; the
# layer's own input-grad and weight-grad for a gradient) is written ONLY as its plane triple: the planes carry all 24 significand
# bits (hi + mid + lo == the fp32 value), the fp32 tensor stays allocated but unwritten and is flagged ``_dg_planes_only`` --
# every op wrapper that would read fp32 memory refuses such a tensor.  model.py decides per layer; DG_X3_PLANES_ONLY=0: off (A/B).
X3_PLANES_ONLY = _env_flag("DG_X3_PLANES_ONLY", True)
# POISON_PLANES_ONLY (debug aid, DG_POISON_PLANES_ONLY=1; round-3 advisor finding): the fp32 memory of a plane-only tensor is never written
# and its only protection is the ``_dg_planes_only`` attribute, which a view / a torch-native reader does not carry.  With the switch on that
# memory is filled with NaN, so anything that reads it (instead of the planes) turns the losses NaN instead of using stale allocator bytes;
# tests/test_model_gpu.py runs a training step under it and requires the results bitwise unchanged.
POISON_PLANES_ONLY = _env_flag("DG_POISON_PLANES_ONLY", False)
# X3_FWW: forward convolutions with <= 128 output channels on the window forward kernel (csrc/igemm_dma_x3_fww.hip; planner code 3:
# needs the transposed weight planes).  OFF by default: built, parity-tested and measured at the benchmark shape (64 -> 128 channels,
# 512 px / batch 32) at 0.923 ms against 0.927 ms for the register-staged f32x3 tiles -- its window pixels are every OTHER pixel of a
# pixel-major plane, 32 bytes of each 128-byte line per fetch, and those loads cost it 0.28 of its 0.92 ms.
# DG_X3_FWW=1 turns it on.
X3_FWW = _env_flag("DG_X3_FWW", False)
# X3_FUSE_STATS: on the plane path the BatchNorm batch statistics come out of the producing conv kernel's epilogue (or its split-K
# reduction) as partial rows, merged by dg_bn_stats_from_partials -- no separate read pass over the conv output.  (On the exact-fp32
# path of the 64 px network the same idea lengthened 140 us kernels by more than the pass it saved: model.FUSE_BN_STATS fuses only
# launches of 40 GFLOP and more there; the plane kernels run for hundreds of microseconds per tile and do not notice ~400 VALU instructions per wave.)
X3_FUSE_STATS = _env_flag("DG_X3_FUSE_STATS", True)
# FUSE_STATS16: the bf16 matrix path takes its BatchNorm statistics from the bf16 conv
# kernels' fp32 accumulators too (LDS-DMA kernel, window input-grad, register-staged tiles, split-K reduction: stat argument of
# dg_conv_fwd_mixed / _dgrad_mixed) instead of dropping to the exact-fp32 kernels for the fused layers.
FUSE_STATS16 = _env_flag("DG_FUSE_BN16", True)
# X3_MFMA: the MFMA shape of the plane kernel's 256 x 256 tile (library option "x3_mfma").  16 = v_mfma_f32_16x16x32_bf16 with the
# planes paired along k (three instructions per 16 x 16 block and K-tile instead of six 32x32x16 ones: the same products, a shape
# under which the chip holds a higher clock; csrc/igemm_dma_x3.hip); 32 / 0 = the 32x32x16 body (default: the paired body is faster
# per launch on the middle layers and not at all in the whole step).  The
# environment variable is applied by _lib.load() like every DG_OPT_*; this constant is what tests restore the option to.
X3_MFMA = int(os.environ.get("DG_OPT_X3_MFMA", "0"))


# X3_RSP (off: measured 45 % SLOWER): forward convs without an LDS-DMA plane kernel (fewer than 192 output channels: the 64 -> 128
# layer and, same GEMM, the input-grad of the 128 -> 64 transposed conv) on the register-staged 128 x 128 tiles READING the plane
# triples their producers wrote (dg_conv_x3_planes_ok codes 3 / 4: igemm_kernel<.., PREC 2, A16, B16>) instead of splitting fp32
# operands inside the kernel.  Bit-identical, a quarter fewer instructions -- and 1.36 instead of 0.94 ms at 512 px / batch 32: a
# 16-channel K-tile of a pixel-major plane is a 32-byte piece of a 128-byte line, three planes make it three times as many load
# instructions of half the useful width (the fp32 operand: 64-byte pieces).  DG_X3_RSP=1 switches it on.  DESIGN.md 3.1.
X3_RSP = _env_flag("DG_X3_RSP", False)


def _plane_code(*request):
    """Which kernel reads plane triples for the request (op, n, h, wd, c, k, stride, pad): 0 none, 1 the LDS-DMA plane kernel, 2 the
    window input-grad kernel with K % 64 == 0 (it takes quad-chunk planes), 3 the window forward kernel, 4 the register-staged tiles
    reading planes (3 and 4: answers of the experiments library only)."""
    return _lib.load().dg_conv_x3_planes_ok(*request)


def _x3_code(op, n, h, wd, c, k, stride, pad):
    """The plane code a launch under the current context goes by: 0 outside the f32x3 plane path and for the one-channel head."""
    return _plane_code(op, n, h, wd, c, k, stride, pad) if (_CUR.x3 and k > 1) else 0


def _plane_code_ok(code):
    return code in (1, 2) or (code == 3 and (X3_FWW or X3_RSP)) or (code == 4 and X3_RSP)


def _fwd_weight_planes(code, w):
    """Which planes of the weight ``w`` the FORWARD launch of a request with plane code ``code`` reads: 1 the transposed copy
    [(r, s, c)][k] (the faster form; weights of a flat Adam group have one), 0 the plain planes, None: no plane launch.  The
    register-staged tiles (code 4, and code 3 without the window forward kernel's transposed planes or without X3_FWW) read the PLAIN
    planes and only under X3_RSP.  The one statement of this rule: _conv_form launches by it, model._first_layer_planes predicts by it."""
    if not _plane_code_ok(code):
        return None
    has_transposed = getattr(w, "_dg_x3", (None, 0, None))[2] is not None
    if code == 4 or (code == 3 and not (has_transposed and X3_FWW)):
        return 0 if X3_RSP else None
    return int(has_transposed)


def planes_clear():
    _CUR.plane_tab.clear()


def planes_put(t, t3, cm=False):
    _CUR.plane_tab[t.data_ptr()] = (t, t3, bool(cm))


def f32_to_bf16x3(x, out3):
    """out3 ([3, P] bf16, P >= x.numel()) <- the plane triple of x's memory image."""
    assert out3.dtype == torch.bfloat16 and out3.dim() == 2 and out3.shape[0] == 3 and out3.stride(1) == 1
    _lib.check(_lib.load().dg_f32_to_bf16x3(_ptr(x), _ptr(out3), x.numel(), out3.stride(0), _stream()), "dg_f32_to_bf16x3")
    return out3


def planes_of(t, allow_cm=False):
    """(plane-0 address, plane distance in bytes, chunk-major?) of an fp32 activation / gradient tensor; splits it on first
    use.  A chunk-major triple (written by a BatchNorm kernel for a window input-grad kernel) is only handed to callers that
    can read it (allow_cm); anybody else gets a pixel-major split of the fp32 tensor."""
    e = _CUR.plane_tab.get(t.data_ptr())
    if e is None or e[0].shape != t.shape or e[0].stride() != t.stride() or (e[2] and not allow_cm):
        if getattr(t, "_dg_planes_only", False):
            raise _lib.DiscoganHipError("plane-only tensor without a usable plane triple (released, or in a layout this reader cannot take)")
        t3 = torch.empty((3, t.numel()), device=t.device, dtype=torch.bfloat16)
        with _hbm("x3_split", 10.0 * t.numel()):
            f32_to_bf16x3(t, t3)
        if e is None or not e[2]:
            planes_put(t, t3)
        return t3.data_ptr(), t3.stride(0) * 2, 0
    return e[1].data_ptr(), e[1].stride(0) * 2, int(e[2])


def x3_all_plane_readers(n, h, wd, c, k, forward_is_dgrad=False, need_wgrad=True):
    """Are the conv kernels that will READ a tensor all plane kernels?  For a layer input x of Conv2d(c, k, 4, 2, 1) on [n, c, h, wd]:
    its forward (op 0) and weight-grad (op 2); with forward_is_dgrad (ConvTranspose2d: the same geometry read as an input-grad): op 1
    and op 2.  For a gradient dy: the layer's input-grad (op 1) and weight-grad -- the same question with forward_is_dgrad.
    (Looser than the launch in one case, kept: plane code 3 under X3_FWW counts although a weight without a transposed copy then takes
    the fp32 form, which refuses a plane-only tensor.)"""
    if not (_CUR.x3 and X3_PLANES_ONLY):
        return False
    first = 1 if forward_is_dgrad else 0
    return _plane_code_ok(_plane_code(first, n, h, wd, c, k, 2, 1)) and (not need_wgrad or _plane_code(2, n, h, wd, c, k, 2, 1) >= 1)


def x3_window_dgrad(n, h, wd, c, k):
    """Will the input-grad of Conv2d(c, k, 4, 2, 1) on an [n, c, h, wd] input (= the forward of the transposed conv with the same
    weight) run on the window kernel AND its weight gradient on the plane kernel?  Then the producer of the gradient operand
    writes chunk-major planes (X3_CM)."""
    if not (_CUR.x3 and X3_CM) or k % 64 != 0:
        return False
    return _plane_code(1, n, h, wd, c, k, 2, 1) == 2 and _plane_code(2, n, h, wd, c, k, 2, 1) == 1


def x3_transpose_table(convs):
    """Host-side table for x3_transpose_planes: convs = [(element offset inside a plane, K, J = 16 C), ...]."""
    import ctypes as C
    n = len(convs)
    return (n, (C.c_int64 * max(n, 1))(*[c[0] for c in convs]), (C.c_int * max(n, 1))(*[c[1] for c in convs]),
            (C.c_int * max(n, 1))(*[c[2] for c in convs]))


def x3_transpose_planes(src3, dst3, table):
    """dst3 <- for every conv weight of the table the [K][J] plane images of src3 transposed to [J][K] (same offsets)."""
    n, off, k, j = table
    assert src3.shape == dst3.shape and src3.stride(0) == dst3.stride(0)
    nbytes = 12.0 * sum(int(k[i]) * int(j[i]) for i in range(n))
    with _hbm("x3_split", nbytes):
        _lib.check(_lib.load().dg_x3_transpose_planes(_ptr(src3), _ptr(dst3), src3.stride(0), off, k, j, n, _stream()),
                   "dg_x3_transpose_planes")


def weight_planes(w, transposed=False):
    """(plane-0 address, plane distance in bytes, is the transposed copy) of a conv weight Parameter's triple.  transposed:
    prefer the [(r, s, c)][k] copy the forward form of the plane kernel reads (weights of a flat Adam group have one)."""
    e = getattr(w, "_dg_x3", None)
    if e is None:                                    # a parameter outside a flat Adam group
        e = (torch.empty((3, w.numel()), device=w.device, dtype=torch.bfloat16), 0, None)
        w._dg_x3, w._dg_x3_ver = e, None
    buf, off, buft = e
    if getattr(w, "_dg_x3_ver", None) != w._version:            # e.g. load_state_dict wrote the fp32 weights
        _lib.check(_lib.load().dg_f32_to_bf16x3(_ptr(w), buf.data_ptr() + 2 * off, w.numel(), buf.stride(0), _stream()),
                   "dg_f32_to_bf16x3")
        if buft is not None:
            x3_transpose_planes(buf, buft, x3_transpose_table([(off, w.shape[0], 16 * w.shape[1])]))
        w._dg_x3_ver = w._version
    if transposed and buft is not None:
        return buft.data_ptr() + 2 * off, buft.stride(0) * 2, 1
    return buf.data_ptr() + 2 * off, buf.stride(0) * 2, 0


def _x3_ok(op, n, h, wd, c, k, stride, pad):
    return _plane_code_ok(_x3_code(op, n, h, wd, c, k, stride, pad))


def x3_fwd_weight_planes(n, h, wd, c, k, stride, pad, w):
    """_fwd_weight_planes of the forward of Conv2d(c, k, 4, stride, pad) with weight ``w`` on [n, c, h, wd] under the current context."""
    return _fwd_weight_planes(_x3_code(0, n, h, wd, c, k, stride, pad), w)


# ---- interior convolutions ------------------------------------------------------------------------------
# One call (_conv) = the operands prepared once, one request (_ConvReq: what is asked), one form choice (_conv_form: which entry point
# family reads which operand forms) and one launch.  DESIGN.md 3.1 "Conv op wrappers".
def _out_hw(h, w, stride, pad):
    return (h + 2 * pad - 4) // stride + 1, (w + 2 * pad - 4) // stride + 1


def _mixed_operand(t, allow_shadow=True):
    """(pointer tensor, is_bf16) of a conv operand: a bf16 tensor as it is, an fp32 tensor's shadow if it has one."""
    if _is16(t):
        return t, 1
    t16 = shadow_get(t) if allow_shadow else None
    return (t16, 1) if t16 is not None else (t, 0)


_CONV_NAME = ("conv_fwd", "conv_dgrad", "conv_wgrad")


class _ConvReq:
    """One interior conv request, built once per call from the operands a, b = (x, w) | (dy, w) | (dy, x) of op 0 forward | 1 input
    gradient | 2 weight gradient: ``geom`` = (n, h, wd, c, k, stride, pad) of the Conv2d (x [n, c, h, wd], k output channels, dy
    [n, k, ho, wo]), the feature-map result's shape and channels (op 0: y, op 1: dx), the current context's arithmetic, and the
    roofline hook's name and algorithmic FLOPs."""
    __slots__ = ("op", "geom", "c", "k", "out_shape", "out_channels", "prec", "name", "flops")

    def __init__(self, op, a, b, stride, pad, x_hw=None):
        if op == 1:                                    # the input's size is not in the operands
            (n, k, ho, wo), c, (h, wd) = a.shape, b.shape[1], x_hw
        else:
            n, c, h, wd = (a if op == 0 else b).shape
            k = b.shape[0] if op == 0 else a.shape[1]
            ho, wo = _out_hw(h, wd, stride, pad) if op == 0 else (a.shape[2], a.shape[3])
        self.op, self.geom, self.c, self.k, self.prec = op, (n, h, wd, c, k, stride, pad), c, k, _CUR.cprec
        self.out_shape, self.out_channels = ((n, k, ho, wo), k) if op == 0 else ((n, c, h, wd), c)
        self.name = _CONV_NAME[op] if k > 1 else "head1"
        self.flops = 2.0 * n * ho * wo * k * c * 16

    def workspace_bytes(self, plan_groups=1):
        return _lib.load().dg_conv_workspace_bytes_p(self.op, *self.geom, self.prec, plan_groups)


# What _conv_form chose: kind "x3" (plane triples; ``w_planes``: 1 the transposed weight copy, forward only; ``cm_ok``: the gradient
# operand may be a quad-chunk triple), "mixed" (``a16 / b16 / o16``: operand A, operand B, the output are bf16), "g" (fp32 tensors, one
# problem) or "refuse" (``why``); ``rows``: statistics rows a "mixed" / "g" launch writes (0: none; the plane form's rows are asked
# for at the launch, once its operands exist); ``declined_planes``: see _conv.
_ConvForm = collections.namedtuple("_ConvForm", "kind a16 b16 o16 rows w_planes cm_ok declined_planes why", defaults=(0, 0, 0, 0, 0, False, False, None))


def _conv_form(rq, a, b, want_stats=False):
    """The form one interior conv request is launched in, from the request, its two operands as they were handed over (dtype,
    ``_dg_planes_only``, shadows, plane entries), ``want_stats`` (False | True | "split"), the current context and the switches X3_FWW,
    X3_RSP, FUSE_STATS16.  Asks the library's host queries; allocates nothing, launches nothing.  The three ops are NOT mirror
    images: every line marked (op ...) is a difference the three-wrapper form had, kept as it was."""
    L = _lib.load()
    op, geom, k, c = rq.op, rq.geom, rq.k, rq.c
    # statistics rows of the fp32 form; "split": only where the split-K reduction kernel can emit them.  (op 2 has no statistics)
    rows = L.dg_conv_bnstats_rows_p(op, *geom, rq.prec) if want_stats else 0
    if want_stats == "split" and L.dg_conv_plan_splits_p(op, *geom, rq.prec, 1) <= 1:
        rows = 0
    # ---- plane triples (f32x3 plane path) ----
    code = _x3_code(op, *geom)
    # (op 0) the forward alone has weight-plane variants and may decline a plane code the predictors accept (_fwd_weight_planes)
    w_planes = _fwd_weight_planes(code, b) if op == 0 else (0 if _plane_code_ok(code) else None)
    if w_planes is not None:
        # (op 1) a quad-chunk gradient triple is read by the window kernel only (code 2); (op 2) the plane weight-grad kernel takes
        # either layout; (op 0) x is never chunk-major
        return _ConvForm("x3", 0, 0, 0, 0, w_planes, (code == 2) if op == 1 else op == 2)
    declined = _plane_code_ok(code)                    # (op 0 only; see _conv)
    # ---- from here on the kernels read memory images ----
    for t in (a, b) if op == 2 else (a,):
        if getattr(t, "_dg_planes_only", False):
            return _ConvForm("refuse", declined_planes=declined, why=f"{_CONV_NAME[op]}: the operand exists only as its plane triple, but "
                                                                     "this shape has no plane kernel")
    a16 = b16 = o16 = 0
    if op == 2:
        if k == 1:
            b16 = int(_is16(b))                        # the one-channel head reads a bf16 x as it is (no shadows, dy stays fp32)
        elif _bf16_ok(2, *geom) or _is16(b) or _is16(a):           # (op 2) bf16 TENSORS go to the mixed entry point whatever the query says
            if c % 8 == 0:                             # (8-element granules of a bf16 x must not straddle a tap: its rows are C channels long)
                b16 = _mixed_operand(b)[1]
            if k % 8 == 0:                             # (the same for the K-channel rows of dy)
                a16 = _mixed_operand(a)[1]
        if (_is16(a) and not a16) or (_is16(b) and not b16):
            return _ConvForm("refuse", why=f"conv_wgrad: no bf16 kernel for bf16 operands of shapes {tuple(a.shape)}, {tuple(b.shape)}")
        return _ConvForm("mixed", a16, b16) if (a16 or b16) else _ConvForm("g")
    if k == 1:
        if op == 0:
            a16 = int(_is16(a))                        # (op 0) head forward: a bf16 x is read as it is, the one-channel output stays fp32
        else:
            o16 = int(_act_dtype(c) == torch.bfloat16)             # (op 1) head input gradient: dy [N,1,1,1] is fp32, the result a feature map
    elif (rows == 0 or FUSE_STATS16) and _bf16_ok(op, *geom):
        if op == 0 or k % 8 == 0:                      # (op 1) dy's rows are K channels long: granule rule as in op 2; x's C % 32 == 0 always
            a16 = _mixed_operand(a)[1]
        b16 = int(_CUR.shadow and getattr(b, "_dg_bf16", None) is not None)      # (weight_shadow(b) is not None, without its refresh)
        o16 = int(_act_dtype(rq.out_channels) == torch.bfloat16)
    mixed = bool(a16 or b16 or o16)
    if op == 0 and _is16(a) and not mixed:             # (op 0) tests the whole form ...
        return _ConvForm("refuse", declined_planes=declined, why=f"conv_fwd: no bf16 kernel for a bf16 input of shape {tuple(a.shape)} -> {k} channels")
    if op == 1 and _is16(a) and not a16:               # (op 1) ... the operand's own flag: kept from the three-wrapper form, reason not recorded
        return _ConvForm("refuse", why=f"conv_dgrad: no bf16 kernel for a bf16 gradient of shape {tuple(a.shape)}")
    if not mixed:
        return _ConvForm("g", 0, 0, 0, rows, 0, False, declined)
    # (op 1) the mixed statistics rows carry k > 1: kept from the three-wrapper form, reason not recorded (the head has no BatchNorm behind it)
    mrows = L.dg_conv_mixed_bnstats_rows(op, *geom, a16, b16) if (want_stats and FUSE_STATS16 and (op == 0 or k > 1)) else 0
    return _ConvForm("mixed", a16, b16, o16, mrows, 0, False, declined)


def _stat_rows(rows, channels, device):
    """Buffer for ``rows`` partial-statistics rows of a ``channels``-channel conv output (None for no rows)."""
    return torch.empty((rows, 3 * channels + 4), device=device, dtype=torch.float32) if rows > 0 else None


def _numel(t):
    return t.numel() if t is not None else 0


def _launch_g(rq, as_, bs, outs, plan_groups, stats, wsl, wsb, share=1, accumulate=False):
    """The fp32-tensor form for a list of problems (one launch per kernel of the plan): arithmetic = the request's, passed with the call;
    ``stats``: one statistics buffer per problem or None; ``wsl``: one workspace per problem."""
    L, g = _lib.load(), len(as_)
    with _prof(rq.name, rq.flops * g):
        if rq.op == 2:
            rc = L.dg_conv_wgrad_g(g, int(share), _tab(as_), _tab(bs), _tab(outs), *rq.geom, rq.prec, plan_groups, int(accumulate), _tab(wsl), wsb, _stream())
        else:
            rc = (L.dg_conv_dgrad_g if rq.op else L.dg_conv_fwd_g)(g, _tab(as_), _tab(bs), _tab(outs), *rq.geom, rq.prec, plan_groups, _tab(stats),
                                                                   _numel(stats[0]) if stats else 0, _tab(wsl), wsb, _stream())
    if rc != 0:
        _lib.check(rc, f"dg_{_CONV_NAME[rq.op]}_g")


def _conv(op, a, b, stride, pad, x_hw=None, want_stats=False, out=None, accumulate=False):
    """One interior conv call, a, b as in _ConvReq: prepare the operands, build the request, choose the form, then fetch the derived
    operands (they may split or refresh), allocate the output and the statistics rows, and launch.  Returns (output, statistics
    rows or None)."""
    _check_dev(*((a, b) if op == 2 else (a,)), allow16=True, planes_ok=True)
    if op != 2:
        _check_dev(b)
    a, b = as_nhwc(a), (as_nhwc(b) if op == 2 else _krsc(b))
    rq = _ConvReq(op, a, b, stride, pad, x_hw)
    if op == 2 and out is None:
        out = empty_krsc(rq.k, rq.c, a.device)
    ws, wsb = _ws(rq.workspace_bytes(), a.device)
    f = _conv_form(rq, a, b, want_stats)
    if f.declined_planes:
        # kept from the three-wrapper form, reason not recorded: a forward that declines its plane code (code 3 under X3_FWW, weight
        # without a transposed copy) still brings the weight's triple up to date before it goes on in another form
        weight_planes(b, transposed=True)
    if f.kind == "refuse":
        raise _lib.DiscoganHipError(f.why)
    if f.kind == "g":
        if out is None:
            out = empty_nhwc(*rq.out_shape, a.device)
        stat = _stat_rows(f.rows, rq.out_channels, a.device)
        _launch_g(rq, [a], [b], [out], 1, None if stat is None else [stat], [ws], wsb, 1, accumulate)
        return out, stat
    L, geom = _lib.load(), rq.geom
    if f.kind == "mixed":
        if f.a16:
            a = _mixed_operand(a)[0]
        if f.b16:
            b = _mixed_operand(b)[0] if op == 2 else weight_shadow(b)
        rows = f.rows
    elif op == 0:                                      # "x3" (op 0: the weight's planes first, then x; op 1: dy first -- the order of the splits, kept)
        pb = weight_planes(b, transposed=bool(f.w_planes))
        pa = planes_of(a)
    else:
        pa = planes_of(a, allow_cm=f.cm_ok)
        pb = weight_planes(b) if op == 1 else planes_of(b)
    if out is None:
        out = empty_nhwc(*rq.out_shape, a.device, torch.bfloat16 if f.o16 else torch.float32)
    if f.kind == "x3":                                 # (the plane form's statistics rows: asked for once its operands exist)
        rows = L.dg_conv_x3_bnstats_rows(op, *geom) if (want_stats and op != 2) else 0
    stat = _stat_rows(rows, rq.out_channels, a.device)
    tail = (_ptr(ws), wsb, _stream())
    with _prof(rq.name, rq.flops):
        if f.kind == "mixed":
            if op == 0:
                rc = L.dg_conv_fwd_mixed(_ptr(a), f.a16, _ptr(b), f.b16, _ptr(out), f.o16, *geom, _ptr(stat), _numel(stat), *tail)
            elif op == 1:
                rc = L.dg_conv_dgrad_mixed(_ptr(a), f.a16, _ptr(b), f.b16, _ptr(out), f.o16, *geom, _ptr(stat), _numel(stat), *tail)
            else:
                rc = L.dg_conv_wgrad_mixed(_ptr(a), f.a16, _ptr(b), f.b16, _ptr(out), *geom, int(accumulate), *tail)
        elif op == 0:                                  # pa / pb = (address, plane distance, chunk-major? | transposed?)
            rc = L.dg_conv_fwd_x3(pa[0], pa[1], pb[0], pb[1], f.w_planes, _ptr(out), *geom, _ptr(stat), _numel(stat), *tail)
        elif op == 1:
            rc = L.dg_conv_dgrad_x3(*pa, pb[0], pb[1], _ptr(out), *geom, _ptr(stat), _numel(stat), *tail)
        else:
            rc = L.dg_conv_wgrad_x3(*pa, pb[0], pb[1], _ptr(out), *geom, int(accumulate), *tail)
    if rc != 0:
        _lib.check(rc, f"dg_{_CONV_NAME[op]}_{f.kind}")
    return out, stat


def conv_fwd(x, w, stride, pad, want_stats=False):
    """nn.Conv2d(C,K,4,stride,pad,bias=False) forward. x NHWC-memory [N,C,H,W], w [K,C,4,4] KRSC.
    want_stats: also return the BatchNorm partial-statistics rows of y (None if the layer has no fused path)."""
    y, stat = _conv(0, x, w, stride, pad, None, want_stats)
    return (y, stat) if want_stats else y


def conv_dgrad(dy, w, x_hw, stride, pad, want_stats=False):
    """Input-gradient of that Conv2d == ConvTranspose2d forward. dy [N,K,Ho,Wo]; returns [N,C,H,W]
    (and, with want_stats, the BatchNorm partial-statistics rows of the result or None)."""
    dx, stat = _conv(1, dy, w, stride, pad, x_hw, want_stats)
    return (dx, stat) if want_stats else dx


def conv_fwd_bias_act(x, w, bias, stride, pad, act=ACT_NONE, slope=0.2):
    """Inference: act(Conv2d(x; w) + bias) in one kernel (BatchNorm folded into w / bias by the caller)."""
    _check_dev(x, w, bias)
    x, w = as_nhwc(x), _krsc(w)
    n, c, h, wd = x.shape
    k = w.shape[0]
    ho, wo = _out_hw(h, wd, stride, pad)
    y = empty_nhwc(n, k, ho, wo, x.device)
    L = _lib.load()
    ws, wsb = _ws(L.dg_conv_workspace_bytes(0, n, h, wd, c, k, stride, pad), x.device)
    _lib.check(L.dg_conv_fwd_bias_act(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), n, h, wd, c, k, stride, pad, act, slope, _ptr(ws), wsb,
                                      _stream()), "dg_conv_fwd_bias_act")
    return y


def conv_dgrad_bias_act(x, w, bias, out_hw, stride, pad, act=ACT_NONE, slope=0.0):
    """Inference: act(ConvTranspose2d(x; w) + bias) in one kernel; w is the transposed conv's [Cin,Cout,4,4] (KRSC memory)."""
    _check_dev(x, w, bias)
    x, w = as_nhwc(x), _krsc(w)
    n, k = x.shape[0], x.shape[1]
    c = w.shape[1]
    h, wd = out_hw
    y = empty_nhwc(n, c, h, wd, x.device)
    L = _lib.load()
    ws, wsb = _ws(L.dg_conv_workspace_bytes(1, n, h, wd, c, k, stride, pad), x.device)
    _lib.check(L.dg_conv_dgrad_bias_act(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), n, h, wd, c, k, stride, pad, act, slope, _ptr(ws), wsb,
                                        _stream()), "dg_conv_dgrad_bias_act")
    return y


def conv_wgrad(dy, x, stride, pad, out=None, accumulate=False):
    """Weight-gradient of that Conv2d: returns logical [K,C,4,4] (KRSC memory)."""
    return _conv(2, dy, x, stride, pad, None, False, out, accumulate)[0]


# ---- 3-channel edge layers ------------------------------------------------------------------------------
def c3_fwd(x_nchw, w, act=ACT_NONE, slope=0.2, want_planes=False):
    """x contiguous NCHW [N,3,H,W], w contiguous [K,3,4,4] -> NHWC-memory [N,K,H/2,W/2] (act fused).
    want_planes (f32x3 plane path): the kernel also writes the plane triple of its output (the next layer's weight-gradient reads it)."""
    _check_dev(x_nchw, w)
    x = x_nchw.contiguous()
    w = w.contiguous()
    n, _, h, wd = x.shape
    k = w.shape[0]
    if want_planes and _CUR.x3 and k == 64 and x.numel() * 4 < (1 << 30) and n * (h // 2) * (wd // 2) < (1 << 30):
        y = empty_nhwc(n, k, h // 2, wd // 2, x.device)
        y3 = torch.empty((3, y.numel()), device=x.device, dtype=torch.bfloat16)
        with _prof("c3_fwd", 2.0 * n * (h // 2) * (wd // 2) * k * 48), _hbm("edge_c3_fwd", 4.0 * x.numel() + 10.0 * y.numel()):
            _lib.check(_lib.load().dg_conv4x4s2_c3_fwd_x3(_ptr(x), _ptr(w), _ptr(y), _ptr(y3), y3.stride(0), n, h, wd, k, act, slope, _stream()),
                       "dg_conv4x4s2_c3_fwd_x3")
        planes_put(y, y3)
        return y
    o16 = _CUR.act16 and k == 64 and x.numel() * 4 < (1 << 30)
    y = empty_nhwc(n, k, h // 2, wd // 2, x.device, torch.bfloat16 if o16 else torch.float32)
    with _prof("c3_fwd", 2.0 * n * (h // 2) * (wd // 2) * k * 48), \
            _hbm("edge_c3_fwd", 4.0 * x.numel() + y.numel() * y.element_size()):
        _lib.check(_lib.load().dg_conv4x4s2_c3_fwd_p(_ptr(x), _ptr(w), _ptr(y), int(o16), n, h, wd, k, act, slope, _CUR.cprec, _stream()),
                   "dg_conv4x4s2_c3_fwd_p")
    if _CUR.shadow and not o16 and k % 8 == 0:
        shadow_put(y, f32_to_bf16(y, empty_nhwc_bf16(n, k, h // 2, wd // 2, x.device)))
    return y


def c3_dgrad_act_ok(k, n=1, h=2, wd=2, dy_bf16=False):
    """Does the input-gradient kernel take the layer's activation backward in its load path (c3_dgrad(..., act_out=...)) for
    dy [n, k, h/2, wd/2] (bf16 or fp32)?  Only the scatter kernel does, and it takes dy up to 2^31 bytes; the defaults ask about
    the smallest problem, i.e. whether the form exists for this k at all."""
    return bool(_lib.load().dg_c3_dgrad_act_ok(int(n), int(h), int(wd), int(k), int(bool(dy_bf16))))


def c3_dgrad(dy, w, act=ACT_NONE, act_out=None, in_act=ACT_NONE, slope=0.2):
    """dy NHWC-memory [N,K,Ho,Wo], w contiguous [K,3,4,4] -> contiguous NCHW [N,3,2Ho,2Wo] (act fused).
    With ``act_out`` (the saved output of the layer's fused LeakyReLU; needs c3_dgrad_act_ok(K, N, H, W, bf16 dy)) dy is taken through the activation
    backward on the fly -- bitwise c3_dgrad(act_bwd(dy, act_out, in_act, slope), w, act) without the pass in front."""
    _check_dev(dy, act_out, allow16=True)
    _check_dev(w)
    dy = as_nhwc(dy)
    w = w.contiguous()
    n, k, ho, wo = dy.shape
    dx = torch.empty((n, 3, 2 * ho, 2 * wo), device=dy.device, dtype=torch.float32)
    L = _lib.load()
    ws, wsb = _ws(L.dg_c3_dgrad_workspace_bytes(k), dy.device)
    if act_out is not None and in_act != ACT_NONE:
        ao = as_nhwc(act_out)
        if ao.shape != dy.shape or ao.dtype != dy.dtype or ao.stride() != dy.stride():
            raise _lib.DiscoganHipError("c3_dgrad: act_out must have dy's shape, type and layout")
        with _hbm("edge_c3_dgrad", 2.0 * dy.numel() * dy.element_size() + 4.0 * dx.numel()):
            _lib.check(L.dg_conv4x4s2_c3_dgrad_act_p(_ptr(dy), int(_is16(dy)), _ptr(ao), in_act, float(slope), _ptr(w), _ptr(dx), n, 2 * ho, 2 * wo, k,
                                                     act, _CUR.cprec, _ptr(ws), wsb, _stream()), "dg_conv4x4s2_c3_dgrad_act_p")
        return dx
    if _is16(dy) and not L.dg_c3_dgrad_act_ok(n, 2 * ho, 2 * wo, k, 1):
        # only the scatter kernel reads a bf16 dy; past its 2^31-byte limit (or with option "kt" 16) the fp32 kernels get an fp32 copy
        dyf = torch.empty_like(dy, dtype=torch.float32)
        dyf.copy_(dy)
        dy = dyf
    with _hbm("edge_c3_dgrad", dy.numel() * dy.element_size() + 4.0 * dx.numel()):
        _lib.check(L.dg_conv4x4s2_c3_dgrad_p(_ptr(dy), int(_is16(dy)), _ptr(w), _ptr(dx), n, 2 * ho, 2 * wo, k, act, _CUR.cprec, _ptr(ws), wsb,
                                             _stream()), "dg_conv4x4s2_c3_dgrad_p")
    return dx


def c3_wgrad(dy, x_nchw, out=None, accumulate=False, act_out=None, act=ACT_NONE, slope=0.0):
    """dw [K,3,4,4] contiguous from dy NHWC-memory [N,K,Ho,Wo] and x NCHW [N,3,H,W].  With ``act_out`` (the saved
    output of the layer's fused LeakyReLU/ReLU) dy is taken through the activation backward on the fly."""
    _check_dev(dy, act_out, allow16=True)
    _check_dev(x_nchw)
    dy = as_nhwc(dy)
    x = x_nchw.contiguous()
    n, k, ho, wo = dy.shape
    h, wd = x.shape[2], x.shape[3]
    dw = out if out is not None else torch.empty((k, 3, 4, 4), device=dy.device, dtype=torch.float32)
    L = _lib.load()
    ws, wsb = _ws(L.dg_c3_wgrad_workspace_bytes(n, h, wd, k), dy.device)
    fuse = act_out is not None and act != ACT_NONE
    ao = None
    if fuse:
        ao = as_nhwc(act_out)
        assert ao.shape == dy.shape and ao.dtype == dy.dtype
    with _hbm("edge_c3_wgrad", float(dy.element_size()) * ((2 if fuse else 1) * dy.numel()) + 4.0 * x.numel()):
        _lib.check(L.dg_conv4x4s2_c3_wgrad_p(_ptr(dy), _ptr(ao), int(_is16(dy)), act if fuse else ACT_NONE, float(slope), _ptr(x), _ptr(dw),
                                             n, h, wd, k, _CUR.cprec, int(accumulate), _ptr(ws), wsb, _stream()), "dg_conv4x4s2_c3_wgrad_p")
    return dw


def c3_tail_bn_ok(y, need_wgrad=True):
    """Last decoder group [BatchNorm][ReLU][ConvTranspose2d(K, 3)]: do the 3-channel kernels take the BatchNorm's INPUT ``y`` and apply
    BatchNorm + ReLU to the values they load (c3_dgrad_bn / c3_wgrad_bn) under the current context?  fp32 storage, exact-fp32 or f32x3
    arithmetic, K == 64, and the sizes dg_c3_dgrad_bn_ok / dg_c3_wgrad_bn_ok accept."""
    if _is16(y) or _CUR.act16 or _CUR.shadow:
        return False
    n, k, ho, wo = y.shape
    L = _lib.load()
    return bool(L.dg_c3_dgrad_bn_ok(n, 2 * ho, 2 * wo, k, _CUR.cprec)) and \
        (not need_wgrad or bool(L.dg_c3_wgrad_bn_ok(n, 2 * ho, 2 * wo, k, _CUR.cprec)))


def c3_dgrad_bn(y, saved, gamma, beta, w, act=ACT_NONE, bn_act=ACT_RELU):
    """Bitwise c3_dgrad(bn_act_fwd(y, saved, gamma, beta, bn_act), w, act) without the BatchNorm apply pass: the scatter kernel reads
    ``y`` and applies BatchNorm + ReLU on load (needs c3_tail_bn_ok(y))."""
    _check_dev(y, saved, gamma, beta, w)
    y = as_nhwc(y)
    w = w.contiguous()
    n, k, ho, wo = y.shape
    dx = torch.empty((n, 3, 2 * ho, 2 * wo), device=y.device, dtype=torch.float32)
    with _hbm("edge_c3_dgrad", 4.0 * y.numel() + 4.0 * dx.numel()):
        _lib.check(_lib.load().dg_conv4x4s2_c3_dgrad_bn_p(_ptr(y), _ptr(saved), _ptr(gamma), _ptr(beta), bn_act, _ptr(w), _ptr(dx), n, 2 * ho, 2 * wo,
                                                          k, act, _CUR.cprec, _stream()), "dg_conv4x4s2_c3_dgrad_bn_p")
    return dx


def c3_wgrad_bn(y, saved, gamma, beta, x_nchw, out=None, accumulate=False, bn_act=ACT_RELU):
    """Bitwise c3_wgrad(bn_act_fwd(y, saved, gamma, beta, bn_act), x_nchw, out, accumulate) from the BatchNorm's input ``y``."""
    _check_dev(y, saved, gamma, beta, x_nchw)
    y = as_nhwc(y)
    x = x_nchw.contiguous()
    n, k, ho, wo = y.shape
    h, wd = x.shape[2], x.shape[3]
    dw = out if out is not None else torch.empty((k, 3, 4, 4), device=y.device, dtype=torch.float32)
    L = _lib.load()
    ws, wsb = _ws(L.dg_c3_wgrad_workspace_bytes(n, h, wd, k), y.device)
    with _hbm("edge_c3_wgrad", 4.0 * y.numel() + 4.0 * x.numel()):
        _lib.check(L.dg_conv4x4s2_c3_wgrad_bn_p(_ptr(y), _ptr(saved), _ptr(gamma), _ptr(beta), bn_act, _ptr(x), _ptr(dw), n, h, wd, k, _CUR.cprec,
                                                int(accumulate), _ptr(ws), wsb, _stream()), "dg_conv4x4s2_c3_wgrad_bn_p")
    return dw


# ---- BatchNorm + activation -----------------------------------------------------------------------------
def bn_train_stats(y, running_mean, running_var, nbt, eps, momentum):
    _check_dev(y, allow16=True)
    y = as_nhwc(y)
    n, c, h, w = y.shape
    m = n * h * w
    saved = torch.empty((2, c), device=y.device, dtype=torch.float32)
    L = _lib.load()
    ws, wsb = _ws(L.dg_bn_workspace_bytes(m, c), y.device)
    with _hbm("bn_stats", float(y.element_size()) * m * c):
        _lib.check(L.dg_bn_train_stats_t(_ptr(y), int(_is16(y)), m, c, eps, momentum, _ptr(running_mean), _ptr(running_var), _ptr(nbt),
                                         _ptr(saved), _ptr(ws), wsb, _stream()), "dg_bn_train_stats")
    return saved


_PARTIALS_ONE_LAUNCH = _env_flag("DG_BN_PARTIALS_ONE_LAUNCH", False)     # same-box A/B of the two-level merge


def bn_stats_from_partials(stat, y, running_mean, running_var, nbt, eps, momentum):
    """Same result as bn_train_stats(y, ...) from the partial rows a conv kernel emitted for y."""
    _check_dev(stat)
    n, c, h, w = y.shape
    saved = torch.empty((2, c), device=y.device, dtype=torch.float32)
    L = _lib.load()
    ws, wsb = (None, 0) if _PARTIALS_ONE_LAUNCH else _ws(L.dg_bn_partials_workspace_bytes(stat.shape[0], c), y.device)
    _lib.check(L.dg_bn_stats_from_partials(_ptr(stat), stat.shape[0], n * h * w, c, eps, momentum,
                                           _ptr(running_mean), _ptr(running_var), _ptr(nbt), _ptr(saved),
                                           _ptr(ws), wsb, _stream()), "dg_bn_stats_from_partials")
    return saved


def _bn_out(y, planes_cm, planes_only):
    """The output form of a BatchNorm apply pass (forward or backward) over ``y`` under the current context, with its empty tensors:
    (form, out, extra, cm, plane_only).
      "bf16"    bf16 activation storage: bf16 in, bf16 out, nothing else is written
      "planes"  f32x3 path: the convs after this pass read ``out`` as the plane triple ``extra`` (quad-chunk if cm: its reader is a window
                input-grad kernel); plane_only: every reader is a plane kernel, the fp32 copy is not written (X3_PLANES_ONLY)
      "shadow"  bf16 path: ``extra`` is the bf16 shadow of ``out``
      "plain"   fp32 only"""
    n, c, h, w = y.shape
    if _is16(y):
        return "bf16", empty_nhwc(n, c, h, w, y.device, torch.bfloat16), None, 0, False
    out = empty_nhwc(n, c, h, w, y.device)
    if _CUR.x3 and c % 8 == 0:
        extra = torch.empty((3, out.numel()), device=y.device, dtype=torch.bfloat16)
        cm = int(bool(planes_cm) and c % 64 == 0 and (n * h * w) % 4 == 0)
        return "planes", out, extra, cm, bool(planes_only) and X3_PLANES_ONLY
    if _CUR.shadow and c % 8 == 0:
        return "shadow", out, empty_nhwc_bf16(n, c, h, w, y.device), 0, False
    return "plain", out, None, 0, False


def _bn_publish(form, out, extra, cm, plane_only):
    """Make what a BatchNorm pass wrote beside ``out`` known to the convs that read it; returns ``out``."""
    if form == "planes":
        planes_put(out, extra, cm)
        if plane_only:
            out._dg_planes_only = True
            if POISON_PLANES_ONLY:
                out.fill_(float("nan"))
    elif form == "shadow":
        shadow_put(out, extra)
    return out


# algorithmic bytes per element of (M, C), by output form (planes_only: "planes" without the fp32 copy)
_BN_FWD_BYTES = {"bf16": 4.0, "planes": 14.0, "planes_only": 10.0, "shadow": 10.0, "plain": 8.0}
_BN_BWD_BYTES = {"bf16": 10.0, "planes": 26.0, "planes_only": 22.0, "shadow": 22.0, "plain": 20.0}


def bn_act_fwd(y, saved, gamma, beta, act, slope=0.2, planes_cm=False, planes_only=False):
    """planes_cm (f32x3 plane path): write z's plane triple in the quad-chunk layout (its reader is a window input-grad kernel);
    planes_only: every reader of z is a plane kernel -> the fp32 copy is not written (X3_PLANES_ONLY)."""
    _check_dev(y, allow16=True)
    y = as_nhwc(y)
    n, c, h, w = y.shape
    m = n * h * w
    form, z, extra, cm, po = _bn_out(y, planes_cm, planes_only)
    L = _lib.load()
    rest = (m, c, _ptr(saved), _ptr(gamma), _ptr(beta), act, slope, _stream())
    with _hbm("bn_apply", _BN_FWD_BYTES["planes_only" if po else form] * m * c):
        if form == "bf16":
            _lib.check(L.dg_bn_act_fwd_t(_ptr(y), _ptr(z), 1, *rest), "dg_bn_act_fwd_t")
        elif form == "planes":
            _lib.check(L.dg_bn_act_fwd_x3(_ptr(y), None if po else _ptr(z), _ptr(extra), extra.stride(0), cm, *rest), "dg_bn_act_fwd_x3")
        elif form == "shadow":
            _lib.check(L.dg_bn_act_fwd_bf16(_ptr(y), _ptr(z), _ptr(extra), *rest), "dg_bn_act_fwd_bf16")
        else:
            _lib.check(L.dg_bn_act_fwd(_ptr(y), _ptr(z), *rest), "dg_bn_act_fwd")
    return _bn_publish(form, z, extra, cm, po)


def bn_act_bwd(dz, y, saved, gamma, beta, act, slope=0.2, need_param_grads=True, out_grads=None, planes_cm=False, planes_only=False,
               accumulate=True):
    """out_grads=(dgamma_buf, dbeta_buf): accumulate the parameter gradients into those buffers in place (accumulate=False: overwrite).
    planes_cm (f32x3 plane path): write dy's plane triple chunk-major (its reader is a window input-grad kernel)."""
    _check_dev(dz, y, allow16=True)
    dz = as_nhwc(dz)
    y = as_nhwc(y)
    n, c, h, w = y.shape
    m = n * h * w
    acc = 0
    if out_grads is not None:
        dgamma, dbeta = out_grads
        acc = int(bool(accumulate))
    else:
        dgamma = torch.empty(c, device=y.device, dtype=torch.float32) if need_param_grads else None
        dbeta = torch.empty(c, device=y.device, dtype=torch.float32) if need_param_grads else None
    L = _lib.load()
    ws, wsb = _ws(L.dg_bn_workspace_bytes(m, c), y.device)
    if _is16(y) and not _is16(dz):
        raise _lib.DiscoganHipError("bn_act_bwd: bf16 y needs a bf16 dz")
    form, dy, extra, cm, po = _bn_out(y, planes_cm, planes_only)
    rest = (m, c, _ptr(saved), _ptr(gamma), _ptr(beta), act, slope, _ptr(dgamma), _ptr(dbeta), acc, _ptr(ws), wsb, _stream())
    with _hbm("bn_backward", _BN_BWD_BYTES["planes_only" if po else form] * m * c):
        if form == "bf16":
            _lib.check(L.dg_bn_act_bwd_t(_ptr(dz), _ptr(y), _ptr(dy), 1, *rest), "dg_bn_act_bwd_t")
        elif form == "planes":
            _lib.check(L.dg_bn_act_bwd_x3(_ptr(dz), _ptr(y), None if po else _ptr(dy), _ptr(extra), extra.stride(0), cm, *rest), "dg_bn_act_bwd_x3")
        elif form == "shadow":
            _lib.check(L.dg_bn_act_bwd_bf16(_ptr(dz), _ptr(y), _ptr(dy), _ptr(extra), *rest), "dg_bn_act_bwd_bf16")
        else:
            _lib.check(L.dg_bn_act_bwd(_ptr(dz), _ptr(y), _ptr(dy), *rest), "dg_bn_act_bwd")
    return _bn_publish(form, dy, extra, cm, po), dgamma, dbeta


def _dense_like(x):
    """empty tensor with x's shape AND memory layout (x must be dense)."""
    return torch.empty_like(x, memory_format=torch.preserve_format)


def _dense(x):
    if x.is_contiguous() or is_nhwc(x):
        return x
    return x.contiguous()


def act_fwd(x, act, slope=0.2):
    _check_dev(x)
    x = _dense(x)
    y = _dense_like(x)
    _lib.check(_lib.load().dg_act_fwd(_ptr(x), _ptr(y), x.numel(), act, slope, _stream()), "dg_act_fwd")
    return y


def act_bwd(dy, out, act, slope=0.2):
    """Elementwise; dy is brought to out's memory layout first."""
    _check_dev(dy, out, allow16=True)
    out = _dense(out)
    if dy.stride() != out.stride():
        dyl = _dense_like(out)
        dyl.copy_(dy)
        dy = dyl
    dx = _dense_like(out)
    if _is16(out) or _is16(dy):
        if dy.dtype != out.dtype:
            raise _lib.DiscoganHipError("act_bwd: dy and out must have the same dtype")
        _lib.check(_lib.load().dg_act_bwd_t(_ptr(dy), _ptr(out), _ptr(dx), 1, out.numel(), act, slope, _stream()), "dg_act_bwd_t")
        return dx
    _lib.check(_lib.load().dg_act_bwd(_ptr(dy), _ptr(out), _ptr(dx), out.numel(), act, slope, _stream()), "dg_act_bwd")
    return dx


# ---- losses ---------------------------------------------------------------------------------------------
def _loss_ws(device):
    L = _lib.load()
    return _ws(L.dg_loss_workspace_bytes(), device)


def same_layout_pair(a, b):
    """Bring b to a's dense memory layout (elementwise kernels index memory linearly)."""
    a = _dense(a)
    if b.stride() != a.stride():
        bl = _dense_like(a)
        bl.copy_(b)
        b = bl
    return a, b


def mse_fwd(x, t, out=None):
    _check_dev(x, t)
    x, t = same_layout_pair(x, t)
    loss = out if out is not None else torch.empty((), device=x.device, dtype=torch.float32)
    ws, wsb = _loss_ws(x.device)
    _lib.check(_lib.load().dg_mse_fwd(_ptr(x), _ptr(t), x.numel(), _ptr(loss), _ptr(ws), wsb, _stream()), "dg_mse_fwd")
    return loss, x, t


def mse_bwd(x, t, gout):
    _check_dev(x, t, gout)
    dx = _dense_like(x)
    _lib.check(_lib.load().dg_mse_bwd(_ptr(x), _ptr(t), x.numel(), _ptr(gout), _ptr(dx), _stream()), "dg_mse_bwd")
    return dx


# Reconstruction criterion (dg_recon_loss_*): w = (w_mse, w_l1, w_ssim) host floats; x the reconstruction, t the real image (data)
def _recon_args(who, xs, ts, w):
    """The argument checks of the recon_loss_* wrappers.  Returns (n, S, the weights as a C float[3])."""
    import ctypes as C
    import math
    w = tuple(float(v) for v in w)
    if len(w) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in w) or not any(v > 0.0 for v in w):
        raise _lib.DiscoganHipError(f"{who}: the weights (w_mse, w_l1, w_ssim) must be three finite numbers >= 0, not all 0, got {w}")
    _check_dev(*xs, *ts)
    x0 = xs[0]
    for x, t in zip(xs, ts):
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise _lib.DiscoganHipError(f"{who} needs [n,3,S,S] image batches, got {tuple(x.shape)}")
        if tuple(t.shape) != tuple(x.shape) or tuple(x.shape) != tuple(x0.shape) or t.device != x0.device or x.device != x0.device:
            raise _lib.DiscoganHipError(f"{who}: input and target must have one shape on one device, got {tuple(x.shape)} and {tuple(t.shape)}")
        if not (x.is_contiguous() and t.is_contiguous()):
            raise _lib.DiscoganHipError(f"{who} needs contiguous NCHW batches")
        if t.requires_grad:
            raise _lib.DiscoganHipError(f"{who}: the target is data -- no gradient with respect to it exists; detach it")
    n, S = int(x0.shape[0]), int(x0.shape[3])
    if n < 1 or S < 1:
        raise _lib.DiscoganHipError(f"{who}: empty batch {tuple(x0.shape)}")
    if w[2] > 0.0 and S < 11:
        raise _lib.DiscoganHipError(f"{who}: the SSIM term needs S >= 11 pixels (the 11 x 11 window), got S={S}")
    return n, S, (C.c_float * 3)(*w)


def recon_loss_fwd(x, t, w, out=None):
    """loss = w_mse mean (x - t)^2 + w_l1 mean |x - t| + w_ssim (1 - mean SSIM) of two float32 NCHW batches [n,3,S,S], a device scalar
    (``out``: the slot to write it into)."""
    n, S, cw = _recon_args("recon_loss_fwd", [x], [t], w)
    loss = out if out is not None else torch.empty((), device=x.device, dtype=torch.float32)
    L = _lib.load()
    ws, wsb = _ws(L.dg_recon_loss_workspace_bytes(n, S), x.device)
    _lib.check(L.dg_recon_loss_fwd(_ptr(x), _ptr(t), n, S, cw, _ptr(loss), _ptr(ws), wsb, _stream()), "dg_recon_loss_fwd")
    return loss


def recon_loss_bwd(x, t, w, gout):
    """d loss / d x times the device scalar ``gout`` (one pass, overwriting)."""
    n, S, cw = _recon_args("recon_loss_bwd", [x], [t], w)
    _check_dev(gout)
    dx = torch.empty_like(x)
    _lib.check(_lib.load().dg_recon_loss_bwd(_ptr(x), _ptr(t), n, S, cw, _ptr(gout), _ptr(dx), _stream()), "dg_recon_loss_bwd")
    return dx


# Multi-scale SSIM criterion (dg_ms_ssim_loss_*): w = (w_mse, w_l1, w_ms) host floats, M scales (0: as many as the size carries)
def ms_ssim_max_scales(S):
    """min(5, number of j with S >> j >= 11): the scales an S x S image carries (0 under 11 pixels)."""
    return int(_lib.load().dg_ms_ssim_max_scales(int(S)))


def _ms_args(who, xs, ts, M, w):
    """The argument checks of the ms_ssim_* wrappers.  Returns (n, S, M, the weights as a C float[3])."""
    n, S, cw = _recon_args(who, xs, ts, w)
    top = ms_ssim_max_scales(S)
    if top < 1:
        raise _lib.DiscoganHipError(f"{who}: multi-scale SSIM needs S >= 11 pixels (the 11 x 11 window), got S={S}")
    M = top if int(M) == 0 else int(M)
    if not 1 <= M <= top:
        raise _lib.DiscoganHipError(f"{who}: {M} scales at S={S}: every scale needs a side >= 11, so 1..{top} (0: the maximum)")
    return n, S, M, cw


def _ms_save(L, n, S, M, g, device):
    """The caller-owned buffers the forward fills for the backward (pyramids of x and t, the k table), one per problem."""
    nbytes = L.dg_ms_ssim_save_bytes(n, S, M)
    per = (nbytes + 255) // 256 * 64
    t = torch.empty(g * per, device=device, dtype=torch.float32)
    return [t[i * per:(i + 1) * per] for i in range(g)], nbytes


def ms_ssim_loss_fwd(x, t, M, w, out=None):
    """loss = w_mse mean (x - t)^2 + w_l1 mean |x - t| + w_ms (1 - mean MS-SSIM) of two float32 NCHW batches [n,3,S,S] over M scales.
    Returns (loss: a device scalar -- ``out``, the slot to write it into --, save: the buffer ``ms_ssim_loss_bwd`` reads)."""
    n, S, M, cw = _ms_args("ms_ssim_loss_fwd", [x], [t], M, w)
    loss = out if out is not None else torch.empty((), device=x.device, dtype=torch.float32)
    L = _lib.load()
    ws, wsb = _ws(L.dg_ms_ssim_workspace_bytes(n, S, M), x.device)
    (save,), sb = _ms_save(L, n, S, M, 1, x.device)
    _lib.check(L.dg_ms_ssim_loss_fwd(_ptr(x), _ptr(t), n, S, M, cw, _ptr(loss), _ptr(save), sb, _ptr(ws), wsb, _stream()), "dg_ms_ssim_loss_fwd")
    return loss, save


def ms_ssim_loss_bwd(x, t, M, w, gout, save):
    """d loss / d x times the device scalar ``gout`` (overwriting); ``save``: what ``ms_ssim_loss_fwd`` returned for these x, t, M."""
    n, S, M, cw = _ms_args("ms_ssim_loss_bwd", [x], [t], M, w)
    _check_dev(gout, save)
    dx = torch.empty_like(x)
    L = _lib.load()
    ws, wsb = _ws(L.dg_ms_ssim_bwd_workspace_bytes(n, S, M), x.device)
    _lib.check(L.dg_ms_ssim_loss_bwd(_ptr(x), _ptr(t), n, S, M, cw, _ptr(gout), _ptr(save), save.numel() * 4, _ptr(dx), _ptr(ws), wsb, _stream()),
               "dg_ms_ssim_loss_bwd")
    return dx


def image_ms_ssim(x, y, M=0):
    """Two float32 NCHW batches [n,3,S,S] (S >= 11) -> float32 [n] on the device: the multi-scale SSIM of the pair (x[i], y[i]) over M
    scales (0: ``ms_ssim_max_scales(S)``), the mean over the channels.  Row i depends on pair i alone and is bitwise repeatable."""
    xc, yc = x.detach().contiguous(), y.detach().contiguous()
    n, S, M, _ = _ms_args("image_ms_ssim", [xc], [yc], M, (0.0, 0.0, 1.0))
    out = torch.empty((n,), device=x.device, dtype=torch.float32)
    L = _lib.load()
    ws, wsb = _ws(L.dg_ms_ssim_workspace_bytes(n, S, M), x.device)
    _lib.check(L.dg_image_ms_ssim(_ptr(xc), _ptr(yc), n, S, M, _ptr(out), _ptr(ws), wsb, _stream()), "dg_image_ms_ssim")
    return out


def bce_fwd(p, label, out=None):
    _check_dev(p)
    p = p.contiguous()
    loss = out if out is not None else torch.empty((), device=p.device, dtype=torch.float32)
    _lib.check(_lib.load().dg_bce_fwd(_ptr(p), p.numel(), float(label), _ptr(loss), None, 0, _stream()), "dg_bce_fwd")
    return loss, p


def bce_bwd(p, label, gout):
    dp = torch.empty_like(p)
    _lib.check(_lib.load().dg_bce_bwd(_ptr(p), p.numel(), float(label), _ptr(gout), _ptr(dp), _stream()), "dg_bce_bwd")
    return dp


# Adversarial objectives on logits (dg_gan_loss_*): kind / role are the library's codes, real_label the target of the D_REAL role
GAN_BCE_LOGITS, GAN_LSGAN, GAN_HINGE = 0, 1, 2
GAN_D_REAL, GAN_D_FAKE, GAN_G_FAKE = 0, 1, 2


def gan_loss_fwd(x, kind, role, real_label=1.0, out=None):
    """mean_i f(x_i) of the logits ``x`` (include/discogan_hip.h: dg_gan_loss_fwd).  Returns (loss, the contiguous logits)."""
    _check_dev(x)
    x = x.contiguous()
    loss = out if out is not None else torch.empty((), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().dg_gan_loss_fwd(_ptr(x), x.numel(), int(kind), int(role), float(real_label), _ptr(loss), _stream()), "dg_gan_loss_fwd")
    return loss, x


def gan_loss_bwd(x, kind, role, real_label, gout):
    dx = torch.empty_like(x)
    _lib.check(_lib.load().dg_gan_loss_bwd(_ptr(x), x.numel(), int(kind), int(role), float(real_label), _ptr(gout), _ptr(dx), _stream()),
               "dg_gan_loss_bwd")
    return dx


def bce_target_fwd(p, target, out=None):
    _check_dev(p, target)
    p, target = p.contiguous(), target.contiguous()
    if p.numel() != target.numel():
        raise ValueError(f"Using a target size ({tuple(target.shape)}) that is different to the input size ({tuple(p.shape)}) is deprecated. Please ensure they have the same size.")
    loss = out if out is not None else torch.empty((), device=p.device, dtype=torch.float32)
    _lib.check(_lib.load().dg_bce_target_fwd(_ptr(p), _ptr(target), p.numel(), _ptr(loss), _stream()), "dg_bce_target_fwd")
    return loss, p, target


def bce_target_bwd(p, target, gout):
    dp = torch.empty_like(p)
    _lib.check(_lib.load().dg_bce_target_bwd(_ptr(p), _ptr(target), p.numel(), _ptr(gout), _ptr(dp), _stream()), "dg_bce_target_bwd")
    return dp


def hinge_fwd(x, y, margin=1.0):
    _check_dev(x, y)
    x, y = same_layout_pair(x, y)
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    ws, wsb = _loss_ws(x.device)
    _lib.check(_lib.load().dg_hinge_fwd(_ptr(x), _ptr(y), x.numel(), float(margin), _ptr(loss), _ptr(ws), wsb, _stream()), "dg_hinge_fwd")
    return loss, x, y


def hinge_bwd(x, y, margin, gout):
    dx = _dense_like(x)
    _lib.check(_lib.load().dg_hinge_bwd(_ptr(x), _ptr(y), x.numel(), float(margin), _ptr(gout), _ptr(dx), _stream()), "dg_hinge_bwd")
    return dx


def fm_fwd(real, fake, out=None):
    """One layer of get_fm_loss; real/fake logical [N,C,H,W] with identical dense layouts."""
    _check_dev(real, fake, allow16=True)
    real, fake = same_layout_pair(real, fake)
    n = real.shape[0]
    j = real.numel() // n
    diff = torch.empty(j, device=real.device, dtype=torch.float32)
    loss = out if out is not None else torch.empty((), device=real.device, dtype=torch.float32)
    ws, wsb = _ws(_lib.load().dg_fm_workspace_bytes(n, j), real.device)
    if real.dtype != fake.dtype:
        raise _lib.DiscoganHipError("fm_fwd: real and fake features must have the same dtype")
    _lib.check(_lib.load().dg_fm_fwd_t(_ptr(real), _ptr(fake), int(_is16(real)), n, j, _ptr(diff), _ptr(loss), _ptr(ws), wsb, _stream()),
               "dg_fm_fwd")
    return loss, diff, real, fake


def fm_bwd(diff, like_real, like_fake, gout, need_real, need_fake):
    n = like_fake.shape[0]
    j = diff.numel()
    dreal = _dense_like(like_real) if need_real else None
    dfake = _dense_like(like_fake) if need_fake else None
    _lib.check(_lib.load().dg_fm_bwd_t(_ptr(diff), n, j, _ptr(gout), _ptr(dreal), _ptr(dfake), int(_is16(like_fake)), _stream()), "dg_fm_bwd")
    return dreal, dfake


def loss_mix_fwd(lossvec, nfm, rate, arch):
    out = torch.empty(8, device=lossvec.device, dtype=torch.float32)
    _lib.check(_lib.load().dg_loss_mix_fwd(_ptr(lossvec), _ptr(out), nfm, float(rate), arch, _stream()), "dg_loss_mix_fwd")
    return out


def loss_mix_bwd(gout, nslots, nfm, rate, arch, which):
    gv = torch.empty(nslots, device=gout.device, dtype=torch.float32)
    _lib.check(_lib.load().dg_loss_mix_bwd(_ptr(gout), _ptr(gv), nfm, float(rate), arch, which, _stream()), "dg_loss_mix_bwd")
    return gv


# ---- Adam -----------------------------------------------------------------------------------------------
def adam_advance(state, lr, beta1, beta2, ctl=None):
    """ctl: the step's control block (grad_clip_finalize); a skipped step (ctl[3] != 0) leaves the state untouched."""
    if ctl is not None:
        _check_ctl(ctl, "adam_advance")
    _lib.check(_lib.load().dg_adam_advance(_ptr(state), lr, beta1, beta2, _ptr(ctl), _stream()), "dg_adam_advance")


def adam_step_flat(p, g, m, v, state, beta1, beta2, eps, weight_decay, grad_scale=1.0, p16=None, p3=None, ctl=None):
    """p3: (plane-0 address of this range, plane distance in elements), the f32x3 plane triples; p16: the bf16 shadow.  ctl: the gradient
    scale (float32(ctl[2])) and the skip flag (ctl[3]) are read on the device; grad_scale is then unused."""
    if ctl is not None:
        _check_ctl(ctl, "adam_step_flat")
    form, out, dist = (3, p3[0], p3[1]) if p3 is not None else ((1, _ptr(p16), 0) if p16 is not None else (0, None, 0))
    with _hbm("adam", (28.0 + 2.0 * form) * p.numel()):
        _lib.check(_lib.load().dg_adam_step_flat(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(state), beta1, beta2, eps,
                                                 weight_decay, grad_scale, _ptr(ctl), out, form, dist, _stream()), "dg_adam_step_flat")


# ADAM_FUSED_T: the f32x3 step of a whole group (optim.Adam.step, active is None) writes the transposed weight planes itself
# (dg_adam_step_group_x3: 40 B/param of a conv weight) instead of dg_adam_step_flat (form 3) followed by dg_x3_transpose_planes, which reads
# the planes back (34 + 12 B/param).  Bit-identical; DG_ADAM_FUSED_T=0 restores the two-kernel form (A/B timing).
ADAM_FUSED_T = _env_flag("DG_ADAM_FUSED_T", True)
# LAZY_ZERO_GRAD: the trainer's iteration does not zero-fill the stepped flat gradient buffer (optim.Adam.zero_grad(lazy=True)); the
# first weight-gradient kernel of every parameter overwrites instead of adding to zeros it would have to read (4 + 4 B/param).
# 0 + x and x differ for x = -0 only, which changes no bit of p, m, v; DG_LAZY_ZERO_GRAD=0 restores the fill (A/B timing).
LAZY_ZERO_GRAD = _env_flag("DG_LAZY_ZERO_GRAD", True)


def adam_group_x3_table(weights, ranges):
    """Host-side tables for adam_step_group_x3: weights = [(element offset, K, J = 16 C), ...] with K % 64 == 0 and J % 64 == 0 (stepped
    by tiles, transposed planes included), ranges = [(begin, end), ...] for everything else; both ascending."""
    import ctypes as C
    nw, nr = len(weights), len(ranges)
    return (nw, (C.c_int64 * max(nw, 1))(*[w[0] for w in weights]), (C.c_int * max(nw, 1))(*[w[1] for w in weights]),
            (C.c_int * max(nw, 1))(*[w[2] for w in weights]),
            nr, (C.c_int64 * max(nr, 1))(*[r[0] for r in ranges]), (C.c_int64 * max(nr, 1))(*[r[1] - r[0] for r in ranges]))


def adam_step_group_x3(p, g, m, v, state, beta1, beta2, eps, weight_decay, grad_scale, p3, p3t, table, ctl=None):
    """One f32x3 Adam step of the whole flat group ``p``: the weights of ``table`` also get their transposed planes in ``p3t``; the bits
    of adam_step_flat(p3=...) followed by x3_transpose_planes.  ctl: as adam_step_flat (grad_scale is then unused)."""
    _check_dev(p, g, m, v)
    if ctl is not None:
        _check_ctl(ctl, "adam_step_group_x3")
    nw, w_off, w_k, w_j, nr, r_off, r_len = table
    assert p3.shape == (3, p.numel()) and p3.stride(1) == 1 and (nw == 0 or (p3t.shape == p3.shape and p3t.stride(0) == p3.stride(0)))
    nbytes = 40.0 * sum(int(w_k[i]) * int(w_j[i]) for i in range(nw)) + 34.0 * sum(int(r_len[i]) for i in range(nr))
    with _hbm("adam", nbytes):
        _lib.check(_lib.load().dg_adam_step_group_x3(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(state), beta1, beta2, eps,
                                                     weight_decay, grad_scale, _ptr(ctl), _ptr(p3), _ptr(p3t) if nw else None,
                                                     p3.stride(0), w_off, w_k, w_j, nw, r_off, r_len, nr, _stream()),
                   "dg_adam_step_group_x3")


# ---- gradient norm / clipping / non-finite guard (include/discogan_hip.h: the control block ctl) ---------
GRAD_STATS_MAX_GRID = 4096          # blocks of one dg_grad_sumsq_partial launch = partial slots of one range at most


def _check_ctl(ctl, who):
    if not (ctl.is_cuda and ctl.dtype == torch.float64 and ctl.dim() == 1 and ctl.numel() >= 8 and ctl.is_contiguous()):
        raise _lib.DiscoganHipError(f"{who}: ctl must be a contiguous float64 HIP tensor of 8 elements")


def grad_stats_workspace(device):
    """The partial-sum workspace of grad_sumsq_partial / grad_clip_finalize (float64 slots)."""
    return torch.zeros(_lib.load().dg_grad_stats_workspace_bytes() // 8, device=device, dtype=torch.float64)


def grad_sumsq_partial(g, ws, slot0=0):
    """One fp64 partial sum of squares per block of the flat fp32 range ``g`` into ``ws[slot0:]``; returns the number of slots used."""
    _check_dev(g)
    if g.dim() != 1 or not g.is_contiguous():
        raise _lib.DiscoganHipError(f"grad_sumsq_partial: a contiguous 1-D fp32 tensor required, got {tuple(g.shape)}")
    if not (ws.is_cuda and ws.dtype == torch.float64 and ws.dim() == 1 and ws.is_contiguous()):
        raise _lib.DiscoganHipError("grad_sumsq_partial: the workspace must be a contiguous float64 HIP tensor")
    import ctypes as C
    used = C.c_int(0)
    with _hbm("gradnorm", 4.0 * g.numel()):
        _lib.check(_lib.load().dg_grad_sumsq_partial(_ptr(g), g.numel(), _ptr(ws), ws.numel() * 8, int(slot0), C.byref(used), _stream()),
                   "dg_grad_sumsq_partial")
    return used.value


def grad_clip_finalize(ws, slots, pre_scale, max_norm, guard, ctl):
    """Fold ``ws[:slots]`` into the control block: ctl[0] sumsq, [1] norm = sqrt(sumsq) * pre_scale, [2] scale = pre_scale * min(1,
    max_norm / (norm + 1e-6)) (max_norm <= 0: pre_scale), [3] skip = guard and sumsq not finite, [4..7] steps seen / clipped / skipped,
    largest finite norm."""
    _check_ctl(ctl, "grad_clip_finalize")
    if not (ws.is_cuda and ws.dtype == torch.float64 and ws.is_contiguous()) or slots > ws.numel():
        raise _lib.DiscoganHipError(f"grad_clip_finalize: {slots} slots of a float64 HIP workspace of {ws.numel()}")
    _lib.check(_lib.load().dg_grad_clip_finalize(_ptr(ws), int(slots), float(pre_scale), float(max_norm), int(bool(guard)), _ptr(ctl),
                                                 _stream()), "dg_grad_clip_finalize")


def _flat_pair(a, b, who):
    _check_dev(a, b)
    if a.dim() != 1 or b.dim() != 1 or a.numel() != b.numel() or not (a.is_contiguous() and b.is_contiguous()):
        raise _lib.DiscoganHipError(f"{who}: two contiguous 1-D fp32 tensors of one length required, got {tuple(a.shape)} and {tuple(b.shape)}")


def ema_update_flat(ema, p, w):
    """ema += (p - ema) * w in place (w = 1 - decay), each operation rounded on its own: p == ema leaves ema bitwise unchanged."""
    _flat_pair(ema, p, "ema_update_flat")
    with _hbm("ema", 12.0 * p.numel()):
        _lib.check(_lib.load().dg_ema_update_flat(_ptr(ema), _ptr(p), p.numel(), float(w), _stream()), "dg_ema_update_flat")


def swap_flat(a, b):
    """Exchange the contents of two flat fp32 buffers bit for bit."""
    _flat_pair(a, b, "swap_flat")
    with _hbm("swap", 16.0 * a.numel()):
        _lib.check(_lib.load().dg_swap_flat(_ptr(a), _ptr(b), a.numel(), _stream()), "dg_swap_flat")


# ---- grouped launches (round 4) -------------------------------------------------------------------------------------------
# The reference issues the passes of an iteration in independent pairs of identical shape -- G_B(A) | G_A(B), G_A(AB) | G_B(BA),
# D_A(A) | D_B(B), D_A(BA) | D_B(AB) (image_translation.py:342-361) -- and each discriminator sees real and fake images with the same
# weights (:353-354,360-361).  The *_g wrappers take one tensor per problem (lists) and issue ONE launch per kernel for all of them
# (dg_*_g: a block index picks the problem); every problem's result is bitwise what the one-problem wrapper computes.  fp32 tensors on
# the exact-fp32 and the register-staged f32x3 arithmetic only: no shadows, no plane triples, no bf16 storage, no fused statistics.
def group_ok():
    """May the current context run grouped launches?"""
    return not (_CUR.shadow or _CUR.act16 or _CUR.x3)


def _plan_groups(g):
    """Split-K plan of a grouped conv launch: sized for the whole launch (the group fills the chip: fewer K-slabs per problem), or --
    Context.group_plan == "single" -- for every problem as if launched alone (bitwise the ungrouped numbers; tests)."""
    return 1 if getattr(_CUR, "group_plan", "launch") == "single" else g


def _same_shape(ts, who):
    for t in ts[1:]:
        if t.shape != ts[0].shape:
            raise _lib.DiscoganHipError(f"{who}: the problems of a grouped launch must have identical shapes")


def _ws_g(nbytes, g, device):
    """One workspace per problem (slices of ONE allocation): (list of tensors or Nones, bytes each)."""
    if nbytes == 0:
        return [None] * g, 0
    per = (nbytes + 255) // 256 * 64                    # floats per problem, 256-byte aligned
    t = torch.empty(g * per, device=device, dtype=torch.float32)
    return [t[i * per:(i + 1) * per] for i in range(g)], per * 4


def _share_of(params):
    """Consecutive problems that name the SAME parameter (a discriminator's real and fake pass) accumulate into one gradient tensor:
    returns the run length when every run has the same length, else raises."""
    g = len(params)
    run = 1
    while run < g and params[run] is params[0]:
        run += 1
    if g % run != 0 or any(params[i] is not params[i // run * run] for i in range(g)) or \
            any(params[i] is params[i - run] for i in range(run, g, run)):
        raise _lib.DiscoganHipError("grouped launch: problems sharing a parameter must form runs of equal length")
    return run


def _conv_g(op, as_, bs, stride, pad, x_hw=None, outs=None, accumulate=False, share=1):
    """One grouped launch of the fp32-tensor form: the problems' operands as lists, in _ConvReq's order."""
    who = _CONV_NAME[op] + "_g"
    g = len(as_)
    _check_dev(*as_, *bs)
    as_ = [as_nhwc(t) for t in as_]
    bs = [as_nhwc(t) if op == 2 else _krsc(t) for t in bs]
    _same_shape(as_, who)
    _same_shape(bs, who)
    rq = _ConvReq(op, as_[0], bs[0], stride, pad, x_hw)
    pg = _plan_groups(g)
    wsl, wsb = _ws_g(rq.workspace_bytes(pg), g, as_[0].device)
    if outs is None:
        outs = [empty_nhwc(*rq.out_shape, as_[0].device) for _ in range(g)]
    _launch_g(rq, as_, bs, outs, pg, None, wsl, wsb, share, accumulate)
    return outs


def conv_fwd_g(xs, ws_, stride, pad):
    """Conv2d forward of ``len(xs)`` problems in one launch (plus one split-K reduction launch)."""
    return _conv_g(0, xs, ws_, stride, pad)


def conv_dgrad_g(dys, ws_, x_hw, stride, pad):
    return _conv_g(1, dys, ws_, stride, pad, x_hw)


def conv_wgrad_g(dys, xs, stride, pad, outs, accumulate, share=1):
    """Weight gradients of ``len(dys)`` problems into ``outs`` (accumulating views of the flat gradient buffer).  share > 1: every
    ``share`` consecutive problems name the same ``outs`` tensor and are summed into it in problem order."""
    _conv_g(2, dys, xs, stride, pad, None, outs, accumulate, share)


def c3_fwd_g(xs, ws_, act=ACT_NONE, slope=0.2):
    g = len(xs)
    _check_dev(*xs, *ws_)
    xs = [x.contiguous() for x in xs]
    ws_ = [w.contiguous() for w in ws_]
    _same_shape(xs, "c3_fwd_g")
    n, _, h, wd = xs[0].shape
    k = ws_[0].shape[0]
    ys = [empty_nhwc(n, k, h // 2, wd // 2, xs[0].device) for _ in range(g)]
    with _prof("c3_fwd", 2.0 * g * n * (h // 2) * (wd // 2) * k * 48), _hbm("edge_c3_fwd", g * (4.0 * xs[0].numel() + 4.0 * ys[0].numel())):
        _lib.check(_lib.load().dg_conv4x4s2_c3_fwd_g(g, _tab(xs), _tab(ws_), _tab(ys), n, h, wd, k, act, slope, _CUR.cprec, _stream()),
                   "dg_conv4x4s2_c3_fwd_g")
    return ys


def c3_dgrad_g(dys, ws_, act=ACT_NONE):
    g = len(dys)
    _check_dev(*dys, *ws_)
    dys = [as_nhwc(d) for d in dys]
    ws_ = [w.contiguous() for w in ws_]
    _same_shape(dys, "c3_dgrad_g")
    n, k, ho, wo = dys[0].shape
    dxs = [torch.empty((n, 3, 2 * ho, 2 * wo), device=dys[0].device, dtype=torch.float32) for _ in range(g)]
    with _hbm("edge_c3_dgrad", g * (4.0 * dys[0].numel() + 4.0 * dxs[0].numel())):
        _lib.check(_lib.load().dg_conv4x4s2_c3_dgrad_g(g, _tab(dys), _tab(ws_), _tab(dxs), n, 2 * ho, 2 * wo, k, act, _CUR.cprec, _stream()),
                   "dg_conv4x4s2_c3_dgrad_g")
    return dxs


def c3_wgrad_g(dys, xs, outs, accumulate, act_outs=None, act=ACT_NONE, slope=0.0, share=1):
    g = len(dys)
    _check_dev(*dys, *xs)
    dys = [as_nhwc(d) for d in dys]
    xs = [x.contiguous() for x in xs]
    _same_shape(dys, "c3_wgrad_g")
    n, k, ho, wo = dys[0].shape
    h, wd = xs[0].shape[2], xs[0].shape[3]
    fuse = act_outs is not None and act != ACT_NONE
    aos = [as_nhwc(a) for a in act_outs] if fuse else None
    L = _lib.load()
    wsl, wsb = _ws_g(L.dg_c3_wgrad_workspace_bytes(n, h, wd, k), g, dys[0].device)
    with _hbm("edge_c3_wgrad", g * 4.0 * ((2 if fuse else 1) * dys[0].numel() + xs[0].numel())):
        _lib.check(L.dg_conv4x4s2_c3_wgrad_g(g, int(share), _tab(dys), _tab(aos), act if fuse else ACT_NONE, float(slope), _tab(xs), _tab(outs),
                                             n, h, wd, k, _CUR.cprec, int(accumulate), _tab(wsl), wsb, _stream()), "dg_conv4x4s2_c3_wgrad_g")


def bn_train_stats_g(ys, running_means, running_vars, nbts, eps, momentum, share=1):
    g = len(ys)
    _check_dev(*ys)
    ys = [as_nhwc(y) for y in ys]
    _same_shape(ys, "bn_train_stats_g")
    n, c, h, w = ys[0].shape
    m = n * h * w
    saved = [torch.empty((2, c), device=ys[0].device, dtype=torch.float32) for _ in range(g)]
    L = _lib.load()
    wsl, wsb = _ws_g(L.dg_bn_workspace_bytes(m, c), g, ys[0].device)
    with _hbm("bn_stats", 4.0 * g * m * c):
        _lib.check(L.dg_bn_train_stats_g(g, int(share), _tab(ys), m, c, eps, momentum, _tab(running_means), _tab(running_vars), _tab(nbts),
                                         _tab(saved), _tab(wsl), wsb, _stream()), "dg_bn_train_stats_g")
    return saved


def bn_act_fwd_g(ys, saveds, gammas, betas, act, slope=0.2):
    g = len(ys)
    _check_dev(*ys)
    ys = [as_nhwc(y) for y in ys]
    n, c, h, w = ys[0].shape
    zs = [empty_nhwc(n, c, h, w, ys[0].device) for _ in range(g)]
    with _hbm("bn_apply", 8.0 * g * n * h * w * c):
        _lib.check(_lib.load().dg_bn_act_fwd_g(g, _tab(ys), _tab(zs), n * h * w, c, _tab(saveds), _tab(gammas), _tab(betas), act, slope, _stream()),
                   "dg_bn_act_fwd_g")
    return zs


def bn_act_bwd_g(dzs, ys, saveds, gammas, betas, act, slope, dgammas, dbetas, accumulate, share=1):
    """dgammas / dbetas: accumulating views of the flat gradient buffer, or None (parameters frozen)."""
    g = len(dzs)
    _check_dev(*dzs, *ys)
    dzs = [as_nhwc(d) for d in dzs]
    ys = [as_nhwc(y) for y in ys]
    _same_shape(dzs, "bn_act_bwd_g")
    n, c, h, w = ys[0].shape
    m = n * h * w
    dys = [empty_nhwc(n, c, h, w, ys[0].device) for _ in range(g)]
    L = _lib.load()
    wsl, wsb = _ws_g(L.dg_bn_workspace_bytes(m, c), g, ys[0].device)
    with _hbm("bn_backward", 20.0 * g * m * c):
        _lib.check(L.dg_bn_act_bwd_g(g, int(share), _tab(dzs), _tab(ys), _tab(dys), m, c, _tab(saveds), _tab(gammas), _tab(betas), act, slope,
                                     _tab(dgammas), _tab(dbetas), int(accumulate), _tab(wsl), wsb, _stream()), "dg_bn_act_bwd_g")
    return dys


def act_fwd_g(xs, act, slope=0.2):
    _check_dev(*xs)
    xs = [_dense(x) for x in xs]
    ys = [_dense_like(x) for x in xs]
    _lib.check(_lib.load().dg_act_fwd_g(len(xs), _tab(xs), _tab(ys), xs[0].numel(), act, slope, _stream()), "dg_act_fwd_g")
    return ys


def act_bwd_g(dys, outs, act, slope=0.2):
    _check_dev(*dys, *outs)
    outs = [_dense(o) for o in outs]
    dys = list(dys)
    for i, (d, o) in enumerate(zip(dys, outs)):
        if d.stride() != o.stride():
            dl = _dense_like(o)
            dl.copy_(d)
            dys[i] = dl
    dxs = [_dense_like(o) for o in outs]
    _lib.check(_lib.load().dg_act_bwd_g(len(outs), _tab(dys), _tab(outs), _tab(dxs), outs[0].numel(), act, slope, _stream()), "dg_act_bwd_g")
    return dxs


def mse_fwd_g(xs, ts, outs):
    g = len(xs)
    _check_dev(*xs, *ts)
    pairs = [same_layout_pair(x, t) for x, t in zip(xs, ts)]
    xs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    L = _lib.load()
    wsl, wsb = _ws_g(L.dg_loss_workspace_bytes(), g, xs[0].device)
    _lib.check(L.dg_mse_fwd_g(g, _tab(xs), _tab(ts), xs[0].numel(), _tab(outs), _tab(wsl), wsb, _stream()), "dg_mse_fwd_g")
    return xs, ts


def mse_bwd_g(xs, ts, gouts):
    dxs = [_dense_like(x) for x in xs]
    _lib.check(_lib.load().dg_mse_bwd_g(len(xs), _tab(xs), _tab(ts), xs[0].numel(), _tab(gouts), _tab(dxs), _stream()), "dg_mse_bwd_g")
    return dxs


def recon_loss_fwd_g(xs, ts, w, outs):
    n, S, cw = _recon_args("recon_loss_fwd_g", xs, ts, w)
    L = _lib.load()
    wsl, wsb = _ws_g(L.dg_recon_loss_workspace_bytes(n, S), len(xs), xs[0].device)
    _lib.check(L.dg_recon_loss_fwd_g(len(xs), _tab(xs), _tab(ts), n, S, cw, _tab(outs), _tab(wsl), wsb, _stream()), "dg_recon_loss_fwd_g")
    return outs


def recon_loss_bwd_g(xs, ts, w, gouts):
    n, S, cw = _recon_args("recon_loss_bwd_g", xs, ts, w)
    _check_dev(*gouts)
    dxs = [torch.empty_like(x) for x in xs]
    _lib.check(_lib.load().dg_recon_loss_bwd_g(len(xs), _tab(xs), _tab(ts), n, S, cw, _tab(gouts), _tab(dxs), _stream()), "dg_recon_loss_bwd_g")
    return dxs


def ms_ssim_loss_fwd_g(xs, ts, M, w, outs):
    """ms_ssim_loss_fwd of ``len(xs)`` problems of one (n, S, M, w) in one launch per kernel; returns the save buffers, one per problem."""
    n, S, M, cw = _ms_args("ms_ssim_loss_fwd_g", xs, ts, M, w)
    L = _lib.load()
    wsl, wsb = _ws_g(L.dg_ms_ssim_workspace_bytes(n, S, M), len(xs), xs[0].device)
    saves, sb = _ms_save(L, n, S, M, len(xs), xs[0].device)
    _lib.check(L.dg_ms_ssim_loss_fwd_g(len(xs), _tab(xs), _tab(ts), n, S, M, cw, _tab(outs), _tab(saves), sb, _tab(wsl), wsb, _stream()),
               "dg_ms_ssim_loss_fwd_g")
    return saves


def ms_ssim_loss_bwd_g(xs, ts, M, w, gouts, saves):
    n, S, M, cw = _ms_args("ms_ssim_loss_bwd_g", xs, ts, M, w)
    _check_dev(*gouts, *saves)
    dxs = [torch.empty_like(x) for x in xs]
    L = _lib.load()
    wsl, wsb = _ws_g(L.dg_ms_ssim_bwd_workspace_bytes(n, S, M), len(xs), xs[0].device)
    _lib.check(L.dg_ms_ssim_loss_bwd_g(len(xs), _tab(xs), _tab(ts), n, S, M, cw, _tab(gouts), _tab(saves), min(s.numel() for s in saves) * 4,
                                       _tab(dxs), _tab(wsl), wsb, _stream()), "dg_ms_ssim_loss_bwd_g")
    return dxs


def _labels(labels):
    import ctypes as C
    return (C.c_float * len(labels))(*[float(l) for l in labels])


def bce_fwd_g(ps, labels, outs):
    _check_dev(*ps)
    ps = [p.contiguous() for p in ps]
    _lib.check(_lib.load().dg_bce_fwd_g(len(ps), _tab(ps), ps[0].numel(), _labels(labels), _tab(outs), _stream()), "dg_bce_fwd_g")
    return ps


def bce_bwd_g(ps, labels, gouts):
    dps = [torch.empty_like(p) for p in ps]
    _lib.check(_lib.load().dg_bce_bwd_g(len(ps), _tab(ps), ps[0].numel(), _labels(labels), _tab(gouts), _tab(dps), _stream()), "dg_bce_bwd_g")
    return dps


def _roles(roles):
    import ctypes as C
    return (C.c_int * len(roles))(*[int(r) for r in roles])


def _gan_group(what, xs, roles, others):
    """One launch reads ``xs[0].numel()`` elements of every problem: the sizes must agree, with one role and one slot per problem."""
    if len(roles) != len(xs) or len(others) != len(xs) or any(x.numel() != xs[0].numel() for x in xs):
        raise ValueError(f"{what}: {len(xs)} logit vectors of sizes {[x.numel() for x in xs]}, {len(roles)} roles, {len(others)} scalars")


def gan_loss_fwd_g(xs, kind, roles, real_label, outs):
    _check_dev(*xs, *outs)
    _gan_group("gan_loss_fwd_g", xs, roles, outs)
    xs = [x.contiguous() for x in xs]
    _lib.check(_lib.load().dg_gan_loss_fwd_g(len(xs), _tab(xs), xs[0].numel(), int(kind), _roles(roles), float(real_label), _tab(outs), _stream()),
               "dg_gan_loss_fwd_g")
    return xs


def gan_loss_bwd_g(xs, kind, roles, real_label, gouts):
    _check_dev(*xs, *gouts)
    _gan_group("gan_loss_bwd_g", xs, roles, gouts)
    dxs =[torch.empty_like(x) for x in xs]
    _lib.check(_lib.load().dg_gan_loss_bwd_g(len(xs), _tab(xs), xs[0].numel(), int(kind), _roles(roles), float(real_label), _tab(gouts), _tab(dxs),
                                             _stream()), "dg_gan_loss_bwd_g")
    return dxs


def fm_fwd_g(reals, fakes, outs):
    g = len(reals)
    _check_dev(*reals, *fakes)
    pairs = [same_layout_pair(r, f) for r, f in zip(reals, fakes)]
    reals, fakes = [p[0] for p in pairs], [p[1] for p in pairs]
    n = reals[0].shape[0]
    j = reals[0].numel() // n
    diffs = [torch.empty(j, device=reals[0].device, dtype=torch.float32) for _ in range(g)]
    L = _lib.load()
    wsl, wsb = _ws_g(L.dg_fm_workspace_bytes(n, j), g, reals[0].device)
    _lib.check(L.dg_fm_fwd_g(g, _tab(reals), _tab(fakes), n, j, _tab(diffs), _tab(outs), _tab(wsl), wsb, _stream()), "dg_fm_fwd_g")
    return diffs, reals, fakes


def fm_bwd_g(diffs, like_reals, like_fakes, gouts, need_real, need_fake):
    n = like_fakes[0].shape[0]
    j = diffs[0].numel()
    dreals = [_dense_like(t) for t in like_reals] if need_real else None
    dfakes = [_dense_like(t) for t in like_fakes] if need_fake else None
    _lib.check(_lib.load().dg_fm_bwd_g(len(diffs), _tab(diffs), n, j, _tab(gouts), _tab(dreals), _tab(dfakes), _stream()), "dg_fm_bwd_g")
    return dreals, dfakes


# ---- module attributes ops.SHADOW / ops.ACT16 / ops.X3: views of the CURRENT context (kept for op-level tests and tools, which set
# them around single calls; a trainer carries its own Context and never touches them) -----------------------------------------------
import sys as _sys
import types as _types


class _OpsModule(_types.ModuleType):
    @property
    def SHADOW(self):
        return _CUR.shadow

    @SHADOW.setter
    def SHADOW(self, v):
        _CUR.shadow = bool(v)

    @property
    def ACT16(self):
        return _CUR.act16

    @ACT16.setter
    def ACT16(self, v):
        _CUR.act16 = bool(v)

    @property
    def _PLANE_TAB(self):           # (the current context's tables, under their pre-round-4 names: op tests look into them)
        return _CUR.plane_tab

    @property
    def _SHADOW_TAB(self):
        return _CUR.shadow_tab

    @property
    def X3(self):
        return _CUR.x3

    @X3.setter
    def X3(self, v):
        _CUR.x3 = bool(v)


_sys.modules[__name__].__class__ = _OpsModule
