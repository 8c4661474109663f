"""Adam over ONE flat fp32 buffer per parameter group (optim.Adam, image_translation.py:272-287).

All parameters handed to ``Adam`` are moved (keeping each one's memory layout) into a single flat
buffer; ``.grad`` of every parameter is a view of a matching flat gradient buffer.  One optimiser step
is then two kernel launches (scalar advance + multi-tensor update), and data parallelism all-reduces
the flat gradient buffer as one message.  Step count and bias corrections live on the device so a
step can be captured in a hipGraph.
"""
from __future__ import annotations

import torch

from . import ops

_ALIGN = 64  # floats (256 B)


def _padded(n):
    return (n + _ALIGN - 1) // _ALIGN * _ALIGN


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def x3_conv_images(entries):
    """The conv weights of a flat group that get transposed planes, as (offset, K, J = 16 C) images.
    entries = [(element offset, shape, is KRSC-strided), ...] in the group's order."""
    return [(off, int(shape[0]), 16 * int(shape[1])) for off, shape, krsc in entries
            if len(shape) == 4 and tuple(shape[2:]) == (4, 4) and shape[0] > 1 and shape[1] > 0 and krsc]


def x3_group_partition(entries):
    """How a step of the whole group (ops.adam_step_group_x3) takes the parameters ``entries`` (as x3_conv_images): (tiled, rest,
    transposed_rest).  tiled: the conv images that are whole tiles (K and J multiples of 64, offset a multiple of 8), stepped by tiles
    with their transposed planes; rest: [begin, end) ranges of every other parameter with the padding behind it, merged when adjacent,
    none of them empty; transposed_rest: the conv images among the ranges, which keep the transpose pass.  Moves no tensor."""
    convs = x3_conv_images(entries)
    tiled = [c for c in convs if c[1] % 64 == 0 and c[2] % 64 == 0 and c[0] % 8 == 0]
    tiled_offs = {c[0] for c in tiled}
    rest = []
    for off, shape, _ in entries:
        n = _numel(shape)
        if n == 0 or off in tiled_offs:      # (a parameter of no elements shares its offset with its successor and covers nothing)
            continue
        end = off + _padded(n)
        if rest and rest[-1][1] == off:
            rest[-1][1] = end
        else:
            rest.append([off, end])
    return tiled, rest, [c for c in convs if c[0] not in tiled_offs]


class Adam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("discogan_modernized_amd.optim.Adam needs parameters on a HIP device (no CPU fallback)")
        self.defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.param_groups = [dict(params=self.params, **self.defaults)]
        offs, total = [], 0
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise RuntimeError("all parameters must be fp32 on one device")
            offs.append(total)
            total += _padded(p.numel())
        self.numel = total
        self.flat_p = torch.zeros(total, device=dev)
        self.flat_g = torch.zeros(total, device=dev)
        self.exp_avg = torch.zeros(total, device=dev)
        self.exp_avg_sq = torch.zeros(total, device=dev)
        self.state = torch.zeros(4, device=dev, dtype=torch.float64)
        self.offsets = offs
        self.ctl = None                                  # enable_grad_control()
        self._unwritten = False                          # zero_grad(lazy=True): some parameter's gradient may still await its first writer
        with torch.no_grad():
            for p, off in zip(self.params, offs):
                n = p.numel()
                view = self.flat_p[off:off + n].as_strided(p.shape, p.stride())
                view.copy_(p.data)
                p.data = view
                gview = self.flat_g[off:off + n].as_strided(p.shape, p.stride())
                p._dg_flat_grad = gview
                p.grad = gview

    def enable_bf16_shadow(self):
        """Keep a bf16 (RNE) shadow of every parameter for the bf16 matrix path: one flat bf16 buffer, refreshed by the
        Adam kernel itself (+2 B/param), exposed as ``param._dg_bf16`` views with the parameter's own memory layout."""
        if getattr(self, "flat_p16", None) is not None:
            return
        self.flat_p16 = torch.empty(self.numel, device=self.flat_p.device, dtype=torch.bfloat16)
        ops.f32_to_bf16(self.flat_p, self.flat_p16)
        for p, off in zip(self.params, self.offsets):
            p._dg_bf16 = self.flat_p16[off:off + p.numel()].as_strided(p.shape, p.stride())
            p._dg_bf16_ver = p._version

    def enable_x3_planes(self):
        """Keep the three bf16 planes (hi / mid / lo, ops.f32_to_bf16x3) of every parameter for the f32x3 matrix path: one
        flat [3, numel] bf16 buffer refreshed by the Adam kernel itself (+6 B/param), exposed as ``param._dg_x3`` =
        (buffer, element offset)."""
        if getattr(self, "flat_p3", None) is not None:
            return
        self.flat_p3 = torch.empty((3, self.numel), device=self.flat_p.device, dtype=torch.bfloat16)
        ops.f32_to_bf16x3(self.flat_p, self.flat_p3)
        # the forward form of the plane kernel wants the conv weights' planes TRANSPOSED ([(r, s, c)][k]): a second buffer,
        # same flat offsets, rewritten with every Adam step: by the step's own kernel when the whole group is stepped (below),
        # else for all conv weights of the group by one launch behind it
        entries = [(off, tuple(p.shape), p.dim() == 4 and ops.is_krsc(p)) for p, off in zip(self.params, self.offsets)]
        convs = x3_conv_images(entries)
        self.flat_p3t = torch.zeros((3, self.numel), device=self.flat_p.device, dtype=torch.bfloat16) if convs else None
        self._x3t_table = ops.x3_transpose_table(convs)
        # a step of the WHOLE group writes the transposed planes itself (ops.adam_step_group_x3): the conv weights that are whole
        # tiles (K and J multiples of 64) by tiles, every other parameter (with the padding behind it) as ranges, merged when adjacent, in one launch;
        # conv weights among the ranges keep the transpose pass, over a table of just those
        tiled, rest, transposed_rest = x3_group_partition(entries)
        self._adam_group_table = ops.adam_group_x3_table(tiled, rest)
        self._x3t_rest_table = ops.x3_transpose_table(transposed_rest)
        conv_offs = {c[0] for c in convs}
        for p, off in zip(self.params, self.offsets):
            p._dg_x3 = (self.flat_p3, off, self.flat_p3t if off in conv_offs else None)
            p._dg_x3_ver = p._version
        if convs:
            ops.x3_transpose_planes(self.flat_p3, self.flat_p3t, self._x3t_table)

    def enable_grad_control(self, max_norm=0.0, guard=False):
        """Measure the global norm of the stepped gradient in every ``step``, clip by it (``max_norm`` > 0, the rule of
        ``torch.nn.utils.clip_grad_norm_``) and / or skip a step whose gradient holds an inf or a NaN (``guard``).  Allocates the
        device control block ``ctl`` (8 x float64, layout in include/discogan_hip.h: sumsq, norm, scale, skip, steps seen / clipped /
        skipped, largest finite norm) and the workspace of the partial sums.  Nothing waits for the host: the Adam kernels read
        their scale and their go / no-go from ``ctl``."""
        max_norm = float(max_norm)
        if not max_norm >= 0.0:
            raise ValueError(f"max_norm must be >= 0 (0 = no clipping), got {max_norm}")
        self.max_norm, self.guard = max_norm, bool(guard)
        if self.ctl is None:
            self.ctl = torch.zeros(8, device=self.flat_p.device, dtype=torch.float64)
            self._stats_ws = ops.grad_stats_workspace(self.flat_p.device)

    def grad_stats(self):
        """The control block on the host (waits for the current stream): dict(sumsq, norm, scale, skip, steps, clipped, skipped, max_norm)."""
        if self.ctl is None:
            raise RuntimeError("grad_stats(): gradient control is off (enable_grad_control)")
        c = self.ctl.cpu().tolist()
        return dict(sumsq=c[0], norm=c[1], scale=c[2], skip=bool(c[3]), steps=int(c[4]), clipped=int(c[5]), skipped=int(c[6]),
                    max_norm=c[7])

    def refresh_derived(self):
        """Recompute everything derived from ``flat_p`` (bf16 shadow, f32x3 plane triples and their transposed copy) after the
        flat buffer was written from outside the optimiser -- e.g. ``ExchangeGroup.broadcast_(opt.flat_p)``; writes through the
        parameters themselves (``load_state_dict``) are noticed per weight by their version counters."""
        if getattr(self, "flat_p16", None) is not None:
            ops.f32_to_bf16(self.flat_p, self.flat_p16)
        if getattr(self, "flat_p3", None) is not None:
            ops.f32_to_bf16x3(self.flat_p, self.flat_p3)
            if self.flat_p3t is not None:
                ops.x3_transpose_planes(self.flat_p3, self.flat_p3t, self._x3t_table)

    # -- torch.optim.Optimizer surface used by the reference loop ------------------------------------
    def zero_grad(self, set_to_none: bool = True, lazy: bool = False):
        """``lazy`` (the trainer's own step; ops.LAZY_ZERO_GRAD): fill nothing, mark every parameter "not yet written" instead.  The
        first backward kernel that writes a marked parameter's gradient (functional._flat_grad_of) OVERWRITES it and clears the mark;
        what is still marked when the flat gradient is read (``step``, an exchange: ``fill_unwritten_grads``) is zero-filled then.
        Until then ``p.grad`` of a marked parameter holds the last iteration's values: only for backward passes made of this
        package's Functions (a torch-native AccumulateGrad would add to them).  The marks are host state that moves the same way
        under hipGraph capture and in eager dispatch."""
        if lazy and ops.LAZY_ZERO_GRAD:
            self._unwritten = True
        else:
            self.flat_g.zero_()
            self._unwritten = False
        for p in self.params:
            p._dg_grad_unwritten = self._unwritten
            if p.grad is not p._dg_flat_grad:
                p.grad = p._dg_flat_grad

    def fill_unwritten_grads(self, ranges=None):
        """Zero-fill the gradient of every parameter (inside the flat ``ranges``; None = the group) that no backward kernel has written
        since ``zero_grad(lazy=True)``, on the current stream, neighbours in one fill: whoever reads the flat gradient calls this first."""
        if not self._unwritten:
            return
        runs = []
        for p, off, end in self.extents():
            if not getattr(p, "_dg_grad_unwritten", False):
                continue
            if ranges is not None and not any(b <= off and end <= e for b, e in ranges):
                continue
            p._dg_grad_unwritten = False
            if runs and runs[-1][1] == off:
                runs[-1][1] = end
            else:
                runs.append([off, end])
        for b, e in runs:
            self.flat_g[b:e].zero_()
        if ranges is None:
            self._unwritten = False

    def _sync_foreign_grads(self):
        # a caller may have replaced .grad (e.g. zero_grad(set_to_none=True) on a plain nn.Module)
        for p in self.params:
            if p.grad is None:
                p._dg_flat_grad.zero_()
                p.grad = p._dg_flat_grad
                p._dg_grad_unwritten = False
            elif p.grad is not p._dg_flat_grad and p.grad.data_ptr() != p._dg_flat_grad.data_ptr():
                p._dg_flat_grad.copy_(p.grad)
                p.grad = p._dg_flat_grad
                p._dg_grad_unwritten = False

    def extents(self):
        """(parameter, begin, end) of every parameter in the flat buffers, the padding behind it included."""
        for p, off in zip(self.params, self.offsets):
            yield p, off, off + _padded(p.numel())

    def ranges_of(self, modules):
        """Flat [begin, end) ranges covering the parameters of the given modules (merged when adjacent)."""
        ids = {id(p) for m in modules for p in m.parameters()}
        out = []
        for p, off, end in self.extents():
            if id(p) in ids:
                if out and out[-1][1] == off:
                    out[-1][1] = end
                else:
                    out.append([off, end])
        return [tuple(r) for r in out]

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, active=None):
        """``active``: flat ranges that received gradients this iteration (from ``ranges_of``).  Like
        torch.optim.Adam, parameters whose ``.grad`` would be None (a network outside the loss of the
        ``recongan`` / ``gan`` architectures, image_translation.py:377-382) are left untouched: no weight
        decay, no moment update.  None = the whole group."""
        self._sync_foreign_grads()
        self.fill_unwritten_grads()
        ranges = active if active is not None else [(0, self.numel)]
        ctl = self.ctl
        if ctl is not None:
            # with gradient control (enable_grad_control): the norm over the active ranges (the padding between parameters is zero),
            # one finalize into ctl, then the guarded advance and the guarded, device-scaled update -- all on this stream.
            # ``grad_scale`` enters the norm, so that it is the norm of the gradient the update sees (data parallel: the average).
            slots = 0
            for b, e in ranges:
                slots += ops.grad_sumsq_partial(self.flat_g[b:e], self._stats_ws, slots)
            ops.grad_clip_finalize(self._stats_ws, slots, float(grad_scale), self.max_norm, self.guard, ctl)
        self._advance(ctl)
        p3 = getattr(self, "flat_p3", None)
        if p3 is not None and active is None and ops.ADAM_FUSED_T:
            # the whole group on the f32x3 planes: one pass that also leaves the transposed weight planes (no transpose pass behind it)
            g = self.param_groups[0]
            ops.adam_step_group_x3(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.state, float(g["betas"][0]),
                                   float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), float(grad_scale), p3,
                                   self.flat_p3t, self._adam_group_table, ctl=ctl)
            if self._x3t_rest_table[0]:
                ops.x3_transpose_planes(p3, self.flat_p3t, self._x3t_rest_table)
            return
        self.step_ranges(ranges, grad_scale, ctl)
        self.finish_step()

    def _advance(self, ctl):
        g = self.param_groups[0]
        ops.adam_advance(self.state, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), ctl=ctl)

    # A step issued in slices (an exchange that overlaps the backward pass): begin_step(), step_ranges() per slice as its gradients
    # arrive, in any order and on any stream ordered behind begin_step(), then finish_step() behind every slice.
    @torch.no_grad()
    def begin_step(self):
        """Advance the step count and the bias corrections once, ahead of the slices.  Not under gradient control: the global norm
        needs the whole gradient before the first slice is stepped."""
        if self.ctl is not None:
            raise RuntimeError("begin_step(): a step issued in slices cannot be norm-controlled (enable_grad_control is on); use step()")
        self._sync_foreign_grads()
        self._advance(None)

    @torch.no_grad()
    def step_ranges(self, ranges, grad_scale: float = 1.0, ctl=None):
        """The update of the flat ``ranges`` [(begin, end), ...] with every derived form the group keeps (bf16 shadow, f32x3 planes):
        one launch per range.  Fills no unwritten gradient: whoever exchanges the gradients does that first (fill_unwritten_grads)."""
        g = self.param_groups[0]
        b1, b2, eps, wd = float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"])
        p16 = getattr(self, "flat_p16", None)
        p3 = getattr(self, "flat_p3", None)
        for b, e in ranges:
            ops.adam_step_flat(self.flat_p[b:e], self.flat_g[b:e], self.exp_avg[b:e], self.exp_avg_sq[b:e], self.state, b1, b2, eps, wd,
                               float(grad_scale), p16=None if p16 is None else p16[b:e],
                               p3=None if p3 is None else (p3.data_ptr() + 2 * b, self.numel), ctl=ctl)

    @torch.no_grad()
    def finish_step(self):
        """Behind every slice of the step: the transposed copy of the conv weights' planes, where the group keeps one."""
        if getattr(self, "flat_p3t", None) is not None:
            ops.x3_transpose_planes(self.flat_p3, self.flat_p3t, self._x3t_table)

    def state_dict(self):
        sd = dict(step=self.state[0:1].clone(), exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(),
                  param_groups=[{k: v for k, v in self.param_groups[0].items() if k != "params"}])
        if self.ctl is not None:                         # steps seen / clipped / skipped, largest finite norm
            sd["grad_control"] = self.ctl[4:8].clone()
        return sd

    def load_state_dict(self, sd):
        self.state.zero_()
        self.state[0:1].copy_(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        if self.ctl is not None:                         # (a state written without gradient control: the counters start at zero)
            self.ctl.zero_()
            if "grad_control" in sd:
                self.ctl[4:8].copy_(sd["grad_control"])
        for k, v in sd["param_groups"][0].items():
            self.param_groups[0][k] = v


class EMA:
    """Exponential moving average of an ``Adam`` group's parameters: ``flat`` has the length and offsets of ``opt.flat_p``
    (+4 B/param), one kernel launch per update (12 B/param of HBM traffic).

    ``update()`` -- the first call COPIES the weights (``ready``), later ones run ``flat += (flat_p - flat) * (1 - decay)``.
    ``swap()``   -- exchanges ``flat`` and ``opt.flat_p`` in place and rebuilds what the optimiser derives from its flat buffer
                    (bf16 shadow, f32x3 planes): the networks then compute with the averaged weights; a second call undoes it."""

    def __init__(self, opt, decay):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError(f"EMA decay must be in (0, 1), got {decay}")
        self.opt = opt
        self.decay = decay
        self.flat = torch.zeros_like(opt.flat_p)
        self.updates = 0
        self.ready = False

    @torch.no_grad()
    def update(self):
        if not self.ready:
            self.flat.copy_(self.opt.flat_p)        # a copy, not the kernel with w = 1, whose e + (p - e) may round
            self.ready = True
            return
        ops.ema_update_flat(self.flat, self.opt.flat_p, float(1.0 - self.decay))
        self.updates += 1

    @torch.no_grad()
    def swap(self):
        ops.swap_flat(self.flat, self.opt.flat_p)
        self.opt.refresh_derived()

    def view_of(self, param):
        """The EMA of one parameter, with the parameter's own shape and strides (conv weights are KRSC-strided)."""
        for p, off in zip(self.opt.params, self.opt.offsets):
            if p is param:
                return self.flat[off:off + p.numel()].as_strided(p.shape, p.stride())
        raise KeyError("not a parameter of this EMA's optimiser")

    def state_dict(self):
        return dict(flat=self.flat.clone(), updates=int(self.updates), ready=bool(self.ready), decay=float(self.decay))

    def load_state_dict(self, sd):
        self.flat.copy_(sd["flat"])
        self.updates = int(sd["updates"])
        self.ready = bool(sd["ready"])
        self.decay = float(sd["decay"])
