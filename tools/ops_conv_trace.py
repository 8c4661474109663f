"""Call trace of the interior-conv op wrappers: what ops.conv_fwd / conv_dgrad / conv_wgrad and their grouped forms ask the library
for, point by point over a matrix of geometries, contexts and operand forms.  Two versions of the package that give the same trace
launch the same kernels on the same operands with the same scalars, so the trace of one commit is the reference for a refactor of
the next (tests/golden/ops_conv_calls.json holds its digests; tests/test_ops_conv_calls_gpu.py replays it).

Only the public wrappers are driven.  Every entry point of the loaded library object is wrapped for the duration of a trace point
(the way tests/gpu_util.conv_requests wraps nine of them), and a point records
  calls   the launches in order, "name(arg, ...)": scalars as they are, pointers by the name of what they point to -- x, w, dy,
          x.shadow, w.planes+off, w.planes_t+off, out, stat, ws, new<i> (a buffer the wrapper allocated and kept to itself), None;
          a pointer table as [..]; the stream as "st"
  q       the host queries that were made, each with its answer (a set: order and repeats do not count)
  ret     dtype and shape of what the wrapper returned (and of the statistics rows, or None)
  tabs    keys added to (+) or removed from (-) the context's shadow_tab / plane_tab
  exc     type and message, if the wrapper raised (a library refusal included: nothing is retried)

The matrix: every geometry of tests/test_plan_cases_cpu.PLAN_CASES (with the case's library options) and the two 4 x 4 head geometries
of tests/test_conv_forms_gpu.GEOMS for all three ops, crossed with want_stats False / True / "split" (op 2: a fresh result and an
accumulating one) and with SCENARIOS below; then groups of 2 and 4 through the *_g wrappers under both group plans; then the
predictors (ops._x3_ok, x3_all_plane_readers, x3_window_dgrad, model._first_layer_planes), which make host queries only.

  python -m tools.ops_conv_trace --out trace.json            # on the GPU: every launch really runs
  python -m tools.ops_conv_trace --dry --out trace.json      # no GPU: CPU tensors, launches recorded and not made
  python -m tools.ops_conv_trace --diff a.json b.json        # number of differing records, the first few shown
  python -m tools.ops_conv_trace --digest golden.json        # the short form that is committed (see digest)
"""
import argparse
import json
import sys
import time

import torch

from discogan_modernized_amd import _lib, model, ops
from tests.test_conv_forms_gpu import GEOMS
from tests.test_plan_cases_cpu import PLAN_CASES

F32, BF16, F32X3 = ops.PREC_F32, ops.PREC_BF16, ops.PREC_F32X3
QUERIES = ("dg_conv_workspace_bytes_p", "dg_conv_bnstats_rows_p", "dg_conv_plan_splits_p", "dg_conv_x3_planes_ok", "dg_conv_x3_bnstats_rows",
           "dg_conv_mixed_bnstats_rows", "dg_conv_bf16_operands_ok", "dg_conv_workspace_bytes", "dg_conv_plan_splits", "dg_conv_bnstats_rows")
SILENT = ("dg_last_error", "dg_set_option", "dg_version", "dg_build_flags", "dg_device_cu_count")
W_OFF = 64                      # element offset of the weight inside its flat plane buffer (a weight of a flat Adam group)

# name: (context arguments, module switches flipped, form of the first feature-map operand, of the weight, of the second feature-map
# operand of op 2).  Feature-map forms: f32 | sh (fp32 with a bf16 shadow) | b16 (a bf16 tensor) | pl (fp32 with a pixel-major plane
# entry) | cm (chunk-major entry) | po+pl (plane-only tensor with its entry) | po (plane-only, entry gone).  Weight forms: f32 | sh |
# flat (planes in a flat buffer) | flat_t (and the transposed copy).
SCENARIOS = {
    "f32": (dict(prec=F32), {}, "f32", "f32", "f32"),
    "f32/b16-in": (dict(prec=F32), {}, "b16", "f32", "b16"),
    "bf16s": (dict(prec=BF16, shadow=True), {}, "f32", "f32", "f32"),
    "bf16s/sh-all": (dict(prec=BF16, shadow=True), {}, "sh", "sh", "sh"),
    "bf16s/sh-a": (dict(prec=BF16, shadow=True), {}, "sh", "f32", "f32"),
    "bf16s/sh-b": (dict(prec=BF16, shadow=True), {}, "f32", "sh", "sh"),
    "act16": (dict(prec=BF16, shadow=True, act16=True), {}, "b16", "f32", "b16"),
    "act16/sh-w": (dict(prec=BF16, shadow=True, act16=True), {}, "b16", "sh", "b16"),
    "act16/f32-in": (dict(prec=BF16, shadow=True, act16=True), {}, "f32", "sh", "f32"),
    "x3": (dict(prec=F32X3, x3=True), {}, "f32", "f32", "f32"),
    "x3/pl-t": (dict(prec=F32X3, x3=True), {}, "pl", "flat_t", "pl"),
    "x3/pl": (dict(prec=F32X3, x3=True), {}, "pl", "flat", "pl"),
    "x3/cm": (dict(prec=F32X3, x3=True), {}, "cm", "flat_t", "pl"),
    "x3/cm-b": (dict(prec=F32X3, x3=True), {}, "pl", "flat_t", "cm"),
    "x3/po+pl": (dict(prec=F32X3, x3=True), {}, "po+pl", "flat_t", "po+pl"),
    "x3/po": (dict(prec=F32X3, x3=True), {}, "po", "flat_t", "pl"),
    "x3rsp/pl-t": (dict(prec=F32X3, x3=True), {"X3_RSP": True}, "pl", "flat_t", "pl"),
    "x3fww/pl-t": (dict(prec=F32X3, x3=True), {"X3_FWW": True}, "pl", "flat_t", "pl"),
    # plane codes 3 and 4 are answers of the experiments library only: forced here (FORCED_CODE), so that the rule for them is traced
    "x3+c3/pl-t": (dict(prec=F32X3, x3=True), {}, "pl", "flat_t", "pl"),
    "x3rsp+c3/pl-t": (dict(prec=F32X3, x3=True), {"X3_RSP": True}, "pl", "flat_t", "pl"),
    "x3rsp+c3/po+pl": (dict(prec=F32X3, x3=True), {"X3_RSP": True}, "po+pl", "flat", "po+pl"),
    "x3rsp+c4/pl-t": (dict(prec=F32X3, x3=True), {"X3_RSP": True}, "pl", "flat_t", "pl"),
    "x3rsp+c4/f32": (dict(prec=F32X3, x3=True), {"X3_RSP": True}, "f32", "f32", "f32"),
    "x3fww+c3/pl-t": (dict(prec=F32X3, x3=True), {"X3_FWW": True}, "pl", "flat_t", "pl"),
    "x3fww+c3/pl": (dict(prec=F32X3, x3=True), {"X3_FWW": True}, "pl", "flat", "pl"),
    "x3fww+c3/po+pl": (dict(prec=F32X3, x3=True), {"X3_FWW": True}, "po+pl", "flat", "po+pl"),
    "x3fww+c3/f32": (dict(prec=F32X3, x3=True), {"X3_FWW": True}, "f32", "f32", "f32"),
    "x3fww+c4/pl-t": (dict(prec=F32X3, x3=True), {"X3_FWW": True}, "pl", "flat_t", "pl"),
    "x3fww+rsp+c3/pl": (dict(prec=F32X3, x3=True), {"X3_FWW": True, "X3_RSP": True}, "pl", "flat", "pl"),
}
GROUP_CONTEXTS = {"f32": dict(prec=F32), "x3reg": dict(prec=F32X3)}
PREDICTOR_CONTEXTS = {"f32": dict(prec=F32), "bf16s": dict(prec=BF16, shadow=True), "act16": dict(prec=BF16, shadow=True, act16=True),
                      "x3": dict(prec=F32X3, x3=True)}
FORCED_CODE = {"+c3": 3, "+c4": 4}          # scenario name part -> the answer dg_conv_x3_planes_ok is made to give
PREDICTOR_SWITCHES = ({}, {"X3_RSP": True}, {"X3_FWW": True}, {"X3_CM": False}, {"X3_PLANES_ONLY": False})


def geometries():
    """(op, N, H, W, C, K, stride, pad), library options: the distinct ones of PLAN_CASES, then the head geometries for every op."""
    out = {}
    for req, opts, _ in PLAN_CASES:
        out.setdefault((req[:8], tuple(sorted(opts.items()))), (req[:8], dict(opts)))
    for N, H, C, K, stride, pad in GEOMS[1:]:
        for op in range(3):
            g = (op, N, H, H, C, K, stride, pad)
            out.setdefault((g, ()), (g, {}))
    return list(out.values())


def geom_id(g, opts):
    return "op{}-n{}-{}x{}-c{}-k{}-s{}-p{}".format(*g) + "".join(f"-{k}{v}" for k, v in sorted(opts.items()))


class _FakeDevice(torch.Tensor):
    """--dry: a CPU tensor that passes the wrappers' device check."""
    is_cuda = property(lambda self: True)


class switches:
    """Module attributes of ops for a block."""

    def __init__(self, kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: getattr(ops, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(ops, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(ops, k, v)
        return False


class library_options:
    def __init__(self, kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            _lib.set_option(k, 0)
        return False


class Recorder:
    """Wraps every entry point of the loaded library object; ``dry`` answers every launch with 0 without making it."""

    def __init__(self, dry):
        self.dry = dry
        self.raw, self.queries, self.force = [], set(), None

    def __enter__(self):
        L = _lib.load()
        self.saved = {}
        for name in _lib.SIGNATURES:
            if name in SILENT:
                continue
            fn = getattr(L, name)
            self.saved[name] = fn
            setattr(L, name, self._wrap(name, fn))
        # a split that ops.planes_of makes for one reader and does not keep is freed on return, and the allocator may hand its block
        # to the output allocated next; the trace names buffers by address, so such splits are held until the point is recorded
        self.split, self.held = ops.f32_to_bf16x3, []
        ops.f32_to_bf16x3 = lambda x, out3: (self.held.append(out3), self.split(x, out3))[1]
        return self

    def _wrap(self, name, fn):
        if name in QUERIES:
            def query(*a):
                r = fn(*a)
                if name == "dg_conv_x3_planes_ok" and self.force is not None:
                    r = self.force
                self.queries.add(f"{name}({','.join(str(int(v)) for v in a)})={int(r)}")
                return r
            return query

        def launch(*a):
            self.raw.append((name, a))
            return 0 if self.dry else fn(*a)
        return launch

    def __exit__(self, *exc):
        L = _lib.load()
        for name, fn in self.saved.items():
            setattr(L, name, fn)
        ops.f32_to_bf16x3 = self.split
        return False

    def reset(self):
        self.raw, self.queries, self.held = [], set(), []


class Names:
    """Pointer -> name: the registered tensors by address (an address inside one: name+element offset of 2-byte units for plane
    buffers, bytes otherwise); what is left is the workspace where it stands in the workspace argument, else new<i>."""

    def __init__(self):
        self.known, self.fresh = [], []

    def add(self, name, t, unit=1):
        if t is not None:
            self.known.append((name, t.data_ptr(), t.numel() * t.element_size(), unit))

    def of(self, p, is_ws=False):
        if p is None or p == 0:
            return "None"
        for name, base, nbytes, unit in self.known:
            if p == base:
                return name
        for name, base, nbytes, unit in self.known:
            if base < p < base + nbytes:
                return f"{name}+{(p - base) // unit}"
        if is_ws:
            self.known.append(("ws", p, 1 << 40, 1))              # the slices of a grouped workspace follow their first one
            return "ws"
        if p not in self.fresh:
            self.fresh.append(p)
        return f"new{self.fresh.index(p)}"


def render_call(name, args, names):
    sig = _lib.SIGNATURES[name][1]
    out = []
    for i, (a, ty) in enumerate(zip(args, sig)):
        if ty is not _lib._p:
            out.append(repr(round(a, 6)) if isinstance(a, float) else str(int(a)))
        elif i == len(sig) - 1:
            out.append("st")
        else:
            is_ws = i == len(sig) - 3 and sig[i + 1] is _lib._z
            if a is None or isinstance(a, int):
                out.append(names.of(a, is_ws))
            elif hasattr(a, "_length_"):                          # a pointer table (ops._tab) or a ctypes array of scalars
                vals = list(a)
                if a._type_ is _lib._p:
                    out.append("[" + ",".join(names.of(v, is_ws) for v in vals) + "]")
                else:
                    out.append("[" + ",".join(str(v) for v in vals) + "]")
            else:
                out.append(names.of(getattr(a, "value", None), is_ws))
    return f"{name}({','.join(out)})"


def describe_tensor(t):
    if t is None:
        return "None"
    if isinstance(t, (list, tuple)):
        return "(" + ",".join(describe_tensor(v) for v in t) + ")"
    return f"{str(t.dtype).replace('torch.', '')}{list(t.shape)}"


class Bench:
    """The device buffers of one geometry (allocated once, zero-filled) and the per-point operands made of them."""

    def __init__(self, g, dev, dry, groups=1):
        op, N, H, W, C, K, stride, pad = g
        Ho, Wo = ((H + 2 * pad - 4) // stride + 1, (W + 2 * pad - 4) // stride + 1)
        self.g, self.dry = g, dry
        self.shape = {"x": (N, C, H, W), "dy": (N, K, Ho, Wo), "w": (K, C, 4, 4)}
        self.base = {}
        for role, (a, b, c, d) in self.shape.items():
            for kind, dtype in (("f32", torch.float32), ("b16", torch.bfloat16)):
                self.base[role, kind] = [torch.zeros((a, c, d, b), device=dev, dtype=dtype).permute(0, 3, 1, 2) for _ in range(groups)]
            numel = a * b * c * d
            extra = W_OFF if role == "w" else 0
            self.base[role, "pl"] = torch.zeros((3, numel + extra), device=dev, dtype=torch.bfloat16)
        self.base["w", "pl_t"] = torch.zeros_like(self.base["w", "pl"])
        self.base["w", "out"] = torch.zeros((K, 4, 4, C), device=dev, dtype=torch.float32).permute(0, 3, 1, 2)

    def fresh(self, role, kind="f32", i=0):
        """A new tensor object (no attributes) over the geometry's buffer."""
        t = self.base[role, kind][i]
        t = t[:]
        return t.as_subclass(_FakeDevice) if self.dry else t

    def fmap(self, role, form, names):
        """A feature-map operand in ``form`` (inside the context it will be used under), or (None, why) where the form cannot be made."""
        n, c, h, w = self.shape[role]
        if form == "b16":
            t = self.fresh(role, "b16")
            names.add(role, t)
            return t
        t = self.fresh(role)
        names.add(role, t)
        if form == "sh":
            t16 = self.base[role, "b16"][0]
            ops.shadow_put(t, t16)
            names.add(role + ".shadow", t16)
        if form in ("pl", "cm", "po+pl"):
            if form == "cm" and not (c % 64 == 0 and (n * h * w) % 4 == 0):       # (what ops._bn_out asks of a chunk-major triple)
                return None
            ops.planes_put(t, self.base[role, "pl"], cm=form == "cm")
            names.add(role + ".planes", self.base[role, "pl"], 2)
        if form in ("po", "po+pl"):
            t._dg_planes_only = True
        return t

    def weight(self, form, names):
        w = self.fresh("w")
        names.add("w", w)
        if form == "sh":
            w._dg_bf16, w._dg_bf16_ver = self.base["w", "b16"][0], w._version
            names.add("w.shadow", w._dg_bf16)
        if form in ("flat", "flat_t"):
            w._dg_x3 = (self.base["w", "pl"], W_OFF, self.base["w", "pl_t"] if form == "flat_t" else None)
            w._dg_x3_ver = w._version
            names.add("w.planes", self.base["w", "pl"], 2)
            names.add("w.planes_t", self.base["w", "pl_t"], 2)
        return w


def finish(rec, names, ctx, before, result, exc, own=(), geom=None):
    """The record of one trace point.  To keep the file small the point's own "N,H,W,C,K,stride,pad" inside a call or a query is
    written "@" (the point's key names the geometry) and the "dg_conv_" / "dg_" of the entry points is dropped."""
    short = lambda s: s.replace(",".join(str(v) for v in geom), "@").replace("dg_conv_", "", 1).replace("dg_", "", 1)
    for name, t in own:
        names.add(name, t)
    if isinstance(result, tuple):
        names.add("out", result[0])
        names.add("stat", result[1])
    elif isinstance(result, list):
        for i, t in enumerate(result):
            names.add(f"out{i}", t)
    else:
        names.add("out", result)
    for role_name, base, _, _ in list(names.known):
        if role_name in ("x", "dy"):
            e = ctx.plane_tab.get(base)
            if e is not None:
                names.add(role_name + ".planes", e[1], 2)
    out = {}
    if rec.raw:
        out["calls"] = [short(render_call(n, a, names)) for n, a in rec.raw]
    if rec.queries:
        out["q"] = sorted(short(q) for q in rec.queries)
    if exc is None:
        out["ret"] = describe_tensor(result)
    else:
        out["exc"] = f"{type(exc).__name__}: {exc}"
    tabs = []
    for tab_name, tab in (("shadow", ctx.shadow_tab), ("plane", ctx.plane_tab)):
        now = set(tab)
        tabs += [f"+{tab_name}:{names.of(k)}" for k in sorted(now - before[tab_name], key=names.of)]
        tabs += [f"-{tab_name}:{names.of(k)}" for k in sorted(before[tab_name] - now, key=names.of)]
    if tabs:
        out["tabs"] = tabs
    return out


def trace_single(bench, scenario, stats_or_acc, rec):
    op, N, H, W, C, K, stride, pad = bench.g
    ckw, sw, a_form, w_form, b_form = SCENARIOS[scenario]
    ctx = ops.Context(**ckw)
    names = Names()
    rec.force = next((v for k, v in FORCED_CODE.items() if k in scenario), None)
    with ops.use(ctx), switches(sw):
        a = bench.fmap("x" if op == 0 else "dy", a_form, names)
        b = bench.weight(w_form, names) if op != 2 else bench.fmap("x", b_form, names)
        if a is None or b is None:
            return {"skip": "no chunk-major triple at this shape"}
        out = None
        if op == 2 and stats_or_acc:
            out = bench.base["w", "out"]
            names.add("dw", out)
        before = {"shadow": set(ctx.shadow_tab), "plane": set(ctx.plane_tab)}
        result = exc = None
        rec.reset()
        try:
            if op == 0:
                result = ops.conv_fwd(a, b, stride, pad, want_stats=stats_or_acc)
            elif op == 1:
                result = ops.conv_dgrad(a, b, (H, W), stride, pad, want_stats=stats_or_acc)
            else:
                result = ops.conv_wgrad(a, b, stride, pad, out=out, accumulate=bool(stats_or_acc))
        except Exception as e:                                    # a refusal is an outcome
            exc = e
        own = []
        if op != 2 and getattr(b, "_dg_x3", None) is not None and w_form not in ("flat", "flat_t"):
            own.append(("w.planes(own)", b._dg_x3[0]))
        if out is not None and result is out:
            result = None if exc is not None else out
        return finish(rec, names, ctx, before, result, exc, own, geom=bench.g[1:])


def trace_group(bench, cname, g, plan, rec):
    op, N, H, W, C, K, stride, pad = bench.g
    ctx = ops.Context(group_plan=plan, **GROUP_CONTEXTS[cname])
    names = Names()
    rec.force = None
    with ops.use(ctx):
        def many(role):
            ts = [bench.fresh(role, "f32", i) for i in range(g)]
            for i, t in enumerate(ts):
                names.add(f"{role}{i}", t)
            return ts
        before = {"shadow": set(), "plane": set()}
        result = exc = None
        rec.reset()
        try:
            if op == 0:
                result = ops.conv_fwd_g(many("x"), many("w"), stride, pad)
            elif op == 1:
                result = ops.conv_dgrad_g(many("dy"), many("w"), (H, W), stride, pad)
            else:
                share = 2 if g == 4 else 1                        # g = 4: a discriminator's real and fake pass share a gradient
                outs = [bench.base["w", "f32"][i // share * share] for i in range(g)]
                for i in range(0, g, share):
                    names.add(f"dw{i}", outs[i])
                result = ops.conv_wgrad_g(many("dy"), many("x"), stride, pad, outs, True, share)
        except Exception as e:
            exc = e
        return finish(rec, names, ctx, before, result, exc, geom=bench.g[1:])


def trace_predictors(g, rec):
    """Return values of the form predictors for one geometry under every context, switch and forced plane code."""
    op, N, H, W, C, K, stride, pad = g
    out = {}
    conv = _PRED_CONV
    conv.in_channels, conv.out_channels, conv.stride = C, K, stride
    image = torch.empty((N, 3, 2 * H, 2 * W), device="meta")
    for cname, ckw in PREDICTOR_CONTEXTS.items():
        for sw, force in [(sw, None) for sw in PREDICTOR_SWITCHES] + [(sw, f) for sw in PREDICTOR_SWITCHES[:3] for f in (3, 4)]:
            if force is not None and cname != "x3":
                continue
            rec.force = force
            key = cname + "".join(f"/{k}={int(v)}" for k, v in sw.items()) + (f"/code={force}" if force else "")
            with ops.use(ops.Context(**ckw)), switches(sw):
                r = {"x3_ok": [bool(ops._x3_ok(o, N, H, W, C, K, stride, pad)) for o in range(3)],
                     "readers": [bool(ops.x3_all_plane_readers(N, H, W, C, K, forward_is_dgrad=f, need_wgrad=nw))
                                 for f in (False, True) for nw in (False, True)],
                     "window": bool(ops.x3_window_dgrad(N, H, W, C, K))}
                first = []
                for x3w in (None, (None, 0, None), (None, 0, image)):         # no triple; one without, one with a transposed copy
                    for grad, req in ((True, True), (True, False), (False, True)):
                        w = conv.weight
                        w.requires_grad_(req)
                        if x3w is None:
                            if hasattr(w, "_dg_x3"):
                                del w._dg_x3
                        else:
                            w._dg_x3 = x3w
                        with torch.set_grad_enabled(grad):
                            first.append(bool(model._first_layer_planes(image, conv)))
                r["first"] = first
            bits = lambda v: "".join(str(int(b)) for b in v)
            out[key] = f"x3_ok {bits(r['x3_ok'])} readers {bits(r['readers'])} window {int(r['window'])} first {bits(r['first'])}"
    return out


_PRED_CONV = None


def setup_predictors():
    global _PRED_CONV
    with torch.random.fork_rng(devices=[]):                       # (the module's weight initialisation draws random numbers)
        _PRED_CONV = model.Conv2d(32, 32)


def predictor_id(g):
    return "n{}-{}x{}-c{}-k{}-s{}-p{}".format(*g[1:])


def run(dry, only=None, progress=False):
    dev = "cpu" if dry else "cuda"
    if dry:
        ops._stream = lambda: 0
    records, slow = {}, []
    geoms = geometries()
    setup_predictors()
    with Recorder(dry) as rec:
        for g, opts in geoms:
            gid = geom_id(g, opts)
            if only and only not in gid:
                continue
            t0 = time.time()
            records[gid] = {}
            with library_options(opts):
                bench = Bench(g, dev, dry, groups=4)
                variants = (False, True) if g[0] == 2 else (False, True, "split")
                for sname in SCENARIOS:
                    for v in variants:
                        records[gid][f"{sname}|{'acc' if g[0] == 2 else 'stats'}={v}"] = trace_single(bench, sname, v, rec)
                for cname in GROUP_CONTEXTS:
                    for n_groups in (2, 4):
                        for plan in ("launch", "single"):
                            records[gid][f"group/{cname}|g={n_groups}|{plan}"] = trace_group(bench, cname, n_groups, plan, rec)
                if not dry:
                    torch.cuda.synchronize()
                del bench
            slow.append((time.time() - t0, gid))
            if progress:
                print(f"{gid}: {slow[-1][0]:.2f} s", flush=True)
        predictors = {}
        done = set()
        for g, opts in geoms:
            if g[1:] in done or (only and only not in geom_id(g, opts)):
                continue
            done.add(g[1:])
            predictors[predictor_id(g)] = trace_predictors(g, rec)
    return {"records": records, "predictors": predictors}, sorted(slow, reverse=True)


def load(path):
    with open(path) as f:
        return json.load(f)


DIGEST_HEX = 8


def digest(trace):
    """The committed form of a trace (tests/golden/ops_conv_calls.json; the full text of 4,716 records is 0.7 MiB): per geometry ONE
    string, the first DIGEST_HEX hex digits of SHA-256(point key + record as sorted JSON) of its points in sorted key order, plus the
    counts.  A changed, missing or extra record changes its geometry's string; `differing` names the points."""
    import hashlib
    out = {"counts": summary(trace)}
    for part in ("records", "predictors"):
        out[part] = {g: "".join(hashlib.sha256((k + json.dumps(pts[k], sort_keys=True)).encode()).hexdigest()[:DIGEST_HEX] for k in sorted(pts))
                     for g, pts in trace[part].items()}
    return out


def differing(trace, want):
    """"part geometry|point" of every point of ``trace`` whose digest is not the one ``want`` (a digest()) holds at its place."""
    got, out = digest(trace), []
    for part in ("records", "predictors"):
        for g in sorted(set(got[part]) | set(want[part])):
            a, b = got[part].get(g, ""), want[part].get(g, "")
            if a != b:
                keys = sorted(trace[part].get(g, {}))
                bad = [k for i, k in enumerate(keys) if a[i * DIGEST_HEX:(i + 1) * DIGEST_HEX] != b[i * DIGEST_HEX:(i + 1) * DIGEST_HEX]]
                out += [f"{part} {g}|{k}" for k in bad] or [f"{part} {g} (another number of points)"]
    return out


def flat(trace):
    """{"part geometry|point": record}"""
    return {f"{part} {g}|{k}": r for part in ("records", "predictors") for g, pts in trace[part].items() for k, r in pts.items()}


def diff(a, b, show=10):
    n = 0
    a, b = flat(a), flat(b)
    for part in ("",):
        for key in sorted(set(a) | set(b)):
            ra, rb = a.get(key), b.get(key)
            if ra != rb:
                n += 1
                if n <= show:
                    print(f"--- {part} {key}\n  a: {json.dumps(ra)}\n  b: {json.dumps(rb)}")
    return n


def summary(trace):
    recs = {f"{g}|{k}": r for g, pts in trace["records"].items() for k, r in pts.items()}
    return dict(records=len(recs), refusals=sum("exc" in r for r in recs.values()), skipped=sum("skip" in r for r in recs.values()),
                predictor_geometries=len(trace["predictors"]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="the full trace (for --diff)")
    ap.add_argument("--digest", help="the trace's digest form (the golden file)")
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--only", help="geometry ids containing this text")
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    a = ap.parse_args(argv)
    if a.diff:
        ta, tb = (load(p) for p in a.diff)
        n = diff(ta, tb)
        print(json.dumps(dict(differing_records=n, a=summary(ta), b=summary(tb))))
        return 1 if n else 0
    t0 = time.time()
    trace, slow = run(a.dry, a.only, progress=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(trace, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
    if a.digest:
        with open(a.digest, "w") as f:
            json.dump(digest(trace), f, indent=0, sort_keys=True)
            f.write("\n")
    print(json.dumps(dict(summary(trace), seconds=round(time.time() - t0, 1), slowest=[(round(t, 2), g) for t, g in slow[:5]])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
