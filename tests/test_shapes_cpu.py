"""Host-side halves of tests/test_shapes_gpu.py (no GPU needed): the plan queries on both sides of the 2 GiB limits, the
c3 input gradient's argument checks past the scatter kernel's limit, the recorded refusals of every 3-channel edge entry point, and
the discrimination of the fp64 error bound."""
import ctypes
import json
import os

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


# ---- every 3-channel edge entry point: what it refuses before any launch -------------------------------------------------------------
EDGE_REFUSALS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_refusals.json")
_E = "dg_conv4x4s2_c3_"
# parameter names of the entry points, in ABI order
EDGE_PARAMS = {
    "fwd": "x w y N H W K act slope stream",
    "fwd_t": "x w y bf16 N H W K act slope stream",
    "fwd_p": "x w y bf16 N H W K act slope prec stream",
    "fwd_g": "groups x w y N H W K act slope prec stream",
    "fwd_x3": "x w y planes plane_elems N H W K act slope stream",
    "dgrad": "dy w dx N H W K act ws ws_bytes stream",
    "dgrad_t": "dy bf16 w dx N H W K act ws ws_bytes stream",
    "dgrad_p": "dy bf16 w dx N H W K act prec ws ws_bytes stream",
    "dgrad_act_p": "dy bf16 act_out in_act slope w dx N H W K act prec ws ws_bytes stream",
    "dgrad_g": "groups dy w dx N H W K act prec stream",
    "wgrad": "dy x dw N H W K accumulate ws ws_bytes stream",
    "wgrad_act": "dy act_out fact slope x dw N H W K accumulate ws ws_bytes stream",
    "wgrad_t": "dy act_out bf16 fact slope x dw N H W K accumulate ws ws_bytes stream",
    "wgrad_p": "dy act_out bf16 fact slope x dw N H W K prec accumulate ws ws_bytes stream",
    "wgrad_g": "groups share dy act_out fact slope x dw N H W K prec accumulate ws ws_bytes stream",
}
EDGE_POINTERS = ("x", "w", "y", "planes", "dy", "dx", "dw", "act_out", "ws")
BIG = (4096, 512, 512)          # N * 3 * H * W = 3 * 2^30 elements: past every edge kernel's 2^31
GIB = (1024, 512, 512)          # an image tensor of 3 GiB: past the streaming forward's 1 GiB


def edge_refusal_cases():
    """(label, entry point, {parameter: value} over the accepted base call, {option: value}) for argument tuples that every edge
    entry point must refuse before it launches anything.  The base call is (N, H, W, K) = (2, 8, 8, 64), fp32 tensors, no activation,
    arithmetic 0, two problems for the grouped forms, a large enough workspace.  Pointer values: "ptr" a non-null dummy (never
    dereferenced: validation fails first), "ptr2" another one, None null; for a grouped form a table of four of them, "hole" a table
    whose second entry is null, "mixed" a table of two different addresses."""
    cases = []

    def add(what, entry, over, **options):
        if all(k in EDGE_PARAMS[entry].split() for k in over):
            opt = "".join(f" [{k} {v}]" for k, v in sorted(options.items()))
            cases.append((f"{entry}: {what}{opt}", entry, dict(over), dict(options)))

    for entry, params in EDGE_PARAMS.items():
        names = params.split()
        op = entry.split("_")[0]
        grouped = entry.endswith("_g")
        for ptr in EDGE_POINTERS:
            if ptr in names and not (op == "dgrad" and ptr == "ws") and not (op == "wgrad" and ptr in ("act_out", "ws")):
                add(f"null {ptr}", entry, {ptr: None})
                if grouped:
                    add(f"null entry in {ptr}", entry, {ptr: "hole"})
        for g in (0, 5):
            add(f"groups {g}", entry, dict(groups=g))
        add("share 3 of 2 problems", entry, dict(share=3))
        add("share 0", entry, dict(share=0))
        add("mismatched dw in a share set", entry, dict(share=2, dw="mixed"))
        for prec in (-2, 3):
            add(f"prec {prec}", entry, dict(prec=prec))
        for K in ((32, 96) if op == "wgrad" else (0, 2, 6)):
            add(f"K {K}", entry, dict(K=K))
        for dim in ("H", "W"):
            for v in (1, 6, 12):
                add(f"{dim} {v}", entry, {dim: v})
        add("N 0", entry, dict(N=0))
        add("image tensor past 2^31 elements", entry, dict(zip("NHW", BIG)))
        for act in ((1, 7) if op == "dgrad" else (3, 7)):
            add(f"bad act {act}", entry, dict(act=act))
            add(f"bad fused act {act}", entry, dict(fact=act, act_out="ptr"))
        for act in (1, 2):
            add(f"fused act {act} without act_out", entry, dict(fact=act, act_out=None))
        if op != "wgrad":
            for K in (32, 128):
                add(f"bf16 tensor at K {K}", entry, dict(bf16=1, K=K))
                if grouped or entry in ("fwd_x3", "dgrad_act_p"):
                    add(f"K {K}", entry, dict(K=K))
            add("bf16 tensor", entry, dict(bf16=1), kt=16)
            if grouped or entry == "dgrad_act_p":
                add("base call", entry, {}, kt=16)
        if op == "wgrad":
            add("null ws", entry, dict(ws=None))
            add("short ws", entry, dict(ws_bytes="short"))
            add("bf16 tensors on the 64-bit addressing kernels", entry, dict(bf16=1), pointer_path=1)
            if grouped:
                add("null entry in ws", entry, dict(ws="hole"))
        if op == "dgrad" and "ws" in names and entry != "dgrad_act_p":
            add("null ws", entry, dict(ws=None), kt=16)
            add("short ws", entry, dict(ws_bytes="short"), kt=16)
    add("image tensor of 3 GiB", "fwd_g", dict(zip("NHW", GIB)))
    add("image tensor of 3 GiB", "fwd_x3", dict(zip("NHW", GIB), plane_elems=1 << 40))
    add("bf16 output with an image tensor of 3 GiB", "fwd_t", dict(zip("NHW", GIB), bf16=1))
    add("plane distance too small", "fwd_x3", dict(plane_elems=2 * 4 * 4 * 64 - 8))
    add("plane distance no multiple of 8", "fwd_x3", dict(plane_elems=2 * 4 * 4 * 64 + 4))
    for a in (0, 2, 3):
        add(f"in_act {a}", "dgrad_act_p", dict(in_act=a))
    add("bf16 dy past 2^31 bytes", "dgrad_t", dict(N=256, H=512, W=512, bf16=1))
    add("bf16 dy past 2^31 bytes", "dgrad_act_p", dict(N=256, H=512, W=512, bf16=1))
    add("fp32 dy past 2^31 bytes", "dgrad_act_p", dict(N=128, H=512, W=512))
    add("fp32 dy past 2^31 bytes", "dgrad_g", dict(N=128, H=512, W=512))
    return cases


def edge_refusal_codes(L):
    """The return code of every case of edge_refusal_cases(), under each process-default arithmetic: {"0": [...], "1": ..., "2": ...}."""
    P = ctypes.c_void_p
    tables = dict(ptr=(P * 4)(8, 8, 8, 8), hole=(P * 4)(8, None, 8, 8), mixed=(P * 4)(8, 16, 8, 8))
    codes = {}
    try:
        for default in (0, 1, 2):
            _lib.set_option("bf16", default)
            row = codes[str(default)] = []
            for label, entry, over, options in edge_refusal_cases():
                grouped = entry.endswith("_g")
                v = dict(N=2, H=8, W=8, K=64, act=0, fact=0, in_act=ops.ACT_LEAKY, slope=0.2, prec=0, bf16=0, groups=2, share=1, accumulate=0,
                         plane_elems=2 * 4 * 4 * 64, ws_bytes=1 << 20, stream=None, **{p: "ptr" for p in EDGE_POINTERS})
                if entry.startswith("wgrad") and "act_out" not in over:
                    v["act_out"] = None
                v.update(over)
                if v["ws_bytes"] == "short":
                    need = L.dg_c3_wgrad_workspace_bytes(v["N"], v["H"], v["W"], v["K"]) if entry.startswith("wgrad") else L.dg_c3_dgrad_workspace_bytes(v["K"])
                    assert need > 0
                    v["ws_bytes"] = need - 1
                for p in EDGE_POINTERS:
                    if v[p] is not None:
                        v[p] = tables[v[p]] if grouped else P(dict(ptr=8, ptr2=16)[v[p]])
                for k, val in options.items():
                    _lib.set_option(k, val)
                try:
                    row.append(getattr(L, _E + entry)(*[v[n] for n in EDGE_PARAMS[entry].split()]))
                finally:
                    for k in options:
                        _lib.set_option(k, 0)
    finally:
        for k in ("kt", "bf16", "pointer_path"):
            _lib.set_option(k, 0)
    return codes


def test_edge_entry_points_refuse_what_the_recorded_table_says():
    """tests/golden/edge_refusals.json holds the return code of every 3-channel edge entry point for argument tuples that are refused
    before any launch, written from the library of the commit BEFORE the edge host code was rewritten around one call record per op
    (tests/golden/make_edge_refusals.py).  The library must still give exactly these codes: DG_ERR_INVALID (-1) or DG_ERR_WORKSPACE (-2),
    whatever the process-default arithmetic."""
    with open(EDGE_REFUSALS) as f:
        table = json.load(f)
    cases = edge_refusal_cases()
    assert table["cases"] == [c[0] for c in cases] and len(set(table["cases"])) == len(cases)
    codes = edge_refusal_codes(_lib.load())
    assert sorted(codes) == sorted(table["codes"]) == ["0", "1", "2"]
    for default, want in table["codes"].items():
        assert len(want) == len(cases) and all(c in (-1, -2) for c in want)
        for label, got, w in zip(table["cases"], codes[default], want):
            assert got == w, f"{label} (process default arithmetic {default}): {got}, recorded {w}"


# ---- every BatchNorm / activation entry point: what it refuses before any launch ----------------------------------------------------
BN_REFUSALS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_refusals.json")
_BN_FWD = "M C saved gamma beta act slope stream"
_BN_BWD = "M C saved gamma beta act slope dgamma dbeta accumulate ws ws_bytes stream"
_BN_STATS = "M C eps momentum rmean rvar nbt saved ws ws_bytes stream"
# parameter names of the entry points, in ABI order
BN_PARAMS = {
    "dg_bn_train_stats": "y " + _BN_STATS,
    "dg_bn_train_stats_t": "y bf16 " + _BN_STATS,
    "dg_bn_train_stats_g": "groups share y " + _BN_STATS,
    "dg_bn_act_fwd": "y z " + _BN_FWD,
    "dg_bn_act_fwd_g": "groups y z " + _BN_FWD,
    "dg_bn_act_fwd_bf16": "y z shadow " + _BN_FWD,
    "dg_bn_act_fwd_x3": "y z planes plane_elems plane_layout " + _BN_FWD,
    "dg_bn_act_fwd_t": "y z bf16 " + _BN_FWD,
    "dg_bn_act_bwd": "dz y dy " + _BN_BWD,
    "dg_bn_act_bwd_g": "groups share dz y dy " + _BN_BWD,
    "dg_bn_act_bwd_bf16": "dz y dy shadow " + _BN_BWD,
    "dg_bn_act_bwd_x3": "dz y dy planes plane_elems plane_layout " + _BN_BWD,
    "dg_bn_act_bwd_t": "dz y dy bf16 " + _BN_BWD,
    "dg_act_fwd": "x out n act slope stream",
    "dg_act_fwd_g": "groups x out n act slope stream",
    "dg_act_bwd": "dy out dx n act slope stream",
    "dg_act_bwd_g": "groups dy out dx n act slope stream",
    "dg_act_bwd_t": "dy out dx bf16 n act slope stream",
}
BN_POINTERS = ("x", "y", "z", "dz", "dy", "dx", "out", "shadow", "planes", "saved", "gamma", "beta", "rmean", "rvar", "nbt", "dgamma", "dbeta", "ws")
BN_OPTIONAL = ("rmean", "rvar", "nbt", "dgamma", "dbeta")          # null is allowed: such a call would launch


def bn_refusal_cases():
    """(label, entry point, {parameter: value} over the accepted base call) for argument tuples that the BatchNorm and activation
    entry points must refuse before they launch anything.  The base call is (M, C) = (16, 64) fp32 with LeakyReLU, n = 64 for the
    stand-alone activations, two problems for the grouped forms, pixel-major planes M * C elements apart, a large enough workspace.
    Pointer values as in edge_refusal_cases(); "short" is one byte less than dg_bn_workspace_bytes of the BASE shape."""
    cases = []

    def add(what, entry, over):
        if all(k in BN_PARAMS[entry].split() for k in over):
            cases.append((f"{entry}: {what}", entry, dict(over)))

    for entry, params in BN_PARAMS.items():
        names = params.split()
        bn, grouped = entry.startswith("dg_bn_"), entry.endswith("_g")
        stats = "train_stats" in entry
        for g in (0, 5):
            add(f"groups {g}", entry, dict(groups=g))
        add("share 3 of 4 problems", entry, dict(groups=4, share=3))
        for ptr in ("rmean", "dgamma", "dbeta"):
            add(f"mismatched {ptr} in a share set", entry, {"share": 2, ptr: "mixed"})
        for ptr in BN_POINTERS:
            plane_only = ptr in ("z", "dy") and entry.endswith("_x3")                # accepted: the plane triple is then the only output
            if ptr in names and ptr not in BN_OPTIONAL and not plane_only:
                add(f"null {ptr}", entry, {ptr: None})
                if grouped:
                    add(f"null entry in {ptr}", entry, {ptr: "hole"})
        if stats:
            add("M 1", entry, dict(M=1))
        for C in (0, 2, 6):
            add(f"C {C}", entry, dict(C=C))
        for C in (4, 12):
            add(f"bf16 storage at C {C}", entry, dict(bf16=1, C=C))
        if not stats:
            for act in ((-1, 3, 4) if bn else (-1, 4)):
                add(f"bad act {act}", entry, dict(act=act))
        add("short ws", entry, dict(ws_bytes="short"))
        add("short ws at bf16 storage", entry, dict(ws_bytes="short", bf16=1))
        for what, over in (("C 6", dict(C=6)), ("bad act 3", dict(act=3)), ("null y", dict(y=None))):
            if bn and not (stats and "act" in over):
                add(f"null ws and {what}", entry, dict(ws=None, **over))
                add(f"short ws and {what}", entry, dict(ws_bytes="short", **over))
        add("plane_layout 2", entry, dict(plane_layout=2))
        add("plane distance too small", entry, dict(plane_elems=16 * 64 - 8))
        add("plane distance no multiple of 8", entry, dict(plane_elems=16 * 64 + 4))
        add("quad-chunk planes at C 32", entry, dict(plane_layout=1, C=32))
        add("quad-chunk planes at M 18", entry, dict(plane_layout=1, M=18, plane_elems=18 * 64))
        add("null planes and no fp32 output", entry, dict(planes=None, z=None))
        add("null planes and no fp32 output", entry, dict(planes=None, dy=None))
    add("bf16 tensors, n 68", "dg_act_bwd_t", dict(bf16=1, n=68))
    add("bf16 tensors, null dx", "dg_act_bwd_t", dict(bf16=1, dx=None))
    add("bf16 tensors, bad act 4", "dg_act_bwd_t", dict(bf16=1, act=4))
    return cases


def _bn_call(L, entry, over):
    P = ctypes.c_void_p
    tables = dict(ptr=(P * 4)(8, 8, 8, 8), hole=(P * 4)(8, None, 8, 8), mixed=(P * 4)(8, 16, 8, 8))
    v = dict(M=16, C=64, n=64, act=ops.ACT_LEAKY, slope=0.2, eps=1e-5, momentum=0.1, bf16=0, groups=2, share=1, accumulate=0,
             plane_elems=16 * 64, plane_layout=0, ws_bytes=1 << 20, stream=None, **{p: "ptr" for p in BN_POINTERS})
    v.update(over)
    if v["ws_bytes"] == "short":
        v["ws_bytes"] = L.dg_bn_workspace_bytes(16, 64) - 1
    for p in BN_POINTERS:
        if v[p] is not None:
            v[p] = tables[v[p]] if entry.endswith("_g") else P(dict(ptr=8, ptr2=16)[v[p]])
    return getattr(L, entry)(*[v[n] for n in BN_PARAMS[entry].split()])


def bn_refusal_codes(L):
    """The return code of every case of bn_refusal_cases(), under option "bn_items" 0 and 1: {"0": [...], "1": [...]}."""
    codes = {}
    try:
        for items in (0, 1):
            _lib.set_option("bn_items", items)
            codes[str(items)] = [_bn_call(L, entry, over) for label, entry, over in bn_refusal_cases()]
    finally:
        _lib.set_option("bn_items", 0)
    return codes


def test_bn_entry_points_refuse_what_the_recorded_table_says():
    """tests/golden/bn_refusals.json holds the return code of every dg_bn_* / dg_act_* entry point for argument tuples that are
    refused before any launch, written from the library of the commit BEFORE the BatchNorm host code was rewritten around one call
    record per pass (tests/golden/make_bn_refusals.py).  The library must still give exactly these codes: DG_ERR_INVALID (-1) or
    DG_ERR_WORKSPACE (-2), whatever option "bn_items" says.  A stand-alone activation over no elements succeeds without a launch."""
    with open(BN_REFUSALS) as f:
        table = json.load(f)
    cases = bn_refusal_cases()
    assert table["cases"] == [c[0] for c in cases] and len(set(table["cases"])) == len(cases)
    assert {c[1] for c in cases} == set(BN_PARAMS)
    L = _lib.load()
    codes = bn_refusal_codes(L)
    assert sorted(codes) == sorted(table["codes"]) == ["0", "1"]
    for items, want in table["codes"].items():
        assert len(want) == len(cases) and all(c in (-1, -2) for c in want)
        for label, got, w in zip(table["cases"], codes[items], want):
            assert got == w, f"{label} (bn_items {items}): {got}, recorded {w}"
    for entry in BN_PARAMS:
        if entry.startswith("dg_act_"):
            for bf16 in (0, 1):
                assert _bn_call(L, entry, dict(n=0, bf16=bf16)) == 0, (entry, bf16)


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
