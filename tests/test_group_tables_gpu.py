"""The group Adam step and the plane transpose past the capacities of their kernel-argument tables.

dg_x3_transpose_planes takes 48 weights per launch (X3TransposeTable, csrc/x3_table.h); dg_adam_step_group_x3 fills such a table once
per tile class (64 x 128 tiles where J % 128 == 0, 64 x 64 tiles otherwise), skipping the weights of the other class, and then a table
of 64 plain ranges (AdamRangeTable, csrc/optim.hip).  A full table is launched and a new one started: the prefix sums start again at 0,
the second launch walks its own table, the two classes interleave, ranges of no parameters take no slot.  The model never gets there
-- the 512 px generator pair is 24 tiled weights (all of the 128-wide class) and 25 ranges, the discriminators fewer
(test_the_model_groups_stay_under_the_capacities below reads nw = 24, nr = 25 from the tables of an optim.Adam over the real pair;
tests/test_group_tables_cpu.py gets the same from the shapes alone) -- so the groups here are built by hand, of tiny tensors.

Every case of the group step is held to two things.  The documented contract: bitwise ops.adam_step_flat(p3=...) per covered range
and weight, then ops.x3_transpose_planes over the tiled weights.  And, because past 48 weights that transpose is itself only tested
here, an independent reference (tests/adam_ref.py): the float64 step on every covered element, torch's own plane split and
transposition bitwise, and the bits of everything that neither list covers -- the buffers are pre-filled with sentinels there.  The
bound on p is shown to reject a missing and a doubled step in every case.

Through optim.Adam: a group of 110 tiled weights and 110 ranges, three steps, fused against two-kernel form bitwise and against
torch.optim.Adam in float64.  torch's own fp32 run of those three steps lies 2.1e-8 from its float64 run (measured on the CPU, printed
by the test), under the 3 * 2e-7 the kernels are held to.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import ops, optim  # noqa: E402
from tests import adam_ref as A  # noqa: E402
from tests.gpu_util import DEV  # noqa: E402

LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-8
CAP_W, CAP_R = A.X3T_MAX, A.ADAM_RANGES_MAX


# ---- a. dg_x3_transpose_planes past one table ---------------------------------------------------------------------------------------
T_SHAPES = [(64, 64), (8, 16), (36, 80), (100, 32)]          # one tile; less than a tile; ragged 1 x 2 on the element path; ragged 2 x 1
T_GRID = (128, 192)                                          # 2 x 3 tiles: entry 48, the first of the second launch


def _transpose_table(n, reverse):
    shapes = [T_SHAPES[i % len(T_SHAPES)] for i in range(n)]
    if n > CAP_W:
        shapes[CAP_W] = T_GRID
    order = list(reversed(range(n))) if reverse else list(range(n))          # memory order of the table's entries
    offs, cur = [0] * n, 0
    for pos, i in enumerate(order):
        cur = (cur + 7) // 8 * 8 + 8 + (4 if pos % 5 == 4 else 0)            # every fifth image off the 16-byte grid: the element path
        offs[i] = cur
        cur += shapes[i][0] * shapes[i][1]
    return [(o, k, j) for o, (k, j) in zip(offs, shapes)], (cur + 7) // 8 * 8 + 8


@pytest.mark.parametrize("n,reverse", [(0, False), (1, False), (48, False), (49, False), (96, False), (97, False), (150, False), (97, True)])
def test_transpose_planes_past_one_table(n, reverse):
    """[K][J] -> [J][K] at the same offsets for n weights, bitwise torch's transposition; everything outside them keeps the sentinel.
    reverse: the table's offsets descend (this entry point takes any order)."""
    convs, total = _transpose_table(n, reverse)
    assert not reverse or all(a[0] > b[0] for a, b in zip(convs, convs[1:]))
    assert n <= CAP_W or (convs[CAP_W][1:] == T_GRID and len(convs) > CAP_W)
    src = torch.randn(3, total, generator=torch.Generator().manual_seed(n)).bfloat16().to(DEV)
    dst = torch.full((3, total), A.BF16_SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    ref = A.transposed_planes(src, dst, convs)
    ops.x3_transpose_planes(src, dst, ops.x3_transpose_table(convs))
    torch.cuda.synchronize()
    assert torch.equal(A.bits(dst), A.bits(ref))
    covered = sum(k * j for _, k, j in convs)
    assert int((A.bits(dst) == A.BF16_SENTINEL).sum()) >= 3 * (total - covered) > 0             # (the gaps are really there)
    if n:
        wrong = A.transposed_planes(torch.roll(src, 1, dims=1), dst, convs)
        assert not torch.equal(A.bits(wrong), A.bits(ref))


# ---- b. ops.adam_step_group_x3 on hand-built tables ----------------------------------------------------------------------------------
W128, W64 = (64, 128), (64, 64)                  # one tile of each class
G128, G64 = (128, 256), (128, 320)               # 2 x 2 tiles of 64 x 128; 2 x 5 tiles of 64 x 64 (320 % 128 == 64)
R_LENS = [8, 9, 15, 64, 72]                      # one 8-parameter trip; + scalar tail; + 4-parameter trip and tail; 8 trips; 9 trips
BIG = 8 * 4096 * 256 + 8 * 1000 + 5              # one range past flat_grid's cap of 4096 blocks of 256 threads x 8 parameters


def _class(n, tj):
    """n weights of one tile class; entry 48 -- the first of a second launch -- has a two-dimensional tile grid."""
    one, grid = (W128, G128) if tj == 128 else (W64, G64)
    return [("w",) + (grid if i == CAP_W else one) for i in range(n)]


def _ranges(n, zeros=()):
    return [("r", 0 if i in zeros else R_LENS[i % len(R_LENS)]) for i in range(n)]


def _interleave(a, b):
    """a[0], b[0], a[1], b[1], ... and what is left of the longer list."""
    out = [x for pair in zip(a, b) for x in pair]
    return out + a[len(b):] + b[len(a):]


def _sprinkle(ws, every=10):
    """A short range behind every tenth weight: the two lists interleave in memory."""
    out = []
    for i, w in enumerate(ws):
        out.append(w)
        if i % every == every - 1:
            out.append(("r", R_LENS[(i // every) % len(R_LENS)]))
    return out


def _one_among(n, tj, pos):
    """n weights of class tj and a single one of the other class (with the two-dimensional grid) at position pos."""
    ws = _class(n, tj)
    ws.insert(pos, ("w",) + (G64 if tj == 128 else G128))
    return ws


def _layout(items):
    """items in memory order, ("w", K, J) or ("r", length): 8 uncovered elements in front of each, offsets multiples of 8.
    Returns (weights [(off, K, J)], ranges [(begin, end)], numel)."""
    weights, ranges, cur = [], [], 0
    for it in items:
        cur = (cur + 7) // 8 * 8 + 8
        if it[0] == "w":
            weights.append((cur, it[1], it[2]))
            cur += it[1] * it[2]
        else:
            ranges.append((cur, cur + it[1]))
            cur += it[1]
    return weights, ranges, (cur + 7) // 8 * 8 + 8


MIXED = _interleave(_interleave(_class(60, 128), _class(60, 64)), _ranges(129))          # 60 + 60 weights alternating, 129 ranges
GROUP_CASES = {
    **{f"{n} weights of the {tj}-wide class": _sprinkle(_class(n, tj)) for tj in (128, 64) for n in (49, 96, 97)},
    "60 + 60 weights alternating": _sprinkle(_interleave(_class(60, 128), _class(60, 64))),
    **{f"48 of the {tj}-wide class, the other one {name}": _sprinkle(_one_among(48, tj, pos))
       for tj in (128, 64) for name, pos in (("first", 0), ("in the middle", 24), ("last", 48))},
    **{f"{n} ranges": _ranges(n) for n in (64, 65, 128, 129, 200)},
    "66 ranges, range 3 empty": _ranges(66, zeros=(3,)),
    "130 ranges, ranges 0 63 64 129 empty": _ranges(130, zeros=(0, 63, 64, 129)),
    "a range past the block cap between two": [("r", 72), ("r", BIG), ("r", 64)],
    "weights only": _interleave(_class(3, 128), _class(3, 64)),
    "ranges only": _ranges(7),
    "nothing": [],
    "60 + 60 weights alternating, 129 ranges": MIXED,
}
# two weights in the middle of the plain range cases, one of each class: the range launches run behind the tiled ones
for _n in (64, 65, 128, 129, 200):
    _items = GROUP_CASES[f"{_n} ranges"]
    GROUP_CASES[f"{_n} ranges"] = _items[:_n // 3] + [("w",) + W128] + _items[_n // 3:2 * _n // 3] + [("w",) + W64] + _items[2 * _n // 3:]


def _state(advances=2):
    st = torch.zeros(8, device=DEV, dtype=torch.float64)
    for _ in range(advances):
        ops.adam_advance(st, LR, B1, B2)                     # t = 2: bias corrections that are not those of the first step
    return st


def _before(weights, ranges, numel, seed):
    """CPU state: 0.05 N(0, 1) (v: its absolute value) where a list covers, the sentinels everywhere else."""
    gen = torch.Generator().manual_seed(seed)
    cw, cr = A.coverage(numel, weights, ranges)
    cov = (cw + cr) > 0
    st = {k: torch.where(cov, torch.randn(numel, generator=gen) * 0.05, torch.tensor(A.FP32_SENTINEL)) for k in ("p", "g", "m", "v")}
    st["v"] = st["v"].abs()
    st["p3"] = torch.full((3, numel), A.BF16_SENTINEL, dtype=torch.int16).view(torch.bfloat16)
    st["p3t"] = st["p3"].clone() if weights else None
    return st


def _to(state, device):
    return {k: None if t is None else t.to(device) for k, t in state.items()}


def _run_group_case(name, wd, ctl_row=None):
    """One step of the case by ops.adam_step_group_x3 and by the two-kernel form on a copy; returns what the assertions need."""
    weights, ranges, numel = _layout(GROUP_CASES[name])
    before = _before(weights, ranges, numel, seed=len(name) + 31 * len(weights))
    if weights or ranges:
        A.assert_sentinels(before, weights, ranges)
    state = _state()
    ctl = None
    if ctl_row is not None:
        ctl = torch.tensor(ctl_row, device=DEV, dtype=torch.float64)
    state0 = state.clone()
    if ctl is not None:
        ops.adam_advance(state, LR, B1, B2, ctl=ctl)           # as optim.Adam.step: the guarded advance, then the guarded update
    fused, two = _to(before, DEV), _to(before, DEV)
    ops.adam_step_group_x3(fused["p"], fused["g"], fused["m"], fused["v"], state, B1, B2, EPS, wd, 1.0, fused["p3"], fused["p3t"],
                           ops.adam_group_x3_table(weights, ranges), ctl=ctl)
    for b, e in ranges + [(off, off + k * j) for off, k, j in weights]:
        if e > b:
            ops.adam_step_flat(two["p"][b:e], two["g"][b:e], two["m"][b:e], two["v"][b:e], state, B1, B2, EPS, wd, 1.0,
                               p3=(two["p3"].data_ptr() + 2 * b, two["p3"].stride(0)), ctl=ctl)
    if weights:
        ops.x3_transpose_planes(two["p3"], two["p3t"], ops.x3_transpose_table(weights))
    torch.cuda.synchronize()
    for k in A.BUFFERS + ("g",):
        if fused[k] is not None:
            assert torch.equal(A.bits(fused[k]), A.bits(two[k])), f"{name}: {k} differs from the two-kernel form"
    return weights, ranges, before, _to(fused, "cpu"), state0.cpu(), state.cpu()


BIG_CASE = "a range past the block cap between two"              # 34 MB per buffer: at one weight decay only


@pytest.mark.parametrize("name,wd", [(n, wd) for n in GROUP_CASES for wd in (0.0, 1e-2) if not (n == BIG_CASE and wd == 0.0)])
def test_group_step_past_the_tables(name, wd):
    """One step of every case at weight decay 0 and 1e-2: the two-kernel form bitwise (_run_group_case), the float64 reference, the
    sentinels, and the bound's discrimination."""
    weights, ranges, before, after, _, st = _run_group_case(name, wd)
    n128 = sum(1 for w in weights if w[2] % 128 == 0)
    nr = sum(1 for b, e in ranges if e > b)
    print(f"CASE {name}: {n128} + {len(weights) - n128} weights, {len(ranges)} ranges ({nr} with parameters), {before['p'].numel()} elements")
    assert float(st[0]) == 2.0
    hp = A.hyper(B1, B2, EPS, wd)
    A.assert_group_state(before, after, weights, ranges, hp, float(st[1]), float(st[2]), what=name)
    if weights or nr:
        # the ranges on both sides of the first table's end are the ones a table window that slips would step twice or not at all
        live = [r for r in ranges if r[1] > r[0]]
        extra = live[CAP_R - 1:CAP_R + 1] + [(o, o + k * j) for o, k, j in weights][CAP_W:CAP_W + 1]
        A.assert_bound_is_not_vacuous(before, weights, ranges, hp, float(st[1]), float(st[2]), what=name, extra_spans=extra)


def test_the_cases_are_what_they_say():
    """Counts and placements the cases are named after, from the tables the kernels get."""
    def tables(name):
        return _layout(GROUP_CASES[name])

    for tj in (128, 64):
        for n in (49, 96, 97):
            w, r, _ = tables(f"{n} weights of the {tj}-wide class")
            assert len(w) == n and all((x[2] % 128 == 0) == (tj == 128) for x in w) and w[CAP_W][1:] == (G128 if tj == 128 else G64) and r
        for name, pos in (("first", 0), ("in the middle", 24), ("last", 48)):
            w, _, _ = tables(f"48 of the {tj}-wide class, the other one {name}")
            assert len(w) == 49 and [i for i, x in enumerate(w) if (x[2] % 128 == 0) != (tj == 128)] == [pos]
    for name in ("60 + 60 weights alternating", "60 + 60 weights alternating, 129 ranges"):
        w, r, numel = tables(name)
        wide = [x[2] % 128 == 0 for x in w]
        assert wide == [True, False] * 60 and numel < 1 << 20
        assert [x for x in w if x[2] % 128 == 0][CAP_W][1:] == G128 and [x for x in w if x[2] % 128][CAP_W][1:] == G64
    assert len(tables("60 + 60 weights alternating, 129 ranges")[1]) == 129
    for n in (64, 65, 128, 129, 200):
        w, r, _ = tables(f"{n} ranges")
        assert len(r) == n and len(w) == 2 and {e - b for b, e in r} == set(R_LENS)
        assert all(r[i + 1][0] - r[i][1] >= 8 for i in range(n - 1))                       # uncovered gaps between the ranges
    _, r, _ = tables("66 ranges, range 3 empty")
    assert len(r) == 66 and [i for i, (b, e) in enumerate(r) if e == b] == [3]
    _, r, _ = tables("130 ranges, ranges 0 63 64 129 empty")
    assert len(r) == 130 and [i for i, (b, e) in enumerate(r) if e == b] == [0, 63, 64, 129]
    _, r, _ = tables("a range past the block cap between two")
    assert [e - b for b, e in r] == [72, BIG, 64] and BIG // 8 > 4096 * 256 and BIG % 8 == 5
    assert tables("weights only")[1] == [] and tables("ranges only")[0] == [] and tables("nothing")[:2] == ([], [])


def test_an_empty_group_changes_nothing():
    weights, ranges, before, after, _, _ = _run_group_case("nothing", 1e-2)
    assert not weights and not ranges
    for k in ("p", "g", "m", "v", "p3"):
        assert torch.equal(A.bits(after[k]), A.bits(before[k])), k


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_group_step_clipped_by_the_control_block(wd):
    """ctl[2] = 0.25, ctl[3] = 0: the step of the 60 + 60 / 129-range group with the gradient scaled by 0.25 on the device."""
    name = "60 + 60 weights alternating, 129 ranges"
    weights, ranges, before, after, st0, st = _run_group_case(name, wd, ctl_row=[0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0])
    assert float(st0[0]) == 2.0 and float(st[0]) == 3.0
    hp = A.hyper(B1, B2, EPS, wd)
    A.assert_group_state(before, after, weights, ranges, hp, float(st[1]), float(st[2]), gscale=0.25, what=name)
    A.assert_bound_is_not_vacuous(before, weights, ranges, hp, float(st[1]), float(st[2]), gscale=0.25, what=name)
    # ... and the scale matters to the bound: the unscaled step is somewhere else
    p_unscaled = A.group_reference(before, weights, ranges, hp, float(st[1]), float(st[2]), gscale=1.0)[0]
    b, e = ranges[0]
    assert float((p_unscaled[b:e] - after["p"][b:e].double()).abs().max()) > A.P_BOUND


def test_group_step_skipped_by_the_control_block():
    """ctl[3] = 1: every bit of the five buffers and of the step state is kept."""
    name = "60 + 60 weights alternating, 129 ranges"
    weights, ranges, before, after, st0, st = _run_group_case(name, 1e-2, ctl_row=[0.0, 0.0, 0.25, 1.0, 0.0, 0.0, 0.0, 0.0])
    assert torch.equal(st, st0) and float(st[0]) == 2.0
    for k in ("p", "g", "m", "v", "p3", "p3t"):
        assert torch.equal(A.bits(after[k]), A.bits(before[k])), k


# ---- c. through optim.Adam ---------------------------------------------------------------------------------------------------------------
OPT_BUFFERS = ("flat_p", "exp_avg", "exp_avg_sq", "flat_p3", "flat_p3t")
OPT_WD = 1e-2
OPT_STEPS = 3


def _opt_shapes():
    """55 + 55 weights of the two classes alternating, a 24-element vector between every two of them, and two conv weights that are
    no whole tiles (K = 100; J = 48) at the end."""
    shapes = []
    for i in range(110):
        shapes.append((64, 4) if i % 2 == 0 else (64, 8))               # [K, C, 4, 4]: J = 64 / J = 128
        if i < 109:
            shapes.append(24)
    return shapes + [(100, 8), (64, 3)]


def _opt_tensors(seed, scale):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen) * scale if isinstance(s, int) else torch.randn(s[0], s[1], 4, 4, generator=gen) * scale
            for s in _opt_shapes()]


def _opt_group(init):
    params = [torch.nn.Parameter(t.to(DEV) if t.dim() == 1 else ops.krsc_param(t.to(DEV))) for t in init]
    opt = optim.Adam(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=OPT_WD)
    opt.enable_x3_planes()
    return opt


def _torch_run(init, grads, dtype):
    ps = [torch.nn.Parameter(t.clone().to(dtype)) for t in init]
    ref = torch.optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=OPT_WD)
    for step in range(OPT_STEPS):
        for p, g in zip(ps, grads[step]):
            p.grad = g.to(dtype)
        ref.step()
    return [p.detach().double() for p in ps]


def test_the_model_groups_stay_under_the_capacities():
    """The real 512 px generator pair in one flat Adam group with planes: 24 tiled weights, all of the 128-wide class, and 25 ranges,
    none of them empty -- one table each, half of the 48 and well under the 64 (the numbers of the module docstring)."""
    from itertools import chain

    from discogan_modernized_amd import model
    nets = [model.Generator(image_size=512).to(DEV) for _ in range(2)]
    opt = optim.Adam(chain(*(n.parameters() for n in nets)), lr=LR, betas=(B1, B2), weight_decay=1e-5)
    opt.enable_x3_planes()
    nw, _, _, w_j, nr, _, r_len = opt._adam_group_table
    wide = sum(1 for i in range(nw) if w_j[i] % 128 == 0)
    print(f"512 px generator pair: nw={nw} ({wide} of the 128-wide class) nr={nr} transposed_rest={opt._x3t_rest_table[0]} numel={opt.numel}")
    assert (nw, wide, nr, opt._x3t_rest_table[0]) == (24, 24, 25, 4) and all(r_len[i] > 0 for i in range(nr))
    assert wide <= CAP_W and nw - wide <= CAP_W and nr <= CAP_R


def test_optimizer_group_past_both_tables(monkeypatch):
    """optim.Adam over 110 tiled weights and 110 ranges: three steps of the fused form against the two-kernel form, every buffer
    bitwise after each; the parameters after the third against torch.optim.Adam in float64, 3 * 2e-7 (one P_BOUND per step) unless
    torch's own fp32 run is further than that from it (it is 2.1e-8 away: printed below)."""
    init = _opt_tensors(1, 0.05)
    grads = [_opt_tensors(10 + s, 1e-2) for s in range(OPT_STEPS)]
    a, b = _opt_group(init), _opt_group(init)
    nw, _, _, w_j, nr, _, r_len = a._adam_group_table
    print(f"optimizer group: nw={nw} nr={nr} transposed_rest={a._x3t_rest_table[0]} numel={a.numel}")
    assert nw > 2 * CAP_W and nr > CAP_R and a._x3t_rest_table[0] == 2
    assert sum(1 for i in range(nw) if w_j[i] % 128 == 0) == 55 and all(r_len[i] > 0 for i in range(nr))
    for step in range(OPT_STEPS):
        for opt, fused in ((a, True), (b, False)):
            for p, g in zip(opt.params, grads[step]):
                p.grad.copy_(g.to(DEV))
            monkeypatch.setattr(ops, "ADAM_FUSED_T", fused)
            opt.step()
        torch.cuda.synchronize()
        for name in OPT_BUFFERS:
            assert torch.equal(A.bits(getattr(a, name)), A.bits(getattr(b, name))), f"step {step}: {name}"
    assert float(a.state[0]) == OPT_STEPS
    ref64, ref32 = _torch_run(init, grads, torch.float64), _torch_run(init, grads, torch.float32)
    d32 = max(float((x - y).abs().max()) for x, y in zip(ref32, ref64))
    bound = OPT_STEPS * A.P_BOUND if d32 <= OPT_STEPS * A.P_BOUND else 2 * d32
    worst = max(float((p.detach().cpu().double() - r).abs().max()) for p, r in zip(a.params, ref64))
    print(f"optimizer group: fp32 torch against float64 torch {d32:.3e}; kernels against float64 torch {worst:.3e}; bound {bound:.3e}")
    assert worst <= bound
    # the bound tells three steps from two: the float64 run is further than that from where it started
    assert min(float((x.double() - r).abs().max()) for x, r in zip(init, ref64)) > bound
    # planes and transposed planes of the final parameters
    flat = a.flat_p.cpu()
    assert torch.equal(A.bits(a.flat_p3.cpu()), A.bits(A.split3(flat)))
    p3, p3t = a.flat_p3.cpu(), a.flat_p3t.cpu()
    convs = [(off, p.shape[0], 16 * p.shape[1]) for p, off in zip(a.params, a.offsets) if p.dim() == 4]
    assert len(convs) == 112
    assert torch.equal(A.bits(p3t), A.bits(A.transposed_planes(p3, torch.zeros_like(p3t), convs)))
