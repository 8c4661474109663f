"""Host-side halves of tests/test_group_tables_gpu.py (no GPU needed): the table capacities the GPU cases are built around, what
dg_adam_step_group_x3 and dg_x3_transpose_planes refuse before they launch anything (dummy non-null 16-byte-aligned pointers: validation
ends the call first), their empty tables, the partition of a parameter group into tiled weights and ranges (optim.x3_group_partition),
and the discrimination of the float64 bound of tests/adam_ref.py."""
import ctypes
import os
import random
import re

import pytest
import torch

from discogan_modernized_amd import _lib, model, ops, optim
from tests import adam_ref as A

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "discogan_modernized_amd", "csrc")
P = ctypes.c_void_p
NUMEL = 1 << 20


def _define(path, name):
    with open(os.path.join(CSRC, path)) as f:
        m = re.findall(rf"^#define {name} (\d+)\s*$", f.read(), flags=re.M)
    assert len(m) == 1, (path, name, m)
    return int(m[0])


def test_the_mirrored_table_capacities_are_the_sources():
    """The GPU cases place weights and ranges around 48 and 64 entries: a changed capacity must change them too."""
    assert _define("x3_table.h", "DG_X3T_MAX") == A.X3T_MAX == 48
    assert _define("optim.hip", "DG_ADAM_RANGES_MAX") == A.ADAM_RANGES_MAX == 64


def _group(weights, ranges, numel=NUMEL, plane_elems=None, ptr=16, odd=None, null=None):
    """dg_adam_step_group_x3 on dummy pointers; odd: one buffer's address instead of `ptr`; null: "w" / "r" = that list's arrays null."""
    nw, w_off, w_k, w_j, nr, r_off, r_len = ops.adam_group_x3_table(weights, ranges)
    buf = {k: P(ptr) for k in ("p", "g", "m", "v", "state", "p3", "p3t")}
    if odd:
        buf[odd[0]] = P(odd[1])
    if null == "w":
        w_off = w_k = w_j = None
    if null == "r":
        r_off = r_len = None
    L = _lib.load()
    rc = L.dg_adam_step_group_x3(buf["p"], buf["g"], buf["m"], buf["v"], numel, buf["state"], 0.5, 0.999, 1e-8, 0.0, 1.0, None, buf["p3"],
                                 buf["p3t"], numel if plane_elems is None else plane_elems, w_off, w_k, w_j, nw, r_off, r_len, nr, None)
    return rc, L.dg_last_error()


def _alternating(n):
    """n weights of 64 x 64 and n ranges of 72 parameters, alternating in memory, 8 elements apart: ([(off, K, J)], [(begin, end)])."""
    weights, ranges, cur = [], [], 0
    for _ in range(n):
        weights.append((cur, 64, 64))
        cur += 4096 + 8
        ranges.append((cur, cur + 72))
        cur += 72 + 8
    return weights, ranges


W, R2 = (0, 64, 64), (4096, 4096 + 72)
GROUP_REFUSALS = [
    ("null weight table", dict(weights=[W], ranges=[], null="w"), b"or a null table"),
    ("null range table", dict(weights=[], ranges=[R2], null="r"), b"or a null table"),
    ("K 96", dict(weights=[(0, 96, 64)], ranges=[]), b"weight 0 (K=96, J=64, offset 0): K and J multiples of 64"),
    ("J 80", dict(weights=[W, (4096, 64, 80)], ranges=[]), b"weight 1 (K=64, J=80, offset 4096): K and J multiples of 64"),
    ("K 0", dict(weights=[(0, 0, 64)], ranges=[]), b"weight 0 (K=0, J=64"),
    ("weight offset 4", dict(weights=[(4, 64, 64)], ranges=[]), b"weight 0 (K=64, J=64, offset 4)"),
    ("descending weights", dict(weights=[(4096, 64, 64), W], ranges=[]), b"weight 1 (K=64, J=64, offset 0)"),
    ("overlapping weights", dict(weights=[W, (4088, 64, 64)], ranges=[]), b"weight 1 (K=64, J=64, offset 4088)"),
    ("weight past numel", dict(weights=[(NUMEL - 4088, 64, 64)], ranges=[]), b"weight 0 (K=64, J=64, offset 1044488)"),
    ("range offset 4", dict(weights=[], ranges=[(4, 12)]), b"range 0 (offset 4, 8 parameters)"),
    ("overlapping ranges", dict(weights=[], ranges=[(0, 16), (8, 24)]), b"range 1 (offset 8, 16 parameters)"),
    ("descending ranges", dict(weights=[], ranges=[(64, 72), (0, 8)]), b"range 1 (offset 0, 8 parameters)"),
    ("negative range length", dict(weights=[], ranges=[(16, 8)]), b"range 0 (offset 16, -8 parameters)"),
    ("range past numel", dict(weights=[], ranges=[(NUMEL - 8, NUMEL + 1)]), b"range 0 (offset 1048568, 9 parameters)"),
    ("plane distance below numel", dict(weights=[W], ranges=[], plane_elems=NUMEL - 8), b"plane distance 1048568 for 1048576 parameters"),
    ("plane distance no multiple of 8", dict(weights=[W], ranges=[], plane_elems=NUMEL + 4), b"plane distance 1048580 for"),
    ("misaligned p", dict(weights=[W], ranges=[], odd=("p", 24)), b"16-byte aligned"),
    ("misaligned transposed planes", dict(weights=[W], ranges=[], odd=("p3t", 8)), b"16-byte aligned"),
    # new: the two lists against each other
    ("range starts inside a weight", dict(weights=[W], ranges=[(4088, 4160)]),
     b"weight 0 (offset 0, 4096 parameters) overlaps range 0 (offset 4088, 72 parameters)"),
    ("weight starts inside a range", dict(weights=[(64, 64, 64)], ranges=[(0, 72)]),
     b"weight 0 (offset 64, 4096 parameters) overlaps range 0 (offset 0, 72 parameters)"),
    ("range inside a weight", dict(weights=[W, (8192, 64, 64)], ranges=[(8, 16), (8200, 8208)]),
     b"weight 0 (offset 0, 4096 parameters) overlaps range 0 (offset 8, 8 parameters)"),
    ("weight inside a range", dict(weights=[(64, 64, 64)], ranges=[(0, 8192)]),
     b"weight 0 (offset 64, 4096 parameters) overlaps range 0 (offset 0, 8192 parameters)"),
]


@pytest.mark.parametrize("what,kw,message", GROUP_REFUSALS, ids=[c[0] for c in GROUP_REFUSALS])
def test_group_step_refusals(what, kw, message):
    rc, err = _group(**kw)
    assert rc == -1 and err.startswith(b"dg_adam_step_group_x3: ") and message in err, err


@pytest.mark.parametrize("which", ["weight", "range"])
def test_group_step_refuses_an_overlap_past_the_first_tables(which):
    """70 weights and 70 ranges, alternating: the last pair overlaps by 8 elements, either way round -- entries past the first
    48-weight and the first 64-range table; one pair fewer and the lists are disjoint."""
    weights, ranges = _alternating(70)
    if which == "range":                   # range 69 starts 8 elements before weight 69 ends
        b, e = ranges[69]
        ranges[69] = (b - 16, e - 16)
        want = b"weight 69 (offset %d, 4096 parameters) overlaps range 69 (offset %d, 72 parameters)" % (weights[69][0], b - 16)
    else:                                  # weight 69 starts 8 elements before range 68 ends
        weights[69] = (weights[69][0] - 16, 64, 64)
        want = b"weight 69 (offset %d, 4096 parameters) overlaps range 68 (offset %d, 72 parameters)" % (weights[69][0], ranges[68][0])
    rc, err = _group(weights, ranges)
    assert rc == -1 and want in err, err
    # only that pair is at fault: the entries before it cover every element at most once (the accepted call would launch, so the
    # GPU module makes it: its alternating cases are such lists)
    cw, cr = A.coverage(NUMEL, weights[:69], ranges[:68])
    assert int((cw + cr).max()) == 1


def test_group_step_takes_empty_tables_and_empty_ranges():
    """No weight and no range, or ranges of no parameters only (even at a weight's offset): DG_OK, nothing to launch."""
    assert _group([], [])[0] == 0
    assert _group([], [], null="w")[0] == 0 and _group([], [], null="r")[0] == 0
    assert _group([], [(0, 0), (0, 0), (64, 64)])[0] == 0
    assert _group([], [(8 * i, 8 * i) for i in range(130)])[0] == 0


def _transpose(convs, n=None, plane_elems=NUMEL):
    tn, off, k, j = ops.x3_transpose_table(convs)
    L = _lib.load()
    rc = L.dg_x3_transpose_planes(P(16), P(16), plane_elems, off, k, j, tn if n is None else n, None)
    return rc, L.dg_last_error()


def test_transpose_refusals():
    """n < 0, K = 0, and a weight past the plane at entry 50: the whole table is checked before the first launch, so the first 48
    weights are not transposed either."""
    rc, err = _transpose([(0, 64, 64)], n=-1)
    assert rc == -1 and b"dg_x3_transpose_planes: n=-1" in err, err
    rc, err = _transpose([(0, 0, 64)])
    assert rc == -1 and b"weight 0 (K=0, J=64, offset 0) outside the plane" in err, err
    rc, err = _transpose([(0, 64, 0)])
    assert rc == -1 and b"weight 0 (K=64, J=0, offset 0) outside the plane" in err, err
    rc, err = _transpose([(-8, 8, 8)])
    assert rc == -1 and b"weight 0 (K=8, J=8, offset -8) outside the plane" in err, err
    convs = [(4096 * i, 64, 64) for i in range(60)]
    convs[50] = (NUMEL - 4088, 64, 64)
    rc, err = _transpose(convs)
    assert rc == -1 and b"weight 50 (K=64, J=64, offset 1044488) outside the plane" in err, err


def test_transpose_takes_an_empty_table():
    assert _transpose([])[0] == 0


# ---- the partition of a parameter group (optim.Adam.enable_x3_planes) ---------------------------------------------------------------
def _random_entries(rng):
    """(offset, shape, is KRSC-strided) of a random parameter list at optim.Adam's offsets (each parameter padded to 64 elements):
    vectors, conv weights of both memory orders with and without whole tiles, 3-channel and one-row weights, parameters of no elements."""
    entries, total = [], 0
    for _ in range(rng.randint(1, 40)):
        kind = rng.choice(["vector", "conv", "conv", "empty", "matrix"])
        if kind == "vector":
            shape, krsc = (rng.choice([1, 7, 24, 64, 100, 129, 2048]),), False
        elif kind == "matrix":
            shape, krsc = (rng.choice([3, 64]), rng.choice([5, 64])), False
        elif kind == "empty":
            shape, krsc = rng.choice([(0,), (0, 4, 4, 4), (64, 0, 4, 4), (3, 0)]), rng.random() < 0.5
        else:
            shape = (rng.choice([1, 3, 64, 100, 128, 192]), rng.choice([3, 4, 8, 12, 20, 64]), 4, 4)
            krsc = rng.random() < 0.8
            if rng.random() < 0.1:
                shape = shape[:2] + (3, 3)
        entries.append((total, shape, krsc))
        total += optim._padded(optim._numel(shape))
    return entries, total


def _partition_before_the_helper(entries):
    """The rule as optim.Adam.enable_x3_planes spelt it out before it became x3_group_partition (parameters of no elements left out:
    they made it emit empty ranges)."""
    convs = [(off, s[0], 16 * s[1]) for off, s, krsc in entries if len(s) == 4 and tuple(s[2:]) == (4, 4) and s[0] > 1 and krsc]
    tiled = [c for c in convs if c[1] % 64 == 0 and c[2] % 64 == 0 and c[0] % 8 == 0]
    tiled_offs = {c[0] for c in tiled}
    rest = []
    for off, s, _ in entries:
        if off in tiled_offs:
            continue
        end = off + (optim._numel(s) + 63) // 64 * 64
        if rest and rest[-1][1] == off:
            rest[-1][1] = end
        else:
            rest.append([off, end])
    return tiled, rest, [c for c in convs if c[0] not in tiled_offs]


@pytest.mark.parametrize("seed", range(40))
def test_group_partition_covers_every_element_once(seed):
    rng = random.Random(seed)
    entries, numel = _random_entries(rng)
    tiled, rest, transposed_rest = optim.x3_group_partition(entries)
    cw, cr = A.coverage(numel, tiled, rest)
    assert numel == 0 or bool(((cw + cr) == 1).all())                          # exactly one tiled weight or one range
    assert all(b < e for b, e in rest)                                        # no range of no parameters
    assert all(a[1] < b[0] for a, b in zip(rest, rest[1:]))                    # ascending, and merged where adjacent
    assert all(a[0] + a[1] * a[2] <= b[0] for a, b in zip(tiled, tiled[1:]))
    assert all(k % 64 == 0 and j % 64 == 0 and k >= 64 and j >= 64 and off % 8 == 0 for off, k, j in tiled)
    # the images that keep the transpose pass lie inside the ranges, and with the tiled ones they are the group's conv images
    assert all(any(b <= off and off + k * j <= e for b, e in rest) for off, k, j in transposed_rest)
    assert sorted(tiled + transposed_rest) == sorted(optim.x3_conv_images(entries))
    # the same lists as the rule gave before it was a helper
    nonempty = [e for e in entries if optim._numel(e[1])]
    old = _partition_before_the_helper(nonempty)
    new = optim.x3_group_partition(nonempty)
    assert (old[0], [tuple(r) for r in old[1]], old[2]) == (new[0], [tuple(r) for r in new[1]], new[2])


def test_model_groups_stay_under_the_table_capacities():
    """The 512 px generator pair as the trainer groups it (shapes only: built on the meta device): 24 tiled weights, all of the
    128-wide class, and 25 ranges (4 conv images among them keep the transpose pass), against capacities of 48 and 64.  One launch
    of the tiled kernel and one for the ranges: all that smoke() and the benchmark exercise, and why
    tests/test_group_tables_gpu.py builds larger groups by hand."""
    with torch.device("meta"):
        nets = [model.Generator(image_size=512), model.Generator(image_size=512)]
    entries, total = [], 0
    for p in (p for net in nets for p in net.parameters()):
        entries.append((total, tuple(p.shape), ops.is_krsc(p)))
        total += optim._padded(p.numel())
    tiled, rest, transposed_rest = optim.x3_group_partition(entries)
    wide = sum(1 for c in tiled if c[2] % 128 == 0)
    print(f"512 px generator pair: nw={len(tiled)} ({wide} of the 128-wide class) nr={len(rest)} transposed_rest={len(transposed_rest)}")
    assert (len(tiled), wide, len(rest), len(transposed_rest)) == (24, 24, 25, 4)
    assert wide <= A.X3T_MAX and len(tiled) - wide <= A.X3T_MAX and len(rest) <= A.ADAM_RANGES_MAX


# ---- the float64 bound tells a missing and a doubled step from the right one ----------------------------------------------------------
def test_the_p_bound_rejects_no_step_and_two_steps():
    """tests/adam_ref.py on the CPU alone: an fp32 evaluation of the step stays inside assert_group_state's bounds; the state left
    as it was, and the state stepped twice, do not."""
    weights, ranges = [(8, 64, 64)], [(4112, 4121), (4128, 4128), (4136, 4200)]
    numel = 4208
    gen = torch.Generator().manual_seed(3)
    cw, cr = A.coverage(numel, weights, ranges)
    cov = (cw + cr) > 0
    before = {k: torch.where(cov, torch.randn(numel, generator=gen) * 0.05, torch.tensor(A.FP32_SENTINEL)) for k in ("p", "g", "m", "v")}
    before["v"] = before["v"].abs()
    for k in ("p3", "p3t"):
        before[k] = torch.full((3, numel), A.BF16_SENTINEL, dtype=torch.int16).view(torch.bfloat16)
    A.assert_sentinels(before, weights, ranges)
    hp = A.hyper(0.5, 0.999, 1e-8, 1e-2)
    step, bc2 = 2e-4 / (1 - 0.5 ** 3), (1 - 0.999 ** 3) ** 0.5

    def fp32_steps(times):
        p, m, v = before["p"].clone(), before["m"].clone(), before["v"].clone()
        for _ in range(times):
            pn, mn, vn = (t.float() for t in A.one_step(p.double(), before["g"].double(), m.double(), v.double(), hp, step, bc2))
            p, m, v = torch.where(cov, pn, p), torch.where(cov, mn, m), torch.where(cov, vn, v)
        p3 = torch.where(cov, A.split3(p), before["p3"])
        return dict(p=p, g=before["g"], m=m, v=v, p3=p3, p3t=A.transposed_planes(p3, before["p3t"], weights))

    A.assert_group_state(before, fp32_steps(1), weights, ranges, hp, step, bc2, what="one step")
    A.assert_bound_is_not_vacuous(before, weights, ranges, hp, step, bc2)
    for times in (0, 2):
        with pytest.raises(AssertionError, match=": p, worst"):
            A.assert_group_state(before, fp32_steps(times), weights, ranges, hp, step, bc2, what=f"{times} steps")
    # a plane buffer written outside the tables, and a transposed image left untransposed, are told apart too
    bad = fp32_steps(1)
    bad["p3"][1, 0] = 1.0
    with pytest.raises(AssertionError, match="p3 outside the tables"):
        A.assert_group_state(before, bad, weights, ranges, hp, step, bc2)
    bad = fp32_steps(1)
    bad["p3t"][:, 8:8 + 4096] = bad["p3"][:, 8:8 + 4096]
    with pytest.raises(AssertionError, match="transposed planes"):
        A.assert_group_state(before, bad, weights, ranges, hp, step, bc2)
