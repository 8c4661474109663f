"""Float64 references of the Adam kernels (csrc/optim.hip), shared by tests/test_reductions_gpu.py, tests/test_group_tables_gpu.py and
tests/test_group_tables_cpu.py: torch's own three-plane split, one step of the kernel's op-by-op formula in float64, and the expected
state of a whole flat group given as host tables (ops.adam_step_group_x3).

Bounds, at the scale these tests use (p, g, m ~ 0.05 N(0, 1), v = |0.05 N(0, 1)|, lr 2e-4, betas (0.5, 0.999)):
  p   2e-7 absolute (test_adam_flat_matches_torch's bound: the update is ~1e-5 and below, the rounding of p itself ~1e-8);
  m   m + (g' - m) (1 - b1) with g' = g s + wd p: four roundings (s and 1 - b1 are powers of two here) relative to the reference
      evaluated on absolute values -> gamma(4);
  v   the same count on v b2 + (1 - b2) g'^2, whose second term is a thousandth of the first.
"""
import torch

from tests import shape_ref as R
from tests.shape_ref import f64, gamma

P_BOUND = 2e-7
# table capacities of the kernels, mirrored (tests/test_group_tables_cpu.py holds them to the sources): weights per launch of
# x3_transpose_kernel / adam_step_x3t_kernel (csrc/x3_table.h), ranges per launch of adam_step_ranges_x3_kernel (csrc/optim.hip)
X3T_MAX = 48
ADAM_RANGES_MAX = 64


def split3(p):
    """torch's own three-plane split of an fp32 CPU tensor."""
    hi = p.bfloat16()
    mid = (p - hi.float()).bfloat16()
    lo = (p - hi.float() - mid.float()).bfloat16()
    return torch.stack([hi, mid, lo])


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def hyper(b1, b2, eps, wd):
    """The hyper-parameters as the kernel takes them: rounded to fp32 (1 - b1 and 1 - b2 formed in fp32 as the kernel forms them)."""
    b1f, b2f = f32(b1), f32(b2)
    return dict(b1=b1f, b2=b2f, eps=f32(eps), wd=f32(wd), omb1=f32(1.0 - b1f), omb2=f32(1.0 - b2f))


def one_step(p0, g0, m0, v0, hp, step_size, bc2_sqrt, gscale=1.0):
    """One step of adam_one in float64: (p, m, v).  hp: hyper(); step_size / bc2_sqrt: elements 1 and 2 of the device state vector."""
    gr = g0 * gscale + hp["wd"] * p0
    m = m0 + (gr - m0) * hp["omb1"]
    v = v0 * hp["b2"] + hp["omb2"] * gr * gr
    return p0 - step_size * (m / (v.sqrt() / bc2_sqrt + hp["eps"])), m, v


def moment_bounds(p0, g0, m0, v0, hp, gscale=1.0):
    """(bound of |m - ref|, bound of |v - ref|): gamma(4) on the two chains evaluated on absolute values."""
    absg = g0.abs() * abs(gscale) + hp["wd"] * p0.abs()
    mabs = m0.abs() + (absg + m0.abs()) * hp["omb1"]
    vabs = v0 * hp["b2"] + hp["omb2"] * absg * absg
    return gamma(4) * mabs + R.TINY, gamma(4) * vabs + R.TINY


# ---- a whole flat group given as host tables -----------------------------------------------------------------------------------------
# weights = [(element offset, K, J), ...] (tiled: p, m, v, planes and transposed planes), ranges = [(begin, end), ...] (p, m, v, planes).
# A state is a dict of CPU tensors p, g, m, v (fp32 [numel]) and p3, p3t (bf16 [3, numel]; p3t may be None when there is no weight).
FP32_SENTINEL = 7.0
BF16_SENTINEL = 0x5A5B              # bit pattern of the plane buffers where nothing may be written (bf16 3.75e16, not zero)
BUFFERS = ("p", "m", "v", "p3", "p3t")


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def coverage(numel, weights, ranges):
    """How many times each element is covered, per list: (by a weight, by a range) as int32 [numel]."""
    cw, cr = torch.zeros(numel, dtype=torch.int32), torch.zeros(numel, dtype=torch.int32)
    for off, k, j in weights:
        cw[off:off + k * j] += 1
    for b, e in ranges:
        cr[b:e] += 1
    return cw, cr


def transposed_planes(p3, p3t_before, weights):
    """The transposed plane buffer after a step: every weight's [K][J] images of p3 as [J][K] at the same offset, the rest as before."""
    out = p3t_before.clone()
    for off, k, j in weights:
        out[:, off:off + k * j] = p3[:, off:off + k * j].view(3, k, j).transpose(1, 2).reshape(3, -1)
    return out


def group_reference(before, weights, ranges, hp, step_size, bc2_sqrt, gscale=1.0, times=1):
    """fp64 (p, m, v) of the whole buffer after `times` steps of every element (the caller looks at the covered ones)."""
    p, m, v = f64(before["p"]), f64(before["m"]), f64(before["v"])
    g = f64(before["g"])
    for _ in range(times):
        p, m, v = one_step(p, g, m, v, hp, step_size, bc2_sqrt, gscale)
    return p, m, v


def assert_group_state(before, after, weights, ranges, hp, step_size, bc2_sqrt, gscale=1.0, what=""):
    """`after` is one step of the group `before`:
      covered elements of p, m, v   the float64 step under P_BOUND and moment_bounds;
      planes                        bitwise split3 of the kernel's own new p, adding up to it exactly;
      transposed planes             bitwise the transposition of the planes, weight by weight at the same offset;
      everything else               the bits it had, in all five buffers (for p3t: everything outside the weights).
    Every element is covered at most once.  Returns the fp64 reference (p, m, v)."""
    numel = before["p"].numel()
    cw, cr = coverage(numel, weights, ranges)
    assert int((cw + cr).max() if numel else 0) <= 1, f"{what}: the case's own tables overlap"
    cov = (cw + cr) > 0
    pr, mr, vr = group_reference(before, weights, ranges, hp, step_size, bc2_sqrt, gscale)
    p0, g0, m0, v0 = (f64(before[k]) for k in ("p", "g", "m", "v"))
    mb, vb = moment_bounds(p0, g0, m0, v0, hp, gscale)
    ep = (after["p"].double() - pr).abs()[cov]
    assert R.exceeds(ep, torch.full_like(ep, P_BOUND)) == 0, f"{what}: p, worst {float(ep.max()):.3e}"
    assert R.exceeds((after["m"].double() - mr).abs()[cov], mb[cov]) == 0, f"{what}: m"
    assert R.exceeds((after["v"].double() - vr).abs()[cov], vb[cov]) == 0, f"{what}: v"
    # planes of the covered elements: torch's split of the new parameters, which add up to them exactly
    ref3 = split3(after["p"])
    assert torch.equal(bits(after["p3"])[:, cov], bits(ref3)[:, cov]), f"{what}: planes"
    assert torch.equal(after["p3"].double().sum(0)[cov], after["p"].double()[cov]), f"{what}: planes do not add up"
    if weights:
        assert torch.equal(bits(after["p3t"]), bits(transposed_planes(after["p3"], before["p3t"], weights))), f"{what}: transposed planes"
    # what neither list covers keeps its bits
    for name in BUFFERS:
        if after.get(name) is None:
            continue
        keep = ~(cw > 0) if name == "p3t" else ~cov
        assert torch.equal(bits(after[name])[..., keep], bits(before[name])[..., keep]), f"{what}: {name} outside the tables"
    assert torch.equal(bits(after["g"]), bits(before["g"])), f"{what}: the gradient was written"
    return pr, mr, vr


def assert_sentinels(before, weights, ranges):
    """The case is built as documented: the sentinel wherever neither list covers, and some such element exists."""
    cw, cr = coverage(before["p"].numel(), weights, ranges)
    free = (cw + cr) == 0
    assert bool(free.any())
    for name in ("p", "m", "v"):
        assert bool((before[name][free] == FP32_SENTINEL).all()), name
    for name in ("p3", "p3t"):
        if before.get(name) is not None:
            keep = (cw == 0) if name == "p3t" else free
            assert bool((bits(before[name])[:, keep] == BF16_SENTINEL).all()), name


def assert_bound_is_not_vacuous(before, weights, ranges, hp, step_size, bc2_sqrt, gscale=1.0, what="", extra_spans=()):
    """P_BOUND tells one step from none and from two: on the first range that holds parameters and on the first weight of the case
    (and on every [begin, end) of extra_spans), the parameters before the step, and the reference formula applied twice, are both
    further than P_BOUND from the reference."""
    p1 = group_reference(before, weights, ranges, hp, step_size, bc2_sqrt, gscale)[0]
    p2 = group_reference(before, weights, ranges, hp, step_size, bc2_sqrt, gscale, times=2)[0]
    p0 = f64(before["p"])
    spans = [(b, e) for b, e in ranges if e > b][:1] + [(off, off + k * j) for off, k, j in weights][:1] + list(extra_spans)
    assert spans, f"{what}: nothing to check"
    for b, e in spans:
        assert float((p0[b:e] - p1[b:e]).abs().max()) > P_BOUND, f"{what}: [{b}, {e}) not stepped would pass"
        assert float((p2[b:e] - p1[b:e]).abs().max()) > P_BOUND, f"{what}: [{b}, {e}) stepped twice would pass"
