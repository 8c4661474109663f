"""Differentiable augmentation on the GPU: the device draw against its numpy restatement, the kernels against the reference (bitwise for
the geometry-only policies, which only copy; within the project's criterion -- four times the float32 reference's own error against
float64, at least one ulp of the value bound 8 -- where colour computes), the grouped forms, the autograd node, the trainer and the CLI.

Kernel buffers sit between sentinel bands; image data of the bitwise tests is random int32 bit patterns viewed as float (NaNs, infinities
and denormals among them), compared as int32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, ops  # noqa: E402
from discogan_modernized_amd import image_translation as it_cli  # noqa: E402
from discogan_modernized_amd.diffaug import DiffAugment, apply_group  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tests import diffaug_ref as DR  # noqa: E402

DEV = "cuda"
BAND = 64                                  # sentinel floats in front of and behind every buffer of the kernel tests
SENTINEL = 0x5EA7BEEF
BIG_SEED, BIG_ITER = (1 << 63) + 5, (1 << 33) + 1
SIZES, BATCHES = (8, 9, 64), (1, 5)
FLOOR = 2.0 ** -20                         # one ulp at the value bound |v| < 8
BIG = 2 ** 31 - 1


def _patterns(shape, seed):
    return np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)


class _Banded:
    """An int32 / float32 array inside a device buffer with a sentinel band on either side; ``shift`` floats of extra offset move the base
    off the 16-byte boundary."""

    def __init__(self, values, shift=0):
        self.shape, self.size = values.shape, values.size
        self.lo = BAND + shift
        host = np.full(self.lo + self.size + BAND, SENTINEL, dtype=np.int32)
        host[self.lo:self.lo + self.size] = np.ascontiguousarray(values).view(np.int32).reshape(-1)
        self.buf = torch.from_numpy(host).to(DEV)

    def view(self):
        return self.buf[self.lo:self.lo + self.size].view(torch.float32).view(self.shape)

    def values(self, dtype=np.int32):
        return self.buf[self.lo:self.lo + self.size].cpu().numpy().view(dtype).reshape(self.shape)

    def bands_intact(self):
        return bool((self.buf[:self.lo] == SENTINEL).all() and (self.buf[self.lo + self.size:] == SENTINEL).all())


def _run_op(op, x_np, recs_np, flags, shift=0, fill=7):
    """One dg_diffaug_fwd / _bwd on banded buffers (the output starts as ``fill``): the output as int32 patterns; the input unwritten,
    every band intact."""
    x, out = _Banded(x_np, shift), _Banded(np.full(x_np.shape, fill, dtype=np.int32), shift)
    recs = torch.from_numpy(np.ascontiguousarray(recs_np)).to(DEV)
    got = op(x.view(), flags, recs, out=out.view())
    assert got.data_ptr() == out.view().data_ptr()
    assert np.array_equal(x.values(), np.ascontiguousarray(x_np).view(np.int32)), "the input was written"
    assert x.bands_intact() and out.bands_intact()
    return out.values()


def _hand_records(S):
    """Shifts at the ends of [-T, T] (and, at 64 px, shifts that keep and that lose the 16-byte alignment of a row); the cut square clipped
    at each corner, covering everything, and fully outside; wild offsets.  Factors are neutral: they are for the geometry-only policies."""
    T, cs = DR.T_of(S), DR.cs_of(S)
    h = cs // 2
    rows = [(T, T, 1, 1), (-T, -T, 0, 0), (T, -T, S - cs, 0), (-T, T, 0, S - cs),
            (0, 0, -h, -h), (0, 0, S - h, -h), (0, 0, -h, S - h), (0, 0, S - h, S - h),            # clipped at the four corners
            (1, 0, S, 0), (0, -1, 0, -cs), (0, 1, -cs, -cs), (-1, 0, S, S),                        # fully outside
            (BIG, 0, 0, 0), (0, -BIG - 1, 0, 0), (-BIG - 1, BIG, BIG, -BIG - 1), (BIG, BIG, -BIG - 1, BIG), (1, 1, BIG - 1, 2),
            (0, 0, -BIG - 1, -BIG - 1), (S, 0, 0, 0), (0, -S, 0, 0), (S - 1, 1 - S, 2, 2)]
    if S >= 16:
        rows += [(4, 0, 3, 5), (-8, 8, 5, 3), (3, -4, 0, 0), (-5, 0, 7, 1), (8, 2, 4, 4)]
    return np.stack([DR.make_record(*r) for r in rows])


def _tables(recs, n):
    """The records in tables of n rows (the last one filled up from the front)."""
    k = -(-len(recs) // n) * n
    idx = np.arange(k) % len(recs)
    return [recs[idx[i:i + n]] for i in range(0, k, n)]


# ---- 1. the draw -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("n", [1, 5, 300])
def test_device_draw_is_the_reference_table(n, S):
    for flags in (7, 1, 6):
        for seed, rank, iteration, d, role in ((1234, 0, 6, 0, 0), (1234, 3, 7, 1, 1), (BIG_SEED, 1, BIG_ITER, 1, 0)):
            got = ops.diffaug_draw(seed, rank, iteration, d, role, n, S, flags, device=DEV)
            assert got.dtype == torch.int32 and tuple(got.shape) == (n, 8)
            assert np.array_equal(got.cpu().numpy(), DR.draw(seed, rank, iteration, d, role, n, S, flags)), (seed, rank, iteration, d, role)
    table = torch.full((n + 3, 8), -7, dtype=torch.int32, device=DEV)                     # rows past n stay as they are
    ops.diffaug_draw(1234, 0, 6, 0, 1, n, S, 7, out=table)
    assert np.array_equal(table[:n].cpu().numpy(), DR.draw(1234, 0, 6, 0, 1, n, S, 7)) and bool((table[n:] == -7).all())


# ---- 2. geometry-only policies: copies -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("n", BATCHES)
def test_geometry_policies_are_bitwise_the_reference(n, S):
    """Forward and backward, policies translation / cutout / both, hand-made and drawn records, the 16-byte path (S = 8, 64) with the base
    shifted by one float onto the 4-byte one, and S = 9."""
    x_np = _patterns((n, 3, S, S), 10 * n + S)
    x_np[0, 0, 0, :4] = (0x7FC00001, 0x7F800000, 0x00000001, -0x00400001)       # a NaN payload, inf, a denormal, a negative NaN
    recs_all = np.concatenate([_hand_records(S), DR.draw(99, 0, 3, 1, 1, 8, S, DR.ALL)])
    moved = 0
    for flags in (DR.TRANSLATION, DR.CUTOUT, DR.TRANSLATION | DR.CUTOUT):
        for recs in _tables(recs_all, n):
            for shift in (0, 1):
                got = _run_op(ops.diffaug_fwd, x_np, recs, flags, shift)
                want = DR.forward(x_np, recs, flags)
                assert np.array_equal(got, want), ("fwd", flags, shift, recs[:, :4].tolist())
                moved += int(not np.array_equal(want, x_np))
                got = _run_op(ops.diffaug_bwd, x_np, recs, flags, shift)
                assert np.array_equal(got, DR.backward(x_np, recs, flags)), ("bwd", flags, shift, recs[:, :4].tolist())
    assert moved > 0
    ident = np.stack([DR.make_record(0, 0, S, S)] * n)                                    # nothing shifted, nothing cut: the identity
    assert np.array_equal(_run_op(ops.diffaug_fwd, x_np, ident, 6), x_np) and np.array_equal(_run_op(ops.diffaug_bwd, x_np, ident, 6), x_np)
    wild = np.stack([DR.make_record(BIG, -BIG - 1, -BIG - 1, BIG, float("nan"), float("inf"), -1.0)] * n)     # factors are not read
    assert (_run_op(ops.diffaug_fwd, x_np, wild, 6) == 0x3F000000).all() and (_run_op(ops.diffaug_bwd, x_np, wild, 6) == 0).all()


# ---- 3. policies with colour ---------------------------------------------------------------------------------------------------------------
def _bound(ref32, ref64):
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    return max(4.0 * e_ref, FLOOR), e_ref


def _colour_records(n, S):
    recs = DR.draw(4321, 0, 9, 0, 1, n, S, DR.ALL)
    if n >= 5:                                               # hand-made rows among the drawn ones: extreme factors, a clipped square
        recs[1] = DR.make_record(DR.T_of(S), -DR.T_of(S), -1, S - 2, 0.25, 2.0, 1.5)
        recs[3] = DR.make_record(-1, 0, S, S, -0.25, 0.0, 0.5)
    return recs


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("n", BATCHES)
def test_colour_policies_against_the_float64_reference(n, S):
    rng = np.random.default_rng(1000 + 10 * n + S)
    x_np = rng.random((n, 3, S, S), dtype=np.float32)
    dz_np = rng.standard_normal((n, 3, S, S)).astype(np.float32)
    recs = _colour_records(n, S)
    for flags in (DR.COLOR, DR.COLOR | DR.TRANSLATION, DR.ALL):
        for op, ref, inp in ((ops.diffaug_fwd, DR.forward, x_np), (ops.diffaug_bwd, DR.backward, dz_np)):
            want = ref(inp.astype(np.float64), recs, flags)
            bound, e_ref = _bound(ref(inp, recs, flags, np.float32), want)
            for shift in (0, 1):
                got = _run_op(op, inp, recs, flags, shift).view(np.float32)
                err = float(np.abs(got.astype(np.float64) - want).max())
                print(f"S {S} n {n} flags {flags} {ref.__name__} shift {shift}: err {err:.3e} e_ref {e_ref:.3e} bound {bound:.3e} "
                      f"max |v| {np.abs(want).max():.2f}")
                assert err <= bound, (flags, ref.__name__, shift, err, bound)
                if shift == 0:
                    first = got
                else:                                        # the statistics do not depend on the alignment class
                    assert np.array_equal(got.view(np.int32), first.view(np.int32))


@pytest.mark.parametrize("S", SIZES)
def test_a_nan_stays_in_its_own_sample(S):
    """A NaN factor, or a NaN pixel (which reaches the sample's mean), in sample 2 of 5: samples 0, 1, 3, 4 are bitwise what they are
    without it, and sample 2 is poisoned wherever it is computed from the image."""
    n = 5
    rng = np.random.default_rng(S)
    x_np = rng.random((n, 3, S, S), dtype=np.float32)
    recs = DR.draw(4321, 0, 9, 0, 1, n, S, DR.ALL)
    recs[2, :4] = (0, 0, S, S)                               # sample 2: nothing shifted, nothing cut
    others = [0, 1, 3, 4]
    for op in (ops.diffaug_fwd, ops.diffaug_bwd):
        clean = _run_op(op, x_np, recs, DR.ALL)
        for col in (4, 5, 6):
            bad = recs.copy()
            bad[2, col] = 0x7FC00000
            got = _run_op(op, x_np, bad, DR.ALL)
            assert np.array_equal(got[others], clean[others]), (op.__name__, col)
            if not (op is ops.diffaug_bwd and col == 4):     # (the backward does not read b)
                assert np.isnan(got[2].view(np.float32)).all(), (op.__name__, col)
        x_bad = x_np.copy()
        x_bad[2, 1, S // 2, 1] = np.nan
        got = _run_op(op, x_bad, recs, DR.ALL)
        assert np.array_equal(got[others], clean[others]) and np.isnan(got[2].view(np.float32)).all(), op.__name__


# ---- 4. grouped forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("flags", [6, 7])
def test_grouped_forms_are_bitwise_the_single_calls(S, flags):
    n, g = 5, 4
    rng = np.random.default_rng(50 + S)
    xs = [torch.from_numpy(rng.random((n, 3, S, S), dtype=np.float32)).to(DEV) for _ in range(g)]
    recs = [ops.diffaug_draw(77, 0, 3, i & 1, i >> 1, n, S, flags, device=DEV) for i in range(g)]
    for single, grouped in ((ops.diffaug_fwd, ops.diffaug_fwd_g), (ops.diffaug_bwd, ops.diffaug_bwd_g)):
        want = [single(x, flags, r) for x, r in zip(xs, recs)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                        # ... and independent of the stream
            on_side = single(xs[1], flags, recs[1])
        torch.cuda.current_stream().wait_stream(side)
        got = grouped(xs, flags, recs)
        again = grouped(xs, flags, recs)
        pair = grouped(xs[2:], flags, recs[2:])
        torch.cuda.synchronize()
        for i in range(g):
            assert torch.equal(got[i].view(torch.int32), want[i].view(torch.int32)), (single.__name__, i)
            assert torch.equal(again[i].view(torch.int32), got[i].view(torch.int32)), (single.__name__, i)
        assert torch.equal(on_side.view(torch.int32), want[1].view(torch.int32))
        assert torch.equal(pair[0].view(torch.int32), want[2].view(torch.int32)) and torch.equal(pair[1].view(torch.int32), want[3].view(torch.int32))
        assert len({int(t.view(torch.int32).sum()) for t in want}) == g                   # four different problems


# ---- 4b. past the grid caps ------------------------------------------------------------------------------------------------------------------
UNWRITTEN = 0x7FC0DEAD                     # a NaN pattern no kernel produces: what the outputs of the tests below start as


def _past_cap_records(n, S, flags, dom):
    """A drawn table with the hand-made records cycled through every fourth row (their geometry; the drawn factors stay)."""
    recs = ops.diffaug_draw(4321, 0, 9, dom & 1, dom >> 1, n, S, flags, device=DEV).cpu().numpy().copy()
    hand = _hand_records(S)
    rows = np.arange(1, n, 4)
    recs[rows, :4] = hand[np.arange(len(rows)) % len(hand), :4]
    return recs, len(hand)


@pytest.mark.parametrize("flags", [6, 7])
@pytest.mark.parametrize("groups,n,S", DR.APPLY_PAST_CAP)
def test_apply_kernel_past_its_per_sample_cap(groups, n, S, flags):
    """More 256-unit blocks wanted per sample than 4096 / (groups n) allows: every block of diffaug_apply_kernel strides.  Forward and
    backward, outputs that start as NaN between sentinel bands.  The launch equals, bit for bit, launches of at most 256 samples (which
    do not stride) with the same rows of the record table; and chosen samples -- the first and last of every group, records that shift
    by a multiple of 4 and by another amount -- pass the file's reference check: bitwise without colour, the float64 criterion with."""
    want, launched = DR.apply_grid(groups, n, S)
    assert want > launched and launched == max(1, 4096 // (groups * n)), (want, launched)
    assert DR.apply_grid(1, DR.APPLY_CHUNK, S)[0] == DR.apply_grid(1, DR.APPLY_CHUNK, S)[1] == want    # the chunks do not stride
    rng = np.random.default_rng(7 * n + S + flags)
    if flags & DR.COLOR:
        data = [(rng.random((n, 3, S, S), dtype=np.float32), rng.standard_normal((n, 3, S, S)).astype(np.float32)) for _ in range(groups)]
    else:
        data = [(_patterns((n, 3, S, S), 10 * n + S + g),) * 2 for g in range(groups)]
    tabs = [_past_cap_records(n, S, flags, g) for g in range(groups)]
    recs_np, n_hand = [t[0] for t in tabs], tabs[0][1]
    recs = [torch.from_numpy(r).to(DEV) for r in recs_np]
    sel = sorted({0, 1, 2, 3, n - 3, n - 2, n - 1} | {4 * h + 1 for h in range(n_hand - 5, n_hand)})      # the last five hand rows shift by 4, -8, 3, -5, 8
    assert len(sel) >= 8 and sel[-1] == n - 1
    tx = recs_np[0][sel, 0]
    assert ((tx % 4 == 0) & (tx != 0) & (abs(tx) < S)).any() and ((tx % 4 != 0) & (abs(tx) < S)).any()
    for k, (single, grouped, ref) in enumerate(((ops.diffaug_fwd, ops.diffaug_fwd_g, DR.forward), (ops.diffaug_bwd, ops.diffaug_bwd_g, DR.backward))):
        ins = [_Banded(d[k]) for d in data]
        outs = [_Banded(np.full((n, 3, S, S), UNWRITTEN, dtype=np.int32)) for _ in range(groups)]
        assert all(b.view().data_ptr() % 16 == 0 for b in ins + outs)
        kept = [b.buf.clone() for b in ins]
        if groups > 1:
            grouped([b.view() for b in ins], flags, recs, outs=[b.view() for b in outs])
        else:
            single(ins[0].view(), flags, recs[0], out=outs[0].view())
        for g in range(groups):
            assert torch.equal(ins[g].buf, kept[g]), "the input was written"
            assert ins[g].bands_intact() and outs[g].bands_intact()
            got_dev = outs[g].view().view(torch.int32)
            for lo in range(0, n, DR.APPLY_CHUNK):
                part = single(ins[g].view()[lo:lo + DR.APPLY_CHUNK], flags, recs[g][lo:lo + DR.APPLY_CHUNK])
                assert torch.equal(part.view(torch.int32), got_dev[lo:lo + DR.APPLY_CHUNK]), (ref.__name__, g, lo)
            got = got_dev[sel].cpu().numpy()
            inp = data[g][k][sel]
            if not flags & DR.COLOR:
                assert np.array_equal(got, ref(inp, recs_np[g][sel], flags)), (ref.__name__, g)
                continue
            wanted = ref(inp.astype(np.float64), recs_np[g][sel], flags)
            bound, e_ref = _bound(ref(inp, recs_np[g][sel], flags, np.float32), wanted)
            err = float(np.abs(got.view(np.float32).astype(np.float64) - wanted).max())
            print(f"groups {groups} n {n} S {S} {ref.__name__} group {g}: err {err:.3e} e_ref {e_ref:.3e} bound {bound:.3e}")
            assert err <= bound, (ref.__name__, g, err, bound)


@pytest.mark.parametrize("n,S", DR.STATS_PARTITIONS)
def test_statistics_partition_at_and_past_its_cap(n, S):
    """diffaug_stats_kernel with 4, 6, exactly 64, and more than 64 chunks wanted per sample (capped: a thread then takes more trips over
    its chunk), in the 16-byte and the scalar form; the apply kernel's tree over up to 64 partials.  Colour alone and the whole policy,
    forward and backward, against float64.  The records shift and cut at the ends of their ranges, so the backward's "sum of g over
    its sources" mask changes inside chunks and across their boundaries."""
    parts, chunk = DR.stats_partition(S)
    E, T, cs = 3 * S * S, DR.T_of(S), DR.cs_of(S)
    assert (parts, chunk) == {100: (4, 7500), 128: (6, 8192), 416: (64, 8112), 418: (64, 8192), 420: (64, 8272), 512: (64, 12288)}[S]
    assert (parts - 1) * chunk < E <= parts * chunk and (S % 4 == 0) != (S == 418)
    assert (-(-E // DR.DA_PART_ELEMS) > 64) == (S in (420, 512)) and (S != 416 or (-(-E // DR.DA_PART_ELEMS) == 64 and 64 * chunk == E))
    assert S != 418 or E - 63 * chunk == 8076
    lo, hi = -(cs // 2), S - cs % 2 - cs // 2                     # the ends of the cut square's range (dg_diffaug_draw)
    recs = np.stack([DR.make_record(T, -T, lo, hi, 0.25, 2.0, 1.5), DR.make_record(-T, T, hi, lo, -0.25, 0.0, 0.5)])[:n]
    rng = np.random.default_rng(1000 + 10 * n + S)
    x_np = rng.random((n, 3, S, S), dtype=np.float32)
    dz_np = rng.standard_normal((n, 3, S, S)).astype(np.float32)
    for flags in (DR.COLOR, DR.ALL):
        for op, ref, inp in ((ops.diffaug_fwd, DR.forward, x_np), (ops.diffaug_bwd, DR.backward, dz_np)):
            want = ref(inp.astype(np.float64), recs, flags)
            bound, e_ref = _bound(ref(inp, recs, flags, np.float32), want)
            for shift in (0, 1):
                got = _run_op(op, inp, recs, flags, shift, fill=UNWRITTEN).view(np.float32)
                err = float(np.abs(got.astype(np.float64) - want).max())
                print(f"S {S} n {n} parts {parts} chunk {chunk} flags {flags} {ref.__name__} shift {shift}: err {err:.3e} e_ref {e_ref:.3e} "
                      f"bound {bound:.3e}")
                assert err <= bound, (flags, ref.__name__, shift, err, bound)
                if shift == 0:
                    first = got
                else:                                        # the statistics do not depend on the alignment class
                    assert np.array_equal(got.view(np.int32), first.view(np.int32))


def test_ops_wrappers_refuse_what_the_kernels_cannot_take():
    x = torch.zeros((4, 3, 8, 8), device=DEV)
    recs = torch.zeros((4, 8), dtype=torch.int32, device=DEV)
    for bad in (recs.float(), recs[:3], recs.cpu(), torch.zeros((4, 4), dtype=torch.int32, device=DEV)):
        with pytest.raises(_lib.DiscoganHipError, match="record table"):
            ops.diffaug_fwd(x, 7, bad)
    with pytest.raises(_lib.DiscoganHipError, match=r"\[n,3,S,S\]"):
        ops.diffaug_fwd(torch.zeros((4, 3, 8, 6), device=DEV), 7, recs)
    with pytest.raises(_lib.DiscoganHipError, match="fp32"):
        ops.diffaug_bwd(x.double(), 7, recs)
    with pytest.raises(_lib.DiscoganHipError, match="overlap"):
        ops.diffaug_fwd(x, 7, recs, out=x)
    with pytest.raises(_lib.DiscoganHipError, match="one shape"):
        ops.diffaug_fwd_g([x, x[:2]], 7, [recs, recs])
    with pytest.raises(_lib.DiscoganHipError, match="groups"):
        ops.diffaug_fwd_g([x] * 5, 6, [recs] * 5)
    with pytest.raises(ValueError, match="policy flags"):
        DiffAugment(0, 8, 1, 0, 0, 0, device=DEV)
    aug = DiffAugment(7, 8, 1, 0, 0, 0, device=DEV)
    with pytest.raises(RuntimeError, match="draw"):
        aug.apply(x)
    torch.cuda.synchronize()


# ---- 5. the autograd node ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_diffaugfn_gradients_match_autograd_through_the_published_function(S):
    n = 5
    rng = np.random.default_rng(70 + S)
    x_np = rng.random((n, 3, S, S), dtype=np.float32)
    w_np = rng.standard_normal((n, 3, S, S)).astype(np.float32)
    aug = DiffAugment(DR.ALL, S, seed=1234, rank=2, domain=1, role=1, device=DEV)
    recs = aug.draw(11, n).cpu().numpy()
    assert np.array_equal(recs, DR.draw(1234, 2, 11, 1, 1, n, S, DR.ALL))
    x64 = torch.from_numpy(x_np.astype(np.float64)).requires_grad_(True)
    z64 = DR.published(x64, recs, DR.ALL)
    (z64 * torch.from_numpy(w_np.astype(np.float64))).sum().backward()
    x = torch.from_numpy(x_np).to(DEV).requires_grad_(True)
    z = aug.apply(x)
    (z * torch.from_numpy(w_np).to(DEV)).sum().backward()
    for name, got, want, ref32 in (("z", z.detach(), z64.detach().numpy(), DR.forward(x_np, recs, DR.ALL)),
                                   ("grad", x.grad, x64.grad.numpy(), DR.backward(w_np, recs, DR.ALL))):
        bound, e_ref = _bound(ref32, want)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print(f"S {S} {name}: err {err:.3e} e_ref {e_ref:.3e} bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
    # needs_input_grad: no gradient wanted of the input, no backward launch and no result
    leaf = torch.from_numpy(x_np).to(DEV)
    assert not aug.apply(leaf).requires_grad
    a, b = apply_group([aug, aug], [x, leaf])
    assert a.requires_grad and torch.equal(a.detach(), z.detach()) and torch.equal(b, z.detach())
    x.grad = None
    (a * 2.0 + b).sum().backward()
    assert torch.equal(x.grad, ops.diffaug_bwd(torch.full_like(x, 2.0), DR.ALL, aug.recs))


# ---- trainer runs shared by the cases below --------------------------------------------------------------------------------------------
S_T, N_T, P_T = 64, 4, 3
POLICY = "color,translation,cutout"
_RUNS = {}
_NAMES = (("A", 0, 0), ("BA", 0, 1), ("B", 1, 0), ("AB", 1, 1))          # dis_inputs key, domain, role


def _snapshot(tr):
    tr.finish()
    torch.cuda.synchronize()
    snap = {f"{side}.{name}": getattr(opt, name).cpu().clone() for side, opt in (("gen", tr.optim_gen), ("dis", tr.optim_dis))
            for name in ("flat_p", "exp_avg", "exp_avg_sq")}
    for k, net in tr.nets.items():
        for name, buf in net.named_buffers():
            snap[f"{k}.{name}"] = buf.detach().cpu().clone()
    return snap


def _differ(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in sorted(a) if not torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                                    b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])]


def _run(key, iters=6, policy=POLICY, first=0, state=None, **kw):
    """Iterations ``first .. iters - 1`` of one trainer on one fixed batch: a snapshot (weights, Adam moments, BatchNorm buffers) and the
    training state after the last, and per iteration what the discriminators were given.  One run per key for the module."""
    if key not in _RUNS:
        A, B = synthetic_batch(N_T, S_T, 5, DEV)
        tr = DiscoGANTrainer(default_args(image_pool=P_T, diffaug=policy), device=DEV, image_size=S_T, seed=1234, **kw)
        if state is not None:
            assert tr.load_train_state(state) == first
        seen = {}
        for i in range(first, iters):
            out = tr.train_iteration(A, B, i)
            torch.cuda.synchronize()
            if out.dis_inputs is None:
                seen[i] = None
            else:
                assert sorted(out.dis_inputs) == ["A", "AB", "B", "BA"]
                seen[i] = dict(src=dict(A=A.cpu(), B=B.cpu(), BA=out.BA_seen.detach().cpu().clone(), AB=out.AB_seen.detach().cpu().clone()),
                               got={k: v.detach().cpu().clone() for k, v in out.dis_inputs.items()})
        _RUNS[key] = dict(seen=seen, last=_snapshot(tr), state=tr.train_state(iters), grouped=bool(tr.group_launch), keys=sorted(vars(out)))
        del tr
    return _RUNS[key]


def _check_inputs(run, policy, iters):
    """Every iteration's four discriminator inputs are the reference applied to A, BA_seen, B, AB_seen with the tables of
    (seed 1234, rank 0, iteration, domain, role): bitwise without colour, else within the bound."""
    flags = DR.COLOR * ("color" in policy) | DR.TRANSLATION * ("translation" in policy) | DR.CUTOUT * ("cutout" in policy)
    for i in iters:
        for name, dom, role in _NAMES:
            recs = DR.draw(1234, 0, i, dom, role, N_T, S_T, flags)
            src, got = run["seen"][i]["src"][name].numpy(), run["seen"][i]["got"][name].numpy()
            if not flags & DR.COLOR:
                assert np.array_equal(got.view(np.int32), DR.forward(src.view(np.int32), recs, flags)), (i, name)
                continue
            want = DR.forward(src.astype(np.float64), recs, flags)
            bound, e_ref = _bound(DR.forward(src, recs, flags), want)
            err = float(np.abs(got.astype(np.float64) - want).max())
            assert err <= bound, (i, name, err, bound)


# ---- 6. the trainer ------------------------------------------------------------------------------------------------------------------------
def test_trainer_gives_the_discriminators_the_reference_batches():
    """64 px, batch 4, pool of 3 (D-step 3 swaps), exact fp32; the default schedule at this size is the grouped one, the other is forced."""
    for key, kw in (("grouped", {}), ("chain", dict(group_launch=False))):
        run = _run(key, **kw)
        assert run["grouped"] == (key == "grouped")
        _check_inputs(run, POLICY, range(6))
        assert all(bool(torch.isfinite(v).all()) for v in run["last"].values() if v.dtype == torch.float32)
    pooled = _run("grouped")["seen"][3]["src"]
    assert not torch.equal(pooled["BA"], _run("grouped")["seen"][3]["got"]["BA"])
    geo = _run("geometry", policy="cutout,translation")
    _check_inputs(geo, "translation,cutout", range(6))
    assert _differ(geo["last"], _run("grouped")["last"])


def test_diffaug_off_is_the_step_without_the_feature():
    """``diffaug=""`` (and "none", and arguments that do not carry the attribute) build no transform, allocate no table, return
    ``dis_inputs is None`` and the same set of outputs, and step bitwise alike; switched on, the weights part from that run."""
    off = _run("off", policy="")
    none = _run("off_none", policy="none")
    assert all(v is None for v in off["seen"].values()) and all(v is None for v in none["seen"].values())
    assert _differ(off["last"], none["last"]) == []
    assert off["keys"] == _run("grouped")["keys"] and "dis_inputs" in off["keys"]
    A, B = synthetic_batch(N_T, S_T, 5, DEV)
    args = default_args(image_pool=P_T)
    del args.diffaug
    tr = DiscoGANTrainer(args, device=DEV, image_size=S_T, seed=1234)
    assert tr.aug_A is None and tr.aug_BA is None and tr.aug_B is None and tr.aug_AB is None and tr.diffaug_flags == 0
    for i in range(6):
        out = tr.train_iteration(A, B, i)
        assert out.dis_inputs is None
    assert _differ(_snapshot(tr), off["last"]) == []
    changed = _differ(_run("grouped")["last"], off["last"])
    assert "dis.flat_p" in changed and "gen.flat_p" in changed
    with pytest.raises(ValueError, match="unknown policy"):
        DiscoGANTrainer(default_args(diffaug="color,blur"), device=DEV, image_size=S_T, seed=1234)


@pytest.mark.parametrize("name,kw", [
    ("grouped", {}),
    ("chain", dict(group_launch=False)),
    ("f32x3_planes", dict(mfma_dtype="f32x3", x3_planes=True)),
])
def test_graph_replay_equals_eager_dispatch(name, kw):
    """Six iterations (graphs captured at iterations 3 and 4, replayed at 5): weights, Adam moments, BatchNorm buffers and the
    discriminators' inputs bitwise."""
    eager = _run(name, **kw)
    graph = _run(name + "_graph", use_graph=True, **kw)
    assert _differ(graph["last"], eager["last"]) == []
    for i in range(6):
        for k in ("A", "BA", "B", "AB"):
            assert torch.equal(graph["seen"][i]["got"][k].view(torch.int32), eager["seen"][i]["got"][k].view(torch.int32)), (i, k)
    if name == "f32x3_planes":
        _check_inputs(eager, POLICY, range(6))


def test_two_chain_equals_grouped_with_single_plans():
    chain = _run("chain", group_launch=False)
    single = _run("grouped_single", group_launch=True, group_plan="single")
    assert single["grouped"] and not chain["grouped"]
    assert _differ(single["last"], chain["last"]) == []
    for i in range(6):
        for k in ("A", "BA", "B", "AB"):
            assert torch.equal(single["seen"][i]["got"][k].view(torch.int32), chain["seen"][i]["got"][k].view(torch.int32)), (i, k)


def test_resume_continues_bitwise(tmp_path):
    """Saved at iteration 3 (three iterations run), resumed, finished: bitwise the uninterrupted run -- the draw is keyed on the
    iteration, and the state holds nothing of the feature."""
    whole = _run("grouped")
    torch.save(_run("head3", iters=3)["state"], tmp_path / "state.pth")
    st = torch.load(tmp_path / "state.pth")
    assert st["iters"] == 3 and not any("diffaug" in k for k in st)
    tail = _run("resumed", first=3, state=st)
    assert _differ(tail["last"], whole["last"]) == []
    for i in (3, 4, 5):
        for k in ("A", "BA", "B", "AB"):
            assert torch.equal(tail["seen"][i]["got"][k].view(torch.int32), whole["seen"][i]["got"][k].view(torch.int32)), (i, k)


# ---- 7. CLI --------------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_with_diffaug(tmp_path, capsys):
    argv = ["--task_name", "edges2shoes", "--image_size", "64", "--batch_size", "4", "--epochs", "3", "--max_iters", "6",
            "--log_interval", "1", "--data_source", "synthetic", "--synthetic_size", "16", "--image_save_interval", "0",
            "--results_dir", str(tmp_path / "res"), "--models_dir", str(tmp_path / "mod")]
    tr = it_cli.main(argv + ["--diffaug", "translation,cutout"])
    out = capsys.readouterr().out
    assert "differentiable augmentation: translation,cutout on every discriminator input" in out
    assert tr.diffaug_flags == 6 and tr.aug_AB.drawn == 4
    rp, _ = it_cli.train.last_paths
    assert len([ln for ln in open(rp / "training_log.txt").read().splitlines() if ln.startswith("Iter")]) == 6
    for net in (tr.generator_A, tr.generator_B, tr.discriminator_A, tr.discriminator_B):
        assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    with pytest.raises(ValueError, match="diffaug: unknown policy 'sharpen'"):
        it_cli.main(argv + ["--diffaug", "translation,sharpen"])
    assert "differentiable augmentation" not in capsys.readouterr().out
