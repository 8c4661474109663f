"""numpy restatement of the differentiable augmentation (include/discogan_hip.h, "differentiable augmentation") -- TEST INFRASTRUCTURE ONLY.

Three independent pieces:
  * ``draw``: the record table of dg_diffaug_draw, eight int32 per sample (tx, ty, cx0, cy0, bits(b), bits(s), bits(c), 0).  Key chain of the
    augmentation draw (tests/augment_ref.py) with one more link, all arithmetic modulo 2^64:
        k = mix(seed + G);  k = mix(k ^ (uint32(rank) << 32 | uint32(domain)));  k = mix(k ^ iteration);  k = mix(k ^ (0x6469666600000000 | role))
        q_i = mix(k + G (4j + i)), i = 1..4;  unit(w) = float32(w >> 8) 2^-24;  range(w, lo, count) = lo + ((w count) >> 32)
        b = (unit(hi q_1) - 0.5) 0.5;  s = 2 unit(lo q_1);  c = unit(hi q_2) + 0.5           (float32 arithmetic)
        tx = range(lo q_2, -T, 2T + 1);  ty = range(hi q_3, -T, 2T + 1);  cx0 = range(lo q_3, 0, S + 1 - cs % 2) - cs // 2;  cy0 from hi q_4
  * ``forward`` / ``backward``: the transform and the adjoint of its linear part, in a chosen float dtype (or, without COLOR, on any
    dtype: a copy).  A stage outside ``flags`` is not evaluated and its record fields are not read.
  * ``published``: the published DiffAugment function (Zhao et al. 2020, DiffAugment_pytorch.py: rand_brightness, rand_saturation,
    rand_contrast, rand_translation via zero pad + gather, rand_cutout via a mask) restated in torch on the CPU, fed the record's random
    numbers instead of torch.rand / torch.randint, applied to x' = 2x - 1 and mapped back by (z' + 1) / 2.
"""
import numpy as np

from tests.augment_ref import _G, _M, mix

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
ALL = 7
LINK = 0x6469666600000000


def T_of(S):
    return int(S / 8 + 0.5)


def cs_of(S):
    return int(S / 2 + 0.5)


def key(seed, rank, iteration, domain, role):
    k = mix((seed & _M) + _G)
    k = mix(k ^ (((rank & 0xFFFFFFFF) << 32) | (domain & 0xFFFFFFFF)))
    k = mix(k ^ (iteration & _M))
    return mix(k ^ (LINK | (role & 0xFFFFFFFF)))


def _unit(w):
    return np.float32(w >> 8) * np.float32(2.0 ** -24)


def _range(w, lo, count):
    return lo + ((w * count) >> 32)


def make_record(tx=0, ty=0, cx0=0, cy0=0, b=0.0, s=1.0, c=1.0):
    rec = np.zeros(8, dtype=np.int32)
    rec[:4] = (tx, ty, cx0, cy0)
    rec[4:7] = np.array([b, s, c], dtype=np.float32).view(np.int32)
    return rec


def factors(recs):
    """float32 [n, 3] = (b, s, c) of a table."""
    return np.ascontiguousarray(recs[:, 4:7]).view(np.float32)


def draw(seed, rank, iteration, domain, role, n, S, flags):
    """int32 [n, 8] per batch position."""
    k = key(seed, rank, iteration, domain, role)
    T, cs = T_of(S), cs_of(S)
    out = np.zeros((n, 8), dtype=np.int32)
    for j in range(n):
        q1, q2, q3, q4 = (mix(k + _G * (4 * j + i)) for i in (1, 2, 3, 4))
        lo = 0xFFFFFFFF
        b, s, c = np.float32(0.0), np.float32(1.0), np.float32(1.0)
        tx = ty = cx0 = cy0 = 0
        if flags & COLOR:
            b = (_unit(q1 >> 32) - np.float32(0.5)) * np.float32(0.5)
            s = np.float32(2.0) * _unit(q1 & lo)
            c = _unit(q2 >> 32) + np.float32(0.5)
        if flags & TRANSLATION:
            tx, ty = _range(q2 & lo, -T, 2 * T + 1), _range(q3 >> 32, -T, 2 * T + 1)
        if flags & CUTOUT:
            count = S + 1 - cs % 2
            cx0, cy0 = _range(q3 & lo, 0, count) - cs // 2, _range(q4 >> 32, 0, count) - cs // 2
        out[j] = make_record(tx, ty, cx0, cy0, b, s, c)
    return out


# ---- the host's launch arithmetic (csrc/diffaug.hip), restated for the tests past the grid caps -----------------------------------------
DA_MAX_PARTS, DA_PART_ELEMS = 64, 8192    # csrc/diffaug.hip
DA_APPLY_BLOCKS = 4096                    # da_run: the apply kernel launches at most 4096 / (groups n) blocks per sample, at least 1
DA_THREADS = 256
# (groups, n, S): scalar form 5 blocks wanted of 3; 16-byte form 4 of 2; grouped 4 of 3; 4096 / 4098 = 0 -> one block, two trips
APPLY_PAST_CAP = ((1, 1025, 34), (1, 1366, 64), (4, 300, 64), (2, 2049, 40))
APPLY_CHUNK = 256                         # samples per launch that does not stride at any of these sizes
# (n, S): 4 parts; 6; exactly 64 that tile E; scalar form, 64 with a short last chunk; 65 wanted, capped; the workload's 96 -> 64
STATS_PARTITIONS = ((2, 100), (2, 128), (2, 416), (2, 418), (2, 420), (1, 512))


def stats_partition(S):
    """(parts, chunk) of da_parts / da_chunk: E = 3 S S values in ``parts`` chunks of ``chunk`` values, a multiple of 4."""
    E = 3 * S * S
    parts = min(-(-E // DA_PART_ELEMS), DA_MAX_PARTS)
    return parts, (-(-E // parts) + 3) // 4 * 4


def apply_grid(groups, n, S, vec=None):
    """(blocks wanted, blocks launched) per sample of the apply kernel; vec: 16-byte units (default: S % 4 == 0)."""
    vec = S % 4 == 0 if vec is None else vec
    units = S * (S // 4) if vec else S * S
    want = -(-units // DA_THREADS)
    return want, min(want, max(1, DA_APPLY_BLOCKS // (groups * n)))


def _geometry(S, rec, flags):
    """(src_y, src_x, keep): output pixel (y, x) reads v(src_y[y], src_x[x]) where keep[y, x]; Python integers, so any int32 is safe."""
    tx, ty = (int(rec[0]), int(rec[1])) if flags & TRANSLATION else (0, 0)
    ys = np.arange(S, dtype=np.int64)
    sy, sx = ys + ty, ys + tx
    keep = ((sy >= 0) & (sy < S))[:, None] & ((sx >= 0) & (sx < S))[None, :]
    if flags & CUTOUT:
        cx0, cy0, cs = int(rec[2]), int(rec[3]), cs_of(S)
        in_y, in_x = (ys >= cy0) & (ys < cy0 + cs), (ys >= cx0) & (ys < cx0 + cs)
        keep = keep & ~(in_y[:, None] & in_x[None, :])
    return np.clip(sy, 0, S - 1), np.clip(sx, 0, S - 1), keep


def _fill(dtype, value):
    if np.issubdtype(dtype, np.floating):
        return dtype.type(value)
    return np.array([value], dtype=np.float32).view(np.int32)[0].astype(dtype)       # bit patterns of float32


def forward(x, recs, flags, dtype=None):
    """z [n, 3, S, S].  With COLOR the arithmetic runs in ``dtype`` (default: x's); without, x may be of any dtype (int32 bit patterns of
    float32 included: the fill is then the pattern of 0.5f)."""
    n, _, S, _ = x.shape
    if flags & COLOR:
        dtype = np.dtype(dtype or x.dtype)
        x = x.astype(dtype)
    z = np.empty_like(x)
    for j in range(n):
        v = x[j]
        if flags & COLOR:
            b, s, c = (dtype.type(f) for f in factors(recs[j:j + 1])[0])
            v = v + b
            m1 = (v[0] + v[1] + v[2]) / dtype.type(3)
            v = (v - m1) * s + m1
            m2 = v.mean(dtype=dtype)
            v = (v - m2) * c + m2
        sy, sx, keep = _geometry(S, recs[j], flags)
        g = v[:, sy][:, :, sx]
        z[j] = np.where(keep[None], g, _fill(x.dtype, 0.5))
    return z


def backward(dz, recs, flags, dtype=None):
    """dx [n, 3, S, S]: the adjoint of forward's linear part."""
    n, _, S, _ = dz.shape
    if flags & COLOR:
        dtype = np.dtype(dtype or dz.dtype)
        dz = dz.astype(dtype)
    dx = np.empty_like(dz)
    zero = _fill(dz.dtype, 0.0)
    for j in range(n):
        # g(q) = dz(q - t) where q - t is inside and not cut: a scatter of the kept outputs to their sources (each source is hit once)
        sy, sx, keep = _geometry(S, recs[j], flags)
        g = np.full_like(dz[j], zero)
        yy, xx = np.nonzero(keep)
        g[:, sy[yy], sx[xx]] = dz[j][:, yy, xx]
        if flags & COLOR:
            b, s, c = (dtype.type(f) for f in factors(recs[j:j + 1])[0])
            one = dtype.type(1)
            cm = (g[0] + g[1] + g[2]) / dtype.type(3)
            g = s * c * g + (one - s) * c * cm + (one - c) * g.mean(dtype=dtype)
        dx[j] = g
    return dx


def published(x, recs, flags):
    """The published function on x' = 2x - 1, mapped back; x: torch CPU tensor [n, 3, S, S] (float64 for the comparisons), differentiable.
    The random numbers are recovered from the record: r_b = 2b + 0.5, r_s = s / 2, r_c = c - 0.5; translation_x/y = ty/tx (the published
    "x" is the row axis); cutout offset = c?0 + cs // 2."""
    import torch
    import torch.nn.functional as F
    n, _, S, _ = x.shape
    f = torch.from_numpy(factors(recs).astype(np.float64)).to(x.dtype)
    r = torch.from_numpy(np.ascontiguousarray(recs[:, :4]).astype(np.int64))
    x = 2 * x - 1
    if flags & COLOR:
        x = x + ((2 * f[:, 0] + 0.5) - 0.5).view(n, 1, 1, 1)                               # rand_brightness
        x_mean = x.mean(dim=1, keepdim=True)                                               # rand_saturation
        x = (x - x_mean) * ((f[:, 1] / 2) * 2).view(n, 1, 1, 1) + x_mean
        x_mean = x.mean(dim=[1, 2, 3], keepdim=True)                                       # rand_contrast
        x = (x - x_mean) * ((f[:, 2] - 0.5) + 0.5).view(n, 1, 1, 1) + x_mean
    if flags & TRANSLATION:                                                                # rand_translation
        translation_x, translation_y = r[:, 1].view(n, 1, 1), r[:, 0].view(n, 1, 1)
        grid_batch, grid_x, grid_y = torch.meshgrid(torch.arange(n), torch.arange(S), torch.arange(S), indexing="ij")
        grid_x = torch.clamp(grid_x + translation_x + 1, 0, S + 1)
        grid_y = torch.clamp(grid_y + translation_y + 1, 0, S + 1)
        x_pad = F.pad(x, [1, 1, 1, 1, 0, 0, 0, 0])
        x = x_pad.permute(0, 2, 3, 1).contiguous()[grid_batch, grid_x, grid_y].permute(0, 3, 1, 2)
    if flags & CUTOUT:                                                                     # rand_cutout
        cs = cs_of(S)
        offset_x, offset_y = (r[:, 3] + cs // 2).view(n, 1, 1), (r[:, 2] + cs // 2).view(n, 1, 1)
        grid_batch, grid_x, grid_y = torch.meshgrid(torch.arange(n), torch.arange(cs), torch.arange(cs), indexing="ij")
        grid_x = torch.clamp(grid_x + offset_x - cs // 2, min=0, max=S - 1)
        grid_y = torch.clamp(grid_y + offset_y - cs // 2, min=0, max=S - 1)
        mask = torch.ones(n, S, S, dtype=x.dtype)
        mask[grid_batch, grid_x, grid_y] = 0
        x = x * mask.unsqueeze(1)
    return (x + 1) / 2
