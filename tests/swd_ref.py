"""Reference for the sliced Wasserstein distance kernels (csrc/swd.hip; include/discogan_hip.h is the definition): every stage restated in
numpy -- float64 for the value, and the same text in plain float32 for the size of an fp32 evaluation's own error -- with the draws in
Python integers.  ``variant`` switches on ONE deliberate mistake, for the test that the bound of the whole chain tells them apart."""
import math

import numpy as np
import torch

MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
LINK = 0x7377640000000000
PATCH, DESC, CH = 7, 147, 49
U = 2.0 ** -24                     # unit roundoff of fp32
# rounding chains counted in the header of csrc/swd.hip
K_DOWN, K_UP, K_PROJ_EXTRA, SORT_THREADS = 10, 10, 3, 1024
W = np.array([1, 4, 6, 4, 1], dtype=np.float64) / 16


def gamma(k, u=U):
    return k * u / (1 - k * u)


def mix(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def level_key(seed, level):
    k = mix((seed + G) & MASK)
    return mix(k ^ (LINK | level))


def draw(seed, level, n, R, P):
    """int32 [n, P, 2] = (oy, ox)"""
    k = level_key(seed, level)
    out = np.empty((n, P, 2), dtype=np.int32)
    for j in range(n):
        for p in range(P):
            q = mix((k + G * (j * P + p + 1)) & MASK)
            out[j, p, 0] = ((q >> 32) * (R - 6)) >> 32
            out[j, p, 1] = ((q & 0xFFFFFFFF) * (R - 6)) >> 32
    return out


def levels(S):
    if S < 16:
        return []
    out = [S]
    while out[-1] % 2 == 0 and out[-1] // 2 >= 16:
        out.append(out[-1] // 2)
    return out


def patches_per_image(n, max_row, patches=128):
    return min(patches, max_row // n)


# ---- pyramid -----------------------------------------------------------------------------------------------------------------------------
def filt(a, w, axis, border="mirror"):
    """5-tap correlation of ``a`` along ``axis`` in a's own dtype.  mirror: -1 -> 1 (numpy pad 'reflect' = scipy 'mirror');
    reflect: -1 -> 0 (numpy 'symmetric' = scipy 'reflect')."""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (2, 2)
    p = np.pad(a, pad, mode="reflect" if border == "mirror" else "symmetric")
    n = a.shape[axis]
    out = np.zeros_like(a)
    for k in range(5):
        out = out + a.dtype.type(w[k]) * np.take(p, np.arange(k, k + n), axis=axis)
    return out


def down(a, border="mirror"):
    return filt(filt(a, W, -1, border), W, -2, border)[..., ::2, ::2]


def up(a, border="mirror"):
    z = np.zeros(a.shape[:-2] + (2 * a.shape[-2], 2 * a.shape[-1]), dtype=a.dtype)
    z[..., ::2, ::2] = a
    return filt(filt(z, 2 * W, -1, border), 2 * W, -2, border)


def pyramid(x, border="mirror"):
    """[n,3,S,S] -> list of Laplacian levels, in x's dtype (float64: the value; float32: a plain fp32 evaluation)."""
    Rs = levels(x.shape[-1])
    g = [x]
    for _ in Rs[1:]:
        g.append(down(g[-1], border))
    return [g[l] - up(g[l + 1], border) for l in range(len(Rs) - 1)] + [g[-1]]


def pyramid_bound(x):
    """Per level the element bound of the header's chain: gamma((l + 1) K_DOWN + K_UP + 1) (mag(G_l) + up(mag(G_{l+1}))); the last level
    gamma(l K_DOWN) mag(G_l) (0 for a one-level pyramid: a bit copy)."""
    Rs = levels(x.shape[-1])
    m = [np.abs(x.astype(np.float64))]
    for _ in Rs[1:]:
        m.append(down(m[-1]))
    out = [gamma((l + 1) * K_DOWN + K_UP + 1) * (m[l] + up(m[l + 1])) for l in range(len(Rs) - 1)]
    return out + [gamma((len(Rs) - 1) * K_DOWN) * m[-1]]


# ---- the host's launch arithmetic (csrc/swd.hip), restated for the tests past the grid caps ----------------------------------------------
PYR_MAX_BLOCKS, PYR_THREADS = 16384, 256       # SWD_PYR_MAX_BLOCKS; one item per thread and trip
DESC_PER_BLOCK, SUM_THREADS = 32, 256          # SWD_DESC_PER_BLOCK; swd_sum_parts: thread t adds the partials t, t + 256, ...
# (n, S): swd_lap_kernel<4> at level 0; swd_lap_kernel<1> and swd_down_kernel<1>; swd_down_kernel<4> (and four trips of swd_lap_kernel<4>)
PYRAMID_PAST_CAP = ((1366, 64), (4840, 34), (5462, 64))
PYRAMID_CHUNK = 512                            # images per launch that does not stride at these sizes
STATS_PAST_256 = ((257, 32), (256, 128))       # (n, P) at R = 16: 257 and 1024 block partials


def pyramid_launches(n, S):
    """dg_lap_pyramid's launches for 16-byte aligned buffers: [(kernel, V, level, items, items per image)] in launch order."""
    out = []
    for l, R in enumerate(levels(S)[:-1]):
        Ro = R // 2
        v = 4 if Ro % 4 == 0 else 1
        out.append(("down", v, l, n * 3 * Ro * (Ro // v), 3 * Ro * (Ro // v)))
        v = 4 if R % 4 == 0 else 1
        out.append(("lap", v, l, n * 3 * R * (R // v), 3 * R * (R // v)))
    return out


def pyramid_boundary_images(n, S):
    """The first and last image and, for every launch that strides, the images that hold the items either side of each trip boundary
    (with their neighbours)."""
    cap = PYR_MAX_BLOCKS * PYR_THREADS
    at = {0, 1, 2, n // 2, n - 3, n - 2, n - 1}
    for _, _, _, items, per in pyramid_launches(n, S):
        for k in range(1, (items - 1) // cap + 1):
            at |= {(k * cap - 1) // per - 1, (k * cap - 1) // per, (k * cap) // per, (k * cap) // per + 1}
    return sorted(i for i in at if 0 <= i < n)


# ---- descriptors, statistics, projection ----------------------------------------------------------------------------------------------------
def gather(level, recs):
    """[n,3,R,R], int [n,P,2] -> [n P, 147] ordered [channel][dy][dx]; offsets clamped to [0, R - 7] as the kernel does"""
    n, _, R, _ = level.shape
    P = recs.shape[1]
    out = np.empty((n * P, DESC), dtype=level.dtype)
    for j in range(n):
        for p in range(P):
            oy, ox = (min(max(int(v), 0), R - PATCH) for v in recs[j, p])
            out[j * P + p] = level[j, :, oy:oy + PATCH, ox:ox + PATCH].reshape(-1)
    return out


def stats(desc):
    """[M,147] -> (mean [3], std [3]) in desc's dtype (population standard deviation)"""
    d = desc.reshape(-1, 3, CH)
    return d.mean(axis=(0, 2)), d.std(axis=(0, 2))


def normalise(desc):
    mean, std = stats(desc)
    d = desc.reshape(-1, 3, CH)
    safe = np.where(std == 0, 1, std)
    out = np.where(std[None, :, None] == 0, 0, (d - mean[None, :, None]) / safe[None, :, None])
    return out.reshape(-1, DESC).astype(desc.dtype)


def directions(seed, D=512):
    """float32 [D,147] as evaluate.make_swd_directions draws them"""
    g = torch.Generator().manual_seed(int(seed))
    v = torch.randn((D, DESC), generator=g, dtype=torch.float64).numpy()
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def project(xhat, dirs):
    """[M,147], [D,147] -> [D,M] in xhat's dtype"""
    return (xhat @ dirs.astype(xhat.dtype).T).T.copy()


def project_bound(xhat64, dirs):
    """[D,M]: gamma(147 + c) sum_k |xhat_k| |dir_k|"""
    return gamma(DESC + K_PROJ_EXTRA) * (np.abs(xhat64) @ np.abs(dirs.astype(np.float64)).T).T


def row_distance(a, b_sorted):
    """[D,M] (unsorted), [D,M] sorted -> float64 [D] mean_i |a_(i) - b_(i)|"""
    return np.abs(np.sort(a.astype(np.float64), axis=1) - b_sorted.astype(np.float64)).mean(axis=1)


def distance_gamma(M):
    return gamma(-(-M // SORT_THREADS) + 2)


# ---- the whole chain --------------------------------------------------------------------------------------------------------------------------
def projections(x, seed, P, dirs, dtype=np.float64, variant=None):
    """All levels' [D,M] projections of one set, evaluated in ``dtype`` throughout.  variant: None or one deliberate mistake --
    'reflect' borders, positions 'shift'ed by one, channels 'roll'ed, 'nonorm' (no normalisation), 'fewer' (P - 1 patches)."""
    x = np.asarray(x, dtype=dtype)
    n, S = x.shape[0], x.shape[-1]
    out = []
    for l, lev in enumerate(pyramid(x, "reflect" if variant == "reflect" else "mirror")):
        R = lev.shape[-1]
        recs = draw(seed, l, n, R, P - 1 if variant == "fewer" else P)
        if variant == "shift":
            recs = np.minimum(recs + 1, R - PATCH)
        if variant == "roll":
            lev = np.roll(lev, 1, axis=1)
        d = gather(lev, recs)
        out.append(project(d if variant == "nonorm" else normalise(d), dirs))
    return out


def swd_levels_from(pa, pb):
    return [1000.0 * float(np.abs(np.sort(a.astype(np.float64), axis=1) - np.sort(b.astype(np.float64), axis=1)).mean()) for a, b in zip(pa, pb)]


def swd(x, y, seed, P, dirs, variant=None):
    """float64 reference: list of SWD_l"""
    return swd_levels_from(projections(x, seed, P, dirs, np.float64, variant), projections(y, seed, P, dirs, np.float64, variant))


def chain_bound(x, y, seed, P, dirs, margin=8.0):
    """Per level 1000 * 2 eps, eps = margin x the sup-norm distance between the plain-fp32 and the float64 evaluation of the whole chain
    (pyramid included) over both sets: sorting is 1-Lipschitz in the sup norm, so projections within eps give distances within 2 eps."""
    out = []
    per_set = []
    for s in (x, y):
        p64, p32 = projections(s, seed, P, dirs, np.float64), projections(s, seed, P, dirs, np.float32)
        per_set.append([float(np.abs(a - b.astype(np.float64)).max()) for a, b in zip(p64, p32)])
    for ex, ey in zip(*per_set):
        out.append(1000.0 * 2.0 * margin * max(ex, ey))
    return out


# ---- test sets ---------------------------------------------------------------------------------------------------------------------------------
def make_set(kind, n, S, seed):
    """float32 [n,3,S,S] in [0,1]: 'indep' uniform noise, 'smooth' low-frequency waves, 'mixed' their half-and-half blend,
    'flat' one constant per channel (0.25, 0.5, 0.75: sums of them are exact)."""
    rng = np.random.default_rng(seed)
    noise = rng.random((n, 3, S, S))
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    f = rng.uniform(0.5, 2.5, (n, 3, 2))
    ph = rng.uniform(0, 2 * math.pi, (n, 3, 2))
    smooth = 0.5 + 0.25 * (np.sin(2 * math.pi * f[..., 0, None, None] * yy / S + ph[..., 0, None, None])
                           + np.cos(2 * math.pi * f[..., 1, None, None] * xx / S + ph[..., 1, None, None]))
    if kind == "indep":
        a = noise
    elif kind == "smooth":
        a = smooth
    elif kind == "mixed":
        a = 0.5 * noise + 0.5 * smooth
    elif kind == "flat":
        a = np.broadcast_to(np.array([0.25, 0.5, 0.75]).reshape(1, 3, 1, 1), (n, 3, S, S))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, dtype=np.float32)
