"""numpy restatement of the training augmentation (include/discogan_hip.h, "training augmentation") -- TEST INFRASTRUCTURE ONLY.

The draw: record j of a batch is a pure function of (seed, rank, iteration, domain 0 = A | 1 = B, j).  All arithmetic modulo 2^64;
``mix`` is the SplitMix64 output function (Steele, Lea & Flood 2014), G = 0x9E3779B97F4A7C15:

    mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
    k = mix(seed + G);   k = mix(k ^ (uint32(rank) << 32 | uint32(domain)));   k = mix(k ^ iteration)
    a = mix(k + G (2j + 1));   b = mix(k + G (2j + 2));   w0 = a >> 32,  w1 = a & 0xFFFFFFFF,  w2 = b >> 32
    flip = w0 >> 31 (0 without FLIP);   ox = (w1 (L - S + 1)) >> 32,  oy = (w2 (L - S + 1)) >> 32 (both 0 without CROP)

The image: ``augment_image`` is, by definition, the oracle's preparation at L, the S x S window at (ox, oy), mirrored when flip.
"""
import numpy as np

from oracle import image_prep_ref as R

FLIP, CROP = 1, 2
_M = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15


def mix(z):
    z &= _M
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M
    z ^= z >> 31
    return z


def draw(seed, rank, iteration, domain, n, S, L, flags):
    """int32 [n, 4] = (ox, oy, flip, 0) per batch position."""
    k = mix((seed & _M) + _G)
    k = mix(k ^ (((rank & 0xFFFFFFFF) << 32) | (domain & 0xFFFFFFFF)))
    k = mix(k ^ (iteration & _M))
    span = L - S + 1
    out = np.zeros((n, 4), dtype=np.int32)
    for j in range(n):
        a, b = mix(k + _G * (2 * j + 1)), mix(k + _G * (2 * j + 2))
        w0, w1, w2 = a >> 32, a & 0xFFFFFFFF, b >> 32
        if flags & CROP:
            out[j, 0], out[j, 1] = (w1 * span) >> 32, (w2 * span) >> 32
        if flags & FLIP:
            out[j, 2] = w0 >> 31
    return out


def window(prepared, S, ox, oy, flip):
    """[..., L, L] -> [..., S, S]: the window at (ox, oy), mirrored left-right when flip."""
    w = prepared[..., oy:oy + S, ox:ox + S]
    return np.ascontiguousarray(w[..., ::-1] if flip else w)


def augment_image(img_u8, domain, S, L, ox, oy, flip):
    """float32 [3, S, S]: R.prepare_image(img, domain, L)[:, oy:oy+S, ox:ox+S], then the flip."""
    return window(R.prepare_image(img_u8, domain, L), S, int(ox), int(oy), bool(flip))


def corner_records(S, L):
    """Five hand-written records that reach every corner of the offset range, mirrored and not."""
    m, mid = L - S, (L - S) // 2
    return np.array([(0, 0, 0, 0), (m, m, 1, 0), (0, m, 1, 0), (m, 0, 0, 0), (mid, mid, 1, 0)], dtype=np.int32)
