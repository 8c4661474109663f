"""Host reference of the weight EMA (optim.EMA / dg_ema_update_flat): numpy float32, one correctly rounded IEEE operation after the
other -- numpy fuses nothing, and the kernel is compiled with contraction off, so the two agree bit for bit."""
import numpy as np


def lerp(e, p, w):
    """``e + (p - e) * w`` on float32 arrays: subtract, multiply, add, each rounded to float32."""
    e = np.asarray(e, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    w = np.float32(w)
    d = p - e
    s = d * w
    out = e + s
    assert out.dtype == np.float32
    return out


def recursion(snapshots, decay):
    """The EMA after a list of weight snapshots (one per qualifying generator step): the first is copied, every later one is one lerp
    with ``w = float32(1 - decay)`` (the double difference rounded once, as the C ABI's float argument does)."""
    w = np.float32(float(1.0 - decay))
    e = np.array(snapshots[0], dtype=np.float32, copy=True)
    for p in snapshots[1:]:
        e = lerp(e, p, w)
    return e


def bits(x):
    """int32 view for bitwise comparisons (NaN payloads and the sign of zero included)."""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.int32)
