"""Image history pool, the parts that need no GPU: the record rule against an independent sequential pool, the statistics of the draw
(the device draw is compared with the numpy one exactly in test_pool_gpu.py), the CLI surface, and the launchers' argument checks."""
import ctypes as C

import numpy as np
import pytest

from discogan_modernized_amd import _lib, trainer
from discogan_modernized_amd import distributed_image_translation as dit
from discogan_modernized_amd import image_translation as it
from tests import pool_ref as PR


@pytest.mark.parametrize("P", [1, 2, 3, 8, 50])
@pytest.mark.parametrize("n", [1, 4, 5, 33])
def test_records_reproduce_the_sequential_pool(P, n):
    """Applying the record table in parallel form (every out from the pool as it was, then the stores) is the in-order ImagePool.query;
    no slot is stored twice, and no slot is read by one record and stored by another."""
    rng = np.random.default_rng(1000 * P + n)
    for filled in sorted({0, max(0, P - 2), P}):
        for trial in range(6):
            seed, rank, domain, iteration = int(rng.integers(0, 1 << 62)), int(rng.integers(0, 8)), trial % 2, int(rng.integers(0, 1 << 40))
            seq = PR.SequentialPool(P, (2,), np.int64, seed, rank, domain)
            seq.slots[:] = rng.integers(0, 1 << 40, seq.slots.shape)
            seq.filled = filled
            before = seq.slots.copy()
            x = rng.integers(0, 1 << 40, (n, 2))
            want = seq.query(x, iteration)
            recs = PR.records(seed, rank, iteration, domain, n, P, filled)
            out, after = PR.apply_records(x, before, recs)
            assert np.array_equal(out, want) and np.array_equal(after, seq.slots), (P, n, filled, recs)
            assert seq.filled == min(P, filled + n)
            stored = recs[recs[:, 1] >= 0, 1]
            assert len(set(stored.tolist())) == len(stored)                                   # only the first toucher stores
            readers = {int(r[1]) for r in recs if r[0] == -1}
            storers = {int(r[1]): j for j, r in enumerate(recs) if r[1] >= 0}
            for j, r in enumerate(recs):                                                      # a slot's reader is its storer
                if r[0] == -1:
                    assert storers[int(r[1])] == j
            assert readers <= set(storers)
            assert not recs[:, 3].any() and recs.dtype == np.int32


def test_draw_statistics():
    """100 000 draws at P = 50 (25 iterations of 4000 positions).  The swap bit is a fair coin: its fraction lies within
    4 sqrt(1 / (4 n)) = 4 sd of 1/2; every slot is hit."""
    P, total = 50, 0
    swaps, counts = 0, np.zeros(P, dtype=np.int64)
    for iteration in range(25):
        d = PR.draws(1234, 0, iteration, 0, 4000, P)
        total += len(d)
        swaps += sum(b for b, _ in d)
        counts += np.bincount([s for _, s in d], minlength=P)
        assert all(0 <= s < P and b in (0, 1) for b, s in d)
    assert total == 100_000 and counts.sum() == total
    assert abs(swaps / total - 0.5) <= 4.0 * np.sqrt(1.0 / (4.0 * total)), swaps / total
    assert counts.min() > 0, counts
    assert PR.draws(1234, 0, 3, 0, 100, P) == PR.draws(1234, 0, 3, 0, 4000, P)[:100]         # position j does not depend on n
    base = PR.draws(1234, 0, 3, 0, 4000, P)
    for other in (PR.draws(1234, 1, 3, 0, 4000, P), PR.draws(1234, 0, 3, 1, 4000, P), PR.draws(1234, 0, 4, 0, 4000, P),
                  PR.draws(1235, 0, 3, 0, 4000, P)):
        assert np.mean([a[0] != b[0] for a, b in zip(base, other)]) > 0.4


def test_pool_key_is_not_the_augmentation_key():
    from tests import augment_ref as AR
    k = AR.mix(AR.mix(AR.mix(1234 + AR._G) ^ ((3 << 32) | 1)) ^ 7)
    assert PR.key(1234, 3, 7, 1) == AR.mix(k ^ 0x706F6F6C) != k


def test_parsers_gain_image_pool_off_by_default():
    for mod in (it, dit):
        assert mod.parse_args([]).image_pool == 0
        assert mod.parse_args(["--image_pool", "50"]).image_pool == 50
    assert trainer.DEFAULTS["image_pool"] == 0
    assert trainer.check_image_pool(0) == 0 and trainer.check_image_pool(50) == 50
    for bad in (-1, 2.5, "8", None, True):
        with pytest.raises(ValueError, match="image_pool"):
            trainer.check_image_pool(bad)


def test_a_negative_image_pool_is_refused_before_the_device_check():
    """``train()`` validates --image_pool like --augment: a ValueError on any machine, ahead of the "no HIP device" RuntimeError."""
    with pytest.raises(ValueError, match="image_pool"):
        it.train(it.parse_args(["--task_name", "edges2shoes", "--image_pool", "-1"]))


def test_launchers_refuse_bad_arguments_before_any_launch():
    """Negative status and a message, nothing launched (no GPU needed); the addresses are non-null dummies, never dereferenced."""
    lib = _lib.load()
    p = C.c_void_p
    x, pool, out, t = p(1 << 20), p(2 << 20), p(3 << 20), p(8192)

    def err():
        return lib.dg_last_error()

    assert lib.dg_pool_draw(1, 0, 0, 0, 4, 8, 0, None, None) == -1 and b"null record table" in err()
    assert lib.dg_pool_draw(1, 0, 0, 0, 4, 8, 0, p(8196), None) == -1 and b"aligned" in err()
    assert lib.dg_pool_draw(1, 0, 0, 0, 4, 0, 0, t, None) == -1 and b"P >= 1" in err()
    assert lib.dg_pool_draw(1, 0, 0, 0, 4, 8, 9, t, None) == -1 and b"filled" in err()
    assert lib.dg_pool_draw(1, 0, 0, 0, 4, 8, -1, t, None) == -1 and b"filled" in err()
    assert lib.dg_pool_draw(1, 0, 0, 0, 0, 8, 0, t, None) == -1 and b"4096" in err()
    assert lib.dg_pool_draw(1, 0, 0, 0, 4097, 8, 0, t, None) == -1 and b"4096" in err()
    assert lib.dg_pool_draw(1, 0, 0, 2, 4, 8, 0, t, None) == -1 and b"domain" in err()
    assert lib.dg_pool_draw(1, -1, 0, 0, 4, 8, 0, t, None) == -1
    assert lib.dg_pool_exchange(x, pool, out, 4, 8, 768, None, None) == -1 and b"null record table" in err()
    assert lib.dg_pool_exchange(None, pool, out, 4, 8, 768, t, None) == -1 and b"null pointer" in err()
    assert lib.dg_pool_exchange(x, pool, out, 4, 8, 768, p(8196), None) == -1 and b"aligned" in err()
    assert lib.dg_pool_exchange(x, pool, out, 4, 0, 768, t, None) == -1
    assert lib.dg_pool_exchange(x, pool, out, 4, 8, 0, t, None) == -1
    assert lib.dg_pool_exchange(x, pool, out, 0, 8, 768, t, None) == -1 and b"4096" in err()
    assert lib.dg_pool_exchange(x, pool, out, 4097, 8, 768, t, None) == -1 and b"4096" in err()
    for a, b, c in ((x, x, out), (x, pool, x), (x, pool, pool), (x, p((1 << 20) + 4 * 768 * 4 - 4), out)):
        assert lib.dg_pool_exchange(a, b, c, 4, 8, 768, t, None) == -1 and b"overlap" in err()
