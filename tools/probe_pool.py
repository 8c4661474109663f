#!/usr/bin/env python3
"""What the image history pool costs (tuning aid; the numbers quoted in DESIGN.md come from here).

(a) per launch, device events over repeated launches, legs alternating in one run, at 512 px, n = 32, P = 50 (a pool of 157 MB), in the
    FILL phase (records of an empty pool: 32 inserts) and in the FULL-POOL phase (records of a full pool: swaps and passes):
      fused     dg_pool_exchange on the drawn table;
      two_step  the form it replaces, on the same records, with torch ops in its cheapest shape -- index tensors precomputed outside the
                timed region: out = x.index_select(src), out[readers] = pool.index_select(slots), pool.index_copy_(slots, x.index_select(st));
      swap      dg_swap_flat over as many floats as move the same number of bytes as the fused launch (16 bytes per float);
      draw      dg_pool_draw.
(b) ms per iteration of the 512 px / batch 32 f32x3 step under hipGraph replay, image_pool 0 against 50: two trainers, alternating rounds
    of whole D,G,G cycles, host clock around a device synchronise.

    python tools/probe_pool.py [--out FILE] [--image_size 512] [--batch 32] [--pool 50] [--rounds 4] [--cycles 2] [--skip_step]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from discogan_modernized_amd import ops  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tools.bench_ops import timeit  # noqa: E402

DEV = "cuda"


def kernel_times(n, S, P, filled, say, reps=3, iters=20):
    elems = 3 * S * S
    x = torch.rand((n, 3, S, S), device=DEV)
    pool = torch.rand((P, 3, S, S), device=DEV)
    out = torch.empty_like(x)
    recs = ops.pool_draw(1234, 0, 6, 0, n, P, filled, device=DEV).clone()
    src, slot, st = (recs[:, c].long() for c in range(3))
    pos = torch.arange(n, device=DEV)
    readers, stores = src < 0, slot >= 0
    gather = torch.where(readers, pos, src)
    reader_pos, reader_slot = pos[readers], slot[readers]
    store_slot, store_src = slot[stores], st[stores]
    extra = int((stores & (st != src)).sum())                 # stores whose image is not the one already loaded for `out`
    moved = 4 * elems * (2 * n + int(stores.sum()) + extra)   # bytes the fused launch reads and writes
    flat = torch.rand(2 * (moved // 16), device=DEV)
    a, b = flat[:moved // 16], flat[moved // 16:]

    def two_step():
        torch.index_select(x, 0, gather, out=out)
        if len(reader_pos):
            out.index_copy_(0, reader_pos, pool.index_select(0, reader_slot))
        if len(store_slot):
            pool.index_copy_(0, store_slot, x.index_select(0, store_src))

    legs = (("fused", lambda: ops.pool_exchange(x, pool, recs, out=out)),
            ("two_step", two_step),
            ("swap", lambda: ops.swap_flat(a, b)),
            ("draw", lambda: ops.pool_draw(1234, 0, 6, 0, n, P, filled, out=recs)))
    rows = []
    for rep in range(reps):                                   # alternating: the legs see the same box in the same minute
        rows.append({name: timeit(fn, iters=iters) for name, fn in legs})
        say(f"  rep {rep}: " + "  ".join(f"{name} {rows[-1][name] * 1e3:.1f} us" for name, _ in legs))
    med = {name: statistics.median(r[name] for r in rows) for name, _ in legs}
    phase = "fill" if filled == 0 else "full pool"
    say(f"(a) {phase}: {S} px, n = {n}, P = {P}, filled = {filled}: {int(readers.sum())} slot reads, {int(stores.sum())} stores, "
        f"{moved / 1e6:.1f} MB moved; medians of {reps} x {iters} launches: dg_pool_exchange {med['fused'] * 1e3:.1f} us "
        f"({moved / med['fused'] / 1e9:.2f} TB/s); two-step torch form {med['two_step'] * 1e3:.1f} us; dg_swap_flat on the same bytes "
        f"{med['swap'] * 1e3:.1f} us; dg_pool_draw {med['draw'] * 1e3:.1f} us; fused / two-step = {med['fused'] / med['two_step']:.2f}, "
        f"fused / swap = {med['fused'] / med['swap']:.2f}")
    return med


def step_times(size, batch, P, rounds, cycles, say):
    A, B = synthetic_batch(batch, size, 0, DEV)
    legs = {name: DiscoGANTrainer(default_args(image_pool=p), device=DEV, image_size=size, seed=1234, use_graph=True, mfma_dtype="f32x3")
            for name, p in (("off", 0), ("pool", P))}
    its = {name: 0 for name in legs}

    def run(name, ncycles):
        tr, n = legs[name], 3 * ncycles
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            tr.train_iteration(A, B, its[name], need_losses=True)
            its[name] += 1
        tr.finish()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    warm = max(3, -(-P // batch) + 2)                         # eager cycle, capture cycle, and D-steps enough to fill the pool
    for name in legs:
        run(name, warm)
    ms = {k: [] for k in legs}
    for r in range(rounds):
        for name in (("off", "pool") if r % 2 == 0 else ("pool", "off")):
            ms[name].append(run(name, cycles))
        say(f"  round {r}: off {ms['off'][-1]:.2f} ms/iteration  image_pool {P} {ms['pool'][-1]:.2f} ms/iteration")
    off, on = statistics.median(ms["off"]), statistics.median(ms["pool"])
    say(f"(b) {size} px / batch {batch} f32x3, hipGraph replay, {rounds} alternating rounds of {cycles} D,G,G cycles, median ms per iteration: "
        f"image_pool 0: {off:.2f} (spread {min(ms['off']):.2f}-{max(ms['off']):.2f}); image_pool {P} (full): {on:.2f} "
        f"(spread {min(ms['pool']):.2f}-{max(ms['pool']):.2f}); difference {on - off:+.2f} ms = {100 * (on - off) / off:+.2f} % "
        f"({batch / off * 1e3:.1f} -> {batch / on * 1e3:.1f} images/s)")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the report lines to this file")
    ap.add_argument("--image_size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--pool", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--skip_step", action="store_true", help="only (a)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: nothing here can be measured without one")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    say(f"tools/probe_pool.py on {torch.cuda.get_device_name(0)}")
    worst = 0.0
    for filled in (0, a.pool):
        med = kernel_times(a.batch, a.image_size, a.pool, filled, say)
        worst = max(worst, med["fused"] / med["two_step"])
    say(f"fused no slower than the two-step form in this run: {'yes' if worst <= 1.0 else 'NO'} (worst ratio {worst:.2f})")
    if not a.skip_step:
        torch.cuda.empty_cache()
        step_times(a.image_size, a.batch, a.pool, a.rounds, a.cycles, say)


if __name__ == "__main__":
    main()
