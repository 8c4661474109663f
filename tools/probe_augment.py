#!/usr/bin/env python3
"""What the training augmentation costs (tuning aid; the numbers quoted in DESIGN.md come from here).

(a) per launch, device events over repeated launches, three legs alternating in one run: dg_image_prep at S (no augmentation), the fused
    dg_image_prep_aug (records drawn by dg_augment_draw for flip,crop), and the two-step form it replaces -- dg_image_prep at L into a float
    batch, then window + mirror with torch ops.  The two-step leg is given its CHEAPEST shape: one window and one mirror for the whole batch
    (a slice, a flip, one copy kernel); per-sample windows would need a gather or a launch per sample on top.
    Sources: uint8 [32,256,512,3] 'B' -> S = 512 and [256,256,512,3] 'B' -> S = 64, L = round(1.125 S).
(b) ms per iteration of the 512 px / batch 32 f32x3 step fed from resident synthetic float data (the CLI's _ResidentData), augmentation off
    against flip,crop (dg_augment_draw + dg_augment_f32 per domain and batch): ONE trainer, alternating rounds, whole D,G,G cycles per timed
    window, host clock around a device synchronise.

    python tools/probe_augment.py [--out FILE] [--image_size 512] [--batch 32] [--rounds 4] [--cycles 2] [--skip_step]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from discogan_modernized_amd import dataset as ds  # noqa: E402
from discogan_modernized_amd import image_translation as it  # noqa: E402
from discogan_modernized_amd import ops  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args  # noqa: E402
from tools.bench_ops import timeit  # noqa: E402

DEV = "cuda"
FLAGS = ds.parse_augment("flip,crop")


def kernel_times(n, S, say, reps=3, iters=20):
    L = ds.augment_size(S, FLAGS)
    src = torch.randint(0, 256, (n, 256, 512, 3), dtype=torch.uint8, device=DEV)
    out = torch.empty((n, 3, S, S), device=DEV)
    full = torch.empty((n, 3, L, L), device=DEV)
    recs = ops.augment_draw(1234, 0, 0, 1, n, S, L, FLAGS, device=DEV)
    ox = oy = (L - S) // 2

    def two_step():
        ds.prepare_batch(src, "B", L, out=full)
        out.copy_(full[:, :, oy:oy + S, ox:ox + S].flip(3))

    legs = (("prep", lambda: ds.prepare_batch(src, "B", S, out=out)),
            ("fused", lambda: ds.prepare_batch(src, "B", S, out=out, aug=(L, recs, None))),
            ("two_step", two_step),
            ("draw", lambda: ops.augment_draw(1234, 0, 0, 1, n, S, L, FLAGS, out=recs)))
    rows = []
    for rep in range(reps):                                  # alternating: the legs see the same box in the same minute
        rows.append({name: timeit(fn, iters=iters) for name, fn in legs})
        say(f"  rep {rep}: " + "  ".join(f"{name} {rows[-1][name] * 1e3:.1f} us" for name, _ in legs))
    med = {name: statistics.median(r[name] for r in rows) for name, _ in legs}
    say(f"(a) uint8 [{n},256,512,3] 'B' -> S = {S}, L = {L}; medians of {reps} x {iters} launches: dg_image_prep {med['prep'] * 1e3:.1f} us; "
        f"dg_image_prep_aug {med['fused'] * 1e3:.1f} us; two-step (dg_image_prep at L + slice/flip copy) {med['two_step'] * 1e3:.1f} us; "
        f"dg_augment_draw {med['draw'] * 1e3:.1f} us; fused / two-step = {med['fused'] / med['two_step']:.2f}, "
        f"fused / plain = {med['fused'] / med['prep']:.2f}")
    return med


def step_times(size, batch, rounds, cycles, say, images=64):
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=size, seed=1234, use_graph=True, mfma_dtype="f32x3")
    g = torch.Generator().manual_seed(1000)
    A = torch.rand(images, 3, size, size, generator=g).to(DEV)
    B = torch.rand(images, 3, size, size, generator=g).to(DEV)
    aug = ds.Augment(seed=1234, rank=0, flags=FLAGS, scale=1.125, first_iteration=0)
    legs = {"off": it._ResidentData(A, B), "aug": it._ResidentData(A, B, augment=aug, image_size=size)}
    gp = torch.Generator().manual_seed(7)
    state = dict(it=0)

    def run(name, ncycles):
        n = 3 * ncycles
        batches = [(torch.randperm(images, generator=gp)[:batch].to(DEV), torch.randperm(images, generator=gp)[:batch].to(DEV)) for _ in range(n)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a, b in legs[name].epoch(batches, 0, state["it"]):
            tr.train_iteration(a, b, state["it"], need_losses=True)
            state["it"] += 1
        tr.finish()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    run("off", 3)                                            # eager first cycle, graph capture in the second, one replayed cycle
    run("aug", 1)
    ms = {k: [] for k in legs}
    for r in range(rounds):
        for name in (("off", "aug") if r % 2 == 0 else ("aug", "off")):
            ms[name].append(run(name, cycles))
        say(f"  round {r}: off {ms['off'][-1]:.2f} ms/iteration  flip,crop {ms['aug'][-1]:.2f} ms/iteration")
    off, on = statistics.median(ms["off"]), statistics.median(ms["aug"])
    say(f"(b) {size} px / batch {batch} f32x3, hipGraph replay, resident float data, {rounds} alternating rounds of {cycles} D,G,G cycles, median ms "
        f"per iteration: augmentation off: {off:.2f} (spread {min(ms['off']):.2f}-{max(ms['off']):.2f}); flip,crop: {on:.2f} "
        f"(spread {min(ms['aug']):.2f}-{max(ms['aug']):.2f}); difference {on - off:+.2f} ms = {100 * (on - off) / off:+.2f} % "
        f"({batch / off * 1e3:.1f} -> {batch / on * 1e3:.1f} images/s)")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the report lines to this file")
    ap.add_argument("--image_size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
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

    say(f"tools/probe_augment.py on {torch.cuda.get_device_name(0)}")
    if not a.skip_step:
        step_times(a.image_size, a.batch, a.rounds, a.cycles, say)
        torch.cuda.empty_cache()
    worst = 0.0
    for n, S in ((32, 512), (256, 64)):
        med = kernel_times(n, S, say)
        worst = max(worst, med["fused"] / med["two_step"])
    say(f"fused no slower than the two-step form in this run: {'yes' if worst <= 1.0 else 'NO'} (worst ratio {worst:.2f})")


if __name__ == "__main__":
    main()
