#!/usr/bin/env python3
"""What gradient control (--grad_clip / --nonfinite_guard / --log_grad_norm) costs (tuning aid; the numbers quoted in DESIGN.md come
from here).

(a) dg_grad_sumsq_partial + dg_grad_clip_finalize (a read-only pass: 4 B/param) at the flat size of the two 512 px generators, next to
    dg_ema_update_flat (12 B/param) and dg_adam_step_flat (28 B/param), host-scaled and device-controlled, at the same size in the same
    run: achieved bytes/s from device events.  Target: the read-only pass streams at >= 0.9 of dg_ema_update_flat's bytes/s.
(b) ms per iteration of the 512 px / batch 32 f32x3 step with the flags off against --grad_clip 1e30 --nonfinite_guard (every
    launch of the feature, no change to any value): two trainers on one box, alternating, whole D,G,G cycles per timed window, host
    clock around a device synchronise.

    python tools/probe_gradclip.py [--out FILE] [--image_size 512] [--batch 32] [--rounds 4] [--cycles 2] [--skip_step]
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


def kernel_rates(n, say):
    p, g, m, v, e = (torch.randn(n, device=DEV) * 0.01 for _ in range(5))
    v.abs_()
    state = torch.zeros(4, device=DEV, dtype=torch.float64)
    ops.adam_advance(state, 2e-4, 0.5, 0.999)
    ws = ops.grad_stats_workspace(DEV)
    ctl = torch.zeros(8, device=DEV, dtype=torch.float64)
    w = float(1.0 - 0.999)

    def stats():
        ops.grad_clip_finalize(ws, ops.grad_sumsq_partial(g, ws, 0), 1.0, 1e30, True, ctl)

    rows = []
    for rep in range(3):                                     # alternating: the kernels see the same box in the same minute
        t_adam = timeit(lambda: ops.adam_step_flat(p, g, m, v, state, 0.5, 0.999, 1e-8, 1e-5), iters=10)
        t_ema = timeit(lambda: ops.ema_update_flat(e, p, w), iters=10)
        t_norm = timeit(stats, iters=10)
        t_adamc = timeit(lambda: ops.adam_step_flat(p, g, m, v, state, 0.5, 0.999, 1e-8, 1e-5, ctl=ctl), iters=10)
        rows.append((t_adam, t_ema, t_norm, t_adamc))
        say(f"  rep {rep}: adam {t_adam:.3f} ms ({28 * n / t_adam / 1e9:.2f} TB/s)  ema {t_ema:.3f} ms ({12 * n / t_ema / 1e9:.2f} TB/s)  "
            f"sumsq+finalize {t_norm:.3f} ms ({4 * n / t_norm / 1e9:.2f} TB/s)  adam with ctl {t_adamc:.3f} ms ({28 * n / t_adamc / 1e9:.2f} TB/s)")
    t_adam, t_ema, t_norm, t_adamc = (statistics.median(r[i] for r in rows) for i in range(4))
    r_ema, r_norm = 12 * n / t_ema / 1e9, 4 * n / t_norm / 1e9
    c = ctl.cpu().tolist()
    assert c[3] == 0.0 and c[2] == 1.0 and c[1] > 0.0
    say(f"(a) n = {n} floats ({n / 1e6:.1f} M), medians of 3 x 10 launches: dg_grad_sumsq_partial + dg_grad_clip_finalize {t_norm:.3f} ms = "
        f"{r_norm:.2f} TB/s (4 B/param); dg_ema_update_flat {t_ema:.3f} ms = {r_ema:.2f} TB/s (12 B/param); ratio of rates "
        f"{r_norm / r_ema:.2f} (target >= 0.90: {'met' if r_norm >= 0.9 * r_ema else 'MISSED'}); dg_adam_step_flat {t_adam:.3f} ms = "
        f"{28 * n / t_adam / 1e9:.2f} TB/s, dg_adam_step_flat with ctl {t_adamc:.3f} ms = {28 * n / t_adamc / 1e9:.2f} TB/s (28 B/param)")


def step_times(size, batch, rounds, cycles, say):
    A, B = synthetic_batch(batch, size, 5, DEV)
    legs = {}
    for name, over in (("off", {}), ("ctl", dict(grad_clip=1e30, nonfinite_guard=True))):
        legs[name] = DiscoGANTrainer(default_args(**over), device=DEV, image_size=size, seed=1234, use_graph=True, mfma_dtype="f32x3")
    it = {k: 0 for k in legs}

    def run(name, ncycles):
        tr = legs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3 * ncycles):
            tr.train_iteration(A, B, it[name], need_losses=True)
            it[name] += 1
        tr.finish()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (3 * ncycles)

    for name in legs:                                        # eager first cycle, graph capture in the second, one replayed cycle
        run(name, 3)
    ms = {k: [] for k in legs}
    for r in range(rounds):
        for name in (("off", "ctl") if r % 2 == 0 else ("ctl", "off")):
            ms[name].append(run(name, cycles))
        say(f"  round {r}: off {ms['off'][-1]:.2f} ms/iteration  grad control {ms['ctl'][-1]:.2f} ms/iteration")
    off, on = statistics.median(ms["off"]), statistics.median(ms["ctl"])
    sg, sd = legs["ctl"].optim_gen.grad_stats(), legs["ctl"].optim_dis.grad_stats()
    assert legs["off"].optim_gen.ctl is None and sg["steps"] + sd["steps"] == it["ctl"] and sg["clipped"] + sg["skipped"] == 0
    say(f"(b) {size} px / batch {batch} f32x3, hipGraph replay, {rounds} alternating rounds of {cycles} D,G,G cycles, median ms per iteration: "
        f"flags off: {off:.2f} (spread {min(ms['off']):.2f}-{max(ms['off']):.2f}); --grad_clip 1e30 --nonfinite_guard: {on:.2f} "
        f"(spread {min(ms['ctl']):.2f}-{max(ms['ctl']):.2f}); difference {on - off:+.2f} ms = {100 * (on - off) / off:+.2f} % "
        f"({batch / off * 1e3:.1f} -> {batch / on * 1e3:.1f} images/s); last norms D {sd['norm']:.4e} G {sg['norm']:.4e}")
    return legs["ctl"].optim_gen.numel


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the report lines to this file")
    ap.add_argument("--image_size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--skip_step", action="store_true", help="only (a), at the flat size of a trainer that is built but never stepped")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: nothing here can be measured without one")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    say(f"tools/probe_gradclip.py on {torch.cuda.get_device_name(0)}")
    if a.skip_step:
        n = DiscoGANTrainer(default_args(), device=DEV, image_size=a.image_size, seed=1234).optim_gen.numel
    else:
        n = step_times(a.image_size, a.batch, a.rounds, a.cycles, say)
    torch.cuda.empty_cache()
    kernel_rates(n, say)


if __name__ == "__main__":
    main()
