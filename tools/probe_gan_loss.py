#!/usr/bin/env python3
"""What the choice of the adversarial objective (--gan_loss) costs (tuning aid; profiles/gan_loss_cost.txt comes from here).

(a) The kernels alone on one logit vector of the batch's size: per call, from device events, dg_gan_loss_fwd / dg_gan_loss_bwd for
    lsgan next to the pair they replace (dg_act_fwd sigmoid + dg_bce_fwd, dg_bce_bwd) -- launch-bound at n = batch.
(b) ms per iteration of the training step with ``gan_loss`` bce against lsgan, at 512 px / batch 32 f32x3 and at 64 px / batch 64 f32:
    two trainers on one box, hipGraph replay, alternating, whole D,G,G cycles per timed window, host clock around a device synchronise.
(c) With ``--parent_tree DIR`` (a checkout of the parent commit; DG_LIB names the library it loads if it has none built): the bce leg
    ALONE, in a fresh process each, for DIR's package and for this one in turn, before anything else.  The default path passes when
    this tree's median lies within the spread of the parent's own rounds in the same run.

    python tools/probe_gan_loss.py [--out FILE] [--rounds 4] [--cycles 2] [--skip_step] [--parent_tree DIR]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("DG_PROBE_TREE") or ROOT)     # (c): the package of another checkout, timed by this file
sys.path.append(ROOT)
import torch  # noqa: E402

from discogan_modernized_amd import ops  # noqa: E402
from discogan_modernized_amd.trainer import DEFAULTS, DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tools.bench_ops import timeit  # noqa: E402

DEV = "cuda"
CONFIGS = ((512, 32, "f32x3"), (64, 64, "f32"))


def kernel_times(batch, say):
    x = torch.randn(batch, device=DEV) * 4.0
    gout = torch.tensor(0.7, device=DEV)
    slot = torch.empty((), device=DEV)
    p = ops.act_fwd(x, ops.ACT_SIGMOID, 0.0)
    cases = [("dg_act_fwd sigmoid", lambda: ops.act_fwd(x, ops.ACT_SIGMOID, 0.0)),
             ("dg_bce_fwd", lambda: ops.bce_fwd(p, 1.0, slot)), ("dg_bce_bwd", lambda: ops.bce_bwd(p, 1.0, gout)),
             ("dg_gan_loss_fwd lsgan", lambda: ops.gan_loss_fwd(x, ops.GAN_LSGAN, ops.GAN_D_REAL, 1.0, slot)),
             ("dg_gan_loss_bwd lsgan", lambda: ops.gan_loss_bwd(x, ops.GAN_LSGAN, ops.GAN_D_REAL, 1.0, gout)),
             ("dg_gan_loss_fwd bce_logits", lambda: ops.gan_loss_fwd(x, ops.GAN_BCE_LOGITS, ops.GAN_D_REAL, 1.0, slot)),
             ("dg_gan_loss_bwd bce_logits", lambda: ops.gan_loss_bwd(x, ops.GAN_BCE_LOGITS, ops.GAN_D_REAL, 1.0, gout))]
    say(f"(a) one logit vector of n = {batch}: microseconds per call (eager dispatch from Python, device events around 200 calls: at "
        "this size the launch, not the kernel), medians of 3 alternating rounds")
    us = {name: [] for name, _ in cases}
    for _ in range(3):
        for name, fn in cases:
            us[name].append(timeit(fn, iters=200) * 1e3)
    for name, _ in cases:
        say(f"  {name:32s} {statistics.median(us[name]):7.1f} us")


def _cycles(tr, A, B, it, ncycles):
    """ms per iteration of ``ncycles`` D,G,G cycles from iteration ``it`` on."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(3 * ncycles):
        tr.train_iteration(A, B, it + k, need_losses=True)
    tr.finish()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / (3 * ncycles)


def step_times(size, batch, dtype, rounds, cycles, say):
    A, B = synthetic_batch(batch, size, 5, DEV)
    legs = {k: DiscoGANTrainer(default_args(gan_loss=k), device=DEV, image_size=size, seed=1234, use_graph=True, mfma_dtype=dtype)
            for k in ("bce", "lsgan")}
    it = {k: 0 for k in legs}

    def run(name, ncycles):
        ms = _cycles(legs[name], A, B, it[name], ncycles)
        it[name] += 3 * ncycles
        return ms

    for name in legs:                                        # eager first cycle, graph capture in the second, one replayed cycle
        run(name, 3)
    ms = {k: [] for k in legs}
    for r in range(rounds):
        for name in (("bce", "lsgan") if r % 2 == 0 else ("lsgan", "bce")):
            ms[name].append(run(name, cycles))
        say(f"  round {r}: bce {ms['bce'][-1]:.3f} ms/iteration  lsgan {ms['lsgan'][-1]:.3f} ms/iteration")
    a, b = statistics.median(ms["bce"]), statistics.median(ms["lsgan"])
    say(f"(b) {size} px / batch {batch} {dtype}, hipGraph replay, {rounds} alternating rounds of {cycles} D,G,G cycles, median ms per iteration: "
        f"bce {a:.3f} (spread {min(ms['bce']):.3f}-{max(ms['bce']):.3f}); lsgan {b:.3f} (spread {min(ms['lsgan']):.3f}-{max(ms['lsgan']):.3f}); "
        f"difference {b - a:+.3f} ms = {100 * (b - a) / a:+.2f} % ({batch / a * 1e3:.1f} -> {batch / b * 1e3:.1f} images/s)")
    del legs
    torch.cuda.empty_cache()


def solo_bce(size, batch, dtype, rounds, cycles):
    """The default step, one trainer alone in this process: one line on stdout."""
    A, B = synthetic_batch(batch, size, 5, DEV)
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=size, seed=1234, use_graph=True, mfma_dtype=dtype)
    it, ms = 9, []
    _cycles(tr, A, B, 0, 3)                                  # eager cycle, capture, one replayed cycle
    for _ in range(rounds):
        ms.append(_cycles(tr, A, B, it, cycles))
        it += 3 * cycles
    print(f"alone, gan_loss {'bce' if 'gan_loss' in DEFAULTS else 'absent'}: {size} px / batch {batch} {dtype}: median {statistics.median(ms):.3f} ms "
          f"per iteration (spread {min(ms):.3f}-{max(ms):.3f}), {rounds} rounds of {cycles} D,G,G cycles")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the report lines to this file")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=2, help="D,G,G cycles per timed window at 512 px; the 64 px windows take 20 times as many")
    ap.add_argument("--skip_step", action="store_true", help="only (a)")
    ap.add_argument("--parent_tree", default=None, help="(c): a checkout of the parent commit whose bce leg is timed alone, next to this one's")
    ap.add_argument("--solo", nargs=3, default=None, metavar=("SIZE", "BATCH", "DTYPE"), help="what (c) runs in its child processes")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: nothing here can be measured without one")
    cyc = lambda size: a.cycles * (20 if size < 256 else 1)  # noqa: E731  (a window of a fraction of a second measures the scheduler)
    if a.solo:
        size, batch = int(a.solo[0]), int(a.solo[1])
        return solo_bce(size, batch, a.solo[2], a.rounds, cyc(size))

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.parent_tree:                                        # fresh processes, one after the other, before this one touches the device
        for size, batch, dtype in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--solo", str(size), str(batch), dtype, "--rounds", str(a.rounds), "--cycles", str(a.cycles)]
            for who, tree in (("parent", os.path.abspath(a.parent_tree)), ("this tree", ROOT)) * 2:
                r = subprocess.run(cmd, env=dict(os.environ, DG_PROBE_TREE=tree), capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(f"the {who} leg failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                say(f"(c) {who}: " + [ln for ln in r.stdout.splitlines() if ln.startswith("alone")][-1])
    say(f"tools/probe_gan_loss.py on {torch.cuda.get_device_name(0)}")
    kernel_times(64, say)
    if not a.skip_step:
        for size, batch, dtype in CONFIGS:
            step_times(size, batch, dtype, a.rounds, cyc(size), say)


if __name__ == "__main__":
    main()
