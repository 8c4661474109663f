#!/usr/bin/env python3
"""What the trainable reconstruction criterion (--recon_loss) costs (tuning aid; profiles/recon_loss_cost.txt comes from here).

(a) The kernels alone on one pair of batches (default 512 px / batch 32, 100.7 MB each): ms per call, from device events, of
    dg_recon_loss_fwd / dg_recon_loss_bwd for ``l1`` (the streaming pass) and ``l1_ssim`` (the stencil), next to dg_mse_fwd / dg_mse_bwd on
    the same tensors as the streaming yardstick.  Byte estimate: forward 8 B/pixel value (x and t read), backward 12 (+ dx written);
    each figure is printed with its multiple of that estimate at the yardstick's rate.  Per kernel: medians of the device durations the
    profiler records.
(b) ms per iteration of the 512 px / batch 32 f32x3 step with ``mse`` against ``l1_ssim``: two trainers on one box, hipGraph replay,
    alternating, whole D,G,G cycles per timed window, host clock around a device synchronise.
(c) With ``--parent_tree DIR`` (a checkout of the parent commit; DG_LIB names the library it loads if it has none built): the ``mse`` leg
    ALONE, in a fresh process each, for DIR's package and for this one, before anything else.

    python tools/probe_recon.py [--out FILE] [--image_size 512] [--batch 32] [--rounds 4] [--cycles 2] [--skip_step] [--parent_tree DIR]
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
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tools.bench_ops import timeit  # noqa: E402

DEV = "cuda"
KIND = "l1_ssim"


def kernel_durations(fn, reps):
    """{kernel name: [device microseconds per launch]} of ``reps`` calls of ``fn``, as the profiler records them."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        if "recon_" in ev.name or "mse_" in ev.name:
            us = getattr(ev, "device_time", None)
            out.setdefault(ev.name, []).append(float(us if us is not None else ev.cuda_time))
    return out


def kernel_rates(size, batch, say):
    from discogan_modernized_amd.losses import recon_weights
    x, t = torch.rand(batch, 3, size, size, device=DEV), torch.rand(batch, 3, size, size, device=DEV)
    gout = torch.tensor(0.5, device=DEV)
    say(f"(a) one pair of batches [{batch},3,{size},{size}] = 2 x {x.numel() * 4 / 1e6:.1f} MB; ms per call, medians of 3 alternating rounds "
        "of 10 calls; estimate: forward 8 B/value, backward 12 B/value")
    cases = [("yardstick dg_mse_fwd", 8.0, lambda: ops.mse_fwd(x, t)), ("yardstick dg_mse_bwd", 12.0, lambda: ops.mse_bwd(x, t, gout))]
    for kind in ("l1", KIND):
        w = recon_weights(kind)
        cases.append((f"dg_recon_loss_fwd {kind}", 8.0, lambda w=w: ops.recon_loss_fwd(x, t, w)))
        cases.append((f"dg_recon_loss_bwd {kind}", 12.0, lambda w=w: ops.recon_loss_bwd(x, t, w, gout)))
    ms = {name: [] for name, _, _ in cases}
    for _ in range(3):
        for name, _, fn in cases:
            ms[name].append(timeit(fn, iters=10))
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, per, _ in cases:
        yard = med["yardstick dg_mse_fwd" if per == 8.0 else "yardstick dg_mse_bwd"]
        say(f"  {name:32s} {med[name]:.3f} ms  {per * x.numel() / med[name] / 1e6:7.0f} GB/s of the estimate  {med[name] / yard:5.2f} x the yardstick")
    try:
        w = recon_weights(KIND)
        per = kernel_durations(lambda: (ops.mse_fwd(x, t), ops.mse_bwd(x, t, gout), ops.recon_loss_fwd(x, t, w), ops.recon_loss_bwd(x, t, w, gout)), 10)
    except Exception as e:      # noqa: BLE001  (a profiler that cannot trace this device: the per-call figures above stand alone)
        say(f"  per-kernel durations: the profiler is not available here ({type(e).__name__}: {e})")
        return
    for name in sorted(per):
        say(f"  kernel {name[:90]:90s} {statistics.median(per[name]) / 1e3:.3f} ms  ({len(per[name])} launches)")


def step_times(size, batch, rounds, cycles, say):
    A, B = synthetic_batch(batch, size, 5, DEV)
    legs = {}
    for name in ("mse", KIND):
        legs[name] = DiscoGANTrainer(default_args(recon_loss=name), device=DEV, image_size=size, seed=1234, use_graph=True, mfma_dtype="f32x3")
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
        for name in (("mse", KIND) if r % 2 == 0 else (KIND, "mse")):
            ms[name].append(run(name, cycles))
        say(f"  round {r}: mse {ms['mse'][-1]:.2f} ms/iteration  {KIND} {ms[KIND][-1]:.2f} ms/iteration")
    off, on = statistics.median(ms["mse"]), statistics.median(ms[KIND])
    # bytes: every iteration two forward terms (8 B/value), a G-step two backward terms more (12 B/value); the MSE terms move the same
    e = 3.0 * batch * size * size
    say(f"(b) {size} px / batch {batch} f32x3, hipGraph replay, {rounds} alternating rounds of {cycles} D,G,G cycles, median ms per iteration: "
        f"mse: {off:.2f} (spread {min(ms['mse']):.2f}-{max(ms['mse']):.2f}); {KIND}: {on:.2f} (spread {min(ms[KIND]):.2f}-{max(ms[KIND]):.2f}); "
        f"difference {on - off:+.2f} ms = {100 * (on - off) / off:+.2f} % ({batch / off * 1e3:.1f} -> {batch / on * 1e3:.1f} images/s).  Bytes of "
        f"either criterion: D-step {2 * 8 * e / 1e9:.2f} GB, G-step {2 * 20 * e / 1e9:.2f} GB")


def solo_mse(size, batch, rounds, cycles):
    """The default step, one trainer alone in this process: one line on stdout."""
    A, B = synthetic_batch(batch, size, 5, DEV)
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=size, seed=1234, use_graph=True, mfma_dtype="f32x3")
    it, ms = 0, []
    for r in range(rounds + 1):                              # round 0: eager cycle, capture, one replayed cycle
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 3 * (3 if r == 0 else cycles)
        for _ in range(n):
            tr.train_iteration(A, B, it, need_losses=True)
            it += 1
        tr.finish()
        torch.cuda.synchronize()
        if r:
            ms.append((time.perf_counter() - t0) * 1e3 / n)
    print(f"alone, recon_loss {'mse' if hasattr(tr, 'recon_w') else 'absent'}: median {statistics.median(ms):.2f} ms per iteration (spread "
          f"{min(ms):.2f}-{max(ms):.2f}), {rounds} rounds of {cycles} D,G,G cycles")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the report lines to this file")
    ap.add_argument("--image_size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--skip_step", action="store_true", help="only (a)")
    ap.add_argument("--parent_tree", default=None, help="(c): a checkout of the parent commit whose default leg is timed alone, next to this one's")
    ap.add_argument("--solo_mse", action="store_true", help="what (c) runs in its child processes")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: nothing here can be measured without one")
    if a.solo_mse:
        return solo_mse(a.image_size, a.batch, a.rounds, a.cycles)

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.parent_tree:                                        # fresh processes, one after the other, before this one touches the device
        cmd = [sys.executable, os.path.abspath(__file__), "--solo_mse", "--image_size", str(a.image_size), "--batch", str(a.batch),
               "--rounds", str(a.rounds), "--cycles", str(a.cycles)]
        for who, tree in (("parent", os.path.abspath(a.parent_tree)), ("this tree", ROOT), ("parent", os.path.abspath(a.parent_tree))):
            r = subprocess.run(cmd, env=dict(os.environ, DG_PROBE_TREE=tree), capture_output=True, text=True, check=True)
            say(f"(c) {who}: " + [ln for ln in r.stdout.splitlines() if ln.startswith("alone")][-1])
    say(f"tools/probe_recon.py on {torch.cuda.get_device_name(0)}")
    kernel_rates(a.image_size, a.batch, say)
    torch.cuda.empty_cache()
    if not a.skip_step:
        step_times(a.image_size, a.batch, a.rounds, a.cycles, say)


if __name__ == "__main__":
    main()
