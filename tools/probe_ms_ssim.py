#!/usr/bin/env python3
"""What the multi-scale SSIM criterion (--recon_loss l1_ms_ssim) costs (tuning aid; profiles/ms_ssim_cost.txt comes from here).

(a) The kernels alone on one pair of batches: ms per call, from device events, of dg_ms_ssim_loss_fwd / _bwd and dg_image_ms_ssim next to
    dg_recon_loss_fwd / _bwd with ``l1_ssim`` (the single-scale stencil) and dg_mse_fwd / _bwd (the streaming yardstick) on the same
    tensors.
(b) ms per iteration of the training step, one trainer ALONE in a fresh process per leg, hipGraph replay, whole D,G,G cycles per timed
    window, host clock around a device synchronise; the legs take turns, twice: ``mse`` and ``l1_ssim`` of ``--parent_tree DIR`` (a
    checkout of the parent commit with its library built), ``l1_ms_ssim`` and ``mse`` of this tree.

    python tools/probe_ms_ssim.py --parent_tree DIR [--out FILE] [--image_size 512] [--batch 32] [--mfma f32x3] [--rounds 4] [--cycles 2]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("DG_PROBE_TREE") or ROOT)     # (b): the package of another checkout, timed by this file
sys.path.append(ROOT)
import torch  # noqa: E402

from discogan_modernized_amd import ops  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tools.bench_ops import timeit  # noqa: E402

DEV = "cuda"


def kernel_rates(size, batch, say):
    from discogan_modernized_amd.losses import recon_weights
    x, t = torch.rand(batch, 3, size, size, device=DEV), torch.rand(batch, 3, size, size, device=DEV)
    t = (0.6 * t + 0.4 * x).contiguous()                      # correlated: no clamped channel, every scale's gradient runs
    gout = torch.tensor(0.5, device=DEV)
    M = ops.ms_ssim_max_scales(size)
    w1, wm = recon_weights("l1_ssim"), recon_weights("l1_ms_ssim")
    _, save = ops.ms_ssim_loss_fwd(x, t, M, wm)
    say(f"(a) one pair of batches [{batch},3,{size},{size}] = 2 x {x.numel() * 4 / 1e6:.1f} MB, M = {M}; ms per call, medians of 3 alternating "
        f"rounds of 10 calls; save buffer {save.numel() * 4 / 1e6:.1f} MB")
    cases = [("dg_mse_fwd", lambda: ops.mse_fwd(x, t)), ("dg_mse_bwd", lambda: ops.mse_bwd(x, t, gout)),
             ("dg_recon_loss_fwd l1_ssim", lambda: ops.recon_loss_fwd(x, t, w1)), ("dg_recon_loss_bwd l1_ssim", lambda: ops.recon_loss_bwd(x, t, w1, gout)),
             ("dg_ms_ssim_loss_fwd l1_ms_ssim", lambda: ops.ms_ssim_loss_fwd(x, t, M, wm)),
             ("dg_ms_ssim_loss_bwd l1_ms_ssim", lambda: ops.ms_ssim_loss_bwd(x, t, M, wm, gout, save)),
             ("dg_image_metrics", lambda: ops.image_metrics(x, t)), ("dg_image_ms_ssim", lambda: ops.image_ms_ssim(x, t, M))]
    ms = {name: [] for name, _ in cases}
    for _ in range(3):
        for name, fn in cases:
            ms[name].append(timeit(fn, iters=10))
    for name, _ in cases:
        say(f"  {name:34s} {statistics.median(ms[name]):.3f} ms")


def solo(kind, size, batch, mfma, rounds, cycles):
    """One criterion, one trainer alone in this process: one line on stdout."""
    A, B = synthetic_batch(batch, size, 5, DEV)
    tr = DiscoGANTrainer(default_args(recon_loss=kind), device=DEV, image_size=size, seed=1234, use_graph=True, mfma_dtype=mfma)
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
    print(f"alone, recon_loss {kind}: {size} px / batch {batch} {mfma}: median {statistics.median(ms):.3f} ms per iteration (spread "
          f"{min(ms):.3f}-{max(ms):.3f}), {rounds} rounds of {cycles} D,G,G cycles")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the report lines to this file")
    ap.add_argument("--image_size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--mfma", default="f32x3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--parent_tree", default=None, help="(b): a checkout of the parent commit, library built")
    ap.add_argument("--solo", default=None, help="what (b) runs in its child processes: the criterion of the leg")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: nothing here can be measured without one")
    if a.solo:
        return solo(a.solo, a.image_size, a.batch, a.mfma, a.rounds, a.cycles)

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    say(f"tools/probe_ms_ssim.py on {torch.cuda.get_device_name(0)}")
    if a.parent_tree:                                        # fresh processes, one after the other
        parent = os.path.abspath(a.parent_tree)
        legs = (("parent", parent, "mse"), ("parent", parent, "l1_ssim"), ("this tree", ROOT, "l1_ms_ssim"), ("this tree", ROOT, "mse"))
        for who, tree, kind in legs + legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--solo", kind, "--image_size", str(a.image_size), "--batch", str(a.batch),
                   "--mfma", a.mfma, "--rounds", str(a.rounds), "--cycles", str(a.cycles)]
            r = subprocess.run(cmd, env=dict(os.environ, DG_PROBE_TREE=tree), capture_output=True, text=True, check=True)
            say(f"(b) {who}: " + [ln for ln in r.stdout.splitlines() if ln.startswith("alone")][-1])
    kernel_rates(a.image_size, a.batch, say)


if __name__ == "__main__":
    main()
