#!/usr/bin/env python3
"""What the differentiable augmentation of the discriminators' inputs costs (tuning aid; profiles/diffaug_cost.txt comes from here).

(a) The kernels alone on one batch (default 512 px / batch 32, 100.7 MB): per call, from device events, the gather pass alone (policy
    translation,cutout), statistics + gather (colour alone, and the whole policy), forward and backward, on a drawn table and on one
    whose shifts are multiples of 4 (every row keeps its 16-byte alignment); dg_pool_exchange with a pass table on a tensor of the same
    size in the same run as the copy yardstick (8 B/element, like the gather).  Per kernel (statistics, forward gather, backward
    gather): medians of the device durations the profiler records for each launch of the whole policy.
(b) ms per iteration of the 512 px / batch 32 f32x3 step with diffaug off against color,translation,cutout: two trainers on one box,
    hipGraph replay, alternating, whole D,G,G cycles per timed window, host clock around a device synchronise.

(c) With ``--parent_tree DIR`` (a checkout of the parent commit; DG_LIB names the library it loads if it has none built): the off leg
    ALONE, in a fresh process each, for DIR's package and for this one, before anything else -- the figure (b)'s off column is held
    against.  (Two trainers alive in one process, as in (b), cost a few tenths of a millisecond per iteration; compare like with like.)

    python tools/probe_diffaug.py [--out FILE] [--image_size 512] [--batch 32] [--rounds 4] [--cycles 2] [--skip_step] [--parent_tree DIR]
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
POLICY = "color,translation,cutout"


def kernel_durations(fn, reps):
    """{kernel name: [device microseconds per launch]} of ``reps`` calls of ``fn``, as the profiler records them."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        if "diffaug" in ev.name:
            us = getattr(ev, "device_time", None)
            out.setdefault(ev.name, []).append(float(us if us is not None else ev.cuda_time))
    return out


def kernel_rates(size, batch, say):
    x = torch.rand(batch, 3, size, size, device=DEV)
    z, pool = torch.empty_like(x), torch.zeros((1, 3, size, size), device=DEV)
    nbytes = 8.0 * x.numel()
    passes = torch.tensor([(j, -1, j, 0) for j in range(batch)], dtype=torch.int32, device=DEV)
    drawn = ops.diffaug_draw(1234, 0, 6, 0, 1, batch, size, 7, device=DEV)
    aligned = drawn.clone()
    aligned[:, 0] = torch.div(aligned[:, 0], 4, rounding_mode="trunc") * 4
    say(f"(a) one batch [{batch},3,{size},{size}] = {x.numel() * 4 / 1e6:.1f} MB; ms per call (GB/s at 8 B/element; the statistics pass "
        "reads 4 B/element more), medians of 3 alternating rounds of 10 calls")
    cases = [("copy yardstick dg_pool_exchange", lambda: ops.pool_exchange(x, pool, passes, out=z))]
    for tname, tab in (("drawn", drawn), ("aligned", aligned)):
        for pname, flags in (("translation,cutout", 6), ("color", 1), (POLICY, 7)):
            if pname == "color" and tname == "aligned":
                continue
            cases.append((f"fwd {pname} [{tname}]", lambda f=flags, t=tab: ops.diffaug_fwd(x, f, t, out=z)))
            cases.append((f"bwd {pname} [{tname}]", lambda f=flags, t=tab: ops.diffaug_bwd(x, f, t, out=z)))
    ms = {name: [] for name, _ in cases}
    for _ in range(3):
        for name, fn in cases:
            ms[name].append(timeit(fn, iters=10))
    for name, _ in cases:
        t = statistics.median(ms[name])
        say(f"  {name:48s} {t:.3f} ms  {nbytes / t / 1e6:7.0f} GB/s")
    try:
        per = kernel_durations(lambda: (ops.diffaug_fwd(x, 7, drawn, out=z), ops.diffaug_bwd(x, 7, drawn, out=z)), 10)
    except Exception as e:      # noqa: BLE001  (a profiler that cannot trace this device: the per-call figures above stand alone)
        say(f"  per-kernel durations: the profiler is not available here ({type(e).__name__}: {e})")
        return
    for name in sorted(per):
        t = statistics.median(per[name]) / 1e3
        b = (4.0 if "stats" in name else 8.0) * x.numel()
        say(f"  kernel {name[:70]:70s} {t:.3f} ms  {b / t / 1e6:7.0f} GB/s  ({len(per[name])} launches, whole policy, drawn table)")


def step_times(size, batch, rounds, cycles, say):
    A, B = synthetic_batch(batch, size, 5, DEV)
    legs = {}
    for name, policy in (("off", ""), ("on", POLICY)):
        legs[name] = DiscoGANTrainer(default_args(diffaug=policy), device=DEV, image_size=size, seed=1234, use_graph=True, mfma_dtype="f32x3")
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
        for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
            ms[name].append(run(name, cycles))
        say(f"  round {r}: off {ms['off'][-1]:.2f} ms/iteration  on {ms['on'][-1]:.2f} ms/iteration")
    off, on = statistics.median(ms["off"]), statistics.median(ms["on"])
    assert legs["on"].aug_A.drawn == batch and legs["off"].aug_A is None
    # bytes the transform moves: a D-step 4 forward passes; a G-step 4 forward + 2 backward; 8 B/element + 4 for each statistics pass
    e = 3.0 * batch * size * size
    d_gb, g_gb = 4 * 12 * e / 1e9, (4 * 12 + 2 * 12) * e / 1e9
    say(f"(b) {size} px / batch {batch} f32x3, hipGraph replay, {rounds} alternating rounds of {cycles} D,G,G cycles, median ms per iteration: "
        f"diffaug off: {off:.2f} (spread {min(ms['off']):.2f}-{max(ms['off']):.2f}); {POLICY}: {on:.2f} "
        f"(spread {min(ms['on']):.2f}-{max(ms['on']):.2f}); difference {on - off:+.2f} ms = {100 * (on - off) / off:+.2f} % "
        f"({batch / off * 1e3:.1f} -> {batch / on * 1e3:.1f} images/s).  Bytes moved by the transform: D-step {d_gb:.2f} GB, G-step {g_gb:.2f} GB "
        f"= {d_gb / 4.7:.2f} / {g_gb / 4.7:.2f} ms at 4.7 TB/s, {(d_gb + 2 * g_gb) / 3 / 4.7:.2f} ms per iteration of a D,G,G cycle")


def solo_off(size, batch, rounds, cycles):
    """The step without the feature, one trainer alone in this process: one line on stdout."""
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
    print(f"alone, diffaug {'off' if hasattr(tr, 'diffaug_flags') else 'absent'}: median {statistics.median(ms):.2f} ms per iteration (spread "
          f"{min(ms):.2f}-{max(ms):.2f}), {rounds} rounds of {cycles} D,G,G cycles")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the report lines to this file")
    ap.add_argument("--image_size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--skip_step", action="store_true", help="only (a)")
    ap.add_argument("--parent_tree", default=None, help="(c): a checkout of the parent commit whose off leg is timed alone, next to this one's")
    ap.add_argument("--solo_off", action="store_true", help="what (c) runs in its child processes")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: nothing here can be measured without one")
    if a.solo_off:
        return solo_off(a.image_size, a.batch, a.rounds, a.cycles)

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.parent_tree:                                        # fresh processes, one after the other, before this one touches the device
        cmd = [sys.executable, os.path.abspath(__file__), "--solo_off", "--image_size", str(a.image_size), "--batch", str(a.batch),
               "--rounds", str(a.rounds), "--cycles", str(a.cycles)]
        for who, tree in (("parent", os.path.abspath(a.parent_tree)), ("this tree", ROOT), ("parent", os.path.abspath(a.parent_tree))):
            r = subprocess.run(cmd, env=dict(os.environ, DG_PROBE_TREE=tree), capture_output=True, text=True, check=True)
            say(f"(c) {who}: " + [ln for ln in r.stdout.splitlines() if ln.startswith("alone")][-1])
    say(f"tools/probe_diffaug.py on {torch.cuda.get_device_name(0)}")
    kernel_rates(a.image_size, a.batch, say)
    torch.cuda.empty_cache()
    if not a.skip_step:
        step_times(a.image_size, a.batch, a.rounds, a.cycles, say)


if __name__ == "__main__":
    main()
