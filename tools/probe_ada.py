#!/usr/bin/env python3
"""What adaptive discriminator augmentation adds to an iteration (tuning aid; profiles/ada_cost.txt comes from here).

ms per iteration of the training step with ``--diffaug color,translation,cutout``, without and with ``--ada_target 0.6`` (every other
flag at its default), under hipGraph replay.  Every leg is ONE trainer alone in a fresh process: warm-up (eager cycle, capture, one
replayed cycle), then ``--rounds`` timed windows of ``--cycles`` whole D,G,G cycles each, host clock around a device synchronise; the
leg's figure is the median window.  The legs alternate, ``--repeats`` processes each.  With ``--parent_tree DIR`` (a checkout of the
parent commit; DG_LIB names the library it loads if it has none built) the leg without ADA runs DIR's package.

What ADA adds to the launches of a D,G,G cycle: two dg_ada_accumulate per D-step, and per window of ``--ada_interval`` D-steps two
dg_ada_update and, under data parallelism, one 16-byte all-reduce.  The four dg_diffaug_draw_p per iteration replace four dg_diffaug_draw.

``--p0 1.0`` starts the ADA leg from p = 1 instead of 0: the transform then does the work of the leg without ADA (at p near 0 most
samples are neither shifted nor cut, and the gather reads whole aligned rows), so the difference is the controller's launches alone.

    python tools/probe_ada.py [--out FILE] [--image_size 512] [--batch 32] [--mfma_dtype f32x3] [--repeats 3] [--p0 P] [--parent_tree DIR]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICY = "color,translation,cutout"


def leg(a):
    """One trainer alone in this process: one line on stdout."""
    sys.path.insert(0, os.environ.get("DG_PROBE_TREE") or ROOT)
    import torch
    from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: nothing here can be measured without one")
    over = dict(diffaug=POLICY)
    if a.leg == "ada":
        over.update(ada_target=0.6)
        if a.p0 is not None:
            over.update(diffaug_p=a.p0)
    A, B = synthetic_batch(a.batch, a.image_size, 5, "cuda")
    tr = DiscoGANTrainer(default_args(**over), device="cuda", image_size=a.image_size, seed=1234, use_graph=True, mfma_dtype=a.mfma_dtype)
    it, ms = 0, []
    for r in range(a.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 3 * (3 if r == 0 else a.cycles)
        for _ in range(n):
            tr.train_iteration(A, B, it, need_losses=True)
            it += 1
        tr.finish()
        torch.cuda.synchronize()
        if r:
            ms.append((time.perf_counter() - t0) * 1e3 / n)
    note = ""
    if getattr(tr, "ada", None) is not None:
        s = tr.ada.stats()
        note = f"; controller: {s['updates'][0]} updates, {s['images'][0]} real images, p {s['p'][0]:.6f}/{s['p'][1]:.6f}"
    print(f"leg {a.leg}: median {statistics.median(ms):.3f} ms per iteration (spread {min(ms):.3f}-{max(ms):.3f}), {a.rounds} windows of "
          f"{a.cycles} D,G,G cycles{note}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the report lines to this file")
    ap.add_argument("--image_size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--mfma_dtype", default="f32x3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent_tree", default=None, help="a checkout of the parent commit: its package runs the leg without ADA")
    ap.add_argument("--p0", type=float, default=None,
                    help="the ADA leg's initial p (--diffaug_p): 1.0 keeps the transform's own work that of the leg without ADA")
    ap.add_argument("--leg", default=None, choices=["diffaug", "ada"], help="what the child processes run")
    a = ap.parse_args(argv)
    if a.leg:
        return leg(a)

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    cmd = [sys.executable, os.path.abspath(__file__), "--image_size", str(a.image_size), "--batch", str(a.batch), "--mfma_dtype", a.mfma_dtype,
           "--rounds", str(a.rounds), "--cycles", str(a.cycles)] + ([] if a.p0 is None else ["--p0", str(a.p0)])
    base_tree = os.path.abspath(a.parent_tree) if a.parent_tree else ROOT
    legs = (("diffaug", base_tree, "parent commit" if a.parent_tree else "this tree"), ("ada", ROOT, "this tree"))
    say(f"tools/probe_ada.py: {a.image_size} px / batch {a.batch} {a.mfma_dtype}, hipGraph replay, --diffaug {POLICY}"
        + ("" if a.p0 is None else f", ADA leg with --diffaug_p {a.p0:g}") + "; each line one fresh process")
    med = {name: [] for name, _, _ in legs}
    for r in range(a.repeats):
        for name, tree, who in (legs if r % 2 == 0 else legs[::-1]):
            out = subprocess.run(cmd + ["--leg", name], env=dict(os.environ, DG_PROBE_TREE=tree), capture_output=True, text=True, timeout=300)
            if out.returncode != 0:                          # nothing more is started on the device after a failed leg
                say(f"  repeat {r} {who}: leg {name} failed with status {out.returncode}: {out.stderr[-2000:]}")
                return 1
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("leg ")][-1]
            med[name].append(float(line.split("median ")[1].split(" ms")[0]))
            say(f"  repeat {r} {who}: {line}")
    off, on = statistics.median(med["diffaug"]), statistics.median(med["ada"])
    say(f"{a.image_size} px / batch {a.batch} {a.mfma_dtype}: without ADA {off:.3f} ms per iteration (processes {min(med['diffaug']):.3f}-"
        f"{max(med['diffaug']):.3f}), with --ada_target 0.6 {on:.3f} ({min(med['ada']):.3f}-{max(med['ada']):.3f}): {on - off:+.3f} ms = "
        f"{100 * (on - off) / off:+.2f} %")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
