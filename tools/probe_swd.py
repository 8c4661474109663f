"""What --eval_swd costs: one evaluation event with and without the sliced Wasserstein distance, the one-off reference build, and the
share of each stage (profiles/swd_cost.txt).

    python tools/probe_swd.py [--sizes 64 512] [--n 200] [--rounds 5] [--out FILE]

An event = evaluate.evaluate_split: the four generator passes over the split, the image metrics, and with SWD the two scores.  Times are
host clocks around work that ends in a device synchronise; the two forms alternate inside one process; medians and spread are printed."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discogan_modernized_amd import evaluate, ops  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def med(v):
    return f"{statistics.median(v):.2f} ms (spread {min(v):.2f}-{max(v):.2f})"


def stages(sw, fake, rounds):
    """ms per stage of one SWD.score, summed over the levels, medians over rounds"""
    acc = dict(pyramid=[], descriptors=[], project=[], sort_distance=[])
    for _ in range(rounds):
        t, levels = timed(lambda: ops.lap_pyramid(fake[:sw.n]))
        acc["pyramid"].append(t)
        d = p = s = 0.0
        for l, level in enumerate(levels):
            t, _ = timed(lambda: ops.swd_descriptors(level, sw.recs[l], desc=sw.desc, stats=sw.stats))
            d += t
            t, _ = timed(lambda: ops.swd_project(sw.desc, sw.stats, sw.dirs, out=sw.proj))
            p += t
            t, _ = timed(lambda: ops.swd_row_distance(sw.proj, sw.ref[l], out=sw.dist[l]))
            s += t
        acc["descriptors"].append(d)
        acc["project"].append(p)
        acc["sort_distance"].append(s)
    return {k: statistics.median(v) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("probe_swd needs a HIP device")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/probe_swd.py on {torch.cuda.get_device_name(0)}; DG_SWD_MAX_ROW = {ops.swd_max_row()} as built "
        f"(a {ops.swd_max_row() * 4 // 1024} KiB workgroup launches); n = {a.n} images per set, P = {ops.swd_patches(a.n)} patches per image, "
        f"M = {a.n * ops.swd_patches(a.n)} values per row, 512 directions")
    for S in a.sizes:
        g = torch.Generator().manual_seed(S)
        split = (torch.rand(a.n, 3, S, S, generator=g).cuda(), torch.rand(a.n, 3, S, S, generator=g).cuda())
        tr = DiscoGANTrainer(default_args(), device="cuda", image_size=S, seed=1234)
        first, (swd, _) = timed(lambda: evaluate.make_swd_pair(*split, S, seed=0))
        ref = [timed(lambda: swd[0].set_reference(split[1]))[0] for _ in range(a.rounds)]
        evaluate.evaluate_split(tr, split, False)                       # warm-up of both forms
        evaluate.evaluate_split(tr, split, False, swd=swd)
        off, on, score = [], [], []
        for _ in range(a.rounds):
            t, (_, outs) = timed(lambda: evaluate.evaluate_split(tr, split, False))
            off.append(t)
            t, _ = timed(lambda: evaluate.evaluate_split(tr, split, False, swd=swd))
            on.append(t)
            t, _ = timed(lambda: (swd[0].score(outs[0]), swd[1].score(outs[1])))
            score.append(t)
        st = stages(swd[0], outs[0], a.rounds)
        total = sum(st.values())
        kept = sum(r.numel() * 4 for s in swd for r in s.ref) / 1e6
        say(f"{S} px, {len(swd[0].sizes)} levels {swd[0].sizes}:")
        say(f"  evaluation event, SWD off: {med(off)}")
        say(f"  evaluation event, SWD on:  {med(on)}   difference {statistics.median(on) - statistics.median(off):+.2f} ms")
        say(f"  the two scores alone (SWD_AB + SWD_BA): {med(score)}")
        say(f"  set_reference, one domain: {med(ref)}; first make_swd_pair (both domains + the domain gap, cold): {first:.1f} ms; "
            f"kept on the device: {kept:.0f} MB")
        say("  one score by stage (each stage synchronised, summed over levels): "
            + ", ".join(f"{k} {v:.2f} ms ({100 * v / total:.0f} %)" for k, v in st.items()))
        del tr, swd, split, outs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
