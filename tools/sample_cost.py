"""Cost of one sampling event (samples.save_samples) by part: the four generator passes on the held-out split, the grid kernel, the
D2H copy of the canvas and the PNG encode.  Host clock around work that ends in a device synchronise; one warm-up event, then the
median of --reps events.  Prints one JSON line per configuration (and writes them to --out).

    python tools/sample_cost.py --sizes 64 512 --n_test 200 --out sample_cost.json
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from discogan_modernized_amd import samples  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args  # noqa: E402

ARITH = {"f32": dict(mfma_dtype="f32"), "f32x3": dict(mfma_dtype="f32x3"), "bf16": dict(mfma_dtype="bf16", act_dtype="bf16")}


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def event(tr, tA, tB):
    from PIL import Image
    outs, t_pass = clock(lambda: tr.sample(tA, tB))
    canvas, t_grid = clock(lambda: samples.compose(tA, tB, *outs))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    samples.compose(tA, tB, *outs)                           # the same launch again between two device events: kernel + allocation only
    e1.record()
    torch.cuda.synchronize()
    host, t_d2h = clock(canvas.cpu)
    buf = io.BytesIO()
    t0 = time.perf_counter()
    Image.fromarray(host.numpy()).save(buf, format="PNG")
    t_png = (time.perf_counter() - t0) * 1e3
    return dict(passes_ms=t_pass, grid_ms=t_grid, grid_device_ms=e0.elapsed_time(e1), d2h_ms=t_d2h, png_ms=t_png), tuple(canvas.shape), buf.tell()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--arith", nargs="+", default=["f32", "f32x3", "bf16"], choices=list(ARITH))
    ap.add_argument("--n_test", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("sample_cost needs a HIP device")
    lines = []
    for S in a.sizes:
        g = torch.Generator(device="cuda").manual_seed(1)
        tA = torch.rand((a.n_test, 3, S, S), device="cuda", generator=g)
        tB = torch.rand((a.n_test, 3, S, S), device="cuda", generator=g)
        for name in a.arith:
            tr = DiscoGANTrainer(default_args(), device="cuda", image_size=S, seed=1234, **ARITH[name])
            event(tr, tA, tB)                                  # warm-up: code objects, allocator
            runs = [event(tr, tA, tB) for _ in range(a.reps)]
            res = dict(image_size=S, n_test=a.n_test, arithmetic=name, canvas=runs[0][1], png_bytes=runs[0][2])
            for k in runs[0][0]:
                vals = [r[0][k] for r in runs]
                res[k] = round(statistics.median(vals), 3)
                res[k + "_all"] = [round(v, 3) for v in vals]
            res["event_ms"] = round(sum(res[k] for k in ("passes_ms", "grid_ms", "d2h_ms", "png_ms")), 3)
            print(json.dumps(res), flush=True)
            lines.append(res)
            del tr
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
