"""Held-out evaluation: PSNR / SSIM / MAE of the generators on the test split (no counterpart in the reference, whose only quality
signal is the ``RECON:`` field of the training log).

The per-image numbers come from one kernel (``ops.image_metrics`` / ``dg_image_metrics``): MSE, MAE and SSIM (11 x 11 Gaussian window,
sigma 1.5, valid windows, data range 1 -- generator outputs are sigmoids and inputs are in [0, 1]; nothing is clamped or quantised).
The ``[n,3]`` rows cross PCIe once; the means over the split and ``PSNR = mean_i 10 log10(1 / mse_i)`` are taken in float64 on the host.

What is scored:
  recon_A, recon_B      the reconstructions ``A->B->A`` against ``A`` and ``B->A->B`` against ``B``
  trans_AB, trans_BA    paired splits only (``edges2shoes`` / ``edges2handbags``: image i of A and image i of B are the two halves of
                        one file): the translation ``A->B`` against ``B`` and ``B->A`` against ``A``, over the first min(n_A, n_B) images

Two ways to run it, which score different things:
  ``--eval_interval N`` of the training CLIs   scores the images of the sample grid: ``DiscoGANTrainer.sample``, generators in TRAINING
                        mode (BatchNorm normalises with the statistics of the whole split, one batch per pass; every event moves the
                        generators' running statistics by two forward calls -- once, also when a sample grid is due at the same
                        iteration).  One line per event in ``results/.../eval_log.txt``; ``training_log.txt`` is untouched.
  this module's CLI     scores a checkpoint the way it will be used: both ``gen_*_final.pth`` through ``inference.load_generator``, eval
                        mode (running statistics), BatchNorm folded into the convolutions unless ``--no_fold`` -- what inference.py runs.

    python -m discogan_modernized_amd.evaluate --model_path models/... --test_A tA.pt --test_B tB.pt --image_size 64 --paired
"""
from __future__ import annotations

import argparse
import json
import math
from pathlib import Path

import torch

PAIRED_TASKS = ("edges2shoes", "edges2handbags")        # dataset.py:52-60: both domains are cut from the same files
MIN_SIZE = 11                                             # the SSIM window


def paired_default(args, data_kind):
    """--eval_paired: ``auto`` is on for the files source of a task whose test images are A | B halves of one file."""
    mode = getattr(args, "eval_paired", "auto")
    if mode == "auto":
        return data_kind == "files" and args.task_name in PAIRED_TASKS
    return mode == "on"


def summarise(rows):
    """float [n,3] host rows of (mse, mae, ssim) -> dict of n and the float64 means; psnr = mean of the per-image 10 log10(1 / mse)."""
    r = rows.double()
    mse = r[:, 0]
    psnr = torch.where(mse == 0, torch.full_like(mse, math.inf), 10.0 * torch.log10(1.0 / mse))
    return dict(n=int(r.shape[0]), mse=float(mse.mean()), mae=float(r[:, 1].mean()), ssim=float(r[:, 2].mean()), psnr=float(psnr.mean()))


def evaluate_outputs(test_A, test_B, AB, BA, ABA, BAB, paired):
    """The metric launches of one evaluation event on the six device batches of a sampling event -> dict of ``summarise`` dicts."""
    from . import ops
    pairs = [("recon_A", test_A, ABA), ("recon_B", test_B, BAB)]
    if paired:
        n = min(len(test_A), len(test_B))
        pairs += [("trans_AB", test_B[:n], AB[:n]), ("trans_BA", test_A[:n], BA[:n])]
    rows = [ops.image_metrics(ref, got) for _, ref, got in pairs]
    host = torch.cat(rows).cpu()                                      # one D2H copy
    res, at = {}, 0
    for (name, _, _), r in zip(pairs, rows):
        res[name] = summarise(host[at:at + len(r)])
        at += len(r)
    return res


def format_eval(iters, res):
    def pair(key, a, b, fmt):
        return f"{format(res[a][key], fmt)}/{format(res[b][key], fmt)}"
    s = (f"Eval [{iters}] RECON_PSNR: {pair('psnr', 'recon_A', 'recon_B', '.3f')}, RECON_SSIM: {pair('ssim', 'recon_A', 'recon_B', '.4f')}, "
         f"RECON_MAE: {pair('mae', 'recon_A', 'recon_B', '.5f')}")
    if "trans_AB" in res:
        s += (f", TRANS_PSNR: {pair('psnr', 'trans_AB', 'trans_BA', '.3f')}, TRANS_SSIM: {pair('ssim', 'trans_AB', 'trans_BA', '.4f')}, "
              f"TRANS_MAE: {pair('mae', 'trans_AB', 'trans_BA', '.5f')}")
    return s + f" (n={res['recon_A']['n']}/{res['recon_B']['n']})"


def evaluate_split(trainer, split, paired, outs=None):
    """One evaluation event of a training run: the four passes of ``trainer.sample`` (unless the sampling event of the same iteration
    already ran them: ``outs``), then the metrics.  Returns ``(res, outs)``."""
    test_A, test_B = split
    if outs is None:
        outs = trainer.sample(test_A, test_B)
    return evaluate_outputs(test_A, test_B, *outs, paired), outs


def check_size(image_size):
    if image_size < MIN_SIZE:
        raise ValueError(f"evaluation needs --image_size >= {MIN_SIZE} (the 11 x 11 SSIM window), got {image_size}")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="PSNR / SSIM / MAE of a DiscoGAN checkpoint on a held-out split (HIP/MI355X)")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--model_path", type=str, required=True, help="directory with gen_A_final.pth and gen_B_final.pth")
    p.add_argument("--test_A", type=str, required=True, help="tensor file: float [n,3,S,S] in [0,1] or uint8 [n,S,S,3]")
    p.add_argument("--test_B", type=str, required=True)
    p.add_argument("--image_size", type=int, default=64)
    p.add_argument("--n_test", type=int, default=200)
    p.add_argument("--paired", action="store_true", help="image i of A and of B show the same thing: also score the translations")
    p.add_argument("--use_extra_layers", action="store_true")
    p.add_argument("--no_fold", action="store_true", help="run the training modules in eval() mode instead of the folded form")
    p.add_argument("--use_ema", action="store_true", help="score gen_A_ema_final.pth / gen_B_ema_final.pth (a run with --ema_decay)")
    p.add_argument("--output", type=str, default="eval.json")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    check_size(args.image_size)
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: this implementation has no CPU path")
    from . import inference, samples
    device = torch.device("cuda", torch.cuda.current_device())
    gens = []
    for direction in ("AtoB", "BtoA"):
        g, path = inference.load_generator(args.model_path, direction, args.image_size, device, args.use_extra_layers, fold=not args.no_fold,
                                             ema=args.use_ema)
        if g is None:
            raise FileNotFoundError(f"{path} not found")
        gens.append(g)
    g_ab, g_ba = gens
    test_A, test_B = (samples._load_tensor_split(p, args.n_test, args.image_size, device) for p in (args.test_A, args.test_B))
    if min(len(test_A), len(test_B)) < 1:
        raise ValueError(f"the test split holds {len(test_A)} / {len(test_B)} images")
    with torch.no_grad():
        AB, BA = g_ab(test_A), g_ba(test_B)
        ABA, BAB = g_ba(AB), g_ab(BA)
    res = evaluate_outputs(test_A, test_B, AB, BA, ABA, BAB, args.paired)
    print(format_eval("final", res), flush=True)
    with open(args.output, "w") as f:
        json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
