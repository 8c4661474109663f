"""Held-out evaluation: PSNR / SSIM / MAE of the generators on the test split (no counterpart in the reference, whose only quality
signal is the ``RECON:`` field of the training log).

The per-image numbers come from one kernel (``ops.image_metrics`` / ``dg_image_metrics``): MSE, MAE and SSIM (11 x 11 Gaussian window,
sigma 1.5, valid windows, data range 1 -- generator outputs are sigmoids and inputs are in [0, 1]; nothing is clamped or quantised).
The ``[n,3]`` rows cross PCIe once; the means over the split and ``PSNR = mean_i 10 log10(1 / mse_i)`` are taken in float64 on the host.

What is scored:
  recon_A, recon_B      the reconstructions ``A->B->A`` against ``A`` and ``B->A->B`` against ``B``
  trans_AB, trans_BA    paired splits only (``edges2shoes`` / ``edges2handbags``: image i of A and image i of B are the two halves of
                        one file): the translation ``A->B`` against ``B`` and ``B->A`` against ``A``, over the first min(n_A, n_B) images

  ms_ssim               with ``--eval_ms_ssim`` / ``--ms_ssim``: every entry above also holds the multi-scale SSIM (``ops.image_ms_ssim``:
                        Wang, Simoncelli, Bovik 2003, over as many scales as the size carries, at most 5)
  swd_AB, swd_BA        with ``--eval_swd`` / ``--swd``, paired or not: the sliced Wasserstein distance (``SWD`` below) between the
                        translations ``A->B`` and ``test_B``, and between ``B->A`` and ``test_A`` -- the only score an unpaired split has
                        for the translations themselves

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
SWD_MIN_SIZE = 16                                         # the coarsest pyramid level of the sliced Wasserstein distance


def paired_default(args, data_kind):
    """--eval_paired: ``auto`` is on for the files source of a task whose test images are A | B halves of one file."""
    mode = getattr(args, "eval_paired", "auto")
    if mode == "auto":
        return data_kind == "files" and args.task_name in PAIRED_TASKS
    return mode == "on"


def summarise(rows):
    """float [n,3] host rows of (mse, mae, ssim) -> dict of n and the float64 means; psnr = mean of the per-image 10 log10(1 / mse).
    A fourth column is the multi-scale SSIM (``--ms_ssim``) and adds the key ``ms_ssim``."""
    r = rows.double()
    mse = r[:, 0]
    psnr = torch.where(mse == 0, torch.full_like(mse, math.inf), 10.0 * torch.log10(1.0 / mse))
    res = dict(n=int(r.shape[0]), mse=float(mse.mean()), mae=float(r[:, 1].mean()), ssim=float(r[:, 2].mean()), psnr=float(psnr.mean()))
    if r.shape[1] > 3:
        res["ms_ssim"] = float(r[:, 3].mean())
    return res


class SWD:
    """Sliced Wasserstein distance between a fixed REAL set and generated sets, on Laplacian-pyramid patches (Karras et al., ICLR 2018,
    section 5; include/discogan_hip.h, "sliced Wasserstein distance", is the definition).  Per level: ``P`` 7 x 7 x 3 patches per image at
    keyed positions, each channel normalised over the set, ``dirs`` unit directions, both sets' projections sorted,
    ``SWD_l = 1000 mean_d mean_i |a_(i) - b_(i)|``; ``mean`` is the mean over the levels.  Deviations from the publication: a channel of
    standard deviation exactly 0 becomes zeros (the publication divides by zero); positions and directions are keyed on ``seed`` alone, so
    every event and every checkpoint is scored on the same patches and directions; no network, no host arithmetic but the last means.

    ``n`` images of both sets are used: ``P = min(patches, DG_SWD_MAX_ROW // n)`` patches per image, so that a row of ``M = n P`` projected
    values fits the LDS of the one workgroup that sorts it (n = 200: P = 128, M = 25600).

    Memory.  ``set_reference`` keeps the real set's sorted projections, ``D M 4`` bytes per level: 52 MB per level at n = 200, so 0.31 GB
    for the six levels of 512 px and about 0.6 GB for the two objects (one per domain) of an evaluation.  The descriptor table (M x 147) and the
    projection table (D x M) are allocated once, here; the few KB of statistics partials and each event's pyramid (4 n S^2 floats) come
    from torch's caching allocator."""

    def __init__(self, n, image_size, device, seed=0, patches=128, dirs=512):
        from . import ops
        self.n, self.size, self.seed, self.device = int(n), int(image_size), int(seed), torch.device(device)
        self.sizes = ops.swd_levels(image_size)
        if not self.sizes:
            raise ValueError(f"the sliced Wasserstein distance needs --image_size >= {SWD_MIN_SIZE}, got {image_size}")
        if not 1 <= self.n <= ops.swd_max_row():
            raise ValueError(f"the sliced Wasserstein distance takes 1 to {ops.swd_max_row()} images per set, got {n}")
        self.patches = ops.swd_patches(self.n, patches)
        self.M, self.D = self.n * self.patches, int(dirs)
        self.dirs = make_swd_directions(self.seed, self.D).to(self.device)
        self.recs = [ops.swd_draw(self.seed, l, self.n, R, self.patches, device=self.device) for l, R in enumerate(self.sizes)]
        self.desc = torch.empty((self.M, ops.SWD_DESC), device=self.device, dtype=torch.float32)
        self.stats = torch.empty((3, 2), device=self.device, dtype=torch.float64)
        self.proj = torch.empty((self.D, self.M), device=self.device, dtype=torch.float32)
        self.dist = torch.empty((len(self.sizes), self.D), device=self.device, dtype=torch.float64)
        self.ref = None

    def _project(self, l, level, out):
        from . import ops
        ops.swd_descriptors(level, self.recs[l], desc=self.desc, stats=self.stats)
        return ops.swd_project(self.desc, self.stats, self.dirs, out=out)

    def _levels(self, x):
        from . import ops
        if x.dim() != 4 or x.shape[0] < self.n or tuple(x.shape[1:]) != (3, self.size, self.size):
            raise ValueError(f"SWD was built for at least {self.n} images [3,{self.size},{self.size}], got {tuple(x.shape)}")
        return ops.lap_pyramid(x[:self.n])

    def set_reference(self, real):
        """Builds and keeps the sorted projections of the first n images of ``real`` for every level (once per run)."""
        from . import ops
        self.ref = []
        for l, level in enumerate(self._levels(real)):
            ref = torch.empty((self.D, self.M), device=self.device, dtype=torch.float32)
            self.ref.append(ops.swd_sort_rows(self._project(l, level, ref)))
        return self

    def score(self, fake):
        """The first n images of ``fake`` against the reference -> dict(levels=[SWD_l], mean, n, patches); one D2H copy of [L][D] doubles."""
        from . import ops
        if self.ref is None:
            raise RuntimeError("SWD.score before SWD.set_reference")
        for l, level in enumerate(self._levels(fake)):
            ops.swd_row_distance(self._project(l, level, self.proj), self.ref[l], out=self.dist[l])
        levels = [1000.0 * float(v) for v in self.dist.cpu().mean(dim=1)]
        return dict(levels=levels, mean=sum(levels) / len(levels), n=self.n, patches=self.patches)


def make_swd_directions(seed, dirs=512):
    """float32 [dirs,147]: standard-normal vectors from ``torch.Generator().manual_seed(seed)``, scaled to unit length in float64 and
    rounded once."""
    g = torch.Generator().manual_seed(int(seed))
    v = torch.randn((int(dirs), 147), generator=g, dtype=torch.float64)
    return (v / v.norm(dim=1, keepdim=True)).float()


def make_swd_pair(test_A, test_B, image_size, seed=0):
    """The two ``SWD`` objects of an evaluation, references built: ``(against test_B, against test_A)`` over the first
    min(n_A, n_B) images -- what ``evaluate_outputs(..., swd=...)`` takes.  Also returns SWD(test_A, test_B), the gap between the domains."""
    n = min(len(test_A), len(test_B))
    to_B = SWD(n, image_size, test_B.device, seed=seed).set_reference(test_B)
    to_A = SWD(n, image_size, test_A.device, seed=seed).set_reference(test_A)
    return (to_B, to_A), to_B.score(test_A)


def format_swd(r):
    return "/".join(f"{v:.3f}" for v in r["levels"]) + f"={r['mean']:.3f}"


def evaluate_outputs(test_A, test_B, AB, BA, ABA, BAB, paired, swd=None, ms_ssim=False):
    """The metric launches of one evaluation event on the six device batches of a sampling event -> dict of ``summarise`` dicts.
    ``swd``: two ``SWD`` objects with their references set, ``(against test_B, against test_A)``: the result also holds ``swd_AB`` and
    ``swd_BA`` (dicts of ``SWD.score``), for paired and unpaired splits alike.  ``ms_ssim``: every entry that has ``ssim`` also gets
    ``ms_ssim``, the mean of ``ops.image_ms_ssim`` over as many scales as the size carries."""
    from . import ops
    pairs = [("recon_A", test_A, ABA), ("recon_B", test_B, BAB)]
    if paired:
        n = min(len(test_A), len(test_B))
        pairs += [("trans_AB", test_B[:n], AB[:n]), ("trans_BA", test_A[:n], BA[:n])]
    rows = [ops.image_metrics(ref, got) for _, ref, got in pairs]
    if ms_ssim:
        rows = [torch.cat([r, ops.image_ms_ssim(ref, got)[:, None]], dim=1) for r, (_, ref, got) in zip(rows, pairs)]
    host = torch.cat(rows).cpu()                                      # one D2H copy
    res, at = {}, 0
    for (name, _, _), r in zip(pairs, rows):
        res[name] = summarise(host[at:at + len(r)])
        at += len(r)
    if swd is not None:
        res["swd_AB"] = swd[0].score(AB)
        res["swd_BA"] = swd[1].score(BA)
    return res


def format_eval(iters, res):
    def pair(key, a, b, fmt):
        return f"{format(res[a][key], fmt)}/{format(res[b][key], fmt)}"
    s = (f"Eval [{iters}] RECON_PSNR: {pair('psnr', 'recon_A', 'recon_B', '.3f')}, RECON_SSIM: {pair('ssim', 'recon_A', 'recon_B', '.4f')}, "
         f"RECON_MAE: {pair('mae', 'recon_A', 'recon_B', '.5f')}")
    if "trans_AB" in res:
        s += (f", TRANS_PSNR: {pair('psnr', 'trans_AB', 'trans_BA', '.3f')}, TRANS_SSIM: {pair('ssim', 'trans_AB', 'trans_BA', '.4f')}, "
              f"TRANS_MAE: {pair('mae', 'trans_AB', 'trans_BA', '.5f')}")
    if "swd_AB" in res:
        s += f", SWD_AB: {format_swd(res['swd_AB'])}, SWD_BA: {format_swd(res['swd_BA'])}"
    if "ms_ssim" in res["recon_A"]:
        s += f", RECON_MSSSIM: {pair('ms_ssim', 'recon_A', 'recon_B', '.4f')}"
        if "trans_AB" in res:
            s += f", TRANS_MSSSIM: {pair('ms_ssim', 'trans_AB', 'trans_BA', '.4f')}"
    return s + f" (n={res['recon_A']['n']}/{res['recon_B']['n']})"


def evaluate_split(trainer, split, paired, outs=None, swd=None, ms_ssim=False):
    """One evaluation event of a training run: the four passes of ``trainer.sample`` (unless the sampling event of the same iteration
    already ran them: ``outs``), then the metrics (``swd``, ``ms_ssim``: see ``evaluate_outputs``).  Returns ``(res, outs)``."""
    test_A, test_B = split
    if outs is None:
        outs = trainer.sample(test_A, test_B)
    return evaluate_outputs(test_A, test_B, *outs, paired, swd=swd, ms_ssim=ms_ssim), outs


def check_size(image_size, swd=False):
    if image_size < MIN_SIZE:
        raise ValueError(f"evaluation needs --image_size >= {MIN_SIZE} (the 11 x 11 SSIM window), got {image_size}")
    if swd and image_size < SWD_MIN_SIZE:
        raise ValueError(f"the sliced Wasserstein distance needs --image_size >= {SWD_MIN_SIZE} (its coarsest pyramid level), got {image_size}")


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
    p.add_argument("--swd", action="store_true",
                   help="also score the sliced Wasserstein distance of the translations against the other domain's test images "
                        "(swd_AB, swd_BA) and of the two test sets against each other (swd_domains); works on unpaired splits")
    p.add_argument("--swd_seed", type=int, default=0, help="key of the patch positions and directions of --swd")
    p.add_argument("--ms_ssim", action="store_true",
                   help="also score the multi-scale SSIM (Wang et al. 2003; up to five scales of a 2 x 2 average pyramid): an ms_ssim "
                        "entry next to every ssim")
    p.add_argument("--output", type=str, default="eval.json")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    check_size(args.image_size, swd=args.swd)
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
    swd, domains = make_swd_pair(test_A, test_B, args.image_size, args.swd_seed) if args.swd else (None, None)
    res = evaluate_outputs(test_A, test_B, AB, BA, ABA, BAB, args.paired, swd=swd, ms_ssim=args.ms_ssim)
    if args.swd:
        res["swd_domains"] = domains
        print(f"SWD_DOMAINS: {format_swd(domains)} (n={domains['n']}, {domains['patches']} patches per image)", flush=True)
    print(format_eval("final", res), flush=True)
    with open(args.output, "w") as f:
        json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
