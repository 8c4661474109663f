"""Re-hosted training CLI (reference image_translation.py:21-81, 211-435).

Same flags and defaults (``--task_name --model_arch --image_size --batch_size --epochs
--learning_rate --beta1 --beta2 --gan_curriculum --starting_rate --default_rate --update_interval
--log_interval --model_save_interval ...``), same log-line format (:394-398) and checkpoint file
names (``gen_A_{iters}.pth`` ... ``*_final.pth``, :420-432).  The training loop dispatches into the
HIP kernels through ``DiscoGANTrainer``.

Data sources (``--data_source``):
  files      the reference's own layout under ``--data_root`` (default ./datasets; dataset.py:14-22): file lists per task
             (dataset.get_data), PIL decode in worker threads, uint8 over PCIe on a copy stream, crop / erosion / resize /
             normalise on the device (dataset.DeviceLoader + dg_image_prep), double-buffered against the training step
  shards     ``--shard_A/--shard_B``: pre-decoded uint8 [n,H,W,3] .npy files (dataset.write_shard), memory-mapped, same device path
  tensors    ``--data_A/--data_B``: ``torch.save``d float tensors [n,3,S,S] in [0,1], or uint8 tensors [n,S,S,3] of decoded image
             rows that stay uint8 in HBM and are normalised / re-laid-out per batch on the device (dg_u8hwc_to_f32chw)
  synthetic  uniform tensors (``--synthetic_size`` images per domain): what the benchmark metric is defined on
  auto       tensors if --data_A/--data_B are given, shards if --shard_A/--shard_B, files if the task's directory exists, else synthetic

Sample grids (samples.py): every ``--image_save_interval`` iterations (0 = never) the four generator passes run on the held-out split
-- the files source's test lists, else ``--test_A/--test_B`` -- and ``results/.../samples/samples_iter_{i}.png`` is written.  As in the
reference these passes move the generators' BatchNorm running statistics.

Held-out evaluation (evaluate.py): every ``--eval_interval`` iterations (0 = never, the default) the same split is scored -- PSNR, SSIM
and MAE of the reconstructions, and of the translations when the split is paired (``--eval_paired``) -- and one line goes to
``results/.../eval_log.txt``.  An iteration that also writes a sample grid runs the four passes once for both.
``--eval_swd`` appends the sliced Wasserstein distance (``evaluate.SWD``: Laplacian-pyramid patches, no pairing needed) between the
translations and the other domain's held-out images to every such line, from the same passes; the held-out sets are projected and sorted
once at start, where ``SWD_DOMAINS:`` prints the distance between the two held-out sets themselves.

Weight EMA (optim.EMA): ``--ema_decay D`` (0 = off) keeps ``ema = D * ema + (1 - D) * w`` of both generators' weights, updated behind every
generator step from ``--ema_start_iter`` on; every model save also writes ``gen_A_ema_{tag}.pth`` / ``gen_B_ema_{tag}.pth`` (EMA weights, live
BatchNorm buffers) for ``inference.py --use_ema`` / ``evaluate.py --use_ema``.  ``--ema_samples`` runs the sample-grid and evaluation passes
on the EMA weights (``trainer.ema_weights()``); the live weights and running statistics are then left exactly as without those passes.
Gradient control: ``--grad_clip F`` clips every step's gradient to the global norm F, ``--nonfinite_guard`` skips a step whose gradient holds
an inf or a NaN, ``--log_grad_norm`` only measures; each of them appends `` GRAD: D <norm> G <norm> clipped c/n skipped s`` to the log line.
All decided on the device (optim.Adam.enable_grad_control); the counters travel in ``train_state_*.pth``.
Augmentation: ``--augment flip,crop`` (default: off) mirrors every training image with probability 1/2 and cuts a random ``image_size`` window
out of its preparation at ``L = round(image_size * --augment_scale)`` -- one fused launch per batch and domain (dg_image_prep_aug for uint8
rows, dg_augment_f32 for float tensors), records drawn on the device as a function of (seed, rank, iteration, domain, position), so
``--resume`` continues the sequence without any saved state.  The held-out split, sample grids and evaluation are never augmented.
Image history pool: ``--image_pool N`` (default 0 = off; 50 is customary) keeps N generated images per domain on the device
(``N * 3 * image_size^2 * 4`` bytes each).  In a D-step -- only there -- each discriminator is trained on the pool's exchange of the newest
fakes: stored and passed on while the pool fills, afterwards swapped with a random stored image with probability 1/2 (CycleGAN's
``ImagePool``).  One fused launch per domain (dg_pool_exchange) on records drawn on the device from (seed, rank, iteration, domain), so graph
replay and ``--resume`` reproduce the run bitwise; the pools travel in ``train_state_*.pth`` (key ``image_pool``).  A D-step's logged GEN / FM
values are then computed on the pooled fakes; G-steps, reconstructions, sample grids and evaluation never see a pool.
Differentiable augmentation: ``--diffaug color,translation,cutout`` (any subset; default "" = off) puts one random transform per sample in
front of everything a discriminator reads -- reals and fakes, D-steps and G-steps, where the gradient flows back through it into the
generator (Zhao et al. 2020, DiffAugment; on images in [0, 1]: brightness amplitude halved, padding and cutout fill 0.5).  HIP kernels
(dg_diffaug_fwd / dg_diffaug_bwd) on records drawn on the device from (seed, rank, iteration, domain, role): graph replay and ``--resume``
reproduce the run bitwise and nothing is saved.  It goes behind the pool exchange; generators, reconstructions, sample grids, evaluation
and the EMA never see it.  ``--diffaug_p P`` applies each stage to a sample with probability P in [0, 1] instead of always (default 1.0;
exactly 1.0 is the draw above).  ``--ada_target T`` (0 = off; in (0, 1), 0.6 is customary) adapts that probability during the run (Karras
et al. 2020, ADA): every discriminator step adds the signs of its outputs on the real batch to a window, and every ``--ada_interval``-th
(default 4) moves p by (real images of the window) / (1000 ``--ada_kimg``) (default 500) up when r_t = E[sign(D(real))] exceeds T, down when
below, within [0, ``--ada_p_max``]; p starts from ``--diffaug_p`` (default 0 then).  One p per domain; p, the window and the controller live
on the device (dg_diffaug_draw_p, dg_ada_accumulate, dg_ada_update), data-parallel ranks sum their windows in one 16-byte all-reduce, the
state travels in ``train_state_*.pth`` (key ``ada``) and log lines end in `` ADA: p <pA>/<pB> rt <rtA>/<rtB>``.
Reconstruction criterion: ``--recon_loss {mse,l1,ssim,l1_ssim}`` (default ``mse``, the reference's) chooses what the two cycle terms
ABA against A and BAB against B are measured with: ``l1`` = mean |x - t| (CycleGAN), ``ssim`` = 1 - SSIM (the 11 x 11 Gaussian window,
sigma 1.5, valid windows, that ``SSIM_ABA`` of the evaluation reports; needs ``--image_size >= 11``), ``l1_ssim`` = (1 - alpha) L1 +
alpha (1 - SSIM) with ``--recon_ssim_alpha`` (default 0.84, Zhao et al. 2017).  One fused forward and one backward kernel per term
(dg_recon_loss_fwd / dg_recon_loss_bwd) in the place of the MSE kernels: captured, replayed and resumed like them, nothing is saved, and
the ``RECON:`` field of the log line prints the criterion's value.  With ``mse`` nothing changes.  ``ms_ssim`` = 1 - MS-SSIM (Wang,
Simoncelli, Bovik 2003: the contrast-structure term at every scale of a 2 x 2 average pyramid, the full SSIM at the coarsest, exponents
normalised) and ``l1_ms_ssim`` = (1 - alpha) L1 + alpha (1 - MS-SSIM) -- the mix Zhao et al.'s 0.84 belongs to -- over
``--recon_ms_scales`` scales (default 0: as many as ``--image_size`` carries with every side >= 11, at most 5); dg_ms_ssim_loss_fwd /
_bwd, whose forward keeps both pyramids and a small table for its backward (freed with the graph of the iteration; nothing to checkpoint).
``--eval_ms_ssim`` appends ``RECON_MSSSIM: a/b`` (paired: and ``TRANS_MSSSIM``) to the evaluation lines.
Adversarial objective: ``--gan_loss {bce,bce_logits,lsgan,hinge}`` (default ``bce``, the reference's nn.BCELoss on the sigmoid output)
chooses what the six GAN terms are measured with.  The other three read the discriminators' LOGITS (the sigmoid is not launched):
``bce_logits`` = the same cross entropy in its stable form (softplus; the gradient of a saturated logit stays accurate instead of coming
from the -100 clamp), ``lsgan`` = mean (x - target)^2 (CycleGAN's), ``hinge`` = mean max(0, 1 -+ x) for the discriminators and -mean x
for the generators (the DiffAugment baselines').  ``--gan_real_label`` (default 1.0, in (0.5, 1]) is the target of a discriminator's real
batch (one-sided label smoothing; not with ``hinge``).  One fused forward and one backward kernel per term (dg_gan_loss_fwd /
dg_gan_loss_bwd) in the place of the BCE kernels: captured, replayed and resumed like them, nothing is saved; ``GEN:`` / ``DIS:`` print
the objective's values.

Batch order.  Single process: A and B are shuffled independently every epoch (shuffle_data, dataset.py:24-35),
``data_size // batch_size`` batches.  Data parallel: the ``DistributedSampler`` contract of
distributed_image_translation.py:203-216,451-452 -- ONE permutation per epoch from a seed shared by all ranks
(``set_epoch``), rank r takes ``perm[r::W]``, A_i is paired with B_i (dataset.py:215-222), the last batch of the
shard may be short (no drop_last); a final batch of a single sample is skipped (train-mode BatchNorm needs two).

    python -m discogan_modernized_amd.image_translation --task_name edges2shoes --image_size 64 --batch_size 256
"""
from __future__ import annotations

import argparse
import contextlib
import os
import time
from datetime import datetime
from pathlib import Path

import torch

from .losses import GAN_KINDS, MS_SSIM_KINDS
from .trainer import DiscoGANTrainer, check_ada, check_diffaug, check_gan_loss, check_image_pool, check_recon_loss
from .trainer import recon_ms_scales as recon_ms_scales_of

TASKS = ["facescrub", "celebA", "edges2shoes", "edges2handbags", "handbags2shoes", "tops2hanbok", "hanbok2tops"]


def build_parser(description="HIP/MI355X implementation of the DiscoGAN training path"):
    p = argparse.ArgumentParser(description=description)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--task_name", type=str, default="facescrub")
    p.add_argument("--results_dir", type=str, default="./results/")
    p.add_argument("--models_dir", type=str, default="./models/")
    p.add_argument("--model_arch", type=str, default="discogan", choices=["discogan", "recongan", "gan"])
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--learning_rate", type=float, default=0.0002)
    p.add_argument("--beta1", type=float, default=0.5)
    p.add_argument("--beta2", type=float, default=0.999)
    p.add_argument("--image_size", type=int, default=64)
    p.add_argument("--gan_curriculum", type=int, default=10000)
    p.add_argument("--starting_rate", type=float, default=0.01)
    p.add_argument("--default_rate", type=float, default=0.5)
    p.add_argument("--style_A", type=str, default=None)
    p.add_argument("--style_B", type=str, default=None)
    p.add_argument("--constraint", type=str, default=None)
    p.add_argument("--constraint_type", type=str, default=None)
    p.add_argument("--n_test", type=int, default=200)
    p.add_argument("--update_interval", type=int, default=3)
    p.add_argument("--log_interval", type=int, default=50)
    p.add_argument("--image_save_interval", type=int, default=1000)
    p.add_argument("--model_save_interval", type=int, default=10000)
    # additions of this implementation
    p.add_argument("--data_A", type=str, default=None, help="torch.save'd float tensor [n,3,S,S] for domain A")
    p.add_argument("--data_B", type=str, default=None, help="torch.save'd float tensor [n,3,S,S] for domain B")
    p.add_argument("--test_A", type=str, default=None,
                   help="held-out images of domain A for the sample grids (tensor file like --data_A: float [n,3,S,S] or uint8 [n,S,S,3], "
                        "first --n_test used); the files source takes its test lists instead")
    p.add_argument("--test_B", type=str, default=None, help="held-out images of domain B (see --test_A)")
    p.add_argument("--eval_interval", type=int, default=0,
                   help="every N iterations score the held-out split (PSNR / SSIM / MAE, evaluate.py) into eval_log.txt; 0 = never")
    p.add_argument("--eval_paired", type=str, default="auto", choices=["auto", "on", "off"],
                   help="image i of test A and of test B show the same thing, so the translations are scored too; auto: the files "
                        "source of edges2shoes / edges2handbags")
    p.add_argument("--eval_swd", action="store_true",
                   help="with --eval_interval: also score the sliced Wasserstein distance on Laplacian-pyramid patches between the "
                        "translations and the other domain's held-out images (SWD_AB, SWD_BA; needs no pairing); keeps "
                        "512 * n * P * 4 bytes per pyramid level and domain on the device (evaluate.SWD)")
    p.add_argument("--eval_ms_ssim", action="store_true",
                   help="with --eval_interval: append the multi-scale SSIM of the reconstructions (and of the translations of a paired "
                        "split) to every evaluation line: RECON_MSSSIM: a/b")
    p.add_argument("--eval_swd_seed", type=int, default=0, help="key of the patch positions and directions of --eval_swd")
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="keep an exponential moving average of both generators' weights with this decay (e.g. 0.999; 0 = off) and "
                        "save it as gen_A_ema_*.pth / gen_B_ema_*.pth next to the live checkpoints")
    p.add_argument("--ema_start_iter", type=int, default=0, help="the first generator step at or after this iteration starts the EMA with a copy")
    p.add_argument("--ema_samples", action="store_true",
                   help="sample grids and evaluation events run on the EMA weights once the EMA has started (eval lines end in ' [ema]')")
    p.add_argument("--grad_clip", type=float, default=0.0,
                   help="clip every optimiser step's gradient to this global L2 norm (torch.nn.utils.clip_grad_norm_'s rule; 0 = off)")
    p.add_argument("--nonfinite_guard", action="store_true",
                   help="skip an optimiser step whose gradient holds an inf or a NaN (weights, Adam moments and step count stay as they are)")
    p.add_argument("--log_grad_norm", action="store_true",
                   help="append ' GRAD: D <norm> G <norm> clipped c/n skipped s' to every log line (implied by the two flags above)")
    p.add_argument("--augment", type=str, default="",
                   help="comma list of 'flip' (random left-right mirror) and 'crop' (prepare at --augment_scale times --image_size, cut a random "
                        "--image_size window): training data only, on the device, keyed on (seed, rank, iteration); empty = off")
    p.add_argument("--augment_scale", type=float, default=1.125, help="with --augment crop: L = round(image_size * scale), >= 1 (286/256 ~ 1.117)")
    p.add_argument("--image_pool", type=int, default=0,
                   help="history pool of generated images per domain for the discriminator steps (CycleGAN's ImagePool; 50 is the customary "
                        "size; 0 = off): N * 3 * image_size^2 * 4 bytes of device memory per domain, keyed on (seed, rank, iteration)")
    p.add_argument("--diffaug", type=str, default="",
                   help="comma list of 'color', 'translation', 'cutout': differentiable augmentation (DiffAugment) of every discriminator "
                        "input, reals and fakes, on the device, keyed on (seed, rank, iteration); empty or 'none' = off")
    p.add_argument("--diffaug_p", type=float, default=None,
                   help="with --diffaug: probability in [0, 1] that each stage of the policy is applied to a sample (drawn per sample and "
                        "stage); default 1.0 (every stage on every sample), or with --ada_target the initial p, default 0.0")
    p.add_argument("--ada_target", type=float, default=0.0,
                   help="with --diffaug: adapt the probability on the device (ADA, Karras et al. 2020) so that the discriminators' "
                        "overfitting measure r_t = E[sign(D(real))] approaches this target in (0, 1) (0.6 is customary); 0 = off")
    p.add_argument("--ada_interval", type=int, default=4, help="with --ada_target: discriminator steps per update of p")
    p.add_argument("--ada_kimg", type=float, default=500.0,
                   help="with --ada_target: thousands of real images it takes p to travel from 0 to 1 (the step per image is 1 / (1000 kimg))")
    p.add_argument("--ada_p_max", type=float, default=1.0, help="with --ada_target: the upper bound of p, in (0, 1]")
    p.add_argument("--recon_loss", type=str, default="mse", choices=["mse", "l1", "ssim", "l1_ssim", "ms_ssim", "l1_ms_ssim"],
                   help="criterion of the two reconstruction (cycle) terms: mse (the reference's nn.MSELoss), l1 (CycleGAN's), ssim "
                        "(1 - SSIM, the 11 x 11 Gaussian window of the evaluation), l1_ssim ((1 - alpha) L1 + alpha (1 - SSIM)), ms_ssim "
                        "(1 - multi-scale SSIM) or l1_ms_ssim ((1 - alpha) L1 + alpha (1 - MS-SSIM)); the SSIM kinds need "
                        "--image_size >= 11")
    p.add_argument("--recon_ssim_alpha", type=float, default=0.84,
                   help="with --recon_loss l1_ssim / l1_ms_ssim: the weight alpha of the SSIM term, in (0, 1) (Zhao et al. 2017: 0.84)")
    p.add_argument("--recon_ms_scales", type=int, default=0,
                   help="with --recon_loss ms_ssim / l1_ms_ssim: the number of scales, each half the side of the one before and at least "
                        "11 pixels; 0 = as many as --image_size carries, at most 5 (64 px: 3, 176 px and more: 5)")
    p.add_argument("--gan_loss", type=str, default="bce", choices=list(GAN_KINDS),
                   help="adversarial objective: bce (the reference's nn.BCELoss on the sigmoid output) or, on the discriminators' logits, "
                        "bce_logits (the same in its stable form), lsgan ((x - target)^2, CycleGAN's) or hinge (max(0, 1 -+ x) | -x)")
    p.add_argument("--gan_real_label", type=float, default=1.0,
                   help="target of a discriminator's real batch, in (0.5, 1] (one-sided label smoothing, e.g. 0.9); hinge takes 1 only")
    p.add_argument("--synthetic_size", type=int, default=1024, help="images per domain when no data files are given")
    p.add_argument("--data_source", type=str, default="auto", choices=["auto", "files", "shards", "tensors", "synthetic"])
    p.add_argument("--data_root", type=str, default=None, help="root of the reference's dataset layout (dataset.py:14-22; default ./datasets)")
    p.add_argument("--shard_A", type=str, nargs="*", default=None, help="pre-decoded uint8 [n,H,W,3] .npy shard(s) for domain A")
    p.add_argument("--shard_B", type=str, nargs="*", default=None, help="pre-decoded uint8 [n,H,W,3] .npy shard(s) for domain B")
    p.add_argument("--loader_workers", type=int, default=4, help="decode threads of the device loader (reference: num_workers=4)")
    p.add_argument("--max_iters", type=int, default=0, help="stop after this many iterations (0 = all epochs)")
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--no_graph", action="store_true", help="dispatch every kernel from Python (no hipGraph replay)")
    p.add_argument("--weight_decay", type=float, default=0.00001)
    p.add_argument("--save_train_state", action="store_true",
                   help="also write train_state_{iters}.pth (weights + Adam moments + iteration) at every model save")
    p.add_argument("--resume", type=str, default=None,
                   help="train_state_*.pth to continue from: weights, BN buffers, Adam moments, iteration and position in the data order")
    p.add_argument("--skip_log_only_passes", action="store_true",
                   help="on iterations that print no log line, D-steps skip the two reconstruction passes (they feed only the "
                        "log). Same weights; the generators' BatchNorm running statistics then differ from the reference's")
    p.add_argument("--comm", type=str, default="auto", choices=["auto", "capi", "c10d"],
                   help="data-parallel transport: the library's own RCCL communicator (capi) or torch.distributed (c10d)")
    p.add_argument("--mfma_dtype", type=str, default="f32", choices=["f32", "bf16", "f32x3"],
                   help="bf16: conv operands rounded to bf16 on the matrix cores, fp32 accumulate/BatchNorm/weights/Adam; "
                        "f32x3: fp32-accurate products from three bf16 planes per operand (six bf16 MFMAs per block)")
    p.add_argument("--act_dtype", type=str, default="f32", choices=["f32", "bf16"],
                   help="with --mfma_dtype bf16: feature maps and their gradients stored in bf16 (fp32 BatchNorm statistics and arithmetic, "
                        "fp32 weights / parameter gradients / Adam)")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def load_domains(args, device, rank=0, world_size=1):
    """Both domains resident in HBM.  Synthetic data: per-rank seed in a single process (benchmark semantics), ONE
    shared dataset under data parallelism (every rank then takes its DistributedSampler shard of it)."""
    if args.data_A and args.data_B:
        A = torch.load(args.data_A, map_location="cpu")
        B = torch.load(args.data_B, map_location="cpu")
        A = A if A.dtype == torch.uint8 else A.float()
        B = B if B.dtype == torch.uint8 else B.float()
    else:
        g = torch.Generator().manual_seed(1000 + (rank if world_size == 1 else 0))
        A = torch.rand(args.synthetic_size, 3, args.image_size, args.image_size, generator=g)
        B = torch.rand(args.synthetic_size, 3, args.image_size, args.image_size, generator=g)
    return A.to(device), B.to(device)


def augment_of(args, rank=0):
    """The dataset.Augment record of a run (``--augment`` / ``--augment_scale``), or None when augmentation is off.  Validates both."""
    from . import dataset as ds
    flags = ds.parse_augment(getattr(args, "augment", ""))
    scale = float(getattr(args, "augment_scale", 1.125))
    ds.augment_size(args.image_size, flags, scale)
    return ds.Augment(int(args.seed), int(rank), flags, scale, 0) if flags else None


class _ResidentData:
    """Both domains resident in HBM (tensor files / synthetic): a batch is an index_select (+ the uint8 ingest kernel).
    ``augment`` (dataset.Augment): batch ``start + i`` of the slice is augmented with the draw of iteration ``first_iteration + i``."""

    def __init__(self, A, B, augment=None, image_size=None):
        self.A, self.B = A, B
        self.size = min(len(A), len(B))
        self.augment, self.S = (augment if augment is not None and augment.flags else None), image_size

    def epoch(self, batches, start=0, first_iteration=None):
        if self.augment is None:
            for ia, ib in batches[start:]:
                yield take_batch(self.A, ia), take_batch(self.B, ib)
            return
        it0 = start if first_iteration is None else first_iteration
        for i, (ia, ib) in enumerate(batches[start:]):
            yield (take_batch(self.A, ia, (self.augment, 0, it0 + i, self.S)), take_batch(self.B, ib, (self.augment, 1, it0 + i, self.S)))


class _StreamedData:
    """Image files or pre-decoded shards: dataset.DeviceLoader stages the next batch while the current one trains."""

    def __init__(self, src_A, src_B, domains, image_size, device, workers, augment=None):
        self.src, self.domains, self.S, self.device, self.workers = (src_A, src_B), domains, image_size, device, workers
        self.size = min(len(src_A), len(src_B))
        self.augment = augment

    def epoch(self, batches, start=0, first_iteration=None):
        from . import dataset as ds
        aug = self.augment
        if aug is not None:
            aug = aug._replace(first_iteration=start if first_iteration is None else first_iteration)
        loader = ds.DeviceLoader(self.src[0], self.src[1], self.domains, self.S,
                                 [(a.cpu().numpy(), b.cpu().numpy()) for a, b in batches[start:]], device=self.device, workers=self.workers,
                                 augment=aug)
        try:
            yield from loader
        finally:
            loader.close()


def open_data(args, device, rank=0, world_size=1):
    """The training data behind one interface (``.size``, ``.epoch(index batches, start)``), chosen by --data_source."""
    from . import dataset as ds
    src = getattr(args, "data_source", "auto")
    ds.set_root(getattr(args, "data_root", None) or "./datasets")      # every run states its root: nothing leaks from an earlier call
    if src == "auto":
        if args.data_A and args.data_B:
            src = "tensors"
        elif getattr(args, "shard_A", None) and getattr(args, "shard_B", None):
            src = "shards"
        else:
            # the synthetic stand-in is for the bare command line on a machine without datasets ONLY: a run that names its data
            # (--data_root, --style_A / --style_B / --constraint) or whose dataset root exists raises what the reference raises
            # (a mistyped style: KeyError, an empty directory: ValueError, a wrong root: FileNotFoundError) instead of training on noise
            named = any(getattr(args, k, None) for k in ("data_root", "style_A", "style_B", "constraint"))
            if named or os.path.isdir(getattr(args, "data_root", None) or "./datasets"):
                ds.get_data(args)
                src = "files"
            else:
                src = "synthetic"
    domains = ds.task_domains(args.task_name)
    workers = getattr(args, "loader_workers", 4)
    aug = augment_of(args, rank)                 # the TRAINING data only: the held-out split (samples.load_split) never passes through here
    if src == "files":
        data_A, data_B, _, _ = ds.get_data(args)
        return _StreamedData(ds.FileSource(data_A), ds.FileSource(data_B), domains, args.image_size, device, workers, aug), src
    if src == "shards":
        return _StreamedData(ds.ShardSource(args.shard_A), ds.ShardSource(args.shard_B), domains, args.image_size, device, workers, aug), src
    if src == "tensors" and not (args.data_A and args.data_B):
        raise ValueError("--data_source tensors needs --data_A and --data_B")
    if src == "synthetic":
        args = argparse.Namespace(**{**vars(args), "data_A": None, "data_B": None})
    return _ResidentData(*load_domains(args, device, rank, world_size), augment=aug, image_size=args.image_size), src


def take_batch(data, idx, aug=None):
    """Rows ``idx`` of a resident domain as the float NCHW batch the networks take (image_translation.py:332-333).
    uint8 [n,S,S,3] sources are normalised and transposed on the device (dataset.py:65-66).
    ``aug = (dataset.Augment, domain 0 | 1, iteration, S)``: the augmented batch -- records drawn on the device for that iteration, then ONE
    launch: dg_image_prep_aug on uint8 rows (the whole image, cv2's 8-bit resize), dg_augment_f32 on a float batch."""
    x = data.index_select(0, idx)
    if aug is not None:
        from . import dataset as ds, ops
        a, d, iteration, S = aug
        L = a.size(S)
        recs = ops.augment_draw(a.seed, a.rank, iteration, d, len(idx), S, L, a.flags, device=x.device)
        if x.dtype == torch.uint8:
            return ds.prepare_batch(x, None, S, aug=(L, recs, None))
        if x.shape[-1] != S:
            raise ValueError(f"float training tensors are [n,3,S,S] with S = --image_size = {S}, got {tuple(x.shape)}")
        return ops.augment_f32(x, L, recs)
    if x.dtype == torch.uint8:
        from . import ops
        return ops.u8hwc_to_f32chw(x)
    return x


def run_dirs(args, rank_suffix=""):
    ts = datetime.now().strftime("%Y%m%d_%H%M%S") + rank_suffix
    sub = Path(args.task_name)
    if args.style_A:
        sub = sub / args.style_A
    sub = sub / args.model_arch / ts
    return Path(args.results_dir) / sub, Path(args.models_dir) / sub


def save_models(trainer, model_path, tag, next_iter=None, with_state=False, loader=None):
    """The four live networks as ``{net}_{tag}.pth``; with the EMA on and started also ``gen_A_ema_{tag}.pth`` / ``gen_B_ema_{tag}.pth``."""
    trainer.finish()                      # join the communication stream before reading parameters
    if with_state and next_iter is not None:
        torch.save(trainer.train_state(next_iter, extra=loader), model_path / f"train_state_{tag}.pth")
    names = dict(gen_A=trainer.generator_A, gen_B=trainer.generator_B,
                 dis_A=trainer.discriminator_A, dis_B=trainer.discriminator_B)
    for k, net in names.items():
        sd = {n: (t.detach().contiguous().cpu()) for n, t in net.state_dict().items()}
        torch.save(sd, model_path / f"{k}_{tag}.pth")
    ema = getattr(trainer, "ema", None)
    if ema is not None and ema.ready:
        for k, sd in trainer.ema_state_dicts().items():
            torch.save(sd, model_path / f"{k}_ema_{tag}.pth")
    elif ema is not None and tag == "final":
        print("EMA: no generator step ran at or after --ema_start_iter, so no gen_*_ema_final.pth is written", flush=True)


def epoch_batches(args, epoch, data_size, rank, world_size, gperm, device):
    """Index tensors (idx_A, idx_B) of every batch of this epoch, in order (see the module docstring)."""
    bs = args.batch_size
    if world_size > 1:
        from .dp import distributed_indices
        idx = torch.tensor(distributed_indices(data_size, world_size, rank, epoch, seed=0), device=device)
        out = [(idx[i:i + bs], idx[i:i + bs]) for i in range(0, len(idx), bs)]
        return [b for b in out if len(b[0]) >= 2]
    perm_A = torch.randperm(data_size, generator=gperm).to(device)     # shuffle_data, dataset.py:24-35
    perm_B = torch.randperm(data_size, generator=gperm).to(device)
    return [(perm_A[i * bs:(i + 1) * bs], perm_B[i * bs:(i + 1) * bs]) for i in range(data_size // bs)]


def batches_per_epoch(args, data_size, world_size):
    if world_size > 1:
        shard = -(-data_size // world_size)
        n = -(-shard // args.batch_size)
        return n - 1 if shard % args.batch_size == 1 else n
    return data_size // args.batch_size


def check_eval_swd(args):
    """--eval_swd scores at the evaluation events, so it needs --eval_interval."""
    on = bool(getattr(args, "eval_swd", False))
    if on and int(getattr(args, "eval_interval", 0) or 0) <= 0:
        raise ValueError("--eval_swd scores at the evaluation events: it needs --eval_interval > 0")
    return on


def train(args, trainer=None, rank=0, world_size=1, is_main=True, process_group=None):
    if args.task_name not in TASKS:
        raise ValueError(f"unknown task_name {args.task_name}; choose from {TASKS}")
    aug = augment_of(args, rank)                          # a mistyped --augment token or a scale below 1 raises before anything is built
    image_pool = check_image_pool(getattr(args, "image_pool", 0))           # likewise: a negative --image_pool
    diffaug = check_diffaug(getattr(args, "diffaug", ""))                   # likewise: an unknown --diffaug policy
    diffaug_p, ada = check_ada(diffaug, getattr(args, "diffaug_p", None), getattr(args, "ada_target", 0.0),     # likewise: --ada_target or
                               getattr(args, "ada_interval", 4), getattr(args, "ada_kimg", 500.0),             # --diffaug_p without --diffaug
                               getattr(args, "ada_p_max", 1.0), batch=args.batch_size, world=world_size)
    recon_loss = getattr(args, "recon_loss", "mse")                         # likewise: an SSIM criterion on images under 11 pixels
    recon_ms_scales = getattr(args, "recon_ms_scales", 0)
    recon_w = check_recon_loss(recon_loss, getattr(args, "recon_ssim_alpha", 0.84), args.image_size, recon_ms_scales)
    gan_loss, gan_real_label = check_gan_loss(getattr(args, "gan_loss", "bce"), getattr(args, "gan_real_label", 1.0))   # likewise: hinge with smoothing
    eval_interval = int(getattr(args, "eval_interval", 0) or 0)
    eval_swd = check_eval_swd(args)                                       # likewise: --eval_swd without --eval_interval
    if eval_interval > 0:
        from . import evaluate
        evaluate.check_size(args.image_size, swd=eval_swd)
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: this implementation has no CPU path (use the reference for CPU runs)")
    device = torch.device("cuda", torch.cuda.current_device())
    result_path, model_path = run_dirs(args)
    if is_main:
        result_path.mkdir(parents=True, exist_ok=True)
        model_path.mkdir(parents=True, exist_ok=True)
    if trainer is None:
        trainer = DiscoGANTrainer(args, device=device, image_size=args.image_size, seed=args.seed,
                                  process_group=process_group, use_graph=not args.no_graph,
                                  mfma_dtype=getattr(args, "mfma_dtype", "f32"), act_dtype=getattr(args, "act_dtype", "f32"),
                                  comm=getattr(args, "comm", "auto"))
    data, data_kind = open_data(args, device, rank, world_size)
    data_size = data.size
    if is_main:
        print(f"data source: {data_kind} ({data_size} images per domain)", flush=True)
        if aug is not None:
            from . import dataset as ds
            parts = ([f"random {args.image_size} x {args.image_size} window"] if aug.flags & ds.AUG_TOKENS["crop"] else []) \
                + (["random mirror"] if aug.flags & ds.AUG_TOKENS["flip"] else [])
            print(f"augmentation: {ds.augment_name(aug.flags)} on the training data (prepared at L = {aug.size(args.image_size)}, "
                  + ", ".join(parts) + "; keyed on seed, rank and iteration; held-out data is never augmented)", flush=True)
        if image_pool > 0:
            print(f"image pool: {image_pool} images per domain ({image_pool * 3 * args.image_size ** 2 * 4 / 2 ** 20:.1f} MiB each) for the "
                  "discriminator steps; keyed on seed, rank and iteration; generator steps and reconstructions see the newest fakes",
                  flush=True)
        if diffaug:
            from .diffaug import policy_names
            print(f"differentiable augmentation: {policy_names(diffaug)} on every discriminator input (reals and fakes, every step); "
                  "keyed on seed, rank and iteration; generators, reconstructions, samples and evaluation never see it", flush=True)
            if ada is not None:
                print(f"ADA: each stage with probability p, from {diffaug_p:g} within [0, {ada['p_max']:g}], moved on the device every "
                      f"{ada['interval']} discriminator steps towards r_t = {ada['target']:g} ({ada['kimg']:g} kimg from 0 to 1)", flush=True)
            elif diffaug_p is not None:
                print(f"differentiable augmentation: each stage applied to a sample with probability {diffaug_p:g}", flush=True)
        if recon_loss in MS_SSIM_KINDS:
            print(f"reconstruction loss: {recon_loss} = {recon_w[0]:g} MSE + {recon_w[1]:g} L1 + {recon_w[2]:g} (1 - MS-SSIM over "
                  f"{recon_ms_scales_of(recon_loss, args.image_size, recon_ms_scales)} scales) on both cycle terms (RECON: prints its value)",
                  flush=True)
        elif recon_loss != "mse":
            print(f"reconstruction loss: {recon_loss} = {recon_w[0]:g} MSE + {recon_w[1]:g} L1 + {recon_w[2]:g} (1 - SSIM) on both cycle "
                  "terms (RECON: prints its value)", flush=True)
        if gan_loss != "bce" or gan_real_label != 1.0:
            print(f"adversarial loss: {gan_loss} (real label {gan_real_label:g})", flush=True)
    # the held-out split of the sample grids (samples.py) and of the evaluation (evaluate.py), resident on the device for the run; the
    # saving rank alone loads it, samples and evaluates
    split = None
    if is_main:
        from . import samples
        split = samples.load_split(args, data_kind, device, world_size)
    eval_paired = eval_interval > 0 and evaluate.paired_default(args, data_kind)
    swd = None
    if eval_swd and split is not None:
        # the real sets' sorted projections, once; SWD(test_A, test_B) is the gap a translation has to close, the same all run long
        swd, domains = evaluate.make_swd_pair(*split, args.image_size, int(getattr(args, "eval_swd_seed", 0)))
        print(f"SWD_DOMAINS: {evaluate.format_swd(domains)} (n={domains['n']}, {domains['patches']} patches per image)", flush=True)
    n_batches = batches_per_epoch(args, data_size, world_size)
    if n_batches < 1:
        raise ValueError(f"batch_size {args.batch_size} leaves no full batch in {data_size} images on {world_size} rank(s)")
    total_iterations = args.epochs * n_batches
    log_file = result_path / "training_log.txt"
    if is_main:
        with open(log_file, "w") as f:
            f.write(f"Task: {args.task_name}, Model: {args.model_arch}\n")
            f.write(f"Batch size: {args.batch_size}, Learning rate: {args.learning_rate}\n\n")
    iters = 0
    start_epoch = start_batch = 0
    if getattr(args, "resume", None):
        st = torch.load(args.resume, map_location="cpu")
        iters = trainer.load_train_state(st)
        # position in the data order: the state's loader record, else derived from the iteration count
        pos = st.get("loader") or dict(epoch=iters // n_batches, batch=iters % n_batches)
        start_epoch, start_batch = int(pos["epoch"]), int(pos["batch"])
        if start_batch >= n_batches:
            start_epoch, start_batch = start_epoch + 1, 0
        if is_main:
            print(f"resumed from {args.resume}: next iteration {iters} (epoch {start_epoch}, batch {start_batch})")
    start_iters = iters
    t0 = time.time()
    lazy = bool(getattr(args, "skip_log_only_passes", False))
    gperm = torch.Generator(device="cpu").manual_seed(args.seed + 17 * rank)
    if world_size == 1:
        for _ in range(start_epoch):                      # replay the generator to the resumed epoch (2 draws per epoch)
            torch.randperm(data_size, generator=gperm)
            torch.randperm(data_size, generator=gperm)
    done = False
    for epoch in range(start_epoch, args.epochs):
        batches = epoch_batches(args, epoch, data_size, rank, world_size, gperm, device)
        first = start_batch if epoch == start_epoch else 0
        for i, (A, B) in enumerate(data.epoch(batches, first, iters), start=first):
            logging = iters % args.log_interval == 0
            out = trainer.train_iteration(A, B, iters, need_losses=logging or not lazy)
            if is_main and logging:
                msg = trainer.format_log(iters, total_iterations, out)
                dt = time.time() - t0
                print(msg + f"  [{(iters - start_iters + 1) * args.batch_size * world_size / max(dt, 1e-9):.1f} img/s]", flush=True)
                with open(log_file, "a") as f:
                    f.write(msg + "\n")
            sampling = split is not None and args.image_save_interval > 0 and iters % args.image_save_interval == 0
            evaluating = split is not None and eval_interval > 0 and iters % eval_interval == 0
            if sampling or evaluating:
                # before the model save of the same iteration (image_translation.py:411-424): the passes move the generators' BatchNorm
                # running statistics, and a checkpoint written at `iters` carries them; they run once for both events
                # --ema_samples: on the EMA weights once there are any; the context puts weights and running statistics back
                on_ema = bool(getattr(args, "ema_samples", False)) and getattr(trainer, "ema", None) is not None and trainer.ema.ready
                with (trainer.ema_weights() if on_ema else contextlib.nullcontext()):
                    outs = trainer.sample(*split)
                if sampling:
                    samples.save_samples(trainer, split, result_path / "samples", iters, outs=outs)
                if evaluating:
                    res, _ = evaluate.evaluate_split(trainer, split, eval_paired, outs=outs, swd=swd,
                                                     ms_ssim=bool(getattr(args, "eval_ms_ssim", False)))
                    msg = evaluate.format_eval(iters, res) + (" [ema]" if on_ema else "")
                    print(msg, flush=True)
                    with open(result_path / "eval_log.txt", "a") as f:
                        f.write(msg + "\n")
            if is_main and iters % args.model_save_interval == 0:
                save_models(trainer, model_path, str(iters), iters + 1, getattr(args, "save_train_state", False),
                            loader=dict(epoch=epoch, batch=i + 1))
            iters += 1
            if args.max_iters and iters >= args.max_iters:
                done = True
                break
        if done:
            break
    if is_main:
        save_models(trainer, model_path, "final", iters, getattr(args, "save_train_state", False),
                    loader=dict(epoch=iters // n_batches, batch=iters % n_batches))
        print(f"Training completed. Final models saved to {model_path}")
        print(f"Results and logs saved to {result_path}")
    train.last_paths = (result_path, model_path)
    return trainer


def main(argv=None):
    args = parse_args(argv)
    return train(args)


if __name__ == "__main__":
    main()
