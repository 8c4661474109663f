"""The DiscoGAN training iteration, re-hosted on the HIP kernels.

Mirrors the loop body of the reference (image_translation.py:336-390; DDP variant
distributed_image_translation.py:466-518): 4 generator passes, 2 reconstruction losses, 4
discriminator passes, GAN + feature-matching losses, the curriculum loss mix, then backward + Adam
of ONE side (D when ``iters % update_interval == 0`` else G).

Differences that do not change any result:
  * dead backward work is skipped: in a D-step the generators run without an autograd graph and the
    fakes are detached; in a G-step the discriminator parameters are frozen, so no D weight-grads
    and no backward through the real passes.  The reference computes those and discards them.
  * data parallelism averages ONLY the stepped side's flat gradient buffer (RCCL all-reduce: one message, or one
    per gradient bucket when the exchange is overlapped with the backward pass), never broadcasts BatchNorm
    buffers (the reference's per-forward broadcast is what makes its DDP backward raise), and keeps BN /
    feature-matching statistics rank-local like DDP does.
  * steady-state iterations replay a captured hipGraph (zero_grad + forward + backward) instead of
    re-dispatching ~600 kernels from Python.
  * the A-side chain (G_A, D_A) and the B-side chain (G_B, D_B) run on two HIP streams and are issued layer by
    layer in lock step (``forward_steps`` generators); every loss term lands in one device vector and the
    curriculum mix / its gradient seeds are one kernel each.
  * ``need_losses=False`` (opt-in, ``--skip_log_only_passes``): a D-step skips the two reconstruction passes,
    which feed only the log line there.  Weights and optimiser state are unaffected, but the generators' BatchNorm
    running statistics then see one forward per D-step instead of two, so saved ``gen_*.pth`` buffers (used by
    eval-mode inference) differ from the reference's; the default keeps the reference's full work.
"""
from __future__ import annotations

import contextlib
import numbers
from itertools import chain
from types import SimpleNamespace

import torch

from . import dp
from . import functional as F_
from . import losses as L
from . import ops
from . import optim
from .model import Discriminator, Generator, group_discriminators, group_generators
from .pool import ImagePool
from .diffaug import AdaController, DiffAugment, apply_group, fixed_p, format_ada_suffix, parse_policy

LOG_KEYS = ("gen_loss_A", "gen_loss_B", "fm_loss_A", "fm_loss_B", "recon_loss_A", "recon_loss_B",
            "dis_loss_A", "dis_loss_B", "gen_loss", "dis_loss")

DEFAULTS = dict(learning_rate=2e-4, beta1=0.5, beta2=0.999, weight_decay=0.00001, gan_curriculum=10000,
                starting_rate=0.01, default_rate=0.5, update_interval=3, model_arch="discogan",
                ema_decay=0.0, ema_start_iter=0, grad_clip=0.0, nonfinite_guard=False, log_grad_norm=False, image_pool=0,
                diffaug="", recon_loss="mse", recon_ssim_alpha=0.84, recon_ms_scales=0, gan_loss="bce", gan_real_label=1.0,
                diffaug_p=None, ada_target=0.0, ada_interval=4, ada_kimg=500.0, ada_p_max=1.0)

# The loss vector every term of an iteration is written into and dg_loss_mix_fwd / _bwd read (the layout is defined by the comment
# above dg_loss_mix_fwd in include/discogan_hip.h): the two reconstruction terms, per discriminator BCE(real, 1), BCE(fake, 0),
# BCE(fake, 1), then the nfm feature-matching layers of D_A from FM0 and those of D_B from FM0 + nfm.
RECON_A, RECON_B = 0, 1
A_REAL1, A_FAKE0, A_FAKE1, B_REAL1, B_FAKE0, B_FAKE1 = 2, 3, 4, 5, 6, 7
FM0 = 8
MIX_KEYS = ("gen_loss_A", "gen_loss_B", "fm_loss_A", "fm_loss_B", "dis_loss_A", "dis_loss_B", "gen_loss", "dis_loss")     # its out8
WHICH_GEN, WHICH_DIS = 6, 7                # dg_loss_mix_bwd's ``which``: backward of gen_loss (out8[6]) / of dis_loss (out8[7])
ARCH_CODES = {"discogan": 0, "recongan": 1, "gan": 2}
D_REAL, D_FAKE, G_FAKE = ops.GAN_D_REAL, ops.GAN_D_FAKE, ops.GAN_G_FAKE         # the role of a GAN term (DG_GAN_*): which target it is held to
PREC_OF = {"f32": ops.PREC_F32, "bf16": ops.PREC_BF16, "f32x3": ops.PREC_F32X3}


def loss_slots(model_arch, dstep, nfm):
    """``(arch_code, which, idx)`` of a D-step / G-step: the library's code of ``model_arch``, which mixed loss is differentiated, and the
    slots of the loss vector that carry gradient then (image_translation.py:374-382): discogan both sides; recongan D_B | recon_A +
    G_B's GAN and feature-matching terms; gan D_B | G_B's.  Raises ValueError for an unknown ``model_arch``."""
    arch = ARCH_CODES.get(model_arch)
    if arch is None:
        raise ValueError(f"unknown model_arch {model_arch}")
    if dstep:
        return arch, WHICH_DIS, ((A_REAL1, A_FAKE0, B_REAL1, B_FAKE0) if arch == 0 else (B_REAL1, B_FAKE0))
    fmA, fmB = tuple(range(FM0, FM0 + nfm)), tuple(range(FM0 + nfm, FM0 + 2 * nfm))
    return arch, WHICH_GEN, ((RECON_A, RECON_B, A_FAKE1, B_FAKE1) + fmA + fmB, (RECON_A, B_FAKE1) + fmB, (B_FAKE1,) + fmB)[arch]


def check_ema_decay(decay):
    """``ema_decay``: 0 = no EMA of the generator weights, else a decay in (0, 1).  Returns it as a float."""
    decay = float(decay)
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"ema_decay must be 0 (off) or in (0, 1), got {decay}")
    return decay


def check_grad_clip(grad_clip):
    """``grad_clip``: 0 = no clipping, else the bound on the global gradient norm of a step.  Returns it as a float."""
    grad_clip = float(grad_clip)
    if not grad_clip >= 0.0:
        raise ValueError(f"grad_clip must be 0 (off) or a positive norm bound, got {grad_clip}")
    return grad_clip


def check_image_pool(size):
    """``image_pool``: 0 = no history pool of generated images, else the number of image slots per domain (50 is customary).  Returns it
    as an int."""
    if isinstance(size, bool) or not isinstance(size, numbers.Integral) or size < 0:
        raise ValueError(f"image_pool must be an integer >= 0 (0 = off), got {size!r}")
    return int(size)


def check_diffaug(policy):
    """``diffaug``: "" (or "none") = off, else a comma-separated subset of color, translation, cutout (diffaug.parse_policy).  Returns the
    DG_DIFFAUG_* flags; raises ValueError on an unknown name."""
    return parse_policy(policy)


ADA_WINDOW_LIMIT = 2 ** 24      # a window's two float32 fields are integer-valued: exact below this


def check_ada(diffaug_flags, diffaug_p=None, ada_target=0.0, ada_interval=4, ada_kimg=500.0, ada_p_max=1.0, batch=None, world=1):
    """The probability of the differentiable augmentation and its controller.  ``diffaug_p``: the probability every stage is applied to a
    sample with, in [0, 1]; None = 1.0 without a controller, 0.0 (the initial p) with one.  ``ada_target``: 0 = no controller, else the
    target of r_t = E[sign(D(real))] in (0, 1) (0.6 is customary) that p is moved by: every ``ada_interval`` discriminator steps, by
    (real images of the window) / (1000 ``ada_kimg``), within [0, ``ada_p_max``].  Both need a ``diffaug`` policy.  ``batch`` (if known):
    ``ada_interval x batch x world`` must stay below 2^24, where the window's float32 counters are exact.

    Returns ``(p, ada)``: ``p`` None = dg_diffaug_draw (every stage on every sample) or the fixed / initial probability; ``ada`` None or
    ``dict(target=, interval=, kimg=, p_max=)``."""
    target = float(ada_target or 0.0)
    if not (target == 0.0 or 0.0 < target < 1.0):
        raise ValueError(f"ada_target must be 0 (off) or lie in (0, 1) (0.6 is customary), got {ada_target!r}")
    if diffaug_p is not None:
        diffaug_p = float(diffaug_p)
        if not 0.0 <= diffaug_p <= 1.0:
            raise ValueError(f"diffaug_p must lie in [0, 1], got {diffaug_p}")
    if not diffaug_flags:
        if target != 0.0:
            raise ValueError("ada_target moves the probability of the differentiable augmentation: it needs a diffaug policy")
        if diffaug_p is not None:
            raise ValueError("diffaug_p is the probability of the differentiable augmentation: it needs a diffaug policy")
        return None, None
    if target == 0.0:
        return (None if diffaug_p is None or diffaug_p == 1.0 else diffaug_p), None
    if isinstance(ada_interval, bool) or not isinstance(ada_interval, numbers.Integral) or ada_interval < 1:
        raise ValueError(f"ada_interval must be an integer >= 1 (discriminator steps per update), got {ada_interval!r}")
    kimg, p_max = float(ada_kimg), float(ada_p_max)
    if not 1e-3 <= kimg < float("inf"):
        raise ValueError(f"ada_kimg must be >= 0.001 (thousands of real images for p to travel from 0 to 1), got {ada_kimg!r}")
    if not 0.0 < p_max <= 1.0:
        raise ValueError(f"ada_p_max must lie in (0, 1], got {ada_p_max!r}")
    if batch is not None and int(ada_interval) * int(batch) * int(world) >= ADA_WINDOW_LIMIT:
        raise ValueError(f"ada_interval x batch x world = {int(ada_interval) * int(batch) * int(world)} real images per window: the "
                         f"window counters are exact below 2^24 only")
    return (0.0 if diffaug_p is None else diffaug_p), dict(target=target, interval=int(ada_interval), kimg=kimg, p_max=p_max)


def ada_threshold(gan_loss, gan_real_label=1.0):
    """Where a discriminator's output changes sides for r_t: 0.5 on the sigmoid outputs of "bce", half the real target for "lsgan", 0 on
    the logits of "bce_logits" and "hinge"."""
    return {"bce": 0.5, "lsgan": float(gan_real_label) / 2.0}.get(gan_loss, 0.0)


def check_recon_loss(kind, alpha, image_size, ms_scales=0):
    """``recon_loss``: the criterion of the two reconstruction (cycle) terms -- "mse" (the reference's nn.MSELoss), "l1", "ssim" (1 - SSIM)
    or "l1_ssim" ((1 - alpha) L1 + alpha (1 - SSIM), ``recon_ssim_alpha`` in (0, 1), read by that kind only), and their multi-scale forms
    "ms_ssim" and "l1_ms_ssim" (MS-SSIM over ``ms_scales`` scales, 0 = as many as the size carries; read by those kinds only).  The SSIM
    kinds need images of at least 11 pixels (the 11 x 11 window), at every scale.  Returns the weights (w_mse, w_l1, w_ssim)
    (losses.recon_weights); ``recon_ms_scales`` gives the scale count."""
    w = L.recon_weights(kind, alpha)
    if w[2] > 0.0 and image_size < 11:
        raise ValueError(f"recon_loss {kind!r} needs image_size >= 11 (the 11 x 11 SSIM window), got {image_size}")
    recon_ms_scales(kind, image_size, ms_scales)
    return w


def recon_ms_scales(kind, image_size, ms_scales=0):
    """The scale count M of the criterion ``kind`` at ``image_size`` (0 for the kinds that have no pyramid); ValueError for a count the
    size cannot carry."""
    return L.ms_ssim_scales(ms_scales, image_size) if kind in L.MS_SSIM_KINDS else 0


# ``gan_loss`` / ``gan_real_label``: the objective of the six GAN terms -- "bce" (the reference's nn.BCELoss on the sigmoid output) or, on the
# discriminators' logits, "bce_logits", "lsgan", "hinge" -- and the target of a discriminator's real batch, in (0.5, 1] (1 with the hinge).
check_gan_loss = L.check_gan_loss


def format_grad_suffix(dis, gen):
    """The log suffix of gradient control from the two optimisers' ``grad_stats()``: each side's norm of its last step, then the
    counters of both sides together."""
    return (f" GRAD: D {dis['norm']:.4e} G {gen['norm']:.4e} clipped {dis['clipped'] + gen['clipped']}/{dis['steps'] + gen['steps']}"
            f" skipped {dis['skipped'] + gen['skipped']}")


class IterationOutputs(SimpleNamespace):
    """What ``forward_losses`` / ``train_iteration`` return: the loss scalars and the tensors of the iteration as attributes, plus
    ``BA_seen`` / ``AB_seen`` = the fake batches the discriminators were given -- ``BA`` / ``AB`` themselves unless a history pool
    exchanged them (``seen``: None, or ``dict(BA=, AB=)`` of a pooled D-step).  The two are properties, not attributes of their own:
    whatever enumerates the returned tensors (``vars(out)``: bench.py --dump-outputs) finds the same set with and without the feature.
    ``dis_inputs``: None, or with differentiable augmentation ``dict(A=, BA=, B=, AB=)`` = the augmented batches the discriminators read
    (a dict for the same reason)."""

    @property
    def BA_seen(self):
        return self.BA if self.seen is None else self.seen["BA"]

    @property
    def AB_seen(self):
        return self.AB if self.seen is None else self.seen["AB"]


def default_args(**over):
    d = dict(DEFAULTS)
    d.update(over)
    return SimpleNamespace(**d)


class DiscoGANTrainer:
    def __init__(self, args=None, device="cuda", image_size=64, seed=1234, process_group=None,
                 use_graph=False, skip_dead_work=True, two_streams=True, overlap_comm=None, mfma_dtype="f32", comm="auto",
                 bucket_mb=128.0, act_dtype="f32", x3_planes=None, group_launch=None, group_plan="launch"):
        self.args = args or default_args()
        for k, v in DEFAULTS.items():
            if not hasattr(self.args, k):
                setattr(self.args, k, v)
        ema_decay = check_ema_decay(self.args.ema_decay)
        grad_clip = check_grad_clip(self.args.grad_clip)
        self.recon_loss = self.args.recon_loss
        self.recon_w = check_recon_loss(self.recon_loss, self.args.recon_ssim_alpha, image_size, self.args.recon_ms_scales)
        self.recon_ms = recon_ms_scales(self.recon_loss, image_size, self.args.recon_ms_scales)      # M; 0: a single-scale kind
        self.gan_loss, self.gan_real_label = check_gan_loss(self.args.gan_loss, self.args.gan_real_label)
        guard, log_norm = bool(self.args.nonfinite_guard), bool(self.args.log_grad_norm)
        loss_slots(self.args.model_arch, True, 0)        # an unknown model_arch is refused here, before anything is allocated
        self.device = torch.device(device)
        self.image_size = image_size
        self.pg = process_group
        self.world_size = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        rank = torch.distributed.get_rank(process_group) if process_group is not None else 0
        stream_seed = 0 if seed is None else seed         # with the rank: the key of the pool's and DiffAugment's device-side draws
        # exchange transport (dp.ExchangeGroup): "capi" = the library's own RCCL communicator (collectives on the
        # caller's stream), "c10d" = torch.distributed, "auto" = capi under backend nccl.  comm="capi" may be forced at
        # world size 1 (tests: the whole exchange path runs against a 1-rank RCCL communicator).
        self.xg = None
        if self.world_size > 1 or comm == "capi":
            self.xg = dp.ExchangeGroup(process_group, transport=comm, device=torch.device(device))
        self.time_comm = False                            # bench: HIP events around every exchange
        self.comm_events = {"D": [], "G": []}
        self.comm_steps = {"D": 0, "G": 0}
        self.use_graph = use_graph
        self.skip_dead_work = skip_dead_work
        if seed is not None:
            torch.manual_seed(seed)                      # distributed_image_translation.py:372
        # construction order G_A, G_B, D_A, D_B on the host RNG (identical replicas on every rank)
        self.generator_A = Generator(extra_layers=True, image_size=image_size).to(self.device)
        self.generator_B = Generator(extra_layers=True, image_size=image_size).to(self.device)
        self.discriminator_A = Discriminator(image_size=image_size).to(self.device)
        self.discriminator_B = Discriminator(image_size=image_size).to(self.device)
        self.nets = dict(gen_A=self.generator_A, gen_B=self.generator_B,
                         dis_A=self.discriminator_A, dis_B=self.discriminator_B)
        # The criterion of the two reconstruction terms (slots 0 and 1 of the loss vector).  "mse": the reference's, through MSELossFn /
        # MSELossGroupFn as ever.  Any other kind: one fused kernel pair per term (functional.ReconLossFn / ReconLossGroupFn,
        # csrc/recon.hip) in the same places on the same streams, capturable, stateless -- nothing to checkpoint or to exchange.  The
        # multi-scale kinds likewise, through MsSsimLossFn / MsSsimLossGroupFn (csrc/msssim.hip) over ``recon_ms`` scales.
        if self.recon_ms:
            self.recon_criterion = L.MSSSIMLoss(self.recon_loss, self.args.recon_ssim_alpha, self.recon_ms)
        else:
            self.recon_criterion = L.MSELoss() if self.recon_loss == "mse" else L.ReconLoss(self.recon_loss, self.args.recon_ssim_alpha)
        # The objective of the six GAN terms (slots A_REAL1 .. B_FAKE1).  "bce": the reference's -- the discriminators end in their sigmoid
        # and BCELossFn / BCELossGroupFn read it, as ever (gan_real_label only replaces the label 1 of the two *_REAL1 terms).  Any other
        # kind: the discriminators return their head conv's LOGITS (no sigmoid launch) and GanLossFn / GanLossGroupFn (csrc/ganloss.hip)
        # write the same slots in the same places on the same streams: capturable, stateless, nothing to checkpoint or to exchange.
        self.gan_kind = None if self.gan_loss == "bce" else L.GAN_KIND_CODES[self.gan_loss]
        self.gan_criterion = L.BCELoss() if self.gan_kind is None else L.GANLoss(self.gan_loss, self.gan_real_label)
        self.feat_criterion = L.HingeEmbeddingLoss()
        a = self.args
        self.optim_gen = optim.Adam(chain(self.generator_A.parameters(), self.generator_B.parameters()),
                                    lr=a.learning_rate, betas=(a.beta1, a.beta2), weight_decay=a.weight_decay)
        self.optim_dis = optim.Adam(chain(self.discriminator_A.parameters(), self.discriminator_B.parameters()),
                                    lr=a.learning_rate, betas=(a.beta1, a.beta2), weight_decay=a.weight_decay)
        # Exponential moving average of both generators' weights (ema_decay > 0; optim.EMA): a second flat buffer, updated by one
        # launch behind every generator Adam step from iteration ema_start_iter on -- eagerly on the main stream, never captured.
        # Sampling, evaluation and the gen_*_ema_*.pth checkpoints read it (ema_weights / ema_state_dicts); training never does.
        self.ema = optim.EMA(self.optim_gen, ema_decay) if ema_decay > 0.0 else None
        # Gradient control (grad_clip > 0, nonfinite_guard or log_grad_norm; optim.Adam.enable_grad_control): every step of either side
        # measures the global norm of its gradient on the device, clips by it and / or skips the step when the gradient is not finite,
        # without a host round trip.  A global norm needs the WHOLE gradient before the first Adam slice, so the schedules that step
        # the generators slice by slice while the backward still runs (_GradBuckets, the split backward of overlap_comm="graph") are
        # not used then: a G-step is backward, one all-reduce, statistics, step.  The D-step's hand-over to the communication stream
        # stays.  The norm is taken behind the all-reduce, so every rank decides alike.  A skipped step leaves weights, moments, step
        # count and derived operand forms untouched; the forward passes of that iteration have run, so BatchNorm running statistics
        # have moved, and the EMA update behind a skipped G-step runs on unchanged weights (p == ema stays put, else the usual lerp).
        self.grad_control = grad_clip > 0.0 or guard or log_norm
        if self.grad_control:
            self.optim_gen.enable_grad_control(grad_clip, guard)
            self.optim_dis.enable_grad_control(grad_clip, guard)
        # History pool of generated images (image_pool = P > 0; pool.ImagePool): in a D-step -- and only there -- D_A is trained on
        # pool_BA.exchange(BA) and D_B on pool_AB.exchange(AB), a mix of this iteration's fakes and earlier ones, instead of BA / AB.  The
        # two record tables are drawn on the device ahead of the iteration's dispatch, outside any capture (_draw_ahead), keyed on
        # (seed, data-parallel rank, iteration, domain): every rank pools its own fakes, and a resumed run continues the sequence.  Each
        # exchange is ONE launch on the stream of the discriminator pass that consumes it, reading only fixed device addresses, so it is
        # captured like any other kernel.  G-steps, the reconstruction passes and sampling never see a pool.
        P = check_image_pool(self.args.image_pool)
        self.pool_BA = self.pool_AB = None
        if P > 0:
            self.pool_BA = ImagePool(P, image_size, stream_seed, rank, 0, device=self.device)      # domain A: the fakes D_A sees
            self.pool_AB = ImagePool(P, image_size, stream_seed, rank, 1, device=self.device)      # domain B: the fakes D_B sees
        # Differentiable augmentation (diffaug = a policy; diffaug.DiffAugment): everything a discriminator reads -- reals and fakes, in
        # D-steps and G-steps -- goes through one random transform per sample first, behind the pool exchange and on the consumer's
        # stream; in a G-step the gradient flows back through it into the generator.  Four tables (A real, A fake, B real, B fake), drawn
        # on the device ahead of EVERY iteration's dispatch, outside any capture (_draw_ahead), keyed on (seed, data-parallel rank,
        # iteration, domain, role): nothing to checkpoint.  Generators, reconstruction passes, sampling, evaluation and the EMA never
        # see the transform.
        self.diffaug_flags = check_diffaug(self.args.diffaug)
        # The probability of the transform (diffaug_p) and its controller (ada_target > 0; diffaug.AdaController: Karras et al. 2020).
        # Every stage is applied to a sample with probability p, which the draw kernel reads from device memory: a constant, or the
        # first field of the domain's control block -- aug_A and aug_BA (what D_A reads) share p_A, aug_B and aug_AB share p_B.  With a
        # controller every discriminator step adds the signs of its own A_dis_real / B_dis_real against ada_threshold to the domain's
        # window, and every ada_interval-th closes both windows (one 16-byte all-reduce of them under data parallelism) and moves p:
        # eager launches directly behind that step's gradient exchange and Adam, on the same stream (_ada_step), never captured, never
        # read by the host; the next iteration's draws are ordered behind them (_draw_ahead).  The captured graphs read the record
        # tables only, so no graph key changes.  Unset (diffaug_p None or 1.0, ada_target 0): dg_diffaug_draw as ever.
        p0, ada = check_ada(self.diffaug_flags, self.args.diffaug_p, self.args.ada_target, self.args.ada_interval, self.args.ada_kimg,
                            self.args.ada_p_max)
        self.ada = None
        self._ada_real = self._ev_ada = None               # a D-step's real outputs until its apply_step; the event behind the update
        self.ada_threshold = ada_threshold(self.gan_loss, self.gan_real_label)
        self.aug_A = self.aug_BA = self.aug_B = self.aug_AB = None
        if self.diffaug_flags:
            p_of = (None, None)
            if ada is not None:
                self.ada = AdaController(ada["target"], ada["interval"], ada["kimg"], ada["p_max"], p0, device=self.device)
                p_of = (self.ada.p_view(0), self.ada.p_view(1))
            elif p0 is not None:
                p_of = (fixed_p(p0, self.device),) * 2
            mk = lambda domain, role: DiffAugment(self.diffaug_flags, image_size, stream_seed, rank, domain, role,  # noqa: E731
                                                  device=self.device, p=p_of[domain])
            self.aug_A, self.aug_BA, self.aug_B, self.aug_AB = mk(0, 0), mk(0, 1), mk(1, 0), mk(1, 1)
        self._graphs = {}
        self._static = None
        # The A-side chain (G_A, D_A) runs on a second HIP stream next to the B-side chain (G_B, D_B):
        # the two are independent except for two hand-overs (AB -> G_A, BA -> G_B), so prologues and
        # tails of one chain's kernels overlap the other chain's kernels.  Every network stays on ONE
        # stream, which keeps its two calls per iteration (and its BN running-stat updates) ordered.
        self.two_streams = two_streams
        self.side_stream = torch.cuda.Stream(device=self.device) if two_streams else None
        # (Round 1-2 experiments on top of the two streams -- CU-masked streams per chain, turn taking on the matrix cores, a phase skew
        # between the chains, weight gradients on a third stream -- all measured slower or equal and were
        # removed in round 4.)
        # mfma_dtype "bf16": the interior conv GEMMs round their operands to bf16 and run on the bf16 matrix path
        # with fp32 accumulation (BASELINE configs[4]); tensors, BatchNorm, losses, master weights, Adam stay fp32.
        # "f32x3": fp32-accurate products on the bf16 matrix path -- every operand is split into three bf16 planes
        # (24 significand bits), six MFMAs per product block, fp32 accumulation (csrc/igemm.hip PREC 2).
        # Passed to the library with every call (self.ctx below): no process-global option is set.
        if mfma_dtype not in ("f32", "bf16", "f32x3"):
            raise ValueError("mfma_dtype must be 'f32', 'bf16' or 'f32x3'")
        self.mfma_dtype = mfma_dtype
        # bf16 path: the conv kernels read bf16 SHADOWS of their operands written by the producers (ops.SHADOW)
        self.bf16_shadow = mfma_dtype == "bf16"
        # act_dtype "bf16" (needs mfma_dtype "bf16"): feature maps and their gradients are STORED in bf16 only -- the conv
        # epilogues round the fp32 accumulators once, BatchNorm reads bf16 and keeps its statistics and arithmetic in
        # fp32 / fp64 (BASELINE configs[4]: "bf16 MFMA + fp32 BatchNorm accum"); 8 / 10 bytes per element and pass instead
        # of 18 / 22.  Images, weights, BatchNorm parameters and buffers, every parameter gradient, losses, Adam: fp32.
        if act_dtype not in ("f32", "bf16"):
            raise ValueError("act_dtype must be 'f32' or 'bf16'")
        if act_dtype == "bf16" and mfma_dtype != "bf16":
            raise ValueError("act_dtype='bf16' needs mfma_dtype='bf16'")
        self.act_dtype = act_dtype
        if self.bf16_shadow:
            self.optim_gen.enable_bf16_shadow()
            self.optim_dis.enable_bf16_shadow()
        # f32x3 path: the conv kernels read the three bf16 PLANES of their operands, written once per tensor (Adam: weights;
        # ops.planes_of: activations and gradients) instead of splitting every fp32 value in every conv (ops.X3,
        # csrc/igemm_dma_x3.hip); x3_planes=False keeps the register-staged split everywhere.  None = by size: the planes cost
        # 6 B/element of extra BatchNorm output and a weight transpose per Adam step, which the faster conv kernels repay at
        # 512 px / batch 32 (257 -> 275 images/s) and do not at 64 px / batch 256 (25.0 k -> 23.0 k, same-box A/B) -> on from 256 px
        if x3_planes is None:
            x3_planes = image_size >= 256
        self.x3_planes = mfma_dtype == "f32x3" and bool(x3_planes)
        if self.x3_planes:
            self.optim_gen.enable_x3_planes()
            self.optim_dis.enable_x3_planes()
        # The arithmetic and operand forms of THIS trainer's calls: an ops.Context handed to every op with the call (the conv
        # arithmetic is an argument of the C ABI: DG_PREC_*), never a process-wide switch -- two trainers with different arithmetic
        # can be interleaved call by call (tests/test_group_gpu.py::test_interleaved_trainers_with_different_arithmetic).
        self.ctx = ops.Context(group_plan=group_plan)
        self._refresh_ctx()
        # Grouped launches (round 4): the A-side / B-side pass of every pair of the iteration (image_translation.py:342-346,353-361)
        # goes out as ONE launch per kernel, and in a D-step each discriminator layer's real and fake pass of both sides as one
        # launch over four problems (same weights fetched once per launch; BatchNorm statistics / feature maps per pass).  Bitwise
        # equal to the ungrouped schedule (tests/test_group_gpu.py).  None = where it pays: below 256 px, where the launches are
        # tens of microseconds (64 px / batch 64: ~500 launches per iteration, a third of them under 6 us), on the arithmetics
        # whose operands are plain fp32 tensors (exact fp32, register-staged f32x3) and the symmetric `discogan` architecture.
        # group_plan "launch" (default): the split-K plan of a grouped conv is sized for all its problems together -- fewer slabs per
        # problem, another (fixed) summation order; "single": every problem keeps the plan of its own launch = bitwise the
        # ungrouped step (test_grouped_training_step_is_bitwise_the_ungrouped_one).
        can_group = (mfma_dtype == "f32" or (mfma_dtype == "f32x3" and not self.x3_planes)) and act_dtype == "f32" and \
            self.args.model_arch == "discogan" and skip_dead_work
        # Measured, same box, 64 px, images/s ungrouped -> grouped (tools/ab_group_64.sh): batch 64 12.7 k -> 14.6 k (f32), 15.4 k -> 17.4 k
        # (f32x3); batch 128 16.6 k -> 17.7 k, 21.5 k -> 22.0 k; batch 256 19.3 k -> 19.4 k, 25.7 k -> 24.5 k: with 4x the rows per launch the
        # two-chain schedule's overlap of one chain's BatchNorm under the other's conv is worth more than the saved launches.  So the
        # automatic mode groups a batch of up to group_max_pixels = 128 x 64 x 64 image pixels per domain (decided per call).
        self._group_auto = group_launch is None
        self.group_max_pixels = 128 * 64 * 64
        if group_launch is None:
            group_launch = can_group and image_size < 256
        if group_launch and not can_group:
            raise ValueError("group_launch needs mfma_dtype f32 (or f32x3 without planes), act_dtype f32, model_arch discogan, skip_dead_work")
        self.group_launch = bool(group_launch)
        self._one = torch.ones((), device=self.device, dtype=torch.float32)
        # Data-parallel exchange overlap: after a D-step the all-reduce of the D gradients and the D Adam
        # step run on a communication stream while the NEXT iteration's generator passes run; the
        # discriminator passes wait on the event.  (A G-step's update is needed by the very next kernel,
        # so it stays on the main stream.)  Needs mid-iteration waits -> eager dispatch, which keeps up
        # with the GPU (measured 14.8 ms vs 15.0 ms under graph replay at 64 px / batch 256).
        # Measured on one MI355X at 64 px / 64 per GPU (BASELINE configs[2]'s per-GPU shape): eager dispatch is
        # host-bound there (8.77 ms/step vs 4.86 under hipGraph replay), so the default for small images keeps the
        # captured graph and runs exchange + Adam behind it; from 256 px the kernels are long enough for eager
        # dispatch and the overlapped exchange is the default.
        # overlap_comm="graph" (round 4; default for data-parallel runs below 256 px on the grouped schedule): the exchange overlaps
        # UNDER hipGraph replay.  The iteration is captured as a SEQUENCE of graphs with host-side gaps between them (_SegCapture):
        #   D-step: one graph; behind it all-reduce + Adam of the discriminators go to the communication stream and run under the
        #           NEXT iteration's first graph (zero_grad + G_A(B) | G_B(A)), whose successor waits for them in the gap;
        #   G-step: [zero_grad + stage-1 forward] gap(wait for the D update) [stage-2 + discriminator passes + losses + the backward pass
        #           down to the stage-1 bottleneck] gap(all-reduce + Adam slices of both DECODERS leave on the communication stream)
        #           [backward of the stage-1 encoders]; the encoders' all-reduce + Adam slices are the only exposed part.
        # The backward is cut with two autograd calls (gradients w.r.t. the bottleneck activations, then from there): the kernels write
        # the parameter gradients into the flat buffer as a side effect, so the first call completes every decoder gradient.
        # On the two-chain schedule (from 256 px, or group_launch=False) the same mode has ONE gap: behind G_A(B) | G_B(A), where the two
        # streams meet anyway -- enough for the D-step half (at 512 px the discriminators' Adam is 1.4-2 ms of HBM-bound work that then runs
        # under the next iteration's first generator passes, also on ONE rank); the G-step update stays behind the backward pass.
        if overlap_comm is None:
            overlap_comm = (True if image_size >= 256 else ("graph" if (self.group_launch and use_graph) else False)) if self.world_size > 1 else False
        self.graph_overlap = overlap_comm == "graph"
        if self.graph_overlap and not skip_dead_work:
            raise ValueError("overlap_comm='graph' needs skip_dead_work")
        self.overlap_comm = bool(overlap_comm) and skip_dead_work and not self.graph_overlap
        self.comm_stream = torch.cuda.Stream(device=self.device) if (self.overlap_comm or self.graph_overlap) else None
        self._ev_dis_ready = None
        self._cap = None                                   # the _SegCapture being recorded, if any
        self._split_backward, self._dec_done = True, False
        if self.graph_overlap and self.group_launch:
            self._group_auto = False                       # the backward cut sits in the grouped schedule: grouped at every batch size
        if self.overlap_comm:
            self.use_graph = False
        # G-step exchange overlap: the generators' flat gradient buffer is cut into buckets of whole layers; a
        # bucket is all-reduced (and its Adam slice applied) on the communication stream as soon as the LAST backward
        # pass through its layers has been issued (functional.FINAL_HOOK), while the rest of the backward runs.
        self._buckets = _GradBuckets(self, bucket_mb) if self.overlap_comm else None
        if self.grad_control and self.world_size > 1 and (self._buckets is not None or self.graph_overlap) and \
                torch.distributed.get_rank(process_group) == 0:
            print("gradient control: the global norm needs the whole gradient, so generator steps exchange it as one message behind "
                  "the backward pass (no bucketed / split-backward overlap); discriminator steps still overlap", flush=True)
        self._eager_until = self.args.update_interval      # first cycle runs eagerly (warm-up)

    # ---------------------------------------------------------------------------------------------
    def active_ranges(self, dstep):
        """Networks that receive gradients in this kind of step (image_translation.py:374-382):
        discogan: both of the stepped side; recongan: D_B | G_A+G_B (G_B through recon_A's cycle);
        gan: D_B | G_B only.  Returned as flat ranges of the stepped optimiser (None = all)."""
        arch = self.args.model_arch
        if arch == "discogan":
            return None
        if dstep:
            return self.optim_dis.ranges_of([self.discriminator_B])
        if arch == "gan":
            return self.optim_gen.ranges_of([self.generator_B])
        return None                                       # recongan: ABA = G_A(G_B(A)) reaches both generators

    def is_dis_step(self, iters):
        return iters % self.args.update_interval == 0          # image_translation.py:385

    def rate(self, iters):
        a = self.args
        return a.starting_rate if iters < a.gan_curriculum else a.default_rate   # :367

    def _set_requires_grad(self, dstep):
        if not self.skip_dead_work:
            return
        for p in self.optim_dis.params:
            p.requires_grad_(dstep)

    def forward_losses(self, A, B, iters, need_losses=True):
        """image_translation.py:342-382.  need_losses=False (D-steps only): the reconstruction passes ABA / BAB and their
        terms feed nothing but the log line in a D-step, so they are not computed (recon_loss_* read NaN)."""
        if self.group_launch and (not self._group_auto or A.shape[0] * A.shape[2] * A.shape[3] <= self.group_max_pixels):
            return self._forward_losses_grouped(A, B, iters, need_losses)
        dstep = self.is_dis_step(iters)
        gen_ctx = torch.no_grad if (self.skip_dead_work and dstep) else torch.enable_grad
        main, side, on_side = self._streams()
        # allocated BEFORE the fork so that the side stream's writes are ordered after whatever used this block on the main stream
        nfm, lv, sl, terms = self._loss_vector()
        if self.two_streams:
            side.wait_stream(main)
            # tensors that cross streams tell the caching allocator (a block is otherwise reusable on its
            # allocation stream as soon as the host drops it, while the other stream may still read it)
            for t_ in (A, B, lv):
                t_.record_stream(side)
        # The A-side chain (G_A, D_A) is issued on `side`, the B-side chain (G_B, D_B) on `main`, layer by layer
        # in lock step (model.forward_steps): host issue order A.l1, B.l1, A.l2, B.l2, ...  autograd replays nodes in reverse
        # creation order, so the backward pass is interleaved the same way.

        def pair(gen_a, gen_b):
            ra = rb = pend = object()
            while ra is pend or rb is pend:
                if ra is pend:
                    with on_side():
                        try:
                            next(gen_a)
                        except StopIteration as e:
                            ra = e.value
                if rb is pend:
                    try:
                        next(gen_b)
                    except StopIteration as e:
                        rb = e.value
            return ra, rb

        want_recon = need_losses or not (dstep and self.skip_dead_work)
        # The symmetric two-chain order: G_A(B) | G_B(A), G_A(AB) | G_B(BA), D_A(A) | D_B(B), D_A(BA) | D_B(AB), each pair in lock step.
        # (Round 4 tried a DEPHASED order -- side: D_A(A), G_A(B), G_A(AB), D_A(BA); main: G_B(A), D_B(B), G_B(BA), D_B(AB) -- so that one
        # chain's HBM-bound BatchNorm kernels would meet the other chain's conv kernels instead of its BatchNorm kernels: bitwise
        # neutral, and no faster: 295.0 / 293.9 -> 294.5 / 294.8 images/s (f32x3), 1014.9 -> 1002.8 (bf16), 194.2 -> 192.9 (f32) at
        # 512 px / batch 32, same box, alternating, profiles/r04_ab_dephased_chain_order.txt.  Removed.)
        # stage 1: the two first-stage translations are independent.  Their backward passes are the LAST ones to
        # touch each generator's parameters (autograd replays in reverse), which the bucketed exchange keys on.
        F_.FINAL_PASS = True
        try:
            with gen_ctx():
                BA, AB = pair(self.generator_A.forward_steps(B), self.generator_B.forward_steps(A))
        finally:
            F_.FINAL_PASS = False
        if self.two_streams:
            AB.record_stream(side)
            BA.record_stream(main)
        if self.graph_overlap:
            # a gap between two captured graphs (the wait for the discriminators' update happens there at replay): the chains join
            # in front of it and fork again behind it, which is also the hand-over of AB / BA
            if self.two_streams:
                main.wait_stream(side)
            self._cut("dis_ready")
            if self.two_streams:
                side.wait_stream(main)
        elif self.two_streams:
            ev_ab, ev_ba = torch.cuda.Event(), torch.cuda.Event()
            ev_ab.record(main)
            ev_ba.record(side)
            side.wait_event(ev_ab)                           # G_A(AB) needs AB
            main.wait_event(ev_ba)                           # G_B(BA) needs BA
        self._wait_dis_ready(*((main, side) if self.two_streams else (main,)))       # D parameters updated on the comm stream
        # stage 2 + discriminators.  Every loss term is written into its slot of one device vector (layout:
        # dg_loss_mix_fwd); the mix and its gradient seeds are one launch each instead of ~45 scalar kernels.
        ABA = BAB = None
        if want_recon:
            with gen_ctx():
                ABA, BAB = pair(self.generator_A.forward_steps(AB), self.generator_B.forward_steps(BA))
        else:
            self._no_recon(lv, sl, terms)
        A_in, B_in, dis_inputs = A, B, None
        logits = self.gan_kind is not None                   # an objective on logits: the discriminators skip their sigmoid
        if self.aug_A is not None:                           # the reals as the discriminators see them (no gradient is wanted of them)
            with torch.no_grad():
                with on_side():
                    A_in = self.aug_A.apply(A)
                B_in = self.aug_B.apply(B)
        (A_dis_real, A_feats_real), (B_dis_real, B_feats_real) = pair(
            self.discriminator_A.forward_steps(A_in, logits), self.discriminator_B.forward_steps(B_in, logits))
        # the fakes the discriminators see: in a D-step with a history pool the exchanged batches, each on its consumer's stream (BA was
        # produced on `side`, where D_A runs; AB on `main`, where D_B runs: no new join)
        BA_seen, AB_seen, seen = self._pooled_fakes(dstep, BA, AB, on_side)
        BA_in, AB_in = BA_seen, AB_seen
        if self.aug_A is not None:                           # behind the exchange, each on its consumer's stream; differentiable
            with on_side():
                BA_in = self.aug_BA.apply(BA_seen)
            AB_in = self.aug_AB.apply(AB_seen)
            dis_inputs = dict(A=A_in, BA=BA_in, B=B_in, AB=AB_in)
        (A_dis_fake, A_feats_fake), (B_dis_fake, B_feats_fake) = pair(
            self.discriminator_A.forward_steps(BA_in, logits), self.discriminator_B.forward_steps(AB_in, logits))
        assert nfm == len(A_feats_real)

        def gan(x, role, k):
            terms[k], = self._gan_terms([x], [role], [sl[k]])

        with on_side():
            if want_recon:
                with gen_ctx():
                    terms[RECON_A], = self._recon_terms([ABA], [A], [sl[RECON_A]])
            gan(A_dis_real, D_REAL, A_REAL1); gan(A_dis_fake, D_FAKE, A_FAKE0); gan(A_dis_fake, G_FAKE, A_FAKE1)
            for l, (r, f) in enumerate(zip(A_feats_real, A_feats_fake)):
                terms[FM0 + l] = F_.FeatureMatchFn.apply(r, f, sl[FM0 + l])
        if want_recon:
            with gen_ctx():
                terms[RECON_B], = self._recon_terms([BAB], [B], [sl[RECON_B]])
        gan(B_dis_real, D_REAL, B_REAL1); gan(B_dis_fake, D_FAKE, B_FAKE0); gan(B_dis_fake, G_FAKE, B_FAKE1)
        for l, (r, f) in enumerate(zip(B_feats_real, B_feats_fake)):
            terms[FM0 + nfm + l] = F_.FeatureMatchFn.apply(r, f, sl[FM0 + nfm + l])
        if self.two_streams:
            main.wait_stream(side)
        return self._mix(lv, terms, iters, dstep, nfm, AB=AB, BA=BA, ABA=ABA, BAB=BAB, seen=seen,
                         A_dis_real=A_dis_real, A_dis_fake=A_dis_fake, B_dis_real=B_dis_real, B_dis_fake=B_dis_fake,
                         A_feats_real=A_feats_real, B_feats_fake=B_feats_fake, dis_inputs=dis_inputs)

    # ---- what the two schedules (two-chain above, grouped below) share: everything but the order of dispatch ----------------------
    def _streams(self):
        """(main, side, on_side): the current stream, the A-side chain's stream (two_streams=False: main) and the context that issues on it."""
        main = torch.cuda.current_stream(self.device)
        if not self.two_streams:
            return main, main, contextlib.nullcontext
        return main, self.side_stream, lambda: torch.cuda.stream(self.side_stream)

    def _wait_dis_ready(self, *streams, keep=False):
        """The discriminators' all-reduce + Adam of the last D-step may still run on the communication stream (``_ev_dis_ready``): the
        given streams wait for it, and the event is dropped unless ``keep`` (a later reader on another stream has to wait as well)."""
        if self._ev_dis_ready is not None:
            for s in streams:
                s.wait_event(self._ev_dis_ready)
            if not keep:
                self._ev_dis_ready = None

    @contextlib.contextmanager
    def _on_comm_behind(self, stream):
        """Hand-over to the communication stream: what is issued inside runs there, behind everything queued on ``stream`` so far."""
        ev = torch.cuda.Event()
        ev.record(stream)
        self.comm_stream.wait_event(ev)
        with torch.cuda.stream(self.comm_stream):
            yield

    def _refresh_ctx(self):
        """``self.ctx`` from the trainer's CURRENT arithmetic attributes (they may have been switched between iterations: tests run one
        trainer in several arithmetics), with no derived operand form of an earlier pass left in it."""
        self.ctx.prec = PREC_OF[self.mfma_dtype]
        self.ctx.shadow, self.ctx.act16, self.ctx.x3 = bool(self.bf16_shadow), self.act_dtype == "bf16", bool(self.x3_planes)
        self.ctx.clear()

    def _loss_vector(self):
        """(nfm, lv, sl, terms): the feature-matching layers per discriminator, the iteration's loss vector, a view of each of its slots
        (where the loss kernels write), and the dict slot -> autograd term that the schedule fills and ``_mix`` reads."""
        nfm = self.discriminator_A.n_stages - 1
        lv = torch.empty(FM0 + 2 * nfm, device=self.device, dtype=torch.float32)
        return nfm, lv, [lv[i] for i in range(FM0 + 2 * nfm)], {}

    def _no_recon(self, lv, sl, terms):
        """A D-step whose losses are not read runs no reconstruction pass: both terms read NaN, and are the bare slots."""
        lv[RECON_A:RECON_B + 1].fill_(float("nan"))
        terms[RECON_A], terms[RECON_B] = sl[RECON_A], sl[RECON_B]

    def _recon_terms(self, xs, ts, slots):
        """The reconstruction terms of ``xs`` against ``ts`` into their slots of the loss vector -- the reference's MSE, or the criterion
        of ``recon_loss``: one pass on its own stream (two-chain schedule), or both as one grouped launch."""
        mse = self.recon_loss == "mse"
        if self.recon_ms:                                 # the multi-scale kinds: csrc/msssim.hip, the same places and streams
            if len(xs) == 1:
                return (F_.MsSsimLossFn.apply(xs[0], ts[0], self.recon_ms, self.recon_w, slots[0]),)
            return F_.MsSsimLossGroupFn.apply(len(xs), self.recon_ms, self.recon_w, *xs, *ts, *slots)
        if len(xs) == 1:
            return (F_.MSELossFn.apply(xs[0], ts[0], slots[0]) if mse else F_.ReconLossFn.apply(xs[0], ts[0], self.recon_w, slots[0]),)
        if mse:
            return F_.MSELossGroupFn.apply(len(xs), *xs, *ts, *slots)
        return F_.ReconLossGroupFn.apply(len(xs), self.recon_w, *xs, *ts, *slots)

    def _gan_terms(self, xs, roles, slots):
        """The GAN terms of the discriminator outputs ``xs`` in their ``roles`` (D_REAL / D_FAKE / G_FAKE) into their slots of the loss
        vector: one term on its own stream (two-chain schedule), or several as one grouped launch.  "bce": the reference's BCELoss of
        the sigmoid outputs against the role's label (gan_real_label, 0, 1); any other kind: the objective on the logits."""
        if self.gan_kind is None:
            labels = tuple((self.gan_real_label, 0.0, 1.0)[r] for r in roles)
            if len(xs) == 1:
                return (F_.BCELossFn.apply(xs[0].reshape(xs[0].size(0), -1), labels[0], slots[0]),)
            return F_.BCELossGroupFn.apply(len(xs), labels, *xs, *slots)
        if len(xs) == 1:
            return (F_.GanLossFn.apply(xs[0].reshape(xs[0].size(0), -1), self.gan_kind, roles[0], self.gan_real_label, slots[0]),)
        return F_.GanLossGroupFn.apply(len(xs), self.gan_kind, tuple(roles), self.gan_real_label, *xs, *slots)

    def _pooled_fakes(self, dstep, BA, AB, ctx_for_BA=contextlib.nullcontext):
        """(BA_seen, AB_seen, seen): the fakes the discriminators see -- in a D-step with a history pool the exchanged batches (BA's
        exchange is issued under ``ctx_for_BA()``, AB's on the current stream), otherwise BA / AB themselves and seen = None."""
        if not dstep or self.pool_BA is None:
            return BA, AB, None
        with ctx_for_BA():
            BA_seen = self.pool_BA.exchange(BA)
        AB_seen = self.pool_AB.exchange(AB)
        return BA_seen, AB_seen, dict(BA=BA_seen, AB=AB_seen)

    def _mix(self, lv, terms, iters, dstep, nfm, **tensors):
        """The tail of both schedules: the curriculum mix of the loss vector (one launch; its backward seeds the gradient of every term
        in ``loss_slots``) and the iteration's namespace: the ten loss scalars, ``lossvec`` and the schedule's ``tensors``.  Among them
        ``A_dis_real`` / ``A_dis_fake`` / ``B_dis_real`` / ``B_dis_fake`` are the discriminators' sigmoid outputs with ``gan_loss="bce"`` and
        their LOGITS with every other objective."""
        arch, which, idx = loss_slots(self.args.model_arch, dstep, nfm)
        mixed = F_.LossMixFn.apply(lv, nfm, self.rate(iters), arch, which, idx, *[terms[i] for i in idx])
        return IterationOutputs(**dict(zip(MIX_KEYS, mixed)), recon_loss_A=terms[RECON_A], recon_loss_B=terms[RECON_B], lossvec=lv, **tensors)

    def _forward_losses_grouped(self, A, B, iters, need_losses=True):
        """image_translation.py:342-382 with every pair of passes as grouped launches (model.group_generators /
        group_discriminators).  Main stream: G_A(B) | G_B(A), then G_A(AB) | G_B(BA) + the two reconstruction terms; side stream
        (from the hand-over of AB / BA on): the discriminator passes + GAN / feature-matching terms -- D-step: D_A(A) | D_A(BA) |
        D_B(B) | D_B(AB) as ONE group of four, G-step: the real pair without an autograd graph, then the fake pair."""
        dstep = self.is_dis_step(iters)
        gen_ctx = torch.no_grad if dstep else torch.enable_grad
        main, side, on_side = self._streams()
        gA, gB, dA, dB = self.generator_A, self.generator_B, self.discriminator_A, self.discriminator_B
        nfm, lv, sl, terms = self._loss_vector()
        F_.FINAL_PASS = True        # the backward of these two passes is the last to touch each generator's parameters
        try:
            cut = None
            with gen_ctx():
                if self.graph_overlap and not dstep and self._split_backward:
                    (BA, AB), hs, leaves = group_generators([gA, gB], [B, A], cut_at_bottleneck=True)
                    cut = (hs, leaves)
                else:
                    BA, AB = group_generators([gA, gB], [B, A])
        finally:
            F_.FINAL_PASS = False
        if self.graph_overlap:
            self._cut("dis_ready")                           # (a gap between two captured graphs: the wait happens at replay)
        else:
            self._wait_dis_ready(main)                       # D parameters updated on the communication stream
        if self.two_streams:
            side.wait_stream(main)
            for t_ in (A, B, lv, AB, BA):
                t_.record_stream(side)
        want_recon = need_losses or not dstep
        ABA = BAB = None
        if want_recon:
            with gen_ctx():
                ABA, BAB = group_generators([gA, gB], [AB, BA])
                terms[RECON_A], terms[RECON_B] = self._recon_terms([ABA, BAB], [A, B], [sl[RECON_A], sl[RECON_B]])
        else:
            self._no_recon(lv, sl, terms)
        dis_inputs = None
        aug = self.aug_A is not None
        logits = self.gan_kind is not None                   # an objective on logits: the discriminators skip their sigmoid
        with on_side():
            BA_seen, AB_seen, seen = self._pooled_fakes(dstep, BA, AB)     # the history pool: both exchanges on the discriminators' stream
            if dstep:
                A_in, BA_in, B_in, AB_in = A, BA_seen, B, AB_seen
                if aug:                                      # the four inputs of the group of four: one launch per pass
                    A_in, BA_in, B_in, AB_in = apply_group([self.aug_A, self.aug_BA, self.aug_B, self.aug_AB], [A, BA_seen, B, AB_seen])
                (A_dis_real, A_feats_real), (A_dis_fake, A_feats_fake), (B_dis_real, B_feats_real), (B_dis_fake, B_feats_fake) = \
                    group_discriminators([dA, dA, dB, dB], [A_in, BA_in, B_in, AB_in], logits)
            else:
                A_in, BA_in, B_in, AB_in = A, BA, B, AB
                with torch.no_grad():
                    if aug:
                        A_in, B_in = apply_group([self.aug_A, self.aug_B], [A, B])
                    (A_dis_real, A_feats_real), (B_dis_real, B_feats_real) = group_discriminators([dA, dB], [A_in, B_in], logits)
                if aug:                                      # the gradient of the fakes flows back through the transform
                    BA_in, AB_in = apply_group([self.aug_BA, self.aug_AB], [BA, AB])
                (A_dis_fake, A_feats_fake), (B_dis_fake, B_feats_fake) = group_discriminators([dA, dB], [BA_in, AB_in], logits)
            if aug:
                dis_inputs = dict(A=A_in, BA=BA_in, B=B_in, AB=AB_in)
            # GAN terms (image_translation.py:157-166): bce(real, 1) and bce(fake, 1) of both sides in one launch, bce(fake, 0) in another
            terms[A_REAL1], terms[A_FAKE1], terms[B_REAL1], terms[B_FAKE1] = self._gan_terms(
                [A_dis_real, A_dis_fake, B_dis_real, B_dis_fake], [D_REAL, G_FAKE, D_REAL, G_FAKE],
                [sl[A_REAL1], sl[A_FAKE1], sl[B_REAL1], sl[B_FAKE1]])
            terms[A_FAKE0], terms[B_FAKE0] = self._gan_terms([A_dis_fake, B_dis_fake], [D_FAKE, D_FAKE], [sl[A_FAKE0], sl[B_FAKE0]])
            for l in range(nfm):
                terms[FM0 + l], terms[FM0 + nfm + l] = F_.FeatureMatchGroupFn.apply(
                    2, A_feats_real[l], B_feats_real[l], A_feats_fake[l], B_feats_fake[l], sl[FM0 + l], sl[FM0 + nfm + l])
        if self.two_streams:
            main.wait_stream(side)
        return self._mix(lv, terms, iters, dstep, nfm, AB=AB, BA=BA, ABA=ABA, BAB=BAB, seen=seen,
                         A_dis_real=A_dis_real, A_dis_fake=A_dis_fake, B_dis_real=B_dis_real, B_dis_fake=B_dis_fake,
                         A_feats_real=A_feats_real, B_feats_fake=B_feats_fake, backward_cut=cut, dis_inputs=dis_inputs)

    # ---- the iteration as a sequence of graphs with gaps (overlap_comm="graph") --------------------------------------------------
    def _cut(self, name):
        """A point of the iteration where the host must act between kernels: while a _SegCapture records, the current graph ends
        here and the next one begins (the action runs in the gap at every replay); in eager dispatch the action runs right away."""
        if self._cap is not None:
            self._cap.cut(name)
        else:
            self._gap(name)

    def _gap(self, name):
        main = torch.cuda.current_stream(self.device)
        if name == "dis_ready":
            self._wait_dis_ready(main)
        elif name == "dec_bucket":
            # every gradient of both decoders is final: their exchange + Adam slices leave while the encoders' backward replays
            with self._on_comm_behind(main):
                self.optim_gen.begin_step()
                self._exchange_and_step_ranges(self.optim_gen, self._gen_ranges()[1], "G")
            self._dec_done = True
        else:
            raise ValueError(name)

    def _gen_ranges(self):
        """(encoder ranges, decoder ranges) of the generators in the flat buffer of optim_gen."""
        if getattr(self, "_gen_rng", None) is None:
            enc = self.optim_gen.ranges_of([self.generator_A.encoder, self.generator_B.encoder])
            dec = self.optim_gen.ranges_of([self.generator_A.decoder, self.generator_B.decoder])
            self._gen_rng = (enc, dec)
        return self._gen_rng

    def _exchange_and_step_ranges(self, opt, ranges, kind):
        """all-reduce(sum) + Adam of flat ranges on the current stream (the step state was advanced by opt.begin_step())."""
        opt.fill_unwritten_grads(ranges)                  # (networks outside the loss: nothing wrote their gradients)
        for b, e in ranges:
            opt.step_ranges([(b, e)], self._all_reduce(opt.flat_g[b:e], kind))
        opt.finish_step()

    def _fwd_bwd(self, A, B, iters, need_losses=True):
        dstep = self.is_dis_step(iters)
        self._set_requires_grad(dstep)
        if self.skip_dead_work:
            # only the stepped side's gradients are written this iteration; the other flat buffer is
            # left alone (it may still be in flight on the communication stream; the event stays for the forward's own streams)
            if dstep and self._cap is None:
                self._wait_dis_ready(torch.cuda.current_stream(self.device), keep=True)
            # lazy: no fill -- the first weight-gradient kernel of every parameter overwrites (optim.Adam.zero_grad)
            (self.optim_dis if dstep else self.optim_gen).zero_grad(lazy=True)
        else:
            self.optim_gen.zero_grad(lazy=not dstep)     # image_translation.py:336-339 (the side that is not stepped: a plain fill)
            self.optim_dis.zero_grad(lazy=dstep)
        self._refresh_ctx()
        try:
            with ops.use(self.ctx):            # this trainer's arithmetic / operand forms ride with every call
                out = self.forward_losses(A, B, iters, need_losses)
                cut = getattr(out, "backward_cut", None)
                if cut is not None:
                    # backward in two calls: down to the stage-1 bottleneck leaves (completes every decoder gradient of both
                    # generators -- stage-2 passes included --, written into the flat buffer by the kernels), gap, then the encoders
                    out.gen_loss.backward(gradient=self._one)
                    if self.two_streams:
                        torch.cuda.current_stream(self.device).wait_stream(self.side_stream)
                    self._cut("dec_bucket")
                    hs, leaves = cut
                    torch.autograd.backward(list(hs), [l.grad for l in leaves])
                    out.backward_cut = None
                else:
                    (out.dis_loss if dstep else out.gen_loss).backward(gradient=self._one)
        finally:
            self.ctx.clear()
        if self.skip_dead_work and not dstep:
            for p in self.optim_dis.params:               # a G-step froze the D parameters: give them back
                p.requires_grad_(True)
        if self.two_streams:
            # the backward kernels of the A-side chain ran on the side stream and wrote the flat gradient
            # buffer directly (no AccumulateGrad leaf for autograd to sync): join before Adam / all-reduce
            torch.cuda.current_stream(self.device).wait_stream(self.side_stream)
        return out

    def _graph_key(self, A, B, iters, need_losses=True):
        return ("D" if self.is_dis_step(iters) else "G", self.rate(iters), bool(need_losses) or not self.is_dis_step(iters),
                tuple(A.shape), tuple(B.shape))

    def _fwd_bwd_graphed(self, A, B, iters, need_losses=True):
        # static input buffers and captured graphs are per batch shape (a short last batch of an epoch gets its own)
        shp = (tuple(A.shape), tuple(B.shape))
        if self._static is None:
            self._static = {}
        if shp not in self._static:
            self._static[shp] = (torch.empty_like(A), torch.empty_like(B))
        sA, sB = self._static[shp]
        sA.copy_(A)
        sB.copy_(B)
        key = self._graph_key(A, B, iters, need_losses)
        ent = self._graphs.get(key)
        if ent is None:
            if self.graph_overlap:
                cap = _SegCapture(self)
                self._cap = cap
                try:
                    with cap:
                        out = self._fwd_bwd(sA, sB, iters, need_losses)
                finally:
                    self._cap = None
                ent = (cap, out)
            else:
                g = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(g):
                    out = self._fwd_bwd(sA, sB, iters, need_losses)
                ent = (g, out)
            self._graphs[key] = ent
        ent[0].replay()
        return ent[1]

    def _all_reduce(self, flat_slice, kind):
        """All-reduce (sum) of a slice of a flat gradient buffer on the current stream, between two timing events under time_comm;
        returns the 1/W scale (1.0 on one device, where nothing is exchanged)."""
        if self.xg is None:
            return 1.0
        if not self.time_comm:
            return self.xg.all_reduce_sum_(flat_slice)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        scale = self.xg.all_reduce_sum_(flat_slice)
        e1.record()
        self.comm_events[kind].append((e0, e1))
        return scale

    def _exchange(self, opt, kind):
        """All-reduce (sum) of the stepped side's flat gradient buffer on the current stream; returns the 1/W scale."""
        if self.xg is None:
            return 1.0
        opt.fill_unwritten_grads()
        return self._all_reduce(opt.flat_g, kind)

    def _draw_ahead(self, A, B, iters):
        """The device draws ahead of an iteration's dispatch, outside any capture.  With a history pool, in a D-step: the record tables
        of this iteration's two exchanges (BA = G_A(B) has B's batch size, AB = G_B(A) has A's).  With differentiable augmentation, in
        EVERY iteration: the four tables of the discriminators' inputs.  Eager launches on the current stream, which everything the
        iteration issues -- eagerly or by graph replay -- is ordered behind.  With an ADA controller the draws read p from its control
        block: they are ordered behind the update of the last D-step, also where that ran on the communication stream."""
        if self.pool_BA is not None and self.is_dis_step(iters):
            self.pool_BA.draw(iters, B.shape[0])
            self.pool_AB.draw(iters, A.shape[0])
        if self.ada is not None:                              # (host arithmetic: the window counters stay exact)
            check_ada(self.diffaug_flags, None, self.ada.target, self.ada.interval, self.ada.kimg, self.ada.p_max,
                      batch=max(A.shape[0], B.shape[0]), world=self.world_size)
        if self._ev_ada is not None:
            # the controller's update of the last D-step may still be queued on the communication stream: the draws read its p
            torch.cuda.current_stream(self.device).wait_event(self._ev_ada)
            self._ev_ada = None
        if self.aug_A is not None:
            self.aug_A.draw(iters, A.shape[0])
            self.aug_BA.draw(iters, B.shape[0])
            self.aug_B.draw(iters, B.shape[0])
            self.aug_AB.draw(iters, A.shape[0])

    def train_iteration(self, A, B, iters, do_step=True, need_losses=True):
        """One full iteration; returns the namespace of (device) loss scalars.  need_losses=False tells the
        trainer that this iteration's loss values will not be read (no log line): a D-step then skips the two
        reconstruction passes, which feed only the log (weights and optimiser state are unaffected).

        The namespace carries ``BA_seen`` / ``AB_seen``, the fake batches the discriminators were given: ``BA`` / ``AB`` themselves in a
        G-step and without a history pool; with ``image_pool > 0`` a D-step's exchanged batches (detached).  Every fake pass of a D-step
        then runs on the pooled fakes, so the GEN and FM values a D-step LOGS (they step nothing there) are computed on them too;
        RECON always comes from the unpooled ``AB`` / ``BA``."""
        dstep = self.is_dis_step(iters)
        opt = self.optim_dis if dstep else self.optim_gen
        self._draw_ahead(A, B, iters)
        if self.graph_overlap:
            return self._train_iteration_graph_overlap(A, B, iters, do_step, need_losses)
        bucketed = self._buckets is not None and not dstep and do_step and self.xg is not None and not self.grad_control
        if self.time_comm:
            self.comm_steps["D" if dstep else "G"] += 1
        if bucketed:
            self._buckets.begin(opt, self.active_ranges(dstep))
        try:
            if self.use_graph and iters >= self._eager_until:       # first cycle (and the first after a resume) runs eagerly
                out = self._fwd_bwd_graphed(A, B, iters, need_losses)
            else:
                out = self._fwd_bwd(A, B, iters, need_losses)
        finally:
            if bucketed:
                F_.FINAL_HOOK = None
        if bucketed:
            self._buckets.finish()
            self._ema_update(iters)                           # (finish() made the main stream wait for every bucket's update)
            return out
        self._ada_note(out, dstep)
        if do_step:
            self.apply_step(iters)
        else:
            opt.fill_unwritten_grads()                        # the caller reads the gradients: none is left as the last iteration's
        return out

    def apply_step(self, iters):
        """Exchange + optimiser step + EMA of the side that iteration ``iters`` steps, on the gradients its backward pass left in the
        flat buffer: ``train_iteration(A, B, iters, do_step=False)`` followed by ``apply_step(iters)`` is a full iteration (with
        ``do_step=False`` the gradients stay rank-local: the exchange belongs to the step).  One flat message, summed; the 1/W rides
        in the Adam kernel.  With gradient control the optimiser measures, clips and guards behind the exchange, on the same stream.
        A D-step of an overlapped schedule runs on the communication stream and is waited for where the discriminators are read."""
        dstep = self.is_dis_step(iters)
        opt = self.optim_dis if dstep else self.optim_gen
        if dstep and (self.overlap_comm or self.graph_overlap):
            with self._on_comm_behind(torch.cuda.current_stream(self.device)):
                scale = self._exchange(opt, "D")
                opt.step(grad_scale=scale, active=self.active_ranges(dstep))
                self._ev_dis_ready = torch.cuda.Event()
                self._ev_dis_ready.record(self.comm_stream)
                self._ada_step(self.comm_stream)
            return
        scale = self._exchange(opt, "D" if dstep else "G")
        opt.step(grad_scale=scale, active=self.active_ranges(dstep))
        if dstep:
            self._ada_step(None)
        else:
            self._ema_update(iters)

    def _ada_note(self, out, dstep):
        """A D-step's discriminator outputs on its real batches, kept for the controller until that step's ``apply_step``."""
        if self.ada is not None and dstep:
            self._ada_real = (out.A_dis_real, out.B_dis_real)

    def _ada_step(self, comm_stream):
        """The controller's part of a discriminator step, on the current stream directly behind that step's gradient exchange and Adam:
        both windows take the signs of the step's real outputs, and every ada_interval-th step closes them (all-reduce of the 16 bytes
        first, so every rank enqueues the collectives of the one communicator in the same order).  ``comm_stream``: the stream this
        runs on when it is not the main one -- the outputs were produced elsewhere, and the next draws wait for the event."""
        if self.ada is None or self._ada_real is None:
            return
        reals, self._ada_real = self._ada_real, None
        for domain, t in enumerate(reals):
            t = t.detach()
            if comm_stream is not None:
                t.record_stream(comm_stream)
            self.ada.accumulate(domain, t if t.dtype == torch.float32 else t.float(), self.ada_threshold)
        self.ada.step(self.xg)
        if comm_stream is not None:
            self._ev_ada = torch.cuda.Event()
            self._ev_ada.record(comm_stream)

    def _ema_update(self, iters):
        """Behind a generator Adam step that is ordered before this point on the current (main) stream."""
        if self.ema is not None and iters >= self.args.ema_start_iter:
            self.ema.update()

    def _train_iteration_graph_overlap(self, A, B, iters, do_step, need_losses):
        """overlap_comm="graph": see __init__.  Results are bitwise those of the plain schedule: the all-reduce and the Adam kernel are
        elementwise, the slices share one step state."""
        dstep = self.is_dis_step(iters)
        opt = self.optim_dis if dstep else self.optim_gen
        main = torch.cuda.current_stream(self.device)
        if self.time_comm:
            self.comm_steps["D" if dstep else "G"] += 1
        if dstep:                                             # (a D-step right behind a D-step: update_interval 1)
            self._wait_dis_ready(main)
        self._split_backward, self._dec_done = bool(do_step) and not self.grad_control, False
        if self.use_graph and iters >= self._eager_until and do_step:
            out = self._fwd_bwd_graphed(A, B, iters, need_losses)
        else:
            out = self._fwd_bwd(A, B, iters, need_losses)
        self._ada_note(out, dstep)
        if not do_step:
            opt.fill_unwritten_grads()
            return out
        if dstep or not self._dec_done:
            # a D-step leaves on the communication stream; a G-step whose backward was not cut (two-chain schedule, gradient control)
            # is needed by the very next kernel -- main stream
            self.apply_step(iters)
            return out
        with self._on_comm_behind(main):
            self._exchange_and_step_ranges(opt, self._gen_ranges()[0], "G")      # the encoders: the exposed part
        main.wait_stream(self.comm_stream)                # the next iteration's first kernels read the generators' weights
        self._ema_update(iters)                           # ... and so does the EMA: decoders' and encoders' slices are both in
        return out

    def comm_ms(self):
        """All-reduce time per D-step / per G-step (ms; a G-step's buckets are summed) from the recorded HIP events
        (time_comm=True)."""
        torch.cuda.synchronize(self.device)
        out = {}
        for k, evs in self.comm_events.items():
            if evs and self.comm_steps[k]:
                out[k] = sum(a.elapsed_time(b) for a, b in evs) / self.comm_steps[k]
        return out

    def finish(self):
        """Join the communication stream (call before reading parameters / saving / timing)."""
        self._wait_dis_ready(torch.cuda.current_stream(self.device), keep=True)     # (kept: the next forward's streams wait on their own)
        if self._ev_ada is not None:                      # the controller's update behind it (kept for the next draws alike)
            torch.cuda.current_stream(self.device).wait_event(self._ev_ada)

    def sample(self, test_A, test_B):
        """The four generator passes of a sampling event on the held-out split (image_translation.py:170-184):
        ``AB = G_B(test_A); BA = G_A(test_B); ABA = G_A(AB); BAB = G_B(BA)``, returned as device tensors [n,3,S,S].

        Like the reference: under ``no_grad`` but in whatever mode the generators are in -- training mode in a training run, so every
        pass normalises with the statistics of the whole split (ONE batch per pass) and each generator's BatchNorm buffers advance by
        two forward calls.  Nothing else changes: the passes run eagerly on the main stream between iterations under this trainer's own
        arithmetic, write no gradient, touch no optimiser or discriminator state and no captured graph or its static inputs."""
        if test_A.dim() != 4 or test_B.dim() != 4 or test_A.shape[0] < 2 or test_B.shape[0] < 2:
            raise ValueError("sample() needs two batches [n,3,S,S] with n >= 2 (train-mode BatchNorm needs more than one value per "
                             f"channel at the bottleneck), got {tuple(test_A.shape)} and {tuple(test_B.shape)}")
        self.finish()
        self._refresh_ctx()
        try:
            with torch.no_grad(), ops.use(self.ctx):
                AB = self.generator_B(test_A)
                BA = self.generator_A(test_B)
                ABA = self.generator_A(AB)
                BAB = self.generator_B(BA)
        finally:
            self.ctx.clear()                   # no bf16 shadow or plane triple of a sampling pass outlives it
        return AB, BA, ABA, BAB

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the body with the EMA weights in both generators: ``ema.swap()`` on entry and again on exit (also on an exception), the
        generators' buffers (BatchNorm running statistics, counters) saved and put back.  Afterwards the live weights, the EMA, every
        derived operand form and every generator buffer are bit for bit what they were -- a train-mode ``sample()`` inside does not
        move the live running statistics."""
        if self.ema is None:
            raise RuntimeError("ema_weights(): this trainer keeps no EMA (ema_decay = 0)")
        if not self.ema.ready:
            raise RuntimeError("ema_weights(): the EMA holds nothing yet (no generator step at iteration >= ema_start_iter so far)")
        self.finish()
        saved = [(b, b.clone()) for net in (self.generator_A, self.generator_B) for b in net.buffers()]
        self.ema.swap()
        try:
            yield self
        finally:
            self.ema.swap()
            with torch.no_grad():
                for b, old in saved:
                    b.copy_(old)

    def ema_state_dicts(self):
        """``dict(gen_A=..., gen_B=...)`` of host tensors in the key order of ``Generator.state_dict()``: parameters from the EMA,
        buffers from the live generators (running statistics are averages already)."""
        if self.ema is None or not self.ema.ready:
            raise RuntimeError("ema_state_dicts(): no EMA weights (ema_decay = 0, or no qualifying generator step yet)")
        self.finish()
        out = {}
        for key, net in (("gen_A", self.generator_A), ("gen_B", self.generator_B)):
            params = dict(net.named_parameters())
            out[key] = {n: (self.ema.view_of(params[n]) if n in params else t).detach().contiguous().cpu()
                        for n, t in net.state_dict().items()}
        return out

    # ---------------------------------------------------------------------------------------------
    def losses_to_floats(self, out):
        vals = torch.stack([getattr(out, k).detach().reshape(()) for k in LOG_KEYS]).cpu().tolist()
        return dict(zip(LOG_KEYS, vals))

    def format_log(self, iters, total, out):
        f = self.losses_to_floats(out)
        return (f"Iter [{iters}/{total}] "
                f"GEN: {f['gen_loss_A']:.4f}/{f['gen_loss_B']:.4f}, "
                f"FM: {f['fm_loss_A']:.4f}/{f['fm_loss_B']:.4f}, "
                f"RECON: {f['recon_loss_A']:.4f}/{f['recon_loss_B']:.4f}, "
                f"DIS: {f['dis_loss_A']:.4f}/{f['dis_loss_B']:.4f}" + self.grad_log_suffix() + self.ada_log_suffix())

    def ada_log_suffix(self):
        """With the controller: `` ADA: p {pA}/{pB} rt {rtA}/{rtB}`` from the two control blocks (read here, where the host waits for
        the losses anyway; rt is nan before the first update); without: the empty string."""
        if self.ada is None:
            return ""
        self.finish()
        return format_ada_suffix(self.ada.stats())

    def grad_log_suffix(self):
        """With gradient control: `` GRAD: D {norm} G {norm} clipped {c}/{n} skipped {s}`` from the two control blocks (read here, where
        the host waits for the losses anyway); without: the empty string."""
        if not self.grad_control:
            return ""
        self.finish()
        return format_grad_suffix(self.optim_dis.grad_stats(), self.optim_gen.grad_stats())

    def state_dicts(self):
        return {k: v.state_dict() for k, v in self.nets.items()}

    def train_state(self, next_iter, extra=None):
        """Everything needed to resume exactly: weights + BN buffers, both Adam states and ``next_iter`` = the index
        of the NEXT iteration to run (the reference resumes weights only and restarts Adam and the GAN curriculum,
        SURVEY.md section 5).  ``extra`` carries the caller's data-loader position (CLI: epoch, batch, RNG state)."""
        self.finish()
        torch.cuda.synchronize(self.device)
        st = dict(iters=int(next_iter), nets={k: {n: t.detach().contiguous().cpu() for n, t in v.state_dict().items()}
                                              for k, v in self.nets.items()},
                  optim_gen=self.optim_gen.state_dict(), optim_dis=self.optim_dis.state_dict())
        if self.ema is not None:
            st["ema"] = self.ema.state_dict()
        if self.pool_BA is not None:
            st["image_pool"] = dict(BA=self.pool_BA.state_dict(), AB=self.pool_AB.state_dict())
        if self.ada is not None:
            st["ada"] = self.ada.state_dict()
        if extra:
            st["loader"] = dict(extra)
        return st

    def load_train_state(self, st):
        for k, v in self.nets.items():
            v.load_state_dict(st["nets"][k])
        self.optim_gen.load_state_dict(st["optim_gen"])
        self.optim_dis.load_state_dict(st["optim_dis"])
        if self.ema is not None:
            if "ema" in st:
                self.ema.load_state_dict(st["ema"])
            else:                                  # a state written without the EMA: the next qualifying G-step starts it with a copy
                self.ema.ready, self.ema.updates = False, 0
        if self.pool_BA is not None:
            if "image_pool" in st:
                self.pool_BA.load_state_dict(st["image_pool"]["BA"])
                self.pool_AB.load_state_dict(st["image_pool"]["AB"])
            else:                                  # a state written without the pool: it fills again from the next D-step on
                self.pool_BA.clear()
                self.pool_AB.clear()
                print(f"image pool: the loaded training state holds no image_pool; both pools ({self.pool_BA.size} images per domain) "
                      "start empty", flush=True)
        if self.ada is not None:
            self._ada_real = None
            if "ada" in st:
                self.ada.load_state_dict(st["ada"])
            else:                                  # a state written without the controller: p starts from its initial value
                self.ada.reset()
                print(f"ADA: the loaded training state holds no ada entry; p starts from {self.ada.p0:g} with empty windows", flush=True)
        self._graphs = {}
        start = int(st["iters"])
        # like a fresh run, the first D,G,G cycle after a resume is dispatched eagerly before anything is captured
        self._eager_until = start + self.args.update_interval
        return start

    def close(self):
        if self.xg is not None:
            self.finish()
            torch.cuda.synchronize(self.device)
            self.xg.close()
            self.xg = None


class _SegCapture:
    """One training iteration captured as a SEQUENCE of hipGraphs sharing a memory pool, with named host-side gaps between them
    (trainer._cut): at replay the graphs are launched in order and the trainer's gap action (an event wait, a hand-over to the
    communication stream) runs between two of them -- what a single graph cannot hold, because a captured stream cannot wait on an
    event recorded outside the capture.  Mirrors torch.cuda.graph's protocol (side capture stream, global capture error mode)."""

    def __init__(self, trainer):
        self.tr = trainer
        self.graphs, self.gaps = [], []
        self.pool = torch.cuda.graph_pool_handle()
        self.stream = torch.cuda.Stream(device=trainer.device)
        self._ctx = None

    def _begin(self):
        g = torch.cuda.CUDAGraph()
        g.capture_begin(pool=self.pool, capture_error_mode="global")
        self.graphs.append(g)

    def __enter__(self):
        import gc
        torch.cuda.synchronize(self.tr.device)
        gc.collect()
        torch.cuda.empty_cache()
        self.stream.wait_stream(torch.cuda.current_stream(self.tr.device))
        self._ctx = torch.cuda.stream(self.stream)
        self._ctx.__enter__()
        self._begin()
        return self

    def cut(self, name):
        self.graphs[-1].capture_end()
        self.gaps.append(name)
        self._begin()

    def __exit__(self, et, ev, tb):
        try:
            self.graphs[-1].capture_end()
        finally:
            self._ctx.__exit__(et, ev, tb)
        torch.cuda.current_stream(self.tr.device).wait_stream(self.stream)
        return False

    def replay(self):
        for i, g in enumerate(self.graphs):
            g.replay()
            if i < len(self.gaps):
                self.tr._gap(self.gaps[i])


class _GradBuckets:
    """Overlap of the G-step gradient exchange with the backward pass (reference: DDP's bucketed reducer hooks,
    distributed_image_translation.py:401-404,513-518).

    The generators' flat gradient range is cut into buckets of whole layers (>= ``bucket_mb`` each, never across
    the two networks).  A parameter's gradient is final once the backward of its network's FIRST forward call of the
    iteration (issued last by autograd) has written it; functional.py reports that through FINAL_HOOK right after
    enqueueing the kernel.  When every parameter of a bucket has reported, an event is recorded on the producing
    stream and the communication stream runs all-reduce(bucket) + Adam(bucket slice) behind it, concurrently with
    the rest of the backward.  Buckets that never report (networks outside the loss in recongan / gan, or the
    last-to-finish ones) are flushed after the backward.  Results are bitwise those of the one-message path: the
    all-reduce is elementwise and the Adam kernel is elementwise with one shared step state."""

    def __init__(self, trainer, bucket_mb):
        self.tr = trainer
        opt = trainer.optim_gen
        target = int(bucket_mb * 1024 * 1024 / 4)
        self.buckets = []
        self.of_param = {}
        for net in (trainer.generator_A, trainer.generator_B):
            ids = {id(p) for p in net.parameters()}
            cur = None
            for p, off, end in opt.extents():
                if id(p) not in ids:
                    continue
                if cur is None or cur["end"] - cur["begin"] >= target:
                    cur = dict(begin=off, end=end, nparams=0, pending=0, done=False)
                    self.buckets.append(cur)
                cur["end"] = end
                cur["nparams"] += 1
                self.of_param[id(p)] = cur
        self.opt = opt
        self.launched = 0
        self.active = None

    def begin(self, opt, active=None):
        """``active``: the flat ranges that receive gradients in this step (trainer.active_ranges; None = all).  The same
        ranges gate the Adam slice of EVERY bucket, whether it is launched early from the backward or flushed afterwards --
        exactly what the one-message path's ``opt.step(active=...)`` does."""
        assert opt is self.opt
        self.active = active
        tr = self.tr
        main = torch.cuda.current_stream(tr.device)
        for b in self.buckets:
            b["pending"], b["done"] = b["nparams"], False
        self.launched = 0
        # the step counter / bias corrections advance once, on the communication stream, behind everything queued
        tr.comm_stream.wait_stream(main)
        with torch.cuda.stream(tr.comm_stream):
            opt.begin_step()
        F_.FINAL_HOOK = self.notify

    def notify(self, param):
        b = self.of_param.get(id(param))
        if b is None or b["done"]:
            return
        # the kernels accumulated into the flat gradient view; a .grad replaced during the backward would not be exchanged
        if param.grad is not param._dg_flat_grad:
            raise RuntimeError("bucketed exchange: a parameter's .grad was replaced during the backward pass "
                               "(it must stay the view of the optimiser's flat gradient buffer)")
        b["pending"] -= 1
        if b["pending"] == 0:
            self._launch(b, torch.cuda.current_stream(self.tr.device), early=True, active=self.active)

    def _launch(self, b, producer_stream, early, active=None):
        tr, opt = self.tr, self.opt
        b["done"] = True
        with tr._on_comm_behind(producer_stream):
            scale = tr._all_reduce(opt.flat_g[b["begin"]:b["end"]], "G")
            if active is None or any(lo <= b["begin"] and b["end"] <= hi for lo, hi in active):
                opt.step_ranges([(b["begin"], b["end"])], scale)    # (with the slice's bf16 shadow / f32x3 plane triples)
        if early:
            self.launched += 1

    def finish(self):
        """After the backward: flush the buckets that did not report, then make the main stream wait for the updates."""
        tr = self.tr
        main = torch.cuda.current_stream(tr.device)
        self.opt.fill_unwritten_grads()                   # before the flush reads them (every bucket launched early was written whole)
        for b in self.buckets:
            if not b["done"]:
                self._launch(b, main, early=False, active=self.active)
        with torch.cuda.stream(tr.comm_stream):
            self.opt.finish_step()                        # every bucket's planes are written: the transposed weight copy follows
        main.wait_stream(tr.comm_stream)


def synthetic_batch(n, image_size, seed, device):
    """rand in [0,1) like dataset.py:65 (/255); A then B from one host generator."""
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(n, 3, image_size, image_size, generator=g)
    B = torch.rand(n, 3, image_size, image_size, generator=g)
    return A.to(device), B.to(device)
