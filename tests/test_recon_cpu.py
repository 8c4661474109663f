"""The reconstruction criterion without a GPU: the reference against the metrics reference, its autograd gradient against the analytic
gather form and a central finite difference, the weight table, the refusals of the trainer's check, the CLI flags, and the new symbols
in header, ctypes table and library."""
import ctypes
import os
import re

import pytest
import torch

from discogan_modernized_amd import _lib, losses, trainer
from discogan_modernized_amd import image_translation as it
from tests import metrics_ref as MR
from tests import recon_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 11), (2, 12), (1, 43), (2, 64), (3, 75))
TRIPLE = (0.3, 0.3, 0.4)
NEW_SYMBOLS = ("dg_recon_loss_workspace_bytes", "dg_recon_loss_fwd", "dg_recon_loss_bwd", "dg_recon_loss_fwd_g", "dg_recon_loss_bwd_g")


@pytest.mark.parametrize("n,S", SHAPES)
def test_ref_ssim_term_is_the_metrics_reference(n, S):
    for kind in MR.KINDS:
        x, t = MR.make_pair(kind, n, S, 7 * S + n)
        mse, l1, ssim = RR.parts_ref(x, t)
        assert abs(float(1.0 - ssim) - float(MR.ssim_ref(x, t).mean())) <= 1e-12, kind
        m, a = MR.mse_mae_ref(x, t)
        assert abs(float(mse) - float(m.mean())) <= 1e-15 and abs(float(l1) - float(a.mean())) <= 1e-15


@pytest.mark.parametrize("n,S", SHAPES)
def test_autograd_gradient_is_the_analytic_gather_form(n, S):
    for kind in MR.KINDS:
        x, t = MR.make_pair(kind, n, S, 7 * S + n)
        for w in ((0.0, 0.0, 1.0), losses.recon_weights("l1_ssim", 0.84), TRIPLE):
            auto, ana = RR.grad_ref(x, t, w, 0.7), RR.grad_analytic(x, t, w, 0.7)
            rel = float((auto - ana).abs().max() / auto.abs().max())
            # two float64 evaluations: 2^-53 x the cancellation in a = dmu - 2 mx dsig - my dc (terms of 1 / C2 ~ 1e3 times the
            # result on the flat data) x the 121-term sums ~ 1e-16 x 1e3 x 1e2; a wrong tap or factor is off by 1e-2 and more
            assert rel <= 1e-11, (kind, w, rel)


def test_gradient_is_the_central_finite_difference():
    x, t = MR.make_pair("indep", 1, 12, 3)
    x64, h = x.double(), 1e-6
    for w in ((0.0, 0.0, 1.0), (0.0, 0.16, 0.84), TRIPLE):
        auto = RR.grad_ref(x, t, w)
        fd = torch.zeros_like(x64).reshape(-1)
        for i in range(x64.numel()):
            e = torch.zeros(x64.numel(), dtype=torch.float64)
            e[i] = h
            e = e.reshape(x64.shape)
            fd[i] = (RR.loss_ref(x64 + e, t, w) - RR.loss_ref(x64 - e, t, w)) / (2 * h)
        rel = float((auto.reshape(-1) - fd).abs().max() / auto.abs().max())
        assert rel <= 1e-6, (w, rel)                  # the difference quotient's own error: h^2 f''' / 6 + rounding / h


def test_shapes_past_the_grid_caps_reach_every_stride_loop():
    """The host's grid arithmetic (csrc/recon.hip, dg_recon_loss_fwd_g / dg_recon_loss_bwd_g) at the shapes the GPU tests run past the
    caps, and the constants they copy against the source."""
    src = open(os.path.join(ROOT, "discogan_modernized_amd", "csrc", "recon.hip")).read()
    assert int(re.search(r"#define RC_MAX_BLOCKS (\d+)", src).group(1)) == RR.RC_MAX_BLOCKS
    assert int(re.search(r"#define RC_STREAM_BLOCKS (\d+)", src).group(1)) == RR.RC_STREAM_BLOCKS
    assert int(re.search(r"#define RT (\d+)", src).group(1)) == RR.TILE
    assert "i += 256" in src.split("void recon_final_kernel")[1].split("__global__")[0] and RR.FINAL_THREADS == 256
    assert "g > 2 * RC_STREAM_BLOCKS ? 2 * RC_STREAM_BLOCKS" in src                          # the backward stream kernel's cap
    assert [RR.tile_items(n, S) for n, S in RR.TILE_PAST_CAP] == [(16410, 3), (8280, 12), (8280, 12)]
    assert RR.planted_images(5470, 11) == [0, 2730, 2731, 5461, 5462, 5469] and RR.planted_images(690, 43) == [0, 682, 683, 689]
    for n, S in RR.TILE_PAST_CAP:
        items, P = RR.tile_items(n, S)
        assert items > RR.RC_MAX_BLOCKS and -(-items // RR.RC_MAX_BLOCKS) == (3 if S == 11 else 2)
        at = RR.planted_images(n, S)
        for k in range(1, (items - 1) // RR.RC_MAX_BLOCKS + 1):                              # the items either side of every trip boundary
            assert (k * RR.RC_MAX_BLOCKS - 1) // P in at and (k * RR.RC_MAX_BLOCKS) // P in at
    assert [S % 4 for _, S in RR.TILE_PAST_CAP] == [3, 3, 0]
    assert RR.tile_items(30, 43)[0] == 360 and RR.stream_blocks(2, 256) == (384, 98304, 0)  # FINAL_PAST_256: one grid, two trips of the final kernel
    assert RR.stream_blocks(11, 256) == (2112, 540672, 0) and RR.stream_blocks(125, 75) == (2060, 527343, 3)
    for n, S in RR.STREAM_PAST_CAP:
        assert RR.stream_blocks(n, S)[0] > 2 * RR.RC_STREAM_BLOCKS
    for n, S in SHAPES:                                                                      # what the older tests reach: one trip everywhere
        assert RR.tile_items(n, S)[0] <= RR.FINAL_THREADS and RR.stream_blocks(n, S)[0] <= RR.FINAL_THREADS


@pytest.mark.parametrize("n,S", RR.TILE_PAST_CAP)
def test_a_planted_channel_moves_the_loss_by_four_forward_bounds(n, S):
    """On ``planted_pair`` data, making x = t in any one channel of any one planted image (what a dropped or misplaced item would
    amount to) moves the float64 loss by more than 4 x the forward bound.  The loss is a mean over images of per-image terms, so the
    move of the whole batch's loss is the move of that image's own loss / n."""
    x, t, at = RR.planted_pair(n, S, 100 * S + n)
    assert all(torch.equal(x[i], t[i]) == (i not in at) for i in range(n))
    bound, loss = RR.fwd_bound(x, t, TRIPLE)
    least = float("inf")
    for i in at:
        own = float(RR.loss_ref(x[i:i + 1], t[i:i + 1], TRIPLE))
        for ch in range(3):
            xi = x[i:i + 1].clone()
            xi[0, ch] = t[i, ch]
            least = min(least, abs(own - float(RR.loss_ref(xi, t[i:i + 1], TRIPLE))) / n)
    print(f"n {n} S {S}: loss {loss:.6e} forward bound {bound:.3e} smallest move {least:.3e} = {least / bound:.1f} bounds")
    assert least > 4 * bound, (least, bound)


def test_recon_weights_table():
    assert losses.recon_weights("mse") == (1.0, 0.0, 0.0)
    assert losses.recon_weights("l1") == (0.0, 1.0, 0.0)
    assert losses.recon_weights("ssim") == (0.0, 0.0, 1.0)
    assert losses.recon_weights("l1_ssim", 0.84) == (0.0, 1.0 - 0.84, 0.84)
    assert losses.recon_weights("l1_ssim", 0.25) == (0.0, 0.75, 0.25)
    assert losses.recon_weights("l1_ssim") == losses.recon_weights("l1_ssim", 0.84)
    assert losses.L1Loss().weights == (0.0, 1.0, 0.0) and losses.SSIMLoss().weights == (0.0, 0.0, 1.0)
    assert losses.ReconLoss("l1_ssim", 0.5).weights == (0.0, 0.5, 0.5)
    assert trainer.DEFAULTS["recon_loss"] == "mse" and trainer.DEFAULTS["recon_ssim_alpha"] == 0.84


def test_check_recon_loss_refusals():
    assert trainer.check_recon_loss("mse", 0.84, 8) == (1.0, 0.0, 0.0)          # mse and l1 take any size; alpha is not read
    assert trainer.check_recon_loss("l1", 7.0, 8) == (0.0, 1.0, 0.0)
    assert trainer.check_recon_loss("ssim", 0.84, 11) == (0.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="unknown reconstruction loss 'huber'"):
        trainer.check_recon_loss("huber", 0.84, 64)
    for alpha in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="recon_ssim_alpha must be in"):
            trainer.check_recon_loss("l1_ssim", alpha, 64)
    for kind in ("ssim", "l1_ssim"):
        with pytest.raises(ValueError, match="needs image_size >= 11"):
            trainer.check_recon_loss(kind, 0.84, 8)


def test_parse_args_takes_the_two_flags():
    args = it.parse_args([])
    assert args.recon_loss == "mse" and args.recon_ssim_alpha == 0.84
    args = it.parse_args(["--recon_loss", "l1_ssim", "--recon_ssim_alpha", "0.5"])
    assert args.recon_loss == "l1_ssim" and args.recon_ssim_alpha == 0.5
    for kind in ("l1", "ssim"):
        assert it.parse_args(["--recon_loss", kind]).recon_loss == kind
    with pytest.raises(SystemExit):
        it.parse_args(["--recon_loss", "huber"])
    assert "--recon_loss" in it.build_parser().format_help() and "--recon_ssim_alpha" in it.build_parser().format_help()


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    txt = open(os.path.join(ROOT, "include", "discogan_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(dg_[a-zA-Z0-9_]+)\s*\(", txt))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    L = _lib.load()
    assert L.dg_recon_loss_workspace_bytes(0, 64) == 0
    assert L.dg_recon_loss_workspace_bytes(1, 11) >= 3 * 3 * 8                    # one tile per channel, three fp64 sums each
    assert L.dg_recon_loss_workspace_bytes(32, 512) >= 3 * 32 * 3 * 256 * 8
    # the entry points validate before anything is launched (no GPU needed): status < 0 and a message, nothing thrown
    P = ctypes.c_void_p
    tab = (P * 2)(16, 16)
    w = lambda *v: (ctypes.c_float * 3)(*v)      # noqa: E731
    assert L.dg_recon_loss_fwd_g(2, tab, tab, 1, 10, w(0, 0, 1), tab, tab, 1 << 20, None) < 0 and b"window does not fit" in L.dg_last_error()
    assert L.dg_recon_loss_fwd_g(2, tab, tab, 1, 16, w(0, 0, 0), tab, tab, 1 << 20, None) < 0 and b"all three weights" in L.dg_last_error()
    assert L.dg_recon_loss_bwd_g(2, tab, tab, 1, 16, w(0, -1, 1), tab, tab, None) < 0 and b"finite and >= 0" in L.dg_last_error()
    assert L.dg_recon_loss_bwd_g(5, tab, tab, 1, 16, w(0, 1, 1), tab, tab, None) < 0 and b"groups" in L.dg_last_error()
    assert L.dg_recon_loss_fwd_g(1, tab, tab, 1, 16, w(0, 1, 1), tab, tab, 8, None) < 0 and b"workspace too small" in L.dg_last_error()
    assert L.dg_recon_loss_bwd(16, None, 1, 16, w(0, 1, 1), 16, 16, None) < 0 and b"null" in L.dg_last_error()
