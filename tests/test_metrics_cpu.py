"""Held-out image metrics, the parts that need no GPU: the checker against a brute-force loop, the host arithmetic of evaluate.py, the
CLI surface, and the argument validation / workspace query of dg_image_metrics."""
import ctypes as C
import math
import re

import pytest
import torch

from discogan_modernized_amd import _lib, evaluate, samples
from discogan_modernized_amd import distributed_image_translation as dit
from discogan_modernized_amd import image_translation as it
from tests import metrics_ref as MR


def test_ssim_ref_equals_a_double_loop_over_windows():
    x, y = MR.make_pair("indep", 1, 12, seed=1)
    assert float((MR.ssim_ref(x, y, torch.float64) - MR.ssim_brute(x, y)).abs().max()) <= 1e-12
    x, y = MR.make_pair("noisy", 1, 12, seed=2)
    assert float((MR.ssim_ref(x, y, torch.float64) - MR.ssim_brute(x, y)).abs().max()) <= 1e-12
    # the wrong problems of the GPU tests are different problems
    r = MR.ssim_ref(x, y)
    for kw in (dict(sigma=1.4), dict(k=9), dict(K2=.02), dict(pad=True)):
        assert float((MR.ssim_ref(x, y, **kw) - r).abs().max()) > 1e-5, kw


def test_identical_images_score_ssim_one_mse_zero_psnr_inf():
    x, _ = MR.make_pair("indep", 3, 16, seed=3)
    assert float((MR.ssim_ref(x, x) - 1).abs().max()) <= 1e-12
    mse, mae = MR.mse_mae_ref(x, x)
    assert float(mse.max()) == 0.0 and float(mae.max()) == 0.0
    assert all(math.isinf(v) and v > 0 for v in MR.psnr_ref(mse).tolist())
    s = evaluate.summarise(torch.tensor([[0.0, 0.0, 1.0], [0.01, 0.05, 0.5]]))
    assert s["n"] == 2 and math.isinf(s["psnr"]) and s["psnr"] > 0 and s["ssim"] == 0.75
    assert s["mse"] == float(torch.tensor([0.0, 0.01]).double().mean())
    s = evaluate.summarise(torch.tensor([[0.01, 0.05, 0.5], [0.001, 0.02, 0.7]]))
    want = (10 * math.log10(1 / float(torch.tensor(0.01))) + 10 * math.log10(1 / float(torch.tensor(0.001)))) / 2
    assert abs(s["psnr"] - want) <= 1e-12


def test_parser_knows_the_evaluation_flags():
    for mod in (it, dit):
        a = mod.parse_args([])
        assert a.eval_interval == 0 and a.eval_paired == "auto" and a.image_save_interval == 1000
        b = mod.parse_args(["--eval_interval", "500", "--eval_paired", "on"])
        assert b.eval_interval == 500 and b.eval_paired == "on"
        with pytest.raises(SystemExit):
            mod.parse_args(["--eval_paired", "maybe"])
    a = it.parse_args(["--task_name", "edges2shoes"])
    assert evaluate.paired_default(a, "files") and not evaluate.paired_default(a, "tensors")
    assert not evaluate.paired_default(it.parse_args(["--task_name", "celebA"]), "files")
    assert evaluate.paired_default(it.parse_args(["--task_name", "edges2handbags"]), "files")
    assert evaluate.paired_default(it.parse_args(["--eval_paired", "on"]), "synthetic")
    assert not evaluate.paired_default(it.parse_args(["--task_name", "edges2shoes", "--eval_paired", "off"]), "files")
    e = evaluate.parse_args(["--model_path", "m", "--test_A", "a.pt", "--test_B", "b.pt", "--image_size", "16", "--paired", "--no_fold"])
    assert e.paired and e.no_fold and e.n_test == 200 and e.output == "eval.json" and not e.use_extra_layers


def test_load_split_follows_either_interval():
    a = it.parse_args(["--image_save_interval", "0", "--test_A", "nowhere.pt", "--test_B", "nowhere.pt"])
    assert samples.load_split(a, "tensors", "cpu") is None            # both off: the files are not even opened
    b = it.parse_args(["--image_save_interval", "0", "--eval_interval", "5", "--test_A", "nowhere.pt", "--test_B", "nowhere.pt"])
    with pytest.raises(FileNotFoundError):
        samples.load_split(b, "tensors", "cpu")                         # evaluation alone asks for the split


def test_small_images_are_refused_at_start_up():
    with pytest.raises(ValueError, match="11"):
        evaluate.check_size(10)
    evaluate.check_size(11)
    with pytest.raises(ValueError, match="11"):
        it.train(it.parse_args(["--task_name", "edges2shoes", "--image_size", "8", "--eval_interval", "4"]))


NUM = r"(-?\d+\.\d+|inf|nan)"
LINE = re.compile(rf"^Eval \[(\w+)\] RECON_PSNR: {NUM}/{NUM}, RECON_SSIM: {NUM}/{NUM}, RECON_MAE: {NUM}/{NUM}"
                  rf"(?:, TRANS_PSNR: {NUM}/{NUM}, TRANS_SSIM: {NUM}/{NUM}, TRANS_MAE: {NUM}/{NUM})? \(n=(\d+)/(\d+)\)$")


def test_format_eval_round_trips_through_a_regex():
    mk = lambda n, mse, mae, ssim, psnr: dict(n=n, mse=mse, mae=mae, ssim=ssim, psnr=psnr)
    res = dict(recon_A=mk(4, 0.01, 0.0812345, 0.43219, 20.12345), recon_B=mk(6, 0.02, 0.09, -0.01234, 16.9897))
    m = LINE.match(evaluate.format_eval(8, res))
    assert m and m.group(1) == "8" and m.group(8) is None and (m.group(14), m.group(15)) == ("4", "6")
    assert [float(v) for v in m.groups()[1:7]] == [20.123, 16.990, 0.4322, -0.0123, 0.08123, 0.09000]
    res.update(trans_AB=mk(4, 0.0, 0.0, 1.0, math.inf), trans_BA=mk(4, 0.1, 0.25, 0.125, 10.0))
    line = evaluate.format_eval("final", res)
    m = LINE.match(line)
    assert m and m.group(1) == "final", line
    assert [float(v) for v in m.groups()[7:13]] == [math.inf, 10.0, 1.0, 0.125, 0.0, 0.25]
    assert line.endswith(" (n=4/6)")


def test_workspace_query_is_per_image():
    L = _lib.load()
    for S in (11, 16, 42, 43, 64, 512):
        b1 = L.dg_image_metrics_workspace_bytes(1, S)
        assert b1 > 0
        last = 0
        for n in (1, 2, 5, 32, 3000):
            b = L.dg_image_metrics_workspace_bytes(n, S)
            assert b > last and b == n * b1, (n, S)
            last = b
    assert L.dg_image_metrics_workspace_bytes(1, 64) > L.dg_image_metrics_workspace_bytes(1, 32)


def test_image_metrics_entry_point_validates_its_arguments():
    """Bad arguments are refused before anything is launched (no GPU needed): negative status, message from dg_last_error."""
    L = _lib.load()
    P = C.c_void_p
    d = P(64)                                       # non-null dummy: validation fails before it is dereferenced
    need = L.dg_image_metrics_workspace_bytes(2, 16)
    assert L.dg_image_metrics(d, d, 2, 10, d, d, 1 << 20, None) < 0 and b"S 10" in L.dg_last_error()
    assert L.dg_image_metrics(d, d, 0, 16, d, d, 1 << 20, None) < 0 and b"n 0" in L.dg_last_error()
    assert L.dg_image_metrics(None, d, 2, 16, d, d, need, None) < 0 and b"null" in L.dg_last_error()
    assert L.dg_image_metrics(d, None, 2, 16, d, d, need, None) < 0 and b"null" in L.dg_last_error()
    assert L.dg_image_metrics(d, d, 2, 16, None, d, need, None) < 0 and b"null" in L.dg_last_error()
    assert L.dg_image_metrics(d, d, 2, 16, d, d, need - 1, None) < 0 and b"workspace" in L.dg_last_error()
    assert L.dg_image_metrics(d, d, 2, 16, d, None, need, None) < 0 and b"workspace" in L.dg_last_error()
    assert L.dg_image_metrics(d, d, 2, 16, d, d, 0, None) < 0 and b"workspace" in L.dg_last_error()
