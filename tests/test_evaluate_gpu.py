"""Held-out evaluation on the GPU: evaluate.evaluate_split against ops.image_metrics and float64, the BatchNorm bookkeeping of an
evaluation event, --eval_interval / --eval_paired of the training CLI (neutrality, shared passes, resume, the files source) and the
stand-alone CLI.  The trainer is 16 px, seed 1234; the split has 4 and 6 images.  The metric bounds are those of
tests/test_metrics_gpu.py (tests/metrics_ref.py): a mean of per-image values each inside a bound is inside it."""
import argparse
import json
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import evaluate, inference, ops  # noqa: E402
from discogan_modernized_amd import image_translation as it_cli  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args  # noqa: E402
from tests import metrics_ref as MR  # noqa: E402

DEV = "cuda"
S = 16
NUM = r"(-?\d+\.\d+|inf|nan)"
LINE = re.compile(rf"^Eval \[(\w+)\] RECON_PSNR: {NUM}/{NUM}, RECON_SSIM: {NUM}/{NUM}, RECON_MAE: {NUM}/{NUM}"
                  rf"(?:, TRANS_PSNR: {NUM}/{NUM}, TRANS_SSIM: {NUM}/{NUM}, TRANS_MAE: {NUM}/{NUM})? \(n=(\d+)/(\d+)\)$")


def _split(nA=4, nB=6, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(nA, 3, S, S, generator=g), torch.rand(nB, 3, S, S, generator=g)


def _counters(tr):
    return [int(v) for net in (tr.generator_A, tr.generator_B) for k, v in net.state_dict().items() if k.endswith("num_batches_tracked")]


# ---- the module -----------------------------------------------------------------------------------------------------------------
def test_evaluate_split_values_and_batchnorm_counters():
    tA, tB = _split()
    split = (tA.to(DEV), tB.to(DEV))
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=1234)
    twin = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=1234)
    c0 = _counters(tr)
    assert c0 and set(c0) == {0}
    res, outs = evaluate.evaluate_split(tr, split, paired=True)
    assert [c - 2 for c in _counters(tr)] == c0                      # one event: two forward calls per generator
    AB, BA, ABA, BAB = twin.sample(*split)
    for a, b in zip(outs, (AB, BA, ABA, BAB)):
        assert torch.equal(a, b)
    pairs = dict(recon_A=(split[0], ABA), recon_B=(split[1], BAB), trans_AB=(split[1][:4], AB[:4]), trans_BA=(split[0][:4], BA[:4]))
    assert set(res) == set(pairs)
    for name, (ref, got) in pairs.items():
        rows = ops.image_metrics(ref, got).cpu()
        assert res[name] == evaluate.summarise(rows), name                   # bit for bit: the same launches, the same host means
        assert res[name]["n"] == len(ref)
        mse, mae = MR.mse_mae_ref(ref, got)
        bound, ssim = MR.ssim_bound(ref.cpu(), got.cpu())
        g = MR.gamma(MR.K_CHAIN)
        assert abs(res[name]["mse"] - float(mse.mean())) <= g * float(mse.mean())
        assert abs(res[name]["mae"] - float(mae.mean())) <= g * float(mae.mean())
        assert abs(res[name]["ssim"] - float(ssim.mean())) <= bound
        # d psnr = 10 / ln 10 * d mse / mse
        assert abs(res[name]["psnr"] - float(MR.psnr_ref(mse).mean())) <= 10 / math.log(10) * g * (1 + g) + 1e-12
        assert res[name]["psnr"] >= 0 and -1 <= res[name]["ssim"] <= 1
    again, same = evaluate.evaluate_split(tr, split, paired=True, outs=outs)
    assert again == res and same is outs
    assert [c - 2 for c in _counters(tr)] == c0                      # passing outs ran no pass
    unpaired, _ = evaluate.evaluate_split(tr, split, paired=False, outs=outs)
    assert set(unpaired) == {"recon_A", "recon_B"} and unpaired["recon_A"] == res["recon_A"]
    res2, _ = evaluate.evaluate_split(tr, split, paired=False)
    assert [c - 4 for c in _counters(tr)] == c0
    assert res2 == unpaired              # train-mode BatchNorm normalises with the split's own statistics: events do not see each other
    del tr, twin


# ---- the training CLI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("evaluate")
    g = torch.Generator().manual_seed(2)
    for name, n in (("A", 16), ("B", 16), ("tA", 4), ("tB", 6)):
        torch.save(torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8), tmp / f"{name}.pt")
    return dict(tmp=tmp, runs={})


def _argv(tmp, tag, extra):
    return ["--task_name", "edges2shoes", "--image_size", str(S), "--batch_size", "4", "--epochs", "3", "--log_interval", "1",
            "--results_dir", str(tmp / f"res_{tag}"), "--models_dir", str(tmp / f"mod_{tag}")] + extra


def _run(work, tag, extra, strip=()):
    """One CLI run per tag, shared by the tests of this module.  strip: attributes removed from the parsed namespace (a caller that
    never heard of them)."""
    if tag not in work["runs"]:
        args = it_cli.parse_args(_argv(work["tmp"], tag, extra))
        if strip:
            args = argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in strip})
        it_cli.train(args)
        work["runs"][tag] = it_cli.train.last_paths
    return work["runs"][tag]


def _tensor_run(work, tag, extra, **kw):
    tmp = work["tmp"]
    return _run(work, tag, ["--data_A", str(tmp / "A.pt"), "--data_B", str(tmp / "B.pt"), "--test_A", str(tmp / "tA.pt"),
                            "--test_B", str(tmp / "tB.pt")] + extra, **kw)


def _lines(rp):
    return open(rp / "eval_log.txt").read().splitlines()


def _load(mp, net, tag="final"):
    return torch.load(mp / f"{net}_{tag}.pth")


def _same_checkpoints(mp_a, mp_b, tag="final"):
    for net in ("gen_A", "gen_B", "dis_A", "dis_B"):
        a, b = _load(mp_a, net, tag), _load(mp_b, net, tag)
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), f"{net}.{k} differs"


def _check_lines(lines, iters, trans, n):
    assert len(lines) == len(iters), lines
    for ln, i in zip(lines, iters):
        m = LINE.match(ln)
        assert m, ln
        assert m.group(1) == str(i) and (m.group(14), m.group(15)) == n
        assert (m.group(8) is not None) == trans, ln
        vals = [float(v) for v in m.groups()[1:13] if v is not None]
        assert all(math.isfinite(v) for v in vals), ln
        for k in range(0, len(vals), 6):
            assert vals[k] >= 0 and vals[k + 1] >= 0                       # PSNR
            assert -1 <= vals[k + 2] <= 1 and -1 <= vals[k + 3] <= 1       # SSIM


def test_cli_eval_only_is_neutral_for_training(work):
    rp_on, mp_on = _tensor_run(work, "eval", ["--eval_interval", "4", "--image_save_interval", "0"])
    rp_off, mp_off = _tensor_run(work, "off", ["--eval_interval", "0", "--image_save_interval", "0"])
    _check_lines(_lines(rp_on), (0, 4, 8), trans=False, n=("4", "6"))
    assert not (rp_on / "samples").exists() and not (rp_off / "eval_log.txt").exists()
    assert open(rp_on / "training_log.txt", "rb").read() == open(rp_off / "training_log.txt", "rb").read()
    for net in ("gen_A", "gen_B"):
        on, off = _load(mp_on, net), _load(mp_off, net)
        for k in on:
            if "running_" in k or k.endswith("num_batches_tracked"):
                assert not torch.equal(on[k], off[k]), k
            else:
                assert torch.equal(on[k], off[k]), k
        nbt = [k for k in on if k.endswith("num_batches_tracked")]
        assert nbt and all(int(on[k]) - int(off[k]) == 2 * 3 for k in nbt)          # three events, two forward calls each
    for net in ("dis_A", "dis_B"):
        a, b = _load(mp_on, net), _load(mp_off, net)
        assert all(torch.equal(a[k], b[k]) for k in a)


def test_cli_eval_paired_on_adds_the_translation_fields(work):
    rp, mp = _tensor_run(work, "paired", ["--eval_interval", "4", "--image_save_interval", "0", "--eval_paired", "on"])
    _check_lines(_lines(rp), (0, 4, 8), trans=True, n=("4", "6"))
    rp_on, mp_on = _tensor_run(work, "eval", ["--eval_interval", "4", "--image_save_interval", "0"])
    assert [ln.split(", TRANS_")[0] for ln in _lines(rp)] == [ln.split(" (n=")[0] for ln in _lines(rp_on)]
    _same_checkpoints(mp, mp_on)


def test_cli_shared_passes_and_default_flags(work):
    rp_both, mp_both = _tensor_run(work, "both", ["--eval_interval", "4", "--image_save_interval", "4"])
    rp_samp, mp_samp = _tensor_run(work, "samp", ["--image_save_interval", "4"])
    _check_lines(_lines(rp_both), (0, 4, 8), trans=False, n=("4", "6"))
    assert sorted(os.listdir(rp_both / "samples")) == sorted(os.listdir(rp_samp / "samples")) == [f"samples_iter_{i}.png" for i in (0, 4, 8)]
    for f in os.listdir(rp_samp / "samples"):
        assert open(rp_both / "samples" / f, "rb").read() == open(rp_samp / "samples" / f, "rb").read()
    _same_checkpoints(mp_both, mp_samp)                                    # the four passes ran once per iteration, for both events
    rp_on, _ = _tensor_run(work, "eval", ["--eval_interval", "4", "--image_save_interval", "0"])
    assert _lines(rp_both) == _lines(rp_on)                                # and the same passes as evaluation alone runs
    # default flags: no eval_log.txt, and bit for bit the run of a caller whose namespace has no such attributes
    assert not (rp_samp / "eval_log.txt").exists()
    rp_old, mp_old = _tensor_run(work, "old", ["--image_save_interval", "4"], strip=("eval_interval", "eval_paired"))
    assert not (rp_old / "eval_log.txt").exists()
    _same_checkpoints(mp_old, mp_samp)
    assert open(rp_old / "training_log.txt", "rb").read() == open(rp_samp / "training_log.txt", "rb").read()


def test_cli_exact_resume_keeps_appending(work):
    tmp = work["tmp"]
    extra = ["--synthetic_size", "16", "--test_A", str(tmp / "tA.pt"), "--test_B", str(tmp / "tB.pt"), "--image_save_interval", "0",
             "--eval_interval", "4", "--model_save_interval", "5", "--save_train_state"]
    rp, mp_full = _run(work, "full", extra)
    full = _lines(rp)
    _check_lines(full, (0, 4, 8), trans=False, n=("4", "6"))
    st = torch.load(mp_full / "train_state_5.pth")
    assert st["iters"] == 6
    rp2, mp_res = _run(work, "resumed", extra + ["--resume", str(mp_full / "train_state_5.pth")])
    assert _lines(rp2) == full[2:]
    _same_checkpoints(mp_full, mp_res, "final")
    _same_checkpoints(mp_full, mp_res, "10")


def test_cli_files_source_scores_the_translations(work, capsys):
    root = work["tmp"] / "three"
    rng = np.random.default_rng(3)
    for split, k in (("train", 9), ("test", 3)):
        d = root / "edges2shoes" / split
        d.mkdir(parents=True)
        for i in range(k):
            Image.fromarray(rng.integers(0, 256, (256, 512, 3), dtype=np.uint8)).save(d / f"{i:03d}_AB.png")
            (d / f"{i:03d}_AB.png").rename(d / f"{i:03d}_AB.jpg")       # PNG bytes under the reference's *.jpg glob: lossless decode
    rp, _ = _run(work, "files", ["--data_root", str(root), "--epochs", "2", "--no_graph", "--eval_interval", "2",
                                 "--image_save_interval", "0"])
    out = capsys.readouterr().out
    assert "data source: files (9 images per domain)" in out
    lines = _lines(rp)
    _check_lines(lines, (0, 2), trans=True, n=("3", "3"))
    assert all(ln in out for ln in lines) and lines[0].endswith("(n=3/3)")


# ---- the stand-alone CLI ---------------------------------------------------------------------------------------------------------
def test_standalone_cli_scores_the_checkpoint_as_inference_runs_it(work, capsys):
    tmp = work["tmp"]
    _, mp = _tensor_run(work, "eval", ["--eval_interval", "4", "--image_save_interval", "0"])
    base = ["--model_path", str(mp), "--test_A", str(tmp / "tA.pt"), "--test_B", str(tmp / "tB.pt"), "--image_size", str(S),
            "--use_extra_layers", "--paired"]
    res = evaluate.main(base + ["--output", str(tmp / "eval.json")])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Eval [final]")]
    assert len(line) == 1 and LINE.match(line[0]) and line[0].endswith("(n=4/6)")
    disk = json.load(open(tmp / "eval.json"))
    assert disk == res and set(res) == {"recon_A", "recon_B", "trans_AB", "trans_BA"}
    tA = ops.u8hwc_to_f32chw(torch.load(tmp / "tA.pt").to(DEV))
    tB = ops.u8hwc_to_f32chw(torch.load(tmp / "tB.pt").to(DEV))
    g_ab, _ = inference.load_generator(mp, "AtoB", S, DEV, True, fold=True)
    g_ba, _ = inference.load_generator(mp, "BtoA", S, DEV, True, fold=True)
    assert isinstance(g_ab, inference.FoldedGenerator)
    AB, BA = g_ab(tA), g_ba(tB)
    ABA, BAB = g_ba(AB), g_ab(BA)
    want = dict(recon_A=(tA, ABA), recon_B=(tB, BAB), trans_AB=(tB[:4], AB[:4]), trans_BA=(tA[:4], BA[:4]))
    for name, (ref, got) in want.items():
        assert disk[name] == evaluate.summarise(ops.image_metrics(ref, got).cpu()), name
    # --no_fold: the training modules in eval() mode.  One forward pass deep (the translations) the outputs agree to the
    # one-forward-pass bound of tests/test_model_gpu.py, d = 1e-4 max|ref| + 1e-5 with max|ref| <= 1 (a sigmoid); MAE is 1-Lipschitz in
    # the output and |d mse| <= 2 d mean|x - y| + d^2 <= 2 d + d^2
    plain = evaluate.main(base + ["--no_fold", "--output", str(tmp / "eval_nofold.json")])
    d = 1e-4 + 1e-5
    for name in ("trans_AB", "trans_BA"):
        assert abs(plain[name]["mae"] - res[name]["mae"]) <= d, name
        assert abs(plain[name]["mse"] - res[name]["mse"]) <= 2 * d + d * d, name
        assert plain[name]["n"] == res[name]["n"] == 4


# ---- two ranks -------------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, initfile, outdir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    try:
        from discogan_modernized_amd import distributed_image_translation as dit
        from discogan_modernized_amd import image_translation as it
        torch.cuda.set_device(0)
        args = dit.parse_args(["--task_name", "edges2shoes", "--image_size", str(S), "--batch_size", "4", "--epochs", "2", "--log_interval", "2",
                               "--data_A", os.path.join(outdir, "A.pt"), "--data_B", os.path.join(outdir, "B.pt"),
                               "--test_A", os.path.join(outdir, "tA.pt"), "--test_B", os.path.join(outdir, "tB.pt"),
                               "--image_save_interval", "0", "--eval_interval", "3",
                               "--results_dir", os.path.join(outdir, f"dp_res_rank{rank}"),
                               "--models_dir", os.path.join(outdir, f"dp_mod_rank{rank}")])
        tr = DiscoGANTrainer(args, device="cuda:0", image_size=S, seed=args.seed, process_group=dist.group.WORLD, use_graph=True)
        it.train(args, trainer=tr, rank=rank, world_size=world, is_main=(rank == 0), process_group=dist.group.WORLD)
        tr.finish()
        torch.cuda.synchronize()
        torch.save(dict(gen=tr.optim_gen.flat_p.cpu(), dis=tr.optim_dis.flat_p.cpu(),
                        nbt=int(tr.generator_A.encoder[3].num_batches_tracked)), os.path.join(outdir, f"dp_rank{rank}.pt"))
        dist.barrier()
        tr.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_only_rank0_evaluates_and_replicas_stay_identical(work):
    """Data-parallel rehearsal (two ranks on the one GPU, gloo): rank 0 alone loads the split and writes eval_log.txt; the weights of
    both ranks stay bitwise equal."""
    import torch.multiprocessing as mp
    tmp = work["tmp"]
    g = torch.Generator().manual_seed(4)
    for name in ("A", "B"):                              # 32 training images: a 16-image shard per rank
        torch.save(torch.randint(0, 256, (32, S, S, 3), generator=g, dtype=torch.uint8), tmp / f"dp_{name}.pt")
    d = tmp / "dp"
    d.mkdir()
    for name in ("A", "B"):
        os.replace(tmp / f"dp_{name}.pt", d / f"{name}.pt")
    for name in ("tA", "tB"):
        torch.save(torch.load(tmp / f"{name}.pt"), d / f"{name}.pt")
    mp.spawn(_dp_worker, args=(2, str(d / "init"), str(d)), nprocs=2, join=True)
    found = [os.path.join(root, f) for root, _, files in os.walk(d) for f in files if f == "eval_log.txt"]
    assert len(found) == 1 and "dp_res_rank0" in found[0], found
    _check_lines(open(found[0]).read().splitlines(), (0, 3, 6), trans=False, n=("4", "6"))
    r0, r1 = (torch.load(d / f"dp_rank{k}.pt") for k in range(2))
    for k in ("gen", "dis"):
        assert torch.equal(r0[k], r1[k]), k
    assert r1["nbt"] == 16 and r0["nbt"] == 16 + 2 * 3              # 8 iterations, two passes each; rank 0's three events on top
