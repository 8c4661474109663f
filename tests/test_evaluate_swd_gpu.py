"""--eval_swd / --swd on the GPU: evaluate_split with SWD objects against SWD.score on the same outputs, the BatchNorm bookkeeping,
the neutrality of the flag for training (checkpoints, training_log.txt, the old fields of eval_log.txt), resume, the stand-alone CLI
and the SWD_DOMAINS line.  The trainer is 16 px, seed 1234; the split has 4 and 6 images, as in tests/test_evaluate_gpu.py."""
import json
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import evaluate, ops  # noqa: E402
from discogan_modernized_amd import image_translation as it_cli  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args  # noqa: E402

DEV = "cuda"
S = 16
NUM = r"(-?\d+\.\d+|inf|nan)"
SWD_TAIL = re.compile(rf", SWD_AB: {NUM}={NUM}, SWD_BA: {NUM}={NUM} \(n=4/6\)( \[ema\])?$")
DOMAINS = re.compile(rf"^SWD_DOMAINS: {NUM}={NUM} \(n=4, 128 patches per image\)$")


def _split(nA=4, nB=6, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(nA, 3, S, S, generator=g).to(DEV), torch.rand(nB, 3, S, S, generator=g).to(DEV)


def _counters(tr):
    return [int(v) for net in (tr.generator_A, tr.generator_B) for k, v in net.state_dict().items() if k.endswith("num_batches_tracked")]


def test_evaluate_split_with_swd_adds_two_entries_and_runs_no_extra_pass():
    split = _split()
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=1234)
    c0 = _counters(tr)
    swd, domains = evaluate.make_swd_pair(*split, S, seed=0)
    assert swd[0].n == swd[1].n == 4 and swd[0].patches == 128 and domains["n"] == 4 and len(domains["levels"]) == 1
    assert domains == swd[0].score(split[0]) and domains["mean"] > 0
    assert domains == swd[1].score(split[1])                           # symmetric in its sets
    assert _counters(tr) == c0                                          # references and the domain gap run no generator
    for paired in (True, False):
        plain, outs = evaluate.evaluate_split(tr, split, paired=paired)
        c1 = _counters(tr)
        res, same = evaluate.evaluate_split(tr, split, paired=paired, outs=outs, swd=swd)
        assert same is outs and _counters(tr) == c1                     # passing outs runs no pass
        assert set(res) == set(plain) | {"swd_AB", "swd_BA"} and len(plain) == (4 if paired else 2)
        for k in plain:
            assert res[k] == plain[k]                                   # the old entries, unchanged
        AB, BA = outs[0], outs[1]
        assert res["swd_AB"] == swd[0].score(AB) and res["swd_BA"] == swd[1].score(BA)           # bit for bit
        assert res["swd_AB"]["n"] == res["swd_BA"]["n"] == 4
        assert all(math.isfinite(v) and v > 0 for v in res["swd_AB"]["levels"] + res["swd_BA"]["levels"])
        line = evaluate.format_eval(3, res)
        assert SWD_TAIL.search(line) and line.replace(SWD_TAIL.search(line).group(0), " (n=4/6)") == evaluate.format_eval(3, plain)
    fresh, _ = evaluate.evaluate_split(tr, split, paired=False, swd=swd)
    assert [c - 2 for c in _counters(tr)] == c1                          # without outs: one event's passes, as without SWD
    assert fresh["swd_AB"] == res["swd_AB"]              # train-mode BatchNorm: events do not see each other
    del tr


# ---- the CLIs -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("evaluate_swd")
    g = torch.Generator().manual_seed(2)
    for name, n in (("A", 16), ("B", 16), ("tA", 4), ("tB", 6)):
        torch.save(torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8), tmp / f"{name}.pt")
    return dict(tmp=tmp, runs={})


def _run(work, tag, extra, capsys=None):
    if tag not in work["runs"]:
        tmp = work["tmp"]
        argv = ["--task_name", "edges2shoes", "--image_size", str(S), "--batch_size", "4", "--epochs", "2", "--log_interval", "1",
                "--results_dir", str(tmp / f"res_{tag}"), "--models_dir", str(tmp / f"mod_{tag}"), "--data_A", str(tmp / "A.pt"),
                "--data_B", str(tmp / "B.pt"), "--test_A", str(tmp / "tA.pt"), "--test_B", str(tmp / "tB.pt"),
                "--image_save_interval", "0"] + extra
        if capsys is not None:
            capsys.readouterr()
        it_cli.train(it_cli.parse_args(argv))
        work["runs"][tag] = it_cli.train.last_paths + (capsys.readouterr().out if capsys is not None else "",)
    return work["runs"][tag]


def _lines(rp):
    return open(rp / "eval_log.txt").read().splitlines()


def _same_checkpoints(mp_a, mp_b, tag="final"):
    for net in ("gen_A", "gen_B", "dis_A", "dis_B"):
        a, b = torch.load(mp_a / f"{net}_{tag}.pth"), torch.load(mp_b / f"{net}_{tag}.pth")
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), f"{net}.{k} differs"


def test_cli_eval_swd_changes_nothing_but_the_appended_fields(work, capsys):
    rp_on, mp_on, out_on = _run(work, "swd", ["--eval_interval", "2", "--eval_swd"], capsys)
    rp_off, mp_off, out_off = _run(work, "plain", ["--eval_interval", "2"], capsys)
    _same_checkpoints(mp_on, mp_off)
    assert open(rp_on / "training_log.txt", "rb").read() == open(rp_off / "training_log.txt", "rb").read()
    on, off = _lines(rp_on), _lines(rp_off)
    assert len(on) == len(off) == 4                                    # 8 iterations, events at 0, 2, 4, 6
    for a, b in zip(on, off):
        m = SWD_TAIL.search(a)
        assert m, a
        assert a[:m.start()] + " (n=4/6)" == b
        assert all(math.isfinite(float(v)) and float(v) > 0 for v in m.groups()[:4])
        assert a in out_on
    dom = [ln for ln in out_on.splitlines() if ln.startswith("SWD_DOMAINS")]
    assert len(dom) == 1 and DOMAINS.match(dom[0]), dom                 # once, at the start
    assert "SWD" not in out_off
    assert out_on.index(dom[0]) < out_on.index(on[0])


def test_cli_resume_reproduces_the_event_numbers(work, capsys):
    extra = ["--eval_interval", "2", "--eval_swd", "--model_save_interval", "3", "--save_train_state"]
    rp, mp, _ = _run(work, "full", extra, capsys)
    full = _lines(rp)
    rp2, mp2, out = _run(work, "resumed", extra + ["--resume", str(mp / "train_state_3.pth")], capsys)
    assert _lines(rp2) == full[2:]                                      # the events at 4 and 6, the same bits
    assert len([ln for ln in out.splitlines() if ln.startswith("SWD_DOMAINS")]) == 1
    _same_checkpoints(mp, mp2)
    rp_on, _, _ = _run(work, "swd", ["--eval_interval", "2", "--eval_swd"], capsys)
    assert _lines(rp_on) == full                                        # saving checkpoints does not move the numbers either


def test_cli_eval_swd_seed_moves_the_swd_fields_only(work, capsys):
    rp_on, mp_on, _ = _run(work, "swd", ["--eval_interval", "2", "--eval_swd"], capsys)
    rp_s, mp_s, _ = _run(work, "seed9", ["--eval_interval", "2", "--eval_swd", "--eval_swd_seed", "9"], capsys)
    _same_checkpoints(mp_on, mp_s)
    for a, b in zip(_lines(rp_on), _lines(rp_s)):
        ma, mb = SWD_TAIL.search(a), SWD_TAIL.search(b)
        assert a[:ma.start()] == b[:mb.start()] and ma.group(0) != mb.group(0)


def test_standalone_cli_writes_the_three_keys(work, capsys):
    tmp = work["tmp"]
    _, mp, _ = _run(work, "swd", ["--eval_interval", "2", "--eval_swd"], capsys)
    base = ["--model_path", str(mp), "--test_A", str(tmp / "tA.pt"), "--test_B", str(tmp / "tB.pt"), "--image_size", str(S), "--use_extra_layers"]
    capsys.readouterr()
    res = evaluate.main(base + ["--swd", "--output", str(tmp / "eval_swd.json")])
    out = capsys.readouterr().out.splitlines()
    plain = evaluate.main(base + ["--output", str(tmp / "eval_plain.json")])
    out_plain = capsys.readouterr().out
    disk = json.load(open(tmp / "eval_swd.json"))
    assert disk == res and set(res) == {"recon_A", "recon_B", "swd_AB", "swd_BA", "swd_domains"}
    assert set(plain) == {"recon_A", "recon_B"} and all(res[k] == plain[k] for k in plain) and "SWD" not in out_plain
    assert json.load(open(tmp / "eval_plain.json")) == plain
    for k in ("swd_AB", "swd_BA", "swd_domains"):
        assert set(res[k]) == {"levels", "mean", "n", "patches"} and res[k]["n"] == 4 and res[k]["patches"] == 128 and res[k]["mean"] > 0
    assert len([ln for ln in out if DOMAINS.match(ln)]) == 1
    line = [ln for ln in out if ln.startswith("Eval [final]")]
    assert len(line) == 1 and SWD_TAIL.search(line[0])
    # the domain gap is what SWD gives for the two test sets, whatever the checkpoint
    tA = ops.u8hwc_to_f32chw(torch.load(tmp / "tA.pt").to(DEV))
    tB = ops.u8hwc_to_f32chw(torch.load(tmp / "tB.pt").to(DEV))
    assert evaluate.SWD(4, S, DEV).set_reference(tB).score(tA) == res["swd_domains"]
