"""Adaptive discriminator augmentation on the GPU: the gated draw, the window and the controller kernels against tests/ada_ref.py (bitwise /
exact), DiffAugment(p=...) through the apply kernels against diffaug_ref on the gated records (bitwise for the geometry-only policy; with
colour the criterion of tests/test_diffaug_gpu.py, restated here: four times the float32 reference's own error against float64, at least
one ulp of the value bound 8), and the trainer: schedules, graph replay, the overlapped variants, resume, the log line, two ranks."""
import os
import re
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, ops  # noqa: E402
from discogan_modernized_amd.diffaug import AdaController, DiffAugment, fixed_p  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tests import ada_ref as AR  # noqa: E402
from tests import diffaug_ref as DR  # noqa: E402

DEV = "cuda"
BAND = 16
SENTINEL = 0x5EA7BEEF
FLOOR = 2.0 ** -20                         # one ulp at the value bound |v| < 8
P_VALUES = (0.0, 2.0 ** -24, 0.3, 1.0 - 2.0 ** -24, 1.0)
KEYS = ((1234, 0, 6, 0, 0), (1234, 3, 7, 1, 1), ((1 << 63) + 5, 1, (1 << 33) + 1, 1, 0))


def _p_dev(p):
    return torch.tensor([p], dtype=torch.float64, device=DEV)


# ---- 1. the gated draw ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (8, 9, 64))
@pytest.mark.parametrize("n", (1, 255, 257, 4096))
def test_device_draw_p_is_the_reference_table(n, S):
    keys = KEYS if n < 4096 else KEYS[:1]
    for flags in ((7, 1, 6, 5) if n < 4096 else (7,)):
        for key in keys:
            full, u = DR.draw(*key, n, S, flags), AR.gates(*key, n)
            for p in P_VALUES:
                got = ops.diffaug_draw_p(*key, n, S, flags, _p_dev(p))
                assert got.dtype == torch.int32 and tuple(got.shape) == (n, 8)
                want = AR.gate(full, u < np.float32(p), S, flags)
                assert np.array_equal(got.cpu().numpy(), want), (key, flags, p)
            assert torch.equal(ops.diffaug_draw_p(*key, n, S, flags, _p_dev(1.0)), ops.diffaug_draw(*key, n, S, flags, device=DEV))
    table = torch.full((n + 3, 8), -7, dtype=torch.int32, device=DEV)                     # rows past n stay as they are
    ops.diffaug_draw_p(*KEYS[0], n, S, 7, _p_dev(0.3), out=table)
    assert np.array_equal(table[:n].cpu().numpy(), AR.draw_p(*KEYS[0], n, S, 7, 0.3)) and bool((table[n:] == -7).all())


def test_p_is_read_on_the_device_at_the_time_of_the_draw():
    """ctl[0] rewritten by a device copy between two draws, nothing synchronised in between: the second table is the new p's."""
    n, S = 257, 9
    ctl = torch.zeros(8, dtype=torch.float64, device=DEV)
    new_p = _p_dev(0.75)
    t1 = torch.zeros((n, 8), dtype=torch.int32, device=DEV)
    t2 = torch.zeros((n, 8), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ops.diffaug_draw_p(*KEYS[0], n, S, 7, ctl, out=t1)
    ctl[0:1].copy_(new_p)
    ops.diffaug_draw_p(*KEYS[0], n, S, 7, ctl, out=t2)
    torch.cuda.synchronize()
    assert np.array_equal(t1.cpu().numpy(), AR.draw_p(*KEYS[0], n, S, 7, 0.0))
    assert np.array_equal(t2.cpu().numpy(), AR.draw_p(*KEYS[0], n, S, 7, 0.75))
    assert not torch.equal(t1, t2)
    for bad in (torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.float64), 0.5):
        with pytest.raises(_lib.DiscoganHipError, match="float64 HIP tensor"):
            ops.diffaug_draw_p(*KEYS[0], n, S, 7, bad, out=t1)


# ---- 2. the window -------------------------------------------------------------------------------------------------------------------------
def _banded(values, dtype):
    """``values`` as a device tensor of ``dtype`` with a band of sentinel words on either side: (the whole buffer as int32, the view)."""
    k = len(values) * torch.empty((), dtype=dtype).element_size() // 4
    raw = torch.from_numpy(np.full(2 * BAND + k, SENTINEL, dtype=np.int32)).to(DEV)
    view = raw[BAND:BAND + k].view(dtype)
    view.copy_(torch.as_tensor(np.asarray(values), dtype=dtype))
    return raw, view


def _bands_intact(raw, view):
    k = view.numel() * view.element_size() // 4
    return bool((raw[:BAND] == SENTINEL).all() and (raw[BAND + k:] == SENTINEL).all())


@pytest.mark.parametrize("n", (1, 63, 64, 255, 256, 257, 1000, 65536))
def test_accumulate_is_exact(n):
    rng = np.random.default_rng(n)
    for thr in (0.0, 0.5, -1.25):
        v = rng.standard_normal(n).astype(np.float32) + np.float32(thr)
        special = np.array([0.0, -0.0, thr, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39, np.nextafter(np.float32(thr), np.float32(9)),
                            np.nextafter(np.float32(thr), np.float32(-9))], dtype=np.float32)
        k = min(n, len(special))
        v[rng.permutation(n)[:k]] = special[:k]
        for start in ((0.0, 0.0), (-3.0, 7.0)):
            buf, acc = _banded(start, torch.float32)
            x = torch.from_numpy(v).to(DEV)
            ops.ada_accumulate(x, thr, acc)
            ops.ada_accumulate(x.view(-1, 1, 1, 1), thr, acc)                                   # a discriminator's output shape; twice onto the window
            want = AR.accumulate(AR.accumulate(np.array(start, dtype=np.float32), v, thr), v, thr)
            assert acc.cpu().numpy().tolist() == want.tolist(), (n, thr, start)
            assert _bands_intact(buf, acc)
    with pytest.raises(_lib.DiscoganHipError, match="fp32"):
        ops.ada_accumulate(torch.zeros(4, device=DEV, dtype=torch.float64), 0.0, torch.zeros(2, device=DEV))
    with pytest.raises(_lib.DiscoganHipError, match="window"):
        ops.ada_accumulate(torch.zeros(4, device=DEV), 0.0, torch.zeros(3, device=DEV))


# ---- 3. the controller ---------------------------------------------------------------------------------------------------------------------
def test_update_follows_the_reference_bitwise():
    """A scripted sequence of windows: up, the clamp at p_max, down, r_t == target, an empty window, the clamp at 0, and steps that do not
    round to short binary fractions (so a fused multiply-add in front of the clamp would show)."""
    up, down = np.ones(8, dtype=np.float32), -np.ones(8, dtype=np.float32)
    half = np.array([1, 1, 1, -1, 0, 0, 0, 0], dtype=np.float32)
    rng = np.random.default_rng(11)
    script = [[up], [up, up], [down], [half], [], [down] * 4, [up] * 9] + [[rng.standard_normal(37).astype(np.float32)] for _ in range(12)]
    for target, step, p_max, p0 in ((0.25, 1.0 / 64, 0.5, 0.25), (0.25, 1.0 / 300, 0.7, 0.1), (0.6, 1.0 / (1000 * 0.37), 1.0, 0.0)):
        ref_ctl, ref_acc = AR.new_ctl(p0), AR.new_acc()
        cbuf, ctl = _banded(ref_ctl, torch.float64)
        abuf, acc = _banded(ref_acc, torch.float32)
        moved = set()
        for batches in script:
            for b in batches:
                AR.accumulate(ref_acc, b, 0.0)
                ops.ada_accumulate(torch.from_numpy(b).to(DEV), 0.0, acc)
            assert acc.cpu().numpy().tolist() == ref_acc.tolist()
            AR.update(ref_ctl, ref_acc, target, step, p_max)
            ops.ada_update(ctl, acc, target, step, p_max)
            got = ctl.cpu().numpy()
            assert np.array_equal(got.view(np.int64), ref_ctl.view(np.int64)), (target, step, got.tolist(), ref_ctl.tolist())
            assert acc.cpu().numpy().tolist() == [0.0, 0.0]
            moved.add(float(np.sign(got[4])))
        assert {-1.0, 1.0} <= moved and (target != 0.25 or 0.0 in moved) and _bands_intact(cbuf, ctl) and _bands_intact(abuf, acc)
    with pytest.raises(_lib.DiscoganHipError, match="control block"):
        ops.ada_update(torch.zeros(8, device=DEV), torch.zeros(2, device=DEV), 0.6, 1e-3)


# ---- 4. DiffAugment(p=...) through the apply kernels ---------------------------------------------------------------------------------------
def _bound(ref32, ref64):
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    return max(4.0 * e_ref, FLOOR), e_ref


@pytest.mark.parametrize("S", (8, 9, 64))
def test_gated_records_through_the_apply_kernels(S):
    n = 5
    rng = np.random.default_rng(300 + S)
    x_np = rng.random((n, 3, S, S), dtype=np.float32)
    dz_np = rng.standard_normal((n, 3, S, S)).astype(np.float32)
    w = torch.from_numpy(dz_np).to(DEV)
    for it in (3, 4):                                                 # two draws: different stages gated off
        aug = DiffAugment(DR.ALL, S, seed=1234, rank=0, domain=1, role=1, device=DEV, p=fixed_p(0.3, DEV))
        recs = aug.draw(it, n).cpu().numpy()
        assert np.array_equal(recs, AR.draw_p(1234, 0, it, 1, 1, n, S, DR.ALL, 0.3))
        x = torch.from_numpy(x_np).to(DEV).requires_grad_(True)
        z = aug.apply(x)
        (z * w).sum().backward()
        for name, got, ref, inp in (("fwd", z.detach(), DR.forward, x_np), ("bwd", x.grad, DR.backward, dz_np)):
            want = ref(inp.astype(np.float64), recs, DR.ALL)
            bound, e_ref = _bound(ref(inp, recs, DR.ALL, np.float32), want)
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
            print(f"S {S} iteration {it} {name}: err {err:.3e} e_ref {e_ref:.3e} bound {bound:.3e}")
            assert err <= bound, (name, err, bound)
    keep = np.concatenate([AR.keep_mask(1234, 0, it, 1, 1, n, 0.3) for it in (3, 4)])
    assert keep.any() and not keep.all()
    # geometry-only policy at p = 0: the output bits are the input bits, the gradient bits are dz's
    geo = DR.TRANSLATION | DR.CUTOUT
    aug = DiffAugment(geo, S, seed=1234, rank=0, domain=0, role=0, device=DEV, p=fixed_p(0.0, DEV))
    aug.draw(3, n)
    bits = rng.integers(-2 ** 31, 2 ** 31, (n, 3, S, S), dtype=np.int64).astype(np.int32)
    bits[0, 0, 0, :3] = (0x7FC00001, 0x00000001, -0x00400001)
    xb = torch.from_numpy(bits).to(DEV).view(torch.float32)
    assert torch.equal(ops.diffaug_fwd(xb, geo, aug.recs).view(torch.int32), xb.view(torch.int32))
    assert torch.equal(ops.diffaug_bwd(xb, geo, aug.recs).view(torch.int32), xb.view(torch.int32))
    x = torch.from_numpy(x_np).to(DEV).requires_grad_(True)
    z = aug.apply(x)
    (z * w).sum().backward()
    assert torch.equal(z.detach().view(torch.int32), x.detach().view(torch.int32)) and torch.equal(x.grad.view(torch.int32), w.view(torch.int32))


# ---- 5. the trainer ------------------------------------------------------------------------------------------------------------------------
S_T, N_T = 16, 4
POLICY = "color,translation,cutout"
ADA = dict(diffaug=POLICY, diffaug_p=0.3, ada_target=0.6, ada_interval=2, ada_kimg=0.1)     # 8 images a window: p moves by 0.08
UI = 3                                                                                      # update_interval of default_args
ITERS = 4 * 2 * UI
_RUNS = {}


def _snapshot(tr):
    tr.finish()
    torch.cuda.synchronize()
    snap = {f"{side}.{name}": getattr(opt, name).cpu().clone() for side, opt in (("gen", tr.optim_gen), ("dis", tr.optim_dis))
            for name in ("flat_p", "exp_avg", "exp_avg_sq")}
    for k, net in tr.nets.items():
        for name, buf in net.named_buffers():
            snap[f"{k}.{name}"] = buf.detach().cpu().clone()
    if tr.ada is not None:
        snap["ada.ctl"], snap["ada.acc"] = tr.ada.ctl.cpu().clone(), tr.ada.acc.cpu().clone()
    return snap


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _differ(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in sorted(a) if not torch.equal(_bits(a[k]), _bits(b[k]))]


def _run(key, iters=ITERS, first=0, state=None, args=None, **kw):
    """Iterations ``first .. iters - 1`` of one trainer on one fixed batch; per D-step the discriminators' outputs on the real batches."""
    if key not in _RUNS:
        A, B = synthetic_batch(N_T, S_T, 5, DEV)
        tr = DiscoGANTrainer(default_args(**(ADA if args is None else args)), device=DEV, image_size=S_T, seed=1234, **kw)
        if state is not None:
            assert tr.load_train_state(state) == first
        reals, losses = {}, []
        for i in range(first, iters):
            out = tr.train_iteration(A, B, i)
            losses.append(tr.losses_to_floats(out))
            if tr.is_dis_step(i):
                reals[i] = (out.A_dis_real.detach().cpu().clone(), out.B_dis_real.detach().cpu().clone())
        _RUNS[key] = dict(last=_snapshot(tr), state=tr.train_state(iters), reals=reals, losses=losses, grouped=bool(tr.group_launch),
                          log=tr.format_log(iters - 1, iters, out), threshold=tr.ada_threshold)
        del tr
    return _RUNS[key]


def _reference_ctl(reals_per_step, threshold, p0=0.3, interval=2, kimg=0.1, target=0.6):
    """tests/ada_ref.py's controller fed the run's own outputs: per D-step a list of (A outputs, B outputs), one pair per rank."""
    ctl, acc = [AR.new_ctl(p0), AR.new_ctl(p0)], [AR.new_acc(), AR.new_acc()]
    for k, ranks in enumerate(reals_per_step, start=1):
        for pair in ranks:
            for d in (0, 1):
                AR.accumulate(acc[d], pair[d].numpy(), threshold)
        if k % interval == 0:
            for d in (0, 1):
                AR.update(ctl[d], acc[d], target, AR.step_per_image(kimg))
    return np.stack(ctl), np.concatenate(acc)


def test_p_one_without_a_controller_is_the_step_without_the_feature():
    base = _run("base", iters=6, args=dict(diffaug=POLICY))
    one = _run("p_one", iters=6, args=dict(diffaug=POLICY, diffaug_p=1.0))
    assert _differ(one["last"], base["last"]) == [] and one["losses"] == base["losses"]
    assert "ADA" not in base["log"] and "ada" not in base["state"]
    half = _run("p_half", iters=6, args=dict(diffaug=POLICY, diffaug_p=0.5))              # a fixed p below 1 parts from it
    assert "dis.flat_p" in _differ(half["last"], base["last"]) and "ADA" not in half["log"]


def test_controller_follows_the_reference_on_the_runs_own_outputs():
    run = _run("chain", group_launch=False)
    assert sorted(run["reals"]) == list(range(0, ITERS, UI)) and run["threshold"] == 0.5
    ctl, acc = _reference_ctl([[run["reals"][i]] for i in sorted(run["reals"])], 0.5)
    got = run["last"]["ada.ctl"].numpy()
    print("ctl A", got[0, :5].tolist(), "ctl B", got[1, :5].tolist())
    assert np.array_equal(got.view(np.int64), ctl.view(np.int64)), (got.tolist(), ctl.tolist())
    assert run["last"]["ada.acc"].numpy().tolist() == acc.tolist() == [0.0] * 4
    assert got[0, 2] == got[1, 2] == 4 and got[0, 3] == got[1, 3] == 4 * 2 * N_T
    assert abs(got[0, 4]) == abs(got[1, 4]) == 2 * N_T * AR.step_per_image(0.1)          # p moved at the last update
    assert re.search(r" ADA: p \d\.\d{4}/\d\.\d{4} rt -?\d\.\d{3}/-?\d\.\d{3}$", run["log"]), run["log"]
    assert f" ADA: p {got[0, 0]:.4f}/{got[1, 0]:.4f} rt {got[0, 1]:.3f}/{got[1, 1]:.3f}" in run["log"]
    assert run["state"]["ada"]["dsteps"] == 8 and torch.equal(run["state"]["ada"]["ctl"], run["last"]["ada.ctl"])
    lsgan = _run("chain_lsgan", iters=2 * UI, args=dict(ADA, gan_loss="lsgan", gan_real_label=0.9), group_launch=False)
    assert lsgan["threshold"] == 0.45
    ctl, _ = _reference_ctl([[lsgan["reals"][i]] for i in sorted(lsgan["reals"])], 0.45)
    assert np.array_equal(lsgan["last"]["ada.ctl"].numpy().view(np.int64), ctl.view(np.int64))


@pytest.mark.parametrize("name,kw", [
    ("chain_graph", dict(group_launch=False, use_graph=True)),
    ("grouped_single", dict(group_launch=True, group_plan="single")),
    ("grouped_single_graph", dict(group_launch=True, group_plan="single", use_graph=True)),
    ("chain_overlap", dict(group_launch=False, overlap_comm=True)),
    ("chain_seggraph", dict(group_launch=False, overlap_comm="graph", use_graph=True)),
])
def test_schedules_and_dispatch_modes_agree_bitwise(name, kw):
    """Against the two-chain schedule dispatched eagerly: graph replay, the grouped schedule (with single plans, which is bitwise the
    two-chain one), and the overlapped variants, where the discriminators' step and the controller run on the communication stream."""
    chain, other = _run("chain", group_launch=False), _run(name, **kw)
    assert other["grouped"] == name.startswith("grouped")
    assert _differ(other["last"], chain["last"]) == [] and other["losses"] == chain["losses"]
    for i in chain["reals"]:
        for d in (0, 1):
            assert torch.equal(_bits(other["reals"][i][d]), _bits(chain["reals"][i][d])), (i, d)


def test_resume_continues_bitwise(tmp_path):
    whole = _run("grouped")
    assert whole["grouped"]
    torch.save(_run("grouped_head", iters=ITERS // 2)["state"], tmp_path / "state.pth")
    st = torch.load(tmp_path / "state.pth")
    assert st["iters"] == ITERS // 2 and st["ada"]["dsteps"] == 4
    tail = _run("grouped_tail", first=ITERS // 2, state=st)
    assert _differ(tail["last"], whole["last"]) == []
    assert torch.equal(tail["state"]["ada"]["ctl"].view(torch.int64), whole["state"]["ada"]["ctl"].view(torch.int64))
    # a state without the entry: p starts from its initial value
    del st["ada"]
    tr = DiscoGANTrainer(default_args(**ADA), device=DEV, image_size=S_T, seed=1234)
    tr.ada.ctl.fill_(0.9)
    tr.load_train_state(st)
    s = tr.ada.stats()
    assert s["p"] == (0.3, 0.3) and s["updates"] == (0, 0) and np.isnan(s["rt"][0]) and tr.ada.dsteps == 0


def test_controller_object_validates_and_round_trips_its_state():
    for bad in (dict(target=0.0), dict(target=1.0), dict(target=0.6, interval=0), dict(target=0.6, kimg=0.0), dict(target=0.6, p_max=0.0),
                dict(target=0.6, p0=1.5)):
        with pytest.raises(ValueError, match="ada_|diffaug_p"):
            AdaController(device=DEV, **bad)
    a = AdaController(0.6, interval=1, kimg=0.001, p_max=0.8, p0=0.5, device=DEV)
    a.accumulate(1, torch.ones(4, 1, 1, 1, device=DEV), 0.0)
    b = AdaController(0.6, interval=1, kimg=0.001, p_max=0.8, p0=0.0, device=DEV)
    b.load_state_dict(a.state_dict())
    for c in (a, b):
        assert c.step() is True
    sa, sb = a.stats(), b.stats()
    assert sa["p"] == sb["p"] == (0.5, 0.8) and sa["images"] == sb["images"] == (0, 4) and sa["updates"] == sb["updates"] == (0, 1)
    assert np.isnan(sa["rt"][0]) and sa["rt"][1] == sb["rt"][1] == 1.0


# ---- 6. two ranks --------------------------------------------------------------------------------------------------------------------------
W, DP_ITERS = 2, 3 * UI + 1                         # D-steps at 0, 3, 6, 9: two windows of two


def _worker(rank, world, initfile, outdir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    try:
        from discogan_modernized_amd import dp
        from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch
        torch.cuda.set_device(0)
        tr = DiscoGANTrainer(default_args(**ADA), device="cuda:0", image_size=S_T, seed=1234, process_group=dist.group.WORLD,
                             overlap_comm=True, use_graph=False, bucket_mb=0.05)
        assert tr.world_size == world and tr.overlap_comm and tr.ada is not None
        A, B = synthetic_batch(N_T, S_T, dp.rank_data_seed(rank), "cuda:0")
        reals = {}
        for it in range(DP_ITERS):
            out = tr.train_iteration(A, B, it)
            if tr.is_dis_step(it):
                reals[it] = (out.A_dis_real.detach().cpu().clone(), out.B_dis_real.detach().cpu().clone())
        tr.finish()
        torch.cuda.synchronize()
        torch.save(dict(ctl=tr.ada.ctl.cpu(), acc=tr.ada.acc.cpu(), reals=reals, dis=tr.optim_dis.flat_p.cpu()), os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_share_one_controller_state():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(W, os.path.join(d, "init"), d), nprocs=W, join=True)
        r = [torch.load(os.path.join(d, f"rank{k}.pt")) for k in range(W)]
    assert torch.equal(r[0]["ctl"].view(torch.int64), r[1]["ctl"].view(torch.int64)) and torch.equal(r[0]["dis"], r[1]["dis"])
    assert r[0]["acc"].tolist() == r[1]["acc"].tolist() == [0.0] * 4
    steps = sorted(r[0]["reals"])
    assert steps == [0, 3, 6, 9]
    assert not torch.equal(r[0]["reals"][9][0], r[1]["reals"][9][0])                      # different shards
    ctl, _ = _reference_ctl([[r[0]["reals"][i], r[1]["reals"][i]] for i in steps], 0.5)
    got = r[0]["ctl"].numpy()
    assert np.array_equal(got.view(np.int64), ctl.view(np.int64)), (got.tolist(), ctl.tolist())
    assert got[0, 2] == 2 and got[0, 3] == 2 * 2 * N_T * W
