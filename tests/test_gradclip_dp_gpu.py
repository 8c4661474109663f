"""Gradient control on the data-parallel path: two gloo ranks on one GPU (the harness of tests/test_dp_gpu.py), 16 px, batch 4 per rank,
seven iterations, every step clipped.  With control on, a generator step is backward -> ONE all-reduce -> statistics -> step on every
dispatch mode (no bucketed exchange, no split backward), the discriminators' step still leaves on the communication stream; the norm is
taken behind the all-reduce, so the ranks decide alike and stay identical."""
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import clip_ref  # noqa: E402
from tests.test_gradclip_gpu import CLIP, same_bits  # noqa: E402

S, N, W, ITERS = 16, 4, 2, 7
# plain: eager, one message per step behind the backward; default: what a data-parallel run below 256 px gets with use_graph=True (the
# segmented-graph exchange); overlap: eager with the bucketed G-step exchange configured -- the one control has to keep from launching
MODES = dict(plain=dict(overlap_comm=False, use_graph=False), default=dict(use_graph=True),
             overlap=dict(overlap_comm=True, use_graph=False, bucket_mb=0.05))


def _worker(rank, world, initfile, outdir, mode):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    try:
        from discogan_modernized_amd import dp
        from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch
        torch.cuda.set_device(0)
        tr = DiscoGANTrainer(default_args(grad_clip=CLIP, nonfinite_guard=True), device="cuda:0", image_size=S, seed=1234,
                             process_group=dist.group.WORLD, **MODES[mode])
        assert tr.world_size == world and tr.grad_control
        assert tr.graph_overlap == (mode == "default") and tr.overlap_comm == (mode == "overlap")
        A, B = synthetic_batch(N, S, dp.rank_data_seed(rank), "cuda:0")
        losses, norms, host = [], [], []
        for i in range(ITERS):
            losses.append(tr.losses_to_floats(tr.train_iteration(A, B, i)))
            if mode == "plain":
                # behind the step the flat buffer still holds the SUM over the ranks; the update saw it times 1 / W
                opt = tr.optim_dis if tr.is_dis_step(i) else tr.optim_gen
                norms.append(opt.grad_stats()["norm"])
                host.append(clip_ref.norm(clip_ref.sumsq(opt.flat_g.cpu().numpy()), 1.0 / world))
        tr.finish()
        torch.cuda.synchronize()
        launched = None if tr._buckets is None else tr._buckets.launched
        cuts = sorted({tuple(v[0].gaps) for k, v in tr._graphs.items() if k[0] == "G"}) if mode == "default" else None
        torch.save(dict(losses=losses, gen=tr.optim_gen.flat_p.cpu(), dis=tr.optim_dis.flat_p.cpu(), norms=norms, host=host,
                        stats_g=tr.optim_gen.grad_stats(), stats_d=tr.optim_dis.grad_stats(), launched=launched, cuts=cuts,
                        numel=max(tr.optim_gen.numel, tr.optim_dis.numel)), os.path.join(outdir, f"rank{rank}.pt"))
        dist.barrier()
        tr.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_clip_alike_in_every_dispatch_mode():
    import torch.multiprocessing as mp
    runs = {}
    for mode in MODES:
        with tempfile.TemporaryDirectory() as d:
            mp.spawn(_worker, args=(W, os.path.join(d, "init"), d, mode), nprocs=W, join=True)
            runs[mode] = [torch.load(os.path.join(d, f"rank{k}.pt")) for k in range(W)]
    base = runs["plain"]
    for mode, r in runs.items():
        # replicas stay identical, and decide alike
        assert same_bits(r[0]["gen"], r[1]["gen"]) and same_bits(r[0]["dis"], r[1]["dis"]), mode
        assert r[0]["stats_g"] == r[1]["stats_g"] and r[0]["stats_d"] == r[1]["stats_d"], mode
        # the modes agree bit for bit
        assert r[0]["losses"] == base[0]["losses"], mode
        assert same_bits(r[0]["gen"], base[0]["gen"]) and same_bits(r[0]["dis"], base[0]["dis"]), mode
        assert r[0]["stats_g"] == base[0]["stats_g"] and r[0]["stats_d"] == base[0]["stats_d"], mode
    sg, sd = base[0]["stats_g"], base[0]["stats_d"]
    assert (sd["steps"], sg["steps"]) == (3, 4) and (sd["clipped"], sg["clipped"]) == (3, 4) and sg["skipped"] == sd["skipped"] == 0
    # no generator step went out in slices: the bucketed exchange launched nothing, the captured G-step has no decoder cut
    assert runs["overlap"][0]["launched"] == 0 and runs["plain"][0]["launched"] is None
    assert runs["default"][0]["cuts"] == [("dis_ready",)]
    # rank 0's norms are those of the averaged gradient
    assert len(base[0]["norms"]) == ITERS
    for i, (got, want) in enumerate(zip(base[0]["norms"], base[0]["host"])):
        assert np.isfinite(got) and abs(got - want) <= base[0]["numel"] * 2.0 ** -53 * want, (i, got, want)
