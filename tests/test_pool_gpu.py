"""Image history pool on the GPU: the device draw against its numpy restatement, the exchange kernel against the reference application
of hand-made and drawn tables, the host ImagePool against an independent sequential pool, and the trainer / CLI with ``image_pool``.

Every comparison is bitwise: the feature only copies and indexes.  Image data for the kernel tests is random int32 bit patterns viewed
as float (NaNs, infinities and denormals among them), compared as int32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, ops  # noqa: E402
from discogan_modernized_amd import image_translation as it_cli  # noqa: E402
from discogan_modernized_amd.pool import ImagePool  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tests import pool_ref as PR  # noqa: E402

DEV = "cuda"
BAND = 64                                  # sentinel floats in front of and behind every buffer of the kernel tests
SENTINEL = 0x5EA7BEEF
BIG_SEED, BIG_ITER = (1 << 63) + 5, (1 << 33) + 1


def _patterns(shape, seed):
    return np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)


class _Banded:
    """``rows`` images of ``elems`` floats inside a device buffer with a sentinel band on either side; ``shift`` floats of extra offset
    move the base off the 16-byte boundary."""

    def __init__(self, values, shift=0):
        self.rows, self.elems = values.shape
        self.lo = BAND + shift
        host = np.full(self.lo + values.size + BAND, SENTINEL, dtype=np.int32)
        host[self.lo:self.lo + values.size] = values.reshape(-1)
        self.buf = torch.from_numpy(host).to(DEV)

    def view(self, image_shape):
        return self.buf[self.lo:self.lo + self.rows * self.elems].view(torch.float32).view((self.rows,) + tuple(image_shape))

    def values(self):
        return self.buf[self.lo:self.lo + self.rows * self.elems].cpu().numpy().reshape(self.rows, self.elems)

    def bands_intact(self):
        host = self.buf.cpu().numpy()
        return bool((host[:self.lo] == SENTINEL).all() and (host[self.lo + self.rows * self.elems:] == SENTINEL).all())


def _exchange_and_check(x_np, pool_np, recs_np, S, shift=0):
    """One dg_pool_exchange on banded buffers against PR.apply_records: out, pool, x untouched, bands untouched."""
    n, P = len(x_np), len(pool_np)
    x, pool, out = _Banded(x_np, shift), _Banded(pool_np, shift), _Banded(np.full_like(x_np, 7), shift)
    recs = torch.from_numpy(np.ascontiguousarray(recs_np)).to(DEV)
    img = (3, S, S)
    got = ops.pool_exchange(x.view(img), pool.view(img), recs, out=out.view(img))
    assert got.data_ptr() == out.view(img).data_ptr()
    want_out, want_pool = PR.apply_records(x_np, pool_np, recs_np)
    assert np.array_equal(out.values(), want_out), "out"
    assert np.array_equal(pool.values(), want_pool), "pool"
    assert np.array_equal(x.values(), x_np), "x was written"
    assert x.bands_intact() and pool.bands_intact() and out.bands_intact()
    return want_out, want_pool


# ---- 1. the draw -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3, 50])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_device_draw_is_the_reference_table(n, P):
    for filled in sorted({0, max(0, P - 2), P}):
        for seed, rank, iteration, d in ((1234, 0, 6, 0), (1234, 3, 7, 1), (BIG_SEED, 1, BIG_ITER, 1)):
            got = ops.pool_draw(seed, rank, iteration, d, n, P, filled, device=DEV)
            assert got.dtype == torch.int32 and tuple(got.shape) == (n, 4)
            assert np.array_equal(got.cpu().numpy(), PR.records(seed, rank, iteration, d, n, P, filled)), (seed, rank, iteration, d, filled)
    table = torch.full((n + 3, 4), -7, dtype=torch.int32, device=DEV)                     # rows past n stay as they are
    ops.pool_draw(1234, 0, 6, 0, n, P, P, out=table)
    assert np.array_equal(table[:n].cpu().numpy(), PR.records(1234, 0, 6, 0, n, P, P)) and bool((table[n:] == -7).all())


# ---- 2. the exchange on hand-made tables -------------------------------------------------------------------------------------------------
def _pass_table(n):
    return np.array([(j, -1, j, 0) for j in range(n)], dtype=np.int32)


def _tables(n):
    """name -> (P, table): all pass; all insert (slots 1 .. n of n + 2); a chain of up to four touches on the single slot of P = 1 (the
    first reads the old slot and stores the LAST toucher's image, each later one receives its predecessor's); a drawn, mixed table of a
    batch that straddles the fill boundary."""
    chain = _pass_table(n)
    m = min(n, 4)
    chain[0] = (-1, 0, m - 1, 0)
    for j in range(1, m):
        chain[j] = (j - 1, -1, j, 0)
    return {"pass": (3, _pass_table(n)),
            "insert": (n + 2, np.array([(j, 1 + j, j, 0) for j in range(n)], dtype=np.int32)),
            "chain": (1, chain),
            "mixed": (5, PR.records(99, 0, 3, 1, n, 5, 3))}


@pytest.mark.parametrize("S", [2, 3, 16])
@pytest.mark.parametrize("n", [1, 5, 64])
def test_exchange_is_the_reference_application(n, S):
    """S = 2 and 16: images of 12 / 768 floats, the 16-byte path (and, with the base shifted by one float, the 4-byte one); S = 3: 27
    floats, not 16-byte aligned from the second image on."""
    elems = 3 * S * S
    x_np = _patterns((n, elems), 10 * n + S)
    x_np[0, :4] = (0x7FC00001, 0x7F800000, 0x00000001, -0x00400001)       # a NaN payload, inf, a denormal, a negative NaN
    for name, (P, recs) in _tables(n).items():
        pool_np = _patterns((P, elems), 1000 + 10 * n + S)
        for shift in ((0, 1) if S == 2 else (0,)):
            want_out, want_pool = _exchange_and_check(x_np, pool_np, recs, S, shift)
        if name == "pass":
            assert np.array_equal(want_out, x_np) and np.array_equal(want_pool, pool_np)
        if name == "mixed" and n >= 5:
            kinds = [k for k, _ in PR.touches(99, 0, 3, 1, n, 5, 3)]
            assert kinds[:2] == ["insert", "insert"] and "swap" in kinds and ("pass" in kinds or n == 5)
        if name == "chain" and n >= 4:                                       # the slot ends with sample 3, sample 0 got the old slot
            assert np.array_equal(want_pool[0], x_np[3]) and np.array_equal(want_out[0], pool_np[0])
            assert np.array_equal(want_out[1:4], x_np[0:3])


# ---- 3. hostile tables -------------------------------------------------------------------------------------------------------------------
def test_hostile_tables_pass_through_and_store_nothing():
    n, S, P = 6, 3, 4
    x_np, pool_np = _patterns((n, 27), 31), _patterns((P, 27), 32)
    big = 2 ** 31 - 1
    for bad in ((-2, 0, 0, 0), (n, 0, 0, 0), (0, P, 0, 0), (0, -2, 0, 0), (0, 0, -1, 0), (0, 0, n, 0), (-1, -1, 0, 0),
                (big, big, big, big), (-big - 1, -big - 1, -big - 1, 0), (-1, P, 0, 0), (-1, 0, n, 0)):
        recs = np.array([bad] * n, dtype=np.int32)
        want_out, want_pool = _exchange_and_check(x_np, pool_np, recs, S)
        assert np.array_equal(want_out, x_np) and np.array_equal(want_pool, pool_np), bad


# ---- 4. the host ImagePool against the sequential pool -------------------------------------------------------------------------------------
def test_six_batches_equal_the_sequential_pool():
    P, n, S = 5, 4, 16
    pool = ImagePool(P, S, seed=77, rank=2, domain=1, device=DEV)
    seq = PR.SequentialPool(P, (3 * S * S,), np.int32, 77, 2, 1)
    fills = []
    for k in range(6):
        x_np = _patterns((n, 3 * S * S), 50 + k)
        x = torch.from_numpy(x_np).to(DEV).view(torch.float32).view(n, 3, S, S)
        recs = pool.draw(3 * k, n)
        assert np.array_equal(recs.cpu().numpy(), PR.records(77, 2, 3 * k, 1, n, P, seq.filled))
        out = pool.exchange(x)
        want = seq.query(x_np, 3 * k)
        assert np.array_equal(out.view(torch.int32).cpu().numpy().reshape(n, -1), want), k
        assert out.data_ptr() != x.data_ptr() and not out.requires_grad
        fills.append(pool.filled)
        assert pool.filled == seq.filled
    assert fills == [4, 5, 5, 5, 5, 5]
    assert np.array_equal(pool.slots.view(torch.int32).cpu().numpy().reshape(P, -1), seq.slots)
    with pytest.raises(RuntimeError, match="drawn for 4"):
        pool.exchange(torch.zeros((3, 3, S, S), device=DEV))


# ---- 5. past the grid cap ----------------------------------------------------------------------------------------------------------------
def test_past_the_grid_cap():
    """9 x 3 x 512 x 512 floats = 1.77 M 16-byte units > 4096 blocks x 256 threads: the grid-stride trip.  Against the two-step device
    form the fused launch replaces: a gather (index_select) and a scatter (index_copy_) driven by the same records."""
    n, S, P = 9, 512, 4
    assert n * 3 * S * S // 4 > 4096 * 256
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, 3, S, S), generator=g, device=DEV, dtype=torch.int64).to(torch.int32).view(torch.float32)
    pool = torch.randint(-2 ** 31, 2 ** 31 - 1, (P, 3, S, S), generator=g, device=DEV, dtype=torch.int64).to(torch.int32).view(torch.float32)
    recs_np = PR.records(11, 0, 9, 0, n, P, 2)                                   # two inserts, then swaps and passes on a full pool
    kinds = [k for k, _ in PR.touches(11, 0, 9, 0, n, P, 2)]
    assert kinds[:2] == ["insert", "insert"] and "swap" in kinds[2:] and "pass" in kinds[2:]
    recs = torch.from_numpy(recs_np).to(DEV)
    src, slot, st = (recs[:, c].long() for c in range(3))
    xi, pi = x.view(torch.int32), pool.view(torch.int32)
    want_out = torch.cat([xi, pi]).index_select(0, torch.where(src < 0, n + slot, src))
    stores = slot >= 0
    want_pool = pi.clone().index_copy_(0, slot[stores], xi.index_select(0, st[stores]))
    got = ops.pool_exchange(x, pool, recs)
    assert torch.equal(got.view(torch.int32), want_out)
    assert torch.equal(pool.view(torch.int32), want_pool)


def test_ops_wrappers_refuse_what_the_kernels_cannot_take():
    x, pool = torch.zeros((4, 3, 2, 2), device=DEV), torch.zeros((3, 3, 2, 2), device=DEV)
    recs = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    for bad in (recs.float(), recs[:3], recs.cpu(), torch.zeros((4, 3), dtype=torch.int32, device=DEV)):
        with pytest.raises(_lib.DiscoganHipError, match="record table"):
            ops.pool_exchange(x, pool, bad)
    with pytest.raises(_lib.DiscoganHipError, match="one image shape"):
        ops.pool_exchange(x, torch.zeros((3, 3, 2, 3), device=DEV), recs)
    with pytest.raises(_lib.DiscoganHipError, match="fp32"):
        ops.pool_exchange(x.double(), pool.double(), recs)
    with pytest.raises(_lib.DiscoganHipError, match="overlap"):
        ops.pool_exchange(x, pool, recs, out=x)
    with pytest.raises(_lib.DiscoganHipError, match="filled"):
        ops.pool_draw(1, 0, 0, 0, 4, 3, 4, device=DEV)
    with pytest.raises(ValueError, match="slots"):
        ImagePool(0, 16, 1, 0, 0, device=DEV)
    torch.cuda.synchronize()


# ---- 9. keys -----------------------------------------------------------------------------------------------------------------------------
def test_pools_that_differ_in_rank_or_domain_draw_different_tables():
    def table(rank, domain):
        p = ImagePool(8, 16, seed=1234, rank=rank, domain=domain, device=DEV)
        p.filled = 8
        return p.draw(6, 64).cpu().numpy().copy()

    base = table(0, 0)
    assert np.array_equal(base, table(0, 0)) and np.array_equal(base, PR.records(1234, 0, 6, 0, 64, 8, 8))
    assert not np.array_equal(base, table(1, 0)) and not np.array_equal(base, table(0, 1))


# ---- trainer runs shared by the cases below --------------------------------------------------------------------------------------------
S, N, P = 16, 4, 8
_RUNS = {}


def _snapshot(tr):
    tr.finish()
    torch.cuda.synchronize()
    snap = {f"{side}.{name}": getattr(opt, name).cpu().clone() for side, opt in (("gen", tr.optim_gen), ("dis", tr.optim_dis))
            for name in ("flat_p", "exp_avg", "exp_avg_sq")}
    if tr.pool_BA is not None:
        for k, p in (("pool_BA", tr.pool_BA), ("pool_AB", tr.pool_AB)):
            snap[k] = p.slots.cpu().clone()
            snap[k + ".filled"] = torch.tensor(p.filled)
    return snap


def _same(a, b, keys=None):
    keys = sorted(a if keys is None else keys)
    return [k for k in keys if not torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                               b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])]


def _run(key, iters, pool=P, keep=(), first=0, state=None, **kw):
    """Iterations ``first .. iters - 1`` of one trainer on one fixed batch; snapshots (weights, Adam moments, pools) after the iterations
    in ``keep`` and after the last; the fakes and what the discriminators saw at every D-step.  One run per key for the module."""
    if key not in _RUNS:
        A, B = synthetic_batch(N, S, 5, DEV)
        tr = DiscoGANTrainer(default_args(image_pool=pool), device=DEV, image_size=S, seed=1234, **kw)
        if state is not None:
            assert tr.load_train_state(state) == first
        snaps, seen = {}, {}
        for i in range(first, iters):
            out = tr.train_iteration(A, B, i)
            if tr.is_dis_step(i):
                torch.cuda.synchronize()
                seen[i] = {k: getattr(out, k).detach().cpu().clone() for k in ("BA", "AB", "BA_seen", "AB_seen")}
            else:
                assert out.BA_seen is out.BA and out.AB_seen is out.AB
            if i in keep or i == iters - 1:
                snaps[i] = _snapshot(tr)
        _RUNS[key] = dict(snaps=snaps, seen=seen, state=tr.train_state(iters), last=snaps[iters - 1])
        del tr
    return _RUNS[key]


def _check_seen(run):
    """What the discriminators saw at D-steps 0, 3 and 6 is the reference applied to the fakes captured there (domain 0: BA, 1: AB), and
    the pools end as the reference's."""
    for dom, name in enumerate(("BA", "AB")):
        pool_np, filled = np.zeros((P, 3 * S * S), dtype=np.int32), 0
        for i in (0, 3, 6):
            x_np = run["seen"][i][name].view(torch.int32).numpy().reshape(N, -1)
            want, pool_np = PR.apply_records(x_np, pool_np, PR.records(1234, 0, i, dom, N, P, filled))
            filled = min(P, filled + N)
            got = run["seen"][i][name + "_seen"].view(torch.int32).numpy().reshape(N, -1)
            assert np.array_equal(got, want), (name, i)
            assert np.array_equal(got, x_np) == (i < 6), (name, i)                       # fills pass the fakes on; the swap does not
        key = "pool_" + name
        assert np.array_equal(run["last"][key].view(torch.int32).numpy().reshape(P, -1), pool_np) and int(run["last"][key + ".filled"]) == P


# ---- 6. the trainer ----------------------------------------------------------------------------------------------------------------------
def test_trainer_fills_then_swaps():
    """16 px, batch 4, P = 8, seed 1234, exact fp32, eager.  D-steps 0 and 3 only fill the pools, so the run equals the pool-off run
    through iteration 5; at D-step 6 the reference table swaps in both domains and the discriminators part from the pool-off run."""
    t0, t1 = PR.touches(1234, 0, 6, 0, N, P, 8), PR.touches(1234, 0, 6, 1, N, P, 8)
    assert [k for k, _ in t0].count("swap") == 1 and [k for k, _ in t1].count("swap") == 3          # the precondition of this test
    on = _run("eager", 7, keep=(5,))
    off = _run("eager_off", 7, pool=0, keep=(5,))
    assert "image_pool" in on["state"] and "image_pool" not in off["state"]
    assert not any(k.startswith("pool") for k in off["last"])
    weights = [k for k in off["last"]]
    assert _same(on["snaps"][5], off["snaps"][5], weights) == []
    _check_seen(on)
    for i in (0, 3, 6):
        for name in ("BA", "AB"):
            assert torch.equal(off["seen"][i][name + "_seen"], off["seen"][i][name])
    assert "dis.flat_p" in _same(on["last"], off["last"], weights)
    assert _same(on["last"], off["last"], [k for k in weights if k.startswith("gen.")]) == []    # no generator step since


# ---- 7. schedules ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [
    ("grouped", dict(group_launch=True)),
    ("chain", dict(group_launch=False)),
    ("f32x3", dict(mfma_dtype="f32x3")),
    ("bf16", dict(mfma_dtype="bf16", act_dtype="bf16")),
])
def test_graph_replay_equals_eager_dispatch(name, kw):
    """Twelve iterations (four D-steps: two fills, two with swaps; graphs captured at iterations 3 and 4, replayed from 6 on): weights,
    Adam moments and pool contents bitwise."""
    eager = _run(name + "_eager12", 12, **kw)
    graph = _run(name + "_graph12", 12, use_graph=True, **kw)
    assert _same(graph["last"], eager["last"]) == []
    assert int(graph["last"]["pool_BA.filled"]) == P and bool(graph["last"]["pool_BA"].any())
    for i in (0, 3, 6, 9):
        for k in ("BA_seen", "AB_seen"):
            assert torch.equal(graph["seen"][i][k].view(torch.int32), eager["seen"][i][k].view(torch.int32)), (i, k)


def test_one_stream_and_dead_work_schedules_run_with_a_pool():
    """two_streams=False equals the two-chain schedule bitwise.  skip_dead_work=False (the generators keep their autograd graph in a
    D-step): the pooled fakes are detached, the backward pass stops there, and the discriminators see the reference's batches."""
    chain = _run("chain_eager12", 12, group_launch=False)
    one = _run("one_stream12", 12, group_launch=False, two_streams=False)
    assert _same(one["last"], chain["last"]) == []
    dead = _run("dead_work7", 7, group_launch=False, skip_dead_work=False)
    _check_seen(dead)
    assert all(bool(torch.isfinite(v).all()) for k, v in dead["last"].items() if v.dtype == torch.float32)


# ---- 8. resume ---------------------------------------------------------------------------------------------------------------------------
def test_resume_continues_bitwise(tmp_path, capsys):
    whole = _run("eager15", 15)
    head = _run("eager9", 9)
    torch.save(head["state"], tmp_path / "state.pth")
    st = torch.load(tmp_path / "state.pth")
    assert sorted(st["image_pool"]) == ["AB", "BA"] and st["image_pool"]["BA"]["filled"] == P
    tail = _run("resumed15", 15, first=9, state=st)
    assert _same(tail["last"], whole["last"]) == []
    for i in (9, 12):
        for k in ("BA_seen", "AB_seen"):
            assert torch.equal(tail["seen"][i][k].view(torch.int32), whole["seen"][i][k].view(torch.int32)), (i, k)
    capsys.readouterr()
    bare = {k: v for k, v in st.items() if k != "image_pool"}                              # a state written without a pool
    tr = DiscoGANTrainer(default_args(image_pool=P), device=DEV, image_size=S, seed=1234)
    tr.pool_BA.filled = 3
    assert tr.load_train_state(bare) == 9
    said = capsys.readouterr().out
    assert said.count("\n") == 1 and "image pool" in said and "start empty" in said
    assert tr.pool_BA.filled == tr.pool_AB.filled == 0 and not bool(tr.pool_BA.slots.any())
    plain = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=1234)           # a pooled state into a trainer without pool
    assert plain.load_train_state(st) == 9 and plain.pool_BA is None
    with pytest.raises(ValueError, match="image_pool"):
        DiscoGANTrainer(default_args(image_pool=-1), device=DEV, image_size=S, seed=1234)


# ---- 10. CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_with_an_image_pool(tmp_path, capsys):
    argv = ["--task_name", "edges2shoes", "--image_size", str(S), "--batch_size", "4", "--epochs", "3", "--max_iters", "7",
            "--log_interval", "1", "--data_source", "synthetic", "--synthetic_size", "16", "--image_save_interval", "0",
            "--results_dir", str(tmp_path / "res"), "--models_dir", str(tmp_path / "mod"), "--image_pool", "8", "--save_train_state"]
    tr = it_cli.main(argv)
    out = capsys.readouterr().out
    assert "image pool: 8 images per domain" in out
    rp, mp = it_cli.train.last_paths
    assert len([ln for ln in open(rp / "training_log.txt").read().splitlines() if ln.startswith("Iter")]) == 7
    st = torch.load(mp / "train_state_final.pth")
    assert st["image_pool"]["BA"]["filled"] == st["image_pool"]["AB"]["filled"] == 8
    assert tuple(st["image_pool"]["AB"]["slots"].shape) == (8, 3, S, S) and bool(st["image_pool"]["AB"]["slots"].any())
    for net in (tr.generator_A, tr.generator_B, tr.discriminator_A, tr.discriminator_B):
        assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
