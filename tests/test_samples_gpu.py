"""Sample grids on the GPU: the grid kernel (bit-exact against a numpy one-liner), DiscoGANTrainer.sample against the CPU oracle and
its neutrality for everything but the generators' BatchNorm buffers, and the CLI (files, tensor files, resume, two ranks).

Kernel bar: no tolerance anywhere.  ``pixel = rint(clip(x, 0, 1) * float32(255))`` in fp32, NaN -> 0, whole canvas compared, gutters
included.  Trainer bar: the one-forward-pass bounds of tests/test_model_gpu.py (outputs 1e-4 max|ref| + 1e-5, buffers 1e-4 max|ref| +
1e-6), each comparison one generator deep (the oracle's second pass is fed the GPU's first-pass output)."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from PIL import Image

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, ops, samples  # noqa: E402
from discogan_modernized_amd import dataset as ds  # noqa: E402
from discogan_modernized_amd import image_translation as it_cli  # noqa: E402
from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, synthetic_batch  # noqa: E402
from tests.test_samples_cpu import GRID_MAX_BLOCKS, GRID_PAST_CAP, GRID_THREADS, grid_units  # noqa: E402  (the host's grid arithmetic)
from oracle import discogan_ref as O  # noqa: E402  (checker only)
from oracle import image_prep_ref as R  # noqa: E402  (checker only)

DEV = "cuda"


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def ref_pixels(x):
    """The reference of the rounding rule: fp32 throughout, half to even, NaN -> 0."""
    x = np.nan_to_num(np.asarray(x, dtype=np.float32), nan=0.0, posinf=np.inf, neginf=-np.inf)
    y = np.rint(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255))
    assert y.dtype == np.float32
    return y.astype(np.uint8)


def ref_canvas(batches, rows, S, gap, bg, order=None, shift=0, transpose=False):
    """numpy canvas; order / shift / transpose build deliberately WRONG layouts (swapped columns, cells moved by a pixel, cells
    transposed) for the sensitivity check."""
    cols = len(batches)
    order = list(range(cols)) if order is None else order
    H, W, _ = samples.canvas_shape(rows, cols, S, gap)
    canvas = np.full((H + shift, W + shift, 3), bg, dtype=np.uint8)
    for c in range(cols):
        for r in range(rows):
            cell = ref_pixels(batches[order[c]][r]).transpose(1, 2, 0)
            if transpose:
                cell = cell.transpose(1, 0, 2)
            y0, x0 = gap + r * (S + gap) + shift, gap + c * (S + gap) + shift
            canvas[y0:y0 + S, x0:x0 + S] = cell
    return canvas[:H, :W]


def special_values():
    """+-inf, NaN, every k / 255, every tie (k + 0.5) / 255 rounded to fp32 and its two fp32 neighbours."""
    k = np.arange(256, dtype=np.float64)
    exact = (k / 255).astype(np.float32)
    ties = ((k[:255] + 0.5) / 255).astype(np.float32)
    below, above = np.nextafter(ties, np.float32(-1)), np.nextafter(ties, np.float32(2))
    return np.concatenate([np.array([np.inf, -np.inf, np.nan], dtype=np.float32), exact, ties, below, above])


def make_batches(rows, cols, S, seed):
    """cols batches of n_c > rows images drawn from [-0.5, 1.5]; the special values are planted at random DISPLAYED positions (images
    < rows), all of them where the grid shows at least twice as many values (a 1 x 1 grid of 10 px images shows 300: it gets the first
    150 -- the infinities, NaN and the low k / 255 -- and the larger grids of the same test get every one)."""
    rng = np.random.default_rng(seed)
    batches = [rng.uniform(-0.5, 1.5, (rows + 1 + c % 2, 3, S, S)).astype(np.float32) for c in range(cols)]
    sp = special_values()
    shown = cols * rows * 3 * S * S
    n = min(len(sp), shown // 2)
    pos = rng.choice(shown, size=n, replace=False)
    per = rows * 3 * S * S
    for p, v in zip(pos, sp[:n]):
        c, q = divmod(int(p), per)
        batches[c].reshape(-1)[q] = v                      # the first `rows` images of a batch are its first rows*3*S*S values
    return batches, n == len(sp)


@pytest.mark.parametrize("rows,cols", [(1, 1), (2, 3), (5, 6), (3, 8)])
@pytest.mark.parametrize("S", [10, 16, 64, 512])
def test_grid_kernel_is_bit_exact(S, rows, cols):
    """The largest case here, the 5 x 6 grid at 512 px, is 2 025 766 units at gap 3: 3 % UNDER the kernel's 8192 x 256 grid.  No case
    of this test strides; test_grid_kernel_past_the_grid_cap does."""
    batches, all_planted = make_batches(rows, cols, S, seed=1000 * S + 10 * rows + cols)
    assert all_planted or cols * rows * S * S * 3 < 2 * len(special_values())
    dev = [torch.from_numpy(b).to(DEV) for b in batches]
    for gap in (0, 2, 3):
        for bg in (0, 255):
            got = ops.sample_grid(dev, rows, gap=gap, bg=bg)
            assert got.dtype == torch.uint8 and tuple(got.shape) == samples.canvas_shape(rows, cols, S, gap) and got.is_contiguous()
            want = ref_canvas(batches, rows, S, gap, bg)
            got = got.cpu().numpy()
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"S={S} {rows}x{cols} gap={gap} bg={bg}: {len(bad)} bytes differ, first at {bad[0]}"


@pytest.mark.parametrize("rows,cols,S", GRID_PAST_CAP)
def test_grid_kernel_past_the_grid_cap(rows, cols, S):
    """More units than 8192 blocks x 256: the kernel's stride loop, with 16-byte loads (S = 128) and with scalar quads and a short last
    quad (S = 10).  The cell units alone outnumber the grid, so every gutter byte is written on a later trip.  The canvas starts as 7s
    (neither background nor, but by chance, a pixel), whole canvas compared."""
    cap = GRID_MAX_BLOCKS * GRID_THREADS
    batches, all_planted = make_batches(rows, cols, S, seed=1000 * S + 10 * rows + cols)
    assert all_planted
    dev = [torch.from_numpy(b).to(DEV) for b in batches]
    assert all(d.data_ptr() % 16 == 0 for d in dev)
    tab = (ctypes.c_void_p * cols)(*[d.data_ptr() for d in dev])
    for gap in ((3, 0) if S == 128 else (3,)):
        cell, band, strip = grid_units(rows, cols, S, gap)
        assert cell > cap and (band > 0 and strip > 0) == (gap > 0)
        got = torch.full(samples.canvas_shape(rows, cols, S, gap), 7, device=DEV, dtype=torch.uint8)
        _lib.check(_lib.load().dg_sample_grid_u8(tab, cols, rows, S, gap, 255, got.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "dg_sample_grid_u8")
        want = ref_canvas(batches, rows, S, gap, 255)
        got = got.cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"S={S} {rows}x{cols} gap={gap}: {len(bad)} bytes differ, first at {bad[0]}"


def test_grid_comparison_notices_a_misplaced_cell():
    """Every source image differs from every other, so the equality above is sensitive to layout: a reference with two columns
    swapped, with every cell moved by one pixel, or with transposed cells does NOT equal the kernel's canvas."""
    rows, cols, S, gap = 2, 3, 16, 2
    batches, all_planted = make_batches(rows, cols, S, seed=7)
    assert all_planted
    got = ops.sample_grid([torch.from_numpy(b).to(DEV) for b in batches], rows, gap=gap, bg=255).cpu().numpy()
    assert np.array_equal(got, ref_canvas(batches, rows, S, gap, 255))
    assert not np.array_equal(got, ref_canvas(batches, rows, S, gap, 255, order=[1, 0, 2]))
    assert not np.array_equal(got, ref_canvas(batches, rows, S, gap, 255, shift=1))
    assert not np.array_equal(got, ref_canvas(batches, rows, S, gap, 255, transpose=True))
    swapped_rows = [b[::-1].copy() for b in batches]
    assert not np.array_equal(got, ref_canvas(swapped_rows, rows, S, gap, 255))


def test_grid_kernel_takes_batches_at_any_float_alignment():
    """A batch that starts 4 bytes into a 16-byte line (a view into a flat buffer): the 16-byte plane loads do not apply, the result
    is the same; and a non-contiguous batch is laid out through a contiguous copy."""
    rows, S = 3, 16
    batches, _ = make_batches(rows, 2, S, seed=9)
    want = ref_canvas(batches, rows, S, 2, 255)
    dev = []
    for b in batches:
        flat = torch.empty(b.size + 1, device=DEV, dtype=torch.float32)
        view = flat[1:].view(b.shape)
        view.copy_(torch.from_numpy(b))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        dev.append(view)
    assert np.array_equal(ops.sample_grid(dev, rows).cpu().numpy(), want)
    nc = [torch.from_numpy(b).to(DEV).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2) for b in batches]
    assert not nc[0].is_contiguous()
    assert np.array_equal(ops.sample_grid(nc, rows).cpu().numpy(), want)
    with pytest.raises(_lib.DiscoganHipError):
        ops.sample_grid(dev, rows + 3)                              # more rows than the shorter batch holds
    with pytest.raises(_lib.DiscoganHipError):
        ops.sample_grid([dev[0]] * 9, rows)                         # nine columns
    with pytest.raises(_lib.DiscoganHipError):
        ops.sample_grid([dev[0].cpu()], rows)                       # no CPU path


@pytest.mark.parametrize("n,S", [(3, 16), (2, 64), (5, 10), (1, 512)])
def test_export_inverts_the_ingest(n, S):
    u8 = torch.randint(0, 256, (n, S, S, 3), generator=torch.Generator().manual_seed(S), dtype=torch.uint8)
    u8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)       # every value occurs
    back = ops.f32chw_to_u8hwc(ops.u8hwc_to_f32chw(u8.to(DEV)))
    assert back.dtype == torch.uint8 and tuple(back.shape) == (n, S, S, 3)
    assert torch.equal(back.cpu(), u8)


# ---- DiscoGANTrainer.sample ----------------------------------------------------------------------------------------------------
def max_close(got, ref, rtol, atol, what):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, f"{what}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs().max().item()
    bound = rtol * ref.abs().max().item() + atol
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _host_sd(net):
    return {k: v.detach().contiguous().cpu().clone() for k, v in net.state_dict().items()}


def _bn_counters(net):
    return {k: int(v) for k, v in net.state_dict().items() if k.endswith("num_batches_tracked")}


def _test_split(n, S, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, S, S, generator=g), torch.rand(n, 3, S, S, generator=g)


@pytest.mark.parametrize("mode", ["f32", "f32x3", "f32x3_planes"])
@pytest.mark.parametrize("S,n", [(16, 4), (64, 6)])
def test_sample_matches_the_oracle_one_generator_deep(S, n, mode):
    kw = dict(f32=dict(mfma_dtype="f32"), f32x3=dict(mfma_dtype="f32x3", x3_planes=False),
              f32x3_planes=dict(mfma_dtype="f32x3", x3_planes=True))[mode]
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=1234, **kw)
    assert tr.generator_A.training and tr.generator_B.training
    oA, oB = O.Generator(True, image_size=S), O.Generator(True, image_size=S)
    oA.load_state_dict(_host_sd(tr.generator_A))
    oB.load_state_dict(_host_sd(tr.generator_B))
    oA.train()
    oB.train()
    tA, tB = _test_split(n, S)
    AB, BA, ABA, BAB = tr.sample(tA.to(DEV), tB.to(DEV))
    torch.cuda.synchronize()
    for t in (AB, BA, ABA, BAB):
        assert tuple(t.shape) == (n, 3, S, S) and t.dtype == torch.float32 and t.is_cuda and not t.requires_grad
    with torch.no_grad():
        rAB, rBA = oB(tA), oA(tB)
        rABA, rBAB = oA(AB.cpu()), oB(BA.cpu())                 # teacher-forced: the second pass starts from the GPU's first
    for got, ref, what in ((AB, rAB, "AB"), (BA, rBA, "BA"), (ABA, rABA, "ABA"), (BAB, rBAB, "BAB")):
        max_close(got, ref, 1e-4, 1e-5, f"{mode} {S}px {what}")
    for name, net, onet in (("gen_A", tr.generator_A, oA), ("gen_B", tr.generator_B, oB)):
        for (k, bo), (_, bm) in zip(onet.named_buffers(), net.named_buffers()):
            if k.endswith("num_batches_tracked"):
                assert int(bm) == int(bo) == 2, (name, k, int(bm))
            else:
                max_close(bm, bo, 1e-4, 1e-6, f"{mode} {S}px {name} buffer {k}")
    assert not tr.ctx.shadow_tab and not tr.ctx.plane_tab
    assert tr.generator_A.training and tr.generator_B.training


@pytest.mark.parametrize("act_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("S,n", [(16, 4), (64, 6)])
def test_sample_on_the_bf16_path_is_finite_and_counts(S, n, act_dtype):
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=1234, mfma_dtype="bf16", act_dtype=act_dtype)
    tA, tB = _test_split(n, S)
    outs = tr.sample(tA.to(DEV), tB.to(DEV))
    for t in outs:
        assert tuple(t.shape) == (n, 3, S, S) and t.dtype == torch.float32
        assert bool(torch.isfinite(t).all()) and float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    for net in (tr.generator_A, tr.generator_B):
        c = _bn_counters(net)
        assert c and set(c.values()) == {2}
    assert not tr.ctx.shadow_tab and not tr.ctx.plane_tab


def test_sample_refuses_a_single_image():
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=16, seed=1)
    tA, tB = _test_split(2, 16)
    with pytest.raises(ValueError):
        tr.sample(tA[:1].to(DEV), tB.to(DEV))
    with pytest.raises(ValueError):
        tr.sample(tA.to(DEV), tB[:1].to(DEV))
    assert set(_bn_counters(tr.generator_A).values()) == {0}        # refused before any pass ran


NEUTRAL = {
    "f32_16px_grouped_graph": dict(S=16, kw=dict(mfma_dtype="f32", use_graph=True)),
    "f32x3_planes_64px": dict(S=64, kw=dict(mfma_dtype="f32x3", x3_planes=True, use_graph=True)),
    "bf16_maps_bf16_64px": dict(S=64, kw=dict(mfma_dtype="bf16", act_dtype="bf16", use_graph=True)),
}


def _neutral_run(cfg, sample_after):
    S, N, ITERS = cfg["S"], 4, 9
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=1234, **cfg["kw"])
    tA, tB = (t.to(DEV) for t in _test_split(5, S))
    losses, first_seen, statics = [], {}, None
    for it in range(ITERS):
        A, B = synthetic_batch(N, S, 100 + it, DEV)
        losses.append(tr.losses_to_floats(tr.train_iteration(A, B, it)))
        for k, v in tr._graphs.items():
            first_seen.setdefault(k, v[0])
        if it in sample_after:
            keys = set(tr._graphs)
            if tr._static:
                statics = {k: (a.clone(), b.clone()) for k, (a, b) in tr._static.items()}
            gflat = tr.optim_gen.flat_g.clone(), tr.optim_dis.flat_g.clone()
            rg = [p.requires_grad for p in list(tr.optim_gen.params) + list(tr.optim_dis.params)]
            tr.sample(tA, tB)
            assert set(tr._graphs) == keys
            assert torch.equal(tr.optim_gen.flat_g, gflat[0]) and torch.equal(tr.optim_dis.flat_g, gflat[1])
            assert rg == [p.requires_grad for p in list(tr.optim_gen.params) + list(tr.optim_dis.params)]
            if tr._static:
                for k, (a, b) in tr._static.items():
                    assert torch.equal(a, statics[k][0]) and torch.equal(b, statics[k][1])
    tr.finish()
    torch.cuda.synchronize()
    assert all(tr._graphs[k][0] is g for k, g in first_seen.items()), "a captured graph was replaced"
    res = dict(losses=losses, graph_keys=set(tr._graphs), group=tr.group_launch,
               gen_counters=[_bn_counters(tr.generator_A), _bn_counters(tr.generator_B)],
               dis_buffers={f"{n}.{k}": v.detach().cpu().clone() for n, d in (("A", tr.discriminator_A), ("B", tr.discriminator_B))
                            for k, v in d.named_buffers()})
    for name, opt in (("gen", tr.optim_gen), ("dis", tr.optim_dis)):
        for f in ("flat_p", "flat_g", "exp_avg", "exp_avg_sq", "state"):
            res[f"{name}.{f}"] = getattr(opt, f).detach().cpu().clone()
    del tr
    torch.cuda.empty_cache()
    return res


@pytest.mark.parametrize("name", list(NEUTRAL))
def test_sampling_changes_nothing_but_the_generators_bn_buffers(name):
    """Two trainers from one seed, 9 iterations on the same batches (graph replay from iteration 3 on); one samples after iterations
    0, 4 and 7.  Everything the training trajectory consists of is bitwise equal; the generators' BatchNorm counters differ by 6."""
    cfg = NEUTRAL[name]
    a = _neutral_run(cfg, ())
    b = _neutral_run(cfg, (0, 4, 7))
    if name == "f32_16px_grouped_graph":
        assert a["group"] and b["group"]
    assert a["losses"] == b["losses"]
    assert a["graph_keys"] == b["graph_keys"] and len(a["graph_keys"]) >= 2
    for k in a:
        if k.startswith(("gen.", "dis.")):
            assert torch.equal(a[k], b[k]), k
    assert a["dis_buffers"].keys() == b["dis_buffers"].keys() and len(a["dis_buffers"]) > 0
    for k in a["dis_buffers"]:
        assert torch.equal(a["dis_buffers"][k], b["dis_buffers"][k]), k
    for ca, cb in zip(a["gen_counters"], b["gen_counters"]):
        assert ca and ca.keys() == cb.keys()
        assert all(cb[k] - ca[k] == 6 for k in ca), (ca, cb)


@pytest.mark.timeout(900)
def test_sample_of_a_large_split_at_512px():
    """512 px, 130 test images, exact fp32, no oracle (the CPU cannot produce one in useful time): the last transposed conv's input is
    past 2^31 bytes (127 images at this size) and conv1's output past 2 GiB, so the public path reaches the pointer / VALU forms that
    tests/test_shapes_gpu.py tests in isolation."""
    S, n = 512, 130
    tr = DiscoGANTrainer(default_args(), device=DEV, image_size=S, seed=1234, mfma_dtype="f32")
    g = torch.Generator(device=DEV).manual_seed(5)
    tA = torch.rand((n, 3, S, S), device=DEV, generator=g)
    tB = torch.rand((n, 3, S, S), device=DEV, generator=g)
    assert n * 64 * 256 * 256 * 4 > 2 ** 31
    outs = tr.sample(tA, tB)
    torch.cuda.synchronize()
    for t, what in zip(outs, ("AB", "BA", "ABA", "BAB")):
        assert tuple(t.shape) == (n, 3, S, S), what
        lo, hi, fin = float(t.min()), float(t.max()), bool(torch.isfinite(t).all())
        print(f"{what}: min {lo:.6f} max {hi:.6f} finite {fin}")
        assert fin and lo >= 0.0 and hi <= 1.0, what
    for net in (tr.generator_A, tr.generator_B):
        c = _bn_counters(net)
        assert c and set(c.values()) == {2}
    canvas = samples.compose(tA, tB, *outs)
    assert tuple(canvas.shape) == samples.canvas_shape(5, 6, S, 2)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
def _u8_files(tmp, n_train=16, n_test=7, S=16):
    g = torch.Generator().manual_seed(2)
    out = {}
    for name, n in (("A", n_train), ("B", n_train), ("tA", n_test), ("tB", n_test)):
        out[name] = torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8)
        torch.save(out[name], tmp / f"{name}.pt")
    return out


def _run(tmp, tag, extra):
    argv = ["--task_name", "edges2shoes", "--image_size", "16", "--batch_size", "4", "--epochs", "3", "--log_interval", "1",
            "--results_dir", str(tmp / f"res_{tag}"), "--models_dir", str(tmp / f"mod_{tag}")] + extra
    it_cli.main(argv)
    return it_cli.train.last_paths


def _png(path):
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _cell(canvas, r, c, S=16, gap=2):
    return canvas[gap + r * (S + gap):gap + r * (S + gap) + S, gap + c * (S + gap):gap + c * (S + gap) + S]


def _same_checkpoints(mp_a, mp_b, tag="final"):
    for net in ("gen_A", "gen_B", "dis_A", "dis_B"):
        a, b = torch.load(mp_a / f"{net}_{tag}.pth"), torch.load(mp_b / f"{net}_{tag}.pth")
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), f"{net}.{k} differs"


def test_cli_writes_sample_grids_from_tensor_files(tmp_path):
    u8 = _u8_files(tmp_path)
    data = ["--data_A", str(tmp_path / "A.pt"), "--data_B", str(tmp_path / "B.pt")]
    test = ["--test_A", str(tmp_path / "tA.pt"), "--test_B", str(tmp_path / "tB.pt")]
    rp, mp_on = _run(tmp_path, "on", data + test + ["--image_save_interval", "4"])
    assert sorted(os.listdir(rp / "samples")) == ["samples_iter_0.png", "samples_iter_4.png", "samples_iter_8.png"]
    grids = [_png(rp / "samples" / f"samples_iter_{i}.png") for i in (0, 4, 8)]
    for gr in grids:
        assert gr.shape == samples.canvas_shape(5, 6, 16, 2) and gr.dtype == np.uint8
        for r in range(5):                                      # the round-trip property: u8 -> / 255 -> grid kernel -> PNG
            assert np.array_equal(_cell(gr, r, 0), u8["tA"][r].numpy()) and np.array_equal(_cell(gr, r, 1), u8["tB"][r].numpy())
        assert np.all(gr[:2] == 255) and np.all(gr[:, :2] == 255) and np.all(gr[-2:] == 255) and np.all(gr[:, -2:] == 255)
    assert not np.array_equal(grids[0][:, 38:], grids[2][:, 38:])          # the translated columns move as the generators train
    # without a test split this source does not sample, and is bit for bit the run with sampling switched off
    rp_none, mp_none = _run(tmp_path, "none", data + ["--image_save_interval", "4"])
    rp_off, mp_off = _run(tmp_path, "off", data + test + ["--image_save_interval", "0"])
    assert not (rp_none / "samples").exists() and not (rp_off / "samples").exists()
    _same_checkpoints(mp_none, mp_off)
    # sampling moves the generators' running statistics and nothing else
    on, off = torch.load(mp_on / "gen_A_final.pth"), torch.load(mp_off / "gen_A_final.pth")
    for k in on:
        if "running_" in k or k.endswith("num_batches_tracked"):
            assert not torch.equal(on[k], off[k]), k
        else:
            assert torch.equal(on[k], off[k]), k
    for net in ("dis_A", "dis_B"):
        a, b = torch.load(mp_on / f"{net}_final.pth"), torch.load(mp_off / f"{net}_final.pth")
        assert all(torch.equal(a[k], b[k]) for k in a)


def test_cli_exact_resume_with_sampling_on(tmp_path):
    _u8_files(tmp_path)
    extra = ["--synthetic_size", "16", "--test_A", str(tmp_path / "tA.pt"), "--test_B", str(tmp_path / "tB.pt"),
             "--image_save_interval", "4", "--model_save_interval", "5", "--save_train_state"]
    rp, mp_full = _run(tmp_path, "full", extra)
    assert sorted(os.listdir(rp / "samples")) == ["samples_iter_0.png", "samples_iter_4.png", "samples_iter_8.png"]
    st = torch.load(mp_full / "train_state_5.pth")
    assert st["iters"] == 6
    assert int(st["nets"]["gen_A"]["encoder.3.num_batches_tracked"]) == 2 * 6 + 2 * 2     # 6 iterations + the events at 0 and 4
    rp2, mp_res = _run(tmp_path, "resumed", extra + ["--resume", str(mp_full / "train_state_5.pth")])
    assert sorted(os.listdir(rp2 / "samples")) == ["samples_iter_8.png"]
    assert open(rp / "samples" / "samples_iter_8.png", "rb").read() == open(rp2 / "samples" / "samples_iter_8.png", "rb").read()
    _same_checkpoints(mp_full, mp_res, "final")
    _same_checkpoints(mp_full, mp_res, "10")


def _tree(root, n_train, n_test, seed=3):
    rng = np.random.default_rng(seed)
    for split, k in (("train", n_train), ("test", n_test)):
        d = root / "edges2shoes" / split
        d.mkdir(parents=True)
        for i in range(k):
            Image.fromarray(rng.integers(0, 256, (256, 512, 3), dtype=np.uint8)).save(d / f"{i:03d}_AB.png")
            (d / f"{i:03d}_AB.png").rename(d / f"{i:03d}_AB.jpg")       # PNG bytes under the reference's *.jpg glob: lossless decode
    return sorted(str(p) for p in (root / "edges2shoes" / "test").glob("*.jpg"))


def test_cli_samples_the_test_split_of_the_files_source(tmp_path, capsys):
    S = 16
    test_files = _tree(tmp_path / "three", 9, 3)
    rp, _ = _run(tmp_path, "files", ["--data_root", str(tmp_path / "three"), "--epochs", "2", "--no_graph"])
    assert "data source: files (9 images per domain)" in capsys.readouterr().out
    assert os.listdir(rp / "samples") == ["samples_iter_0.png"]           # default interval 1000, 4 iterations
    grid = _png(rp / "samples" / "samples_iter_0.png")
    assert grid.shape == samples.canvas_shape(3, 6, S, 2)
    imgs = [ds.decode_rgb(f) for f in test_files]
    wantB = np.rint(255.0 * R.read_images(imgs, "B", S).astype(np.float64)).astype(np.uint8)
    vA = 255.0 * R.read_images(imgs, "A", S).astype(np.float64)
    wantA = np.rint(vA)
    n_off = 0
    for r in range(3):
        assert np.array_equal(_cell(grid, r, 1), wantB[r].transpose(1, 2, 0)), f"column B row {r}"
        diff = _cell(grid, r, 0).astype(np.float64) - wantA[r].transpose(1, 2, 0)
        v = vA[r].transpose(1, 2, 0)
        near_tie = np.abs(v - np.floor(v) - 0.5) <= 255 * 2e-6
        assert np.all(np.abs(diff) <= 1) and np.all(near_tie[diff != 0]), f"column A row {r}"
        n_off += int((diff != 0).sum())
    print(f"column A: {n_off} pixels one count off (all within 255 * 2e-6 of a tie)")
    # a test split of one image: one printed line, no samples, training completes
    _tree(tmp_path / "one", 9, 1)
    rp1, mp1 = _run(tmp_path, "one", ["--data_root", str(tmp_path / "one"), "--epochs", "2", "--no_graph"])
    out = capsys.readouterr().out
    assert out.count("sampling off") == 1 and "Training completed" in out
    assert not (rp1 / "samples").exists() and (mp1 / "gen_A_final.pth").exists()
    lines = [ln for ln in open(rp1 / "training_log.txt").read().splitlines() if ln.startswith("Iter")]
    assert len(lines) == 4


def _dp_worker(rank, world, initfile, outdir, interval):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    try:
        from discogan_modernized_amd import distributed_image_translation as dit
        from discogan_modernized_amd import image_translation as it
        from discogan_modernized_amd.trainer import DiscoGANTrainer
        torch.cuda.set_device(0)
        args = dit.parse_args(["--task_name", "edges2shoes", "--image_size", "16", "--batch_size", "4", "--epochs", "2", "--log_interval", "2",
                               "--data_A", os.path.join(outdir, "A.pt"), "--data_B", os.path.join(outdir, "B.pt"),
                               "--test_A", os.path.join(outdir, "tA.pt"), "--test_B", os.path.join(outdir, "tB.pt"),
                               "--image_save_interval", str(interval),
                               "--results_dir", os.path.join(outdir, f"res_i{interval}_rank{rank}"),
                               "--models_dir", os.path.join(outdir, f"mod_i{interval}_rank{rank}")])
        tr = DiscoGANTrainer(args, device="cuda:0", image_size=16, seed=args.seed, process_group=dist.group.WORLD, use_graph=True)
        it.train(args, trainer=tr, rank=rank, world_size=world, is_main=(rank == 0), process_group=dist.group.WORLD)
        tr.finish()
        torch.cuda.synchronize()
        torch.save(dict(gen=tr.optim_gen.flat_p.cpu(), dis=tr.optim_dis.flat_p.cpu(),
                        nbt=int(tr.generator_A.encoder[3].num_batches_tracked)), os.path.join(outdir, f"i{interval}_rank{rank}.pt"))
        dist.barrier()
        tr.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_only_rank0_samples_and_replicas_stay_identical():
    """Data-parallel rehearsal (two ranks on the one GPU, gloo): rank 0 alone loads the split, samples and writes; the weights of both
    ranks stay bitwise equal to each other and to a run with sampling off."""
    W = 2
    with tempfile.TemporaryDirectory() as d:
        from pathlib import Path
        _u8_files(Path(d), n_train=32)
        runs = {}
        for interval in (3, 0):
            mp.spawn(_dp_worker, args=(W, os.path.join(d, f"init{interval}"), d, interval), nprocs=W, join=True)
            runs[interval] = [torch.load(os.path.join(d, f"i{interval}_rank{k}.pt")) for k in range(W)]
        found = {}
        for root, dirs, files in os.walk(d):
            if os.path.basename(root) == "samples":
                found[root] = sorted(files)
        assert len(found) == 1, found
        (root, files), = found.items()
        assert "res_i3_rank0" in root and files == ["samples_iter_0.png", "samples_iter_3.png", "samples_iter_6.png"], found
        assert _png(os.path.join(root, files[0])).shape == samples.canvas_shape(5, 6, 16, 2)
    on, off = runs[3], runs[0]
    for k in ("gen", "dis"):
        assert torch.equal(on[0][k], on[1][k]) and torch.equal(on[0][k], off[0][k]) and torch.equal(off[0][k], off[1][k]), k
    n_iters = off[0]["nbt"] // 2
    assert n_iters == 8 and off[1]["nbt"] == 16                      # 2 epochs x 4 batches of the 16-image shard, two passes each
    assert on[0]["nbt"] == 16 + 2 * 3 and on[1]["nbt"] == 16         # rank 0's generator buffers are the ones that move
