"""Training augmentation on the GPU: the device draw against its numpy restatement (exact), the fused kernels against the numpy oracle and
against the two-step device form "prepare at L, slice, mirror" (bitwise), the float path, the loader and the CLI.

Bars: everything on the uint8 path (domain None / 'B') and every comparison of two DEVICE results is bitwise.  Against numpy, domain 'A' and
the float batch carry test_ingest_gpu.py's float-path bound of 2e-6 (fp32 sums against the oracle's fp64 ones, values in [0, 1]: about 16 ulp
of 1.0, while a wrong tap, window or mirror is off by O(1e-2) on random pixels)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from discogan_modernized_amd import _lib, ops  # noqa: E402
from discogan_modernized_amd import dataset as ds  # noqa: E402
from discogan_modernized_amd import image_translation as it_cli  # noqa: E402
from oracle import image_prep_ref as R  # noqa: E402  (checker only)
from tests import augment_ref as AR  # noqa: E402

DEV = "cuda"
S = 16
FLOAT_BOUND = 2e-6


def _batch(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _two_step(src, domain, L, recs, size=S):
    """The form the fused kernel replaces, on the device: dg_image_prep at L, then the window and the mirror with torch ops."""
    full = ds.prepare_batch(src, domain, L)
    out = []
    for i, (ox, oy, flip, _) in enumerate(recs.tolist()):
        w = full[i, :, oy:oy + size, ox:ox + size]
        out.append(torch.flip(w, dims=[2]) if flip else w)
    return torch.stack(out).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the draw --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 257])
def test_device_draw_is_the_numpy_draw(n):
    for seed, rank, iteration, d, L, flags in ((1234, 0, 0, 0, 24, 3), (1234, 3, 7, 1, 18, 3), ((1 << 63) + 5, 1, (1 << 33) + 1, 1, 24, 3),
                                               (7, 0, 2, 0, 24, AR.FLIP), (7, 0, 2, 0, 24, AR.CROP), (7, 0, 2, 0, 16, 0)):
        got = ops.augment_draw(seed, rank, iteration, d, n, S, L, flags, device=DEV)
        assert got.dtype == torch.int32 and tuple(got.shape) == (n, 4)
        assert np.array_equal(got.cpu().numpy(), AR.draw(seed, rank, iteration, d, n, S, L, flags)), (seed, rank, iteration, d, L, flags)
    table = torch.full((n + 3, 4), -7, dtype=torch.int32, device=DEV)                  # a slot's table: rows past n stay as they are
    ops.augment_draw(1234, 0, 0, 0, n, S, 24, 3, out=table)
    assert np.array_equal(table[:n].cpu().numpy(), AR.draw(1234, 0, 0, 0, n, S, 24, 3)) and bool((table[n:] == -7).all())


# ---- uint8 path ------------------------------------------------------------------------------------------------------------------
U8_SOURCES = {"whole": ((5, 20, 24), None, 21), "B": ((5, 12, 264), "B", 22)}              # 'B': an 8-column crop of 264-pixel rows


@pytest.mark.parametrize("L", [16, 18, 24])
@pytest.mark.parametrize("name", sorted(U8_SOURCES))
def test_uint8_path_is_bitwise(name, L):
    shape, domain, seed = U8_SOURCES[name]
    src = _batch(*shape, seed)
    recs = AR.corner_records(S, L)
    dsrc = _dev(src)
    got = ds.prepare_batch(dsrc, domain, S, aug=(L, _dev(recs), None))
    want = np.stack([AR.augment_image(src[i], domain, S, L, *recs[i, :3]) for i in range(len(src))])
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, 3, S, S)
    assert np.array_equal(got.cpu().numpy(), want), f"max diff {np.abs(got.cpu().numpy() - want).max():.3e}"
    assert torch.equal(_bits(got), _bits(_two_step(dsrc, domain, L, recs)))
    if L == S:
        zero = torch.zeros((5, 4), dtype=torch.int32, device=DEV)
        assert torch.equal(_bits(ds.prepare_batch(dsrc, domain, S, aug=(S, zero, None))), _bits(ds.prepare_batch(dsrc, domain, S)))


def test_records_outside_the_range_are_clamped_into_it():
    """A stale table cannot move the window off the size-L image (nor a read off the source): offsets clamp to [0, L - S]."""
    src = _batch(3, 20, 24, 23)
    wild = np.array([(-5, 1000, 1, 0), (1 << 30, -(1 << 30), 0, 0), (9, -1, 7, 0)], dtype=np.int32)
    tame = np.array([(0, 8, 1, 0), (8, 0, 0, 0), (8, 0, 1, 0)], dtype=np.int32)
    a = ds.prepare_batch(_dev(src), None, S, aug=(24, _dev(wild), None))
    b = ds.prepare_batch(_dev(src), None, S, aug=(24, _dev(tame), None))
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("L", [18, 24])
def test_domain_A_erosion_and_float_resize(L):
    src = _batch(3, 12, 264, 24)
    src[1, 4:7, 50:53] = 0                                                        # a black dot for the erosion to grow
    recs = AR.corner_records(S, L)[[1, 3, 4]]                                     # far corner mirrored, top right, middle mirrored
    got = ds.prepare_batch(_dev(src), "A", S, aug=(L, _dev(recs), None))
    assert torch.equal(_bits(got), _bits(_two_step(_dev(src), "A", L, recs)))
    want = np.stack([AR.augment_image(src[i], "A", S, L, *recs[i, :3]) for i in range(3)])
    diff = np.abs(got.cpu().numpy() - want).max()
    assert diff <= FLOAT_BOUND, f"max diff {diff:.3e}"


def test_rec_index_sub_launches_equal_the_one_launch():
    src, L = _batch(5, 20, 24, 25), 24
    recs = _dev(AR.corner_records(S, L))
    one = ds.prepare_batch(_dev(src), None, S, aug=(L, recs, None))
    out = torch.empty_like(one)
    for pos in ([0, 2, 4], [1, 3]):
        idx = torch.tensor(pos, dtype=torch.int32, device=DEV)
        out[torch.tensor(pos, device=DEV)] = ds.prepare_batch(_dev(src[pos]), None, S, aug=(L, recs, idx))
    assert torch.equal(_bits(out), _bits(one))


def test_past_the_grid_cap():
    """9 x 512 x 512 output pixels > 8192 blocks x 256 threads: the grid-stride trip and its 64-bit index."""
    size, L, n = 512, 576, 9
    assert n * size * size > 8192 * 256
    src = _dev(_batch(n, 64, 64, 26))
    recs = AR.draw(5, 0, 1, 0, n, size, L, 3)
    recs[0, :3], recs[n - 1, :3] = (0, 0, 0), (L - size, L - size, 1)
    got = ds.prepare_batch(src, None, size, aug=(L, _dev(recs), None))
    assert torch.equal(_bits(got), _bits(_two_step(src, None, L, recs, size)))


# ---- float path ------------------------------------------------------------------------------------------------------------------
def test_float_path():
    x_np = np.random.default_rng(27).random((5, 3, S, S), dtype=np.float32)
    x = _dev(x_np)
    zero = torch.zeros((5, 4), dtype=torch.int32, device=DEV)
    assert torch.equal(_bits(ops.augment_f32(x, S, zero)), _bits(x))                    # L = S, zero records: the input, bitwise
    odd = x.clone()
    odd[0, 0, 0, 0], odd[1, 1, 3, 4], odd[2, 2, 15, 15] = -0.0, float("inf"), float("nan")
    assert torch.equal(_bits(ops.augment_f32(odd, S, zero)), _bits(odd))                # ... whatever the values are
    L = 24
    recs = AR.corner_records(S, L)
    got = ops.augment_f32(x, L, _dev(recs))
    want = np.stack([AR.window(R.resize_linear_float(x_np[i].transpose(1, 2, 0), L).transpose(2, 0, 1), S, *recs[i, :2], recs[i, 2])
                     for i in range(5)])
    diff = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    assert diff <= FLOAT_BOUND, f"max diff {diff:.3e}"
    # the mirror alone: the same windows unflipped, then torch.flip -- at L = S (the full window) and at L = 24
    flipped = zero.clone()
    flipped[:, 2] = 1
    assert torch.equal(_bits(ops.augment_f32(x, S, flipped)), _bits(torch.flip(x, dims=[3])))
    unflipped = recs.copy()
    unflipped[:, 2] = 0
    mirrored = unflipped.copy()
    mirrored[:, 2] = 1
    assert torch.equal(_bits(ops.augment_f32(x, L, _dev(mirrored))), _bits(torch.flip(ops.augment_f32(x, L, _dev(unflipped)), dims=[3])))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_a_message():
    lib = _lib.load()
    src = _dev(_batch(2, 20, 24, 28))
    recs = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    out = torch.empty((2, 3, S, S), device=DEV)
    with pytest.raises(_lib.DiscoganHipError, match="smaller than"):
        ds.prepare_batch(src, None, S, aug=(S - 1, recs, None))
    with pytest.raises(_lib.DiscoganHipError, match="smaller than"):
        ops.augment_f32(out, S - 4, recs)
    with pytest.raises(_lib.DiscoganHipError, match="smaller than"):
        ops.augment_draw(1, 0, 0, 0, 2, S, S - 1, 3, device=DEV)
    p = C.c_void_p
    assert lib.dg_image_prep_aug(p(src.data_ptr()), p(out.data_ptr()), 2, 20, 24, 0, 24, 0, 1, S, 24, None, None, None) == -1
    assert b"null record table" in lib.dg_last_error()
    assert lib.dg_augment_f32(p(out.data_ptr()), p(out.data_ptr()), 2, S, 24, None, None) == -1 and b"null record table" in lib.dg_last_error()
    assert lib.dg_augment_draw(1, 0, 0, 0, 2, S, 24, 3, None, None) == -1 and b"null record table" in lib.dg_last_error()
    assert lib.dg_image_prep_aug(p(src.data_ptr()), p(out.data_ptr()), 2, 20, 24, 20, 8, 0, 1, S, 24, p(recs.data_ptr()), None, None) == -1
    assert b"crop [20, 28) outside the 24-pixel rows" in lib.dg_last_error()
    for bad in (recs.float(), recs[:1], recs.cpu(), torch.zeros((2, 3), dtype=torch.int32, device=DEV)):
        with pytest.raises(_lib.DiscoganHipError, match="record table"):
            ds.prepare_batch(src, None, S, aug=(24, bad, None))
    with pytest.raises(_lib.DiscoganHipError, match="rec_index"):
        ds.prepare_batch(src, None, S, aug=(24, recs, torch.zeros(1, dtype=torch.int32, device=DEV)))
    torch.cuda.synchronize()                                                      # nothing above reached the device


# ---- loader, resident data, CLI ----------------------------------------------------------------------------------------------------
class _MemSource:
    """Decoded images of several sizes held in memory; ``load(i)`` like FileSource / ShardSource."""

    def __init__(self, sizes, seed):
        self.imgs = [_batch(1, h, w, seed + i)[0] for i, (h, w) in enumerate(sizes)]

    def __len__(self):
        return len(self.imgs)

    def load(self, i):
        return self.imgs[i]


SIZES = [(20, 24), (20, 24), (20, 24), (33, 47), (20, 24), (40, 30), (33, 47), (20, 24)]
# batch 0: one size (one launch, no rec_index); batches 1, 2: mixed sizes (one launch per size, records by batch position); ragged tail
LOADER_BATCHES = [(np.array([0, 1, 2]), np.array([4, 7, 0])), (np.array([3, 4, 5]), np.array([5, 1, 6])), (np.array([6, 7]), np.array([3, 2]))]


def test_loader_draws_by_iteration_and_batch_position():
    src = (_MemSource(SIZES, 40), _MemSource(SIZES, 60))
    aug = ds.Augment(seed=99, rank=1, flags=3, scale=1.5, first_iteration=10)
    L = aug.size(S)
    assert L == 24
    loader = ds.DeviceLoader(src[0], src[1], (None, None), S, LOADER_BATCHES, device=DEV, workers=2, augment=aug)
    seen = 0
    for k, (idx, got) in enumerate(zip(LOADER_BATCHES, loader)):
        for d in range(2):
            recs = AR.draw(99, 1, 10 + k, d, len(idx[d]), S, L, 3)
            want = np.stack([AR.augment_image(src[d].imgs[i], None, S, L, *recs[j, :3]) for j, i in enumerate(idx[d])])
            assert np.array_equal(got[d].cpu().numpy(), want), (k, d)
        seen += 1
    loader.close()
    assert seen == len(LOADER_BATCHES)


def test_loader_without_augmentation_is_todays_loader():
    src = (_MemSource(SIZES, 40), _MemSource(SIZES, 60))
    for aug in (None, ds.Augment(seed=99, rank=1, flags=0, scale=1.5, first_iteration=10)):
        loader = ds.DeviceLoader(src[0], src[1], (None, None), S, LOADER_BATCHES, device=DEV, workers=2, augment=aug)
        assert loader.augment is None and "recs" not in loader.slots[0]
        for idx, got in zip(LOADER_BATCHES, loader):
            for d in range(2):
                assert np.array_equal(got[d].cpu().numpy(), R.read_images([src[d].imgs[i] for i in idx[d]], None, S)), d
        loader.close()


@pytest.mark.parametrize("kind", ["uint8", "float"])
def test_resident_epoch_resumes_mid_epoch(kind):
    rng = np.random.default_rng(29)
    if kind == "uint8":
        A, B = _dev(_batch(12, S, S, 30)), _dev(_batch(12, S, S, 31))
    else:
        A, B = _dev(rng.random((12, 3, S, S), dtype=np.float32)), _dev(rng.random((12, 3, S, S), dtype=np.float32))
    aug = ds.Augment(seed=3, rank=0, flags=3, scale=1.25, first_iteration=0)
    L = aug.size(S)
    data = it_cli._ResidentData(A, B, augment=aug, image_size=S)
    batches = [(_dev(rng.permutation(12)[:4]), _dev(rng.permutation(12)[:4])) for _ in range(5)]
    whole = list(data.epoch(batches, 0))
    tail = list(data.epoch(batches, start=3))
    assert len(whole) == 5 and len(tail) == 2
    for (a, b), (ta, tb) in zip(whole[3:], tail):
        assert torch.equal(_bits(a), _bits(ta)) and torch.equal(_bits(b), _bits(tb))
    later = list(data.epoch(batches, start=3, first_iteration=103))               # the same batches at other iterations: other draws
    assert not torch.equal(later[0][0], tail[0][0])
    if kind == "uint8":                                                           # and the batches are the reference's
        for t, ((ia, ib), (a, b)) in enumerate(zip(batches, whole)):
            for d, (src, idx, got) in enumerate(((A, ia, a), (B, ib, b))):
                recs = AR.draw(3, 0, t, d, 4, S, L, 3)
                want = np.stack([AR.augment_image(src[i].cpu().numpy(), None, S, L, *recs[j, :3]) for j, i in enumerate(idx.tolist())])
                assert np.array_equal(got.cpu().numpy(), want), (t, d)
    plain = list(it_cli._ResidentData(A, B).epoch(batches, 3))                    # augmentation off: today's batches
    assert torch.equal(plain[0][0], it_cli.take_batch(A, batches[3][0]))


def test_cli_trains_with_augmentation(tmp_path, capsys):
    argv = ["--task_name", "edges2shoes", "--image_size", str(S), "--batch_size", "4", "--epochs", "3", "--max_iters", "4",
            "--log_interval", "1", "--data_source", "synthetic", "--synthetic_size", "16", "--image_save_interval", "0",
            "--results_dir", str(tmp_path / "res"), "--models_dir", str(tmp_path / "mod"), "--augment", "flip,crop"]
    tr = it_cli.main(argv)
    out = capsys.readouterr().out
    assert "augmentation: flip,crop on the training data (prepared at L = 18" in out
    rp, _ = it_cli.train.last_paths
    assert len([ln for ln in open(rp / "training_log.txt").read().splitlines() if ln.startswith("Iter")]) == 4
    for net in (tr.generator_A, tr.generator_B, tr.discriminator_A, tr.discriminator_B):
        assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    with pytest.raises(ValueError, match="augment"):
        it_cli.main(argv[:-1] + ["flip,shear"])
