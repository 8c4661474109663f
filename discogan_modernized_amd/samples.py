"""Sample image grids during training (reference image_translation.py:170-209, 238-253, 411-417; data-parallel form
distributed_image_translation.py:228-245, 369, 521, 542-549).

Every ``--image_save_interval`` iterations the four generator passes run on the held-out split (``DiscoGANTrainer.sample``) and
``results/.../samples/samples_iter_{i}.png`` is written: ``min(5, n)`` rows by the six columns ``A, B, A->B, B->A, A->B->A, B->A->B``
with a 2-pixel white gutter.  The grid is laid out on the device by one kernel (``ops.sample_grid`` / ``dg_sample_grid_u8``), crosses
PCIe once as the uint8 canvas and is encoded with PIL.  It is a pixel grid, not the reference's matplotlib figure (no titles, no
resampling): ``pixel = rint(clamp(x, 0, 1) * 255)``.

As in the reference the passes run under ``no_grad`` with the generators in training mode, so every sampling event moves the
generators' BatchNorm running statistics (two forward calls each); ``--image_save_interval 0`` turns sampling off.

Where the split comes from:
  files                        the test lists of ``dataset.get_data`` through ``dataset.read_images`` (whole split; data parallel: the
                               first 10 of each list), resident on the device for the run
  tensors, shards, synthetic   ``--test_A`` / ``--test_B``: tensor files in the formats of ``--data_A`` / ``--data_B``, truncated to
                               ``--n_test``; without them these sources do not sample
Data parallel: rank 0 alone loads the split and samples (it is the rank that saves).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

TITLES = ("A", "B", "A->B", "B->A", "A->B->A", "B->A->B")       # column order, image_translation.py:186-192
N_ROWS = 5                                                        # n_samples, image_translation.py:170
GAP, BG = 2, 255
DP_N_TEST = 10                                                    # distributed_image_translation.py:369


def canvas_shape(rows, cols, S, gap=GAP):
    """Shape [Hc, Wc, 3] of the canvas ``dg_sample_grid_u8`` writes."""
    return rows * (S + gap) + gap, cols * (S + gap) + gap, 3


def _load_tensor_split(path, n_test, image_size, device):
    from . import ops
    t = torch.load(path, map_location="cpu")[:max(int(n_test), 0)]
    S = image_size
    if t.dtype == torch.uint8:
        if t.dim() != 4 or tuple(t.shape[1:]) != (S, S, 3):
            raise ValueError(f"{path}: a uint8 test tensor must be [n,{S},{S},3], got {tuple(t.shape)}")
        return ops.u8hwc_to_f32chw(t.to(device)) if len(t) else torch.empty((0, 3, S, S), device=device)
    if t.dim() != 4 or tuple(t.shape[1:]) != (3, S, S):
        raise ValueError(f"{path}: a float test tensor must be [n,3,{S},{S}], got {tuple(t.shape)}")
    return t.float().contiguous().to(device)


def load_split(args, data_kind, device, world_size=1):
    """(test_A, test_B) float [n,3,S,S] on the device, or None when this run neither samples (--image_save_interval) nor evaluates
    (--eval_interval, evaluate.py) (one printed line per event kind says why when a split was asked for and is too small).  Call it on
    the rank that saves only."""
    from . import dataset as ds
    sampling = int(getattr(args, "image_save_interval", 0) or 0) > 0
    evaluating = int(getattr(args, "eval_interval", 0) or 0) > 0
    if not (sampling or evaluating):
        return None
    test_A, test_B = getattr(args, "test_A", None), getattr(args, "test_B", None)
    if data_kind == "files":
        _, _, files_A, files_B = ds.get_data(args)
        if world_size > 1:
            files_A, files_B = files_A[:DP_N_TEST], files_B[:DP_N_TEST]
        dom_A, dom_B = ds.task_domains(args.task_name)
        split = []
        for files, dom in ((files_A, dom_A), (files_B, dom_B)):
            try:
                split.append(ds.read_images(list(files), dom, args.image_size, device=device))
            except ValueError:                   # no readable image at all
                split.append(torch.empty((0, 3, args.image_size, args.image_size), device=device))
    elif test_A and test_B:
        n_test = getattr(args, "n_test", 200)
        split = [_load_tensor_split(p, n_test, args.image_size, device) for p in (test_A, test_B)]
    else:
        return None
    if min(len(split[0]), len(split[1])) < 2:
        for on, what in ((sampling, "sampling"), (evaluating, "evaluation")):
            if on:
                print(f"{what} off: the test split holds {len(split[0])} / {len(split[1])} usable images (two per side are needed)", flush=True)
        return None
    return split[0], split[1]


def compose(test_A, test_B, AB, BA, ABA, BAB, rows=None):
    """The six columns of a sampling event as one uint8 canvas on the device (one kernel launch)."""
    from . import ops
    cols = (test_A, test_B, AB, BA, ABA, BAB)
    if rows is None:
        rows = min(N_ROWS, *(len(c) for c in cols))
    return ops.sample_grid(cols, rows, gap=GAP, bg=BG)


def write_png(canvas, path):
    """uint8 [H,W,3] (numpy array or host tensor) -> ``path`` as an RGB PNG (lossless: decodes to the same bytes)."""
    from PIL import Image
    arr = np.ascontiguousarray(canvas.numpy() if isinstance(canvas, torch.Tensor) else canvas)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"write_png needs a uint8 [H,W,3] canvas, got {arr.dtype} {arr.shape}")
    Image.fromarray(arr).save(path, format="PNG")
    return path


def save_samples(trainer, split, save_dir, iteration, outs=None):
    """One sampling event: four passes (unless the caller already ran them for this iteration: ``outs``), grid kernel, one D2H copy,
    PNG.  Returns the path written."""
    test_A, test_B = split
    AB, BA, ABA, BAB = trainer.sample(test_A, test_B) if outs is None else outs
    canvas = compose(test_A, test_B, AB, BA, ABA, BAB).cpu()
    save_dir = Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    return write_png(canvas, save_dir / f"samples_iter_{iteration}.png")
