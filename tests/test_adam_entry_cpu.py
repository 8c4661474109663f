"""What the one flat Adam entry of the C ABI refuses before it launches anything, and what it takes without a launch (no GPU needed:
dummy non-null 16-byte-aligned pointers, validation ends the call first -- the pattern of tests/test_group_tables_cpu.py)."""
import ctypes

import pytest

from discogan_modernized_amd import _lib

P = ctypes.c_void_p
N = 4096


def _flat(n=N, form=0, out=16, plane_elems=N, ctl=None, null=None):
    """dg_adam_step_flat on dummy pointers; null: the name of one buffer passed as NULL."""
    buf = {k: (None if k == null else P(16)) for k in ("p", "g", "m", "v", "state")}
    L = _lib.load()
    rc = L.dg_adam_step_flat(buf["p"], buf["g"], buf["m"], buf["v"], n, buf["state"], 0.5, 0.999, 1e-8, 0.0, 1.0,
                             None if ctl is None else P(ctl), None if out is None else P(out), form, plane_elems, None)
    return rc, L.dg_last_error()


FLAT_REFUSALS = [
    ("form 2", dict(form=2), b"form 2 (0 plain, 1 bf16 shadow, 3 planes)"),
    ("form 1 without an output", dict(form=1, out=None), b"form 1 without an output"),
    ("form 3 without an output", dict(form=3, out=None), b"form 3 without an output"),
    ("plane distance below n", dict(form=3, plane_elems=N - 8), b"plane distance 4088 for 4096 parameters"),
    ("plane distance no multiple of 8", dict(form=3, plane_elems=N + 4), b"plane distance 4100 for 4096 parameters"),
] + [(f"null {k}", dict(null=k), b"null pointer") for k in ("p", "g", "m", "v", "state")]


@pytest.mark.parametrize("ctl", [None, 16], ids=["host scale", "ctl"])
@pytest.mark.parametrize("what,kw,message", FLAT_REFUSALS, ids=[c[0] for c in FLAT_REFUSALS])
def test_flat_step_refusals(what, kw, message, ctl):
    rc, err = _flat(ctl=ctl, **kw)
    assert rc == -1 and err.startswith(b"dg_adam_step_flat: ") and message in err, err


@pytest.mark.parametrize("ctl", [None, 16], ids=["host scale", "ctl"])
@pytest.mark.parametrize("form", [0, 1, 3])
def test_flat_step_of_no_parameters_launches_nothing(form, ctl):
    assert _flat(n=0, form=form, ctl=ctl)[0] == 0


def test_advance_refuses_a_null_state():
    L = _lib.load()
    for ctl in (None, P(16)):
        assert L.dg_adam_advance(None, 2e-4, 0.5, 0.999, ctl, None) == -1
        assert L.dg_last_error().startswith(b"dg_adam_advance: ")


def test_the_removed_entries_are_gone():
    L = _lib.load()
    for name in ("dg_adam_advance_c", "dg_adam_step_flat_c", "dg_adam_step_flat_bf16", "dg_adam_step_flat_x3"):
        assert name not in _lib.SIGNATURES and not hasattr(L, name), name
    assert L.dg_version() >= 101
