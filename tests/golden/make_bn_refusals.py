#!/usr/bin/env python3
"""Write tests/golden/bn_refusals.json: the return code of every BatchNorm / activation entry point for the argument tuples of
tests/test_shapes_cpu.py::bn_refusal_cases (test_bn_entry_points_refuse_what_the_recorded_table_says).

The table pins the refusals ACROSS a change of the host code, so it is written from the library of the commit BEFORE the change:
build that commit's library somewhere and name it in DG_LIB (the variable discogan_modernized_amd/_lib.py reads).

    DG_LIB=/path/to/parent/libdiscogan_hip.so python tests/golden/make_bn_refusals.py

Only refused tuples may be in it (a call that is not refused would try to launch): the script stops at any other code.
Needs no GPU.  Data only.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from discogan_modernized_amd import _lib  # noqa: E402
from tests import test_shapes_cpu as T  # noqa: E402

cases = [c[0] for c in T.bn_refusal_cases()]
assert len(set(cases)) == len(cases)
codes = T.bn_refusal_codes(_lib.load())
for items, row in codes.items():
    for label, code in zip(cases, row):
        assert code in (-1, -2), f"{label} (bn_items {items}): code {code} is no refusal"
table = dict(order='codes[option "bn_items"][case]: DG_ERR_INVALID -1, DG_ERR_WORKSPACE -2', cases=cases, codes=codes)
with open(T.BN_REFUSALS, "w") as f:
    json.dump(table, f, separators=(",", ":"))
    f.write("\n")
print(f"{T.BN_REFUSALS}: {len(cases)} cases x {len(codes)} from {_lib.LIB_PATH}")
