#!/usr/bin/env python3
"""Write tests/golden/conv_plan_table.json: what the conv plan queries answer for the shapes of
tests/test_channels_cpu.py::plan_table_shapes, per op, arithmetic and plan_groups (test_plans_match_the_recorded_table).

The table pins the planner ACROSS a change of the host code, so it is written from the library of the commit BEFORE the change:
build that commit's library somewhere and name it in DG_LIB (the variable discogan_modernized_amd/_lib.py reads).

    DG_LIB=/path/to/parent/libdiscogan_hip.so python tests/golden/make_conv_plan_table.py

Needs no GPU.  Data only.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from discogan_modernized_amd import _lib  # noqa: E402
from tests import test_channels_cpu as T  # noqa: E402

table = dict(columns=list(T.PLAN_COLUMNS), order="shape x op (0, 1, 2) x arithmetic (0, 1, 2) x plan_groups (1, 4); option kt 0",
             shapes=[list(s) for s in T.plan_table_shapes()], rows=T.plan_table_rows(_lib.load()))
with open(T.PLAN_TABLE, "w") as f:
    json.dump(table, f, separators=(",", ":"))
    f.write("\n")
print(f"{T.PLAN_TABLE}: {len(table['rows'])} rows from {_lib.LIB_PATH}")
