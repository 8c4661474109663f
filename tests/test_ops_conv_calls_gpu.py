"""The interior-conv op wrappers ask the library for what the recorded call trace says.

tools/ops_conv_trace.py drives ops.conv_fwd / conv_dgrad / conv_wgrad and the grouped forms over every geometry of
tests/test_plan_cases_cpu.PLAN_CASES and the 4 x 4 heads, crossed with want_stats, the arithmetic contexts, operands with and without
shadows or plane entries (chunk-major and plane-only ones among them), accumulation, the X3_RSP / X3_FWW switches and groups of 2 and
4 under both group plans, and records per point the library calls with every scalar and every pointer by name, the host queries,
what came back, the derived-copy table changes and any refusal.  tests/golden/ops_conv_calls.json holds that record as the three
separate wrappers (before the request record and the single form choice) made it, as one digest per point (the text is 0.7 MiB;
T.digest); a wrapper that launches another entry point, hands
over another operand, sizes a workspace or a statistics buffer differently or refuses with another message differs from it."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

from tools import ops_conv_trace as T  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_conv_calls.json")


def test_conv_wrappers_make_the_recorded_calls():
    with open(GOLDEN) as f:
        want = json.load(f)
    trace, slow = T.run(dry=False)
    print("slowest geometries:", [(round(t, 2), g) for t, g in slow[:5]])
    assert T.summary(trace) == want["counts"]
    differing, now = T.differing(trace, want), T.flat(trace)
    assert not differing, f"{len(differing)} of {want['counts']['records']} records differ from the recorded ones, e.g.\n" + "\n".join(
        f"  {k}\n    now: {now.get(k)}" for k in differing[:5]) + "\n(tools/ops_conv_trace.py --out on both commits, then --diff, shows both sides)"
