"""The predictors of the conv form (ops._x3_ok, x3_all_plane_readers, x3_window_dgrad, model._first_layer_planes) answer what the
recorded trace says (tests/golden/ops_conv_calls.json, part "predictors": tools/ops_conv_trace.py).  They make host queries only, so
no GPU is needed; the plane codes 3 and 4, which only the experiments library answers, are forced by the tool."""
import json
import os

from tools import ops_conv_trace as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_conv_calls.json")


def test_predictors_answer_as_recorded():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert want["predictors"], "no predictor records"
    with T.Recorder(dry=True) as rec:
        T.setup_predictors()
        got = {"records": {}, "predictors": {T.predictor_id(g): T.trace_predictors(g, rec) for g, _ in T.geometries()}}
    differing = T.differing(got, {"records": {}, "predictors": want["predictors"]})
    assert not differing, [(k, T.flat(got).get(k)) for k in differing[:5]]
