"""GPU: the Python layer hands the C ABI what it handed it before every launch was folded into HipEngine.call().

tests/golden/engine_calls.json is what tools/record_engine_calls.py recorded on an MI355X from the commit BEFORE that refactor:
per launch of a fixed script of tiny problems the entry, the launch hook's label, every integer argument and the null-ness of
every pointer; per case the dtype and size of the tensors returned; per ill-formed call the exception type.  The same script
runs here, once, and must give the same record."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_engine_calls", os.path.join(ROOT, "tools", "record_engine_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool()


@pytest.fixture(scope="module")
def got(tool):
    return json.loads(json.dumps(tool.record()))   # (through JSON, as the golden file went: tuples become lists)


@pytest.fixture(scope="module")
def want(golden_dir):
    with open(os.path.join(golden_dir, "engine_calls.json")) as f:
        return json.load(f)


def test_every_launch_gets_the_same_arguments(got, want):
    assert [c["case"] for c in got["calls"]] == [c["case"] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        for k, (gl, wl) in enumerate(zip(g["launches"], w["launches"])):
            assert gl == wl, f"case {g['case']!r}, launch {k}: got {gl}, recorded {wl}"
        assert len(g["launches"]) == len(w["launches"]), (g["case"], [x["entry"] for x in g["launches"]], [x["entry"] for x in w["launches"]])
        assert g["returned"] == w["returned"], g["case"]
    entries = {x["entry"] for c in got["calls"] for x in c["launches"]}
    # the script reaches every launching entry the package uses (sdp_traceback_i32 is the C ABI's older spelling, unused here)
    assert entries == {"sdp_forward_f32", "sdp_forward_value_f32", "sdp_backward_f32", "sdp_backward_range_f32", "sdp_adjoint_forward_f32",
                       "sdp_adjoint_forward_loss_f32", "sdp_adjoint_backward_f32", "sdp_forward_f64", "sdp_backward_f64",
                       "sdp_adjoint_forward_f64", "sdp_adjoint_backward_f64", "sdp_traceback_rule_i32", "sdp_hard_forward_f32",
                       "sdp_hard_forward_value_f32", "sdp_hard_walk_f32", "sdp_loss_forward_f32", "sdp_loss_backward_f32",
                       "sdp_scores_f32", "sdp_scores_backward_f32", "sdp_alignment_targets", "sdp_alignment_stats"}


def test_ill_formed_calls_raise_what_they_raised(tool, got, want):
    """A tensor of the wrong dtype, one on the CPU, an `out` of the wrong shape, ...: per engine method and public function
    the exception type of the recorded commit, which is also the type written down next to each case in the tool."""
    from deepblast_amd._engine import get_engine
    eng = get_engine()
    noted = {name: (None if exc is None else exc.__name__) for name, exc, _ in tool.error_cases(eng, tool.Tensors(eng))}
    assert got["errors"] == want["errors"] == noted
    assert {"TypeError", "ValueError", "RuntimeError"} <= set(noted.values())


def test_a_failing_range_sweep_is_reported_under_its_own_name():
    """The one intended change of behaviour: sdp_backward_range_f32 used to fail under the name of sdp_backward_f32."""
    import torch
    from deepblast_amd._engine import get_engine
    eng = get_engine()
    th = torch.rand(2, 4, 4, device="cuda:0")
    _, Q = eng.forward(th, -th, 0)
    with pytest.raises(ValueError, match="sdp_backward_range_f32"):
        eng.backward(torch.ones(2, device="cuda:0"), Q, (2, 4, 4), 7, pair_range=(0, 1), out=torch.empty_like(th))   # variant 7: refused
