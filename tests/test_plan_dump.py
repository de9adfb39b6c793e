"""tools/plan_dump.py keeps working: the canonical plan / call-trace dumps that hold a rewrite of the plan builders to
"byte for byte the same" build every record, on the CPU, under tests/emulator.py's emulation."""
import importlib.util
import os

import pytest

from usflows_amd import _ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope="module")
def plan_dump():
    spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(ROOT, "tools", "plan_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _collect(run):
    records = []
    n = run(records.append)
    assert n == len(records) and n > 0
    bad = [r[:2] for r in records if any(line.startswith("rejected") for line in r)]
    assert not bad, bad
    return records


def test_plans_of_a_golden_a_tiny_and_a_vector_context_case(plan_dump):
    only = ["synth_d7_k3_hh0_laplace", "tiny:init_d2_k10_gmlive", "vctx:d7_k3"]
    records = _collect(lambda emit: plan_dump.dump_plans(emit, only))
    text = "\n".join("\n".join(r) for r in records)
    assert len(records) == 36 + 2 + 2
    assert "tiny: True" in text and "hidden_saved_fused: True" in text
    assert f"call fn={_ext.FN_COUPLING_VCTX} n_args=6" in text


def test_trace_runs_whole(plan_dump):
    _collect(plan_dump.dump_trace)
