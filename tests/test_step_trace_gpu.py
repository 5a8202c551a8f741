"""The layer that issues a training step makes the same library calls, in the same order, on the same streams, as when
tests/golden/step_traces.json was recorded (tools/make_golden_step_traces.py: the 16 schedule cases of tests/test_sched_gpu.py with both
graphs of split_text_bwd, the MLM step, and a forward-only recording of each step class).

Per graph the recorder's pointer-free call trace (etp_graph_trace: kind, stream, event, node per call), the node names in creation order
and n_kernels / n_edges / n_streams are compared for EQUALITY: a host-side change to step.py / pretrain.py that keeps the schedule keeps
every row.  Nothing is replayed and no tensor is compared here; tests/test_sched_gpu.py does that on the same recordings.
"""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("kernel", "memset", "join node", "event record", "stream wait")


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_step_traces", os.path.join(ROOT, "tools", "make_golden_step_traces.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


@pytest.fixture(scope="module")
def golden():
    return TOOL.load()


@pytest.fixture(scope="module")
def stream():
    from etpnav_amd import _lib
    s = TOOL.new_stream()
    yield s
    torch.cuda.synchronize()
    _lib.lib().etp_stream_destroy(s)


def _row_text(g, i):
    kind, s, ev, node = g["rows"][4 * i:4 * i + 4]
    what = g["nodes"][node] if 0 <= node < len(g["nodes"]) else f"event {ev}"
    return f"row {i}: {KINDS[kind] if 0 <= kind < len(KINDS) else kind} on stream {s}, event {ev}, node {node} ({what})"


def _first_difference(got, want):
    """the first differing trace row with the rows around it, from both sides"""
    n_got, n_want = len(got["rows"]) // 4, len(want["rows"]) // 4
    at = next((i for i in range(min(n_got, n_want)) if got["rows"][4 * i:4 * i + 4] != want["rows"][4 * i:4 * i + 4]
               or _row_text(got, i) != _row_text(want, i)), min(n_got, n_want))
    lines = [f"{n_got} trace rows against {n_want} recorded; first difference at row {at}"]
    for name, g, n in (("now", got, n_got), ("recorded", want, n_want)):
        lines += [f"  {name:8s} {'>' if i == at else ' '} {_row_text(g, i)}" for i in range(max(0, at - 3), min(n, at + 3))]
    return "\n".join(lines)


def test_fixture_covers_every_case(golden):
    assert list(golden) == TOOL.keys() and len(golden) == 19
    assert [len(golden[k]) for k in golden] == [2 if k == "split_text_bwd" else 1 for k in golden]


@pytest.mark.parametrize("key", TOOL.keys())
def test_recorded_step_trace_equals_the_fixture(key, golden, stream):
    got, want = TOOL.record_key(key, stream), golden[key]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if g["rows"] != w["rows"] or g["nodes"] != w["nodes"]:
            raise AssertionError(f"{key}, graph {k}: " + _first_difference(g, w))
        assert {f: g[f] for f in ("n_kernels", "n_edges", "n_streams")} == {f: w[f] for f in ("n_kernels", "n_edges", "n_streams")}, \
            (key, k)
