"""The parameter-arena layout and every scratch-size query of the planner and the three frozen engines equal the snapshot recorded
from the build before their host-side machinery was consolidated into csrc/arena.h (tests/golden/arena_layouts.json, written by
tools/make_golden_arena_layouts.py).  Needs the built library, no GPU."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_arena_layouts", os.path.join(ROOT, "tools", "make_golden_arena_layouts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_layouts_and_scratch_sizes_equal_the_recorded_snapshot():
    tool = _tool()
    with open(tool.GOLDEN) as f:
        want = json.load(f)
    got = tool.snapshot()
    # 4 planner, 2 waypoint, 4 CLIP and 4 depth configurations, every one with its size queries at two batch sizes
    assert sorted(want) == sorted(got) and len(want) == 14
    for key in sorted(want):
        for field in sorted(want[key]):
            assert got[key][field] == want[key][field], (key, field)
        assert sorted(got[key]) == sorted(want[key]), key


def test_offsets_follow_the_64_element_rule_and_matrices_come_first():
    """What the fused AdamW and the data-parallel slice plan rely on, on the small tables the snapshot holds in full: every offset is a
    multiple of 64, slots do not overlap, and the matrix region [0, n_matrix) is a prefix of the arena."""
    snap = _tool().snapshot()
    seen = 0
    for key, e in snap.items():
        if "table" not in e:
            continue
        seen += 1
        spans = []
        for row in e["table"]:
            _, shape, off = row.split("|")
            n = 1
            for s in shape.split("x"):
                n *= int(s)
            assert int(off) % 64 == 0, (key, row)
            spans.append((int(off), int(off) + n))
        spans.sort()
        assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), key
        assert spans[-1][1] <= e["total"] and 0 < e["n_matrix"] <= e["total"] and e["n_matrix"] % 64 == 0, key
        assert any(a == e["n_matrix"] for a, _ in spans), key
    assert seen == 6
