"""Pins tests/sched_ref.py, the model that tests/test_sched_gpu.py holds the recorded step schedule to, on random stream programs
(no GPU, no library):

  * validity     every member of extensions() is a linear extension of the model's happens-before relation;
  * coverage     every incomparable pair of nodes occurs in both orders somewhere in the family (checked exhaustively);
  * recorder     a line-by-line Python port of csrc/graphrec.hip's rule (take_deps, event_record with its join node,
                 stream_wait_event) builds a graph whose closure equals the model's;
  * sensitivity  abstract programs with declared read / write sets, simulated from a poisoned state: a join dropped in front of a
                 reader, in front of an overwriter of a buffer that is still read, and in front of a second writer each make at least
                 one extension differ from program order, and the unmutated program agrees in all of them.
"""
import random

import pytest

from tests import sched_ref as sr

N_PROGRAMS = 300
SEED = 20240611


# ---- random stream programs: ("node", s) | ("record", s, e) | ("wait", s, e) ---------------------------------------------------------
def random_program(rng):
    S = rng.randint(2, 5)
    E = rng.randint(1, 6)
    ops = []
    for _ in range(rng.randint(5, 60)):
        r = rng.random()
        s = rng.randrange(S)
        if r < 0.45:
            ops.append(("node", s))
        elif r < 0.70:
            ops.append(("record", s, rng.randrange(E)))            # re-records of the same event are common (E is small)
        else:
            ops.append(("wait", s, rng.randrange(E + 1)))           # event E is never recorded
            if rng.random() < 0.4:
                ops.append(("record", s, rng.randrange(E)))        # record right after a pending wait: the join-node case
    if rng.random() < 0.5:                                          # waits before a stream's first node
        ops = [("node", 0), ("record", 0, 0), ("wait", S - 1, 0), ("wait", S - 1, E)] + ops
    return ops


# ---- the recorder's rule, ported line by line from csrc/graphrec.hip -----------------------------------------------------------------
class RecorderPort:
    def __init__(self):
        self.last, self.pending, self.events = {}, {}, {}
        self.edges, self.trace, self.n = [], [], 0

    def take_deps(self, s):
        d = []
        if s in self.last:
            d.append(self.last[s])
        if s in self.pending:
            for n in self.pending[s]:
                if n not in d:
                    d.append(n)
            self.pending[s] = []
        return d

    def _add_node(self, kind, s, deps):
        node = self.n
        self.n += 1
        self.edges += [(d, node) for d in deps]
        self.trace.append((kind, s, -1, node))
        return node

    def kernel(self, s):
        deps = self.take_deps(s)
        self.last[s] = self._add_node(sr.KERNEL, s, deps)

    def event_record(self, e, s):
        if self.pending.get(s):
            deps = self.take_deps(s)
            self.last[s] = self._add_node(sr.JOIN, s, deps)
        self.trace.append((sr.RECORD, s, e, -1))
        if s in self.last:
            self.events[e] = self.last[s]
        else:
            self.events.pop(e, None)

    def stream_wait_event(self, s, e):
        self.trace.append((sr.WAIT, s, e, -1))
        if e in self.events:
            self.pending.setdefault(s, []).append(self.events[e])


def record(ops):
    r = RecorderPort()
    for op in ops:
        if op[0] == "node":
            r.kernel(op[1])
        elif op[0] == "record":
            r.event_record(op[2], op[1])
        else:
            r.stream_wait_event(op[1], op[2])
    return r


@pytest.fixture(scope="module")
def programs():
    rng = random.Random(SEED)
    return [random_program(rng) for _ in range(N_PROGRAMS)]


def test_programs_contain_the_cases_the_model_is_pinned_on(programs):
    rerecorded = unrecorded = early_wait = join_nodes = 0
    for ops in programs:
        seen_rec, seen_node = set(), set()
        for op in ops:
            if op[0] == "record":
                rerecorded += op[2] in seen_rec
                seen_rec.add(op[2])
            elif op[0] == "wait":
                unrecorded += op[2] not in seen_rec
                early_wait += op[1] not in seen_node
            else:
                seen_node.add(op[1])
        join_nodes += sum(1 for row in record(ops).trace if row[0] == sr.JOIN)
    assert min(rerecorded, unrecorded, early_wait, join_nodes) > 50, (rerecorded, unrecorded, early_wait, join_nodes)


def test_every_extension_is_a_valid_linear_extension(programs):
    for ops in programs:
        trace = record(ops).trace
        anc = sr.hb_closure(trace)
        exts = sr.extensions(trace)
        assert len(exts) == len(set(sr.node_streams(trace)))
        for o in exts:
            assert sr.is_extension(anc, o), (ops, o)


def test_every_incomparable_pair_occurs_in_both_orders(programs):
    pairs = 0
    for ops in programs:
        trace = record(ops).trace
        anc = sr.hb_closure(trace)
        assert sr.uncovered_pairs(anc, sr.extensions(trace)) == [], ops
        pairs += sr.incomparable_pairs(anc)
    assert pairs > 1000             # the programs are not all chains


def test_nodes_of_one_stream_are_totally_ordered(programs):
    for ops in programs:
        trace = record(ops).trace
        anc, streams = sr.hb_closure(trace), sr.node_streams(trace)
        last = {}
        for x, s in enumerate(streams):
            if s in last:
                assert (anc[x] >> last[s]) & 1
            last[s] = x


def test_recorder_rule_has_the_models_closure(programs):
    for ops in programs:
        r = record(ops)
        assert sr.graph_closure(r.n, r.edges) == sr.hb_closure(r.trace), ops


def test_graph_closure_rejects_cycles_and_bad_edges():
    assert sr.graph_closure(3, [(0, 1), (1, 2)]) == [0, 1, 3]
    with pytest.raises(ValueError):
        sr.graph_closure(2, [(0, 1), (1, 0)])
    with pytest.raises(ValueError):
        sr.graph_closure(2, [(0, 2)])
    assert not sr.is_extension([0, 1], [1, 0])
    assert not sr.is_extension([0, 0], [0, 0])


def test_introspection_entry_points_refuse_a_null_graph_without_a_gpu():
    import ctypes
    from etpnav_amd import _lib
    L = _lib.lib()
    out, rows, g = (ctypes.c_int64 * 4)(), (ctypes.c_int32 * 4)(), ctypes.c_void_p()
    buf = ctypes.create_string_buffer(16)
    assert [L.etp_graph_info(None, out), L.etp_graph_trace(None, rows, 1), L.etp_graph_edges(None, rows, rows, 1),
            L.etp_graph_node_name(None, 0, buf, 16), L.etp_graph_linearize(None, rows, 1, ctypes.byref(g))] == [-1] * 5


# ---- sensitivity: abstract programs with read / write sets ---------------------------------------------------------------------------
POISON = "poison"


def simulate(rw, order):
    """rw[x] = (reads, writes) of node x.  Every buffer starts poisoned; a node writes a version value made of its own index and what
    it read (poison if anything it read was poison) into every buffer of its write set."""
    state = {}
    for x in order:
        reads, writes = rw[x]
        vals = tuple(state.get(b, POISON) for b in reads)
        v = POISON if POISON in vals else (x, vals)
        for b in writes:
            state[b] = v
    return state


def hazard_program(rng, kind, mutate):
    """A random amount of private work on 2 to 5 streams around one producer / consumer pattern between two of them.  `mutate` drops
    the one wait that the pattern depends on.  Returns (ops, rw) with rw aligned to the "node" ops."""
    S = rng.randint(2, 5)
    a, b = rng.sample(range(S), 2)
    ops, rw = [], []

    def node(s, reads, writes):
        ops.append(("node", s))
        rw.append((tuple(reads), tuple(writes)))

    def filler():
        for _ in range(rng.randint(0, 6)):
            s = rng.randrange(S)
            node(s, [f"priv{s}"] if any(f"priv{s}" in w for _, w in rw) else [], [f"priv{s}"])

    filler()
    node(a, [], ["X"])                                  # P
    ops.append(("record", a, 0))
    filler()
    if kind == "reader":                                # the join in front of a reader of X
        if not mutate:
            ops.append(("wait", b, 0))
        node(b, ["X"], ["Y"])
    elif kind == "overwriter":                          # the join in front of an overwriter of X while b still reads it
        ops.append(("wait", b, 0))
        node(b, ["X"], ["Y"])                           # R
        ops.append(("record", b, 1))
        filler()
        if not mutate:
            ops.append(("wait", a, 1))
        node(a, [], ["X"])                              # O
    elif kind == "second_writer":                       # the join in front of a second writer of X
        if not mutate:
            ops.append(("wait", b, 0))
        node(b, [], ["X"])
    filler()
    for s in range(S):                                  # the program ends joined into stream a, where X and Y are read
        if s != a:
            ops.append(("record", s, 2 + s))
            ops.append(("wait", a, 2 + s))
    node(a, ["X"] + (["Y"] if kind != "second_writer" else []), ["OUT"])
    return ops, rw


@pytest.mark.parametrize("kind", ["reader", "overwriter", "second_writer"])
def test_family_catches_a_dropped_join(kind):
    rng = random.Random(SEED + len(kind))
    for _ in range(100):
        st = rng.getstate()
        results = {}
        for mutate in (False, True):
            rng.setstate(st)                            # the same program, with and without its join
            ops, rw = hazard_program(rng, kind, mutate)
            r = record(ops)
            full = [None] * r.n                         # join nodes read and write nothing
            it = iter(rw)
            for row in r.trace:
                if row[0] == sr.KERNEL:
                    full[row[3]] = next(it)
                elif row[0] == sr.JOIN:
                    full[row[3]] = ((), ())
            want = simulate(full, range(r.n))
            assert POISON not in want.values()
            results[mutate] = [simulate(full, o) == want for o in sr.extensions(r.trace)]
        assert all(results[False]), (kind, "the joined program must agree in every extension")
        assert not all(results[True]), (kind, "a dropped join must show in at least one extension")
