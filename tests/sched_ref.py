"""An independent model of stream / event ordering over a recorder trace (etp_graph_trace), and the family of total orders that
tests/test_sched_gpu.py replays a recorded step in.

A trace is a list of rows (kind, stream, event, node), in call order:

    kind 0 kernel node | 1 memset node | 2 empty join node | 3 event record | 4 stream wait

The model knows nothing of how csrc/graphrec.hip turns calls into edges (last node + pending list + join nodes).  It states what
the calls MEAN on a device:

  * a stream is FIFO: whatever is enqueued on it runs after everything enqueued on it, and waited for by it, before;
  * a record stands for everything its stream has enqueued and waited for so far;
  * a wait binds to the latest record of that event at the time of the wait;
  * an event with no record (inside the trace) is complete: waiting for it orders nothing.

Sets of nodes are Python integers used as bit sets (bit i = node i), so a closure is a list `anc` with anc[x] = every node that
happens before x.  Node indices are creation indices; a node is created after everything it depends on, so anc[x] < 2**x.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

KERNEL, MEMSET, JOIN, RECORD, WAIT = 0, 1, 2, 3, 4
Row = Tuple[int, int, int, int]


def n_nodes(trace: Sequence[Row]) -> int:
    return sum(1 for r in trace if r[0] in (KERNEL, MEMSET, JOIN))


def node_streams(trace: Sequence[Row]) -> List[int]:
    """stream of every node, by node index; raises if the trace's node indices are not 0, 1, 2, ... in call order"""
    out = []
    for kind, s, _e, x in trace:
        if kind in (KERNEL, MEMSET, JOIN):
            if x != len(out):
                raise ValueError(f"node rows must carry 0, 1, 2, ... in call order: found {x} where {len(out)} was due")
            out.append(s)
    return out


def hb_closure(trace: Sequence[Row]) -> List[int]:
    """happens-before under the model: anc[x] = bit set of all nodes ordered before node x"""
    return _run(trace)[0]


def stream_frontiers(trace: Sequence[Row]) -> Dict[int, int]:
    """per stream, at the end of the trace: every node enqueued on it or waited for by it -- what the NEXT call on that stream would
    be ordered after.  A step "ends joined" when its origin stream's frontier holds every node: a closing wait with no node behind
    it is part of this state, not of the graph."""
    return _run(trace)[1]


def _run(trace: Sequence[Row]):
    known: Dict[int, int] = {}      # per stream: everything enqueued on it or waited for by it so far
    snap: Dict[int, int] = {}       # per event: what its latest record stands for
    anc: List[int] = []
    for kind, s, e, x in trace:
        if kind in (KERNEL, MEMSET, JOIN):
            if x != len(anc):
                raise ValueError(f"node rows must carry 0, 1, 2, ... in call order: found {x} where {len(anc)} was due")
            anc.append(known.get(s, 0))
            known[s] = known.get(s, 0) | (1 << x)
        elif kind == RECORD:
            snap[e] = known.get(s, 0)
        elif kind == WAIT:
            known[s] = known.get(s, 0) | snap.get(e, 0)
        else:
            raise ValueError(f"unknown trace kind {kind}")
    return anc, known


def graph_closure(n: int, edges: Sequence[Tuple[int, int]]) -> List[int]:
    """transitive closure of a set of graph edges (from, to): anc[x] = bit set of all ancestors of x.  Raises on a cycle."""
    preds: List[List[int]] = [[] for _ in range(n)]
    succs: List[List[int]] = [[] for _ in range(n)]
    for a, b in edges:
        if not (0 <= a < n and 0 <= b < n) or a == b:
            raise ValueError(f"bad edge {(a, b)} in a graph of {n} nodes")
        preds[b].append(a)
        succs[a].append(b)
    left = [len(p) for p in preds]
    ready = [x for x in range(n) if left[x] == 0]
    anc = [0] * n
    done = 0
    while ready:
        x = ready.pop()
        done += 1
        for a in preds[x]:
            anc[x] |= anc[a] | (1 << a)
        for b in succs[x]:
            left[b] -= 1
            if left[b] == 0:
                ready.append(b)
    if done != n:
        raise ValueError("the edges contain a cycle")
    return anc


def incomparable_pairs(anc: Sequence[int]) -> int:
    n = len(anc)
    ordered = sum(bin(a).count("1") for a in anc)
    return n * (n - 1) // 2 - ordered


def late_extension(anc: Sequence[int], streams: Sequence[int], k: int) -> List[int]:
    """The linear extension of `anc` that emits stream k as late as possible: any ready node that is not on k goes first (lowest
    index), a node of k only when nothing else is ready.  Every node unordered with a node x of k then runs before x."""
    n = len(anc)
    emitted, order = 0, []
    pending = list(range(n))
    while pending:
        pick = None
        for x in pending:                      # ascending: the first ready node off k, else the first ready node of k
            if anc[x] & ~emitted:
                continue
            if streams[x] != k:
                pick = x
                break
            if pick is None:
                pick = x
        if pick is None:
            raise ValueError("no node is ready: the relation is not a partial order")
        order.append(pick)
        emitted |= 1 << pick
        pending.remove(pick)
    return order


def extensions(trace: Sequence[Row]) -> List[List[int]]:
    """one extension per stream that owns a node, in stream-index order"""
    anc = hb_closure(trace)
    streams = node_streams(trace)
    return [late_extension(anc, streams, k) for k in sorted(set(streams))]


def is_extension(anc: Sequence[int], order: Sequence[int]) -> bool:
    """`order` is a permutation of all nodes in which every node comes after all of anc[node]"""
    if sorted(order) != list(range(len(anc))):
        return False
    seen = 0
    for x in order:
        if anc[x] & ~seen:
            return False
        seen |= 1 << x
    return True


def uncovered_pairs(anc: Sequence[int], orders: Sequence[Sequence[int]]) -> List[Tuple[int, int]]:
    """every incomparable pair (x, y) that the family does NOT show in both orders (exhaustive)"""
    n = len(anc)
    pos = []
    for o in orders:
        p = [0] * n
        for i, x in enumerate(o):
            p[x] = i
        pos.append(p)
    miss = []
    for y in range(n):
        for x in range(y):
            if (anc[y] >> x) & 1 or (anc[x] >> y) & 1:
                continue
            xy = any(p[x] < p[y] for p in pos)
            yx = any(p[y] < p[x] for p in pos)
            if not (xy and yx):
                miss.append((x, y))
    return miss
