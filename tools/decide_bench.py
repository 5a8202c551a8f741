"""One rollout decision -- node logits to environment actions -- at B = 8, 16, 32 with G = 64 (15 visited nodes, 48 ghosts) on the
GPU: RolloutDecider.decide (etpnav_amd/decide.py: one launch of etp_nav_decide, one device-to-host copy) against what the reference
pays for the same step, restated by us: eager torch for ss_trainer_ETP.py:880-903 (softmax, one .item() per episode,
Categorical.sample, rand_like, where, .cpu()), the networkx all-pairs Dijkstra GraphMap.update_graph runs per episode and step
(graph_utils.py:256-257) on graphs of the same size, and the Python loop over its paths (:908-977).

    python tools/decide_bench.py [--out profiles/decide_bench.json] [--rounds 5] [--iters 50]

Same box, one process.  Every leg is warmed up; the legs alternate within a round, `rounds` times; a call is timed with a host clock
and ends in a device synchronise (the record copy, or .cpu() of the actions).  Reported per leg: the median over rounds of the
per-call mean, the lowest and the highest round.  Legs:
  native            decide() packing and uploading the compact arrays itself
  native_reuse      decide(compact=...) on the tensors nav_gmap_variable(keep_compact=True) uploaded anyway: the trainer's case
  eager_networkx    the restated reference step, Dijkstra included
  eager_only        the same without the Dijkstra (paths taken from a table built once): the B + 1 synchronisations alone
The kernel's own time comes from the library's per-launch events, in a run of its own.  Both sides must choose the same actions.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd import decide  # noqa: E402
from etpnav_amd.graph_inputs import GraphMapLite  # noqa: E402
from tests import decide_ref as dr  # noqa: E402

DEV = "cuda"
N, M = 15, 48


def graph_of(ep):
    """a GraphMapLite holding one decide_ref.random_episode"""
    g = GraphMapLite(False, 0.5, True, 0)
    for i in range(ep["n_nodes"]):
        g.node_pos[str(i)], g.node_stepId[str(i)] = ep["node_pos"][i], i + 1
    for i in range(ep["n_nodes"]):
        for j in range(i + 1, ep["n_nodes"]):
            if ep["adj"][i, j] >= 0:
                g.edges[(str(i), str(j))] = float(ep["adj"][i, j])
    for k in range(ep["n_ghost"]):
        g.ghost_pos[f"g{k}"] = [ep["ghost_pos"][k]]
        g.ghost_aug_pos[f"g{k}"] = ep["ghost_pos"][k]
        g.ghost_fronts[f"g{k}"] = [str(f) for f in ep["ghost_fronts"][k]]
    return g


def eager_step(nx, logits, gmaps, nxgraphs, cur_vp, uniforms, teacher, sample_ratio, scores, paths=None):
    """our restatement of ss_trainer_ETP.py:880-977 in eager torch + networkx (paths None: all-pairs Dijkstra per episode, as
    GraphMap.update_graph does at every step)"""
    probs = torch.softmax(logits, 1)
    for i in range(len(gmaps)):
        scores[i][cur_vp[i]] = probs[i, 0].item()
    cdf = probs.cumsum(1)
    a_t = (cdf > (uniforms[:, :1] * cdf[:, -1:])).int().argmax(1)          # the inverse-CDF draw in place of Categorical's stream
    a_t = torch.where(uniforms[:, 1] <= sample_ratio, teacher, a_t)
    cpu_a_t = a_t.cpu().numpy()
    out = []
    for i, g in enumerate(gmaps):
        if paths is None:
            sp = dict(nx.all_pairs_dijkstra_path(nxgraphs[i]))
            dict(nx.all_pairs_dijkstra_path_length(nxgraphs[i]))
        else:
            sp = paths[i]
        nodes, ghosts = list(g.node_pos.keys()), list(g.ghost_pos.keys())
        if cpu_a_t[i] == 0:
            vs = list(scores[i].items())
            target = vs[int(np.argmax([s for _, s in vs]))][0]
            out.append((0, target, [(vp, g.node_pos[vp]) for vp in sp[cur_vp[i]][target]][1:]))
        else:
            gvp = ghosts[cpu_a_t[i] - 1 - len(nodes)]
            d = [float(np.sqrt(((g.node_pos[f] - g.ghost_aug_pos[gvp]) ** 2).sum())) for f in g.ghost_fronts[gvp]]
            front = g.ghost_fronts[gvp][int(np.argmin(d))]
            out.append((4, front, [(vp, g.node_pos[vp]) for vp in sp[cur_vp[i]][front]][1:]))
    return cpu_a_t, out


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def kernel_us(fn):
    L = _lib.lib()
    L.etp_prof_reset()
    L.etp_prof_enable(1)
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    ents = (_lib.ProfEntry * 32)()
    n = L.etp_prof_report(ents, 32)
    L.etp_prof_enable(0)
    L.etp_prof_reset()
    return {e.name.decode(): round(1e3 * e.ms / e.launches, 2) for e in list(ents)[:n]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decide_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/decide_bench.py measures on the GPU; there is none here")
    import networkx as nx
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "unit": "us per call",
              "shape": {"G": 1 + N + M, "visited_nodes": N, "ghosts": M}, "B": {}}
    for B in (8, 16, 32):
        c = dr.make_case([N] * B, [M] * B, seed=B, sample=True, name=f"bench B={B}")
        gmaps = [graph_of(ep) for ep in c["eps"]]
        cur_vp = [str(ep["cur_node"]) for ep in c["eps"]]
        nxgraphs = []
        for g in gmaps:
            G_ = nx.Graph()
            G_.add_nodes_from(g.node_pos.keys())
            G_.add_weighted_edges_from((u, v, w) for (u, v), w in g.edges.items())
            nxgraphs.append(G_)
        paths = [dict(nx.all_pairs_dijkstra_path(x)) for x in nxgraphs]
        logits = torch.from_numpy(c["logits"]).to(DEV)
        uni, teacher = torch.from_numpy(c["uniforms"]).to(DEV), torch.from_numpy(c["teacher"]).to(DEV)
        d = decide.RolloutDecider(B, DEV, "control", False, True, 15)
        batch = decide.pack_for_decide(gmaps, cur_vp)
        compact = {k: torch.from_numpy(batch[k]).to(DEV) for k in decide.COMPACT_KEYS}
        compact["_dims"] = batch["_dims"]
        scores = [dict() for _ in range(B)]
        for i, g in enumerate(gmaps):
            g.node_stop_scores = {vp: 0.0 for vp in g.node_pos}
            scores[i] = {vp: 0.0 for vp in g.node_pos}
        legs = {
            "native": lambda: d.decide(logits, gmaps, cur_vp, 0, "sample", 0.25, teacher, uniforms=uni),
            "native_reuse": lambda: d.decide(logits, gmaps, cur_vp, 0, "sample", 0.25, teacher, uniforms=uni, compact=compact),
            "eager_networkx": lambda: eager_step(nx, logits, gmaps, nxgraphs, cur_vp, uni, teacher, 0.25, scores),
            "eager_only": lambda: eager_step(nx, logits, gmaps, nxgraphs, cur_vp, uni, teacher, 0.25, scores, paths),
        }
        for fn in legs.values():
            for _ in range(5):
                fn()
        a_native, ea = legs["native_reuse"]()
        a_eager, eo = legs["eager_networkx"]()
        same = bool((a_native == a_eager).all()) and all(
            x["action"]["act"] == y[0] and x["action"].get("front_vp", x["action"].get("stop_vp")) == y[1]
            and [vp for vp, _ in x["action"]["back_path"]] == [vp for vp, _ in y[2]] for x, y in zip(ea, eo))
        kus = kernel_us(legs["native_reuse"])
        per_round = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                per_round[name].append(timed(fn, a.iters))
        row = {name: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
               for name, v in per_round.items()}
        row["kernel_us"] = kus
        row["decisions_equal_eager"] = same
        result["B"][str(B)] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
