"""The map work of one 15-step rollout at B = 8, 16, 32 on the GPU: everything between the panorama encoder and forward_navigation
that concerns the topological map -- update_graph, the graph inputs of forward_navigation and gmap_img_fts -- by the two routes:
  host     GraphMapLite.update_graph per episode + nav_gmap_variable (pack_episode / pack_batch, eleven uploads, etp_gmap_assemble)
           + gather_rows (pack_img_csr in Python, six uploads, etp_gather_sum)
  device   DeviceGraphMaps.update (one upload, etp_gmap_update, the record copy) + nav_inputs (etp_gmap_assemble on the emitted
           arrays) + img_fts (etp_gmap_embed_csr, etp_gather_sum)

    python tools/gmap_update_bench.py [--out profiles/gmap_update_bench.json] [--rounds 5] [--iters 5]

The rollout is tests/gmap_update_ref.random_calls (0 .. 6 candidates per step, some on earlier nodes or candidates, most steps move to
a ghost that is deleted before the next update), loc_noise 0.5, merge_ghost on, ghost_aug 0, an embedding store of H = 768.  Same box,
one process (tools/decide_bench.py's method): both legs are warmed up, they alternate within a round, `rounds` times; a rollout is
timed with a host clock, and EVERY step of BOTH legs ends in torch.cuda.synchronize() once its inputs are
enqueued, so neither leg overlaps a step's launches with the next step's host work (the device route also waits for its record copy
in the middle of the step; that wait is part of its cost).  Reported per leg: the median over rounds of the
per-rollout mean, the lowest and the highest round, and the median per step.  Both routes must end with bit-equal inputs."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from etpnav_amd import graph_inputs  # noqa: E402
from etpnav_amd.graph_inputs import DeviceGraphMaps, GraphMapLite  # noqa: E402
from tests import gmap_update_ref as gr  # noqa: E402

DEV, STEPS, H = "cuda", 15, 768
KEYS = ("gmap_step_ids", "gmap_masks", "gmap_visited_masks", "gmap_pos_fts", "gmap_pair_dists", "gmap_img_fts")


def prepared(calls, B):
    """the arguments of both routes as plain lists, built once: the timed loops only do the map work"""
    steps = []
    for t, c in enumerate(calls):
        ks = c["n_cand"].tolist()
        steps.append(dict(prev=[None if p < 0 else str(p) for p in c["prev_node"]], dele=c["del_ghost"].tolist(), cur_vp=[str(t)] * B, cur_pos=c["cur_pos"],
                          heading=c["cur_heading"].tolist(), cand_vp=[[f"{t}_{k}" for k in range(ks[b])] for b in range(B)],
                          cand_pos=[[c["cand_pos"][b, k] for k in range(ks[b])] for b in range(B)], cur_row=c["cur_row"].tolist(),
                          cand_row=[c["cand_row"][b, :ks[b]].tolist() for b in range(B)]))
    return steps


def host_rollout(steps, B, store):
    lites = [GraphMapLite(False, 0.5, True, 0) for _ in range(B)]
    for t, s in enumerate(steps):
        for b, g in enumerate(lites):
            if s["dele"][b] >= 0:
                g.delete_ghost(list(g.ghost_pos)[s["dele"][b]])
            g.update_graph(s["prev"][b], t + 1, s["cur_vp"][b], s["cur_pos"][b], s["cur_row"][b], s["cand_vp"][b], s["cand_pos"][b], s["cand_row"][b], None)
        nav = graph_inputs.nav_gmap_variable(lites, s["cur_vp"], s["cur_pos"], s["heading"], DEV)
        nav["gmap_img_fts"] = graph_inputs.gather_rows(store, lites, [0] * B, nav["gmap_masks"].shape[1])
        torch.cuda.synchronize()
    return nav


def device_rollout(steps, B, store, maps):
    maps.reset()
    for t, s in enumerate(steps):
        for b, v in enumerate(maps.gmaps):
            if s["dele"][b] >= 0:
                v.delete_ghost(list(v.ghost_pos)[s["dele"][b]])
        maps.update(s["prev"], t + 1, s["cur_vp"], s["cur_pos"], s["heading"], s["cand_pos"], s["cur_row"], s["cand_row"])
        nav = maps.nav_inputs()
        nav["gmap_img_fts"] = maps.img_fts(store, nav["gmap_masks"].shape[1])
        torch.cuda.synchronize()
    return nav


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmap_update_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gmap_update_bench.py measures on the GPU; there is none here")
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "unit": "us per 15-step rollout",
              "shape": {"steps": STEPS, "candidates_per_step": "0..6", "H": H, "loc_noise": 0.5, "merge_ghost": True, "ghost_aug": 0}, "B": {}}
    for B in (8, 16, 32):
        calls, R = gr.random_calls(B, STEPS, None, 1000 + B)
        steps = prepared(calls, B)
        store = torch.randn(R, H, device=DEV)
        maps = DeviceGraphMaps(B, DEV, False, 0.5, True, 0.0)
        legs = {"host": lambda: host_rollout(steps, B, store), "device": lambda: device_rollout(steps, B, store, maps)}
        for fn in legs.values():
            for _ in range(2):
                fn()
        na, nb = legs["host"](), legs["device"]()
        same = all(torch.equal(na[k], nb[k]) for k in KEYS)
        per_round = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                per_round[name].append(timed(fn, a.iters))
        row = {name: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                      "median_us_per_step": round(statistics.median(v) / STEPS, 1)} for name, v in per_round.items()}
        row["final_map"] = {"G": int(na["gmap_masks"].shape[1]), "store_rows": R}
        row["inputs_equal"] = same
        row["speedup"] = round(row["host"]["median_us"] / row["device"]["median_us"], 2)
        result["B"][str(B)] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
