"""The embedding store's work of one 15-step training rollout at B = 8, 16, 32 (V = 17 views, H = 768) on the GPU: from pano_embeds to
gmap_img_fts at every step, and the one backward of the rollout's loss into every step's pano_embeds, by two routes:
  native   EmbedStore.append (etp_pano_store_fwd) + DeviceGraphMaps.img_fts(store) ; backward: etp_gather_sum transposed, autograd's
           sums over the later steps, etp_pano_store_bwd per step
  eager    the trainer's statements (ss_trainer_ETP.py:838-839, 864-865) in torch, a torch.cat-grown store, the same img_fts on that
           tensor ; backward: torch autograd through cat / index / mean
Both legs drive the same DeviceGraphMaps.update with the same rows, so the map's cost is in both; the leg "map_only" runs that alone
(rows precomputed, no store, no gather, no backward) so that it can be subtracted.

    python tools/pano_store_bench.py [--out profiles/pano_store_bench.json] [--rounds 5] [--iters 3]

The rollout is tests/gmap_update_ref.random_calls (0 .. 6 candidates per step, edges and merges occur, most steps delete the ghost
moved to); candidates are interleaved with the panorama views; loss = sum_t (gmap_img_fts_t * W_t).sum().  Same box, one process: the
legs are warmed up and alternate within a round; a rollout is timed with a host clock and ends in torch.cuda.synchronize() after the
backward (every step of every leg already waits for the map's record copy).  Reported per leg: the median over rounds of the
per-rollout mean, the lowest and the highest round.  The two routes' gradients are compared (max |difference| / max |gradient|)."""
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

from etpnav_amd.graph_inputs import DeviceGraphMaps, EmbedStore  # noqa: E402
from tests import gmap_update_ref as gr  # noqa: E402
from tests import pano_store_ref as pr  # noqa: E402

DEV, STEPS, V, H, GMAX = "cuda", 15, 17, 768, 128


def prepared(calls, B, seed):
    """per step: the map's arguments as plain lists, masks / types on the device, and the rows EmbedStore will hand out"""
    rng = np.random.default_rng(seed)
    steps, used = [], 0
    for t, c in enumerate(calls):
        ks = c["n_cand"].tolist()
        types = np.zeros((B, V), np.int64)
        for b in range(B):
            types[b, np.sort(rng.permutation(V)[:ks[b]])] = 1
        base, cand_rows, used = pr.allocate(used, ks)
        steps.append(dict(prev=[None if p < 0 else str(p) for p in c["prev_node"]], dele=c["del_ghost"].tolist(), cur_vp=[str(t)] * B,
                          cur_pos=c["cur_pos"], heading=c["cur_heading"].tolist(), cand_pos=[[c["cand_pos"][b, k] for k in range(ks[b])] for b in range(B)],
                          ks=ks, cur_rows=base.tolist(), cand_rows=cand_rows, types=torch.from_numpy(types).to(DEV),
                          masks=torch.ones(B, V, dtype=torch.bool, device=DEV)))
    return steps, used


def map_step(maps, s, t, cur_rows, cand_rows):
    for b, v in enumerate(maps.gmaps):
        if s["dele"][b] >= 0:
            v.delete_ghost(list(v.ghost_pos)[s["dele"][b]])
    maps.update(s["prev"], t + 1, s["cur_vp"], s["cur_pos"], s["heading"], s["cand_pos"], cur_rows, cand_rows)
    return max(1 + len(v.node_pos) + len(v.ghost_pos) for v in maps.gmaps)


def native_rollout(steps, xs, W, maps, store):
    maps.reset(); store.reset()
    loss = 0.0
    for t, s in enumerate(steps):
        cur_rows, cand_rows = store.append(xs[t], s["masks"], s["types"], s["ks"])
        G = map_step(maps, s, t, cur_rows, cand_rows)
        loss = loss + (maps.img_fts(store, G) * W[t][:, :G]).sum()
    loss.backward()
    return loss


def eager_rollout(steps, xs, W, maps):
    maps.reset()
    loss, store = 0.0, None
    B = xs[0].shape[0]
    for t, s in enumerate(steps):
        m = s["masks"].float()
        avg = (xs[t] * m[..., None]).sum(1) / m.sum(1, keepdim=True)
        rows = [r for i in range(B) for r in (avg[i:i + 1], xs[t][i][s["types"][i] == 1])]
        store = torch.cat(([store] if store is not None else []) + rows, 0)
        G = map_step(maps, s, t, s["cur_rows"], s["cand_rows"])
        loss = loss + (maps.img_fts(store, G) * W[t][:, :G]).sum()
    loss.backward()
    return loss


def map_only_rollout(steps, maps):
    maps.reset()
    for t, s in enumerate(steps):
        map_step(maps, s, t, s["cur_rows"], s["cand_rows"])


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pano_store_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pano_store_bench.py measures on the GPU; there is none here")
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "unit": "us per 15-step rollout, backward included",
              "shape": {"steps": STEPS, "V": V, "H": H, "candidates_per_step": "0..6"}, "B": {}}
    for B in (8, 16, 32):
        calls, _ = gr.random_calls(B, STEPS, None, 2000 + B)
        steps, R = prepared(calls, B, B)
        g = torch.Generator(device=DEV).manual_seed(B)
        xs = [torch.randn(B, V, H, device=DEV, generator=g).requires_grad_(True) for _ in range(STEPS)]
        W = [torch.randn(B, GMAX, H, device=DEV, generator=g) for _ in range(STEPS)]
        maps, store = DeviceGraphMaps(B, DEV, False, 0.5, True, 0.0), EmbedStore(R, H, DEV)

        def clear():
            for x in xs:
                x.grad = None

        legs = {"native": lambda: (clear(), native_rollout(steps, xs, W, maps, store)), "eager": lambda: (clear(), eager_rollout(steps, xs, W, maps)),
                "map_only": lambda: map_only_rollout(steps, maps)}
        for fn in legs.values():
            for _ in range(2):
                fn()
        legs["native"](); store.check()
        gn = [x.grad.clone() for x in xs]
        legs["eager"]()
        diff = max(float((x.grad - n).abs().max()) for x, n in zip(xs, gn)) / max(float(n.abs().max()) for n in gn)
        per_round = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                per_round[name].append(timed(fn, a.iters))
        row = {name: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for name, v in per_round.items()}
        for name in ("native", "eager"):
            row[name]["median_us_less_map"] = round(row[name]["median_us"] - row["map_only"]["median_us"], 1)
        row["store_rows"] = R
        row["grad_max_rel_diff"] = diff
        row["speedup"] = round(row["eager"]["median_us"] / row["native"]["median_us"], 2)
        row["speedup_less_map"] = round(row["eager"]["median_us_less_map"] / row["native"]["median_us_less_map"], 2)
        result["B"][str(B)] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
