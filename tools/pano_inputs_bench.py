"""The stretch of a rollout step between the waypoint head and the panorama encoder at B = 8, 16, 32 on the GPU: from "candidate table
and embeddings ready on the device" to "rgb_fts, dep_fts, loc_fts, nav_types, view_lens ready on the device", by three routes:
  existing    waypoint._waypoint_tail_mode (the table copy, two flips + pools, the per-episode gathers and angle features) +
              graph_inputs.vp_feature_variable (host mask loop, three torch.cat + uploads, three etp_vp_gather launches)
  fused       the same call with net.fuse_pano_inputs: the table copy, the host values the simulator side needs, and ONE launch of
              etp_pano_inputs at the reference's padded length (computed from the copy)
  fused_v16   the same at the fixed capacity of 16 view rows
and, to be subtracted, copy_only: the candidate table's device-to-host copy alone, which every route makes.

    python tools/pano_inputs_bench.py [--out profiles/pano_inputs_bench.json] [--rounds 7] [--iters 20]

The predictor is a stand-in that hands back a prepared device table (K mixed 0 .. 5 per episode, sampled and eval rows differing), so
neither the head's GEMMs nor the tail kernel is in any leg; embeddings are random [12B, 512] / [12B, 128, 4, 4] fp32.  Same box, one
process: the legs are warmed up and alternate within a round; a leg is timed with a host clock over `iters` calls and ends in
torch.cuda.synchronize().  Reported per leg: the median over rounds of the per-call mean, the lowest and the highest round.  The fused
outputs are compared with the existing route's before timing (exact outputs bit for bit, dep_fts max |difference|)."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from etpnav_amd import graph_inputs  # noqa: E402
from etpnav_amd import waypoint as wp  # noqa: E402

DEV = "cuda"


def mixed_table(B, seed):
    rng = np.random.default_rng(seed)
    t = np.full((7, B, 5), -1, np.int32)
    for b in range(B):
        k = b % 6 if b < 6 else int(rng.integers(0, 6))
        t[0, b, 0] = k
        t[1, b, :k], t[5, b, :k] = np.sort(rng.integers(0, 120, k)), rng.integers(0, 120, k)
        t[2, b, :k], t[6, b, :k] = rng.integers(0, 12, k), rng.integers(0, 12, k)
    return t


class Tail:
    def __init__(self, table):
        self.cand = wp.CandidateTable(None, None, torch.from_numpy(table).to(DEV), True)

    def __call__(self, rgb, dep):
        return None

    def candidates(self, logits, in_train, generator=None, uniforms=None):
        return self.cand


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pano_inputs_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pano_inputs_bench.py measures on the GPU; there is none here")
    pool = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d((1, 1)), torch.nn.Flatten(start_dim=2))
    idx, fts = wp.pano_constants()
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters,
              "unit": "us per call, host clock, from table + embeddings on the device to the five planner inputs on the device",
              "shape": {"rgb_embedding": "[12B, 512]", "depth_embedding": "[12B, 128, 4, 4]", "candidates_per_episode": "0..5, mixed",
                        "in_train": True}, "B": {}}
    for B in (8, 16, 32):
        g = torch.Generator(device=DEV).manual_seed(B)
        rgb = torch.randn(12 * B, 512, device=DEV, generator=g)
        dep = torch.randn(12 * B, 128, 4, 4, device=DEV, generator=g)
        tail = Tail(mixed_table(B, 300 + B))
        net = SimpleNamespace(space_pool_rgb=pool, space_pool_depth=pool, pano_img_idxes=idx, pano_angle_fts=fts, fuse_pano_inputs=False,
                              pano_inputs_capacity=None)

        def route(fuse, cap):
            net.fuse_pano_inputs, net.pano_inputs_capacity = fuse, cap
            return graph_inputs.vp_feature_variable(wp._waypoint_tail_mode(net, tail, rgb, dep, B, True, None, None), DEV)

        legs = {"existing": lambda: route(False, None), "fused": lambda: route(True, None), "fused_v16": lambda: route(True, 16),
                "copy_only": lambda: tail.cand.table.cpu().numpy()}
        for fn in legs.values():
            for _ in range(3):
                fn()
        old, new, cap = legs["existing"](), legs["fused"](), legs["fused_v16"]()
        V = old["rgb_fts"].shape[1]
        for k in ("rgb_fts", "loc_fts", "nav_types", "view_lens"):
            assert torch.equal(old[k], new[k]), k
            assert torch.equal(old[k], cap[k][:, :V] if cap[k].dim() > 1 else cap[k]), k
        dep_diff = float((old["dep_fts"] - new["dep_fts"]).abs().max())
        per_round = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                per_round[name].append(timed(fn, a.iters))
        row = {name: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for name, v in per_round.items()}
        for name in ("existing", "fused", "fused_v16"):
            row[name]["median_us_less_copy"] = round(row[name]["median_us"] - row["copy_only"]["median_us"], 1)
        row["reference_length"] = V
        row["dep_fts_max_abs_diff"] = dep_diff
        row["speedup"] = round(row["existing"]["median_us"] / row["fused"]["median_us"], 2)
        row["speedup_v16"] = round(row["existing"]["median_us"] / row["fused_v16"]["median_us"], 2)
        result["B"][str(B)] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
