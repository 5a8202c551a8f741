"""One 15-step fine-tuning rollout with its backward at B = 8, 16, 32 on the GPU: etpnav_amd.rollout.RolloutDriver (the loss, its scale
and the IL_loss log on the device: csrc/rollout_loss.hip) against tests/rollout_ref.hand_composed_rollout, the same loop written out
from the package's public pieces as INTEGRATION.md §2b-§2h tells a user to, with torch's F.cross_entropy per step, the host-side
scale and loss.item() -- what the parent's pieces give.

    python tools/rollout_driver_bench.py [--out profiles/rollout_driver_bench.json] [--rounds 5] [--batches 8,16,32]
                                         [--image-size 64] [--clip-layers 2] [--dtype bf16]

Same box, one process.  Environments: tests/rollout_ref.ScriptedEnvs with goals out of reach, so every environment runs all 15 steps
(the last one is the forced stop); observations are drawn once and reused.  The planner is the full-size model; the two perception
encoders are the small ones of the tests unless --image-size 224 --clip-layers 12 asks for the real sizes.  Both legs are warmed up;
they alternate within a round, `rounds` times; a rollout is timed with a host clock from envs.resume_all() to the end of
loss.backward() and a device synchronise (the hand-composed leg's loss.item() included, as the reference's :1057 has it).  Reported
per leg: the median over rounds, the lowest and the highest round.  There is no target: nobody has measured either route before.

  --small-kernels   nothing is timed: the three loss kernels are launched over a 15-step rollout of B = 32, G = 64, `--iters` times, for
                    a kernel-trace run of its own (rocprofv3 --kernel-trace --stats -- python tools/rollout_driver_bench.py --small-kernels)
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from etpnav_amd import rollout  # noqa: E402
from tests import rollout_ref as rr  # noqa: E402

DEV = "cuda"
MAX_LEN = 15


def world(a):
    from etpnav_amd import clip as cl
    from etpnav_amd import depth as dp
    from etpnav_amd import waypoint as wp
    from etpnav_amd.policy import ETP
    from tests import clip_ref as cr
    from tests import depth_ref as dr
    from tests import waypoint_ref as wr
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    S = a.image_size
    net = ETP(model_config=SimpleNamespace(task_type="r2r"), dtype=dtype, device=DEV)
    small = S != 256 and S != 224
    bp, blocks = (dr.ALL_CASES[0][1], dr.ALL_CASES[0][2]) if small else (32, (3, 4, 6, 3))
    S_dep = S if small else 256
    net.rgb_encoder = cl.CLIPEncoder(device=DEV, dtype=dtype, image_size=S, layers=a.clip_layers)
    net.rgb_encoder.load_state_dict(cr.make_weights(S, a.clip_layers, 3), strict=True)
    net.depth_encoder = dp.DepthEncoder(device=DEV, dtype=dtype, image_size=S_dep, base_planes=bp, blocks=blocks)
    net.depth_encoder.load_state_dict(dr.make_weights(S_dep, bp, blocks, 3), strict=True)
    pred = wp.BinaryDistPredictorTRM(device=DEV, dtype=dtype)
    pred.load_state_dict(wr.make_weights(2), strict=True)
    pred.eval()
    net.train()
    pool = []
    for i in range(6):
        images, depth = cr.make_images(12, S, 50 + i), dr.make_depth(40 + i, 12, S_dep)
        obs = {}
        for v in range(12):
            suffix = "" if v == 0 else f"_{v * 30.0}"
            obs["rgb" + suffix], obs["depth" + suffix] = images[v].contiguous(), depth[v].contiguous()
        pool.append(obs)
    return net, pred, pool


def make_obs_fn(pool):
    def make_obs(slot, step, pos):
        obs = dict(pool[(slot + 2 * step) % len(pool)])
        ids = np.random.default_rng(slot).integers(2, 1000, 40)
        ids[30 - slot % 7:] = 0
        obs["instruction"] = torch.from_numpy(ids.astype(np.int64))
        return obs
    return make_obs


def obs_to_batch(observations):
    return {k: torch.stack([o[k] for o in observations]).to(DEV) for k in observations[0]}


def small_kernels(iters):
    steps = rr.make_steps(32, 64, MAX_LEN, 0.0, "some", 1, DEV)
    rec = torch.zeros(8, dtype=torch.int64, device=DEV)
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    log = torch.zeros(3, dtype=torch.int64, device=DEV)
    dl = [torch.empty_like(x) for x, _ in steps]
    for _ in range(iters):
        rec.zero_()
        for x, y in steps:
            rollout.rollout_ce_fwd(x, y, rec)
        rollout.rollout_loss(rec, 1.0, loss, log)
        for (x, y), d in zip(steps, dl):
            rollout.rollout_ce_bwd(x, y, rec, 1.0, None, dlogits=d)
    torch.cuda.synchronize()
    print(f"{iters} rollouts: {iters * MAX_LEN} forward, {iters} loss and {iters * MAX_LEN} backward launches, B = 32 shrinking, G = 64")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_driver_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="8,16,32")
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--clip-layers", type=int, default=2)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--small-kernels", action="store_true")
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rollout_driver_bench.py measures on the GPU; there is none here")
    if a.small_kernels:
        small_kernels(a.iters)
        return
    net, pred, pool = world(a)
    make_obs = make_obs_fn(pool)
    cfg = rollout.RolloutConfig(max_len=MAX_LEN, waypoint_aug=False, hidden=768)
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "unit": "ms per rollout (forward, loss, backward)",
              "steps": MAX_LEN, "dtype": a.dtype, "image_size": a.image_size, "clip_layers": a.clip_layers, "B": {}}
    for B in [int(b) for b in a.batches.split(",")]:
        starts = [[30.0 * s, 0.0, 0.0] for s in range(B)]
        goals = [[30.0 * s, 0.0, -500.0] for s in range(B)]
        uni = np.random.default_rng(B).random((MAX_LEN, B, 2)).astype(np.float32)
        uni[..., 1] = 0.0                                  # the teacher's action: towards the goal, never a stop before the last step
        steps_seen = {}

        def driver_leg():
            envs = rr.ScriptedEnvs(starts, goals, make_obs=make_obs)
            drv = rollout.RolloutDriver(net, pred, envs, cfg, obs_to_batch, DEV, rng=random.Random(1))
            net.zero_grad()
            loss = drv.rollout("train", 1.0, 0.5, uniforms=uni)
            loss.backward()
            drv.check()
            steps_seen["driver"] = drv.steps_run
            return loss

        def hand_leg():
            envs = rr.ScriptedEnvs(starts, goals, make_obs=make_obs)
            net.zero_grad()
            loss, trace = rr.hand_composed_rollout(net, pred, envs, cfg, obs_to_batch, DEV, 1.0, 0.5, uni, random.Random(1))
            loss.backward()
            loss.item()                                    # self.logs['IL_loss'].append(loss.item())   (:1057)
            steps_seen["hand"] = len(trace)
            return loss

        legs = {"driver": driver_leg, "hand_composed": hand_leg}
        for fn in legs.values():
            fn()
        per_round = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                per_round[name].append((time.perf_counter() - t0) * 1e3)
        row = {name: {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2)}
               for name, v in per_round.items()}
        row["steps_run"] = dict(steps_seen)
        result["B"][str(B)] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
