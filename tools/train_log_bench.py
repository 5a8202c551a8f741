"""What the training log costs on the GPU (csrc/trainlog.hip, etpnav_amd/trainlog.py):

  norm      the squared gradient norm of the full-size pre-training planner's gradient arena (169.77 M floats, 679 MB: the 140.79 M of the
            fine-tuning model plus the lang2visn layers), by two routes
    report    etp_tensor_report: per tensor, in double, three launches, totals stored
    atomic    etp_grad_sqnorm behind the two zeroing launches FusedAdamW issues in front of it
  driver    PretrainDriver at B = 32, bf16, SAP : MLM 1 : 1, per optimizer step
    off       log_steps=None: as before (task_losses grows by one device scalar per micro-step)
    log100    log_steps=100: two small launches per step, one read every 100 optimizer steps
    item      log_steps=None with ``loss.item()`` after every micro-step: the reference's loop (train_r2r.py:259)
  --small-kernels   nothing is timed: the two meter kernels are launched `--iters` x 100 times, for a kernel-trace run of its own
                    (rocprofv3 --kernel-trace --stats -- python tools/train_log_bench.py --small-kernels)

    python tools/train_log_bench.py [--out profiles/train_log_bench.json] [--rounds 7] [--iters 20] [--steps 8]

Same box, one process: the legs are warmed up and alternate within a round; a leg is timed with a host clock around work that ends in a
device synchronise.  Reported per leg: the median over rounds of the per-call mean, the lowest and the highest round.  The two norm
routes must agree to 1e-5 relative before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402

DEV = "cuda"
B, LT, T, VIEWS = 32, 80, 5, 36


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def legs_stats(legs, rounds, iters, warm=3, scale=1.0, unit="us"):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            per_round[k].append(timed(fn, iters))
    return {k: {f"median_{unit}": round(statistics.median(v) * scale, 3), f"min_{unit}": round(min(v) * scale, 3),
                f"max_{unit}": round(max(v) * scale, 3)} for k, v in per_round.items()}


def build_model():
    from oracle import planner_oracle as po
    from etpnav_amd.planner import GlocalTextPathNavCMT
    cfg = po.PlannerConfig.r2r(use_lang2visn_attn=True)
    return cfg, GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.bfloat16, device=DEV)


def norm_legs(model):
    from etpnav_amd.trainlog import TensorReport
    L, eng = _lib.lib(), model._engine
    g = torch.Generator(device=DEV).manual_seed(0)
    eng.grads.copy_(torch.randn(eng.total, device=DEV, generator=g) * 1e-3)
    rep = TensorReport(eng.table, eng.total, DEV)
    sumsq = torch.zeros(1, dtype=torch.float32, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def report():
        rep.run(eng.grads, s)

    def atomic():
        sumsq.zero_(); bad.zero_()
        check(L.etp_grad_sqnorm(ptr(eng.grads), eng.total, ptr(sumsq), ptr(bad), s), "grad_sqnorm")

    report(); atomic()
    a, b = float(rep.sumsq.item()), float(sumsq.item())
    assert abs(a - b) <= 1e-5 * b, (a, b)
    info = {"arena_elems": eng.total, "arena_bytes": eng.total * 4, "tensors": len(eng.table), "chunks": rep.chunks,
            "sumsq_report": a, "sumsq_atomic": b}
    return {"report": report, "atomic": atomic}, info, rep


def driver_legs(model, cfg, steps):
    from etpnav_amd.pretrain import PretrainDriver
    from etpnav_amd.synthetic import make_sap_batch
    batches = []
    for i in range(4):
        b = make_sap_batch(cfg.vocab_size, cfg.image_feat_size, cfg.depth_feat_size, B, LT, T, VIEWS, n_cand=4, seed=40 + i, ragged=False)
        g = torch.Generator().manual_seed(140 + i)
        lab = torch.full_like(b["txt_ids"], -1)
        pick = (torch.rand(lab.shape, generator=g) < 0.15) & b["txt_masks"]
        pick[:, 1] = True
        lab[pick] = b["txt_ids"][pick]
        b["txt_labels"] = lab
        batches.append(b)

    def driver(**kw):
        return PretrainDriver(model, {"mlm": (batches, 1, None), "sap": (batches, 1, None)}, learning_rate=1e-5, warmup_steps=100,
                              num_train_steps=100000, generator=torch.Generator().manual_seed(3), reuse_steps=True, batch_size=B,
                              max_txt_len=LT, **kw)

    drivers = {"off": driver(), "log100": driver(log_steps=100), "item": driver()}
    its = {k: iter(d.meta) for k, d in drivers.items()}

    def leg(k):
        d, it = drivers[k], its[k]

        def run():
            for _ in range(steps):
                name, batch = next(it)
                loss = d.train_step(name, batch)
                if k == "item":
                    loss.item()
                if k != "log100":
                    d.task_losses.clear()           # keep the comparison about the per-step work, not about a growing list
        return run
    info = {"B": B, "L": LT, "T": T, "V": VIEWS, "dtype": "bf16", "optimizer_steps_per_call": steps, "tasks": "sap : mlm 1 : 1",
            "reuse_steps": True}
    return {k: leg(k) for k in drivers}, info, drivers


def small_kernels(n):
    from etpnav_amd.trainlog import TrainMeter
    L = _lib.lib()
    meter = TrainMeter(["mlm", "sap"], DEV)
    loss = torch.tensor([2.5], device=DEV)
    masks = torch.ones(B, LT, dtype=torch.bool, device=DEV)
    sumsq = torch.tensor([4.0], device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(n):
        check(L.etp_train_meter_loss(ptr(loss), 0.99, ptr(masks), B * LT, B, B, meter.ptr("mlm"), s), "train_meter_loss")
        check(L.etp_train_meter_step(ptr(sumsq), ptr(bad), meter.ptr(None), s), "train_meter_step")
    torch.cuda.synchronize()
    print(json.dumps({"launched": n, "read": meter.read()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_log_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--small-kernels", action="store_true")
    ap.add_argument("--skip-driver", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/train_log_bench.py measures on the GPU; there is none here")
    if a.small_kernels:
        small_kernels(a.iters * 100)
        return
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
              "unit": "us per call, host clock, the timed window ends in a device synchronise; median / min / max over the rounds"}
    cfg, model = build_model()
    legs, info, rep = norm_legs(model)
    result["norm"] = dict(info, iters=a.iters, **legs_stats(legs, a.rounds, a.iters))
    for k in ("report", "atomic"):
        result["norm"][k]["GB_per_s"] = round(info["arena_bytes"] / result["norm"][k]["median_us"] / 1e3, 1)
    rep.close()
    if not a.skip_driver:
        model._engine.grads.zero_()
        legs, info, drivers = driver_legs(model, cfg, a.steps)
        result["driver"] = dict(info, unit="ms per optimizer step", **legs_stats(legs, a.rounds, 1, warm=2, scale=1e-3 / a.steps, unit="ms"))
        for d in drivers.values():
            d.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
