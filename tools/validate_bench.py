"""The validation tail and one validation pass on the GPU, each by two routes:

  tail      Nm = 300 masked rows, V = 30 522 (ldv 30 528), fp32 logits
    native    etp_vocab_eval + etp_eval_accum: two launches, nothing read by the host (the window ends in one synchronise)
    torch     the reference's three statements on the same logits (train_r2r.py:365-367): F.cross_entropy(reduction='sum'),
              scores.max(dim=-1)[1] == labels, with their two .item() calls
  validate  PretrainDriver.validate over `--batches` MLM and SAP batches (B = 32, L = 80, T = 5, V = 36, full-size bf16 planner)
    native    as the library does it: counters on the device, one read per task
    torch     the same forwards, then the reference's statements on MlmStep.scores() / PlannerStep.logits, two .item() per batch

    python tools/validate_bench.py [--out profiles/validate_bench.json] [--rounds 7] [--iters 20]

Same box, one process: the legs are warmed up and alternate within a round; a leg is timed with a host clock around work that ends in a
device synchronise.  Reported per leg: the median over rounds of the per-call mean, the lowest and the highest round.  Both routes must
agree before anything is timed (the tail on the same logits: counts equal, loss sums to 1e-5 relative; the passes: two forwards of
their own, losses to 1e-4 relative)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402

DEV = "cuda"
NM, V = 300, 30522
B, LT, T, VIEWS = 32, 80, 5, 36


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def legs_stats(legs, rounds, iters):
    for fn in legs.values():
        for _ in range(3):
            fn()
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            per_round[k].append(timed(fn, iters))
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
            for k, v in per_round.items()}


def tail_legs():
    from etpnav_amd.validate import EvalCounters
    L = _lib.lib()
    g = torch.Generator().manual_seed(0)
    ldv = (V + 7) // 8 * 8
    buf = torch.zeros(NM, ldv)
    buf[:, :V] = torch.randn(NM, V, generator=g) * 3
    labels = torch.randint(0, V, (NM,), generator=g)
    labels[::2] = buf[::2, :V].argmax(-1)
    buf, labels = buf.to(DEV), labels.to(DEV)
    scores = buf[:, :V]
    nll = torch.empty(NM, dtype=torch.float32, device=DEV)
    pred = torch.empty(NM, dtype=torch.int32, device=DEV)
    counters = EvalCounters(DEV)
    s = torch.cuda.current_stream().cuda_stream
    host = {"loss": 0.0, "correct": 0}

    def native():
        check(L.etp_vocab_eval(ptr(buf), ptr(labels), NM, V, ldv, ptr(nll), ptr(pred), s), "vocab_eval")
        check(L.etp_eval_accum(ptr(nll), ptr(pred), ptr(labels), NM, -1, counters.ptr(), s), "eval_accum")

    def torch_tail():
        loss = F.cross_entropy(scores, labels, reduction="sum")
        host["loss"] += loss.item()
        host["correct"] += (scores.max(dim=-1)[1] == labels).sum().item()

    native()
    torch_tail()
    loss_sum, n_correct, n_rows = counters.read()
    assert n_rows == NM and n_correct == host["correct"], (n_correct, host["correct"])
    assert abs(loss_sum - host["loss"]) <= 1e-5 * abs(host["loss"]), (loss_sum, host["loss"])
    return {"native": native, "torch": torch_tail}, {"Nm": NM, "V": V, "ldv": ldv, "logits_bytes": NM * V * 4, "n_correct": n_correct}


def validate_legs(n_batches):
    from oracle import planner_oracle as po
    from etpnav_amd.planner import GlocalTextPathNavCMT
    from etpnav_amd.pretrain import MlmStep, PretrainDriver
    from etpnav_amd.synthetic import make_sap_batch
    cfg = po.PlannerConfig.r2r(use_lang2visn_attn=True)
    model = GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.bfloat16, device=DEV).eval()
    batches = []
    for i in range(n_batches):
        b = make_sap_batch(cfg.vocab_size, cfg.image_feat_size, cfg.depth_feat_size, B, LT, T, VIEWS, n_cand=4, seed=40 + i, ragged=False)
        g = torch.Generator().manual_seed(140 + i)
        lab = torch.full_like(b["txt_ids"], -1)
        pick = (torch.rand(lab.shape, generator=g) < 0.15) & b["txt_masks"]
        pick[:, 1] = True
        lab[pick] = b["txt_ids"][pick]
        b["txt_labels"] = lab
        batches.append(b)
    loaders = {"mlm": batches, "sap": batches}
    drv = PretrainDriver(model, {"mlm": batches, "sap": batches}, dropout=None)
    last = {}

    def native():
        last["native"] = drv.validate(loaders)

    def torch_route():
        out = {}
        loss, correct, rows = 0.0, 0, 0
        for b in batches:
            st = MlmStep(model, b, dropout=None)
            st.run_eager(backward=False)
            scores = st.scores()
            loss += F.cross_entropy(scores, st.labels, reduction="sum").item()
            correct += (scores.max(dim=-1)[1] == st.labels).sum().item()
            rows += st.labels.numel()
            torch.cuda.current_stream().synchronize()
            st.close()
        out["val_mlm_loss"], out["val_mlm_acc"] = loss / rows, correct / rows
        loss, correct, rows = 0.0, 0, 0
        for b in batches:
            st = drv._step_for("sap", False, b)
            st.run_eager(backward=False)
            labels = st.inp["labels"]
            loss += F.cross_entropy(st.logits, labels, reduction="sum").data.item()
            correct += torch.sum(torch.argmax(st.logits, 1) == labels).item()
            rows += len(labels)
        out["val_sap_gloss"], out["val_sap_gacc"] = loss / rows, correct / rows
        last["torch"] = out

    native()
    torch_route()
    for k, v in last["torch"].items():
        w = last["native"][k]
        assert abs(v - w) <= (2.0 / B if k.endswith("acc") else 1e-4 * abs(v)), (k, v, w)      # two separate bf16 forwards
    masked = [int((b["txt_labels"] != -1).sum()) for b in batches]
    info = {"batches_per_task": n_batches, "B": B, "L": LT, "T": T, "V": VIEWS, "G": int(batches[0]["gmap_step_ids"].shape[1]),
            "dtype": "bf16", "masked_rows": masked, "vocab": cfg.vocab_size,
            "result": {k: v for k, v in last["native"].items() if not k.endswith("tok_per_s")}}
    return {"native": native, "torch": torch_route}, info, drv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/validate_bench.py measures on the GPU; there is none here")
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
              "unit": "us per call, host clock, the timed window ends in a device synchronise; median / min / max over the rounds"}
    legs, info = tail_legs()
    result["tail"] = dict(info, iters=a.iters * 10, **legs_stats(legs, a.rounds, a.iters * 10))
    result["tail"]["speedup"] = round(result["tail"]["torch"]["median_us"] / result["tail"]["native"]["median_us"], 2)
    legs, info, drv = validate_legs(a.batches)
    result["validate"] = dict(info, iters=max(1, a.iters // 5), **legs_stats(legs, a.rounds, max(1, a.iters // 5)))
    result["validate"]["speedup"] = round(result["validate"]["torch"]["median_us"] / result["validate"]["native"]["median_us"], 3)
    drv.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
