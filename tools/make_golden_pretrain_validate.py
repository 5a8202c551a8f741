"""Write tests/golden/pretrain_validate_small.npz from the REAL pre-training model (needs the reference tree).

    python tools/make_golden_pretrain_validate.py

GlocalTextPathCMTPreTraining (through oracle/ref_pretrain_harness.py, eval() mode) runs the statements of validate_mlm /
validate_sap (pretrain_src/pretrain_src/train_r2r.py:355-380, :416-444) over two batches per task: oracle.make_golden_pretrain's
make_case() and a second seed (tests/eval_ref.py::val_case).  Labels do not enter the forward, and with random weights no prediction
would be right, so on a copy of each batch every second masked row's label is replaced by the model's own arg-max and the SAP
labels become [arg-max, 0, 5] -- the accuracy is then neither 0 nor 1.  The file holds data only: the scores, the edited labels,
per-batch loss sums and counts, and the final dicts without the time field.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_pretrain_harness as rp      # noqa: E402
from tests import eval_ref as ev                   # noqa: E402


@torch.no_grad()
def main():
    cfg, P, batches = ev.val_case()
    model = rp.build_pretrain_model(cfg, P)
    model.eval()
    z = {}
    # validate_mlm (:355-380)
    val_loss, n_correct, n_word = 0, 0, 0
    for i, batch in enumerate(batches):
        rb = rp.to_ref_batch(batch)
        scores = model(rb, task="mlm", compute_loss=False)
        labels = batch["txt_labels"]
        labels = labels[labels != -1].clone()
        labels[::2] = scores.max(dim=-1)[1][::2]
        loss = F.cross_entropy(scores, labels, reduction="sum")
        val_loss += loss.item()
        c = (scores.max(dim=-1)[1] == labels).sum().item()
        n_correct += c
        n_word += labels.numel()
        z[f"mlm/scores/{i}"] = scores.numpy().astype(np.float32)
        z[f"mlm/labels/{i}"] = labels.numpy().astype(np.int64)
        z[f"mlm/loss_sum/{i}"] = np.float64(loss.item())
        z[f"mlm/n_correct/{i}"] = np.int64(c)
        z[f"mlm/n_word/{i}"] = np.int64(labels.numel())
        print("mlm batch", i, "rows", labels.numel(), "loss sum", loss.item(), "correct", c, "top-2 margin", ev.top2_margin(scores))
    z["mlm/loss"] = np.float64(val_loss / n_word)
    z["mlm/acc"] = np.float64(n_correct / n_word)
    # validate_sap (:416-444)
    val_gloss, n_gcorrect, n_data = 0, 0, 0
    for i, batch in enumerate(batches):
        rb = rp.to_ref_batch(batch)
        global_logits, _ = model(rb, task="sap", compute_loss=False)
        am = torch.argmax(global_logits, 1)
        labels = torch.tensor([int(am[0]), 0, 5][:am.numel()], dtype=torch.int64)
        assert bool(torch.isfinite(global_logits[torch.arange(labels.numel()), labels]).all()), "an edited label sits on a masked node"
        loss = F.cross_entropy(global_logits, labels, reduction="sum").data.item()
        val_gloss += loss
        c = torch.sum(torch.argmax(global_logits, 1) == labels).item()
        n_gcorrect += c
        n_data += len(labels)
        z[f"sap/logits/{i}"] = global_logits.numpy().astype(np.float32)
        z[f"sap/labels/{i}"] = labels.numpy()
        z[f"sap/loss_sum/{i}"] = np.float64(loss)
        z[f"sap/n_correct/{i}"] = np.int64(c)
        z[f"sap/n_data/{i}"] = np.int64(len(labels))
        fin = torch.where(torch.isfinite(global_logits), global_logits, torch.full_like(global_logits, -1e30))
        print("sap batch", i, "rows", len(labels), "loss sum", loss, "correct", c, "top-2 margin", ev.top2_margin(fin))
    z["sap/gloss"] = np.float64(val_gloss / n_data)
    z["sap/gacc"] = np.float64(n_gcorrect / n_data)
    np.savez_compressed(ev.GOLDEN, **z)
    print("wrote", ev.GOLDEN, os.path.getsize(ev.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
