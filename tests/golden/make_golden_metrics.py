"""Generate tests/golden/k0_metrics.npz by running the REFERENCE's metric code (build container only).

    python tests/golden/make_golden_metrics.py

Imports the reference the way make_golden.py does (same stubs) and feeds closed-form logits and labels through
  * common.utils.accuracy                                   (hard labels: acc1 / acc5),
  * BasicLossAccuracy.forward_future_action, MixUp branch   (soft targets built by common.mixup._mix_labels: adjusted logits,
                                                             labels, acc1 / acc5),
  * MeanTopKRecallMeter.update, twice (the two halves of the batch), and once per row for the per-row hit `tp`.
Every input is tie-free, and each condition is asserted below: all scores of a row distinct; the two largest target values
distinct from each other and from the rest; after the MixUp adjustment no score equal to the label's.  On such rows "the label is
among the k largest" has one meaning, so the reference alone decides every stored value.  Nothing of the reference (source,
bytecode, pickles) is written: the .npz holds numeric arrays only.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

B, C, LAM, SMOOTH = 48, 211, 0.3, 0.1


def inputs():
    from closed_form import _hash_uniform
    logits = (8.0 * _hash_uniform(B * C, 0x4D7A)).astype(np.float32).reshape(B, C)
    labels = (np.arange(B, dtype=np.int64) * 37 + 11) % C
    labels[0], labels[1] = 0, C - 1                      # both ends of the row
    labels[40:44] = labels[40]                           # a class with several rows
    partner = labels[::-1]                               # MixUp pairs sample r with sample B - 1 - r
    for r in range(B):
        # hard labels: the label's logit goes midway between two neighbours of the sorted rest, so that its rank is r % 9 (both
        # sides of the top-5 boundary); MixUp: the partner's logit is set so that the folded score x[i1] + x[i2] has rank (r // 2) % 8
        rest = np.sort(np.delete(logits[r], [labels[r], partner[r]]))[::-1]
        j = r % 9
        logits[r, labels[r]] = rest[0] + 0.5 if j == 0 else 0.5 * (rest[j - 1] + rest[j])
        rest = np.sort(np.append(np.delete(logits[r], [labels[r], partner[r]]), np.float32(0.0)))[::-1]      # s[i2] = 0 takes part
        j = (r // 2) % 8
        folded = rest[0] + 0.25 if j == 0 else 0.5 * (rest[j - 1] + rest[j])
        logits[r, partner[r]] = folded - logits[r, labels[r]]
    return logits, labels


def main():
    import make_golden
    make_golden.install_stubs()
    from common import utils
    from common.metric_tracking import MeanTopKRecallMeter
    from common.mixup import _mix_labels
    from common.runner import BasicLossAccuracy

    logits, labels = inputs()
    assert LAM != 0.5 and (labels != labels[::-1]).all(), "paired samples need different labels"
    for r in range(B):
        assert len(np.unique(logits[r])) == C, f"row {r}: equal scores"
    out = {"logits": logits, "labels": labels}

    def meter_run(scores, lab, tag):
        m = MeanTopKRecallMeter("mt5r_action", C)
        m.reset()
        m.update({"logits": scores[:B // 2], "labels": lab[:B // 2]})
        m.update({"logits": scores[B // 2:], "labels": lab[B // 2:]})
        tp = np.zeros(B, dtype=np.int64)
        for r in range(B):
            one = MeanTopKRecallMeter("row", C)
            one.reset()
            one.update({"logits": scores[r:r + 1], "labels": lab[r:r + 1]})
            tp[r] = int(one.tps.sum())
        assert tp.sum() == m.tps.sum() and m.nums.sum() == B
        out.update({f"{tag}_tp": tp, f"{tag}_tps": m.tps.astype(np.int64), f"{tag}_nums": m.nums.astype(np.int64),
                    f"{tag}_value": np.asarray(float(m.value), dtype=np.float64)})
        return tp

    # ---- hard labels
    acc1, acc5 = utils.accuracy(torch.from_numpy(logits)[:, None, :], torch.from_numpy(labels)[:, None], topk=(1, 5))
    out["hard_acc1"], out["hard_acc5"] = np.asarray(float(acc1), np.float32), np.asarray(float(acc5), np.float32)
    tp = meter_run(logits, labels, "hard")
    assert abs(float(acc5) - 100.0 * tp.mean()) < 1e-4

    # ---- soft targets (MixUp)
    soft = _mix_labels(torch.from_numpy(labels), C, LAM, SMOOTH).to(torch.float32)
    top3 = torch.topk(soft, 3, dim=1).values
    assert bool((top3[:, 0] > top3[:, 1]).all()) and bool((top3[:, 1] > top3[:, 2]).all()), "top-2 targets must stand alone"
    losses, metrics = {}, {}
    BasicLossAccuracy().forward_future_action(torch.from_numpy(logits)[:, None, :].clone(), soft, True, losses, metrics,
                                              "acc1", "acc5", "mt5r", "cls")
    adj, lab = metrics["mt5r"]["logits"], metrics["mt5r"]["labels"]
    for r in range(B):
        assert (np.delete(adj[r], lab[r]) != adj[r, lab[r]]).all(), f"row {r}: a score equals the label's after the adjustment"
    out.update({"soft": soft.numpy(), "soft_labels": lab.astype(np.int64),
                "soft_acc1": np.asarray(float(metrics["acc1"]), np.float32), "soft_acc5": np.asarray(float(metrics["acc5"]), np.float32)})
    tp = meter_run(adj, lab, "soft")
    assert abs(float(metrics["acc5"]) - 100.0 * tp.mean()) < 1e-4
    out["meta"] = np.asarray(json.dumps(dict(case="k0_metrics", B=B, C=C, lam=LAM, label_smoothing=SMOOTH, torch=torch.__version__,
                                             numpy=np.__version__, reference="zeyun-zhong/AFFT (v1)")))
    path = os.path.join(HERE, "k0_metrics.npz")
    np.savez_compressed(path, **out)
    print("[k0_metrics]", {k: (v.tolist() if v.ndim == 0 else v.shape) for k, v in out.items() if k != "meta"}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
