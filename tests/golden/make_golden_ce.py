"""Generate tests/golden/c0_weighted_ce.npz by running the REFERENCE's criterion (build container only).

    python tests/golden/make_golden_ce.py

Imports the reference's common.runner.MultiDimCrossEntropy on the CPU (with make_golden.py's stubs for the packages the image lacks)
and evaluates it in float64 on float32 inputs: class weights only, label smoothing only, both -- on hard labels (some -1) and on soft
targets with an ignore mask.  Stored: the inputs, the per-row losses (soft: scattered back to all rows, ignored rows 0 -- the
reference returns the kept rows only) and the gradient of their sum with respect to the logits.  Numeric arrays and a JSON 'meta'
only; nothing of the reference is written.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

B, T, C, EPS = 6, 4, 13, 0.1
VARIANTS = {"w": (True, 0.0), "s": (False, EPS), "ws": (True, EPS)}      # name -> (weights, smoothing)


def inputs():
    g = torch.Generator().manual_seed(20260)
    logits = (torch.randn(B, T, C, generator=g) * 2.5).float()
    labels = torch.randint(0, C, (B, T), generator=g)
    weight = (torch.rand(C, generator=g) * 2.0 + 0.25).float()
    weight[4] = 0.0
    labels[0, 1] = labels[3, 3] = labels[5, 0] = -1
    labels[1, 2] = labels[4, 1] = 4                          # rows whose own class has weight 0
    # soft targets as MixUp makes them: two classes share the mass
    lam = torch.rand(B, T, generator=g).float()
    c0, c1 = torch.randint(0, C, (B, T), generator=g), torch.randint(0, C, (B, T), generator=g)
    c0[2, 2] = c1[2, 2] = 4                                  # all of this row's mass on the class of weight 0
    soft = torch.zeros(B, T, C)
    soft.scatter_add_(2, c0[..., None], lam[..., None])
    soft.scatter_add_(2, c1[..., None], (1.0 - lam)[..., None])
    ignore = torch.zeros(B, T, dtype=torch.bool)
    ignore[0, 0] = ignore[2, 3] = ignore[5, 1] = ignore[5, 2] = True
    return logits, labels, soft.float(), ignore, weight


def main():
    from make_golden import install_stubs
    install_stubs()
    from common.runner import MultiDimCrossEntropy

    logits, labels, soft, ignore, weight = inputs()
    out = dict(logits=logits.numpy(), labels=labels.numpy(), soft=soft.numpy(), ignore=ignore.numpy(), weight=weight.numpy())
    for name, (use_w, eps) in VARIANTS.items():
        crit = MultiDimCrossEntropy(ignore_index=-1, reduction='none', weight=weight.double() if use_w else None, label_smoothing=eps)
        x = logits.double().requires_grad_(True)
        loss = crit(x, labels)
        out[f"hard_{name}_loss"] = loss.detach().numpy()
        out[f"hard_{name}_grad"] = torch.autograd.grad(loss.sum(), x)[0].numpy()
        x = logits.double().requires_grad_(True)
        kept = crit(x, soft.double(), one_hot=True, ignore_index=ignore)
        full = torch.zeros(B * T, dtype=torch.float64).index_add(0, torch.nonzero(~ignore.reshape(-1)).reshape(-1), kept)
        out[f"soft_{name}_loss"] = full.detach().numpy()
        out[f"soft_{name}_grad"] = torch.autograd.grad(kept.sum(), x)[0].numpy()
    for k, v in out.items():
        assert v.dtype in (np.float32, np.float64, np.int64, np.bool_), (k, v.dtype)
    meta = dict(case="c0_weighted_ce", B=B, T=T, C=C, eps=EPS, variants={k: dict(weight=w, smoothing=e) for k, (w, e) in VARIANTS.items()},
                criterion="common.runner.MultiDimCrossEntropy(ignore_index=-1, reduction='none', weight=, label_smoothing=), float64",
                loss="per row, (B*T,); soft: ignored rows 0", grad="d sum(loss) / d logits, (B, T, C)", torch=torch.__version__,
                numpy=np.__version__)
    np.savez_compressed(os.path.join(HERE, "c0_weighted_ce.npz"), **out, meta=np.asarray(json.dumps(meta)))
    print("wrote c0_weighted_ce.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
