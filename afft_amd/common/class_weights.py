"""Class weights for the weighted cross-entropy (MultiDimCrossEntropy(weight=...), Runner(cls_weight=...)) from per-class sample
counts, and the logit adjustment (MultiDimCrossEntropy(logit_adjust=...), Runner(logit_adjust=...)) from the same counts.  Host
arithmetic only."""
from __future__ import annotations

import numpy as np


def class_weights(counts, scheme: str = 'inverse', power: float = 1.0, beta: float = 0.999) -> np.ndarray:
    """counts: [C] non-negative sample counts per class.  Returns float64 [C]:

      'inverse'    w_c = counts_c ** -power                       (power = 1: inverse frequency, 0.5: inverse square root, 0: all ones)
      'effective'  w_c = (1 - beta) / (1 - beta ** counts_c)      (the inverse "effective number of samples", 0 <= beta < 1)

    A class without samples gets weight 0 (it never appears as a label; with label smoothing it takes no mass either).  The result
    is scaled so that the count-weighted mean weight is 1, sum(counts * w) / sum(counts) == 1: the mean loss over a training set
    drawn with these counts keeps its scale, and the learning rate its meaning."""
    n = np.asarray(counts, dtype=np.float64).reshape(-1)
    if n.size == 0 or not np.all(np.isfinite(n)) or np.any(n < 0):
        raise ValueError("class_weights: counts must be finite and non-negative, one per class")
    seen = n > 0
    if not seen.any():
        raise ValueError("class_weights: every count is 0")
    w = np.zeros_like(n)
    if scheme == 'inverse':
        w[seen] = n[seen] ** -float(power)
    elif scheme == 'effective':
        if not 0.0 <= beta < 1.0:
            raise ValueError(f"class_weights: beta must lie in [0, 1), got {beta}")
        w[seen] = (1.0 - beta) / -np.expm1(n[seen] * np.log(beta)) if beta > 0 else 1.0
    else:
        raise ValueError(f"class_weights: unknown scheme {scheme!r} ('inverse' or 'effective')")
    return w * (n.sum() / np.dot(n, w))


def logit_adjustment(counts, tau: float = 1.0) -> np.ndarray:
    """counts: [C] non-negative sample counts per class.  Returns float32 [C]: tau * log(counts_c / sum(counts)), the logit adjustment
    of Menon et al. 2021 (tau = 1: "balanced softmax") for MultiDimCrossEntropy(logit_adjust=...) / Runner(logit_adjust={type: ...}).

    A class without samples takes the smallest positive count present: log 0 would be -inf, and the kernel wants finite entries;
    such a class is then treated as the rarest class seen (the total in the denominator stays the true sum of the counts)."""
    n = np.asarray(counts, dtype=np.float64).reshape(-1)
    if n.size == 0 or not np.all(np.isfinite(n)) or np.any(n < 0):
        raise ValueError("logit_adjustment: counts must be finite and non-negative, one per class")
    if not np.isfinite(tau):
        raise ValueError(f"logit_adjustment: tau must be finite, got {tau}")
    seen = n > 0
    if not seen.any():
        raise ValueError("logit_adjustment: every count is 0")
    filled = np.where(seen, n, n[seen].min())
    return (float(tau) * np.log(filled / n.sum())).astype(np.float32)
