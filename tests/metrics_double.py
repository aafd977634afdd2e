"""TEST DOUBLE of ops.label_rank / ops.recall_accumulate -- test infrastructure, never part of the product.

Plain-torch restatements of the two contracts in include/afft_hip.h (rank of the label's score, lower class index wins a tie, labels
outside [0, C) rank C and are left out of the counters), so that the HOST logic around them -- afft_amd.common.metric_tracking, the
Runner switch, install_as_models -- runs in the build container on CPU tensors, the way tests/cpu_ops.py stands in for the rest of
afft_amd.ops.  The kernels themselves are tested on the GPU only (tests/test_metrics_gpu.py).
"""
import contextlib

import numpy as np
import torch


def _argmax_low(t):
    """per-row arg-max, the lowest index among equal values"""
    C = t.shape[1]
    idx = torch.arange(C).expand_as(t)
    return torch.where(t == t.max(dim=1, keepdim=True).values, idx, C).min(dim=1).values


def label_rank(logits, C_, *, labels=None, soft=None, k, rank, label_out, acc=None):
    assert (labels is None) != (soft is None) and 1 <= k <= C_
    rows = logits.shape[0]
    x = logits[:, :C_].detach().clone()
    r = torch.arange(rows)
    if soft is not None:
        t = soft[:, :C_].detach().clone()
        lab = _argmax_low(t)
        if C_ > 1:
            t[r, lab] = float("-inf")
            i2 = _argmax_low(t)
            x[r, lab] += x[r, i2]
            x[r, i2] = 0.0
    else:
        lab = labels.reshape(-1).to(torch.int64)
    valid = (lab >= 0) & (lab < C_)
    safe = lab.clamp(0, C_ - 1)
    sl = x[r, safe].unsqueeze(1)
    idx = torch.arange(C_).unsqueeze(0)
    ahead = ((x > sl) | ((x == sl) & (idx < safe.unsqueeze(1)))) & (idx != safe.unsqueeze(1))
    rank.copy_(torch.where(valid, ahead.sum(1), C_).to(torch.int32))
    label_out.copy_(lab)
    if acc is not None:
        scale = torch.tensor(np.float32(100.0 / rows))
        acc[0] = (rank < 1).sum().to(torch.float32) * scale
        acc[1] = (rank < k).sum().to(torch.float32) * scale
    return rank, label_out


def recall_accumulate(rank, label, k, tps, nums):
    C_ = tps.numel()
    keep = (label >= 0) & (label < C_)
    lab = label[keep]
    nums += torch.bincount(lab, minlength=C_).to(torch.int32)
    tps += torch.bincount(lab[rank[keep] < k], minlength=C_).to(torch.int32)


@contextlib.contextmanager
def installed():
    """ops.label_rank / ops.recall_accumulate become the restatements above for the duration of the block"""
    from afft_amd import ops
    saved = (ops.label_rank, ops.recall_accumulate)
    ops.label_rank, ops.recall_accumulate = label_rank, recall_accumulate
    try:
        yield
    finally:
        ops.label_rank, ops.recall_accumulate = saved
