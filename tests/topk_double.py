"""TEST DOUBLE of ops.topk_rows -- test infrastructure, never part of the product.

A numpy restatement of the ORDER that include/afft_hip.h defines for afft_topk_rows, in float64 / int64 and sharing no code with the
kernel: one stable sort per row on (NaN last, value descending with -0.0 == +0.0, class ascending).  The GPU test compares the kernel
with `topk` below; `installed()` puts a wrapper of it in place of ops.topk_rows, a numpy sum in place of ops.weighted_sum_fwd and a
pass-through in place of challenge._on_device (the product moves scores to the GPU there and has no CPU path), so that the HOST logic
of afft_amd.challenge -- late fusion, the submission structure, test.json / submit.zip -- runs in the build container on CPU tensors,
the way tests/metrics_double.py stands in for the metric kernels.
"""
import contextlib

import numpy as np
import torch


def order(row):
    """int64 [C]: the classes of one row, best first"""
    with np.errstate(invalid="ignore"):         # a signalling NaN among the inputs: the cast quiets it, which is all that is needed
        v = np.asarray(row, dtype=np.float64)
    nan = np.isnan(v)
    key = np.where(nan, 0.0, -v) + 0.0          # ascending -v = descending v; -0.0 + 0.0 = +0.0, and 0.0 == -0.0 compares equal anyway
    # np.lexsort: the LAST key is the primary one; it is stable, so equal (nan, key) pairs stay in class order
    return np.lexsort((np.arange(len(v)), key, nan)).astype(np.int64)


def topk(x, k):
    """x [rows, C] -> (vals [rows, k] in x's dtype, gathered and never recomputed, idx int64 [rows, k])"""
    x = np.asarray(x)
    idx = np.stack([order(r)[:k] for r in x]) if len(x) else np.zeros((0, k), np.int64)
    return np.take_along_axis(x, idx, axis=1), idx


def topk_rows(x, k, vals=None, idx=None):
    """ops.topk_rows on CPU tensors, with its refusals"""
    if x.dtype != torch.float32:
        raise TypeError(f"topk_rows takes fp32 scores, got {x.dtype}")
    if x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError("x must be a 2-D tensor with unit column stride")
    rows, C = x.shape
    if not (rows >= 1 and 1 <= k <= C <= 8192):
        raise RuntimeError(f"topk_rows: 1 <= k <= C <= 8192 (got k = {k}, C = {C})")
    v, i = topk(x.detach().numpy(), k)
    vals = torch.empty(rows, k, dtype=torch.float32) if vals is None else vals
    idx = torch.empty(rows, k, dtype=torch.int32) if idx is None else idx
    vals[:, :k] = torch.from_numpy(np.ascontiguousarray(v))
    idx[:, :k] = torch.from_numpy(i.astype(np.int32))
    return vals, idx


def weighted_sum_fwd(xs, w, out):
    """out[r, :] = sum_i w[r, i] * xs[i][r, :], products and sum in fp32 like the kernel's"""
    acc = np.zeros(tuple(out.shape), np.float32)
    for i, x in enumerate(xs):
        acc += w[:, i:i + 1].numpy().astype(np.float32) * x.numpy().astype(np.float32)
    out.copy_(torch.from_numpy(acc))
    return out


@contextlib.contextmanager
def installed():
    """ops.topk_rows / ops.weighted_sum_fwd become the restatements above and challenge keeps its tensors on the CPU for the duration
    of the block"""
    from afft_amd import challenge, ops
    saved = (ops.topk_rows, ops.weighted_sum_fwd, challenge._on_device)
    ops.topk_rows, ops.weighted_sum_fwd = topk_rows, weighted_sum_fwd
    challenge._on_device = lambda x: torch.as_tensor(x).float()
    try:
        yield
    finally:
        ops.topk_rows, ops.weighted_sum_fwd, challenge._on_device = saved
