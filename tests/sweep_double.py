"""TEST DOUBLE of ops.fused_label_rank / ops.rank_counts_sets -- test infrastructure, never part of the product.

A numpy restatement of the two contracts in include/afft_hip.h that shares no code with the kernels: the combination of one weight set
as fp32 products and fp32 sums in run order (each rounded on its own: where the kernel's fused multiply-add rounds once the two differ
by an ulp at most, so a test that compares with the kernel on arbitrary scores either uses exactly representable products and sums or
asserts a margin first), then the comparator `c != l and (v > sl or (v == sl and c < l))` spelled out per row.  The GPU test compares
the kernels with `label_ranks` / `counts` below; `installed()` puts wrappers of them in place of the two ops and enters
topk_double.installed(), so that the HOST logic of afft_amd.challenge.device_sweep / late_fuse_sweep runs in the build container on CPU
tensors.
"""
import contextlib

import numpy as np
import torch

import topk_double


def combine(xs, wj):
    """fp32 [rows, C]: s = 0, then s = fl(s + fl(wj[i] * xs[i])) for the runs in order"""
    s = np.zeros(np.asarray(xs[0]).shape, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, x in enumerate(xs):
            s = (s + np.float32(wj[i]) * np.asarray(x, np.float32)).astype(np.float32)
    return s


def label_ranks(xs, w, labels):
    """int64 [nsets, rows]: the rank of labels[r] in row r of every combination; C for a label outside [0, C)"""
    w = np.asarray(w, np.float32)
    labels = np.asarray(labels, np.int64)
    rows, C = np.asarray(xs[0]).shape
    out = np.empty((w.shape[0], rows), np.int64)
    classes = np.arange(C)
    for j in range(w.shape[0]):
        s = combine(xs, w[j])
        for r in range(rows):
            l = int(labels[r])
            if not 0 <= l < C:
                out[j, r] = C
                continue
            v, sl = s[r], s[r, l]
            with np.errstate(invalid="ignore"):
                ahead = (classes != l) & ((v > sl) | ((v == sl) & (classes < l)))
            out[j, r] = int(ahead.sum())
    return out


def counts(rank, labels, C, k):
    """(hits int64 [nsets, 2], tps int64 [nsets, C], nums int64 [C]) of rank [nsets, rows]"""
    rank = np.asarray(rank, np.int64)
    labels = np.asarray(labels, np.int64)
    nsets = rank.shape[0]
    hits = np.stack([(rank < 1).sum(axis=1), (rank < k).sum(axis=1)], axis=1).astype(np.int64)
    tps = np.zeros((nsets, C), np.int64)
    nums = np.zeros(C, np.int64)
    for r, l in enumerate(labels.tolist()):
        if 0 <= l < C:
            nums[l] += 1
            for j in range(nsets):
                tps[j, l] += int(rank[j, r] < k)
    return hits, tps, nums


def fused_label_rank(xs, w, labels, rank=None):
    """ops.fused_label_rank on CPU tensors, with its refusals"""
    rows, C = xs[0].shape
    if any(x.dim() != 2 or (C > 1 and x.stride(1) != 1) for x in xs):
        raise ValueError("x must be a 2-D tensor with unit column stride")
    assert all(x.shape == xs[0].shape and x.dtype == torch.float32 for x in xs)
    if any(x.stride(0) != xs[0].stride(0) for x in xs):
        raise RuntimeError("fused_label_rank: every run must have the row stride of the first")
    nsets = w.shape[0]
    assert w.dtype == torch.float32 and w.shape[1] == len(xs)
    assert labels.dtype == torch.int64 and labels.numel() == rows
    if not (1 <= len(xs) <= 8 and nsets >= 1 and rows >= 1 and C >= 1):
        raise RuntimeError(f"fused_label_rank: bad sizes (n = {len(xs)}, nsets = {nsets}, rows = {rows}, C = {C})")
    rank = torch.empty(nsets, rows, dtype=torch.int32) if rank is None else rank
    assert rank.dtype == torch.int32 and tuple(rank.shape) == (nsets, rows)
    rank.copy_(torch.from_numpy(label_ranks([x.detach().numpy() for x in xs], w.numpy(), labels.numpy()).astype(np.int32)))
    return rank


def rank_counts_sets(rank, labels, C, k, hits, tps, nums):
    """ops.rank_counts_sets on CPU tensors: the three buffers are ADDED to"""
    nsets, rows = rank.shape
    assert rank.dtype == torch.int32 and labels.dtype == torch.int64 and labels.numel() == rows
    assert hits.dtype == tps.dtype == nums.dtype == torch.int32
    assert hits.numel() == 2 * nsets and tps.numel() == nsets * C and nums.numel() == C
    if not (rows >= 1 and C >= 1 and 1 <= k <= C and nsets >= 1):
        raise RuntimeError(f"rank_counts_sets: bad sizes (rows = {rows}, C = {C}, k = {k}, nsets = {nsets})")
    h, t, n = counts(rank.numpy(), labels.numpy(), C, k)
    hits += torch.from_numpy(h.astype(np.int32)).reshape(hits.shape)
    tps += torch.from_numpy(t.astype(np.int32)).reshape(tps.shape)
    nums += torch.from_numpy(n.astype(np.int32)).reshape(nums.shape)


@contextlib.contextmanager
def installed():
    """ops.fused_label_rank / ops.rank_counts_sets become the restatements above, on top of topk_double.installed() (ops.topk_rows,
    ops.weighted_sum_fwd, and challenge keeps its tensors on the CPU), for the duration of the block"""
    from afft_amd import ops
    with topk_double.installed():
        saved = (ops.fused_label_rank, ops.rank_counts_sets)
        ops.fused_label_rank, ops.rank_counts_sets = fused_label_rank, rank_counts_sets
        try:
            yield
        finally:
            ops.fused_label_rank, ops.rank_counts_sets = saved
