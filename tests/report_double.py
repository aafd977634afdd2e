"""TEST DOUBLE of ops.rank_counts_groups and of the report built from its counters -- test infrastructure, never part of the product.

An integer restatement in numpy of the four counters of afft_rank_counts_groups (include/afft_hip.h), one row at a time and sharing no
code with the kernel or with afft_amd.challenge, and a float64 restatement of the EPIC-KITCHENS-100 report dict that
challenge.device_accuracies_epic finishes from them (challenge.py:94-193 of the reference: hits / N * 100; the recall as the per-class
shares summed in ascending class order over the classes with a row, divided by their number, times 100).  `label_ranks` gives the rank
vector of one score matrix under the header's comparator.  The GPU test compares the kernel with `counts`; `installed()` puts wrappers
in place of ops.rank_counts_groups / ops.label_rank on top of sweep_double.installed(), so that the HOST logic of the report and of the
grouped sweep runs in the build container on CPU tensors.
"""
import contextlib

import numpy as np
import torch

import metrics_double
import sweep_double


def label_ranks(scores, labels):
    """int64 [rows]: #{c != l : s[c] > s[l] or (s[c] == s[l] and c < l)}; C for a label outside [0, C)"""
    scores = np.asarray(scores)
    rows, C = scores.shape
    out = np.empty(rows, np.int64)
    classes = np.arange(C)
    for r, l in enumerate(np.asarray(labels, np.int64).tolist()):
        if not 0 <= l < C:
            out[r] = C
            continue
        v, sl = scores[r], scores[r, l]
        out[r] = int(((classes != l) & ((v > sl) | ((v == sl) & (classes < l)))).sum())
    return out


def counts(rank, labels, member, ngroups, C, k):
    """(hits int64 [nsets, G, 2], tps int64 [nsets, G, C], nums int64 [G, C], group_rows int64 [G]) of rank [nsets, rows];
    member None = every row in group 0"""
    rank = np.asarray(rank, np.int64)
    nsets, rows = rank.shape
    labels = np.asarray(labels, np.int64).tolist()
    words = [1] * rows if member is None else [int(m) & 0xFFFFFFFF for m in np.asarray(member).tolist()]
    hits = np.zeros((nsets, ngroups, 2), np.int64)
    tps = np.zeros((nsets, ngroups, C), np.int64)
    nums = np.zeros((ngroups, C), np.int64)
    group_rows = np.zeros(ngroups, np.int64)
    for r in range(rows):
        for g in range(ngroups):
            if not (words[r] >> g) & 1:
                continue
            group_rows[g] += 1
            inside = 0 <= labels[r] < C
            if inside:
                nums[g, labels[r]] += 1
            for j in range(nsets):
                hits[j, g, 0] += int(rank[j, r] < 1)
                hits[j, g, 1] += int(rank[j, r] < k)
                if inside and rank[j, r] < k:
                    tps[j, g, labels[r]] += 1
    return hits, tps, nums, group_rows


def recall(tps, nums, subset=None):
    """float64: mean over the classes with a row (and in `subset`, an iterable of class ids) of tps / nums, in percent; NaN without one"""
    classes = [c for c in range(len(nums)) if nums[c] > 0 and (subset is None or c in subset)]
    if not classes:
        return float("nan")
    total = 0
    for c in classes:
        total = total + np.float64(tps[c]) / np.float64(nums[c])
    return float(total / len(classes) * 100)


def accuracies(per_space, manyshot, report, grouped):
    """the dict of compute_accuracies_epic from per_space = {'verb' | 'noun' | 'action': (N, hits [G, 2], tps [G, C], nums [G, C])}
    (one set's counters); report = compute_manyshot_unseen_tail, grouped = report on an EPIC-100 dataset (groups: all, unseen, tail)"""
    res, tail, unseen = {}, {}, {}
    for short, key in (("v", "verb"), ("n", "noun"), ("a", "action")):
        N, hits, tps, nums = per_space[key]
        res[f"{short}top1"] = float(np.float64(hits[0][0]) / N * 100)
        res[f"{short}top5"] = float(np.float64(hits[0][1]) / N * 100)
        res[f"{short}mt5r"] = recall(tps[0], nums[0])
        res[f"{short}mt5r_ms"] = float("nan")
        if report and key in manyshot:
            res[f"{short}mt5r_ms"] = recall(tps[0], nums[0], {int(c) for c in manyshot[key].values()})
        if grouped:
            unseen[f"{short}mt5r_unseen"] = recall(tps[1], nums[1])
            tail[f"{short}mt5r_tail"] = recall(tps[2], nums[2])
    res.update(tail)
    res.update(unseen)
    return res


def rank_counts_groups(rank, labels, C, k, member, ngroups, hits, tps, nums, group_rows):
    """ops.rank_counts_groups on CPU tensors, with its refusals: the four buffers are ADDED to"""
    nsets, rows = rank.shape
    assert rank.dtype == torch.int32 and labels.dtype == torch.int64 and labels.numel() == rows
    assert hits.dtype == tps.dtype == nums.dtype == group_rows.dtype == torch.int32
    if not (1 <= ngroups <= 8) or (member is None and ngroups != 1):
        raise RuntimeError(f"rank_counts_groups: 1 <= ngroups <= 8, null member with one group only (got {ngroups})")
    if not (rows >= 1 and C >= 1 and 1 <= k <= C and nsets >= 1):
        raise RuntimeError(f"rank_counts_groups: bad sizes (rows = {rows}, C = {C}, k = {k}, nsets = {nsets})")
    assert member is None or (member.dtype in (torch.int32, torch.uint32) and member.numel() == rows)
    assert hits.numel() == 2 * nsets * ngroups and tps.numel() == nsets * ngroups * C and nums.numel() == ngroups * C
    assert group_rows.numel() == ngroups
    words = None if member is None else member.numpy().view(np.uint32)
    for buf, add in zip((hits, tps, nums, group_rows), counts(rank.numpy(), labels.numpy(), words, ngroups, C, k)):
        buf += torch.from_numpy(add.astype(np.int32)).reshape(buf.shape)


@contextlib.contextmanager
def installed():
    """ops.rank_counts_groups becomes the restatement above and ops.label_rank the one of tests/metrics_double.py, on top of
    sweep_double.installed() (the sweep's two ops, ops.topk_rows, ops.weighted_sum_fwd; challenge keeps its tensors on the CPU)"""
    from afft_amd import ops
    with sweep_double.installed():
        saved = (ops.rank_counts_groups, ops.label_rank)
        ops.rank_counts_groups, ops.label_rank = rank_counts_groups, metrics_double.label_rank
        try:
            yield
        finally:
            ops.rank_counts_groups, ops.label_rank = saved
