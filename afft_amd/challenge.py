"""GPU side of the reference's ``challenge.marginalize_verb_noun`` (challenge.py:196-210): action logits -> softmax ->
verb and noun scores by the class-mapping matrices, as one row-softmax kernel and two exact-fp32 MFMA GEMMs on tensors
that are already on the device (the reference does this in numpy on host copies), followed by the reference's accuracy
bookkeeping (top-1 / top-5 / mean top-5 recall per verb, noun and action: challenge.py:94-106,161-193, common/utils.py:19-56)
on ONE host copy of the three score matrices.  Pinned by tests/golden/m0_marginalize.npz, produced by the reference's own
``marginalize_verb_noun`` on a stub dataset object.

The second half of the reference's file (challenge.py:243-434) follows below: late fusion of several runs' stored logits and the
EPIC-KITCHENS-100 ``test.json`` / ``submit.zip``.  Its one hot spot, the 100 best of 3806 action scores per segment, is
``ops.topk_rows`` (afft_topk_rows, include/afft_hip.h); a combination of complete runs is one ``ops.weighted_sum_fwd`` per space.
Pinned by tests/golden/s0_submission.npz, produced by the reference's own ``get_struct_outputs_per_dataset``."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from . import ops


def marginalize_scores(res_action: torch.Tensor, class_mappings: Dict[Tuple[str, str], torch.Tensor], to_prob: bool = True):
    """res_action fp32 [N, A] action logits (or probabilities if to_prob=False); class_mappings[('verb','action')] fp32
    [A, V], [('noun','action')] fp32 [A, Nn] (datasets/epic_kitchens.py).  Returns [verb [N,V], noun [N,Nn], action]:
    like the reference, the ACTION scores returned are the inputs themselves, not the probabilities."""
    x = res_action.reshape(-1, res_action.shape[-1])
    x = x if x.dtype == torch.float32 else x.float()
    x = x if x.stride(-1) == 1 else x.contiguous()
    probs = x
    if to_prob:
        probs = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
        ops.softmax_rows(x, probs)
    out = []
    for key in (("verb", "action"), ("noun", "action")):
        m = class_mappings[key].to(device=x.device, dtype=torch.float32)
        y = torch.empty(x.shape[0], m.shape[1], dtype=torch.float32, device=x.device)
        ops.gemm(probs, m, y)      # fp32 operands -> exact v_mfma_f32_32x32x2_f32 path
        out.append(y)
    return [out[0], out[1], res_action]


def group_of_from_mapping(M) -> torch.Tensor:
    """int64 [A] group (verb, noun) of every action class from a one-hot [A, G] class mapping (the dataset's
    class_mappings[('verb', 'action')], as marginalize_scores takes it): the column of the row's non-zero entry; a row that is all zero
    gives -1 (the class is in no group); a row with more than one non-zero entry is no partition and raises ValueError.  The form
    common.runner.MarginalCrossEntropy and ops.group_csr take."""
    M = torch.as_tensor(M)
    if M.dim() != 2:
        raise ValueError(f"group_of_from_mapping: a class mapping is a matrix [A, G], got {tuple(M.shape)}")
    hot = M != 0
    per_row = hot.sum(1)
    if bool((per_row > 1).any()):
        row = int(torch.nonzero(per_row > 1)[0])
        raise ValueError(f"group_of_from_mapping: class {row} maps to {int(per_row[row])} groups; a marginal needs at most one")
    return torch.where(per_row == 1, hot.to(torch.int64).argmax(1), -1)


EPIC100_VERSION = 0.2       # datasets/epic_kitchens.py: the dataset object's `version` for EPIC-KITCHENS-100


def topk_accuracy(scores: np.ndarray, labels: np.ndarray, ks, selected_class=None):
    """common/utils.py:19-42: share of rows whose label is among the k best scores.  Ties rank as in the reference's
    `scores.argsort()[:, ::-1]`: among equal scores the HIGHER class index comes first."""
    if selected_class is not None:
        keep = labels == selected_class
        scores, labels = scores[keep], labels[keep]
    kmax = int(max(ks))
    order = np.argsort(scores, axis=1, kind="stable")[:, ::-1][:, :kmax]
    hit = order == labels.reshape(-1, 1)
    return [hit[:, :k].any(axis=1).mean() for k in ks]


def topk_recall(scores: np.ndarray, labels: np.ndarray, k: int = 5, classes=None):
    """common/utils.py:45-56: mean over the classes present in `labels` of their top-k accuracy"""
    present = np.unique(labels)
    classes = present if classes is None else np.intersect1d(classes, present)
    return sum(topk_accuracy(scores, labels, ks=(k,), selected_class=c)[0] for c in classes) / len(classes)


def compute_accuracy(predictions: np.ndarray, labels: np.ndarray, classes=None):
    """challenge.py:94-106: (top-1, top-5, mean top-5 recall) in percent; classes: optional {name: class id} subset"""
    if classes is not None:
        classes = list(classes.values())
    top1, top5 = topk_accuracy(predictions, labels, ks=(1, 5))
    return top1 * 100, top5 * 100, topk_recall(predictions, labels, k=5, classes=classes) * 100


def device_accuracy(scores: torch.Tensor, labels: torch.Tensor, classes=None):
    """compute_accuracy for score matrices that are on the device (evaluate.py keeps them there): (top-1, top-5, mean top-5 recall)
    in percent from ops.label_rank + ops.recall_accumulate; what reaches the host is the two accuracies and the 2 x C integer
    counters, never the (N, C) scores.  scores fp32 [N, C] with unit column stride, labels [N] integer; classes: optional
    {name: class id} subset (many-shot / tail classes) the recall mean is restricted to.  Ties rank as include/afft_hip.h says
    (the lower class index first); on tie-free scores the three numbers are compute_accuracy's."""
    scores = scores if scores.dtype == torch.float32 else scores.float()
    scores = scores if scores.stride(-1) == 1 else scores.contiguous()
    N, C = scores.shape
    k = min(5, C)
    rank = torch.empty(N, dtype=torch.int32, device=scores.device)
    lab = torch.empty(N, dtype=torch.int64, device=scores.device)
    acc = torch.empty(2, dtype=torch.float32, device=scores.device)
    counters = torch.zeros(2, C, dtype=torch.int32, device=scores.device)
    ops.label_rank(scores, C, labels=labels.reshape(-1).to(device=scores.device, dtype=torch.int64).contiguous(), k=k, rank=rank,
                   label_out=lab, acc=acc)
    ops.recall_accumulate(rank, lab, k, counters[0], counters[1])
    tps, nums = counters.cpu().numpy().astype(np.float64)
    seen = nums > 0
    if classes is not None:
        subset = np.zeros(C, dtype=bool)
        subset[[int(c) for c in classes.values() if 0 <= int(c) < C]] = True
        seen &= subset
    top1, top5 = acc.tolist()
    return top1, top5, float((tps[seen] / nums[seen]).mean() * 100)


def _read_id_column(path: str) -> np.ndarray:
    """the RULSTM id tables are header-less one-column CSV files (one narration id per line)"""
    with open(path, "r", encoding="utf-8") as fh:
        return np.asarray([line.strip() for line in fh if line.strip()])


def epic100_unseen_tail_eval(probs, dataset) -> Dict[str, float]:
    """challenge.py:109-158: mean top-5 recall on the validation segments of unseen participants and on the segments whose
    verb / noun / action is a tail class.  The four id tables are read from dataset.rulstm_annotation_dir
    (validation_unseen_participants_ids.csv, validation_tail_{verbs,nouns,actions}_ids.csv) and matched against
    dataset.df.narration_id; the verb table selects rows for the verb scores, and so on; the unseen table for all three."""
    import os.path as osp  # noqa: PLC0415
    narration = np.asarray(dataset.df.narration_id.values).astype(str)
    res = {}
    tables = {"tail": {k: f"validation_tail_{k}s_ids.csv" for k in ("verb", "noun", "action")},
              "unseen": dict.fromkeys(("verb", "noun", "action"), "validation_unseen_participants_ids.csv")}
    for split, files in tables.items():
        for i, key in enumerate(("verb", "noun", "action")):
            rows = np.isin(narration, _read_id_column(osp.join(dataset.rulstm_annotation_dir, files[key])))
            labels = getattr(dataset.df, f"{key}_class").values[rows]
            res[f"{key[0]}mt5r_{split}"] = compute_accuracy(np.asarray(probs[i])[rows], labels)[2]
    return res


def compute_accuracies_epic(probs, dataset, compute_manyshot_unseen_tail: bool = False) -> Dict[str, float]:
    """challenge.py:161-193: probs = [verb, noun, action] score matrices; dataset.df carries verb_class / noun_class /
    action_class, dataset.classes_manyshot the many-shot subsets; with compute_manyshot_unseen_tail on an EPIC-100 dataset
    the unseen / tail recalls of :109-158 are added."""
    assert len(probs) == 3, 'Probs should contain probs for verb, noun and action'
    many = dataset.classes_manyshot
    res = {}
    for short, key, p in (("v", "verb", probs[0]), ("n", "noun", probs[1]), ("a", "action", probs[2])):
        labels = getattr(dataset.df, f"{key}_class").values
        p = np.asarray(p)
        res[f"{short}top1"], res[f"{short}top5"], res[f"{short}mt5r"] = compute_accuracy(p, labels)
        res[f"{short}mt5r_ms"] = float("nan")
        if key in many and compute_manyshot_unseen_tail:
            res[f"{short}mt5r_ms"] = compute_accuracy(p, labels, classes=many[key])[2]
    if compute_manyshot_unseen_tail and getattr(dataset, "version", None) == EPIC100_VERSION:
        res.update(epic100_unseen_tail_eval(probs, dataset))
    return res


GROUP_ALL, GROUP_UNSEEN, GROUP_TAIL = 0, 1, 2      # the row groups of the EPIC-KITCHENS-100 report: bit g of row_groups()[space][r]


def row_groups(dataset) -> Dict[str, np.ndarray]:
    """{'verb': uint32 [N], 'noun': ..., 'action': ...}: the membership words afft_rank_counts_groups takes, one per row of dataset.df.
    Bit GROUP_ALL is set for every row, bit GROUP_UNSEEN for the rows whose narration_id is in validation_unseen_participants_ids.csv,
    bit GROUP_TAIL for the rows in that space's validation_tail_{verb,noun,action}s_ids.csv: the files and the matching of
    epic100_unseen_tail_eval (challenge.py:109-135).  Host code only."""
    import os.path as osp  # noqa: PLC0415
    narration = np.asarray(dataset.df.narration_id.values).astype(str)

    def rows_of(name):
        return np.isin(narration, _read_id_column(osp.join(dataset.rulstm_annotation_dir, name))).astype(np.uint32)
    unseen = rows_of("validation_unseen_participants_ids.csv")
    return {key: (np.uint32(1 << GROUP_ALL) | (unseen << np.uint32(GROUP_UNSEEN))
                  | (rows_of(f"validation_tail_{key}s_ids.csv") << np.uint32(GROUP_TAIL))).astype(np.uint32)
            for key in ("verb", "noun", "action")}


def _class_subset(classes, C: int):
    """bool [C] of a {name: class id} subset (ids outside [0, C) name no class); None = every class"""
    if classes is None:
        return None
    subset = np.zeros(C, dtype=bool)
    subset[[int(c) for c in classes.values() if 0 <= int(c) < C]] = True
    return subset


def _recall_percent(tps: np.ndarray, nums: np.ndarray, subset=None) -> np.ndarray:
    """float64 [m]: the mean top-k recall in percent of m counter rows tps int [m, C] over the classes with a row (nums int [C] > 0, and in
    `subset` where given), in compute_accuracy's order of operations: the per-class shares summed in ascending class order, divided by
    their number, times 100.  NaN where no class qualifies."""
    seen = nums > 0
    if subset is not None:
        seen = seen & subset
    per_class = tps[:, seen] / nums[seen]
    n = per_class.shape[1]
    return np.asarray([sum(row.tolist()) / n * 100 if n else float('nan') for row in per_class], dtype=np.float64)


def _member_tensor(member, rows: int, dev) -> torch.Tensor:
    """membership words on the device as int32 with the bits of the uint32 (torch has no arithmetic on uint32; the kernel reads bits)"""
    if isinstance(member, torch.Tensor):
        member = member.reshape(-1)
        member = member if member.dtype in (torch.int32, torch.uint32) else member.to(torch.int32)
        member = member.to(dev).contiguous()
    else:
        member = torch.from_numpy(np.ascontiguousarray(np.asarray(member).reshape(-1).astype(np.uint32)).view(np.int32)).to(dev)
    if member.numel() != rows:
        raise ValueError(f'one membership word per row: got {member.numel()} for {rows} rows')
    return member


def device_accuracies_epic(probs, dataset, compute_manyshot_unseen_tail: bool = False) -> Dict[str, float]:
    """compute_accuracies_epic (challenge.py:161-193) for score matrices that stay on the device: probs = [verb, noun, action] as device
    tensors (or anything _on_device takes); the same dict, keys in the same order, NaN where that function has NaN.  Per space: one
    ops.label_rank, one ops.rank_counts_groups over that one rank vector, and one copy of the space's integer counters to the host
    (ngroups * (2 C + 3) int32).  With compute_manyshot_unseen_tail on a dataset of version EPIC100_VERSION the rows are counted in
    three groups (row_groups: all, unseen participants, the space's tail classes); otherwise in one, and no id table is read (the
    reference's rule, challenge.py:190).  Many-shot recall = group GROUP_ALL's counters restricted to dataset.classes_manyshot[space],
    as device_accuracy restricts them.  Every percentage is finished on the host in float64 from the integers, in compute_accuracy's
    order of operations (hits / N * 100; _recall_percent) -- not through afft_label_rank's fp32 acc.  Labels outside [0, C) are never
    a hit, stay in the accuracy denominators and out of the recalls; ties rank as include/afft_hip.h says (the lower class index
    first): on tie-free scores the dict is compute_accuracies_epic's."""
    assert len(probs) == 3, 'Probs should contain probs for verb, noun and action'
    many = dataset.classes_manyshot
    grouped = bool(compute_manyshot_unseen_tail) and getattr(dataset, "version", None) == EPIC100_VERSION
    groups = row_groups(dataset) if grouped else None
    G = 3 if grouped else 1
    res, tail, unseen = {}, {}, {}
    for short, key, p in (("v", "verb", probs[0]), ("n", "noun", probs[1]), ("a", "action", probs[2])):
        scores = _on_device(p)
        scores = scores.reshape(-1, scores.shape[-1])
        scores = scores if scores.stride(-1) == 1 else scores.contiguous()
        dev = scores.device
        N, C = scores.shape
        k = min(5, C)
        labels = getattr(dataset.df, f"{key}_class").values
        labels = torch.as_tensor(np.asarray(labels).reshape(-1).astype(np.int64)).to(dev)
        rank = torch.empty(1, N, dtype=torch.int32, device=dev)
        lab = torch.empty(N, dtype=torch.int64, device=dev)
        counters = torch.zeros(G * (2 * C + 3), dtype=torch.int32, device=dev)      # hits [G, 2] | tps [G, C] | nums [G, C] | rows [G]
        ops.label_rank(scores, C, labels=labels, k=k, rank=rank[0], label_out=lab)
        ops.rank_counts_groups(rank, lab, C, k, _member_tensor(groups[key], N, dev) if grouped else None, G, counters[:2 * G],
                               counters[2 * G:G * (2 + C)], counters[G * (2 + C):G * (2 + 2 * C)], counters[G * (2 + 2 * C):])
        back = counters.cpu().numpy().astype(np.int64)
        hits = back[:2 * G].reshape(G, 2)
        tps = back[2 * G:G * (2 + C)].reshape(G, C)
        nums = back[G * (2 + C):G * (2 + 2 * C)].reshape(G, C)
        res[f"{short}top1"], res[f"{short}top5"] = float(hits[0, 0] / N * 100), float(hits[0, 1] / N * 100)
        res[f"{short}mt5r"] = float(_recall_percent(tps[:1], nums[0])[0])
        res[f"{short}mt5r_ms"] = float("nan")
        if key in many and compute_manyshot_unseen_tail:
            res[f"{short}mt5r_ms"] = float(_recall_percent(tps[:1], nums[0], _class_subset(many[key], C))[0])
        if grouped:
            tail[f"{short}mt5r_tail"] = float(_recall_percent(tps[GROUP_TAIL:GROUP_TAIL + 1], nums[GROUP_TAIL])[0])
            unseen[f"{short}mt5r_unseen"] = float(_recall_percent(tps[GROUP_UNSEEN:GROUP_UNSEEN + 1], nums[GROUP_UNSEEN])[0])
    res.update(tail)
    res.update(unseen)
    return res


def marginalize_verb_noun(res_action, dataset, to_prob: bool = True, compute_manyshot_unseen_tail: bool = False,
                          device_metrics: bool = False):
    """challenge.py:196-210 with the same signature and return value: (accuracies, [verb, noun, action] as numpy arrays).
    res_action: action logits, a device tensor (kept on the device for the softmax and the two mapping GEMMs) or anything
    torch.as_tensor accepts (moved to cuda:0).  device_metrics=True: the accuracies come from device_accuracies_epic on the three
    matrices while they are on the device, in place of compute_accuracies_epic's sorts of their host copies; the scores returned are
    the same."""
    x = torch.as_tensor(res_action)
    if not x.is_cuda:
        x = x.cuda()
    verb, noun, action = marginalize_scores(x.float(), dataset.class_mappings, to_prob=to_prob)
    on_device = (verb, noun, action.reshape(-1, action.shape[-1]))
    accuracies = device_accuracies_epic(on_device, dataset, compute_manyshot_unseen_tail) if device_metrics else None
    scores = [t.detach().cpu().numpy() for t in on_device]
    if accuracies is None:
        accuracies = compute_accuracies_epic(scores, dataset, compute_manyshot_unseen_tail)
    return accuracies, scores


LOGITS_DIR = 'logits'        # challenge.py:28
PREFIX_H5 = 'test'           # challenge.py:32


def gen_load_resfiles(resdir: str):
    """challenge.py:79-91: every '<PREFIX_H5>*h5' logits file of a run directory as {leaf key: array} (through h5py when it is
    installed, else through afft_amd.h5lite, which reads the same files)."""
    import glob  # noqa: PLC0415
    import os.path as osp  # noqa: PLC0415
    from .evaluate import load_logits  # noqa: PLC0415
    resfiles = sorted(glob.glob(osp.join(resdir, PREFIX_H5 + '*h5')))
    if len(resfiles) == 0:
        raise ValueError(f'Didnt find any resfiles in {resdir}')
    for resfile in resfiles:
        yield load_logits(resfile)


def get_epic_marginalize_verb_noun(resdir: str, dataset):
    """challenge.py:213-222: verb / noun scores from the action logits stored in a run directory."""
    res = next(gen_load_resfiles(resdir))
    res_action = None
    for key, val in res.items():
        if key.startswith('logits/action'):
            res_action = val
    assert res_action is not None, 'Can not find logits/action in h5.'
    return marginalize_verb_noun(res_action, dataset)


# ----------------------------------------------------------------------------- late fusion and the EPIC-KITCHENS-100 submission
# challenge.py:225-434.  The reference keeps the dataset object in a module global that its __main__ block sets; here every function
# takes it as the keyword `dataset` and falls back to this attribute.
dataset = None


def _dataset(ds):
    ds = ds if ds is not None else dataset
    if ds is None:
        raise ValueError('a dataset object is needed: pass dataset=..., or set afft_amd.challenge.dataset')
    return ds


def _on_device(x) -> torch.Tensor:
    """fp32 tensor on the GPU (there is no CPU path); what is there already stays where it is"""
    x = torch.as_tensor(x)
    if not x.is_cuda:
        x = x.cuda()
    return x if x.dtype == torch.float32 else x.float()


def _uids(ds, uid_key):
    return [str(u) for u in ds.df[uid_key].values]


def print_accuracies_epic(metrics: dict, prefix: str = ''):
    """challenge.py:225-240"""
    groups = [('Accuracies', ('vtop1', 'vtop5', 'ntop1', 'ntop5', 'atop1', 'atop5')), ('Mean top 5', ('vmt5r', 'nmt5r', 'amt5r')),
              ('Mean top 5 many shot', ('vmt5r_ms', 'nmt5r_ms', 'amt5r_ms'))]
    if 'vmt5r_tail' in metrics:      # the tail / unseen numbers come as one group (compute_accuracies_epic)
        groups += [('Mean top 5 tail', ('vmt5r_tail', 'nmt5r_tail', 'amt5r_tail')),
                   ('Mean top 5 unseen', ('vmt5r_unseen', 'nmt5r_unseen', 'amt5r_unseen'))]
    for title, keys in groups:
        print(f'[{prefix}] {title} verb/noun/action: ' + ' '.join(f'{metrics[k]:.1f}' for k in keys))


def top_actions(action_scores, k: int = 100):
    """(vals fp32 [N, k'], idx int32 [N, k']) as numpy arrays, k' = min(k, C): per row the k' best scores, best first, in the order
    include/afft_hip.h defines for afft_topk_rows (among equal scores the lower class first, NaN last).  The scores go to the device
    if they are not there; k' columns per row come back.  (The reference's np.argpartition(row, -100) raises for C < 100.)"""
    x = _on_device(action_scores)
    x = x.reshape(-1, x.shape[-1])
    x = x if x.stride(-1) == 1 else x.contiguous()
    vals, idx = ops.topk_rows(x, min(int(k), x.shape[1]))
    return vals.cpu().numpy(), idx.cpu().numpy()


def _concat_with_uids(scores, dataset, uid_key):
    """challenge.py:243-249: [verb, noun, action] matrices -> three {uid: row} dicts; row i belongs to the i-th uid of dataset.df (a
    matrix with fewer rows covers the first uids only)"""
    uids = _uids(dataset, uid_key)
    return [dict(zip(uids, per_space)) for per_space in scores]


def _normalize_scores(scores, p):
    """challenge.py:252-260: every row divided by its p-norm + 0.000001"""
    return [{uid: row / (np.linalg.norm(row, ord=p, axis=-1) + 0.000001) for uid, row in per_space.items()} for per_space in scores]


def contains_list_or_tuple(items) -> bool:
    return any(isinstance(el, (list, tuple)) for el in items)


def read_all_single_models(resdirs, uid_key='narration_id', normalize_before_combine=None, dataset=None):
    """challenge.py:271-284: per run directory the three {uid: row} dicts of its verb / noun / action scores"""
    ds = _dataset(dataset)
    all_scores = []
    for resdir in resdirs:
        accuracies, scores = get_epic_marginalize_verb_noun(resdir, ds)
        scores = _concat_with_uids(scores, ds, uid_key)
        print_accuracies_epic(accuracies, prefix=resdir)
        if normalize_before_combine is not None:      # AVT does not normalise
            scores = _normalize_scores(scores, p=normalize_before_combine)
        all_scores.append(scores)
    return all_scores


MAX_DEVICE_RUNS = 8      # afft_weighted_sum_fwd adds up to 8 matrices (include/afft_hip.h)


def _combine_on_device(per_run, uids, weight):
    """sum_i weight[i] * run_i for runs that all cover `uids`: one ops.weighted_sum_fwd over the [N, C] matrices"""
    xs = [_on_device(np.stack([run[u] for u in uids])) for run in per_run]
    w = torch.tensor([[float(x) for x in weight]], dtype=torch.float32).repeat(len(uids), 1).to(xs[0].device)
    out = torch.empty_like(xs[0])
    ops.weighted_sum_fwd(xs, w, out)
    return dict(zip(uids, out.cpu().numpy()))


def _combine_per_uid(per_run, weight):
    """the reference's union: every uid any run has, summed over the runs that have it (in the order of their first appearance)"""
    combined = {}
    for uid in dict.fromkeys(u for run in per_run for u in run):
        parts = [run[uid] * weight[i] for i, run in enumerate(per_run) if uid in run]
        combined[uid] = np.sum(np.stack(parts), axis=0)
    return combined


def get_epic_marginalize_late_fuse(resdirs, weights=1.0, mp_best_weights=None, n_best=5, uid_key='narration_id', dataset=None):
    """challenge.py:287-351: weighted sum of the verb / noun / action scores of several runs.  weights: one float (every run), one
    weight per run, or a list of such lists (each is combined and scored; the last one's combination is returned).  mp_best_weights
    (optional list, updated in place) keeps the n_best (amt5r, weights) pairs seen, ascending.  Returns (accuracies, combined,
    dataset) with combined = three {uid: row} dicts.  When every run covers all rows of dataset.df and there are at most
    MAX_DEVICE_RUNS of them, a space is combined by one ops.weighted_sum_fwd on the device; otherwise per uid in numpy."""
    ds = _dataset(dataset)
    if not isinstance(resdirs, list):
        resdirs = [resdirs]
    if isinstance(weights, float):
        weights = [[weights] * len(resdirs)]
    elif not isinstance(weights, np.ndarray) and not contains_list_or_tuple(weights):
        assert len(weights) == len(resdirs)
        weights = [weights]
    else:
        assert all(len(weight) == len(resdirs) for weight in weights)
    mp_best_weights = [] if mp_best_weights is None else mp_best_weights
    all_scores = read_all_single_models(resdirs, uid_key=uid_key, dataset=ds)
    uids = _uids(ds, uid_key)
    full = len(resdirs) <= MAX_DEVICE_RUNS and all(len(per_space) == len(uids) for run in all_scores for per_space in run)
    accuracies, combined = None, None
    for weight in weights:
        combined = []
        for space in range(3):      # verb / noun / action
            per_run = [run[space] for run in all_scores]
            combined.append(_combine_on_device(per_run, uids, weight) if full else _combine_per_uid(per_run, weight))
        # the accuracies need matrices again, in the order of the annotations
        accuracies = compute_accuracies_epic([np.array([per_space[u] for u in uids]) for per_space in combined], ds)
        print_accuracies_epic(accuracies, prefix=f'combined with {weight}')
        metric = accuracies['amt5r']
        if len(mp_best_weights) == 0 or metric > mp_best_weights[0][0]:
            at = sum(1 for m, _ in mp_best_weights if m <= metric)
            mp_best_weights.insert(at, (metric, weight))
            if len(mp_best_weights) > n_best:
                mp_best_weights.pop(0)
    return accuracies, combined, ds


def device_sweep(xs, labels, weights, k=5, classes=None, sets_per_call=512, member=None, ngroups=1):
    """compute_accuracy of sum_i weights[j, i] * xs[i] for every weight set j, without any of the sums being formed: three float64
    vectors of length nsets, (top-1, top-k, mean top-k recall) in percent.  xs: R <= MAX_DEVICE_RUNS score matrices [N, C] of one space
    (arrays or device tensors; they go to the device once), labels [N] integer, weights [nsets, R].  Per chunk of sets_per_call sets:
    one ops.fused_label_rank (the label's rank under every set of the chunk, counted while the runs' rows stream past), one
    ops.rank_counts_sets, and one copy of the chunk's integer counters (2 hits and C true positives per set) to the host; the C class
    counts come back once.  Nothing of width N * C leaves the device.  The numbers follow from the integer counts in float64, in the
    order of operations of compute_accuracy: hits / N * 100, and the recall mean summed in ascending class order over the classes with
    a row (restricted to `classes`, a {name: class id} subset, when given).  Labels outside [0, C) are never a hit, stay in the accuracy
    denominators and out of the recall (device_accuracy's rule).  Ties rank as include/afft_hip.h says (the lower class index first); on
    tie-free scores the three numbers are compute_accuracy's of the materialised combination, bit for bit.

    ROW GROUPS.  With member (uint32 [N], bit g = row r is in group g < ngroups <= 8: row_groups) the chunk's counting launch is
    ops.rank_counts_groups and the return value is FOUR float64 arrays of shape [nsets, ngroups], (top-1, top-k, recall, recall_in_classes):
    column g holds the numbers of the rows of group g alone -- the accuracies over that group's rows (NaN for a group without rows), the
    recall over the classes with a row in the group.  `classes` does not narrow the third array there: the fourth is the recall narrowed
    to `classes` (NaN throughout without `classes`), so that one pass yields both the overall and the many-shot recall of the
    EPIC-KITCHENS-100 report.  Without member (and ngroups = 1) the call sequence and the three vectors are as described above."""
    grouped = member is not None
    if not grouped and ngroups != 1:
        raise ValueError(f'device_sweep: ngroups = {ngroups} needs the membership words (member)')
    xs = [_on_device(x) for x in xs]
    xs = [x.reshape(-1, x.shape[-1]) for x in xs]
    if not 1 <= len(xs) <= MAX_DEVICE_RUNS:
        raise ValueError(f'device_sweep takes 1 to {MAX_DEVICE_RUNS} runs, got {len(xs)}')
    if any(x.shape != xs[0].shape for x in xs):
        raise ValueError(f'every run must cover the same rows and classes, got {[tuple(x.shape) for x in xs]}')
    if any(x.stride(-1) != 1 or x.stride(0) != xs[0].stride(0) for x in xs):
        xs = [x.contiguous() for x in xs]
    dev = xs[0].device
    N, C = xs[0].shape
    k = min(int(k), C)
    w = torch.as_tensor(np.asarray(weights, dtype=np.float32).reshape(-1, len(xs))).to(dev)
    nsets = w.shape[0]
    lab = torch.as_tensor(np.asarray(labels).reshape(-1).astype(np.int64)).to(dev) if not isinstance(labels, torch.Tensor) \
        else labels.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    per_call = max(1, min(int(sets_per_call), nsets))
    rank = torch.empty(per_call, N, dtype=torch.int32, device=dev)
    if grouped:
        return _grouped_sweep(xs, w, lab, rank, k, _class_subset(classes, C), _member_tensor(member, N, dev), int(ngroups))
    hits = np.empty((nsets, 2), np.int64)
    tps = np.empty((nsets, C), np.int64)
    nums = None
    for at in range(0, nsets, per_call):
        m = min(per_call, nsets - at)
        counters = torch.zeros(m * (2 + C) + C, dtype=torch.int32, device=dev)      # hits [m, 2] | tps [m, C] | nums [C]
        ops.fused_label_rank(xs, w[at:at + m], lab, rank=rank[:m])
        ops.rank_counts_sets(rank[:m], lab, C, k, counters[:2 * m], counters[2 * m:m * (2 + C)], counters[m * (2 + C):])
        back = (counters if nums is None else counters[:m * (2 + C)]).cpu().numpy()
        hits[at:at + m] = back[:2 * m].reshape(m, 2)
        tps[at:at + m] = back[2 * m:m * (2 + C)].reshape(m, C)
        if nums is None:
            nums = back[m * (2 + C):].astype(np.int64)
    seen = nums > 0
    if classes is not None:
        subset = np.zeros(C, dtype=bool)
        subset[[int(c) for c in classes.values() if 0 <= int(c) < C]] = True
        seen &= subset
    top1 = hits[:, 0] / N * 100
    topk = hits[:, 1] / N * 100
    per_class = tps[:, seen] / nums[seen]
    recall = np.asarray([sum(row.tolist()) / per_class.shape[1] * 100 if per_class.shape[1] else float('nan') for row in per_class])
    return top1, topk, recall


def _grouped_sweep(xs, w, lab, rank, k, subset, member, G):
    """device_sweep's loop with the counters kept per row group: per chunk one ops.fused_label_rank, one ops.rank_counts_groups and one
    copy of hits [m, G, 2] | tps [m, G, C]; nums [G, C] | group rows [G] come back with the first chunk only"""
    dev = xs[0].device
    N, C = xs[0].shape
    nsets, per_call = w.shape[0], rank.shape[0]
    hits = np.empty((nsets, G, 2), np.int64)
    tps = np.empty((nsets, G, C), np.int64)
    nums = group_rows = None
    for at in range(0, nsets, per_call):
        m = min(per_call, nsets - at)
        per_set = m * G * (2 + C)
        counters = torch.zeros(per_set + G * (C + 1), dtype=torch.int32, device=dev)
        ops.fused_label_rank(xs, w[at:at + m], lab, rank=rank[:m])
        ops.rank_counts_groups(rank[:m], lab, C, k, member, G, counters[:2 * m * G], counters[2 * m * G:per_set],
                               counters[per_set:per_set + G * C], counters[per_set + G * C:])
        back = (counters if nums is None else counters[:per_set]).cpu().numpy()
        hits[at:at + m] = back[:2 * m * G].reshape(m, G, 2)
        tps[at:at + m] = back[2 * m * G:per_set].reshape(m, G, C)
        if nums is None:
            nums = back[per_set:per_set + G * C].reshape(G, C).astype(np.int64)
            group_rows = back[per_set + G * C:].astype(np.int64)
    out = [np.full((nsets, G), np.nan, dtype=np.float64) for _ in range(4)]
    for g in range(G):
        if group_rows[g]:
            out[0][:, g] = hits[:, g, 0] / group_rows[g] * 100
            out[1][:, g] = hits[:, g, 1] / group_rows[g] * 100
        out[2][:, g] = _recall_percent(tps[:, g], nums[g])
        if subset is not None:
            out[3][:, g] = _recall_percent(tps[:, g], nums[g], subset)
    return tuple(out)


def late_fuse_sweep(resdirs, weights, mp_best_weights=None, n_best=5, uid_key='narration_id', dataset=None,
                    compute_manyshot_unseen_tail=False):
    """The weight search of challenge.py:287-351 (get_epic_marginalize_late_fuse over a list of weight combinations, which the reference
    runs under multiprocessing) with every combination scored on the device by device_sweep: one call per space (verb, noun, action),
    no combination is materialised, and what comes back per combination is integer counters.  resdirs are read as
    get_epic_marginalize_late_fuse reads them and weights takes the same forms under the same assertions.  Every run must cover all rows of
    dataset.df and there may be at most MAX_DEVICE_RUNS of them: otherwise ValueError (get_epic_marginalize_late_fuse handles those, on
    the host).  Returns a list with one accuracies dict per weight combination: the keys of compute_accuracies_epic without the many-shot
    option (the *_ms entries are NaN).  mp_best_weights (optional list, updated in place) keeps the n_best (amt5r, weights) pairs seen,
    ascending, by the rule of get_epic_marginalize_late_fuse.  Ties rank as include/afft_hip.h says (the lower class index first); on
    tie-free scores every number is the one get_epic_marginalize_late_fuse reports for that combination.
    compute_manyshot_unseen_tail=True: every dict is compute_accuracies_epic(combination, dataset, True)'s instead -- the *_ms entries
    from dataset.classes_manyshot and, on a dataset of version EPIC100_VERSION, the *_tail and *_unseen recalls of row_groups' groups.
    Each chunk still makes one ops.fused_label_rank per space; its counting launch is ops.rank_counts_groups (device_sweep with member)."""
    ds = _dataset(dataset)
    if not isinstance(resdirs, list):
        resdirs = [resdirs]
    if isinstance(weights, float):
        weights = [[weights] * len(resdirs)]
    elif not isinstance(weights, np.ndarray) and not contains_list_or_tuple(weights):
        assert len(weights) == len(resdirs)
        weights = [weights]
    else:
        assert all(len(weight) == len(resdirs) for weight in weights)
    if len(resdirs) > MAX_DEVICE_RUNS:
        raise ValueError(f'late_fuse_sweep combines at most {MAX_DEVICE_RUNS} runs on the device, got {len(resdirs)}: use '
                         f'get_epic_marginalize_late_fuse')
    mp_best_weights = [] if mp_best_weights is None else mp_best_weights
    all_scores = read_all_single_models(resdirs, uid_key=uid_key, dataset=ds)
    uids = _uids(ds, uid_key)
    if not all(len(per_space) == len(uids) for run in all_scores for per_space in run):
        raise ValueError('late_fuse_sweep needs complete runs (every run covering all rows of dataset.df): use '
                         'get_epic_marginalize_late_fuse, which sums such runs per uid')
    table = np.asarray([[float(x) for x in weight] for weight in weights], dtype=np.float32)
    results = [{} for _ in weights]
    report = bool(compute_manyshot_unseen_tail)
    grouped = report and getattr(ds, 'version', None) == EPIC100_VERSION      # the rule of compute_accuracies_epic (challenge.py:190)
    groups = row_groups(ds) if grouped else None
    tails, unseens = [{} for _ in weights], [{} for _ in weights]
    for space, (short, key) in enumerate((('v', 'verb'), ('n', 'noun'), ('a', 'action'))):
        xs = [np.stack([run[space][u] for u in uids]) for run in all_scores]
        labels = getattr(ds.df, f'{key}_class').values
        if not report:
            top1, top5, mt5r = device_sweep(xs, labels, table)
            for j, res in enumerate(results):
                res[f'{short}top1'], res[f'{short}top5'], res[f'{short}mt5r'] = float(top1[j]), float(top5[j]), float(mt5r[j])
                res[f'{short}mt5r_ms'] = float('nan')
            continue
        member = groups[key] if grouped else np.full(len(uids), 1 << GROUP_ALL, dtype=np.uint32)
        top1, top5, mt5r, ms = device_sweep(xs, labels, table, classes=ds.classes_manyshot.get(key), member=member,
                                            ngroups=3 if grouped else 1)
        for j, res in enumerate(results):
            res[f'{short}top1'], res[f'{short}top5'] = float(top1[j, GROUP_ALL]), float(top5[j, GROUP_ALL])
            res[f'{short}mt5r'], res[f'{short}mt5r_ms'] = float(mt5r[j, GROUP_ALL]), float(ms[j, GROUP_ALL])
            if grouped:
                tails[j][f'{short}mt5r_tail'] = float(mt5r[j, GROUP_TAIL])
                unseens[j][f'{short}mt5r_unseen'] = float(mt5r[j, GROUP_UNSEEN])
    for res, tail, unseen in zip(results, tails, unseens):      # compute_accuracies_epic's key order: the tail numbers, then the unseen ones
        res.update(tail)
        res.update(unseen)
    for weight, accuracies in zip(weights, results):
        metric = accuracies['amt5r']
        if len(mp_best_weights) == 0 or metric > mp_best_weights[0][0]:
            at = sum(1 for m, _ in mp_best_weights if m <= metric)
            mp_best_weights.insert(at, (metric, weight))
            if len(mp_best_weights) > n_best:
                mp_best_weights.pop(0)
    return results


def struct_outputs_from_scores(scores, dataset, uid_key='narration_id', k=100, uids=None):
    """The `results` dict of challenge.py:358-377 from scores = [verb, noun, action], arrays or device tensors whose rows follow
    dataset.df (or `uids`, where given).  Per uid: 'verb' / 'noun' {str(class): score} over every class; 'action' {"verb,noun": score}
    for the k best actions, inserted best first (top_actions: of the action matrix only k columns per row leave the device).  Every
    value is a Python float."""
    uids = _uids(dataset, uid_key) if uids is None else list(uids)
    to_verb_noun = {action: pair for pair, action in dataset.verb_noun_to_action.items()}
    verb, noun = (s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else np.asarray(s) for s in scores[:2])
    vals, idx = top_actions(scores[2], k)
    assert len(verb) == len(noun) == len(vals) == len(uids), 'one row per uid in each space'
    names = {}      # class -> "verb,noun", built for the classes that occur
    results = {}
    for r, uid in enumerate(uids):
        action = {}
        for j, v in zip(idx[r].tolist(), vals[r].tolist()):
            if j not in names:
                names[j] = ','.join(str(el) for el in to_verb_noun[j])
            action[names[j]] = v
        results[uid] = {'verb': {str(j): v for j, v in enumerate(verb[r].tolist())},
                        'noun': {str(j): v for j, v in enumerate(noun[r].tolist())},
                        'action': action}
    return results


def get_struct_outputs_per_dataset(resdirs, weights, uid_key='narration_id', dataset=None):
    """challenge.py:354-398: the submission structure {'version', 'challenge', 'results'}.  results is keyed in dataset.df order (the
    uids that have scores), then the rows of dataset.discarded_df that are not yet present, with zero scores for every verb and noun
    class and for the actions '0,0' .. '0,99'."""
    _, combined, ds = get_epic_marginalize_late_fuse(resdirs, weights, uid_key=uid_key, dataset=dataset)
    uids = [u for u in dict.fromkeys(_uids(ds, uid_key)) if u in combined[0]]
    results = struct_outputs_from_scores([np.stack([per_space[u] for u in uids]) for per_space in combined], ds, uid_key=uid_key,
                                         uids=uids)
    if ds.discarded_df is not None:
        for _, row in ds.discarded_df.iterrows():
            uid = str(row[uid_key])
            if uid in results:
                continue
            results[uid] = {'verb': {str(j): 0.0 for j in range(len(ds.verb_classes))},
                            'noun': {str(j): 0.0 for j in range(len(ds.noun_classes))},
                            'action': {f'0,{j}': 0.0 for j in range(100)}}
    return {'version': f'{ds.version}', 'challenge': ds.challenge_type, 'results': results}


def package_results_for_submission_ek100(resdirs, weights, sls=(1, 4, 3), dataset=None, output_dir=None):
    """challenge.py:401-414: <output_dir>/test.json and <output_dir>/submit.zip (test.json at its top level); sls = the supervision
    levels (pretraining, training labels, training data) the challenge asks for.  output_dir defaults to LOGITS_DIR.  Returns the dict."""
    import json  # noqa: PLC0415
    import os  # noqa: PLC0415
    import zipfile  # noqa: PLC0415
    res = get_struct_outputs_per_dataset(resdirs, weights, uid_key='narration_id', dataset=dataset)
    res['sls_pt'], res['sls_tl'], res['sls_td'] = sls[0], sls[1], sls[2]
    output_dir = LOGITS_DIR if output_dir is None else output_dir
    print(f'Saving outputs to {output_dir}')
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, 'test.json')
    with open(path, 'w') as fout:
        json.dump(res, fout, indent=4)      # every value is a Python number already: no numpy encoder
    with zipfile.ZipFile(os.path.join(output_dir, 'submit.zip'), 'w', zipfile.ZIP_DEFLATED) as z:
        z.write(path, arcname='test.json')
    return res


def generate_test_json(args, dataset=None):
    """challenge.py:417-428: args.models = run directories under LOGITS_DIR, args.weights = one weight per model"""
    import os  # noqa: PLC0415
    models = args.models if isinstance(args.models, list) else [args.models]
    weights = args.weights if isinstance(args.weights, list) else [args.weights]
    return package_results_for_submission_ek100([os.path.join(LOGITS_DIR, m) for m in models], [float(w) for w in weights],
                                                dataset=dataset)


def parse_args(argv=None):
    import argparse  # noqa: PLC0415
    parser = argparse.ArgumentParser(description='EPIC-KITCHENS-100 test.json / submit.zip from stored logits')
    parser.add_argument('--prefix_h5', type=str, default='test', choices=['test', 'val'], help='Prefix of h5 file to be selected')
    parser.add_argument('--models', type=str, nargs='+', required=True, help='List of models to be selected')
    parser.add_argument('--weights', type=str, nargs='+', required=True, help='List of weights for selected models')
    return parser.parse_args(argv)


if __name__ == '__main__':
    from afft_amd import _hydra_compat  # noqa: PLC0415
    _args = parse_args()
    PREFIX_H5 = _args.prefix_h5
    _get_dataset = getattr(_hydra_compat, 'get_dataset', None)
    if _get_dataset is None:
        raise SystemExit('afft_amd.challenge: no dataset loader here. Build the dataset object (datasets/epic_kitchens.py of the '
                         'reference) and call generate_test_json(args, dataset=...) or package_results_for_submission_ek100(...).')
    generate_test_json(_args, dataset=_get_dataset())
