"""TEST DOUBLE of afft_amd.ops.softmax_ce_groups / softmax_ce_frames_groups, on top of tests/cpu_ops.py (which stays as it is): the
float64 restatement of tests/groups_double.py behind the wrappers' signatures.  `installed()` swaps the two in together with every
double of cpu_ops and yields the list of calls made: (name, (logits, C, groups), keywords)."""
from __future__ import annotations

import contextlib

import torch

import cpu_ops
import groups_double

CALLS = []


def _run(name, logits2, C_, groups, kw, d2):
    group_of, members, offs = groups
    assert group_of.dtype == members.dtype == offs.dtype == torch.int32 and group_of.numel() == C_
    G = offs.numel() - 1
    gsoft = kw.get("gsoft")
    got = groups_double.groups(logits2[:, :C_], group_of, G, glabels=kw.get("glabels"), gsoft=None if gsoft is None else gsoft[:, :G],
                               keep=kw.get("keep"), gscale=kw.get("gscale", 1.0), row_g=kw.get("row_g"))
    if kw.get("row_loss") is not None:
        kw["row_loss"].copy_(got["loss"])
    if kw.get("loss_sum") is not None:
        kw["loss_sum"] += got["loss"].sum()
    if d2 is not None:
        d2.zero_()
        d2[:, :C_].copy_(got["grad"])


@torch.no_grad()
def softmax_ce_groups(logits, C_, groups, **kw):
    CALLS.append(("softmax_ce_groups", (logits, C_, groups), kw))
    _run("softmax_ce_groups", logits, C_, groups, kw, kw.get("dlogits"))


@torch.no_grad()
def softmax_ce_frames_groups(logits3, C_, groups, **kw):
    CALLS.append(("softmax_ce_frames_groups", (logits3, C_, groups), kw))
    clips, frames = logits3.shape[:2]
    d3 = kw.get("dlogits3")
    d2 = None if d3 is None else torch.zeros(clips * frames, d3.shape[2])
    _run("softmax_ce_frames_groups", logits3.reshape(clips * frames, -1), C_, groups, kw, d2)
    if d3 is not None:
        d3.copy_(d2.view(clips, frames, -1))


@contextlib.contextmanager
def installed():
    from afft_amd import ops
    saved = ops.softmax_ce_groups, ops.softmax_ce_frames_groups
    del CALLS[:]
    with cpu_ops.installed():
        ops.softmax_ce_groups, ops.softmax_ce_frames_groups = softmax_ce_groups, softmax_ce_frames_groups
        try:
            yield CALLS
        finally:
            ops.softmax_ce_groups, ops.softmax_ce_frames_groups = saved
