"""float64 restatement, in torch on the CPU, of the marginal cross-entropy over class groups of csrc/loss.hip (afft_softmax_ce_groups;
the formulas of include/afft_hip.h), with the magnitude sums its tests scale their tolerances by.

x: a row of logits, lse = logsumexp(x), p = softmax(x); group_of[c] in [0, G) or -1 (no group); lse_g = logsumexp over the classes of
group g (no value for an empty group); q_c = exp(x_c - lse_g(c)), 0 for an ungrouped class.
  hard label y:   t_g = [g == y]
  soft target t:  as given
  T = sum_g t_g,  loss = T lse - sum_{g: t_g != 0} t_g lse_g,  dloss/dx_c = T p_c - t_g(c) q_c
Ignored rows (label -1, keep == 0): loss 0, gradient 0.  Bad rows -- a label outside [-1, G), a label that names an empty group, a soft
target with t_g != 0 on an empty group --: NaN loss and gradient in that row.

Magnitude sums (the absolute values of the terms each result adds up):
  s_loss = |T lse| + sum_g |t_g lse_g|                  the loss is a difference of these
  s_grad = |gscale row_g| sum_g |t_g|                   per row: the scale of T p_c and of t_g q_c (p_c, q_c <= 1), the one
                                                        tests/ce_double.py uses for the sibling (|gscale row_g| A)
"""
import torch

F64 = torch.float64


def group_lse(x, group_of, G):
    """lse_g [rows, G] float64 (NaN for an empty group) and the mask [G] of the empty groups"""
    rows = x.shape[0]
    out = torch.full((rows, G), float("nan"), dtype=F64)
    empty = torch.ones(G, dtype=torch.bool)
    for g in torch.unique(group_of[group_of >= 0]).tolist():
        out[:, g] = torch.logsumexp(x[:, group_of == g], 1)
        empty[g] = False
    return out, empty


def groups(x, group_of, G, *, glabels=None, gsoft=None, keep=None, gscale=1.0, row_g=None):
    """x [rows, C] (any float type, taken to float64), group_of int [C].  Returns a dict of float64 tensors: loss [rows], grad
    [rows, C] (= gscale * row_g * dloss/dx), s_loss [rows], s_grad [rows], T [rows], t [rows, G], and the boolean rows `kept`, `bad`."""
    assert (glabels is None) != (gsoft is None)
    x = x.to(F64)
    rows, C = x.shape
    group_of = group_of.to(torch.int64)
    assert group_of.shape == (C,) and int(group_of.min()) >= -1 and int(group_of.max()) < G
    lse_g, empty = group_lse(x, group_of, G)
    kept = torch.ones(rows, dtype=torch.bool)
    if glabels is not None:
        kept = glabels != -1
        inside = (glabels >= 0) & (glabels < G)
        t = torch.zeros(rows, G, dtype=F64)
        idx = torch.nonzero(inside).reshape(-1)
        t[idx, glabels[idx]] = 1.0
        bad = (glabels >= G) | (glabels < -1)
    else:
        t = gsoft.to(F64).clone()
        bad = torch.zeros(rows, dtype=torch.bool)
    if keep is not None:
        kept = kept & (keep != 0)
    bad = (bad | ((t != 0) & empty[None, :]).any(1)) & kept
    t = t * kept[:, None]
    T = t.sum(1)
    lse = torch.logsumexp(x, 1)
    p = torch.softmax(x, 1)
    tl = torch.where(t != 0, t * lse_g, torch.zeros((), dtype=F64))      # groups with t_g == 0 take no part, empty or not
    grouped = group_of >= 0
    gi = group_of.clamp(min=0)
    tc = torch.where(grouped[None, :], t[:, gi], torch.zeros((), dtype=F64))
    q = torch.where(tc != 0, torch.exp(x - lse_g[:, gi]), torch.zeros((), dtype=F64))
    g = torch.full((rows,), float(gscale), dtype=F64)
    if row_g is not None:
        g = g * row_g.to(F64)
    loss = T * lse - tl.sum(1)
    grad = g[:, None] * (T[:, None] * p - tc * q)
    s_loss = (T * lse).abs() + tl.abs().sum(1)
    s_grad = g.abs() * t.abs().sum(1)
    for v in (loss, grad, s_loss, s_grad):
        v[~kept] = 0.0
    loss[bad] = float("nan")
    grad[bad] = float("nan")
    return dict(loss=loss, grad=grad, s_loss=s_loss, s_grad=s_grad, T=T, t=t, kept=kept, bad=bad)
