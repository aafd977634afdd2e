"""float64 restatement, in torch on the CPU, of the weighted / label-smoothed softmax cross-entropy of csrc/loss.hip
(afft_softmax_ce_w; the formulas of include/afft_hip.h), with the magnitude sums its tests scale their tolerances by.

x: a row of logits, lse = logsumexp(x), p = softmax(x); w: the class weights (ones when absent); eps: the smoothing.
  hard label y != -1:  a_c = (eps / C) w_c + (1 - eps) w_y [c == y]
  soft target t:       a_c = w_c ((1 - eps) t_c + eps / C)
  A = sum_c a_c,  loss = lse A - sum_c a_c x_c,  dloss/dx_j = p_j A - a_j
Ignored rows (label -1, keep == 0): loss 0, gradient 0.  A label outside [-1, C): NaN loss and gradient in that row.
"""
import torch

F64 = torch.float64


def coefficients(C, *, labels=None, soft=None, weight=None, eps=0.0):
    """a [rows, C] float64; rows with a label of -1 or out of range get zeros (ce() overrides them)"""
    w = torch.ones(C, dtype=F64) if weight is None else weight.to(F64)
    if soft is not None:
        return w[None, :] * ((1.0 - eps) * soft.to(F64) + eps / C)
    rows = labels.numel()
    a = (eps / C) * w[None, :].repeat(rows, 1)
    ok = (labels >= 0) & (labels < C)
    idx = torch.nonzero(ok).reshape(-1)
    a[idx, labels[idx]] += (1.0 - eps) * w[labels[idx]]
    a[~ok] = 0.0
    return a


def ce(x, *, labels=None, soft=None, keep=None, weight=None, eps=0.0, gscale=1.0, row_g=None):
    """x [rows, C] (any float type, taken to float64).  Returns a dict of float64 tensors:
    loss [rows], grad [rows, C] (= gscale * row_g * dloss/dx), s_loss [rows] = |lse| A + sum_c a_c |x_c|, s_grad [rows] =
    |gscale * row_g| A, A [rows], and the boolean rows `kept` and `bad`."""
    assert (labels is None) != (soft is None)
    x = x.to(F64)
    rows, C = x.shape
    a = coefficients(C, labels=labels, soft=soft, weight=weight, eps=eps)
    kept = torch.ones(rows, dtype=torch.bool)
    bad = torch.zeros(rows, dtype=torch.bool)
    if labels is not None:
        kept = labels != -1
        bad = (labels >= C) | (labels < -1)
    if keep is not None:
        kept = kept & (keep != 0)
    bad = bad & kept
    a = a * kept[:, None]
    A = a.sum(1)
    lse = torch.logsumexp(x, 1)
    p = torch.softmax(x, 1)
    g = torch.full((rows,), float(gscale), dtype=F64)
    if row_g is not None:
        g = g * row_g.to(F64)
    loss = lse * A - (a * x).sum(1)
    grad = g[:, None] * (p * A[:, None] - a)
    loss[~kept] = 0.0
    grad[~kept] = 0.0
    loss[bad] = float("nan")
    grad[bad] = float("nan")
    return dict(loss=loss, grad=grad, s_loss=lse.abs() * A + (a * x.abs()).sum(1), s_grad=g.abs() * A, A=A, kept=kept, bad=bad)


def torch_reference(x, *, labels=None, soft=None, keep=None, weight=None, eps=0.0):
    """the same loss and its gradient by torch.nn.functional.cross_entropy in float64 (reduction='none', ignore_index=-1; rows with
    keep == 0 are dropped before the call, as the reference's criterion drops them, and come back as zeros).  Labels must be in range."""
    x = x.to(F64).clone().requires_grad_(True)
    w = None if weight is None else weight.to(F64)
    rows = x.shape[0]
    sel = torch.arange(rows) if keep is None else torch.nonzero(keep != 0).reshape(-1)
    tgt = labels[sel] if labels is not None else soft.to(F64)[sel]
    part = torch.nn.functional.cross_entropy(x[sel], tgt, weight=w, ignore_index=-1, reduction='none', label_smoothing=eps)
    loss = torch.zeros(rows, dtype=F64).index_add(0, sel, part)
    grad, = torch.autograd.grad(loss.sum(), x)
    return loss.detach(), grad
