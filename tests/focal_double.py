"""float64 restatement, in torch on the CPU, of the focal / logit-adjusted softmax cross-entropy of csrc/loss.hip
(afft_softmax_ce_focal; the formulas of include/afft_hip.h), with the magnitude sums its tests scale their tolerances by.

x: a row of logits, b: the adjustment (zeros when absent), gamma >= 0: the focusing exponent.
  z = x + b,  m = max z,  k = the first index with z_k = m,  r = sum_{c != k} exp(z_c - m),  lse = m + log1p(r)
  class k:        p = 1 / (1 + r),            q = r / (1 + r),   l = log1p(r)
  every other c:  p = exp(z_c - m) / (1 + r), q = 1 - p (>= 1/2), l = (m - z_c) + log1p(r)
  f_c = q_c^gamma l_c,  g_c = q_c^gamma (1 + gamma p_c l_c / q_c)   (the second term 0 when q_c = 0)
  a_c: ce_double.coefficients (hard label, soft target, weights, smoothing),  A = sum_c a_c
  loss = sum_c a_c f_c,  G = sum_c a_c g_c,  dloss/dx_j = p_j G - a_j g_j;  for j = k: p_k (G - a_k g_k) - q_k a_k g_k
The arg-max is left out of r, and its own gradient element is formed without 1 - p, because float64 cancels there as well: at a gap
of 30 between the largest logit and the rest, 1 - p is 1e-13 with four digits left; at a gap of 40 it is 0.
Ignored rows (label -1, keep == 0): loss 0, gradient 0.  A label outside [-1, C): NaN loss and gradient in that row.
"""
import torch

from ce_double import coefficients

F64 = torch.float64


def terms(x, adjust=None, gamma=0.0):
    """per class, [rows, C] float64: z, p, q, l, f, g, the one-hot arg-max mask `top`, and lse [rows]"""
    z = x.to(F64)
    if adjust is not None:
        z = z + adjust.to(F64)[None, :]
    rows, C = z.shape
    m, k = z.max(1)
    # torch.max returns an index of the maximum; the kernel's rule is the FIRST one
    k = (z == m[:, None]).to(torch.int64).argmax(1)
    top = torch.zeros(rows, C, dtype=torch.bool)
    top[torch.arange(rows), k] = True
    e = torch.exp(z - m[:, None])
    r = (e * ~top).sum(1)
    l1p = torch.log1p(r)
    inv = 1.0 / (1.0 + r)
    p = torch.where(top, inv[:, None], e * inv[:, None])
    q = torch.where(top, (r * inv)[:, None], 1.0 - p)
    l = torch.where(top, l1p[:, None], (m[:, None] - z) + l1p[:, None])
    qg = torch.ones_like(q) if gamma == 0 else q ** gamma
    ratio = torch.where(q > 0, l / torch.where(q > 0, q, torch.ones_like(q)), torch.zeros_like(q))
    g = qg + gamma * p * qg * ratio
    return dict(z=z, p=p, q=q, l=l, f=qg * l, g=g, top=top, lse=m + l1p)


def focal(x, *, labels=None, soft=None, keep=None, weight=None, eps=0.0, adjust=None, gamma=0.0, gscale=1.0, row_g=None):
    """x [rows, C] (any float type, taken to float64).  Returns a dict of float64 tensors: loss [rows], grad [rows, C]
    (= gscale * row_g * dloss/dx), s_loss [rows] = (1 + gamma) (|lse| A + sum_c a_c |z_c|), s_grad [rows] = (1 + gamma)
    |gscale * row_g| A, A [rows], and the boolean rows `kept` and `bad`."""
    assert (labels is None) != (soft is None)
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
    t = terms(x, adjust, gamma)
    gs = torch.full((rows,), float(gscale), dtype=F64)
    if row_g is not None:
        gs = gs * row_g.to(F64)
    loss = (a * t["f"]).sum(1)
    ag = a * t["g"]
    g_max = (ag * t["top"]).sum(1)
    g_rest = (ag * ~t["top"]).sum(1)
    d = torch.where(t["top"], t["p"] * g_rest[:, None] - t["q"] * g_max[:, None], t["p"] * (g_rest + g_max)[:, None] - ag)
    grad = gs[:, None] * d
    loss[~kept] = 0.0
    grad[~kept] = 0.0
    loss[bad] = float("nan")
    grad[bad] = float("nan")
    return dict(loss=loss, grad=grad, s_loss=(1.0 + gamma) * (t["lse"].abs() * A + (a * t["z"].abs()).sum(1)),
                s_grad=(1.0 + gamma) * gs.abs() * A, A=A, kept=kept, bad=bad)
