"""afft_softmax_ce_focal / afft_softmax_ce_frames_focal (focal exponent and logit adjustment in the fused cross-entropy, csrc/loss.hip)
ELEMENTWISE against the float64 double of tests/focal_double.py, over a pruned grid of the shapes at which a 256-thread-per-row kernel
can go wrong: C in {1, 2, 255, 256, 257, 513} and one C = 3806; rows in {1, 5}; leading dimensions C and C rounded up to 64 (the pad
columns of the gradient must come back exactly 0); fp32 and bf16 gradients; gamma in {0, 0.5, 2, 5}; no adjustment / one uniform in
[-8, 0]; hard labels with -1 rows, soft targets with and without keep; smoothing in {0, 0.1}; weights none / with zeros that include a
label's own class; gscale and row_g set.  Per C the 12 (target, smoothing, weights) cases run, the other dimensions rotating through
their values (grid(); 84 cases, two launches each).  Every gradient is written into a view with a sentinel row above and below.

Tolerances, per element, u = 2^-24:   loss  |got - ref| <= c u S,  S = (1 + gamma) (|lse| A + sum_c a_c |z_c|)
                                      grad  |got - ref| <= c u S,  S = (1 + gamma) |gscale row_g| A      (+ 2^-8 |ref| for a bf16 gradient)
c: the worst |got - ref| / (u S) measured on an MI355X over the grid, separately for loss / gradient and hard / soft, rounded up to the
next power of two (MEASURED and C_BAR below).  The same ratio for afft_softmax_ce_w on the gamma = 0, no-adjustment cases of the grid
(which the focal entry points forward to it) is measured by the same test and listed as "w"; its bars are 4.

Required exactly: gamma = 0 with no adjustment returns ops.softmax_ce_w's bits; ignored rows and rows whose A is 0 are exactly 0; pad
columns are exactly 0; a label out of range gives NaN in its row only; sentinels intact; two runs give equal bits.

Dominant-class rows: the label is the arg-max by a gap of 4, 12 or 30 -- the label's loss and its own gradient element RELATIVE to the
double, at most 2^-16: a condition, not a measurement (1 - p formed directly misses it by orders of magnitude at 12 and gives 0 at 30).
"""
import itertools
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import focal_double  # noqa: E402
from ce_cases import SENT, U, dev, framed, launch, make_inputs, ratios, to_dev, up  # noqa: E402

pytestmark = pytest.mark.gpu

CS = [1, 2, 255, 256, 257, 513, 3806]
ROWS = [1, 5]
GAMMAS = [0.0, 0.5, 2.0, 5.0]
EPS = [0.0, 0.1]
WMODES = ["none", "zeros"]
KINDS = ["hard", "soft", "soft_keep"]
EPS32 = {0.0: 0.0, 0.1: float(torch.tensor(0.1, dtype=torch.float32))}       # the smoothing as the kernel receives it

# worst |got - ref| / (u S) over the grid on an MI355X: the focal kernel, and afft_softmax_ce_w on the gamma = 0, no-adjustment cases
MEASURED = {
    "focal": dict(loss_hard=2.195, loss_soft=1.722, grad_hard=1.566, grad_soft=1.707),
    "w": dict(loss_hard=2.013, loss_soft=1.281, grad_hard=0.988, grad_soft=1.905),
}
# c = 4 for the hard-label loss, 2 for the other three.  The other tests of this file stay below 1.1 (frames 1.03, SoftmaxCE.apply
# 0.88, dominant-class rows 0.78, a label 30 below the maximum 0.33).
C_BAR = {k: 2.0 ** math.ceil(math.log2(v)) for k, v in MEASURED["focal"].items()}
assert C_BAR == dict(loss_hard=4.0, loss_soft=2.0, grad_hard=2.0, grad_soft=2.0)
W_BAR = 4.0


def grid(C):
    """the pruned grid of one C: every (target, smoothing, weights) -- 12 cases -- with gamma, the adjustment, rows, leading dimension
    and gradient type rotating so that over the seven C every pair of values of two dimensions meets (checked below)"""
    ci = CS.index(C)
    for i, (kind, eps, wmode) in enumerate(itertools.product(KINDS, EPS, WMODES)):
        j = i + 5 * ci
        yield dict(kind=kind, eps=eps, wmode=wmode, gamma=GAMMAS[(j + j // 4) % 4], adj=(j // 2 + ci) % 2 == 1,
                   rows=ROWS[(i + i // 2 + ci) % 2], pad=(i // 4 + i + ci) % 2 == 0, bf16=(i // 2 + i // 6 + ci) % 2 == 1, seed=1000 * ci + i)


_ALL = [c for C_ in CS for c in grid(C_)]
assert len({(c["gamma"], c["adj"], c["kind"]) for c in _ALL}) == 24 and len({(c["gamma"], c["adj"], c["eps"]) for c in _ALL}) == 16
assert len({(c["gamma"], c["adj"]) for c in _ALL if c["kind"] == "hard" and c["eps"] == 0.0}) == 8      # the one-term path meets all
assert len({(c["bf16"], c["gamma"], c["adj"]) for c in _ALL}) == 16 and len(_ALL) == 84

WORST = {"focal": {}, "w": {}}


@pytest.mark.parametrize("C", CS)
def test_focal_ce_against_float64(C):
    from afft_amd import ops
    worst = {"focal": {}, "w": {}}
    fails = []
    for c in grid(C):
        x, labels, soft, keep, w, b = make_inputs(c["rows"], C, c["kind"], c["wmode"], c["seed"], adj=c["adj"])
        ld = up(C, 64) if c["pad"] else C
        gscale, row_g = 0.37, torch.randn(c["rows"], generator=torch.Generator().manual_seed(c["seed"])) + 0.2
        ref = focal_double.focal(x, labels=labels, soft=soft, keep=keep, weight=w, eps=EPS32[c["eps"]], adjust=b, gamma=c["gamma"],
                                 gscale=gscale, row_g=row_g)
        loss, dblock, border = launch(ops.softmax_ce_focal, x, C, labels, soft, keep, ld, c["bf16"], gscale, row_g, weight=to_dev(w),
                                      smoothing=c["eps"], adjust=to_dev(b), gamma=c["gamma"])
        assert border, c
        forwarded = b is None and c["gamma"] == 0.0
        hs = "hard" if c["kind"] == "hard" else "soft"
        r_loss, r_grad = ratios(loss, dblock, ref, C, c["bf16"])
        for what, r in (("loss_" + hs, r_loss), ("grad_" + hs, r_grad)):
            tab = worst["w" if forwarded else "focal"]
            tab[what] = max(tab.get(what, 0.0), r)
            if r > (W_BAR if forwarded else C_BAR[what]):
                fails.append((what, r, c))
        if c["eps"] == 0.0 and c["wmode"] == "zeros" and c["rows"] > 1 and (keep is None or keep[1]):
            assert float(ref["A"][1]) == 0.0 and float(loss[1]) == 0.0 and bool((dblock[1] == 0).all())      # the A == 0 row is in the grid
        if forwarded:
            # the _w entry point on the same inputs: the same bits
            loss0, dblock0, _ = launch(ops.softmax_ce_w, x, C, labels, soft, keep, ld, c["bf16"], gscale, row_g, weight=to_dev(w),
                                       smoothing=c["eps"])
            assert torch.equal(loss0, loss) and torch.equal(dblock0, dblock), c
    for k in worst:
        for what, r in worst[k].items():
            WORST[k][what] = max(WORST[k].get(what, 0.0), r)
    print(f"C={C}: worst |got-ref|/(u S): " + json.dumps({k: {w_: round(r, 3) for w_, r in v.items()} for k, v in worst.items()}))
    print("so far: " + json.dumps({k: {w_: round(r, 3) for w_, r in v.items()} for k, v in WORST.items()}))
    assert not fails, fails[:4]


@pytest.mark.parametrize("soft", [False, True])
def test_frames_form_inside_a_wider_tensor(soft):
    """afft_softmax_ce_frames_focal on frames 2..3 of a padded (3, 5, ld) buffer, C = 257: the gradient lands in the same frames of a
    (3, 5, ld) buffer, pad columns 0, the other frames untouched"""
    from afft_amd import ops
    clips, L, lo, hi, C = 3, 5, 2, 4, 257
    ld = up(C, 64)
    g = torch.Generator().manual_seed(11)
    buf = torch.full((clips, L, ld), float("nan"))
    buf[:, :, :C] = torch.randn(clips, L, C, generator=g) * 3.0
    w = torch.rand(C, generator=g) * 2.0 + 0.1
    w[C // 2] = 0.0
    b = -8.0 * torch.rand(C, generator=g)
    rows = clips * (hi - lo)
    labels = t = keep = None
    if soft:
        t = torch.softmax(torch.randn(rows, C, generator=g), 1)
        keep = (torch.rand(rows, generator=g) < 0.7).to(torch.uint8)
    else:
        labels = torch.randint(0, C, (rows,), generator=g)
        labels[::3] = -1
    row_g = torch.randn(rows, generator=g) + 0.3
    x = buf.to(dev())[:, lo:hi, :C]
    dfull = torch.full((clips, L, ld), SENT, device=dev())
    kw = dict(labels=to_dev(labels), soft=to_dev(t), keep=to_dev(keep), weight=w.to(dev()), smoothing=0.1, adjust=b.to(dev()), gamma=2.0)
    rl = torch.full((rows,), SENT, device=dev())
    ops.softmax_ce_frames_focal(x, C, row_loss=rl, **kw)
    ops.softmax_ce_frames_focal(x, C, row_g=row_g.to(dev()), dlogits3=dfull[:, lo:hi], **kw)
    ref = focal_double.focal(buf[:, lo:hi, :C].reshape(rows, C), labels=labels, soft=t, keep=keep, weight=w, eps=EPS32[0.1], adjust=b,
                             gamma=2.0, row_g=row_g)
    hs = "soft" if soft else "hard"
    r_loss, r_grad = ratios(rl.cpu(), dfull[:, lo:hi].cpu().reshape(rows, ld), ref, C, False)
    print(f"frames {hs}: loss {r_loss:.3f} grad {r_grad:.3f}")
    assert r_loss <= C_BAR["loss_" + hs] and r_grad <= C_BAR["grad_" + hs]
    assert bool((dfull[:, :lo] == SENT).all()) and bool((dfull[:, hi:] == SENT).all()) and not bool((dfull[:, lo:hi] == SENT).any())
    # gamma 0, no adjustment: the _w form's bits
    d_f, d_w = torch.full_like(dfull, SENT), torch.full_like(dfull, SENT)
    l_f, l_w = torch.empty(rows, device=dev()), torch.empty(rows, device=dev())
    kw.update(adjust=None, gamma=0.0)
    ops.softmax_ce_frames_focal(x, C, row_loss=l_f, **kw)
    ops.softmax_ce_frames_focal(x, C, dlogits3=d_f[:, lo:hi], **kw)
    del kw["adjust"], kw["gamma"]
    ops.softmax_ce_frames_w(x, C, row_loss=l_w, **kw)
    ops.softmax_ce_frames_w(x, C, dlogits3=d_w[:, lo:hi], **kw)
    assert torch.equal(l_f, l_w) and torch.equal(d_f, d_w)


def dominant(C, gap, label_is_max, seed):
    """4 rows whose largest logit leads the next one by `gap` (to fp32 rounding); the label is that class, or (mirror) another one"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(4, C, generator=g)
    top = torch.tensor([0, C - 1, C // 2, (C // 3) % C])
    x[torch.arange(4), top] = -1.0
    x[torch.arange(4), top] = x.max(1).values + gap
    labels = top if label_is_max else (top + 1) % C
    return x, labels


@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("gap", [4.0, 12.0, 30.0])
@pytest.mark.parametrize("C", [2, 257])
def test_dominant_class_rows_keep_their_relative_accuracy(C, gap, gamma):
    from afft_amd import ops
    x, labels = dominant(C, gap, True, int(C + gap))
    ref = focal_double.focal(x, labels=labels, gamma=gamma)
    loss, d, border = launch(ops.softmax_ce_focal, x, C, labels, None, None, C, False, 1.0, None, gamma=gamma)
    i = torch.arange(4)
    own, own_ref = d[i, labels].double(), ref["grad"][i, labels]
    assert border and bool((ref["loss"] > 0).all()) and bool((own_ref < 0).all())
    rel_l = float(((loss.double() - ref["loss"]).abs() / ref["loss"]).max())
    rel_g = float(((own - own_ref).abs() / own_ref.abs()).max())
    print(f"C={C} gap={gap} gamma={gamma}: relative error loss {rel_l:.3e} own gradient {rel_g:.3e} (bar {2.0 ** -16:.3e})")
    assert rel_l <= 2.0 ** -16 and rel_g <= 2.0 ** -16
    r_loss, r_grad = ratios(loss, d, ref, C, False)
    print(f"  against S: loss {r_loss:.3f} grad {r_grad:.3f}")
    assert r_loss <= C_BAR["loss_hard"] and r_grad <= C_BAR["grad_hard"]


@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("C", [2, 257])
def test_label_far_below_the_maximum_is_finite(C, gamma):
    """the mirror: another class leads the label by 30"""
    from afft_amd import ops
    x, labels = dominant(C, 30.0, False, C)
    ref = focal_double.focal(x, labels=labels, gamma=gamma)
    loss, d, border = launch(ops.softmax_ce_focal, x, C, labels, None, None, C, False, 1.0, None, gamma=gamma)
    assert border and bool((loss > 29.0).all())
    r_loss, r_grad = ratios(loss, d, ref, C, False)       # asserts finiteness
    print(f"C={C} gamma={gamma}, the label 30 below the maximum, against S: loss {r_loss:.3f} grad {r_grad:.3f}")
    assert r_loss <= C_BAR["loss_hard"] and r_grad <= C_BAR["grad_hard"]


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_out_of_range_labels_poison_their_rows_only(eps):
    from afft_amd import ops
    rows, C = 9, 257
    x, labels, _, _, w, b = make_inputs(rows, C, "hard", "zeros", 77, adj=True)
    bad = labels.clone()
    bad[0], bad[3], bad[5], bad[8] = C, -2, C + 5, 1 << 40
    out = {}
    for name, lb in (("clean", labels), ("bad", bad)):
        out[name] = launch(ops.softmax_ce_focal, x, C, lb, None, None, up(C, 64), False, 1.0, None, weight=to_dev(w), smoothing=eps,
                           adjust=to_dev(b), gamma=2.0)
    (l0, d0, b0), (l1, d1, b1) = out["clean"], out["bad"]
    assert b0 and b1
    poisoned = torch.tensor([i in (0, 3, 5, 8) for i in range(rows)])
    assert bool(torch.isnan(l1[poisoned]).all()) and bool(torch.isnan(d1[poisoned][:, :C]).all())
    assert bool((d1[poisoned][:, C:] == 0).all())
    assert torch.equal(l1[~poisoned], l0[~poisoned]) and torch.equal(d1[~poisoned], d0[~poisoned])
    assert bool(torch.isfinite(l0).all()) and bool(torch.isfinite(d0).all())


@pytest.mark.parametrize("rows,C,kind", [(5, 3806, "hard"), (5, 257, "soft_keep"), (5, 513, "soft")])
def test_two_runs_give_equal_bits(rows, C, kind):
    from afft_amd import ops
    x, labels, soft, keep, w, b = make_inputs(rows, C, kind, "zeros", 5, adj=True)
    row_g = torch.randn(rows, generator=torch.Generator().manual_seed(6))
    opts = dict(weight=to_dev(w), smoothing=0.1 if kind != "hard" else 0.0, adjust=to_dev(b), gamma=2.0)
    runs = [launch(ops.softmax_ce_focal, x, C, labels, soft, keep, up(C, 64), False, 0.5, row_g, **opts) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ls = [torch.zeros(1, device=dev()) for _ in range(2)]
    for s in ls:      # loss_sum: the ordered sum of the row losses
        ops.softmax_ce_focal(framed(x, C), C, labels=to_dev(labels), soft=to_dev(soft), keep=to_dev(keep),
                             row_loss=torch.empty(rows, device=dev()), loss_sum=s, **opts)
    assert torch.equal(ls[0], ls[1])
    ref = focal_double.focal(x, labels=labels, soft=soft, keep=keep, weight=w, eps=EPS32[0.1] if kind != "hard" else 0.0, adjust=b, gamma=2.0)
    # every row loss within its bar, then a sum of `rows` terms
    bar = (C_BAR["loss_hard" if kind == "hard" else "loss_soft"] + rows) * U * float(ref["s_loss"].sum())
    assert abs(float(ls[0]) - float(ref["loss"].sum())) <= bar


def test_argument_errors_raise_and_launch_nothing():
    from afft_amd import ops
    rows, C = 5, 63
    x, labels, _, _, _, b = make_inputs(rows, C, "hard", "none", 3, adj=True)
    xd, lb, bd = framed(x, C), labels.to(dev()), b.to(dev())
    rl = torch.full((rows,), SENT, device=dev())
    d = torch.full((rows, C), SENT, device=dev())
    d3 = torch.full((1, rows, C), SENT, device=dev())
    bad = [dict(gamma=-0.5), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(adjust=bd, gamma=-1.0),
           dict(adjust=bd[:-1].contiguous()), dict(adjust=torch.cat([bd, bd])), dict(adjust=bd.double()), dict(adjust=b),
           dict(adjust=torch.cat([bd, bd])[::2]), dict(adjust=bd, gamma=2.0, smoothing=1.5)]
    for opts in bad:
        with pytest.raises((RuntimeError, ValueError)):
            ops.softmax_ce_focal(xd, C, labels=lb, row_loss=rl, dlogits=d, **opts)
        with pytest.raises((RuntimeError, ValueError)):
            ops.softmax_ce_frames_focal(xd[None], C, labels=lb, row_loss=rl, dlogits3=d3, **opts)
    torch.cuda.synchronize()
    assert bool((rl == SENT).all()) and bool((d == SENT).all()) and bool((d3 == SENT).all())
    # the library's own check, behind the wrapper's
    from afft_amd import _lib as L
    rc = L.lib().afft_softmax_ce_focal(xd.data_ptr(), C, rows, C, lb.data_ptr(), None, 0, None, 1.0, None, None, None, 0, 0, rl.data_ptr(),
                                       None, 0.0, None, float("nan"), None)
    assert rc != 0
    torch.cuda.synchronize()
    assert bool((rl == SENT).all())


# ----------------------------------------------------------------------------- end to end
def test_autograd_function_on_a_frames_view():
    """SoftmaxCE.apply with the nine arguments on a (clips, frames, C) view of a wider tensor, through autograd"""
    from afft_amd import functional as F_
    clips, L, n, C = 3, 5, 2, 257
    g = torch.Generator().manual_seed(21)
    full = (torch.randn(clips, L, C, generator=g) * 3.0)
    w = torch.rand(C, generator=g) + 0.5
    b = -8.0 * torch.rand(C, generator=g)
    labels = torch.randint(0, C, (clips * n,), generator=g)
    labels[1] = -1
    coef = torch.randn(clips * n, generator=g)
    leaf = full.to(dev()).requires_grad_(True)
    loss = F_.SoftmaxCE.apply(leaf[:, 1:1 + n], labels.to(dev()), None, None, None, w.to(dev()), 0.1, b.to(dev()), 2.0)
    (loss * coef.to(dev())).sum().backward()
    ref = focal_double.focal(full[:, 1:1 + n].reshape(-1, C), labels=labels, weight=w, eps=EPS32[0.1], adjust=b, gamma=2.0, row_g=coef)
    grad = leaf.grad.cpu()
    assert bool((grad[:, :1] == 0).all()) and bool((grad[:, 1 + n:] == 0).all())
    r_loss, r_grad = ratios(loss.detach().cpu(), grad[:, 1:1 + n].reshape(-1, C), ref, C, False)
    print(f"SoftmaxCE.apply: loss {r_loss:.3f} grad {r_grad:.3f}")
    assert r_loss <= C_BAR["loss_hard"] and r_grad <= C_BAR["grad_hard"]


def test_loss_accuracy_adjusts_the_loss_and_not_the_metrics():
    """BasicLossAccuracy(focal_gamma=2, logit_adjust={'action': b}): its loss terms are the double's, its acc1 / acc5 bitwise those
    of a default BasicLossAccuracy on the same logits (the adjustment is strong enough to change the arg-max of adjusted logits)"""
    from afft_amd.common.runner import BasicLossAccuracy
    B, T, C = 32, 3, 257
    g = torch.Generator().manual_seed(31)
    fut, past = torch.randn(B, 1, C, generator=g), torch.randn(B, T, C, generator=g)
    b = -8.0 * torch.rand(C, generator=g)
    target = {"action": torch.randint(0, C, (B,), generator=g)}
    past_t = {"action": torch.randint(0, C, (B, T, 1), generator=g)}
    out = {"logits/action": {"rgb": fut.to(dev())}, "past_logits/action": {"rgb": past.to(dev())}}
    tgt_d, past_d = {"action": target["action"].to(dev())}, {"action": past_t["action"].to(dev())}
    assert not torch.equal((fut[:, 0] + b).argmax(1), fut[:, 0].argmax(1))
    losses, metrics = BasicLossAccuracy(focal_gamma=2.0, logit_adjust={"action": b})(out, tgt_d, past_d)
    losses0, metrics0 = BasicLossAccuracy()(out, tgt_d, past_d)
    for k in ("acc1_action_rgb", "acc5_action_rgb"):
        assert torch.equal(torch.as_tensor(metrics[k]), torch.as_tensor(metrics0[k])), k
    for key, x, lb in (("cls_action_rgb", fut.reshape(-1, C), target["action"]), ("past_cls_action_rgb", past.reshape(-1, C), past_t["action"].reshape(-1))):
        ref = focal_double.focal(x, labels=lb, adjust=b, gamma=2.0)
        got = losses[key].detach().double().cpu().reshape(-1)
        tol = C_BAR["loss_hard"] * U * ref["s_loss"]
        assert bool(((got - ref["loss"]).abs() <= tol).all()), key
        n = got.numel()
        assert abs(float(got.mean()) - float(ref["loss"].mean())) <= float(tol.mean()) + n * U * float(ref["loss"].mean())
        assert not torch.equal(losses[key].reshape(-1), losses0[key].reshape(-1))
