"""afft_softmax_ce_w / afft_softmax_ce_frames_w (class weights and label smoothing in the fused cross-entropy kernel, csrc/loss.hip)
ELEMENTWISE against the float64 double of tests/ce_double.py, over a pruned grid of the shapes at which a 256-thread-per-row kernel can
go wrong -- not the workload's shapes: C in {1, 2, 63, 255, 256, 257, 513} and one C = 3806; rows in {1, 5, 64}; leading dimensions C
and C rounded up to 64 (the pad columns of the gradient must come back exactly 0); fp32 and bf16 gradients; hard labels with -1 rows,
soft targets with and without keep; gscale and row_g; smoothing in {0, 0.1, 1}; weights none / random positive / with zeros that
include a label's own class.  Every gradient is written into a view with a sentinel row above and below.

Tolerances, per element, u = 2^-24:   loss  |got - ref| <= c u S,  S = |lse| A + sum_c a_c |x_c|
                                      grad  |got - ref| <= c u S,  S = |gscale row_g| A      (+ 2^-8 |ref| for a bf16 gradient)
c: the worst |got - ref| / (u S) measured on an MI355X over the grid, separately for loss / gradient and hard / soft, rounded up to the
next power of two (MEASURED and C_BAR below).  The same ratio for the unchanged entry points (afft_softmax_ce, which the smoothing-0,
no-weight cases reach through the _w entry points as well) is measured by the same test over the same inputs and listed as "plain".

Required exactly: a null weight with smoothing 0 returns the sibling entry point's bits; a row whose A is 0 gives a loss and gradient
of exactly 0; ignored rows are exactly 0; a label out of range gives NaN in that row only; two runs give equal bits.
"""
import itertools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import ce_double  # noqa: E402
from ce_cases import SENT, U, dev, framed, launch, make_inputs, ratios, to_dev, up  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = [1, 2, 63, 255, 256, 257, 513, 3806]
ROWS = [1, 5, 64]
EPS = [0.0, 0.1, 1.0]
WMODES = ["none", "pos", "zeros"]
KINDS = ["hard", "soft", "soft_keep"]

# worst |got - ref| / (u S) over the grid on an MI355X: the weighted / smoothed kernel, and the plain kernel on the same inputs
MEASURED = {
    "w": dict(loss_hard=3.181, loss_soft=2.779, grad_hard=3.229, grad_soft=3.159),
    "plain": dict(loss_hard=1.660, loss_soft=2.344, grad_hard=2.690, grad_soft=2.717),
}
# c = 4 for all four; the plain kernel's own figures round to 2, 4, 4, 4: three block sums instead of one cost less than a factor of 2
C_BAR = {k: 2.0 ** math.ceil(math.log2(v)) for k, v in MEASURED["w"].items()}
assert C_BAR == dict(loss_hard=4.0, loss_soft=4.0, grad_hard=4.0, grad_soft=4.0)


def grid(C):
    """the pruned grid of one C: every (kind, smoothing, weights) -- 27 cases -- with rows, leading dimension, gradient type and
    gradient scaling rotating through their values, so that each value meets each kernel path"""
    ci = CS.index(C)
    for i, (kind, eps, wmode) in enumerate(itertools.product(KINDS, EPS, WMODES)):
        rows = ROWS[(i + ci) % 3] if C != 3806 else ROWS[(i + i // 3) % 3]
        yield dict(kind=kind, eps=eps, wmode=wmode, rows=rows, pad=(i + i // 3 + ci) % 2 == 0, bf16=(i + i // 9 + ci) % 2 == 1,
                   scaled=(i // 2 + ci) % 2 == 0, seed=1000 * ci + i)


WORST = {"w": {}, "plain": {}}


@pytest.mark.parametrize("C", CS)
def test_weighted_ce_against_float64(C):
    from afft_amd import ops
    worst = {"w": {}, "plain": {}}
    fails = []
    for c in grid(C):
        x, labels, soft, keep, w, _ = make_inputs(c["rows"], C, c["kind"], c["wmode"], c["seed"])
        ld = up(C, 64) if c["pad"] else C
        gscale, row_g = (0.37, torch.randn(c["rows"], generator=torch.Generator().manual_seed(c["seed"])) + 0.2) if c["scaled"] else (1.0, None)
        ref = ce_double.ce(x, labels=labels, soft=soft, keep=keep, weight=w, eps=float(np.float32(c["eps"])), gscale=gscale, row_g=row_g)
        loss, dblock, border = launch(ops.softmax_ce_w, x, C, labels, soft, keep, ld, c["bf16"], gscale, row_g, weight=to_dev(w),
                                      smoothing=c["eps"])
        assert border, c
        plain = w is None and c["eps"] == 0.0
        hs = "hard" if c["kind"] == "hard" else "soft"
        r_loss, r_grad = ratios(loss, dblock, ref, C, c["bf16"])
        for what, r in (("loss_" + hs, r_loss), ("grad_" + hs, r_grad)):
            tab = worst["plain" if plain else "w"]
            tab[what] = max(tab.get(what, 0.0), r)
            if r > C_BAR[what]:
                fails.append((what, r, c))
        if c["eps"] == 0.0 and c["wmode"] == "zeros" and c["rows"] > 1 and (keep is None or keep[1]):
            assert float(ref["A"][1]) == 0.0 and float(loss[1]) == 0.0 and bool((dblock[1] == 0).all())      # the A == 0 row is in the grid
        if plain:
            # the sibling entry point on the same inputs: the same bits, and its own ratio
            loss0, dblock0, _ = launch(ops.softmax_ce, x, C, labels, soft, keep, ld, c["bf16"], gscale, row_g)
            assert torch.equal(loss0, loss) and torch.equal(dblock0, dblock), c
    for k in ("w", "plain"):
        for what, r in worst[k].items():
            WORST[k][what] = max(WORST[k].get(what, 0.0), r)
    print(f"C={C}: worst |got-ref|/(u S): " + json.dumps({k: {w_: round(r, 3) for w_, r in v.items()} for k, v in worst.items()}))
    print("so far: " + json.dumps({k: {w_: round(r, 3) for w_, r in v.items()} for k, v in WORST.items()}))
    assert not fails, fails[:4]


def frames_case(clips, L, n0, C, seed):
    ld = up(C, 64)
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((clips, L, ld), float("nan"))
    buf[:, :, :C] = torch.randn(clips, L, C, generator=g) * 3.0
    w = torch.rand(C, generator=g) * 2.0 + 0.1
    w[C // 2] = 0.0
    return buf, ld, w, g


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("clips,L,n0,C", [(3, 5, 1, 11), (5, 7, 4, 257), (4, 3, 2, 3806)])
def test_frames_form_lands_both_gradients_in_one_buffer(clips, L, n0, C, soft):
    """afft_softmax_ce_frames_w on the two slices x[:, :n0], x[:, n0:] of one padded (clips, L, ld) buffer: both gradients land in one
    (clips, L, ld) buffer, pad columns 0, every element written"""
    from afft_amd import ops
    buf, ld, w, g = frames_case(clips, L, n0, C, 7 * C + L)
    xfull = buf.to(dev())
    x = xfull[:, :, :C]
    dfull = torch.full((clips, L, ld), SENT, device=dev())
    hs = "soft" if soft else "hard"
    for lo, hi in ((0, n0), (n0, L)):
        n = hi - lo
        rows = clips * n
        labels = t = keep = None
        if soft:
            t = torch.softmax(torch.randn(rows, C, generator=g), 1)
            keep = (torch.rand(rows, generator=g) < 0.7).to(torch.uint8)
        else:
            labels = torch.randint(0, C, (rows,), generator=g)
            labels[::3] = -1
        row_g = torch.randn(rows, generator=g) + 0.3
        kw = dict(labels=to_dev(labels), soft=to_dev(t), keep=to_dev(keep), weight=w.to(dev()), smoothing=0.1)
        rl = torch.full((rows,), SENT, device=dev())
        ops.softmax_ce_frames_w(x[:, lo:hi], C, row_loss=rl, **kw)
        ops.softmax_ce_frames_w(x[:, lo:hi], C, row_g=row_g.to(dev()), dlogits3=dfull[:, lo:hi], **kw)
        ref = ce_double.ce(buf[:, lo:hi, :C].reshape(rows, C), labels=labels, soft=t, keep=keep, weight=w, eps=float(np.float32(0.1)),
                           row_g=row_g)
        r_loss, r_grad = ratios(rl.cpu(), dfull[:, lo:hi].cpu().reshape(rows, ld), ref, C, False)
        print(f"frames {clips}x{L}x{C} [{lo}:{hi}] {hs}: loss {r_loss:.3f} grad {r_grad:.3f}")
        assert r_loss <= C_BAR["loss_" + hs] and r_grad <= C_BAR["grad_" + hs]
    assert not bool((dfull == SENT).any())          # every element of the shared buffer was written
    # the null-weight, smoothing-0 form is the sibling's launch: equal bits, slice by slice
    d_w, d_0 = torch.full_like(dfull, SENT), torch.full_like(dfull, SENT)
    for lo, hi in ((0, n0), (n0, L)):
        rows = clips * (hi - lo)
        labels = torch.randint(-1, C, (rows,), generator=g).to(dev())
        l_w, l_0 = torch.empty(rows, device=dev()), torch.empty(rows, device=dev())
        ops.softmax_ce_frames_w(x[:, lo:hi], C, labels=labels, row_loss=l_w, weight=None, smoothing=0.0)
        ops.softmax_ce_frames(x[:, lo:hi], C, labels=labels, row_loss=l_0)
        ops.softmax_ce_frames_w(x[:, lo:hi], C, labels=labels, dlogits3=d_w[:, lo:hi])
        ops.softmax_ce_frames(x[:, lo:hi], C, labels=labels, dlogits3=d_0[:, lo:hi])
        assert torch.equal(l_w, l_0)
    assert torch.equal(d_w, d_0) and not bool((d_w == SENT).any())


def test_out_of_range_labels_poison_their_rows_only():
    from afft_amd import ops
    rows, C = 9, 257
    x, labels, _, _, w, _ = make_inputs(rows, C, "hard", "pos", 77)
    bad = labels.clone()
    bad[0], bad[3], bad[5], bad[8] = C, -2, C + 5, 1 << 40
    out = {}
    for name, lb in (("clean", labels), ("bad", bad)):
        out[name] = launch(ops.softmax_ce_w, x, C, lb, None, None, up(C, 64), False, 1.0, None, weight=to_dev(w), smoothing=0.1)
    (l0, d0, b0), (l1, d1, b1) = out["clean"], out["bad"]
    assert b0 and b1
    poisoned = torch.tensor([i in (0, 3, 5, 8) for i in range(rows)])
    assert bool(torch.isnan(l1[poisoned]).all()) and bool(torch.isnan(d1[poisoned][:, :C]).all())
    assert bool((d1[poisoned][:, C:] == 0).all())
    assert torch.equal(l1[~poisoned], l0[~poisoned]) and torch.equal(d1[~poisoned], d0[~poisoned])
    assert bool(torch.isfinite(l0).all()) and bool(torch.isfinite(d0).all())


@pytest.mark.parametrize("rows,C,kind", [(64, 3806, "hard"), (5, 257, "soft_keep"), (64, 513, "soft")])
def test_two_runs_give_equal_bits(rows, C, kind):
    from afft_amd import ops
    x, labels, soft, keep, w, _ = make_inputs(rows, C, kind, "zeros", 5)
    row_g = torch.randn(rows, generator=torch.Generator().manual_seed(6))
    runs = [launch(ops.softmax_ce_w, x, C, labels, soft, keep, up(C, 64), False, 0.5, row_g, weight=to_dev(w), smoothing=0.1)
            for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ls = [torch.zeros(1, device=dev()) for _ in range(2)]
    for s in ls:      # loss_sum: the ordered sum of the row losses
        ops.softmax_ce_w(framed(x, C), C, labels=to_dev(labels), soft=to_dev(soft), keep=to_dev(keep), weight=to_dev(w), smoothing=0.1,
                         row_loss=torch.empty(rows, device=dev()), loss_sum=s)
    assert torch.equal(ls[0], ls[1])
    ref = ce_double.ce(x, labels=labels, soft=soft, keep=keep, weight=w, eps=float(np.float32(0.1)))
    # every row loss within its bar, then a sum of `rows` terms
    bar = (C_BAR["loss_hard" if kind == "hard" else "loss_soft"] + rows) * U * float(ref["s_loss"].sum())
    assert abs(float(ls[0]) - float(ref["loss"].sum())) <= bar


def test_argument_errors_raise_and_launch_nothing():
    from afft_amd import ops
    rows, C = 5, 63
    x, labels, _, _, w, _ = make_inputs(rows, C, "hard", "pos", 3)
    xd, lb, wd = framed(x, C), labels.to(dev()), w.to(dev())
    rl = torch.full((rows,), SENT, device=dev())
    d = torch.full((rows, C), SENT, device=dev())
    d3 = torch.full((1, rows, C), SENT, device=dev())
    bad = [dict(weight=wd, smoothing=-0.1), dict(weight=wd, smoothing=1.5), dict(weight=None, smoothing=float("nan")),
           dict(weight=wd[:-1].contiguous(), smoothing=0.1), dict(weight=torch.cat([wd, wd]), smoothing=0.1),
           dict(weight=wd.double(), smoothing=0.1), dict(weight=w, smoothing=0.1), dict(weight=torch.cat([wd, wd])[::2], smoothing=0.1)]
    for opts in bad:
        with pytest.raises((RuntimeError, ValueError)):
            ops.softmax_ce_w(xd, C, labels=lb, row_loss=rl, dlogits=d, **opts)
        with pytest.raises((RuntimeError, ValueError)):
            ops.softmax_ce_frames_w(xd[None], C, labels=lb, row_loss=rl, dlogits3=d3, **opts)
    torch.cuda.synchronize()
    assert bool((rl == SENT).all()) and bool((d == SENT).all()) and bool((d3 == SENT).all())
    with pytest.raises(RuntimeError, match=r"smoothing must lie in \[0, 1\]"):
        ops.softmax_ce_w(xd, C, labels=lb, row_loss=rl, smoothing=1.5)
    ops.softmax_ce_w(xd, C, labels=lb, row_loss=rl, weight=wd, smoothing=1.0)      # the ends of the range are fine
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rl).all())


# ----------------------------------------------------------------------------- the module path against the reference's fixture
@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "c0_weighted_ce.npz"))
    return {k: z[k] for k in z.files if k != "meta"}, json.loads(str(z["meta"]))


@pytest.mark.parametrize("form", ["rows", "walked", "landing"])
@pytest.mark.parametrize("one_hot", [False, True])
@pytest.mark.parametrize("variant", ["w", "s", "ws"])
def test_module_path_matches_the_reference_fixture(golden, variant, one_hot, form):
    """MultiDimCrossEntropy(weight=, label_smoothing=) on (B, T, C) logits, loss and logits.grad, against the fixture computed by the
    reference's criterion in float64: flattened to rows (a 4-D view), the 3-D tensor walked in place, and the two halves of
    functional.split_rows with their gradients landing in one buffer"""
    from afft_amd import functional as F_
    from afft_amd.common.runner import MultiDimCrossEntropy
    arr, meta = golden
    v = meta["variants"][variant]
    B, T, C = arr["logits"].shape
    w = torch.from_numpy(arr["weight"]) if v["weight"] else None
    crit = MultiDimCrossEntropy(weight=None if w is None else w.double(), label_smoothing=v["smoothing"])
    x = torch.from_numpy(arr["logits"]).to(dev())
    x = (x.reshape(3, 2, T, C) if form == "rows" else x).requires_grad_(True)
    lead = x.shape[:-1]
    kind = "soft" if one_hot else "hard"
    labels, soft, ign = (torch.from_numpy(arr[k]).to(dev()) for k in ("labels", "soft", "ignore"))
    cpu = dict(labels=None if one_hot else torch.from_numpy(arr["labels"]).reshape(-1),
               soft=torch.from_numpy(arr["soft"]).reshape(-1, C) if one_hot else None,
               keep=torch.from_numpy(~arr["ignore"]).reshape(-1).to(torch.uint8) if one_hot else None)
    ref = ce_double.ce(torch.from_numpy(arr["logits"]).reshape(-1, C), weight=w, eps=v["smoothing"], **cpu)      # for S alone

    def run(xs, sl):
        if one_hot:
            ig = ign[sl] if form == "landing" else ign.reshape(lead)
            out = crit(xs, soft[sl] if form == "landing" else soft.reshape(*lead, C), one_hot=True, ignore_index=ig)
            return out * ((~ig).sum().float() / ig.numel())      # the keep rescaling of the module undone
        return crit(xs, labels[sl] if form == "landing" else labels.reshape(lead))

    if form == "landing":
        n = 1
        a, b = F_.split_rows(x, n)
        la, lb_ = run(a, (slice(None), slice(0, n))), run(b, (slice(None), slice(n, T)))
        (la.sum() + lb_.sum()).backward()
        loss = torch.cat([la.reshape(B, n), lb_.reshape(B, T - n)], 1).reshape(-1)
    else:
        loss = run(x, None)
        loss.sum().backward()
    assert crit.weight is None or (crit.weight.dtype == torch.float32 and crit.weight.is_cuda)
    got_l, got_g = loss.detach().double().cpu(), x.grad.double().cpu().reshape(-1, C)
    want_l, want_g = torch.from_numpy(arr[f"{kind}_{variant}_loss"]), torch.from_numpy(arr[f"{kind}_{variant}_grad"]).reshape(-1, C)
    # the rescaling above and the module's own cost the loss two more roundings (u |loss| each), and make the kernel's row_g
    # rows / kept * kept / rows: 1 to within two roundings
    tol_l = C_BAR["loss_" + kind] * U * ref["s_loss"] + (2 * U * want_l.abs() if one_hot else 0)
    tol_g = C_BAR["grad_" + kind] * U * ref["s_grad"][:, None] + (2 * U * want_g.abs() if one_hot else 0)
    assert bool(((got_l - want_l).abs() <= tol_l).all()), float(((got_l - want_l).abs() - tol_l).max())
    assert bool(((got_g - want_g).abs() <= tol_g).all()), float(((got_g - want_g).abs() - tol_g).max())
    zero = ref["s_loss"] == 0
    assert bool((got_l[zero] == 0).all()) and bool((got_g[zero] == 0).all())
