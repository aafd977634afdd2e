"""afft_softmax_ce_groups / afft_softmax_ce_frames_groups (the marginal cross-entropy over class groups, csrc/loss.hip) ELEMENTWISE
against the float64 double of tests/groups_double.py over the case table of tests/groups_cases.py, each case with hard group labels
and with soft group targets, into an fp32 gradient of leading dimension C, and into fp32 and bf16 gradients of leading dimension
C + 5 inside sentinel rows (the pad columns must come back exactly 0).

Tolerances, per element, u = 2^-24:   loss  |got - ref| <= c u S,  S = |T lse| + sum_g |t_g lse_g|
                                      grad  |got - ref| <= c u S,  S = |gscale row_g| sum_g |t_g|     (+ 2^-8 |ref| for a bf16 gradient)
c: the worst |got - ref| / (u S) measured on an MI355X over the table, separately for loss / gradient and hard / soft, rounded up to
the next power of two (MEASURED and C_BAR below).  The yardstick is the unchanged afft_softmax_ce: the same test measures its ratios
(against tests/ce_double.py) on the same logits with class labels / class targets, and the new kernel's c may be at most 4 times the
sibling's -- one more max / exp / log in the chain is about a factor of 2, and 4 leaves one power of two.

Required exactly: ignored rows are 0; a bad row is NaN and no other row notices; pad columns are 0; two runs give equal bits.
"""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import ce_cases  # noqa: E402
import ce_double  # noqa: E402
import groups_cases  # noqa: E402
import groups_double  # noqa: E402
from ce_cases import SENT, U, dev, ratios, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
# worst |got - ref| / (u S) over the table on an MI355X: the group kernel, and afft_softmax_ce on the same logits
MEASURED = {
    "groups": dict(loss_hard=1.430, loss_soft=1.207, grad_hard=3.119, grad_soft=4.026),
    "plain": dict(loss_hard=1.136, loss_soft=1.407, grad_hard=3.119, grad_soft=3.631),
}
# c = 2, 2, 4, 8 against the sibling's 2, 2, 4, 4: the soft gradient's 4.026 (case sizes_keep) sits just over a power of two, where the
# sibling's own 3.631 sits just under it; every bar is within 2 times the sibling's, the allowance is 4


def bars(measured):
    return {k: 2.0 ** math.ceil(math.log2(v)) for k, v in measured.items()}


C_BAR, SIB_BAR = bars(MEASURED["groups"]), bars(MEASURED["plain"])
assert C_BAR == dict(loss_hard=2.0, loss_soft=2.0, grad_hard=4.0, grad_soft=8.0) and SIB_BAR == dict(loss_hard=2.0, loss_soft=2.0, grad_hard=4.0, grad_soft=4.0)
assert all(C_BAR[k] <= 4.0 * SIB_BAR[k] for k in C_BAR), (C_BAR, SIB_BAR)

WORST = {"groups": {}, "plain": {}}
LAYOUTS = [(0, False), (5, True), (5, False)]      # (pad columns, bf16 gradient)


def note(tab, what, r):
    WORST[tab][what] = max(WORST[tab].get(what, 0.0), r)


def double_of(c, kind):
    return groups_double.groups(c["x"], c["group_of"], c["G"], glabels=c["glabels"] if kind == "hard" else None,
                                gsoft=c["gsoft"] if kind == "soft" else None, keep=c["keep"], gscale=c["gscale"], row_g=c["row_g"])


@pytest.fixture(scope="module")
def refs():
    """the float64 results of every case, computed once"""
    return {(c["name"], kind): double_of(c, kind) for c in groups_cases.CASES for kind in ("hard", "soft")}


@pytest.mark.parametrize("c", groups_cases.CASES, ids=lambda c: c["name"])
def test_cases_against_float64(c, refs):
    from afft_amd import ops
    x = c["x"]
    rows, C = x.shape
    fails = []
    for kind in ("hard", "soft"):
        ref = refs[(c["name"], kind)]
        assert not bool(ref["bad"].any())
        for pad, bf16 in LAYOUTS:
            loss, dblock, border = groups_cases.launch(ops, c, kind, C + pad, bf16)
            assert border, (kind, pad, bf16)
            r_loss, r_grad = ratios(loss, dblock, ref, C, bf16)
            for what, r in (("loss_" + kind, r_loss), ("grad_" + kind, r_grad)):
                note("groups", what, r)
                if r > C_BAR[what]:
                    fails.append((what, r, pad, bf16))
    # the yardstick: afft_softmax_ce on the same logits, class labels / class targets drawn for them
    g = groups_cases.gen(1000 + C)
    labels = torch.randint(0, C, (rows,), generator=g)
    soft = torch.softmax(torch.randn(rows, C, generator=g), 1)
    for kind, lb, sf in (("hard", labels, None), ("soft", None, soft)):
        ref = ce_double.ce(x, labels=lb, soft=sf, keep=c["keep"], gscale=c["gscale"], row_g=c["row_g"])
        for pad, bf16 in LAYOUTS:
            loss, dblock, border = ce_cases.launch(ops.softmax_ce, x, C, lb, sf, c["keep"], C + pad, bf16, c["gscale"], c["row_g"])
            r_loss, r_grad = ratios(loss, dblock, ref, C, bf16)
            note("plain", "loss_" + kind, r_loss)
            note("plain", "grad_" + kind, r_grad)
    print(f"{c['name']}: worst |got-ref|/(u S) so far: " + json.dumps({k: {w: round(r, 3) for w, r in v.items()} for k, v in WORST.items()}))
    assert not fails, fails[:4]


def test_spread_rows_are_finite_and_about_240(refs):
    """a row-max-only implementation gives inf (hard) or loses the target's term here"""
    from afft_amd import ops
    for c in (c for c in groups_cases.CASES if c["name"].startswith("spread")):
        loss, dblock, _ = groups_cases.launch(ops, c, "hard", c["x"].shape[1], False)
        assert bool(torch.isfinite(loss).all()) and bool((loss > 235).all()) and bool((loss < 250).all()), loss
        assert bool(torch.isfinite(dblock).all())
        # the target group's classes take -q_c: they sum to -1 per row, although every p_c there is 0 in fp32
        for r in range(loss.numel()):
            assert abs(float(dblock[r, c["group_of"] == c["glabels"][r]].double().sum()) + 1.0) <= 1e-5


def test_identities(refs):
    from afft_amd import ops
    by_name = {c["name"]: c for c in groups_cases.CASES}
    # G = 1, every class grouped: lse_0 is lse -- loss 0 and gradient 0, each within its tolerance
    c = by_name["G1_all"]
    for kind in ("hard", "soft"):
        ref = refs[("G1_all", kind)]
        loss, dblock, _ = groups_cases.launch(ops, c, kind, 130, False)
        assert bool((loss.double().abs() <= C_BAR["loss_" + kind] * U * ref["s_loss"]).all()), loss
        assert bool((dblock.double().abs() <= C_BAR["grad_" + kind] * U * ref["s_grad"][:, None]).all())
    # every gradient row sums to 0: T sum_c p_c - sum_g t_g sum_{c in g} q_c = T - T
    for c in groups_cases.CASES:
        C = c["x"].shape[1]
        for kind in ("hard", "soft"):
            ref = refs[(c["name"], kind)]
            _, dblock, _ = groups_cases.launch(ops, c, kind, C, False)
            tol = C * C_BAR["grad_" + kind] * U * ref["s_grad"]
            assert bool((dblock.double().sum(1).abs() <= tol).all()), (c["name"], kind)
    # group_of = arange(C): the plain cross-entropy on the same labels
    C, rows = 257, 6
    g = groups_cases.gen(31)
    x = torch.randn(rows, C, generator=g) * 3
    labels = torch.randint(0, C, (rows,), generator=g)
    labels[2] = -1
    c = groups_cases.case("arange", x, torch.arange(C), C, labels, None)
    loss, dblock, _ = groups_cases.launch(ops, c, "hard", C, False)
    loss0, dblock0, _ = ce_cases.launch(ops.softmax_ce, x, C, labels, None, None, C, False, 1.0, None)
    ref, ref0 = double_of(c, "hard"), ce_double.ce(x, labels=labels)
    print(f"group_of = arange: equal bits with afft_softmax_ce: loss {torch.equal(loss, loss0)}, gradient {torch.equal(dblock, dblock0)}")
    tol_l = U * (C_BAR["loss_hard"] * ref["s_loss"] + SIB_BAR["loss_hard"] * ref0["s_loss"])
    tol_g = U * (C_BAR["grad_hard"] * ref["s_grad"] + SIB_BAR["grad_hard"] * ref0["s_grad"])
    assert bool(((loss.double() - loss0.double()).abs() <= tol_l).all())
    assert bool(((dblock.double() - dblock0.double()).abs() <= tol_g[:, None]).all())


@pytest.mark.parametrize("name", ["C257_G5", "sizes_1_65_300", "C3806_G300"])
def test_hard_loss_is_minus_log_of_the_marginal(name):
    """-log((softmax64(x) @ M)[y]) for the one-hot M of the mapping: what challenge.marginalize_scores ranks by"""
    from afft_amd import ops
    c = next(c for c in groups_cases.CASES if c["name"] == name)
    x, go, G, y = c["x"], c["group_of"], c["G"], c["glabels"]
    M = torch.zeros(x.shape[1], G, dtype=F64)
    M[go >= 0, go[go >= 0]] = 1.0
    c = dict(c, keep=None, gscale=1.0, row_g=None)
    loss, _, _ = groups_cases.launch(ops, c, "hard", x.shape[1], False)
    marg = torch.softmax(x.to(F64), 1) @ M
    live = y >= 0
    want = -torch.log(marg[live, y[live]])
    s = double_of(c, "hard")["s_loss"][live]
    assert bool(((loss.double()[live] - want).abs() <= C_BAR["loss_hard"] * U * s).all())
    assert bool((loss[~live] == 0).all())


@pytest.mark.parametrize("name", ["C3806_G300", "G1024", "sizes_keep"])
def test_two_runs_give_equal_bits(name):
    from afft_amd import ops
    c = next(c for c in groups_cases.CASES if c["name"] == name)
    C = c["x"].shape[1]
    for kind in ("hard", "soft"):
        a, b = (groups_cases.launch(ops, c, kind, C + 5, False) for _ in range(2))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # loss_sum: the ordered sum of the row losses
    ls = [torch.zeros(1, device=dev()) for _ in range(2)]
    groups = ops.group_csr(c["group_of"], c["G"], device=dev())
    for s in ls:
        ops.softmax_ce_groups(c["x"].to(dev()), C, groups, glabels=c["glabels"].to(dev()), keep=to_dev(c["keep"]),
                              row_loss=torch.empty(c["x"].shape[0], device=dev()), loss_sum=s)
    ref = groups_double.groups(c["x"], c["group_of"], c["G"], glabels=c["glabels"], keep=c["keep"])
    assert torch.equal(ls[0], ls[1])
    assert abs(float(ls[0]) - float(ref["loss"].sum())) <= (C_BAR["loss_hard"] + c["x"].shape[0]) * U * float(ref["s_loss"].sum())


def test_a_bad_row_is_nan_and_no_other_row_notices():
    from afft_amd import ops
    c, = groups_cases.BAD_CASES
    C, G = c["x"].shape[1], c["G"]
    clean = dict(c, glabels=c["glabels"].clone(), gsoft=c["gsoft"].clone())
    clean["glabels"][c["bad_hard"]] = 0
    clean["gsoft"][:, 3] = 0.0
    for kind in ("hard", "soft"):
        bad = torch.tensor([r in c["bad_" + kind] for r in range(c["x"].shape[0])])
        for pad, bf16 in LAYOUTS:
            l1, d1, b1 = groups_cases.launch(ops, c, kind, C + pad, bf16)
            l0, d0, b0 = groups_cases.launch(ops, clean, kind, C + pad, bf16)
            assert b0 and b1
            assert bool(torch.isnan(l1[bad]).all()) and bool(torch.isnan(d1[bad][:, :C]).all()) and bool((d1[bad][:, C:] == 0).all())
            assert torch.equal(l1[~bad], l0[~bad]) and torch.equal(d1[~bad], d0[~bad])
            assert bool(torch.isfinite(l0).all()) and bool(torch.isfinite(d0).all())
            ref = double_of(clean, kind)
            r_loss, r_grad = ratios(l0, d0, ref, C, bf16)
            assert r_loss <= C_BAR["loss_" + kind] and r_grad <= C_BAR["grad_" + kind]
            if kind == "hard":
                assert float(l1[5]) == 0.0 and bool((d1[5] == 0).all())      # the ignored row among them stays exactly 0


def test_frames_form_on_a_slice_of_a_wider_tensor():
    """afft_softmax_ce_frames_groups on frames 1..3 of a NaN-filled (2, 5, C + 8) tensor; the gradient into the same slice of a
    sentinel-filled buffer of that shape: pad columns 0, frames 0 and 4 untouched"""
    from afft_amd import ops
    C, G, clips, L = 257, 5, 2, 5
    g = groups_cases.gen(41)
    go = groups_cases.random_map(C, G, g, ungrouped=0.2)
    groups = ops.group_csr(go, G, device=dev())
    full = torch.full((clips, L, C + 8), float("nan"))
    full[:, 1:4, :C] = torch.randn(clips, 3, C, generator=g) * 3
    xd = full.to(dev())[:, 1:4, :C]
    x2 = full[:, 1:4, :C].reshape(6, C)
    gl, gs = groups_cases.targets(6, G, g)
    gl[4] = -1
    row_g = torch.randn(6, generator=g) + 0.3
    keep = torch.tensor([1, 1, 0, 1, 1, 1], dtype=torch.uint8)
    for kind, kw, ref in (("hard", dict(glabels=gl.to(dev())), groups_double.groups(x2, go, G, glabels=gl, row_g=row_g)),
                          ("soft", dict(gsoft=gs.to(dev()), keep=keep.to(dev())), groups_double.groups(x2, go, G, gsoft=gs, keep=keep, row_g=row_g))):
        dfull = torch.full((clips, L, C + 8), SENT, device=dev())
        rl = torch.full((6,), SENT, device=dev())
        ops.softmax_ce_frames_groups(xd, C, groups, row_g=row_g.to(dev()), dlogits3=dfull[:, 1:4], row_loss=rl, **kw)
        d = dfull.cpu()
        assert bool((d[:, 0] == SENT).all()) and bool((d[:, 4] == SENT).all())
        r_loss, r_grad = ratios(rl.cpu(), d[:, 1:4].reshape(6, C + 8), ref, C, False)
        print(f"frames {kind}: loss {r_loss:.3f} grad {r_grad:.3f}")
        assert r_loss <= C_BAR["loss_" + kind] and r_grad <= C_BAR["grad_" + kind]
        # the row form on a copy of the same rows: the same bits
        rl2, d2 = torch.empty(6, device=dev()), torch.empty(6, C + 8, device=dev())
        ops.softmax_ce_groups(xd.reshape(6, C), C, groups, row_g=row_g.to(dev()), dlogits=d2, row_loss=rl2, **kw)
        assert torch.equal(rl2, rl) and torch.equal(d2.cpu(), d[:, 1:4].reshape(6, C + 8))


def test_launcher_refusals_raise_and_launch_nothing():
    from afft_amd import _lib as L
    from afft_amd import ops
    rows, C, G = 4, 63, 5
    g = groups_cases.gen(51)
    go = groups_cases.random_map(C, G, g)
    x = (torch.randn(rows, C, generator=g)).to(dev())
    groups = ops.group_csr(go, G, device=dev())
    gl = torch.randint(0, G, (rows,), generator=g).to(dev())
    gs = torch.rand(rows, G, generator=g).to(dev())
    rl = torch.full((rows,), SENT, device=dev())
    d = torch.full((rows, C), SENT, device=dev())
    d3 = torch.full((1, rows, C), SENT, device=dev())
    none = ops.group_csr(torch.full((C,), -1), 0, device=dev())
    many = ops.group_csr(go, 1025, device=dev())
    limit = r"the number of groups G must lie in \[1, 1024\]"
    one_of = "give exactly one of group labels / soft group targets"
    for grp, kw, text in ((none, dict(glabels=gl), limit + r" \(got 0\)"), (many, dict(glabels=gl), limit + r" \(got 1025\)"),
                          (groups, dict(glabels=gl, gsoft=gs), one_of), (groups, dict(), one_of)):
        with pytest.raises(RuntimeError, match="softmax_ce_groups: " + text):
            ops.softmax_ce_groups(x, C, grp, row_loss=rl, dlogits=d, **kw)
        with pytest.raises(RuntimeError, match="softmax_ce_frames_groups: " + text):
            ops.softmax_ce_frames_groups(x[None], C, grp, row_loss=rl, dlogits3=d3, **kw)
    # a group_of that is not 4-byte aligned: no tensor has such an address, so the C entry is called with one
    with pytest.raises(RuntimeError, match="group_of, members and offs must be 4-byte aligned"):
        L.check(L.lib().afft_softmax_ce_groups(x.data_ptr(), C, rows, C, G, groups[0].data_ptr() + 1, groups[1].data_ptr(),
                                               groups[2].data_ptr(), gl.data_ptr(), None, 0, None, 1.0, None, None, d.data_ptr(), C, 0,
                                               rl.data_ptr(), None), "softmax_ce_groups")
    for bad in ((groups[0].long(), groups[1], groups[2]), (groups[0][:-1].contiguous(), groups[1], groups[2]),
                (groups[0].cpu(), groups[1], groups[2])):
        with pytest.raises(ValueError):
            ops.softmax_ce_groups(x, C, bad, glabels=gl, row_loss=rl, dlogits=d)
    torch.cuda.synchronize()
    assert bool((rl == SENT).all()) and bool((d == SENT).all()) and bool((d3 == SENT).all())


@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("kind", ["hard", "soft"])
def test_autograd_function_gives_the_double_s_gradient(kind, three_d):
    from afft_amd import functional as F_
    from afft_amd import ops
    c = next(c for c in groups_cases.CASES if c["name"] == "C257_G5")
    rows, C = c["x"].shape
    x = c["x"].to(dev())
    x = (x.reshape(1, rows, C) if three_d else x).requires_grad_(True)
    groups = ops.group_csr(c["group_of"], c["G"], device=dev())
    up = torch.randn(rows, generator=groups_cases.gen(61)) + 0.5      # an upstream gradient that differs per row
    args = (to_dev(c["glabels"]), None) if kind == "hard" else (None, to_dev(c["gsoft"]))
    loss = F_.SoftmaxCEGroups.apply(x, groups, *args, None)
    (loss * up.to(dev())).sum().backward()
    ref = groups_double.groups(c["x"], c["group_of"], c["G"], glabels=c["glabels"] if kind == "hard" else None,
                               gsoft=c["gsoft"] if kind == "soft" else None, row_g=up)
    got_l, got_g = loss.detach().cpu().double(), x.grad.cpu().double().reshape(rows, C)
    unit = groups_double.groups(c["x"], c["group_of"], c["G"], glabels=c["glabels"] if kind == "hard" else None,
                                gsoft=c["gsoft"] if kind == "soft" else None)
    assert bool(((got_l - unit["loss"]).abs() <= C_BAR["loss_" + kind] * U * unit["s_loss"]).all())
    # the kernel's gradient is that of row_g = 1; the product with the upstream gradient is one more rounding
    tol = C_BAR["grad_" + kind] * U * ref["s_grad"][:, None] + U * ref["grad"].abs()
    assert bool(((got_g - ref["grad"]).abs() <= tol).all())
    with torch.no_grad():
        assert torch.equal(F_.SoftmaxCEGroups.apply(x.detach(), groups, *args, None), loss.detach())      # no gradient wanted: the same loss


@pytest.mark.parametrize("mixup", [False, True])
def test_loss_accuracy_step_with_a_marginal_term(mixup):
    """BasicLossAccuracy(marginal={'verb': ...}) on a tiny output dict, through Runner._reduce_loss and backward, against a float64
    restatement of the same four terms: the row losses, the weighted total and the gradients of both logits tensors"""
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    B, T, C, G = 2, 3, 40, 7
    g = groups_cases.gen(71 + mixup)
    go = groups_cases.random_map(C, G, g, ungrouped=0.1)
    fut = (torch.randn(B, 1, C, generator=g) * 3).to(dev()).requires_grad_(True)
    past = (torch.randn(B, T, C, generator=g) * 3).to(dev()).requires_grad_(True)
    outputs = {"logits/action": {"rgb": fut}, "past_logits/action": {"rgb": past}}
    M = torch.zeros(C, G, dtype=F64)
    M[go >= 0, go[go >= 0]] = 1.0
    ign = None
    if mixup:
        tf, tp = torch.softmax(torch.randn(B, C, generator=g), -1), torch.softmax(torch.randn(B, T, C, generator=g), -1)
        ignore = torch.tensor([[False, True, False], [False, False, False]])
        ign = {"action": ignore.to(dev())}
        keep = (~ignore).reshape(-1).to(torch.uint8)
        scale = keep.numel() / float(keep.sum())
        # the module adds the soft targets up in fp32: the double takes the fp32 sums' exact values, group by group
        want = {"cls_action_rgb": ce_double.ce(fut.detach().cpu().reshape(-1, C), soft=tf),
                "marg_verb_action_rgb": groups_double.groups(fut.detach().cpu().reshape(-1, C), go, G, gsoft=tf.double() @ M),
                "past_cls_action_rgb": ce_double.ce(past.detach().cpu().reshape(-1, C), soft=tp.reshape(-1, C), keep=keep),
                "past_marg_verb_action_rgb": groups_double.groups(past.detach().cpu().reshape(-1, C), go, G,
                                                                  gsoft=tp.reshape(-1, C).double() @ M, keep=keep)}
        scales = {"cls_action_rgb": 1.0, "marg_verb_action_rgb": 1.0, "past_cls_action_rgb": scale, "past_marg_verb_action_rgb": scale}
    else:
        tf, tp = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B, T, 1), generator=g)
        tp[1, 2, 0] = -1
        glab = lambda a: torch.where(a >= 0, go[a.clamp(min=0)], a)      # noqa: E731
        want = {"cls_action_rgb": ce_double.ce(fut.detach().cpu().reshape(-1, C), labels=tf),
                "marg_verb_action_rgb": groups_double.groups(fut.detach().cpu().reshape(-1, C), go, G, glabels=glab(tf)),
                "past_cls_action_rgb": ce_double.ce(past.detach().cpu().reshape(-1, C), labels=tp.reshape(-1)),
                "past_marg_verb_action_rgb": groups_double.groups(past.detach().cpu().reshape(-1, C), go, G, glabels=glab(tp.reshape(-1)))}
        scales = dict.fromkeys(want, 1.0)
    fn = BasicLossAccuracy(compute_metrics=False, marginal={"verb": go})
    losses, _ = fn(outputs, {"action": tf.to(dev())}, {"action": tp.to(dev())}, mixup_enable=mixup, target_subclips_ignore_index=ign)
    assert list(losses) == ["cls_action_rgb", "marg_verb_action_rgb", "past_cls_action_rgb", "past_marg_verb_action_rgb"]
    kind = "soft" if mixup else "hard"
    wts = {"cls": 1.0, "past_cls": 0.5, "marg_verb": 0.75, "past_marg_verb": 0.25}
    bar = {k: (C_BAR if "marg" in k else SIB_BAR) for k in want}
    total_want, total_tol = 0.0, 0.0
    nmax = int(M.sum(0).max())
    extra = 2 + nmax if mixup else 0
    grads = {"": torch.zeros(B, C, dtype=F64), "past_": torch.zeros(B * T, C, dtype=F64)}
    gtol = {"": torch.zeros(B, C, dtype=F64), "past_": torch.zeros(B * T, C, dtype=F64)}
    for k, ref in want.items():
        got = losses[k].detach().cpu().double()
        w = next(v for p, v in wts.items() if k.startswith(p))
        # MixUp: two more roundings where the module rescales the kept rows, and a group target is an fp32 sum of up to `nmax`
        # action targets (nmax - 1 roundings of a positive sum: (nmax - 1) u t_g)
        tol = (bar[k]["loss_" + kind] + extra) * U * ref["s_loss"] * scales[k]
        assert bool(((got - ref["loss"] * scales[k]).abs() <= tol).all()), k
        n = got.numel()
        total_want += w * float(ref["loss"].sum()) * scales[k] / n
        total_tol += w * float(tol.sum()) / n + 2 * U * abs(w * float(ref["loss"].sum()) * scales[k] / n)
        half = "past_" if k.startswith("past_") else ""
        grads[half] += ref["grad"] * (w * scales[k] / n)
        # the row gradient w * scale / n is a product of fp32 roundings, and autograd adds the two terms of a tensor in fp32
        gtol[half] += (bar[k]["grad_" + kind] + extra) * U * ref["s_grad"][:, None] * (w * scales[k] / n) \
            + 4 * U * (ref["grad"] * (w * scales[k] / n)).abs()
    total, means = Runner._reduce_loss(losses, wts, sync=False)
    total.backward()
    assert abs(float(total.detach()) - total_want) <= total_tol + 4 * U * abs(total_want)
    for half, leaf in (("", fut), ("past_", past)):
        err = (leaf.grad.cpu().double().reshape(-1, C) - grads[half]).abs()
        assert bool((err <= gtol[half]).all()), (half, float((err - gtol[half]).max()))
