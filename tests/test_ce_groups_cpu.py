"""CPU: the marginal cross-entropy over class groups, everything but the kernel itself -- the C-ABI symbols and the launcher's refusals
(they come before any HIP call), the float64 double (tests/groups_double.py) against torch's autograd on the definition
-log (softmax(x) @ M)[y], ops.group_csr, challenge.group_of_from_mapping, and -- with the double installed behind the two wrappers
(tests/cpu_ops_groups.py) -- MarginalCrossEntropy, BasicLossAccuracy / Runner and _reduce_loss."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import cpu_ops_groups  # noqa: E402
import groups_cases  # noqa: E402
import groups_double  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NAMES = ("afft_softmax_ce_groups", "afft_softmax_ce_frames_groups")


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ----------------------------------------------------------------------------- the C-ABI
@pytest.fixture(scope="module")
def lib():
    from afft_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afft_amd", "csrc"), "-j4"])
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        fn = getattr(so, name)
        fn.argtypes, fn.restype = _lib._SIGS[name]
    so.afft_last_error.argtypes, so.afft_last_error.restype = [], ctypes.c_char_p
    return so


def test_symbols_are_exported_and_bound_with_the_header_s_signature(lib):
    from afft_amd import _lib, ops
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    target = [i32, vp, vp, vp, vp, vp, i64]      # G, group_of, members, offs, glabels, gsoft, ldgs
    want = {"afft_softmax_ce_groups": [vp, i64, i32, i32] + target + [vp, f32, vp, vp, vp, i64, i32, vp, vp],
            "afft_softmax_ce_frames_groups": [vp, i64, i64, i32, i32, i32] + target + [vp, f32, vp, vp, i64, i64, i32, vp, vp]}
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert _lib._SIGS[name] == (want[name], ctypes.c_int), name
    # the sibling's list with the group description and the group targets in the place of labels / soft / lds
    sib = _lib._SIGS["afft_softmax_ce"][0]
    assert want[NAMES[0]][:4] == sib[:4] and want[NAMES[0]][11:] == sib[7:]
    assert _lib.CE_GROUPS_MAX == 1024
    assert callable(ops.softmax_ce_groups) and callable(ops.softmax_ce_frames_groups) and callable(ops.group_csr)


PTR, C, G = 0x1000, 7, 3


def call(lib, name, **over):
    """the entry with valid arguments for an EMPTY problem (the checks come first: nothing is launched or dereferenced), but for `over`"""
    a = dict(logits=PTR, clip_stride=3 * C, ldl=C, rows=0, clips=0, frames=3, C=C, G=G, group_of=PTR, members=PTR, offs=PTR, glabels=PTR,
             gsoft=None, ldgs=0, keep=None, gscale=1.0, row_g=None, loss_sum=None, dlogits=PTR, d_clip_stride=3 * C, ldd=C, d_dtype=0,
             row_loss=PTR)
    assert set(over) <= set(a), over
    a.update(over)
    head = ("logits", "clip_stride", "ldl", "clips", "frames", "C") if "frames" in name else ("logits", "ldl", "rows", "C")
    mid = ("G", "group_of", "members", "offs", "glabels", "gsoft", "ldgs", "keep", "gscale", "row_g")
    tail = ("dlogits", "d_clip_stride", "ldd", "d_dtype", "row_loss") if "frames" in name else ("loss_sum", "dlogits", "ldd", "d_dtype", "row_loss")
    rc = getattr(lib, name)(*[a[k] for k in head + mid + tail], None)
    return rc, lib.afft_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_launcher_refusals(lib, name):
    short = name[len("afft_"):]
    one_of = "give exactly one of group labels / soft group targets"
    aligned = "group_of, members and offs must be 4-byte aligned"
    bad = [(dict(G=0), "the number of groups G must lie in [1, 1024] (got 0)"),
           (dict(G=1025), "the number of groups G must lie in [1, 1024] (got 1025)"),
           (dict(G=-1), "the number of groups G must lie in [1, 1024] (got -1)"),
           (dict(logits=None), "null logits"),
           (dict(gsoft=PTR, ldgs=G), one_of), (dict(glabels=None), one_of),
           (dict(C=0), "bad sizes"), (dict(ldl=C - 1), "bad sizes"), (dict(ldd=C - 1), "bad sizes"),
           (dict(glabels=None, gsoft=PTR, ldgs=G - 1), "bad sizes"),
           (dict(group_of=None), "null group_of / offs"), (dict(offs=None), "null group_of / offs"),
           (dict(group_of=PTR + 2), aligned), (dict(members=PTR + 1), aligned), (dict(offs=PTR + 3), aligned)]
    bad.append((dict(frames=0), "bad sizes") if "frames" in name else (dict(loss_sum=PTR, row_loss=None),
                                                                       "loss_sum is the ordered sum of row_loss: give row_loss as well"))
    for over, text in bad:
        assert call(lib, name, **over) == (1, f"{short}: {text}"), over
    for ok in (dict(), dict(G=1), dict(G=1024), dict(members=None), dict(glabels=None, gsoft=PTR, ldgs=G), dict(dlogits=None, ldd=0)):
        assert call(lib, name, **ok)[0] == 0, ok


# ----------------------------------------------------------------------------- the double
def one_hot_mapping(group_of, G):
    M = torch.zeros(group_of.numel(), G, dtype=F64)
    idx = torch.nonzero(group_of >= 0).reshape(-1)
    M[idx, group_of[idx]] = 1.0
    return M


@pytest.mark.parametrize("c", [c for c in groups_cases.CASES if not c["name"].startswith(("G1024", "C3806"))], ids=lambda c: c["name"])
def test_double_is_the_definition(c):
    """-log((softmax64(x) @ M)[y]) and, for soft targets, -sum_g t_g log(softmax64(x) @ M)_g, with their gradients by autograd.
    The spread rows are left to the log-space form: softmax @ M underflows to 0 there even in float64 -- the reason for lse_g."""
    x, go, G = c["x"], c["group_of"], c["G"]
    M = one_hot_mapping(go, G)
    rg = torch.ones(x.shape[0], dtype=F64) * c["gscale"] * (1.0 if c["row_g"] is None else c["row_g"].to(F64))
    for kind, gl, gs in groups_cases.variants(c):
        got = groups_double.groups(x, go, G, glabels=gl, gsoft=gs, keep=c["keep"], gscale=c["gscale"], row_g=c["row_g"])
        assert not bool(got["bad"].any())
        xx = x.to(F64).clone().requires_grad_(True)
        live = torch.nonzero(M.sum(0) > 0).reshape(-1)      # an empty group has no logarithm; no case here puts mass on one
        if c["name"].startswith("spread"):
            lg = torch.stack([torch.logsumexp(xx[:, go == g], 1) for g in live.tolist()], 1) - torch.logsumexp(xx, 1, keepdim=True)
        else:
            lg = torch.log(torch.softmax(xx, 1) @ M[:, live])
        t = got["t"][:, live]      # the targets the double used: one-hot for hard labels, zero rows where ignored
        want = -(t * lg).sum(1)
        grad, = torch.autograd.grad((want * rg).sum(), xx)
        want = want.detach()
        assert (got["loss"] - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max())), (c["name"], kind)
        assert (got["grad"] - grad).abs().max() <= 1e-12 * max(1.0, float(rg.abs().max())), (c["name"], kind)
        assert bool((got["loss"][~got["kept"]] == 0).all()) and bool((got["grad"][~got["kept"]] == 0).all())
    if c["name"].startswith("spread"):
        assert bool((got["loss"] > 170).all()) and bool(torch.isfinite(got["loss"]).all())      # about 0.75 * 240


def test_double_marks_bad_rows_and_only_them():
    c, = groups_cases.BAD_CASES
    for kind, gl, gs in groups_cases.variants(c):
        got = groups_double.groups(c["x"], c["group_of"], c["G"], glabels=gl, gsoft=gs)
        bad = c["bad_" + kind]
        assert torch.nonzero(got["bad"]).reshape(-1).tolist() == bad
        assert bool(torch.isnan(got["loss"][bad]).all()) and bool(torch.isnan(got["grad"][bad]).all())
        rest = ~got["bad"]
        assert bool(torch.isfinite(got["loss"][rest]).all()) and bool(torch.isfinite(got["grad"][rest]).all())
    hard = groups_double.groups(c["x"], c["group_of"], c["G"], glabels=c["glabels"])
    assert int(c["glabels"][5]) == -1 and float(hard["loss"][5]) == 0.0 and bool((hard["grad"][5] == 0).all())      # ignored, not bad


# ----------------------------------------------------------------------------- host helpers
def test_group_csr():
    from afft_amd import ops
    go = torch.tensor([2, 0, -1, 2, 4, 0, 2, -1])      # group 1 and group 3 are empty
    group_of, members, offs = ops.group_csr(go)
    assert group_of.dtype == members.dtype == offs.dtype == torch.int32
    assert group_of.tolist() == go.tolist()
    assert members.tolist() == [1, 5, 0, 3, 6, 4]      # group by group, ascending inside a group
    assert offs.tolist() == [0, 2, 2, 5, 5, 6]
    assert ops.group_csr(go, 7)[2].tolist() == [0, 2, 2, 5, 5, 6, 6, 6]      # trailing empty groups
    assert ops.group_csr(go.to(torch.int32))[1].tolist() == members.tolist()
    none = ops.group_csr(torch.full((4,), -1))
    assert none[1].numel() == 0 and none[2].tolist() == [0]
    for c in groups_cases.CASES:
        gof, mem, off = ops.group_csr(c["group_of"], c["G"])
        assert off.numel() == c["G"] + 1 and int(off[-1]) == mem.numel() == int((c["group_of"] >= 0).sum())
        for g in (0, c["G"] // 2, c["G"] - 1):
            assert mem[int(off[g]):int(off[g + 1])].tolist() == torch.nonzero(c["group_of"] == g).reshape(-1).tolist()
    for bad in (torch.tensor([0, 3]), torch.tensor([0, -2])):
        with pytest.raises(ValueError, match=r"values in \[-1, "):
            ops.group_csr(bad, 3)
    with pytest.raises(ValueError, match="integer type"):
        ops.group_csr(torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError, match="integer type"):
        ops.group_csr(torch.zeros(2, 2, dtype=torch.int64))


def test_group_of_from_mapping():
    from afft_amd.challenge import group_of_from_mapping
    M = torch.zeros(5, 3)
    M[0, 2] = M[1, 0] = M[3, 0] = M[4, 1] = 1.0      # row 2 is all zero
    got = group_of_from_mapping(M)
    assert got.dtype == torch.int64 and got.tolist() == [2, 0, -1, 0, 1]
    assert group_of_from_mapping(M.numpy()).tolist() == got.tolist()
    assert torch.equal(one_hot_mapping(got, 3), (M != 0).to(F64))
    M[3, 1] = 1.0
    with pytest.raises(ValueError, match="class 3 maps to 2 groups"):
        group_of_from_mapping(M)
    with pytest.raises(ValueError):
        group_of_from_mapping(torch.zeros(5))


# ----------------------------------------------------------------------------- the module, with the double behind the wrappers
A_, G_ = 13, 4
GO = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3, -1, 0, 0, 1, 3])


def test_module_maps_hard_labels_and_keeps_minus_one():
    from afft_amd.common.runner import MarginalCrossEntropy
    crit = MarginalCrossEntropy(GO)
    assert crit.num_groups == G_ and list(crit.state_dict()) == []
    labels = torch.tensor([[0, 5, -1], [8, 12, 3]])      # class 8 is in no group: ignored like -1
    with cpu_ops_groups.installed() as calls:
        for three_d in (True, False):
            x = (rnd(2, 3, A_, seed=1) if three_d else rnd(2, 3, 1, A_, seed=1)).requires_grad_(True)
            loss = crit(x, labels)
            (loss * torch.arange(1.0, 7.0)).sum().backward()
            name, (lg, C_, groups), kw = calls[-1]
            assert name == ("softmax_ce_frames_groups" if three_d else "softmax_ce_groups") and C_ == A_ and lg.dim() == (3 if three_d else 2)
            assert kw["glabels"].tolist() == [0, 1, -1, -1, 3, 3] and kw["gsoft"] is None and kw["keep"] is None
            assert groups[0].tolist() == GO.tolist() and groups[2].numel() == G_ + 1
            want = groups_double.groups(x.detach().reshape(6, A_), GO, G_, glabels=kw["glabels"], row_g=torch.arange(1.0, 7.0))
            assert (loss.detach().double() - want["loss"]).abs().max() <= 1e-6 and loss.shape == (6,)
            assert (x.grad.reshape(6, A_).double() - want["grad"]).abs().max() <= 1e-5
            assert loss.detach()[2:4].tolist() == [0.0, 0.0] and bool((x.grad.reshape(6, A_)[2:4] == 0).all())
        assert len(calls) == 2      # forward and gradient in ONE call each
        # an action label out of range stays out of range as a group label
        crit(rnd(2, 3, A_, seed=1), torch.tensor([[0, A_, -2], [1, 2, 3]]))
        assert calls[-1][2]["glabels"].tolist() == [0, G_, G_, 1, 2, 3]


def test_module_sums_soft_targets_by_group_and_renormalises_kept_rows():
    from afft_amd.common.runner import MarginalCrossEntropy
    crit = MarginalCrossEntropy(GO)
    g = torch.Generator().manual_seed(3)
    soft = torch.softmax(torch.randn(2, 3, A_, generator=g), -1)
    soft[..., 8] = 0.0                                  # all mass on grouped classes: the group targets keep the sum
    ign = torch.tensor([[False, True, False], [False, False, True]])
    x = rnd(2, 3, A_, seed=4).requires_grad_(True)
    with cpu_ops_groups.installed() as calls:
        loss = crit(x, soft, one_hot=True, ignore_index=ign)
        loss.sum().backward()
        plain = crit(x.detach(), soft, one_hot=True)
    _, (lg, C_, groups), kw = calls[0]
    gs = kw["gsoft"]
    assert gs.shape == (6, G_) and kw["glabels"] is None and kw["keep"].tolist() == [1, 0, 1, 1, 1, 0]
    assert (gs.sum(1) - soft.reshape(6, A_).sum(1)).abs().max() <= 1e-6
    want_t = soft.reshape(6, A_).double() @ one_hot_mapping(GO, G_)
    assert (gs.double() - want_t).abs().max() <= 1e-6
    want = groups_double.groups(x.detach().reshape(6, A_), GO, G_, gsoft=gs, keep=kw["keep"])
    # the reference drops ignored rows before the mean: here they are 0 and the kept rows carry rows / kept
    assert (loss.detach().double() - want["loss"] * (6 / 4)).abs().max() <= 1e-6
    assert abs(float(loss.mean()) - float(want["loss"][want["kept"]].mean())) <= 1e-6
    assert (x.grad.reshape(6, A_).double() - want["grad"] * (6 / 4)).abs().max() <= 1e-5
    assert calls[1][2]["keep"] is None and plain.shape == (6,)
    # mass on an ungrouped class is left out
    soft2 = torch.zeros(1, 1, A_)
    soft2[0, 0, 8], soft2[0, 0, 1] = 0.6, 0.4
    with cpu_ops_groups.installed() as calls:
        crit(rnd(1, 1, A_, seed=5), soft2, one_hot=True)
    assert calls[0][2]["gsoft"].tolist() == [[0.0, pytest.approx(0.4), 0.0, 0.0]]


def _outputs(B=3, T=2, Cv=5, seed=0):
    out = {"logits/action": {"rgb": rnd(B, 1, A_, seed=seed + 1).requires_grad_(True)}, "logits/verb": {"rgb": rnd(B, 1, Cv, seed=seed + 2)},
           "past_logits/action": {"rgb": rnd(B, T, A_, seed=seed + 3).requires_grad_(True)}, "past_logits/verb": {"rgb": rnd(B, T, Cv, seed=seed + 4)}}
    g = torch.Generator().manual_seed(seed + 5)
    target = {"action": torch.randint(0, A_, (B,), generator=g), "verb": torch.randint(0, Cv, (B,), generator=g)}
    past = {"action": torch.randint(-1, A_, (B, T, 1), generator=g), "verb": torch.randint(0, Cv, (B, T, 1), generator=g)}
    return out, target, past


TODAY = {"cls_action_rgb", "past_cls_action_rgb", "cls_verb_rgb", "past_cls_verb_rgb"}


def test_default_is_today_s_losses_and_no_call_of_the_new_ops():
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    out, target, past = _outputs()
    with cpu_ops_groups.installed() as calls:
        for fn in (BasicLossAccuracy(compute_metrics=False), BasicLossAccuracy(compute_metrics=False, marginal=None),
                   BasicLossAccuracy(compute_metrics=False, marginal={}),
                   Runner(None, torch.device("cpu"), {"cls": 1.0, "past": 1.0}, compute_metrics=False).loss_acc_fn):
            assert fn.marginal is None and list(fn.state_dict()) == []
            losses, _ = fn(out, target, past)
            assert list(losses) == ["cls_action_rgb", "past_cls_action_rgb", "cls_verb_rgb", "past_cls_verb_rgb"]
        assert calls == []


def test_marginal_adds_its_keys_for_the_action_type_only():
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    out, target, past = _outputs()
    GO2 = (GO + 1) % 3
    r = Runner(None, torch.device("cpu"), {}, compute_metrics=False, marginal={"verb": GO, "noun": GO2})
    fn = r.loss_acc_fn
    assert list(fn.marginal) == ["verb", "noun"] and list(fn.state_dict()) == []
    with cpu_ops_groups.installed() as calls:
        losses, _ = fn(out, target, past)
        new = {"marg_verb_action_rgb", "marg_noun_action_rgb", "past_marg_verb_action_rgb", "past_marg_noun_action_rgb"}
        assert set(losses) == TODAY | new
        assert [c[0] for c in calls] == ["softmax_ce_frames_groups"] * 4
        x, lab = out["logits/action"]["rgb"].detach().reshape(-1, A_), target["action"]
        want = groups_double.groups(x, GO2, 3, glabels=GO2[lab])
        assert (losses["marg_noun_action_rgb"].detach().double() - want["loss"]).abs().max() <= 1e-6
        xp, labp = out["past_logits/action"]["rgb"].detach().reshape(-1, A_), past["action"].reshape(-1)
        glab = torch.where(labp >= 0, GO[labp.clamp(min=0)], labp)
        want = groups_double.groups(xp, GO, G_, glabels=glab)
        assert (losses["past_marg_verb_action_rgb"].detach().double() - want["loss"]).abs().max() <= 1e-6
        # _reduce_loss finds the weights by prefix, drops nothing silently, and weighs what it finds
        wts = {"cls": 1.0, "past_cls": 0.5, "marg_verb": 0.25, "marg_noun": 0.125, "past_marg": 2.0}
        total, means = Runner._reduce_loss(losses, wts, sync=False)
        by_hand = sum(w * float(losses[k].mean()) for k in losses for p, w in wts.items() if k.startswith(p))
        assert abs(float(total) - by_hand) <= 1e-5 * abs(by_hand) and set(means) == set(losses)
        total.backward()
        assert out["logits/action"]["rgb"].grad is not None and out["past_logits/action"]["rgb"].grad is not None
        with pytest.raises(ValueError, match="marg_verb_action_rgb not contained in predefined loss_wts"):
            Runner._reduce_loss(losses, {"cls": 1.0, "past": 1.0}, sync=False)


def test_marginal_with_mixup_targets_and_ignored_past_frames():
    from afft_amd.common.runner import BasicLossAccuracy
    B, T = 3, 2
    out, _, _ = _outputs(B, T)
    out = {k: v for k, v in out.items() if "action" in k}
    g = torch.Generator().manual_seed(9)
    target = {"action": torch.softmax(torch.randn(B, A_, generator=g), -1)}
    past = {"action": torch.softmax(torch.randn(B, T, A_, generator=g), -1)}
    ign = {"action": torch.tensor([[False, True], [False, False], [True, False]])}
    fn = BasicLossAccuracy(compute_metrics=False, marginal={"verb": GO})
    with cpu_ops_groups.installed() as calls:
        losses, _ = fn(out, target, past, mixup_enable=True, target_subclips_ignore_index=ign)
    assert list(losses) == ["cls_action_rgb", "marg_verb_action_rgb", "past_cls_action_rgb", "past_marg_verb_action_rgb"]
    M = one_hot_mapping(GO, G_)
    want = groups_double.groups(out["past_logits/action"]["rgb"].detach().reshape(-1, A_), GO, G_,
                                gsoft=past["action"].reshape(-1, A_).double() @ M, keep=(~ign["action"]).reshape(-1).to(torch.uint8))
    assert (losses["past_marg_verb_action_rgb"].detach().double() - want["loss"] * (6 / 4)).abs().max() <= 1e-5
    assert [c[2]["keep"] is None for c in calls] == [True, False]
