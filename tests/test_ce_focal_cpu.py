"""CPU: the focal exponent and the logit adjustment of the fused cross-entropy, everything but the kernel itself -- the float64 double
(tests/focal_double.py) against autograd of its own loss, against tests/ce_double.py, against torch's cross_entropy on adjusted logits
and against the textbook focal loss; the C-ABI symbols; logit_adjustment; the calls MultiDimCrossEntropy / SoftmaxCE make into
afft_amd.ops (a recording stub); the constructors of the criteria, Runner and Trainer."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import ce_cases  # noqa: E402
import ce_double  # noqa: E402
import focal_double  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
GAMMAS = [0.0, 0.5, 2.0, 5.0]


def _case(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 3.0
    labels = torch.randint(0, C, (rows,), generator=g)
    labels[::4] = -1
    soft = torch.softmax(torch.randn(rows, C, generator=g), 1) * (torch.rand(rows, C, generator=g) < 0.5)
    keep = (torch.rand(rows, generator=g) < 0.7).to(torch.uint8)
    w = torch.rand(C, generator=g) + 0.1
    w[int(labels[1])] = 0.0
    b = -8.0 * torch.rand(C, generator=g)
    row_g = torch.randn(rows, generator=g)
    return x, labels, soft, keep, w, b, row_g


def _targets(labels, soft, keep):
    return (dict(labels=labels), dict(soft=soft), dict(soft=soft, keep=keep))


# ----------------------------------------------------------------------------- the double
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("rows,C", [(9, 2), (12, 13), (5, 300)])
def test_double_gradient_is_the_derivative_of_its_loss(rows, C, eps, gamma):
    x, labels, soft, keep, w, b, row_g = _case(rows, C, 100 * rows + C)
    for kw in _targets(labels, soft, keep):
        for wt, adj in ((None, None), (w, b)):
            x64 = x.to(F64).requires_grad_(True)
            got = focal_double.focal(x64, weight=wt, eps=eps, adjust=adj, gamma=gamma, gscale=0.37, row_g=row_g, **kw)
            auto, = torch.autograd.grad((got["loss"] * 0.37 * row_g.to(F64)).sum(), x64)
            assert (got["grad"].detach() - auto).abs().max() <= 1e-12
            assert bool(torch.isfinite(got["loss"]).all()) and bool((got["loss"] >= 0).all())


def test_double_gradient_with_a_dominant_class():
    """gaps of 4, 12 and 30 between the label's logit and the rest, where 1 - p has lost its digits: the arg-max-excluded form of the
    double agrees with autograd of itself and with the closed form in r"""
    for C in (2, 257):
        for gap in (4.0, 12.0, 30.0):
            for gamma in (0.5, 2.0):
                x = torch.rand(3, C, dtype=F64)
                labels = torch.tensor([0, C - 1, C // 2])
                x[torch.arange(3), labels] += gap + 1.0
                x.requires_grad_(True)
                got = focal_double.focal(x, labels=labels, gamma=gamma)
                auto, = torch.autograd.grad(got["loss"].sum(), x)
                own, own_auto = got["grad"][torch.arange(3), labels], auto[torch.arange(3), labels]
                assert ((own - own_auto).abs() <= 1e-12 * own.abs()).all()
                xd = x.detach()
                r = torch.stack([torch.exp(xd[i][torch.arange(C) != labels[i]] - xd[i, labels[i]]).sum() for i in range(3)])
                q, l = r / (1 + r), torch.log1p(r)
                assert ((got["loss"].detach() - q ** gamma * l).abs() <= 1e-14 * got["loss"].detach()).all()
                assert bool((got["loss"] > 0).all())


@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("rows,C", [(7, 1), (9, 2), (12, 13), (5, 300)])
def test_double_without_options_is_the_weighted_double(rows, C, eps):
    x, labels, soft, keep, w, _, row_g = _case(rows, C, 10 * rows + C)
    for kw in _targets(labels, soft, keep):
        for wt in (None, w):
            got = focal_double.focal(x, weight=wt, eps=eps, gscale=0.5, row_g=row_g, **kw)
            ref = ce_double.ce(x, weight=wt, eps=eps, gscale=0.5, row_g=row_g, **kw)
            assert (got["loss"] - ref["loss"]).abs().max() <= 1e-12 * max(1.0, float(ref["loss"].abs().max()))
            assert (got["grad"] - ref["grad"]).abs().max() <= 1e-12
            assert torch.equal(got["A"], ref["A"]) and torch.equal(got["kept"], ref["kept"]) and torch.equal(got["bad"], ref["bad"])
            assert (got["s_loss"] - ref["s_loss"]).abs().max() <= 1e-12 * max(1.0, float(ref["s_loss"].max()))
            assert (got["s_grad"] - ref["s_grad"]).abs().max() <= 1e-12


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("use_w", [False, True])
@pytest.mark.parametrize("rows,C", [(9, 2), (12, 13), (5, 300)])
def test_adjustment_alone_is_torch_cross_entropy_of_the_adjusted_logits(rows, C, use_w, eps):
    x, labels, soft, keep, w, b, _ = _case(rows, C, rows + 7 * C)
    wt = w if use_w else None
    for kw in _targets(labels, soft, keep):
        got = focal_double.focal(x, weight=wt, eps=eps, adjust=b, gamma=0.0, **kw)
        loss, grad = ce_double.torch_reference(x.to(F64) + b.to(F64), weight=wt, eps=eps, **kw)
        assert (got["loss"] - loss).abs().max() <= 1e-12 * max(1.0, float(loss.abs().max()))
        assert (got["grad"] - grad).abs().max() <= 1e-12


@pytest.mark.parametrize("gamma", GAMMAS)
def test_hard_label_without_smoothing_is_the_textbook_focal_loss(gamma):
    rows, C = 12, 13
    x, labels, _, _, w, b, _ = _case(rows, C, 5)
    for wt, adj in ((None, None), (w, None), (w, b)):
        got = focal_double.focal(x, labels=labels, weight=wt, adjust=adj, gamma=gamma)
        z = x.to(F64) + (0 if adj is None else adj.to(F64))
        logp = torch.log_softmax(z, 1)
        for i in range(rows):
            y = int(labels[i])
            want = 0.0 if y == -1 else -(1.0 if wt is None else float(wt[y])) * (1.0 - float(logp[i, y].exp())) ** gamma * float(logp[i, y])
            assert abs(float(got["loss"][i]) - want) <= 1e-12 * max(1.0, abs(want))
    # a label out of range: NaN in that row alone
    lb = labels.clone()
    lb[1], lb[2] = C, -2
    bad = focal_double.focal(x, labels=lb, weight=w, adjust=b, gamma=gamma)
    clean = focal_double.focal(x, labels=labels, weight=w, adjust=b, gamma=gamma)
    assert bad["bad"].tolist() == [i in (1, 2) for i in range(rows)]
    assert torch.isnan(bad["loss"][1:3]).all() and torch.isnan(bad["grad"][1:3]).all()
    rest = ~bad["bad"]
    assert torch.equal(bad["loss"][rest], clean["loss"][rest]) and torch.equal(bad["grad"][rest], clean["grad"][rest])


def test_one_class_rows_are_zero():
    """C = 1: p = 1, q = 0, l = 0 -- loss 0 and gradient 0 for every gamma, not NaN"""
    x = torch.randn(4, 1)
    for gamma in GAMMAS:
        got = focal_double.focal(x, labels=torch.tensor([0, -1, 0, 0]), gamma=gamma, adjust=torch.tensor([-3.0]))
        assert bool((got["loss"] == 0).all()) and bool((got["grad"] == 0).all())


# ----------------------------------------------------------------------------- the C-ABI
def test_symbols_are_declared_and_exported():
    from afft_amd import _lib
    for name, sib in (("afft_softmax_ce_focal", "afft_softmax_ce_w"), ("afft_softmax_ce_frames_focal", "afft_softmax_ce_frames_w")):
        assert name in _lib.EXPORTS
        (args, res), sargs = _lib._SIGS[name], _lib._SIGS[sib][0]
        assert res is ctypes.c_int and len(args) == len(sargs) + 2
        assert args[:len(sargs) - 1] == sargs[:-1]                                  # the sibling's list ...
        assert args[-3:] == [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]      # ... then adjust, gamma, stream
    with open(os.path.join(ROOT, "include", "afft_hip.h")) as f:
        header = f.read()
    assert "int afft_softmax_ce_focal(" in header and "int afft_softmax_ce_frames_focal(" in header
    assert "const float* adjust, float gamma, void* stream);" in header
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afft_amd", "csrc"), "-j4"])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "afft_softmax_ce_focal") and hasattr(lib, "afft_softmax_ce_frames_focal")
    from afft_amd import ops
    assert callable(ops.softmax_ce_focal) and callable(ops.softmax_ce_frames_focal)


def test_wrappers_refuse_bad_arguments_before_the_library_is_called():
    from afft_amd import ops
    x = torch.randn(4, 7)
    labels = torch.zeros(4, dtype=torch.int64)
    rl = torch.empty(4)
    b = torch.zeros(7)
    bad = [dict(gamma=-0.5), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(adjust=b.double()), dict(adjust=b[:-1].clone()),
           dict(adjust=torch.zeros(14)[::2]), dict(adjust=torch.zeros(1, 7)), dict(adjust=torch.zeros(7, device="meta"))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.softmax_ce_focal(x, 7, labels=labels, row_loss=rl, **kw)
        with pytest.raises(ValueError):
            ops.softmax_ce_frames_focal(x[None], 7, labels=labels, row_loss=rl, **kw)


# ----------------------------------------------------------------------------- the adjustment from counts
def test_logit_adjustment():
    from afft_amd.common.class_weights import logit_adjustment
    counts = np.array([1000, 100, 10, 1, 0, 37], dtype=np.int64)
    b = logit_adjustment(counts)
    assert b.dtype == np.float32 and b.shape == (6,) and np.isfinite(b).all()
    total = float(counts.sum())
    want = np.log(np.array([1000, 100, 10, 1, 1, 37], dtype=np.float64) / total)        # the empty class takes the smallest count seen
    assert np.array_equal(b, want.astype(np.float32))
    assert b[4] == b[3] == b.min() and (b < 0).all()
    assert np.array_equal(logit_adjustment(counts, tau=0.5), (0.5 * want).astype(np.float32))
    assert np.array_equal(logit_adjustment(counts, tau=0.0), np.zeros(6, dtype=np.float32))
    assert np.allclose(np.exp(logit_adjustment([3, 5, 2]).astype(np.float64)), [0.3, 0.5, 0.2], rtol=1e-6)
    assert np.array_equal(logit_adjustment([0, 4, 0, 12]), np.log(np.array([4, 4, 4, 12]) / 16.0).astype(np.float32))
    for bad in (dict(counts=[1, -1]), dict(counts=[0, 0]), dict(counts=[1.0, float("nan")]), dict(counts=[]),
                dict(counts=[1, 2], tau=float("inf")), dict(counts=[1, 2], tau=float("nan"))):
        with pytest.raises(ValueError):
            logit_adjustment(**bad)


# ----------------------------------------------------------------------------- the calls into afft_amd.ops
@pytest.fixture
def rec(monkeypatch):
    return ce_cases.Recorder(monkeypatch)


@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("one_hot", [False, True])
@pytest.mark.parametrize("variant", ["gamma", "adjust", "both", "all"])
def test_options_go_to_the_focal_calls_and_give_the_double(rec, variant, one_hot, three_d):
    """focal_gamma / logit_adjust set: the _focal wrapper in forward and in backward with the same adjust tensor and gamma in both, and
    (the stub computing by the double) the double's loss and gradient through the module"""
    from afft_amd.common.runner import MultiDimCrossEntropy
    B, T, C = 6, 4, 13
    x0, labels, soft, _, w, b, _ = _case(B * T, C, 3)
    gamma = 0.0 if variant == "adjust" else 2.0
    adj = None if variant == "gamma" else b.double()          # any float type: converted at first use
    wt, eps = (w, 0.1) if variant == "all" else (None, 0.0)
    crit = MultiDimCrossEntropy(weight=wt, label_smoothing=eps, focal_gamma=gamma, logit_adjust=adj)
    assert list(crit._buffers) == ["weight"] and "logit_adjust" not in crit.state_dict()
    x = (x0.reshape(B, T, C).clone() if three_d else x0.reshape(3, 2, T, C).clone()).requires_grad_(True)
    keep = None
    if one_hot:
        ign = torch.zeros(x.shape[:-1], dtype=torch.bool)
        ign.view(-1)[3] = True
        keep = (~ign).reshape(-1).to(torch.uint8)
        loss = crit(x, soft.reshape(x.shape), one_hot=True, ignore_index=ign) * (float((~ign).sum()) / ign.numel())
    else:
        loss = crit(x, labels.reshape(x.shape[:-1]))
    loss.sum().backward()
    name = "softmax_ce_frames_focal" if three_d else "softmax_ce_focal"
    assert [c[0] for c in rec.calls] == [name, name]
    kw_f, kw_b = rec.calls[0][2], rec.calls[1][2]
    assert kw_f["gamma"] == kw_b["gamma"] == gamma and kw_f["smoothing"] == kw_b["smoothing"] == eps
    assert kw_f["adjust"] is kw_b["adjust"] and kw_f["weight"] is kw_b["weight"]
    if adj is None:
        assert kw_f["adjust"] is None
    else:
        assert kw_f["adjust"] is crit.logit_adjust and crit.logit_adjust.dtype == torch.float32 and torch.equal(crit.logit_adjust, b)
    assert "row_loss" in kw_f and ("dlogits3" if three_d else "dlogits") in kw_b and "row_g" in kw_b
    ref = focal_double.focal(x0, labels=None if one_hot else labels, soft=soft if one_hot else None, keep=keep, weight=wt, eps=eps,
                             adjust=None if adj is None else b, gamma=gamma)
    assert (loss.detach().double() - ref["loss"]).abs().max() <= 2e-6 * max(1.0, float(ref["loss"].max()))
    assert (x.grad.double().reshape(-1, C) - ref["grad"]).abs().max() <= 2e-6 * max(1.0, float(ref["grad"].abs().max()))


@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("extra,kind", [((None, None, 0.0, None, 0.0), ""), ((None, "w", 0.1, None, 0.0), "_w"),
                                        ((None, None, 0.0, "b", 0.0), "_focal"), ((None, None, 0.0, None, 2.0), "_focal"),
                                        ((None, "w", 0.1, "b", 0.5), "_focal")])
def test_gradient_slots_match_the_nine_arguments(rec, extra, kind, three_d):
    """nine arguments of apply, nine gradients back; the narrowest wrapper that serves the options is called: with adjust None and
    gamma 0 the nine-argument form makes the calls of the seven-argument one"""
    from afft_amd import functional as F_
    C = 13
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(3, 2, C, generator=g) if three_d else torch.randn(6, C, generator=g)).requires_grad_(True)
    labels = torch.randint(0, C, (6,), generator=g)
    vec = {"w": torch.rand(C) + 0.5, "b": -torch.rand(C)}
    args = tuple(vec.get(a, a) if isinstance(a, str) else a for a in extra)
    loss = F_.SoftmaxCE.apply(x, labels, None, None, *args)
    loss.sum().backward()
    assert {c[0] for c in rec.calls} == {("softmax_ce_frames" if three_d else "softmax_ce") + kind} and len(rec.calls) == 2
    assert x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all())
    with pytest.raises(AssertionError):
        F_.SoftmaxCE.apply(x, labels, None, None, None, None, 0.0, None, 0.0, None)


# ----------------------------------------------------------------------------- the constructors
def test_constructors_take_the_keywords_and_refuse_a_bad_gamma(rec):
    from afft_amd.common.runner import BasicLossAccuracy, MultiDimCrossEntropy, Runner
    from afft_amd.parallel import Trainer
    b = {"action": -torch.rand(4)}
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            MultiDimCrossEntropy(focal_gamma=bad)
        with pytest.raises(ValueError):
            BasicLossAccuracy(focal_gamma=bad)
        with pytest.raises(ValueError):
            Runner(None, torch.device("cpu"), {"cls": 1.0}, focal_gamma=bad)
    with pytest.raises(AssertionError):
        MultiDimCrossEntropy(logit_adjust=torch.zeros(3, 2))
    crit = MultiDimCrossEntropy()
    assert crit.focal_gamma == 0.0 and crit.logit_adjust is None and crit._options(torch.zeros(2, 4)) == ()
    w = torch.ones(4)
    assert MultiDimCrossEntropy(weight=w, label_smoothing=0.1)._options(torch.zeros(2, 4))[1:] == (0.1,)      # two options, as before
    opts = MultiDimCrossEntropy(focal_gamma=2.0)._options(torch.zeros(2, 4))
    assert opts == (None, 0.0, None, 2.0)
    fn = BasicLossAccuracy(compute_metrics=False, focal_gamma=2.0, logit_adjust=b, cls_weight={"verb": torch.ones(3)})
    assert set(fn.cls_criteria) == {"action", "verb"} and fn.cls_criterion.focal_gamma == 2.0 and fn.cls_criterion.logit_adjust is None
    assert torch.equal(fn.cls_criteria["action"].logit_adjust, b["action"]) and fn.cls_criteria["action"].weight is None
    assert fn.cls_criteria["verb"].logit_adjust is None and fn.cls_criteria["verb"].focal_gamma == 2.0
    r = Runner(None, torch.device("cpu"), {"cls": 1.0}, focal_gamma=1.5, logit_adjust=b)
    assert r.loss_acc_fn.cls_criteria["action"].focal_gamma == 1.5 and torch.equal(r.loss_acc_fn.cls_criteria["action"].logit_adjust, b["action"])
    r = Runner(None, torch.device("cpu"), {"cls": 1.0})
    assert len(r.loss_acc_fn.cls_criteria) == 0 and r.loss_acc_fn.cls_criterion._options(torch.zeros(2, 4)) == ()
    t = Trainer(torch.nn.Linear(4, 3), {"cls": 1.0}, focal_gamma=1.5, logit_adjust=b)
    assert t.loss_fn.cls_criteria["action"].focal_gamma == 1.5 and torch.equal(t.loss_fn.cls_criteria["action"].logit_adjust, b["action"])
    for cls in (MultiDimCrossEntropy, BasicLossAccuracy, Runner, Trainer):
        p = inspect.signature(cls.__init__).parameters
        assert p["focal_gamma"].default == 0.0 and p["logit_adjust"].default is None


def test_loss_accuracy_adjusts_the_loss_and_not_the_metrics(rec):
    """the adjusted criterion gets the SAME logits tensor the metrics get: the adjustment is an argument of the kernel call, never
    added to the logits; acc1 / acc5 equal those of a default BasicLossAccuracy"""
    from afft_amd.common.runner import BasicLossAccuracy
    B, Ca = 16, 7
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(B, 1, Ca, generator=g)
    target = {"action": torch.randint(0, Ca, (B,), generator=g)}
    b = torch.tensor([0.0, -8.0, -8.0, -8.0, -8.0, -8.0, -8.0])      # strong enough to change the arg-max of adjusted logits
    out = {"logits/action": {"rgb": logits}}
    focal = BasicLossAccuracy(focal_gamma=2.0, logit_adjust={"action": b})
    losses, metrics = focal(out, target, None)
    name, (lg, C_), kw = rec.calls[0]
    assert name.endswith("_focal") and torch.equal(lg.reshape(B, Ca), logits.reshape(B, Ca)) and torch.equal(kw["adjust"], b) and kw["gamma"] == 2.0
    rec.calls.clear()
    _, metrics0 = BasicLossAccuracy()(out, target, None)
    assert not rec.calls[0][0].endswith("_focal")
    for k in ("acc1_action_rgb", "acc5_action_rgb"):
        assert float(metrics[k]) == float(metrics0[k])
    ref = focal_double.focal(logits.reshape(B, Ca), labels=target["action"], adjust=b, gamma=2.0)
    assert (losses["cls_action_rgb"].double() - ref["loss"]).abs().max() <= 2e-6 * float(ref["loss"].max())
