"""CPU: class weights and label smoothing of the fused cross-entropy, everything but the kernel itself -- the C-ABI symbols, the
float64 double (tests/ce_double.py) against torch and against the fixture made from the reference's criterion
(tests/golden/c0_weighted_ce.npz), the calls MultiDimCrossEntropy / SoftmaxCE make into afft_amd.ops (a recording stub), the gradient
slots of SoftmaxCE, class_weights, and BasicLossAccuracy's choice of weights by target type."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import ce_cases  # noqa: E402
import ce_double  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "c0_weighted_ce.npz")


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    return {k: z[k] for k in z.files if k != "meta"}, meta


# ----------------------------------------------------------------------------- the C-ABI
def test_symbols_are_declared_and_exported():
    from afft_amd import _lib
    want = {"afft_softmax_ce": 16, "afft_softmax_ce_w": 18, "afft_softmax_ce_frames": 18, "afft_softmax_ce_frames_w": 20}
    for name, nargs in want.items():
        assert name in _lib.EXPORTS
        args, res = _lib._SIGS[name]
        assert len(args) == nargs and res is ctypes.c_int, (name, len(args))
    for name, sib in (("afft_softmax_ce_w", "afft_softmax_ce"), ("afft_softmax_ce_frames_w", "afft_softmax_ce_frames")):
        args, sargs = _lib._SIGS[name][0], _lib._SIGS[sib][0]
        assert args[:len(sargs) - 1] == sargs[:-1]                                  # the sibling's list ...
        assert args[-3:] == [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]      # ... then weight, smoothing, stream
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afft_amd", "csrc"), "-j4"])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "afft_softmax_ce_w") and hasattr(lib, "afft_softmax_ce_frames_w")
    from afft_amd import ops
    assert callable(ops.softmax_ce_w) and callable(ops.softmax_ce_frames_w)


# ----------------------------------------------------------------------------- the double
def _case(rows, C, seed, zero_w=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 3.0
    labels = torch.randint(0, C, (rows,), generator=g)
    labels[::4] = -1
    soft = torch.softmax(torch.randn(rows, C, generator=g), 1) * (torch.rand(rows, C, generator=g) < 0.5)
    keep = (torch.rand(rows, generator=g) < 0.7).to(torch.uint8)
    w = torch.rand(C, generator=g) + 0.1
    if zero_w:
        w[int(labels[1])] = 0.0
    return x, labels, soft, keep, w


@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("use_w", [False, True])
@pytest.mark.parametrize("rows,C", [(7, 1), (9, 2), (12, 13), (5, 300)])
def test_double_matches_torch(rows, C, use_w, eps):
    x, labels, soft, keep, w = _case(rows, C, rows * 1000 + C)
    w = w if use_w else None
    for kw in (dict(labels=labels), dict(soft=soft), dict(soft=soft, keep=keep)):
        got = ce_double.ce(x, weight=w, eps=eps, **kw)
        loss, grad = ce_double.torch_reference(x, weight=w, eps=eps, **kw)
        assert (got["loss"] - loss).abs().max() <= 1e-12 * max(1.0, float(loss.abs().max()))
        assert (got["grad"] - grad).abs().max() <= 1e-12
    # a label out of range (torch raises there): NaN in that row alone; the other rows as without it
    if C > 1:
        clean = ce_double.ce(x, labels=labels, weight=w, eps=eps)
        lb = labels.clone()
        lb[1], lb[2] = C, -2
        got = ce_double.ce(x, labels=lb, weight=w, eps=eps)
        assert got["bad"].tolist() == [i in (1, 2) for i in range(rows)]
        assert torch.isnan(got["loss"][1:3]).all() and torch.isnan(got["grad"][1:3]).all()
        rest = ~got["bad"]
        assert torch.equal(got["loss"][rest], clean["loss"][rest]) and torch.equal(got["grad"][rest], clean["grad"][rest])


def test_double_matches_the_reference_fixture(golden):
    arr, meta = golden
    assert arr["logits"].shape == (6, 4, 13) and arr["logits"].dtype == np.float32 and arr["hard_ws_grad"].dtype == np.float64
    assert (arr["labels"] == -1).any() and arr["ignore"].any() and int((arr["weight"] == 0).sum()) == 1 and meta["eps"] == 0.1
    C = arr["logits"].shape[-1]
    x = torch.from_numpy(arr["logits"]).reshape(-1, C)
    labels = torch.from_numpy(arr["labels"]).reshape(-1)
    soft = torch.from_numpy(arr["soft"]).reshape(-1, C)
    keep = torch.from_numpy(~arr["ignore"]).reshape(-1).to(torch.uint8)
    for name, v in meta["variants"].items():
        w = torch.from_numpy(arr["weight"]) if v["weight"] else None
        for kind, kw in (("hard", dict(labels=labels)), ("soft", dict(soft=soft, keep=keep))):
            got = ce_double.ce(x, weight=w, eps=v["smoothing"], **kw)
            assert np.abs(got["loss"].numpy() - arr[f"{kind}_{name}_loss"]).max() <= 1e-12, (kind, name)
            assert np.abs(got["grad"].numpy().reshape(6, 4, C) - arr[f"{kind}_{name}_grad"]).max() <= 1e-12, (kind, name)


# ----------------------------------------------------------------------------- the calls into afft_amd.ops
@pytest.fixture
def rec(monkeypatch):
    return ce_cases.Recorder(monkeypatch)


def _leaf(x, three_d):
    """logits as a leaf: 3-D fp32 with contiguous classes is walked in place, a non-collapsing 4-D view is flattened to rows"""
    return (x.clone() if three_d else x.clone().reshape(3, 2, 4, -1)).requires_grad_(True)


@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("one_hot", [False, True])
def test_defaults_make_the_old_calls_with_the_old_arguments(rec, three_d, one_hot):
    from afft_amd.common.runner import MultiDimCrossEntropy
    C = 13
    x = _leaf(rnd(6, 4, C, seed=1), three_d)
    crit = MultiDimCrossEntropy()
    assert crit.weight is None and crit.label_smoothing == 0.0 and list(crit._buffers) == ["weight"]
    if one_hot:
        tgt = torch.softmax(rnd(*x.shape, seed=2), -1)
        ign = torch.zeros(x.shape[:-1], dtype=torch.bool)
        ign.view(-1)[3] = True
        loss = crit(x, tgt, one_hot=True, ignore_index=ign)
    else:
        tgt = torch.randint(0, C, x.shape[:-1], generator=torch.Generator().manual_seed(3))
        loss = crit(x, tgt)
    loss.sum().backward()
    name = "softmax_ce_frames" if three_d else "softmax_ce"
    assert [c[0] for c in rec.calls] == [name, name]
    (_, (lg_f, C_f), kw_f), (_, (lg_b, C_b), kw_b) = rec.calls
    assert C_f == C_b == C and lg_f.dim() == (3 if three_d else 2) and lg_b.shape == lg_f.shape
    assert set(kw_f) == {"labels", "soft", "keep", "row_loss"}                                        # exactly the arguments of before
    assert set(kw_b) == {"labels", "soft", "keep", "row_g", "dlogits3" if three_d else "dlogits"}
    assert (kw_f["labels"] is None) == one_hot and (kw_f["soft"] is None) != one_hot and (kw_f["keep"] is None) != one_hot
    assert x.grad is not None and x.grad.shape == x.shape


@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("one_hot", [False, True])
@pytest.mark.parametrize("variant", ["w", "s", "ws"])
def test_options_go_to_the_w_calls_and_match_the_fixture(rec, golden, variant, one_hot, three_d):
    """with weight / label_smoothing set: the _w wrapper in forward and in backward, the same weight tensor and smoothing in both, and
    (the stub computing by the double) the fixture's loss and gradient through the module, the keep rescaling undone"""
    from afft_amd.common.runner import MultiDimCrossEntropy
    arr, meta = golden
    v = meta["variants"][variant]
    w64 = torch.from_numpy(arr["weight"]).double() if v["weight"] else None      # any float type: converted at first use
    crit = MultiDimCrossEntropy(weight=w64, label_smoothing=v["smoothing"])
    assert (crit.weight is None) == (w64 is None) and list(crit._buffers) == ["weight"]
    C = arr["logits"].shape[-1]
    x = _leaf(torch.from_numpy(arr["logits"]), three_d)
    kind = "soft" if one_hot else "hard"
    if one_hot:
        ign = torch.from_numpy(arr["ignore"]).reshape(x.shape[:-1])
        loss = crit(x, torch.from_numpy(arr["soft"]).reshape(x.shape), one_hot=True, ignore_index=ign)
        loss = loss * (float((~ign).sum()) / ign.numel())
    else:
        loss = crit(x, torch.from_numpy(arr["labels"]).reshape(x.shape[:-1]))
    loss.sum().backward()
    name = "softmax_ce_frames_w" if three_d else "softmax_ce_w"
    assert [c[0] for c in rec.calls] == [name, name]
    kw_f, kw_b = rec.calls[0][2], rec.calls[1][2]
    assert kw_f["smoothing"] == kw_b["smoothing"] == v["smoothing"]
    assert kw_f["weight"] is kw_b["weight"]
    if v["weight"]:
        assert kw_f["weight"] is crit.weight and crit.weight.dtype == torch.float32 and crit.weight.is_contiguous()
        assert torch.equal(crit.weight, torch.from_numpy(arr["weight"]))
    else:
        assert kw_f["weight"] is None
    assert "row_loss" in kw_f and ("dlogits3" if three_d else "dlogits") in kw_b and "row_g" in kw_b
    assert np.abs(loss.detach().double().numpy() - arr[f"{kind}_{variant}_loss"]).max() <= 2e-6
    assert np.abs(x.grad.double().numpy().reshape(6, 4, C) - arr[f"{kind}_{variant}_grad"]).max() <= 2e-6


@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("extra", [(), (None,), (None, None, 0.0), (None, "w", 0.0), (None, None, 0.1), (None, "w", 0.1)])
def test_gradient_slots_match_the_arguments_passed(rec, extra, three_d):
    """autograd refuses a backward that returns another number of gradients than apply took arguments: four (landing defaulted), five
    (every call site of before) and seven; (None, None, 0.0) is seven arguments and still the plain call"""
    from afft_amd import functional as F_
    C = 13
    x = (rnd(3, 2, C, seed=5) if three_d else rnd(6, C, seed=5)).requires_grad_(True)
    labels = torch.randint(0, C, (6,), generator=torch.Generator().manual_seed(6))
    w = torch.rand(C) + 0.5
    args = tuple(w if a == "w" else a for a in extra) if extra else ()
    loss = F_.SoftmaxCE.apply(x, labels, None, None, *args)
    loss.sum().backward()
    plain = len(extra) < 3 or (extra[1] is None and extra[2] == 0.0)
    names = {c[0] for c in rec.calls}
    assert names == {("softmax_ce_frames" if three_d else "softmax_ce") + ("" if plain else "_w")} and len(rec.calls) == 2
    assert x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all())
    with pytest.raises(AssertionError):
        F_.SoftmaxCE.apply(x, labels, None, None, None, None, 0.0, None)


def test_constructor_refuses_what_the_kernel_would():
    from afft_amd.common.runner import MultiDimCrossEntropy
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            MultiDimCrossEntropy(label_smoothing=bad)
    with pytest.raises(AssertionError):
        MultiDimCrossEntropy(weight=torch.ones(3, 2))
    with pytest.raises(AssertionError):
        MultiDimCrossEntropy(reduction='mean')


# ----------------------------------------------------------------------------- weights from counts
def test_class_weights():
    from afft_amd.common.class_weights import class_weights
    counts = np.array([1000, 100, 10, 1, 0, 37], dtype=np.int64)
    n = counts.astype(np.float64)
    for kw in (dict(), dict(power=0.5), dict(scheme='effective'), dict(scheme='effective', beta=0.99), dict(power=0.0)):
        w = class_weights(counts, **kw)
        assert w.dtype == np.float64 and w.shape == (6,)
        assert w[4] == 0.0 and (w[counts > 0] > 0).all()                                 # no samples: weight 0
        assert abs(np.dot(n, w) / n.sum() - 1.0) <= 1e-12                                # the count-weighted mean weight is 1
    seen = counts > 0
    w = class_weights(counts)
    raw = np.where(seen, 1.0 / np.maximum(n, 1), 0.0)
    assert np.allclose(w, raw * n.sum() / np.dot(n, raw), rtol=1e-13, atol=0)
    assert np.allclose(w[0] / w[1], 0.1, rtol=1e-13) and np.allclose(class_weights(counts, power=0.5)[0] / class_weights(counts, power=0.5)[2], 0.1)
    e = class_weights(counts, scheme='effective', beta=0.99)
    raw = np.where(seen, (1 - 0.99) / (1 - 0.99 ** np.maximum(n, 1)), 0.0)
    assert np.allclose(e, raw * n.sum() / np.dot(n, raw), rtol=1e-12, atol=0)
    assert e[3] > e[2] > e[1] > e[0]                                                     # rarer is heavier, and it saturates:
    assert e[3] / e[0] < 1 / 0.01 < w[3] / w[0]
    assert np.array_equal(class_weights(counts, power=0.0), seen.astype(np.float64) * 1.0)      # power 0: all ones (0 where unseen)
    assert np.array_equal(class_weights([3, 5, 2], power=0.0), np.ones(3))
    assert np.allclose(class_weights([5, 5, 5], scheme='effective'), np.ones(3), rtol=1e-13)
    for bad in (dict(counts=[1, -1]), dict(counts=[0, 0]), dict(counts=[1, 2], scheme='focal'), dict(counts=[1, 2], scheme='effective', beta=1.0)):
        with pytest.raises(ValueError):
            class_weights(**bad)


# ----------------------------------------------------------------------------- BasicLossAccuracy / Runner / Trainer
def test_loss_accuracy_picks_the_weight_by_target_type(rec):
    """one criterion per target type, for its future and its past term; a type without weights gets none (smoothing still applies)"""
    from afft_amd.common.runner import BasicLossAccuracy
    B, T, Ca, Cv = 3, 2, 7, 5
    wa = torch.rand(Ca) + 0.5
    fn = BasicLossAccuracy(compute_metrics=False, cls_weight={"action": wa}, label_smoothing=0.1)
    outputs = {"logits/action": {"rgb": rnd(B, 1, Ca, seed=1).requires_grad_(True)}, "logits/verb": {"rgb": rnd(B, 1, Cv, seed=2)},
               "past_logits/action": {"rgb": rnd(B, T, Ca, seed=3)}, "past_logits/verb": {"rgb": rnd(B, T, Cv, seed=4)}}
    g = torch.Generator().manual_seed(5)
    target = {"action": torch.randint(0, Ca, (B,), generator=g), "verb": torch.randint(0, Cv, (B,), generator=g)}
    past = {"action": torch.randint(0, Ca, (B, T, 1), generator=g), "verb": torch.randint(0, Cv, (B, T, 1), generator=g)}
    losses, _ = fn(outputs, target, past)
    assert set(losses) == {"cls_action_rgb", "past_cls_action_rgb", "cls_verb_rgb", "past_cls_verb_rgb"}
    by_C = {}
    for name, (lg, C_), kw in rec.calls:
        assert name.endswith("_w") and kw["smoothing"] == 0.1
        by_C.setdefault(C_, []).append(kw["weight"])
    assert len(by_C[Ca]) == 2 and all(w is fn.cls_criteria["action"].weight for w in by_C[Ca]) and torch.equal(by_C[Ca][0], wa)
    assert by_C[Cv] == [None, None]
    # the defaults: one plain criterion, the plain calls
    rec.calls.clear()
    fn = BasicLossAccuracy(compute_metrics=False)
    assert len(fn.cls_criteria) == 0 and fn.cls_criterion.weight is None and fn.cls_criterion.label_smoothing == 0.0
    fn(outputs, target, past)
    assert len(rec.calls) == 4 and all(not c[0].endswith("_w") for c in rec.calls)


def test_runner_and_trainer_take_the_two_arguments():
    import inspect
    from afft_amd.common.runner import Runner
    from afft_amd.parallel import Trainer
    w = {"action": torch.ones(4)}
    r = Runner(None, torch.device("cpu"), {"cls": 1.0}, cls_weight=w, label_smoothing=0.2)
    assert torch.equal(r.loss_acc_fn.cls_criteria["action"].weight, w["action"]) and r.loss_acc_fn.cls_criterion.label_smoothing == 0.2
    r = Runner(None, torch.device("cpu"), {"cls": 1.0})
    assert len(r.loss_acc_fn.cls_criteria) == 0 and r.loss_acc_fn.cls_criterion.label_smoothing == 0.0
    t = Trainer(torch.nn.Linear(4, 3), {"cls": 1.0}, cls_weight=w, label_smoothing=0.2)
    assert torch.equal(t.loss_fn.cls_criteria["action"].weight, w["action"]) and t.loss_fn.cls_criterion.label_smoothing == 0.2
    for cls in (Runner, Trainer):
        p = inspect.signature(cls.__init__).parameters
        assert p["cls_weight"].default is None and p["label_smoothing"].default == 0.0
