"""The call-by-call path of the three sub-layer Functions (AttnSublayer, MLPSublayer, CrossAttnSublayer), driven through `apply` directly:
every output and the gradient of EVERY tensor argument against a float64 plain-torch restatement of the sub-layer under torch.autograd.
The whole-model goldens never have every argument live, so only this file pins that each returned gradient lands on its own argument.

Shapes: nseq = 3, L = 4, H = 2, d = 16, MLP hidden = 40, cross-attention memory width 24 -- the smallest at which two arguments cannot be
mixed up unseen; every tensor is drawn from a seed of its own.  The two two-sub-layer cells use d = 64 (hidden 128): the gradient
hand-over is only planned for widths that are multiples of 64 (functional._plan_handover), so that is the smallest width at which it
can be accepted or turned down at all.

CPU (tests/cpu_ops.py stands in for afft_amd.ops; precision fp32): rel_l2 < 2e-4, the bound of test_host_logic_cpu.py for the fp32 host
wiring.  GPU (runtime.set_composite(False); fp32 and bf16): the bounds of test_model_gpu.py for model outputs and gradients, imported.
The bf16 output-dropout cells have no float64 statement (the mask is the kernel's); they are held to the call-by-call result of the
build BEFORE the shared driver, recorded in tests/golden/cbc_dropout.npz by tests/golden/make_golden_cbc_dropout.py."""
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

import cpu_ops
from helpers import GOLDEN, rel_l2

NSEQ, L, H, D, HIDDEN, MEM = 3, 4, 2, 16, 40, 24
EPS = 1e-6
CPU_TOL = 2e-4      # test_host_logic_cpu.py::test_host_wiring_reproduces_reference_golden, fp32
DROP_P, DROP_KEY = 0.3, 0x5EED1234


def _t(seed, *shape, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(*shape, generator=g) * scale + shift


MASKS = ["none", "causal", "blockcausal", "table", "bias_grad", "bias_nograd"]


def _mask_tensor(kind):
    """the additive tensor of the tensor masks; no row is hidden entirely"""
    if kind == "table":
        t = _t(90, L, L)
        t[0, 3] = t[1, 2] = t[3, 0] = float("-inf")
        return t
    return _t(91, NSEQ, 1, L, L)


def _additive(kind, tensor):
    """float64 additive mask that broadcasts to (nseq, H, L, L): this file's own statement of the mask kinds"""
    i = torch.arange(L)
    if kind == "none":
        return torch.zeros(L, L, dtype=torch.float64)
    if kind == "causal":
        return torch.where(i[None, :] > i[:, None], float("-inf"), 0.0).double()
    if kind == "blockcausal":
        return torch.where((i[None, :] % 2) > (i[:, None] % 2), float("-inf"), 0.0).double()
    return tensor


# --------------------------------------------------------------------------- cells
def _cells():
    out = []
    for pre_ln, conv1d, biases, gm, mask in itertools.product((True, False), (False, True), (True, False), ("sink", "autograd"), MASKS):
        out.append(dict(fn="attn", pre_ln=pre_ln, conv1d=conv1d, biases=biases, grad_mode=gm, mask=mask))
    for pre_ln, conv1d, biases, gm in itertools.product((True, False), (False, True), (True, False), ("sink", "autograd")):
        out.append(dict(fn="mlp", pre_ln=pre_ln, conv1d=conv1d, biases=biases, grad_mode=gm))
    for pre_ln, biases, gm, mask, edge in itertools.product((True, False), (True, False), ("sink", "autograd"), MASKS, (False, True)):
        out.append(dict(fn="cross", pre_ln=pre_ln, biases=biases, grad_mode=gm, mask=mask, edge=edge))      # edge: qkv_bias and mem_dim != d
    for fn in ("attn", "mlp", "cross"):      # y has no consumer of its gradient
        out.append(dict(fn=fn, pre_ln=True, conv1d=False, biases=True, grad_mode="sink", mask="none", edge=False, cut=True))
    for second in (False, True):             # attention then MLP on one residual stream; second: another consumer of the attention output
        for gm in ("sink", "autograd"):
            out.append(dict(fn="pair", pre_ln=True, conv1d=False, biases=True, grad_mode=gm, mask="none", second=second, d=64, hidden=128))
    return out


def cell_id(c):
    return "-".join(f"{k}={v}" for k, v in c.items())


CELLS = _cells()
DROPOUT_CELLS = [dict(fn=fn, pre_ln=True, conv1d=False, biases=True, grad_mode="sink", mask="none", edge=False, dropout=True)
                 for fn in ("attn", "mlp", "cross")]


def cell_args(c):
    """name -> fp32 tensor (or None) of every tensor argument of the cell, in a fixed order; each from a seed of its own"""
    d, hid = c.get("d", D), c.get("hidden", HIDDEN)
    R = NSEQ * L
    b = c["biases"]
    A = {"x": _t(0, R, d)}
    # weights of standard deviation fan_in ** -0.5: every projection keeps its output near unit variance at either width (d = 16 or 64),
    # so the softmax is not saturated and the column sums behind the bias gradients are as well conditioned as a model's are
    lin = lambda seed, n_out, n_in, conv1d: _t(seed, *((n_in, n_out) if conv1d else (n_out, n_in)), scale=n_in ** -0.5)      # noqa: E731
    conv1d = c.get("conv1d", False)
    if c["fn"] in ("attn", "pair"):
        A.update(ln_w=_t(1, d, scale=0.2, shift=1.0), ln_b=_t(2, d, scale=0.2) if b else None, w_qkv=lin(3, 3 * d, d, conv1d),
                 b_qkv=_t(4, 3 * d, scale=0.2) if b else None, w_proj=lin(5, d, d, conv1d), b_proj=_t(6, d, scale=0.2) if b else None)
    if c["fn"] in ("mlp", "pair"):
        A.update(ln2_w=_t(11, d, scale=0.2, shift=1.0), ln2_b=_t(12, d, scale=0.2) if b else None, w1=lin(13, hid, d, conv1d),
                 b1=_t(14, hid, scale=0.2) if b else None, w2=lin(15, d, hid, conv1d), b2=_t(16, d, scale=0.2) if b else None)
    if c["fn"] == "cross":
        dm = MEM if c["edge"] else d
        qb = b and c["edge"]
        A.update(mem=_t(20, R, dm), nq_w=_t(21, d, scale=0.2, shift=1.0), nq_b=_t(22, d, scale=0.2) if b else None,
                 nkv_w=_t(23, dm, scale=0.2, shift=1.0), nkv_b=_t(24, dm, scale=0.2) if b else None, w_q=lin(25, d, d, False),
                 w_k=lin(26, d, dm, False), w_v=lin(27, d, dm, False), w_proj=lin(28, d, d, False), b_proj=_t(29, d, scale=0.2) if b else None,
                 b_q=_t(30, d, scale=0.2) if qb else None, b_k=_t(31, d, scale=0.2) if qb else None, b_v=_t(32, d, scale=0.2) if qb else None)
    kind = c.get("mask", "none")
    if kind in ("table", "bias_grad", "bias_nograd"):
        A["mask_t"] = _mask_tensor(kind)
    A["dy"] = _t(40, R, d)          # the weights of the scalar the cell differentiates
    A["xw"] = _t(41, R, d)          # ... and of a second path from x (so that x always has a gradient of its own)
    return A


NO_GRAD = ("dy", "xw")


def _wants_grad(c, name):
    if name in NO_GRAD:
        return False
    if name == "mask_t":
        return c["mask"] == "bias_grad"
    return True


# --------------------------------------------------------------------------- the float64 statement
def _ln(x, w, b, on):
    if not on:
        return x
    return torch.nn.functional.layer_norm(x, x.shape[-1:], w, b, EPS)


def _lin(x, W, b, conv1d):
    y = x @ (W if conv1d else W.t())
    return y if b is None else y + b


def _core(q, k, v, add, d):
    hd = d // H
    heads = lambda t: t.reshape(NSEQ, L, H, hd).permute(0, 2, 1, 3)      # noqa: E731
    s = heads(q) @ heads(k).transpose(-1, -2) * hd ** -0.5 + add
    p = torch.softmax(s, -1)
    return (p @ heads(v)).permute(0, 2, 1, 3).reshape(NSEQ * L, d), p


def _ref_attn(c, A, x):
    d = x.shape[1]
    qkv = _lin(_ln(x, A["ln_w"], A["ln_b"], c["pre_ln"]), A["w_qkv"], A["b_qkv"], c["conv1d"])
    o, p = _core(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], _additive(c["mask"], A.get("mask_t")), d)
    y = _lin(o, A["w_proj"], A["b_proj"], c["conv1d"])
    return (x + y if c["pre_ln"] else y), p


def _ref_mlp(c, A, x):
    h = torch.nn.functional.gelu(_lin(_ln(x, A["ln2_w"], A["ln2_b"], c["pre_ln"]), A["w1"], A["b1"], c["conv1d"]))
    y = _lin(h, A["w2"], A["b2"], c["conv1d"])
    return x + y if c["pre_ln"] else y


def _ref_cross(c, A, x):
    d = x.shape[1]
    xq, mkv = _ln(x, A["nq_w"], A["nq_b"], c["pre_ln"]), _ln(A["mem"], A["nkv_w"], A["nkv_b"], c["pre_ln"])
    q, k, v = _lin(xq, A["w_q"], A["b_q"], False), _lin(mkv, A["w_k"], A["b_k"], False), _lin(mkv, A["w_v"], A["b_v"], False)
    o, _ = _core(q, k, v, _additive(c["mask"], A.get("mask_t")), d)
    y = _lin(o, A["w_proj"], A["b_proj"], False)
    return x + y if c["pre_ln"] else y


class _Cut(torch.autograd.Function):
    """identity whose backward returns no gradient: what stands behind it sees a y nobody differentiates"""

    @staticmethod
    def forward(ctx, y):
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        return None


def _scalar(c, A, y, y_mid=None):
    """the scalar a cell differentiates, written once for both sides"""
    if c.get("cut"):
        y = _Cut.apply(y) if y.dtype != torch.float64 else y.detach()
    s = (y * A["dy"].to(y)).sum() + (A["x"] * A["xw"].to(y)).sum()
    if c.get("second"):
        s = s + (y_mid * y_mid).sum()
    return s


_REF = {}


def reference(c):
    """float64 outputs and gradients of the cell, computed once and shared (the dropout flag does not enter: those cells have no float64 side)"""
    key = cell_id({k: v for k, v in c.items() if k != "grad_mode"})
    if key not in _REF:
        A = {k: (None if v is None else v.double().requires_grad_(_wants_grad(c, k))) for k, v in cell_args(c).items()}
        res = {}
        x = A["x"]
        if c["fn"] == "attn":
            y, res["out:probs"] = _ref_attn(c, A, x)
            mid = None
        elif c["fn"] == "mlp":
            y, mid = _ref_mlp(c, A, x), None
        elif c["fn"] == "cross":
            y, mid = _ref_cross(c, A, x), None
        else:
            mid, res["out:probs"] = _ref_attn(c, A, x)
            y = _ref_mlp(c, A, mid)
        res["out:y"] = y
        _scalar(c, A, y, mid).backward()
        for k, v in A.items():
            if v is not None and _wants_grad(c, k):
                res["grad:" + k] = v.grad if v.grad is not None else torch.zeros_like(v)
        _REF[key] = {k: v.detach() for k, v in res.items()}
    return _REF[key]


# --------------------------------------------------------------------------- the Functions
def _mask_arg(c, A):
    kind = c.get("mask", "none")
    if kind == "blockcausal":
        return ("blockcausal", 2)
    if kind == "table":
        return ("table", A["mask_t"])
    if kind in ("bias_grad", "bias_nograd"):
        return ("bias", A["mask_t"])
    return kind


def run_cell(c, device, after_backward=None):
    """the cell through the Functions' apply at the current precision; returns name -> fp32 cpu tensor (outputs and every gradient)"""
    from afft_amd import functional as F_, runtime as rt
    from afft_amd.dropout import DropCfg
    rt.set_grad_mode(c["grad_mode"])
    try:
        rt.SINK.begin_step()
        F_._forget_output()
        A = {k: (None if v is None else v.to(device).requires_grad_(_wants_grad(c, k))) for k, v in cell_args(c).items()}
        drop = DropCfg(p_out=DROP_P, k_out=DROP_KEY) if c.get("dropout") else None
        mask = _mask_arg(c, A)
        x = A["x"]
        res = {}
        mid = None
        if c["fn"] in ("attn", "pair"):
            y, res["out:probs"] = F_.AttnSublayer.apply(x, A["ln_w"], A["ln_b"], A["w_qkv"], A["b_qkv"], A["w_proj"], A["b_proj"], L, H, mask,
                                                        EPS, c["conv1d"], c["pre_ln"], None, drop, None, 0, F_.mask_bias(mask))
        if c["fn"] == "pair":
            mid = y
        if c["fn"] in ("mlp", "pair"):
            y = F_.MLPSublayer.apply(x if mid is None else mid, A["ln2_w"], A["ln2_b"], A["w1"], A["b1"], A["w2"], A["b2"], EPS, "erf",
                                     c["conv1d"], c["pre_ln"], drop)
        if c["fn"] == "cross":
            y = F_.CrossAttnSublayer.apply(x, A["mem"], A["nq_w"], A["nq_b"], A["nkv_w"], A["nkv_b"], A["w_q"], A["w_k"], A["w_v"], A["w_proj"],
                                           A["b_proj"], L, H, mask, EPS, c["pre_ln"], None, drop, A["b_q"], A["b_k"], A["b_v"], F_.mask_bias(mask))
        res["out:y"] = y
        _scalar(c, A, y, mid).backward()
        if after_backward is not None:
            after_backward(F_)
        for k, v in A.items():
            if v is not None and _wants_grad(c, k):
                res["grad:" + k] = v.grad if v.grad is not None else torch.zeros_like(v)
        return {k: v.detach().float().cpu() for k, v in res.items()}
    finally:
        rt.set_grad_mode("sink")


def check(got, ref, tol, gtol, what):
    assert set(got) == set(ref), (what, sorted(set(got) ^ set(ref)))
    for k in sorted(got):
        assert got[k].shape == ref[k].shape, (what, k)
        # the key bias shifts every score of a row alike, so its gradient is zero in exact arithmetic (softmax): what comes back is
        # rounding, measured on the scale of the query bias's gradient beside it
        scale = ref["grad:b_q"].float() if k == "grad:b_k" else ref[k].float()
        e = rel_l2(got[k] - ref[k].float() + scale, scale)
        print(f"{what} {k} {e:.3e}")
        assert e < (tol if k.startswith("out:") else gtol), (what, k, e)


def _nothing_outlives(F_):
    assert F_._TS.shadow is None and F_._TS.pending_ready == []


# --------------------------------------------------------------------------- CPU
def _bias_fwd(q, k, v, nseq, L_, H_, hd, scale, bias, out, probs, drop_p=0.0, drop_key=0):
    """afft_attention_fwd_bias on the double: the table restatement takes anything that broadcasts to (nseq, H, L, L)"""
    return cpu_ops.attention_fwd_table(q, k, v, nseq, L_, H_, hd, scale, bias.reshape((1,) * (4 - bias.dim()) + tuple(bias.shape)), out, probs)


@torch.no_grad()
def _bias_bwd(dout, v, probs, nseq, L_, H_, hd, dbias, drop_p=0.0, drop_key=0):
    """afft_attention_bias_bwd on the double: dS = P (dP - sum_j P dP), summed over the dimensions the bias broadcasts"""
    assert drop_p == 0.0
    vh, doh = (cpu_ops._heads(t, nseq, L_, H_, hd) for t in (v, dout))
    dp = doh @ vh.transpose(-1, -2)
    ds = probs * (dp - (dp * probs).sum(-1, keepdim=True))
    return dbias.copy_(ds.sum_to_size((1,) * (4 - dbias.dim()) + tuple(dbias.shape)).reshape(dbias.shape))


@pytest.fixture
def cpu_double(monkeypatch):
    import afft_amd
    from afft_amd import ops
    afft_amd.set_precision("fp32")
    try:
        with cpu_ops.installed():
            monkeypatch.setattr(ops, "attention_fwd_bias", _bias_fwd)
            monkeypatch.setattr(ops, "attention_bias_bwd", _bias_bwd)
            yield
            monkeypatch.undo()
    finally:
        afft_amd.set_precision("bf16")


@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_cpu_cell_matches_float64(cell, cpu_double):
    got = run_cell(cell, torch.device("cpu"), after_backward=_nothing_outlives if cell.get("cut") else None)
    check(got, reference(cell), CPU_TOL, CPU_TOL, cell_id(cell))


@pytest.mark.parametrize("second", [False, True])
def test_cpu_pair_handover_is_accepted_or_turned_down(second, cpu_double, monkeypatch):
    """bf16 on the double, where the hand-over is live: attention then MLP on one residual stream accepts it (the attention output bias
    gets its gradient from the hand-over, once); a second consumer of the attention output turns it down.  Either way the gradients are
    those of the run with the hand-over switched off, inside the 2e-2 of test_host_logic_cpu.py::test_gradient_handover_accepted_and_off_agree."""
    import afft_amd
    from afft_amd import functional as F_, runtime as rt
    afft_amd.set_precision("bf16")
    cell = next(c for c in CELLS if c["fn"] == "pair" and c["second"] == second and c["grad_mode"] == "sink")
    accepted = []
    inner = F_._accept_bias
    monkeypatch.setattr(F_, "_accept_bias", lambda sh: (accepted.append(sh.bias.shape), inner(sh))[1])
    res = {}
    try:
        for on in (True, False):
            rt.set_handover(on)
            res[on] = run_cell(cell, torch.device("cpu"), after_backward=_nothing_outlives)
            if on:
                assert len(accepted) == (0 if second else 1)
    finally:
        rt.set_handover(True)
    assert len(accepted) == (0 if second else 1)
    check(res[True], res[False], 2e-2, 2e-2, cell_id(cell))


def test_argument_counts_are_those_of_the_forward_signatures():
    from afft_amd import functional as F_
    for fn, n, at in ((F_.AttnSublayer, F_._ATTN_NARGS, F_._ATTN_BIAS_AT), (F_.MLPSublayer, F_._MLP_NARGS, None),
                      (F_.CrossAttnSublayer, F_._CROSS_NARGS, F_._CROSS_BIAS_AT)):
        names = list(inspect.signature(fn.forward).parameters)[1:]
        assert len(names) == n
        assert at is None or names[at] == "bias"
    assert list(inspect.signature(F_.CrossAttnSublayer.forward).parameters)[1:][F_._CROSS_BIAS_AT - 3:F_._CROSS_BIAS_AT] == ["b_q", "b_k", "b_v"]


# --------------------------------------------------------------------------- GPU
@pytest.fixture
def call_by_call():
    import afft_amd
    from afft_amd import runtime as rt
    was = rt.composite()
    rt.set_composite(False)
    try:
        yield
    finally:
        rt.set_composite(was)
        afft_amd.set_precision("bf16")


def _gpu_bounds(precision):
    from test_model_gpu import GTOL_BF16, TOL
    return TOL[precision], (GTOL_BF16 if precision == "bf16" else TOL[precision])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_gpu_cell_matches_float64(cell, precision, call_by_call):
    import afft_amd
    afft_amd.set_precision(precision)
    got = run_cell(cell, torch.device("cuda:0"), after_backward=_nothing_outlives if cell.get("cut") or cell["fn"] == "pair" else None)
    tol, gtol = _gpu_bounds(precision)
    check(got, reference(cell), tol, gtol, cell_id(cell) + "/" + precision)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", DROPOUT_CELLS, ids=cell_id)
def test_gpu_output_dropout_cell_equals_the_recorded_call_by_call_result(cell, call_by_call):
    """bf16, output dropout p = 0.3 with a fixed key: against the arrays tests/golden/make_golden_cbc_dropout.py recorded from the build
    before the shared driver.  Every recorded entry reproduced bit for bit over two runs of that build, so equality is asked."""
    import afft_amd
    afft_amd.set_precision("bf16")
    z = np.load(os.path.join(GOLDEN, "cbc_dropout.npz"))
    got = run_cell(cell, torch.device("cuda:0"))
    names = [k for k in z.files if k.startswith(cell["fn"] + ".")]
    assert sorted(names) == sorted(cell["fn"] + "." + k for k in got)
    for k in names:
        assert torch.equal(got[k.split(".", 1)[1]], torch.from_numpy(z[k])), k
