"""Additive attention bias that broadcasts over batch and heads (afft_attention_fwd_bias, afft_attention_long_fwd_bias) and its gradient
(afft_attention_bias_bwd) against float64 math, with the bars of the table cases of test_attention_long_gpu.py: relative L2, f32 2e-5
(out, probs) / 3e-5 (gradients), bf16 1e-2 (out) / 2e-3 (probs) / 2e-2 (gradients); dbias takes the gradients' bar.  Then: bias == table
bitwise, dbias bit-stable, the mirrored Block / DecoderBlock against the reference's own numbers (tests/golden/b0_attn_bias.npz), and the
argument errors."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from helpers import GOLDEN, edge_error, rel_l2  # noqa: E402
from kernel_doubles import mix32  # noqa: E402

pytestmark = pytest.mark.gpu

NSEQ, H, SENTINEL = 3, 2, 512.0
NEG = float("-inf")
BIAS_SHAPES = {"table": lambda L: (L, L), "pad": lambda L: (NSEQ, 1, 1, L), "head": lambda L: (1, H, L, L),
               "sample": lambda L: (NSEQ, 1, L, L), "full": lambda L: (NSEQ, H, L, L)}


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def bfr(t):
    return t.to(torch.bfloat16).float()


def make_bias(shape, seed):
    """random additive bias with ~20 % -inf, never a whole row: key 0 stays finite"""
    t = 0.5 * rnd(*shape, seed=seed)
    hide = torch.rand(*shape, generator=torch.Generator().manual_seed(seed + 1)) < 0.2
    hide[..., 0] = False
    return t.masked_fill(hide, NEG)


def keep_mask(key, p, nseq, L):
    """the kernels' dropout mask (csrc/common.h: drop_keep): keep(idx) = mix32(mix32(idx) ^ key) >= p * 2^32, idx the flat index into
    [nseq, H, L, L]; the device salt, if an earlier test has left it on, is part of the key"""
    from afft_amd import dropout as D_
    if D_._salt is not None:
        key ^= int(D_._salt.item()) & 0xFFFFFFFF
    idx = np.arange(nseq * H * L * L, dtype=np.uint64)
    keep = mix32(mix32(idx) ^ np.uint64(key)) >= np.uint64(int(p * 4294967296.0))
    return torch.from_numpy(keep.reshape(nseq, H, L, L))


def run_hip(tdt, qkv, dout, bias, L, hd, p, key, dbias_runs=1):
    """forward with the bias, dq / dk / dv from the existing backward entry points, dbias -> CPU tensors"""
    from afft_amd import ops
    d, R, long_ = H * hd, NSEQ * L, L > 128
    g = qkv.to(tdt).to(dev())
    q, k, v = g[:, :d], g[:, d:2 * d], g[:, 2 * d:]
    out = torch.full((R, d), SENTINEL, dtype=tdt, device=dev())
    probs = torch.full((NSEQ, H, L, L), SENTINEL, device=dev())
    b = bias.to(dev())
    (ops.attention_long_fwd_bias if long_ else ops.attention_fwd_bias)(q, k, v, NSEQ, L, H, hd, hd ** -0.5, b, out, probs, drop_p=p, drop_key=key)
    do = dout.to(tdt).to(dev())
    dg = torch.full((R, 3 * d), SENTINEL, dtype=tdt, device=dev())
    (ops.attention_long_bwd if long_ else ops.attention_bwd)(do, q, k, v, probs, NSEQ, L, H, hd, hd ** -0.5, dg[:, :d], dg[:, d:2 * d],
                                                             dg[:, 2 * d:], drop_p=p, drop_key=key)
    dbs = []
    for _ in range(dbias_runs):
        db = torch.full(tuple(bias.shape), SENTINEL, device=dev())
        ops.attention_bias_bwd(do, v, probs, NSEQ, L, H, hd, db, drop_p=p, drop_key=key)
        dbs.append(db)
    torch.cuda.synchronize()
    return out.float().cpu(), probs.cpu(), dg.float().cpu(), [t.cpu() for t in dbs]


_INPUTS = {}


def inputs(L, hd, dt):
    """q | k | v and dout of a (L, hd, storage) cell, made once and left unchanged"""
    if (L, hd, dt) not in _INPUTS:
        qkv, dout = rnd(NSEQ * L, 3 * H * hd, seed=1), rnd(NSEQ * L, H * hd, seed=2)
        _INPUTS[(L, hd, dt)] = (bfr(qkv), bfr(dout)) if dt == "bf16" else (qkv, dout)
    return _INPUTS[(L, hd, dt)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind", list(BIAS_SHAPES))
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("hd", [24, 64])
@pytest.mark.parametrize("L", [5, 40, 128, 129, 160])
def test_attention_bias_fwd_bwd(L, hd, dt, kind, p):
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    d, R, scale, key = H * hd, NSEQ * L, hd ** -0.5, 4321
    qkv, dout = inputs(L, hd, dt)
    bias = make_bias(BIAS_SHAPES[kind](L), seed=5)
    out, probs, dg, (dbias,) = run_hip(tdt, qkv, dout, bias, L, hd, p, key)
    # float64: softmax(q k^T scale + bias), dropout with the kernels' mask, times v
    qr = qkv.double().requires_grad_(True)
    br = bias.double().requires_grad_(True)
    t = qr.view(NSEQ, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    p_ref = ((t[0] @ t[1].transpose(-2, -1)) * scale + br).softmax(dim=-1)
    pd = p_ref
    if p > 0:
        pd = p_ref * keep_mask(key, p, NSEQ, L).double() * float(np.float32(1) / (np.float32(1) - np.float32(p)))
    o_ref = (pd @ t[2]).transpose(1, 2).reshape(R, d)
    o_ref.backward(dout.double())
    e_out, e_p = rel_l2(out, o_ref), rel_l2(probs, p_ref)
    e_g, e_b = rel_l2(dg, qr.grad), rel_l2(dbias, br.grad)
    print(f"attention_bias {dt} L={L} hd={hd} {kind} p={p}: out {e_out:.3e} probs {e_p:.3e} grads {e_g:.3e} dbias {e_b:.3e}")
    assert e_out < (2e-5 if dt == "f32" else 1e-2)
    assert e_p < (2e-5 if dt == "f32" else 2e-3)
    assert e_g < (3e-5 if dt == "f32" else 2e-2)
    assert e_b < (3e-5 if dt == "f32" else 2e-2)
    # hidden entries: probability and bias gradient exactly zero; every element of every result was written
    hidden = torch.isinf(bias).expand(NSEQ, H, L, L)
    assert float(probs[hidden].abs().max()) == 0.0
    assert float(dbias[torch.isinf(bias)].abs().max()) == 0.0
    assert all(bool(torch.isfinite(x).all()) and not bool((x == SENTINEL).any()) for x in (out, probs, dg, dbias))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("L,hd", [(5, 64), (40, 24), (128, 64), (129, 64), (160, 24), (160, 64)])
def test_attention_bias_equals_table_bitwise(L, hd, dt, p):
    """sb = sh = 0, si = L: the results of afft_attention_fwd_table / afft_attention_long_fwd on the same table, bit for bit"""
    from afft_amd import ops
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    d, R = H * hd, NSEQ * L
    qkv, _ = inputs(L, hd, dt)
    g = qkv.to(tdt).to(dev())
    q, k, v = g[:, :d], g[:, d:2 * d], g[:, 2 * d:]
    table = make_bias((L, L), seed=9).to(dev())
    assert ops.bias_strides(table, NSEQ, L, H) == (0, 0, L)
    res = []
    for use_bias in (False, True):
        out = torch.full((R, d), SENTINEL, dtype=tdt, device=dev())
        probs = torch.full((NSEQ, H, L, L), SENTINEL, device=dev())
        if use_bias:
            (ops.attention_long_fwd_bias if L > 128 else ops.attention_fwd_bias)(q, k, v, NSEQ, L, H, hd, hd ** -0.5, table, out, probs, drop_p=p, drop_key=99)
        elif L > 128:
            ops.attention_long_fwd(q, k, v, NSEQ, L, H, hd, hd ** -0.5, 0, out, probs, drop_p=p, drop_key=99, table=table)
        else:
            ops.attention_fwd_table(q, k, v, NSEQ, L, H, hd, hd ** -0.5, table, out, probs, drop_p=p, drop_key=99)
        torch.cuda.synchronize()
        res.append((out.cpu(), probs.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not bool((res[1][1] == SENTINEL).any())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("L", [40, 160])
def test_attention_dbias_bit_stable(L, dt):
    """the fully broadcast (L, L) bias: every element of dbias is a sum over nseq * H terms, in a fixed order -- two runs, the same bits"""
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    qkv, dout = inputs(L, 64, dt)
    _, _, _, (a, b) = run_hip(tdt, qkv, dout, make_bias((L, L), seed=7), L, 64, 0.1, 777, dbias_runs=2)
    assert torch.equal(a, b) and float(a.abs().max()) > 0


# ----------------------------------------------------------------------------- the mirrored modules against the reference's numbers
def _fixture():
    from bias_cases import B, D, N
    import closed_form as cf
    z = np.load(os.path.join(GOLDEN, "b0_attn_bias.npz"), allow_pickle=False)
    shapes = json.loads(str(z["shapes"]))
    states = {tag: {k: cf.tensor_for(f"b0.{tag}.{k}", tuple(s)) for k, s in shapes[tag].items()} for tag in ("block", "dec")}
    x = {tag: cf.tensor_for(f"b0.{tag}.x", (B, N, D), "input") for tag in ("block", "dec")}
    return z, states, x, cf.tensor_for("b0.dec.mem", (B, N, D), "input")


def _run_module(case, z, states, x, mem, leaf=True):
    """-> {fixture key: tensor}; leaf: the mask itself requires grad (gradient sink), else a computed copy of it (autograd)"""
    from afft_amd import runtime as rt
    from afft_amd.models.transformerblock import Block, DecoderBlock
    from bias_cases import D, GRAD_KEYS, H as HEADS
    tag = "dec" if case == "dec" else "block"
    needs = f"{case}.dmask" in z.files
    m = torch.from_numpy(z[f"{case}.mask"]).to(dev()).requires_grad_(needs)
    mod = (DecoderBlock(D, num_heads=HEADS) if tag == "dec" else Block(D, HEADS)).eval()
    mod.load_state_dict(states[tag])
    mod = mod.to(dev())
    rt.SINK.begin_step()
    xin = x[tag].to(dev()).requires_grad_(True)
    mask = m if leaf else m * 1.0
    got = {}
    if tag == "dec":
        mm = mem.to(dev()).requires_grad_(True)
        y = mod(xin, mm, mask)
        y.pow(2).mean().backward()
        got["dec.dmem"] = mm.grad
    else:
        y, attn = mod(xin, mask)
        y.pow(2).mean().backward()
        got[f"{case}.attn"] = attn
    rt.SINK.finish_step(list(mod.parameters()))
    got.update({f"{case}.y": y, f"{case}.dx": xin.grad})
    params = dict(mod.named_parameters())
    got.update({f"{case}.grad.{k}": params[k].grad for k in GRAD_KEYS})
    if needs:
        got[f"{case}.dmask"] = m.grad
    return got


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 3e-2)])
@pytest.mark.parametrize("case", ["pad", "head", "sample", "full", "grad2d", "dec"])
def test_modules_with_broadcast_masks_match_reference_golden(case, precision, tol):
    """Block / DecoderBlock with masks that broadcast over batch and heads, and masks that require grad, through the C-ABI against the
    reference's own outputs, attention maps and gradients (the mask's included); bars of
    test_model_gpu.py::test_interface_edges_arbitrary_mask_mem_dim_qkv_bias_on_the_hip_path's fixture: 1e-3 in the fp32 mode, 3e-2 in bf16"""
    import afft_amd
    from afft_amd import runtime as rt
    z, states, x, mem = _fixture()
    afft_amd.set_precision(precision)
    rt.set_grad_mode("sink")
    try:
        got = _run_module(case, z, states, x, mem)
        torch.cuda.synchronize()
    finally:
        afft_amd.set_precision("bf16")
    want = {k for k in z.files if k.startswith(case + ".") and not k.endswith(".mask")}
    assert want == set(got)
    worst = {}
    for k in sorted(want):
        assert got[k] is not None, k
        worst[k] = edge_error(got[k], torch.from_numpy(z[k]))
    print(f"modules {case} {precision}:", {k: f"{e:.2e}" for k, e in worst.items()})
    bad = {k: v for k, v in worst.items() if not v < tol}
    assert not bad, bad


@pytest.mark.parametrize("case", ["grad2d", "dec"])
def test_mask_gradient_through_autograd_equals_the_sink(case):
    """a computed (non-leaf) mask hands its gradient back to autograd; a leaf gets it through the gradient sink: the same kernel, the same bits"""
    import afft_amd
    from afft_amd import runtime as rt
    z, states, x, mem = _fixture()
    afft_amd.set_precision("fp32")
    rt.set_grad_mode("sink")
    try:
        a = _run_module(case, z, states, x, mem, leaf=True)[f"{case}.dmask"]
        b = _run_module(case, z, states, x, mem, leaf=False)[f"{case}.dmask"]
        torch.cuda.synchronize()
    finally:
        afft_amd.set_precision("bf16")
    assert a is not None and b is not None and torch.equal(a, b)


def test_a_mask_without_grad_takes_no_bias_gradient_launch(monkeypatch):
    from afft_amd import ops
    import afft_amd
    z, states, x, mem = _fixture()

    def never(*a, **k):
        raise AssertionError("attention_bias_bwd ran for a mask that takes no gradient")

    monkeypatch.setattr(ops, "attention_bias_bwd", never)
    afft_amd.set_precision("fp32")
    try:
        got = _run_module("sample", z, states, x, mem)
    finally:
        afft_amd.set_precision("bf16")
    assert got["sample.dx"] is not None


# ----------------------------------------------------------------------------- errors
def test_attention_bias_errors_are_returned_not_launched():
    from afft_amd import _lib, ops
    lib = _lib.lib()
    for L, fwd, cfwd in ((40, ops.attention_fwd_bias, lib.afft_attention_fwd_bias), (160, ops.attention_long_fwd_bias, lib.afft_attention_long_fwd_bias)):
        hd, d, R = 64, H * 64, NSEQ * L
        g = torch.zeros(R, 3 * d, device=dev())
        q, k, v = g[:, :d], g[:, d:2 * d], g[:, 2 * d:]
        out = torch.full((R, d), SENTINEL, device=dev())
        probs = torch.full((NSEQ, H, L, L), SENTINEL, device=dev())
        dbias = torch.full((NSEQ, 1, L, L), SENTINEL, device=dev())
        with pytest.raises(ValueError, match=r"got \(4, 1, %d, %d\)" % (L, L)):      # a wrong batch size
            fwd(q, k, v, NSEQ, L, H, hd, 0.125, torch.zeros(NSEQ + 1, 1, L, L, device=dev()), out, probs)
        with pytest.raises(ValueError, match=r"got \(4, 1, %d, %d\)" % (L, L)):
            ops.attention_bias_bwd(out, v, probs, NSEQ, L, H, hd, torch.zeros(NSEQ + 1, 1, L, L, device=dev()))
        bias = torch.zeros(NSEQ, 1, L, L, device=dev())
        args = (q.data_ptr(), 3 * d, k.data_ptr(), 3 * d, v.data_ptr(), 3 * d, _lib.F32, NSEQ, L, H, hd, 0.125)
        rc = cfwd(*args, bias.data_ptr(), -L * L, 0, L, 0.0, 0, out.data_ptr(), d, probs.data_ptr(), None)       # a negative stride
        assert rc != 0 and "negative bias stride (sb=-%d" % (L * L) in lib.afft_last_error().decode()
        rc = lib.afft_attention_bias_bwd(out.data_ptr(), d, v.data_ptr(), 3 * d, _lib.F32, probs.data_ptr(), NSEQ, L, H, hd, 0.0, 0,
                                         dbias.data_ptr(), L * L, 0, -L, None, None)
        assert rc != 0 and "si=-%d" % L in lib.afft_last_error().decode()
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (out, probs, dbias))
