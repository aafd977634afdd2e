"""Build-container test of the HOST logic of the cached roll-out in the 'fp16x2' precision (runtime.kv_cache_fp16x2, BaseFuturePredictor.forward,
GPT2Block.forward_step, functional.attn_step / mlp_step) on CPU tensors.  The two composite calls of that step
(ops.attn_step_sublayer_f16x2, ops.mlp_step_sublayer_f16x2) are replaced by the plain-torch doubles of tests/cpu_ops_step_f16x2.py --
restatements of the contracts in include/afft_hip.h -- which record what they were handed: when the path
engages, with which rows and lengths, which one-pass flags, and how much plane scratch.  What the kernels compute is tested on the GPU."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch

import cpu_ops_step_f16x2
from cpu_ops_step_f16x2 import ONE1, ONE2, ONE_ATTN      # AFFT_F16X2_ONE_PASS_1 / _2 / _ATTN

B, T, D, H, LAYERS = 2, 4, 64, 2, 2


@contextlib.contextmanager
def _installed():
    """cpu_ops_step's doubles, the two composite ones of cpu_ops_step_f16x2, and counters on the QKV GEMMs and the call-by-call step"""
    from afft_amd import ops
    with cpu_ops_step_f16x2.installed() as dbl:
        saved = ops.gemm, ops.attention_step
        dbl.qkv_rows, dbl.steps = [], 0

        def gemm(a, b, out, **kw):
            if out.shape[1] == 3 * D:
                dbl.qkv_rows.append(out.shape[0])
            return saved[0](a, b, out, **kw)

        def step(*a, **k):
            dbl.steps += 1
            return saved[1](*a, **k)
        ops.gemm, ops.attention_step = gemm, step
        try:
            yield dbl
        finally:
            ops.gemm, ops.attention_step = saved


@pytest.fixture()
def rt_state():
    """the switches this file turns, put back afterwards"""
    import afft_amd
    from afft_amd import runtime as rt
    saved = rt.kv_cache(), rt.kv_cache_fp16x2(), rt.kv_cache_train(), rt.one_pass_sites()
    min_dim = rt.set_one_pass_min_dim(0)
    rt.set_one_pass_min_dim(min_dim)
    afft_amd.set_precision("fp16x2")
    yield rt
    afft_amd.set_precision("bf16")
    rt.set_kv_cache(saved[0])
    rt.set_kv_cache_fp16x2(saved[1])
    rt.set_kv_cache_train(saved[2])
    rt.set_one_pass_sites(saved[3])
    rt.set_one_pass_min_dim(min_dim)


@pytest.fixture()
def predictor(rt_state):
    from afft_amd.models.future_prediction import BaseFuturePredictor
    torch.manual_seed(0)
    return BaseFuturePredictor(D, inter_dim=D, n_layer=LAYERS, n_head=H, embd_pdrop=0.0, resid_pdrop=0.0, attn_pdrop=0.0,
                               output_attentions=True).eval()


def _run(predictor, feats, output_len, grad=False):
    with _installed() as dbl, torch.set_grad_enabled(grad):
        out, att = predictor(feats, output_len)
    return out, att, dbl


RECOMPUTE_ROWS = [B * T] * LAYERS + [B * (T + 1)] * LAYERS + [B * (T + 2)] * LAYERS


def test_switch_is_off_by_default_and_fp16x2_then_recomputes(predictor, rt_state):
    assert rt_state.kv_cache() and not rt_state.kv_cache_fp16x2()
    out, att, dbl = _run(predictor, torch.randn(B, T, D), 3)
    assert dbl.attn == [] and dbl.mlp == [] and dbl.steps == 0
    assert dbl.qkv_rows == RECOMPUTE_ROWS


def test_switch_on_rolls_out_through_the_composite_step(predictor, rt_state):
    feats = torch.randn(B, T, D)
    out0, att0, _ = _run(predictor, feats, 3)
    rt_state.set_kv_cache_fp16x2(True)
    out, att, dbl = _run(predictor, feats, 3)
    assert dbl.steps == 0 and dbl.qkv_rows == []                                  # no call-by-call step, no QKV GEMM outside the composite
    assert len(dbl.attn) == len(dbl.mlp) == LAYERS * 3
    assert [(c["Lq"], c["Lk"]) for c in dbl.attn] == [(T, T)] * LAYERS + [(1, T + 1)] * LAYERS + [(1, T + 2)] * LAYERS
    assert [c["rows"] for c in dbl.attn] == [B * T] * LAYERS + [B] * LAYERS * 2 == [c["rows"] for c in dbl.mlp]
    assert all(c["probs"] for c in dbl.attn)
    assert out.shape == (B, T + 2, D)
    assert att["gpt2_att_0"].shape == (B, LAYERS, H, T, T)
    assert att["gpt2_att_1"].shape == (B, LAYERS, H, 1, T + 1) and att["gpt2_att_2"].shape == (B, LAYERS, H, 1, T + 2)
    upper = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    assert float(att["gpt2_att_0"][..., upper].abs().max()) == 0.0
    # the same model by the recompute: the doubles round where the kernels do, the results agree to that rounding
    assert torch.allclose(out, out0, rtol=2e-3, atol=2e-3)
    for k in att0:
        assert torch.allclose(att[k], att0[k], rtol=2e-3, atol=2e-3), k


def test_training_grad_and_the_main_switch_keep_the_recompute(predictor, rt_state):
    feats = torch.randn(B, T, D)
    rt_state.set_kv_cache_fp16x2(True)
    assert len(_run(predictor, feats, 1)[2].attn) == 0                            # output_len == 1: nothing to roll out
    assert len(_run(predictor, feats, 2)[2].attn) == LAYERS * 2
    dbl = _run(predictor, feats, 3, grad=True)[2]
    assert dbl.attn == [] and dbl.steps == 0 and dbl.qkv_rows == RECOMPUTE_ROWS   # grad enabled
    predictor.train()
    dbl = _run(predictor, feats, 3)[2]
    assert dbl.attn == [] and dbl.steps == 0 and dbl.qkv_rows == RECOMPUTE_ROWS   # training mode
    rt_state.set_kv_cache_train(True)                                             # training through the cache stays closed to fp16x2
    dbl = _run(predictor, feats, 3, grad=True)[2]
    assert dbl.attn == [] and dbl.steps == 0 and dbl.qkv_rows == RECOMPUTE_ROWS
    rt_state.set_kv_cache_train(False)
    predictor.eval()
    rt_state.set_kv_cache(False)                                                  # AFFT_KV_CACHE=0: it needs kv_cache() on as well
    dbl = _run(predictor, feats, 3)[2]
    assert dbl.attn == [] and dbl.steps == 0 and dbl.qkv_rows == RECOMPUTE_ROWS


@pytest.mark.parametrize("precision", ["bf16", "fp32", "bf16x3"])
def test_other_precisions_keep_their_call_by_call_step(predictor, rt_state, precision):
    import afft_amd
    afft_amd.set_precision(precision)
    feats = torch.randn(B, T, D)
    res = {}
    for on in (False, True):
        rt_state.set_kv_cache_fp16x2(on)
        out, att, dbl = _run(predictor, feats, 3)
        assert dbl.attn == [] and dbl.mlp == []
        assert dbl.steps == LAYERS * 3 and dbl.qkv_rows == [B * T] * LAYERS + [B] * LAYERS * 2
        res[on] = out
    assert torch.equal(res[True], res[False])


def test_env_switch():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("1", "True"), ("0", "False"), (None, "False")):
        env = {k: v for k, v in os.environ.items() if k != "AFFT_KV_CACHE_FP16X2"}
        if value is not None:
            env["AFFT_KV_CACHE_FP16X2"] = value
        r = subprocess.run([sys.executable, "-c", "from afft_amd import runtime as rt; print(rt.kv_cache_fp16x2())"], cwd=root, env=env,
                           capture_output=True, text=True)
        assert r.stdout.strip() == want, (value, r.stdout, r.stderr)


# ---------------------------------------------------------------- flag plumbing and plane scratch (functional.attn_step / mlp_step)
def _step_once(d, rows, Lq, heads=4):
    from afft_amd import functional as F_
    g = torch.Generator().manual_seed(d + rows)
    r = lambda *s: 0.02 * torch.randn(*s, generator=g)      # noqa: E731
    x = torch.randn(rows, d, generator=g)
    past = 2
    caches = torch.zeros(2, rows // Lq, past + Lq, d)
    with _installed() as dbl, torch.no_grad():
        y, probs = F_.attn_step(x, torch.ones(d), torch.zeros(d), r(d, 3 * d), r(3 * d), r(d, d), r(d), Lq, heads, 1e-5, True, caches[0],
                                caches[1], past, False)
        y = F_.mlp_step(y, torch.ones(d), torch.zeros(d), r(d, 4 * d), r(4 * d), r(4 * d, d), r(d), 1e-5, "tanh", True)
    assert probs is None and y.shape == (rows, d) and torch.isfinite(y).all()
    assert len(dbl.attn) == len(dbl.mlp) == 1 and dbl.steps == 0
    return dbl.attn[0], dbl.mlp[0]


def test_wide_model_gets_the_default_one_pass_sites_and_no_lo_planes(rt_state):
    d, rows = 2048, 3
    pr = 64
    a, m = _step_once(d, rows, 1)
    assert a["flags"] == 1 | ONE1 | ONE2 and m["flags"] == 1 | ONE1 | ONE2
    assert (a["xn"], a["ao"]) == (pr * d, pr * d)                      # hi planes alone
    assert a["qkv"] == 2 * pr * 3 * d                                  # the attention core keeps hi + lo by default
    assert (m["xn"], m["h"]) == (pr * d, pr * 4 * d)
    assert not a["probs"]
    rt_state.set_one_pass_sites("")                                    # every site two passes
    a, m = _step_once(d, rows, 1)
    assert a["flags"] == 1 and m["flags"] == 1
    assert (a["xn"], a["qkv"], a["ao"], m["xn"], m["h"]) == (2 * pr * d, 2 * pr * 3 * d, 2 * pr * d, 2 * pr * d, 2 * pr * 4 * d)


def test_narrow_model_keeps_every_lo_plane(rt_state):
    d, rows, Lq = 64, 70, 5
    pr = 128                                                           # pad64(70)
    a, m = _step_once(d, rows, Lq, heads=2)
    assert a["flags"] == 1 and m["flags"] == 1
    assert (a["xn"], a["qkv"], a["ao"]) == (2 * pr * d, 2 * pr * 3 * d, 2 * pr * d)      # lo planes at pad64(rows) * width
    assert (m["xn"], m["h"]) == (2 * pr * d, 2 * pr * 4 * d)
    assert (a["Lq"], a["Lk"]) == (Lq, 2 + Lq)


def test_all_sites_on_a_narrow_model(rt_state):
    rt_state.set_one_pass_sites("linear,conv1d")
    rt_state.set_one_pass_min_dim(0)
    d, rows = 64, 3
    pr = 64
    a, m = _step_once(d, rows, 1, heads=2)
    assert a["flags"] == 1 | ONE1 | ONE2 | ONE_ATTN and m["flags"] == 1 | ONE1 | ONE2
    assert (a["xn"], a["qkv"], a["ao"]) == (pr * d, pr * 3 * d, pr * d)                  # no lo plane anywhere: the step reads q, k, v with in_lo = 0
    assert (m["xn"], m["h"]) == (pr * d, pr * 4 * d)


def test_widths_off_the_64_grid_take_the_call_by_call_step(rt_state):
    """as the sub-layer Functions leave the composite path there (functional._composite_ok)"""
    from afft_amd import functional as F_
    d, rows = 48, 3
    g = torch.Generator().manual_seed(1)
    r = lambda *s: 0.02 * torch.randn(*s, generator=g)      # noqa: E731
    caches = torch.zeros(2, rows, 3, d)
    with _installed() as dbl, torch.no_grad():
        y, _ = F_.attn_step(torch.randn(rows, d, generator=g), torch.ones(d), torch.zeros(d), r(d, 3 * d), r(3 * d), r(d, d), r(d), 1, 2, 1e-5,
                            True, caches[0], caches[1], 2, False)
    assert dbl.attn == [] and dbl.steps == 1 and torch.isfinite(y).all()
