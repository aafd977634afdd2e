"""Build-container test of the HOST logic of the roll-out that trains through the key / value cache (runtime.kv_cache_train,
BaseFuturePredictor._rollout_cached, GPT2Model.forward_step_train, functional.AttnSublayer with `cache`, KVCache's gradient twin) on CPU
tensors, with tests/cpu_ops_step_train.py standing in for the C-ABI wrappers: when the path engages, which rows reach the QKV GEMM, and
that loss, input gradient and every parameter gradient are the recompute's.  What the kernels compute is tested on the GPU."""
import pytest
import torch

import cpu_ops_step_train

B, T, D, H, LAYERS = 3, 4, 16, 2, 2


@pytest.fixture()
def predictor():
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.models.future_prediction import BaseFuturePredictor
    saved = rt.kv_cache(), rt.kv_cache_train(), rt.grad_mode()
    afft_amd.set_precision("fp32")
    rt.set_grad_mode("autograd")
    torch.manual_seed(0)
    yield BaseFuturePredictor(D, inter_dim=D, n_layer=LAYERS, n_head=H, embd_pdrop=0.0, resid_pdrop=0.0, attn_pdrop=0.0,
                              output_attentions=True).eval()
    afft_amd.set_precision("bf16")
    rt.set_kv_cache(saved[0])
    rt.set_kv_cache_train(saved[1])
    rt.set_grad_mode(saved[2])


class _Spy:
    """records the row counts of the GEMMs with N = 3 D (in a forward: the QKV GEMMs) and how often each step op ran"""

    def __init__(self):
        from afft_amd import ops
        self.ops, self.qkv_rows, self.steps, self.step_bwds = ops, [], 0, 0
        self.saved = ops.gemm, ops.attention_step, ops.attention_step_bwd

    def __enter__(self):
        gemm_, step_, bwd_ = self.saved

        def gemm(a, b, out, **kw):
            if out.shape[1] == 3 * D:
                self.qkv_rows.append(out.shape[0])
            return gemm_(a, b, out, **kw)

        def step(*a, **k):
            self.steps += 1
            return step_(*a, **k)

        def bwd(*a, **k):
            self.step_bwds += 1
            return bwd_(*a, **k)
        self.ops.gemm, self.ops.attention_step, self.ops.attention_step_bwd = gemm, step, bwd
        return self

    def __exit__(self, *exc):
        self.ops.gemm, self.ops.attention_step, self.ops.attention_step_bwd = self.saved


def _run(predictor, feats, output_len, grad=True):
    with cpu_ops_step_train.installed(), _Spy() as spy, torch.set_grad_enabled(grad):
        out, att = predictor(feats, output_len)
    return out, att, spy


def test_switch_is_off_by_default_and_selects_the_path(predictor):
    import afft_amd
    from afft_amd import runtime as rt
    feats = torch.randn(B, T, D)
    recompute = [B * T] * LAYERS + [B * (T + 1)] * LAYERS + [B * (T + 2)] * LAYERS
    assert not rt.kv_cache_train()                                          # default off: the recompute, as before
    out0, att0, spy = _run(predictor, feats, 3)
    assert spy.steps == 0 and spy.qkv_rows == recompute
    rt.set_kv_cache_train(True)
    out, att, spy = _run(predictor, feats, 3)
    assert spy.steps == 3 * LAYERS and spy.qkv_rows == [B * T] * LAYERS + [B] * LAYERS * 2      # T + output_len - 1 rows per clip
    assert out.requires_grad and out.shape == (B, T + 2, D)
    assert torch.allclose(out, out0, rtol=1e-5, atol=1e-6)
    assert sorted(att) == sorted(att0)
    for k in att0:                                                          # the same gpt2_att_i shapes
        assert att[k].shape == att0[k].shape and torch.allclose(att[k], att0[k], rtol=1e-5, atol=1e-6), k
    assert _run(predictor, feats, 1)[2].steps == 0                          # output_len == 1: nothing to roll out
    predictor.train()                                                       # training mode without grad: the train path too
    assert _run(predictor, feats, 2, grad=False)[2].steps == 2 * LAYERS
    predictor.eval()
    rt.set_kv_cache(False)                                                  # AFFT_KV_CACHE=0 recomputes everywhere
    assert _run(predictor, feats, 3)[2].qkv_rows == recompute
    rt.set_kv_cache(True)
    afft_amd.set_precision("fp16x2")                                        # fp16x2 keeps recomputing
    predictor.train()
    spy = _run(predictor, feats, 3, grad=False)[2]
    assert spy.steps == 0 and spy.qkv_rows == recompute
    predictor.eval()
    for precision in ("bf16", "bf16x3"):
        afft_amd.set_precision(precision)
        assert _run(predictor, feats, 3)[2].steps == 3 * LAYERS, precision


def test_forward_step_still_refuses_training(predictor):
    from afft_amd import functional as F_
    from afft_amd import runtime as rt
    rt.set_kv_cache_train(True)
    gpt = predictor.gpt_model
    with cpu_ops_step_train.installed(), pytest.raises(AssertionError, match="inference path"):
        gpt.forward_step(torch.randn(B, D), 1, F_.KVCache(LAYERS, B, 8, D, "cpu"))
    with cpu_ops_step_train.installed(), pytest.raises(ValueError, match="gradient twin"):
        gpt.forward_step_train(torch.randn(B, D), 1, F_.KVCache(LAYERS, B, 8, D, "cpu"))
    cache = gpt.new_cache(B, 8, "cpu", grad=True)
    assert cache.gkv.shape == (LAYERS, 2, B, 8, D) and cache.gkv.dtype == torch.float32 and float(cache.gkv.abs().max()) == 0.0
    assert gpt.new_cache(B, 8, "cpu").gkv is None                           # allocated for the training roll-out only


def _loss_and_grads(predictor, feats, output_len):
    x = feats.clone().requires_grad_(True)
    for p in predictor.parameters():
        p.grad = None
    g = torch.Generator().manual_seed(7)
    with cpu_ops_step_train.installed(), _Spy() as spy:
        out, _ = predictor(x, output_len)
        w = torch.randn(out.shape, generator=g)
        loss = (out * w).sum() + out.pow(2).mean()
        loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in predictor.named_parameters() if p.grad is not None}
    return float(loss.detach()), x.grad.detach().clone(), grads, spy


def test_gradients_equal_the_recompute(predictor):
    """2 layers, B = 3, T = 4, output_len = 3: loss, input gradient and every predictor parameter's gradient of the cached-train
    roll-out equal the recompute's to fp32 rounding (the doubles compute in fp32; the two paths add the same terms in another order)"""
    from afft_amd import runtime as rt
    feats = torch.randn(B, T, D, generator=torch.Generator().manual_seed(1))
    rt.set_kv_cache_train(False)
    l0, dx0, g0, spy0 = _loss_and_grads(predictor, feats, 3)
    rt.set_kv_cache_train(True)
    l1, dx1, g1, spy1 = _loss_and_grads(predictor, feats, 3)
    assert spy0.steps == 0 and spy0.step_bwds == 0
    assert spy1.steps == 3 * LAYERS and spy1.step_bwds == 3 * LAYERS
    assert abs(l1 - l0) <= 1e-5 * max(1.0, abs(l0))
    assert torch.allclose(dx1, dx0, rtol=1e-4, atol=1e-6)
    names = [k for k, _ in predictor.named_parameters()]
    assert sorted(g0) == sorted(g1) == sorted(names)                        # every parameter takes a gradient on both paths
    for k in names:
        err = float((g1[k] - g0[k]).norm() / (g0[k].norm() + 1e-30))
        assert err < 1e-5, (k, err)


def test_both_symbols_are_declared_and_bound():
    import ctypes
    from afft_amd import _cabi, _lib
    for name, nargs in (("afft_attention_step_fwd_drop", 24), ("afft_attention_step_bwd", 30)):
        args, res = _cabi.protos[name]
        assert len(args) == nargs and res is ctypes.c_int, name
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib(), name).argtypes == args                   # the built library carries it
    fwd = _cabi.protos["afft_attention_step_fwd"][0]
    drop = _cabi.protos["afft_attention_step_fwd_drop"][0]
    assert drop[:18] == fwd[:18] and drop[18:20] == [ctypes.c_float, ctypes.c_uint32] and drop[20:] == fwd[18:]      # fwd plus (drop_p, drop_key)


def test_env_switch_turns_it_on():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "from afft_amd import runtime as rt; print(rt.kv_cache_train())"], cwd=root,
                       env=dict(os.environ, AFFT_KV_CACHE_TRAIN="1"), capture_output=True, text=True)
    assert r.stdout.strip() == "True", (r.stdout, r.stderr)
