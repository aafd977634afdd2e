"""Build-container test of the HOST logic of the cached roll-out (BaseFuturePredictor.forward, GPT2Model.forward_step, KVCache) on CPU
tensors, with tests/cpu_ops_step.py standing in for the C-ABI wrappers: which rows reach the QKV GEMM, which positions are added, what
the attention maps look like, and when the cached path engages.  What the kernel computes is tested on the GPU."""
import pytest
import torch

import cpu_ops_step

B, T, D, H, LAYERS = 2, 4, 16, 2, 2


@pytest.fixture()
def predictor():
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.models.future_prediction import BaseFuturePredictor
    saved = rt.kv_cache()
    afft_amd.set_precision("fp32")
    torch.manual_seed(0)
    yield BaseFuturePredictor(D, inter_dim=D, n_layer=LAYERS, n_head=H, output_attentions=True).eval()
    afft_amd.set_precision("bf16")
    rt.set_kv_cache(saved)


class _Spy:
    """records the row counts of the QKV GEMMs (N = 3 D) and the position rows handed to add_rows_periodic"""

    def __init__(self, wpe):
        from afft_amd import ops
        self.ops, self.wpe, self.qkv_rows, self.positions, self.steps = ops, wpe, [], [], 0
        self.gemm, self.add, self.step = ops.gemm, ops.add_rows_periodic, ops.attention_step

    def __enter__(self):
        def gemm(a, b, out, **kw):
            if out.shape[1] == 3 * D:
                self.qkv_rows.append(out.shape[0])
            return self.gemm(a, b, out, **kw)

        def add(x, table, period, y):
            first = (table.data_ptr() - self.wpe.data_ptr()) // (self.wpe.element_size() * self.wpe.shape[1])
            self.positions.append((first, period))
            return self.add(x, table, period, y)

        def step(*a):
            self.steps += 1
            return self.step(*a)
        self.ops.gemm, self.ops.add_rows_periodic, self.ops.attention_step = gemm, add, step
        return self

    def __exit__(self, *exc):
        self.ops.gemm, self.ops.add_rows_periodic, self.ops.attention_step = self.gemm, self.add, self.step


def _run(predictor, feats, output_len, grad=False):
    with cpu_ops_step.installed(), _Spy(predictor.gpt_model.wpe.weight) as spy, torch.set_grad_enabled(grad):
        out, att = predictor(feats, output_len)
    return out, att, spy


def test_cached_rollout_runs_new_rows_only(predictor):
    feats = torch.randn(B, T, D)
    out, att, spy = _run(predictor, feats, 3)
    assert spy.qkv_rows == [B * T] * LAYERS + [B] * LAYERS * 2            # the observed frames once, then one row per clip and frame
    assert spy.positions == [(0, T), (T, 1), (T + 1, 1)]                  # positions advance with the cache
    assert spy.steps == 3 * LAYERS
    assert out.shape == (B, T + 2, D)
    assert att["gpt2_att_0"].shape == (B, LAYERS, H, T, T)                # the reference's shapes (future_prediction.py:395-412)
    assert att["gpt2_att_1"].shape == (B, LAYERS, H, 1, T + 1) and att["gpt2_att_2"].shape == (B, LAYERS, H, 1, T + 2)
    upper = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    assert float(att["gpt2_att_0"][..., upper].abs().max()) == 0.0
    for a in att.values():
        assert torch.allclose(a.sum(-1), torch.ones(()), atol=1e-5)


def test_cached_rollout_equals_recompute(predictor):
    from afft_amd import runtime as rt
    feats = torch.randn(B, T, D)
    out, att, spy = _run(predictor, feats, 3)
    rt.set_kv_cache(False)
    out0, att0, spy0 = _run(predictor, feats, 3)
    assert spy0.steps == 0 and spy0.qkv_rows == [B * T] * LAYERS + [B * (T + 1)] * LAYERS + [B * (T + 2)] * LAYERS
    assert torch.allclose(out, out0, rtol=1e-5, atol=1e-6)
    for k in att0:
        assert att[k].shape == att0[k].shape and torch.allclose(att[k], att0[k], rtol=1e-5, atol=1e-6), k


def test_switch_and_grad_mode_select_the_path(predictor):
    import afft_amd
    from afft_amd import runtime as rt
    feats = torch.randn(B, T, D)
    assert rt.kv_cache()                                                   # default on
    assert _run(predictor, feats, 1)[2].steps == 0                         # output_len == 1: nothing to roll out
    assert _run(predictor, feats, 2, grad=True)[2].steps == 0              # grad enabled: the recompute, which has a backward pass
    predictor.train()
    for m in predictor.modules():                                          # (the CPU double models no dropout)
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    assert _run(predictor, feats, 2)[2].steps == 0                         # training mode
    predictor.eval()
    assert _run(predictor, feats, 2)[2].steps == LAYERS * 2
    rt.set_kv_cache(False)
    assert _run(predictor, feats, 2)[2].steps == 0
    rt.set_kv_cache(True)
    for precision, steps in (("bf16", LAYERS * 2), ("bf16x3", LAYERS * 2), ("fp16x2", 0)):      # fp16x2: one-pass sites are composite-only
        afft_amd.set_precision(precision)
        assert _run(predictor, feats, 2)[2].steps == steps, precision


def test_forward_step_refuses_training_and_overflow(predictor):
    from afft_amd import functional as F_
    gpt = predictor.gpt_model
    with cpu_ops_step.installed(), torch.no_grad():
        cache = gpt.new_cache(B, T, "cpu")
        assert cache.kv.shape == (LAYERS, 2, B, T, D) and cache.kv.dtype == torch.float32 and cache.len == 0
        gpt.forward_step(torch.randn(B * T, D), T, cache)
        assert cache.len == T
        with pytest.raises(ValueError, match="exceed the cache"):
            gpt.forward_step(torch.randn(B, D), 1, cache)
    with cpu_ops_step.installed(), pytest.raises(AssertionError, match="inference path"):
        gpt.forward_step(torch.randn(B, D), 1, F_.KVCache(LAYERS, B, 8, D, "cpu"))


def test_env_switch_turns_it_off():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "from afft_amd import runtime as rt; print(rt.kv_cache())"], cwd=root,
                       env=dict(os.environ, AFFT_KV_CACHE="0"), capture_output=True, text=True)
    assert r.stdout.strip() == "False", (r.stdout, r.stderr)
