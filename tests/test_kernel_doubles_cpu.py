"""The float64 / integer doubles of tests/kernel_doubles.py, kept honest without a GPU: the mask replica against the binomial bound of
its own keep rate, act_bwd against torch float64 autograd, loss_reduce against a transcription of Runner._reduce_loss."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import kernel_doubles as kd  # noqa: E402

KEYS = (4321, 0x9E3779B9, 77)      # the keys tests/test_elementwise_gpu.py uses


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("key", KEYS)
def test_keep_fraction_is_within_the_binomial_bound(key, p):
    """n = 2^20 independent keeps of probability 1 - p: the fraction has standard deviation sqrt(p (1 - p) / n); 4 of them"""
    n = 1 << 20
    frac = float(kd.drop_keep(key, np.arange(n), p).mean())
    assert abs(frac - (1.0 - p)) <= 4.0 * math.sqrt(p * (1.0 - p) / n), frac


def test_masks_depend_on_the_key_alone():
    idx = np.arange(1 << 12)
    a, b = kd.drop_keep(KEYS[0], idx, 0.3), kd.drop_keep(KEYS[1], idx, 0.3)
    assert np.array_equal(a, kd.drop_keep(KEYS[0], idx, 0.3))
    assert not np.array_equal(a, b)
    assert np.array_equal(kd.drop_keep(5, idx + (1 << 32), 0.3), kd.drop_keep(5, idx, 0.3))      # the index is taken mod 2^32
    assert kd.drop_thresh(0.5) == 1 << 31 and kd.drop_thresh(1.0) == 0xFFFFFFFF
    assert kd.drop_thresh(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32)                        # the rate is a C float


def test_drop_scales_compose_element_and_path_masks():
    rows, cols = 7, 5
    d = SimpleNamespace(p=0.3, key=KEYS[0], path_p=0.5, path_key=KEYS[2], path_group=3)
    s = kd.drop_scales(d, rows, cols)
    el = kd.drop_keep(d.key, np.arange(rows * cols), d.p).reshape(rows, cols)
    row = kd.drop_keep(d.path_key, np.arange(rows) // 3, d.path_p, path=True)
    assert s.dtype == np.float32 and np.array_equal(s != 0, el & row[:, None])
    kept = np.float32(np.float32(1) / (np.float32(1) - np.float32(0.5))) * np.float32(np.float32(1) / (np.float32(1) - np.float32(0.3)))
    assert set(np.unique(s).tolist()) <= {0.0, float(kept)}
    assert np.array_equal(kd.drop_scales(None, rows, cols), np.ones((rows, cols), dtype=np.float32))


PRE = [0.0, 1e-4, -1e-4, 3.0, -3.0, 9.0, -9.0, 30.0, -30.0, 0.5, -1.7]


@pytest.mark.parametrize("act", ["none", "gelu_erf", "gelu_tanh", "relu", "gate"])
def test_act_bwd_equals_float64_autograd(act):
    code = {"none": kd.ACT_NONE, "gelu_erf": kd.ACT_GELU_ERF, "gelu_tanh": kd.ACT_GELU_TANH, "relu": kd.ACT_RELU,
            "gate": kd.ACT_SIGMOID_GATE}[act]
    pre = torch.tensor(PRE, dtype=torch.float64, requires_grad=True)
    aux = torch.linspace(-2.0, 2.0, len(PRE), dtype=torch.float64).requires_grad_(True)
    dy = torch.linspace(0.5, 1.5, len(PRE), dtype=torch.float64)
    y = {"none": lambda t: t * 1.0, "gelu_erf": torch.nn.functional.gelu,
         "gelu_tanh": lambda t: torch.nn.functional.gelu(t, approximate="tanh"), "relu": torch.relu,
         "gate": lambda t: aux * torch.sigmoid(t)}[act](pre)
    y.backward(dy)
    dpre, daux = kd.act_bwd(code, dy.numpy(), pre.detach().numpy(), aux.detach().numpy())
    assert np.allclose(dpre, pre.grad.numpy(), rtol=1e-12, atol=1e-300)
    if act == "gate":
        assert np.allclose(daux, aux.grad.numpy(), rtol=1e-12, atol=0)
    scale = np.where(np.arange(len(PRE)) % 2 == 0, 2.0, 0.0)
    dropped, _ = kd.act_bwd(code, dy.numpy(), pre.detach().numpy(), aux.detach().numpy(), scale=scale)
    assert np.allclose(dropped, dpre * scale, rtol=1e-15, atol=0)


def _reduce_loss_transcribed(losses, wts):
    """the torch branch of afft_amd.common.runner.Runner._reduce_loss: means of all terms, the total over the weights > 0"""
    means = {k: torch.mean(v) for k, v in losses.items()}
    return torch.sum(torch.stack([w * means[k] for k, w in wts.items() if w > 0])), means


def test_loss_reduce_double_drops_zero_weight_terms():
    g = torch.Generator().manual_seed(3)
    losses = {"cls": torch.randn(257, generator=g, dtype=torch.float64), "bad": torch.full((5,), float("nan"), dtype=torch.float64),
              "feat": torch.randn(40, generator=g, dtype=torch.float64), "inf": torch.full((3,), float("inf"), dtype=torch.float64)}
    wts = {"cls": 1.0, "bad": 0.0, "feat": 0.25, "inf": 0.0}
    total, means = _reduce_loss_transcribed(losses, wts)
    m, t = kd.loss_reduce([v.numpy() for v in losses.values()], list(wts.values()))
    assert math.isfinite(t) and abs(t - float(total)) <= 1e-15 * abs(float(total))
    assert math.isnan(m[1]) and math.isinf(m[3])
    assert np.allclose(m[[0, 2]], [float(means["cls"]), float(means["feat"])], rtol=1e-15, atol=0)
    m0, t0 = kd.loss_reduce([np.zeros(0), np.ones(4)], [1.0, 2.0])
    assert m0[0] == 0.0 and t0 == 2.0
    vals, ok = kd.loss_reduce_bwd([257, 0, 40], [1.0, 0.5, 0.25], g_total=0.5, total=t)
    assert ok == 1.0 and vals[1] is None and vals[0] == np.float32(np.float32(0.5) / np.float32(257))
    assert kd.loss_reduce_bwd([1], [1.0], total=float("nan"))[1] == 0.0 and kd.loss_reduce_bwd([1], [1.0], g_total=float("inf"))[1] == 0.0


def test_small_doubles_equal_torch_float64():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 9, generator=g, dtype=torch.float64)
    x[1, 2] = float("-inf")
    assert np.allclose(kd.softmax_rows(x.numpy()), x.softmax(-1).numpy(), rtol=1e-14, atol=0)
    xr = x.clone().nan_to_num(neginf=-3.0).requires_grad_(True)
    dy = torch.randn(6, 9, generator=g, dtype=torch.float64)
    y = xr.softmax(-1)
    y.backward(dy)
    assert np.allclose(kd.softmax_small_bwd(y.detach().numpy(), dy.numpy()), xr.grad.numpy(), rtol=1e-12, atol=1e-16)
    xs = [torch.randn(6, 11, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(3)]
    w = torch.randn(6, 3, generator=g, dtype=torch.float64, requires_grad=True)
    out = sum(w[:, i:i + 1] * xs[i] for i in range(3))
    dout = torch.randn(6, 11, generator=g, dtype=torch.float64)
    out.backward(dout)
    assert np.allclose(kd.weighted_sum_fwd([t.detach().numpy() for t in xs], w.detach().numpy()), out.detach().numpy(), rtol=1e-14)
    dxs, dw = kd.weighted_sum_bwd([t.detach().numpy() for t in xs], w.detach().numpy(), dout.numpy())
    assert np.allclose(dw, w.grad.numpy(), rtol=1e-12) and all(np.allclose(a, b.grad.numpy(), rtol=1e-14) for a, b in zip(dxs, xs))
    # frames: cat along the frame axis, and the MSE between frame ranges through autograd
    a = torch.randn(2, 5, 4, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(2, 6, 4, generator=g, dtype=torch.float64, requires_grad=True)
    cat = kd.gather_frames(2, 7, 4, [(a.detach().numpy(), 0, 1, 0), (b.detach().numpy(), 1, 7, -1)])
    assert np.array_equal(cat, torch.cat([a[:, :1], b], dim=1).detach().numpy())
    (0.5 * (a[:, 1:4] - b[:, 2:5]).pow(2).sum()).backward()
    da, db = kd.mse_frames_bwd(a.detach().numpy(), b.detach().numpy(), 1, 2, 3, g=0.5)
    assert np.allclose(da, a.grad.numpy(), rtol=1e-14) and np.allclose(db, b.grad.numpy(), rtol=1e-14)
    s, ga, gb = kd.mse(a.detach().numpy()[:, 0], b.detach().numpy()[:, 0])
    assert abs(s - float((a[:, 0] - b[:, 0]).detach().pow(2).sum())) < 1e-12 and np.array_equal(ga, -gb)
    src = torch.randn(11, 3, generator=g, dtype=torch.float64)
    ref = torch.cat([src, torch.zeros(1, 3, dtype=torch.float64)]).view(3, 4, 3).sum(0)
    assert np.allclose(kd.reduce_rows_periodic(src.numpy(), 4), ref.numpy(), rtol=1e-14)


def test_mixup_plan_double():
    sub = np.array([[1, 2], [-1, 3], [4, 5], [6, 7], [8, -1]])
    partner, ign = kd.mixup_plan(sub, 5, -1)
    assert partner.tolist() == [3, 1, 2, 0, 4] and ign.tolist() == [[0, 0], [1, 0], [0, 0], [0, 0], [0, 1]]
    assert kd.mixup_plan(None, 4, -1)[0].tolist() == [3, 2, 1, 0] and kd.mixup_plan(None, 4, -1)[1] is None
    assert kd.mixup_plan(np.array([[1], [-1], [-1]]), 3, -1)[0].tolist() == [0, 1, 2]      # one participant: no mixing
