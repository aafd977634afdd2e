"""CPU: what can be said without a GPU about attention masks that broadcast over batch and heads: mask_kind's classification (shapes,
strides, no detach and no host probe of a mask that requires grad, the cache of the 2-D probes), the fixture b0_attn_bias.npz against a
float64 restatement written here, and the declaration / binding of the three new entry points."""
import json
import os
import re

import numpy as np
import pytest
import torch

import closed_form as cf
from bias_cases import B, BLOCK_CASES, D, DEC_CASE, GRAD_KEYS, H, N, make_mask
from helpers import GOLDEN, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("afft_attention_fwd_bias", "afft_attention_long_fwd_bias", "afft_attention_bias_bwd")
NEG = float("-inf")


# ----------------------------------------------------------------------------- mask_kind
# mask shape -> element strides (sb, sh, si) of its view as (B, H, N, N)
SHAPES = {(B, 1, 1, N): (N, 0, 0), (1, H, N, N): (0, N * N, N), (H, N, N): (0, N * N, N), (B, 1, N, N): (N * N, 0, N),
          (B, H, N, N): (H * N * N, N * N, N), (1, N): (0, 0, 0), (B, H, 1, N): (H * N, N, 0)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_mask_kind_accepts_every_broadcastable_shape_with_expand_strides(shape):
    from afft_amd import ops
    from afft_amd.functional import mask_bias
    from afft_amd.models.transformerblock import mask_kind
    m = torch.randn(*shape)
    kind = mask_kind(m, N, B, H)
    assert isinstance(kind, tuple) and kind[0] == "bias"
    t = mask_bias(kind)
    assert t is m                                               # fp32 with unit stride: the tensor itself, nothing materialised
    assert ops.bias_strides(t, B, N, H) == SHAPES[shape]
    # another dtype / a strided last dimension: converted, still in its own shape (never the broadcast one)
    t64 = mask_bias(mask_kind(m.double(), N, B, H))
    assert t64.dtype == torch.float32 and tuple(t64.shape) == shape
    if len(shape) == 4 and shape[2] == N:
        tt = mask_bias(mask_kind(m.transpose(-1, -2), N, B, H))
        assert tt.stride(-1) == 1 and torch.equal(tt, m.transpose(-1, -2))


def test_mask_kind_still_recognises_todays_kinds():
    from afft_amd.models.transformerblock import mask_kind
    causal = lambda t: torch.triu(torch.full((t, t), NEG), diagonal=1)   # noqa: E731
    eye = torch.zeros(6, 6)
    eye.fill_diagonal_(NEG)
    assert mask_kind(None, 6) == "none" and mask_kind("causal", 6) == "causal" and mask_kind(("blockcausal", 3), 6) == ("blockcausal", 3)
    assert mask_kind(torch.zeros(6, 6), 6, B, H) == "none"
    assert mask_kind(causal(6), 6, B, H) == "causal"
    assert mask_kind(eye, 6, B, H) == "diag"
    assert mask_kind(causal(3).repeat(2, 2), 6, B, H) == ("blockcausal", 3)
    arb = torch.randn(6, 6)
    kind = mask_kind(arb, 6, B, H)
    assert kind[0] == "table" and kind[1].dtype == torch.float32 and torch.equal(kind[1], arb)
    assert mask_kind(kind, 6) is kind
    with pytest.raises(ValueError):
        mask_kind("banded", 6)


@pytest.mark.parametrize("shape", [(N + 1, N + 1), (N, N + 1), (B + 1, 1, N, N), (B, H + 1, N, N), (B, 1, 2, N), (B, 1, N, 1), (N,), (1, B, H, N, N)])
def test_mask_kind_refuses_what_does_not_broadcast(shape):
    from afft_amd.models.transformerblock import mask_kind
    with pytest.raises(ValueError) as e:
        mask_kind(torch.zeros(*shape), N, B, H)
    msg = str(e.value)
    assert str(tuple(shape)) in msg and f"{N}" in msg and f"({B}|1, {H}|1, {N}|1, {N})" in msg


def test_ops_bias_strides_refuses_a_wrong_batch_size():
    from afft_amd import ops
    with pytest.raises(ValueError, match=r"broadcast to \(3, 4, 5, 5\).*got \(2, 1, 5, 5\)"):
        ops.bias_strides(torch.zeros(2, 1, N, N), B, N, H)
    with pytest.raises(TypeError):
        ops.bias_strides(torch.zeros(B, 1, N, N, dtype=torch.float64), B, N, H)


def test_a_mask_that_requires_grad_is_neither_detached_nor_probed(monkeypatch):
    """whatever its shape, (N, N) and the causal pattern included: ('bias', the tensor itself), and torch.equal is never called"""
    from afft_amd.functional import mask_bias
    from afft_amd.models import transformerblock as tb

    def no_probe(*a, **k):
        raise AssertionError("torch.equal was called on a mask that requires grad")

    monkeypatch.setattr(torch, "equal", no_probe)
    for m in (torch.zeros(N, N), torch.triu(torch.full((N, N), NEG), diagonal=1), torch.randn(H, N, N), torch.randn(B, 1, 1, N)):
        m.requires_grad_(True)
        kind = tb.mask_kind(m, N, B, H)
        assert kind[0] == "bias" and mask_bias(kind) is m and mask_bias(kind).requires_grad
    # a converted one stays attached to its leaf
    m = torch.randn(N, N, dtype=torch.float64, requires_grad=True)
    t = mask_bias(tb.mask_kind(m, N, B, H))
    t.sum().backward()
    assert m.grad is not None and bool((m.grad == 1).all())


def test_the_2d_classification_is_cached_per_storage_version_and_shape(monkeypatch):
    from afft_amd.models import transformerblock as tb
    calls = []
    real = tb._classify_2d
    monkeypatch.setattr(tb, "_classify_2d", lambda m, n: (calls.append(1), real(m, n))[1])
    m = torch.triu(torch.full((6, 6), NEG), diagonal=1)
    assert tb.mask_kind(m, 6) == "causal" and tb.mask_kind(m, 6) == "causal" and len(calls) == 1
    m.zero_()                                                   # an in-place write moves _version: classified again
    assert tb.mask_kind(m, 6) == "none" and len(calls) == 2
    assert tb.mask_kind(m.clone(), 6) == "none" and len(calls) == 3      # another tensor: its own entry


# ----------------------------------------------------------------------------- the fixture against float64 math
def _ln(x, w, b):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def _attend(q, k, v, mask, proj_w, proj_b):
    """q, k, v: [B, N, D] -> (proj(softmax(q k^T hd^-0.5 + mask) v), attention [B, H, N, N])"""
    hd = D // H
    q, k, v = (t.view(B, N, H, hd).transpose(1, 2) for t in (q, k, v))
    attn = ((q @ k.transpose(-2, -1)) * hd ** -0.5 + mask).softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, N, D) @ proj_w.T + proj_b, attn


def _mlp(P, x, norm):
    h = torch.nn.functional.gelu(_ln(x, P[norm + ".weight"], P[norm + ".bias"]) @ P["mlp.mlp.0.weight"].T + P["mlp.mlp.0.bias"])
    return x + h @ P["mlp.mlp.2.weight"].T + P["mlp.mlp.2.bias"]


def _block64(P, x, mask):
    q, k, v = (_ln(x, P["norm1.weight"], P["norm1.bias"]) @ P["attn.qkv.weight"].T).split(D, dim=-1)
    o, attn = _attend(q, k, v, mask, P["attn.proj.weight"], P["attn.proj.bias"])
    return _mlp(P, x + o, "norm2"), attn


def _dec64(P, x, mem, mask):
    q, k, v = (_ln(x, P["norm_self.weight"], P["norm_self.bias"]) @ P["attn.qkv.weight"].T).split(D, dim=-1)
    x = x + _attend(q, k, v, mask, P["attn.proj.weight"], P["attn.proj.bias"])[0]
    xq, mkv = _ln(x, P["norm_q.weight"], P["norm_q.bias"]), _ln(mem, P["norm_kv.weight"], P["norm_kv.bias"])
    x = x + _attend(xq @ P["cross_attn.w_q.weight"].T, mkv @ P["cross_attn.w_k.weight"].T, mkv @ P["cross_attn.w_v.weight"].T, mask,
                    P["cross_attn.proj.weight"], P["cross_attn.proj.bias"])[0]
    return _mlp(P, x, "norm_mlp")


def _fixture():
    z = np.load(os.path.join(GOLDEN, "b0_attn_bias.npz"), allow_pickle=False)
    return z, json.loads(str(z["shapes"]))


def _state64(shapes, tag):
    return {k: cf.tensor_for(f"b0.{tag}.{k}", tuple(s)).double().requires_grad_(True) for k, s in shapes[tag].items()}


def test_fixture_masks_are_the_closed_form_ones_and_hide_no_whole_row():
    z, _ = _fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "b0_attn_bias.npz")) < 1 << 20
    for case in list(BLOCK_CASES) + ["dec"]:
        m, grad = make_mask(case)
        shape, g2 = DEC_CASE if case == "dec" else BLOCK_CASES[case]
        assert tuple(m.shape) == shape and grad == g2
        assert np.array_equal(z[f"{case}.mask"], m.numpy())
        assert bool(torch.isfinite(m).any(dim=-1).all()) and bool(torch.isinf(m).any()) and bool(torch.isfinite(m).any())
        assert (f"{case}.dmask" in z.files) == grad


@pytest.mark.parametrize("case", list(BLOCK_CASES) + ["dec"])
def test_fixture_matches_float64_restatement(case):
    """fp32 reference against float64 math, relative L2 per tensor"""
    z, shapes = _fixture()
    m = torch.from_numpy(z[f"{case}.mask"]).double()
    grad = f"{case}.dmask" in z.files
    m.requires_grad_(grad)
    got = {}
    if case == "dec":
        P = _state64(shapes, "dec")
        x = cf.tensor_for("b0.dec.x", (B, N, D), "input").double().requires_grad_(True)
        mem = cf.tensor_for("b0.dec.mem", (B, N, D), "input").double().requires_grad_(True)
        y = _dec64(P, x, mem, m)
        y.pow(2).mean().backward()
        got.update({"dec.y": y, "dec.dx": x.grad, "dec.dmem": mem.grad})
    else:
        P = _state64(shapes, "block")
        x = cf.tensor_for("b0.block.x", (B, N, D), "input").double().requires_grad_(True)
        y, attn = _block64(P, x, m)
        y.pow(2).mean().backward()
        got.update({f"{case}.y": y, f"{case}.attn": attn, f"{case}.dx": x.grad})
    got.update({f"{case}.grad.{k}": P[k].grad for k in GRAD_KEYS})
    if grad:
        got[f"{case}.dmask"] = m.grad
    want = {k for k in z.files if k.startswith(case + ".") and not k.endswith(".mask")}
    assert want == set(got)
    errs = {k: rel_l2(torch.from_numpy(z[k]), got[k]) for k in sorted(want)}
    print(case, {k: f"{e:.2e}" for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if not e < 1.6e-6}
    assert not bad, bad


# ----------------------------------------------------------------------------- C-ABI
def test_bias_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "afft_hip.h")).read()
    from afft_amd import _lib
    lib = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        fn = getattr(lib, s)
        assert fn is not None and fn.argtypes is not None and fn.restype is not None
    assert re.search(r"scratch: fp32 \[nseq \* H \* L \* L\]", header)


def test_bias_argument_errors_name_the_offending_value():
    """argument checks run before anything touches a device: the dummy pointers are never dereferenced"""
    from afft_amd import _lib
    lib = _lib.lib()
    p, F32 = 4096, _lib.F32
    err = lambda: lib.afft_last_error().decode()   # noqa: E731
    fwd = lambda fn, L, bias, sb, sh, si: fn(p, 64, p, 64, p, 64, F32, 1, L, 1, 64, 0.125, bias, sb, sh, si, 0.0, 0, p, 64, None, None)   # noqa: E731
    bwd = lambda L, db, sb, sh, si, scr: lib.afft_attention_bias_bwd(p, 64, p, 64, F32, p, 1, L, 1, 64, 0.0, 0, db, sb, sh, si, scr, None)   # noqa: E731
    for fn, L in ((lib.afft_attention_fwd_bias, 40), (lib.afft_attention_long_fwd_bias, 160)):
        assert fwd(fn, L, p, -1, 0, L) != 0 and "negative bias stride (sb=-1" in err()
        assert fwd(fn, L, p, 0, 0, -7) != 0 and "si=-7" in err()
        assert fwd(fn, L, p + 2, 0, 0, L) != 0 and "not 4-byte aligned" in err() and "0x1002" in err()
        assert fwd(fn, L, None, 0, 0, L) != 0 and "null pointer" in err()
    assert fwd(lib.afft_attention_fwd_bias, 129, p, 0, 0, 129) != 0 and "sequence length 129 outside 1..128" in err()
    assert fwd(lib.afft_attention_long_fwd_bias, 128, p, 0, 0, 128) != 0 and "sequence length 128 outside 129..512" in err()
    assert fwd(lib.afft_attention_long_fwd_bias, 513, p, 0, 0, 513) != 0 and "sequence length 513 outside 129..512" in err()
    assert bwd(0, p, 0, 0, 40, p) != 0 and "sequence length 0 outside 1..512" in err()
    assert bwd(513, p, 0, 0, 513, p) != 0 and "sequence length 513 outside 1..512" in err()
    assert bwd(40, p, 0, -2, 40, p) != 0 and "sh=-2" in err()
    assert bwd(40, p + 1, 0, 0, 40, p) != 0 and "not 4-byte aligned" in err()
    assert bwd(40, p, 0, 0, 40, None) != 0 and "scratch" in err()
