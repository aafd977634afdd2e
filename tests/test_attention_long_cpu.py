"""CPU: what can be said about the long-sequence attention (129..512 tokens) without a GPU: the two entry points are declared and
exported, the oracle reproduces both long goldens, and the range errors name the range."""
import os
import re

import pytest
import torch

import closed_form as cf
from helpers import flatten_outputs, load_golden, rel_l2
from long_cases import LONG_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("afft_attention_long_fwd", "afft_attention_long_bwd")


def test_long_entry_points_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "afft_hip.h")).read()
    from afft_amd import _lib
    lib = _lib.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert getattr(lib, s) is not None


@pytest.mark.parametrize("name", list(LONG_CASES))
def test_oracle_matches_long_golden(name):
    """bars of test_oracle_golden.py::test_oracle_matches_reference_golden"""
    from cases import oracle_cfg
    from oracle import afft_oracle as O
    c = LONG_CASES[name]
    z, shapes = load_golden(name)
    state = cf.fill_state(shapes)
    data = cf.inputs_for(name, c["modal_dims"], c["B"], c["T"])
    tgt, sub = cf.labels_for(name, c["B"], c["T"], c["num_classes"], c.get("ignore_frac", 0.25))
    P = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    out = O.base_model_forward(P, data, oracle_cfg(c))
    flat = flatten_outputs(out)
    n = 0
    for k in z.files:
        if k.startswith("out:"):
            assert rel_l2(flat[k[4:]], torch.from_numpy(z[k])) < 2e-5, k
            n += 1
    assert n >= 6
    assert flat["attentions/modality_attns"].shape[-1] == (len(c["modal_dims"]) + bool(c.get("frame_level_token"))) * c["T"] > 128
    total, _ = O.loss(out, tgt, sub)
    assert abs(float(total) - float(z["loss:total"])) < 2e-5 * max(1.0, abs(float(z["loss:total"])))
    total.backward()
    for k in z.files:
        if k.startswith("grad:"):
            assert rel_l2(P[k[5:]].grad, torch.from_numpy(z[k])) < 5e-5, k


@pytest.mark.parametrize("L", [128, 513])
def test_long_range_errors_name_the_range(L):
    """argument checks run before anything touches a device: null-free dummy pointers are never dereferenced"""
    from afft_amd import _lib
    lib = _lib.lib()
    p = 4096
    rc = lib.afft_attention_long_fwd(p, 64, p, 64, p, 64, _lib.F32, 1, L, 1, 64, 0.125, 0, 0, None, 0.0, 0, p, 64, None, None)
    assert rc != 0 and "outside 129..512" in lib.afft_last_error().decode()
    rc = lib.afft_attention_long_bwd(p, 64, p, 64, p, 64, p, 64, _lib.F32, p, 1, L, 1, 64, 0.125, 0.0, 0, p, 64, p, 64, p, 64, p, None)
    assert rc != 0 and "outside 129..512" in lib.afft_last_error().decode()
    rc = lib.afft_attention_long_fwd(p, 64, p, 64, p, 64, _lib.F32, 1, 160, 1, 1025, 0.125, 0, 0, None, 0.0, 0, p, 64, None, None)
    assert rc != 0 and "outside 1..1024" in lib.afft_last_error().decode()


def test_tsa_limit_is_512(monkeypatch):
    """the T-SA-Fuser itself, on the torch test double (the long forward under the double's short restatement, which has no length
    limit): the longest sequence a model of the five known streams reaches, (5 + frame-level token) x 64 frames = 384 tokens, runs and
    returns 384-wide attention maps; 4 x 130 = 520 tokens are refused with the number in the text"""
    import afft_amd
    import cpu_ops
    from afft_amd import ops
    from test_host_logic_cpu import _build

    def long_fwd(q, k, v, nseq, L_, H, hd, scale, mask, out, probs, drop_p=0.0, drop_key=0, mask_period=0, table=None):
        assert table is None
        return cpu_ops.attention_fwd(q, k, v, nseq, L_, H, hd, scale, mask, out, probs, drop_p, drop_key, mask_period)

    try:
        with cpu_ops.installed():
            monkeypatch.setattr(ops, "attention_long_fwd", long_fwd)
            five = {m: 64 for m in ("rgb", "objects", "audio", "poses", "flow")}
            for T, extra, refused in ((64, dict(modal_dims=five, frame_level_token=True), False), (130, {}, True)):
                c = dict(LONG_CASES["t9_tsa_l160"], T=T, **extra)
                model = _build(c, "fp32").eval()
                data = cf.inputs_for("t9_tsa_l160", c["modal_dims"], 1, T)
                tgt, sub = cf.labels_for("t9_tsa_l160", 1, T, c["num_classes"], 0.25)
                with torch.no_grad():
                    if refused:
                        with pytest.raises(NotImplementedError, match=r"520 tokens \(> 512\) are not built"):
                            model(data, mixup_fn=None, target={"action": tgt}, target_subclips={"action": sub},
                                  target_subclips_ignore_index=None)
                    else:
                        out, _ = model(data, mixup_fn=None, target={"action": tgt}, target_subclips={"action": sub},
                                       target_subclips_ignore_index=None)
                        assert flatten_outputs(out)["attentions/modality_attns"].shape[-1] == 384
            monkeypatch.undo()
    finally:
        afft_amd.set_precision("bf16")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(LONG_CASES))
def test_host_wiring_routes_long_sequences_to_the_long_entry_points(name, precision, monkeypatch):
    """functional.py on the torch test double (tests/cpu_ops.py): above 128 tokens the forward and both backward call sites use
    ops.attention_long_fwd / _bwd (here: the double's short restatements under the long names, which have no length limit), never the
    short wrappers or a composite entry point; bars of test_host_logic_cpu.py::test_host_wiring_reproduces_reference_golden"""
    import afft_amd
    import cpu_ops
    from afft_amd import ops
    from test_host_logic_cpu import _build, _step
    c = LONG_CASES[name]
    z, shapes = load_golden(name)
    state = cf.fill_state(shapes)
    data = cf.inputs_for(name, c["modal_dims"], c["B"], c["T"])
    tgt, sub = cf.labels_for(name, c["B"], c["T"], c["num_classes"], c.get("ignore_frac", 0.25))
    Ltok = (len(c["modal_dims"]) + bool(c.get("frame_level_token"))) * c["T"]
    calls = {"fwd": 0, "bwd": 0}

    def long_fwd(q, k, v, nseq, L_, H, hd, scale, mask, out, probs, drop_p=0.0, drop_key=0, mask_period=0, table=None):
        assert L_ == Ltok and table is None
        calls["fwd"] += 1
        return cpu_ops.attention_fwd(q, k, v, nseq, L_, H, hd, scale, mask, out, probs, drop_p, drop_key, mask_period)

    def long_bwd(dout, q, k, v, probs, nseq, L_, H, hd, scale, dq, dk, dv, drop_p=0.0, drop_key=0):
        assert L_ == Ltok
        calls["bwd"] += 1
        return cpu_ops.attention_bwd(dout, q, k, v, probs, nseq, L_, H, hd, scale, dq, dk, dv, drop_p, drop_key)

    def short(*a, **kw):
        assert a[4] <= 128, "a short wrapper was called with a long sequence"
        return short.inner(*a, **kw)

    tol = 6e-2 if precision == "bf16" else 2e-4
    with cpu_ops.installed():
        short.inner = ops.attention_fwd
        monkeypatch.setattr(ops, "attention_fwd", short)
        monkeypatch.setattr(ops, "attention_long_fwd", long_fwd)
        monkeypatch.setattr(ops, "attention_long_bwd", long_bwd)
        model = _build(c, precision)
        model.load_state_dict(state, strict=True)
        model.eval()
        out, total = _step(model, data, tgt, sub)
        monkeypatch.undo()
    afft_amd.set_precision("bf16")
    assert calls == {"fwd": c["depth"], "bwd": c["depth"]}
    flat = flatten_outputs(out)
    for k in z.files:
        if k.startswith("out:") and not k.endswith("modality_attns"):
            assert rel_l2(flat[k[4:]].float(), torch.from_numpy(z[k])) < tol, k
    assert abs(float(total) - float(z["loss:total"])) < tol * max(1.0, abs(float(z["loss:total"])))
    params = dict(model.named_parameters())
    for k in z.files:
        if k.startswith("grad:"):
            assert rel_l2(params[k[5:]].grad, torch.from_numpy(z[k])) < (0.2 if precision == "bf16" else tol), k
