"""GPU: the two long-sequence goldens (tests/golden/long_cases.py: a T-SA-Fuser over 160 and over 320 tokens, produced by the
reference itself) through BaseModel, as test_model_gpu.py::test_model_matches_reference_golden does for the small goldens and with
its tolerances."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import closed_form as cf  # noqa: E402
from helpers import flatten_outputs, load_golden, max_rel, rel_l2  # noqa: E402
from long_cases import LONG_CASES  # noqa: E402
from test_model_gpu import BF16_BWD, GTOL_BF16, TOL, build  # noqa: E402


def long_case_tensors(name):
    c = LONG_CASES[name]
    z, shapes = load_golden(name)
    state = cf.fill_state(shapes)
    data = cf.inputs_for(name, c["modal_dims"], c["B"], c["T"])
    tgt, sub = cf.labels_for(name, c["B"], c["T"], c["num_classes"], c.get("ignore_frac", 0.25))
    return c, z, state, data, tgt, sub


def _forward(model, data, tgt, sub):
    dev = torch.device("cuda:0")
    return model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                 target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3", "fp16x2"])
@pytest.mark.parametrize("name", list(LONG_CASES))
def test_long_model_matches_reference_golden(name, precision):
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    c, z, state, data, tgt, sub = long_case_tensors(name)
    try:
        model = build(c, precision)
        res = model.load_state_dict(state, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        model = model.cuda().eval()
        tol = TOL[precision]
        rt.SINK.begin_step()
        for p in model.parameters():
            p.grad = None
        wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
        out, out_t = _forward(model, data, tgt, sub)
        losses, _ = BasicLossAccuracy(compute_metrics=False)(out, out_t["target"], out_t["target_subclips"])
        total, _ = Runner._reduce_loss(losses, wts, sync=False)
        flat = flatten_outputs(out)
        checked, worst = 0, 0.0
        for k in z.files:
            if not k.startswith("out:"):
                continue
            ref = torch.from_numpy(z[k])
            got = flat[k[4:]].detach().float().cpu()
            assert got.shape == ref.shape, (k, got.shape, ref.shape)
            e, em = rel_l2(got, ref), max_rel(got, ref)
            worst = max(worst, e, em)
            assert e < tol and em < tol * 3, (k, e, em)
            checked += 1
        assert checked >= 6 and "out:attentions/modality_attns" in z.files
        lt = float(z["loss:total"])
        assert abs(float(total) - lt) < tol * max(1.0, abs(lt)), (float(total), lt)
        for k, v in losses.items():
            assert abs(float(v.mean()) - float(z["loss:" + k])) < tol * max(1.0, abs(float(z["loss:" + k]))), k
        total.backward()
        rt.SINK.finish_step(list(model.parameters()))
        torch.cuda.synchronize()
        params = dict(model.named_parameters())
        gtol = GTOL_BF16 if precision in BF16_BWD else tol
        ng, gworst = 0, 0.0
        for k in z.files:
            if k.startswith("grad:"):
                g = params[k[5:]].grad
                assert g is not None, k
                e = rel_l2(g.cpu(), torch.from_numpy(z[k]))
                gworst = max(gworst, e)
                assert e < gtol, (k, e)
                ng += 1
        assert ng >= 5
        for nm, gn in zip([str(s) for s in z["gradnames"]], z["gradnorm"]):
            g = params[nm].grad
            assert g is not None, nm
            assert abs(float(g.norm()) - gn) < gtol * max(gn, 1e-3) * 2, (nm, float(g.norm()), gn)
        print(f"[{name}/{precision}] worst output error {worst:.2e} worst gradient error {gworst:.2e}")
    finally:
        afft_amd.set_precision("bf16")


@pytest.mark.parametrize("name", list(LONG_CASES))
def test_long_fp16x2_no_grad_forward(name):
    import afft_amd
    from afft_amd import runtime as rt
    c, z, state, data, tgt, sub = long_case_tensors(name)
    try:
        model = build(c, "fp16x2")
        model.load_state_dict(state, strict=True)
        model = model.cuda().eval()
        rt.SINK.begin_step()
        with torch.no_grad():
            out, _ = _forward(model, data, tgt, sub)
        flat = flatten_outputs(out)
        checked = 0
        for k in z.files:
            if k.startswith("out:"):
                e = rel_l2(flat[k[4:]].detach().float().cpu(), torch.from_numpy(z[k]))
                assert e < 1e-3, (k, e)
                checked += 1
        assert checked >= 6
    finally:
        afft_amd.set_precision("bf16")


@pytest.mark.parametrize("name", list(LONG_CASES))
def test_long_train_step_is_finite(name):
    """one training-mode step with the reference's drop rates (make_model_cfg's defaults): dropout inside the long attention kernels"""
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    c, z, state, data, tgt, sub = long_case_tensors(name)
    model = build(c, "bf16")
    model.load_state_dict(state, strict=True)
    model = model.cuda().train()
    rt.SINK.begin_step()
    for p in model.parameters():
        p.grad = None
    out, out_t = _forward(model, data, tgt, sub)
    losses, _ = BasicLossAccuracy(compute_metrics=False)(out, out_t["target"], out_t["target_subclips"])
    total, _ = Runner._reduce_loss(losses, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, sync=False)
    total.backward()
    rt.SINK.finish_step(list(model.parameters()))
    torch.cuda.synchronize()
    assert torch.isfinite(total).all()
    for k, v in flatten_outputs(out).items():
        assert torch.isfinite(v.float()).all(), k
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) >= 5 and all(torch.isfinite(g).all() for g in grads)
    afft_amd.set_precision("bf16")


def test_tsa_above_512_tokens_is_refused():
    import afft_amd
    c = dict(LONG_CASES["t9_tsa_l160"], T=130)              # 4 x 130 = 520 tokens
    model = build(c, "bf16").cuda().eval()
    data = cf.inputs_for("t9_tsa_l160", c["modal_dims"], 1, c["T"])
    tgt, sub = cf.labels_for("t9_tsa_l160", 1, c["T"], c["num_classes"], 0.25)
    with pytest.raises(NotImplementedError, match=r"520 tokens \(> 512\)"):
        with torch.no_grad():
            _forward(model, data, tgt, sub)
    afft_amd.set_precision("bf16")
