"""GPU: the HIP path (through the mirrored reference modules, i.e. through the C-ABI) against
(a) the golden vectors produced by the reference itself and (b) the CPU oracle on the same inputs.

Tolerances (north_star: logits within 1e-3 relative fp32): parity (fp32) mode 1e-3 on every output tensor,
loss and gradient -- measured ~1e-6..1e-5; the bf16x3 mode against the same 1e-3 (measured ~1e-5); the bf16 speed mode is
reported against 2e-2 on outputs and 2.5e-2 on gradients (bf16 operand rounding: measured 4e-3..1.1e-2 and 7e-3..1.25e-2 over all
fixtures and the four full-width configurations; SURVEY.md 7 hard part 1 measured 1e-2 for bf16 autocast of the reference
itself), except the score-fusion fixtures, where a bf16 rounding that flips a ReLU gate of MATT moves gradients by up to 8e-2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import CASES, FULL_CASES, oracle_cfg  # noqa: E402
from helpers import (case_tensors, compact_error, flatten_outputs, full_case_tensors, full_gradient_errors, load_golden,  # noqa: E402
                     max_rel, rel_l2, surrogate)

TOL = {"fp32": 1e-3, "bf16": 2e-2, "bf16x3": 1e-3, "fp16x2": 1e-3}
GTOL_BF16 = 2.5e-2
BF16_BWD = ("bf16", "fp16x2")     # precisions whose backward pass is the single-pass bf16 one: gradients against the bf16 bars
                                  # (fp16x2: forward fp16 two-pass -- outputs and losses inside 1e-3 --, backward as bf16)


def build(c, precision):
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    afft_amd.set_precision(precision)
    rt.set_grad_mode("sink")
    cfg = make_model_cfg(c["modal_dims"], c["d"], c["D"], fuser=c["fuser"], depth=c.get("depth", 1),
                         num_heads=c["num_heads"], fp_layers=c["fp_layers"], fp_heads=c["fp_heads"],
                         fp_output_len=c.get("fp_output_len", 1), cross_attn=c.get("cross_attn", False),
                         modal_encoding=c.get("modal_encoding", False),
                         frame_level_token=c.get("frame_level_token", False), T=c["T"], cmfp=c.get("cmfp", "early"),
                         mapping=c.get("mapping", "linear"), mapping_activation=c.get("mapping_activation", "relu"),
                         mapping_layernorm=c.get("mapping_layernorm"), share_predictors=c.get("share_predictors", True),
                         share_classifiers=c.get("share_classifiers", True))
    model = BaseModel(cfg, num_classes={"action": c["num_classes"]}, class_mappings={})
    return model


@pytest.mark.parametrize("name", list(CASES))
def test_fp16x2_forward_matches_reference_golden(name):
    """precision 'fp16x2' in an evaluation forward (no_grad: no bf16 copies are made): every output of every small golden within the north-star 1e-3 of
    the reference"""
    from afft_amd import runtime as rt
    import afft_amd
    z, shapes = load_golden(name)
    c, state, data, tgt, sub = case_tensors(name)
    if c.get("soft"):
        pytest.skip("the MixUp golden is a training-mode case")
    model = build(c, "fp16x2")
    model.load_state_dict(state, strict=True)
    model = model.cuda().eval()
    dev = torch.device("cuda:0")
    try:
        rt.SINK.begin_step()
        with torch.no_grad():
            out, out_t = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                               target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
        flat = flatten_outputs(out)
        worst, checked = 0.0, 0
        for k in z.files:
            if not k.startswith("out:") or (k[4:] == "attentions/modality_attns" and c["fuser"] == "ca"):
                continue
            e = rel_l2(flat[k[4:]].detach().float().cpu(), torch.from_numpy(z[k]))
            worst = max(worst, e)
            assert e < 1e-3, (k, e)
            checked += 1
        assert checked >= 6
        print(f"[{name}/fp16x2] worst output error {worst:.2e}")
    finally:
        afft_amd.set_precision("bf16")


@pytest.mark.parametrize("name", list(CASES))
def test_fp16x2_one_pass_sites_on_the_small_goldens(name):
    """The one-pass sites (runtime.one_pass_sites: every site here, attention core included) forced on at the small goldens' widths
    (set_one_pass_min_dim(0)): every fuser / predictor variant of the goldens runs its composite sub-layers with the AFFT_F16X2_ONE_PASS_*
    flags -- the GEMM launch records show split3 = 4 -- and stays within 2e-3 of the reference's outputs (a wiring error -- a lo plane read
    that was never written, a wrong operand -- would be orders of magnitude; single-pass fp16 sits at ~1e-3, which is why the default keeps
    the second pass at these widths)."""
    from afft_amd import runtime as rt, _lib
    import afft_amd
    z, shapes = load_golden(name)
    c, state, data, tgt, sub = case_tensors(name)
    if c.get("soft"):
        pytest.skip("the MixUp golden is a training-mode case")
    saved_sites, saved_dim = rt.one_pass_sites(), rt.set_one_pass_min_dim(0)
    rt.set_one_pass_sites("linear,conv1d")
    model = build(c, "fp16x2")
    model.load_state_dict(state, strict=True)
    model = model.cuda().eval()
    dev = torch.device("cuda:0")
    try:
        rt.SINK.begin_step()
        _lib.check(_lib.lib().afft_gemm_trace_begin(2048))
        with torch.no_grad():
            out, _ = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                           target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
        torch.cuda.synchronize()
        buf = (_lib.GemmTraceRec * 2048)()
        nrec = _lib.lib().afft_gemm_trace_end(buf, 2048)
        one_pass = sum(1 for i in range(nrec) if buf[i].split3 == 4)
        flat = flatten_outputs(out)
        worst = 0.0
        for k in z.files:
            if not k.startswith("out:") or (k[4:] == "attentions/modality_attns" and c["fuser"] == "ca"):
                continue
            worst = max(worst, rel_l2(flat[k[4:]].detach().float().cpu(), torch.from_numpy(z[k])))
        print(f"[{name}/fp16x2/every site one pass] worst output error {worst:.2e}, {one_pass} of {nrec} traced GEMM launches one fp16 pass")
        assert worst < 2e-3, worst
        assert one_pass >= 4, (one_pass, nrec)      # the composite sub-layers of this golden ran with the flags
    finally:
        afft_amd.set_precision("bf16")
        rt.set_one_pass_sites(saved_sites)
        rt.set_one_pass_min_dim(saved_dim)


@pytest.mark.parametrize("sites", ["two_pass_everywhere", "default"])
@pytest.mark.parametrize("name", ["f_cfg2", "f_ek100"])
def test_fp16x2_forward_full_size(name, sites):
    """the same at the bench's widths and at the EK100 widths of expts/01, against the reference's own outputs
    (tests/golden/f_*.npz).  With every GEMM site on two passes: within 8e-4 (measured 5.7e-4 / see the printed line); with the default
    one-pass sites (runtime.one_pass_sites: the predictor's GEMMs and the fusers' fc2 read one fp16 plane): inside the north star's 1e-3
    with the margin the bar states."""
    import afft_amd
    from afft_amd import runtime as rt
    c, z, state, data, tgt, sub = full_case_tensors(name)
    default_sites = rt.one_pass_sites()
    if sites == "two_pass_everywhere":
        rt.set_one_pass_sites("")
    bar = 8e-4 if sites == "two_pass_everywhere" else 9e-4
    model = build(c, "fp16x2")
    model.load_state_dict(state, strict=True)
    dev = torch.device("cuda:0")
    model = model.to(dev).eval()
    try:
        from afft_amd import _lib
        _lib.check(_lib.lib().afft_gemm_trace_begin(1024))
        with torch.no_grad():
            out, _ = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                           target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
        torch.cuda.synchronize()
        buf = (_lib.GemmTraceRec * 1024)()
        nrec = _lib.lib().afft_gemm_trace_end(buf, 1024)
        one_pass = sum(1 for i in range(nrec) if buf[i].split3 == 4)
        # default: the predictor's 4 GEMMs per layer and the fusers' fc2 run one fp16 pass (afft_gemm_t.split3 = 4) at these widths
        assert (one_pass == 0) if sites == "two_pass_everywhere" else (one_pass >= 12), (one_pass, nrec)
        flat = flatten_outputs(out)
        keys = sorted({k.split(":")[1] for k in z.files if k.startswith("out:")})
        worst = max(compact_error(flat[key].float(), z, "out:" + key) for key in keys)
        print(f"[{name}/fp16x2/{sites}] worst output error {worst:.2e}, {one_pass} of {nrec} GEMM launches one fp16 pass")
        assert worst < bar, worst
    finally:
        afft_amd.set_precision("bf16")
        rt.set_one_pass_sites(default_sites)
        del model
        torch.cuda.empty_cache()


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3", "fp16x2"])
@pytest.mark.parametrize("name", list(CASES))
def test_model_matches_reference_golden(name, precision):
    from afft_amd import runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    from oracle import afft_oracle as O
    z, shapes = load_golden(name)
    c, state, data, tgt, sub = case_tensors(name)
    model = build(c, precision)
    res = model.load_state_dict(state, strict=True)   # identical parameter names and shapes as the reference
    assert not res.missing_keys and not res.unexpected_keys
    model = model.cuda().eval()
    dev = torch.device("cuda:0")
    tol = TOL[precision]
    rt.SINK.begin_step()
    for p in model.parameters():
        p.grad = None
    K = c["num_classes"]
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    if c.get("soft"):
        # the golden was made with the reference's MixUp (Beta sample pinned to lam) inside BaseModel.forward
        # (mixup_backbone path, base_model.py:55-58): run OUR MixUp, on the GPU, the same way
        from afft_amd.common.mixup import MixUp
        mix = MixUp(alpha=0.1, label_smoothing={"action": c["label_smoothing"]}, num_classes={"action": K})

        class _Fixed:
            def sample(self_inner):
                return torch.tensor(c["lam"])
        mix.mixup_beta_sampler = _Fixed()
        out, out_t = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=mix, target={"action": tgt.to(dev)},
                           target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
        losses, _ = BasicLossAccuracy(compute_metrics=False)(out, out_t["target"], out_t["target_subclips"],
                                                             mixup_enable=True,
                                                             target_subclips_ignore_index=out_t["target_subclips_ignore_index"])
        total, _ = Runner._reduce_loss(losses, wts, sync=False)
    else:
        out, out_t = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                           target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
        if c.get("fp_output_len", 1) > 1:
            losses, total = {}, surrogate(out)
        else:
            losses, _ = BasicLossAccuracy(compute_metrics=False)(out, out_t["target"], out_t["target_subclips"])
            total, _ = Runner._reduce_loss(losses, wts, sync=False)
    flat = flatten_outputs(out)
    checked = 0
    worst = 0.0
    for k in z.files:
        if not k.startswith("out:"):
            continue
        key = k[4:]
        if key == "attentions/modality_attns" and c["fuser"] == "ca":
            assert flat[key].shape == (c["B"],)
            continue
        ref = torch.from_numpy(z[k])
        got = flat[key].detach().float().cpu()
        assert got.shape == ref.shape, (key, got.shape, ref.shape)
        e, em = rel_l2(got, ref), max_rel(got, ref)
        worst = max(worst, e, em)
        assert e < tol and em < tol * 3, (key, e, em)
        checked += 1
    assert checked >= 6
    lt = float(z["loss:total"])
    assert abs(float(total) - lt) < tol * max(1.0, abs(lt)), (float(total), lt)
    for k, v in losses.items():
        assert abs(float(v.mean()) - float(z["loss:" + k])) < tol * max(1.0, abs(float(z["loss:" + k]))), k
    total.backward()
    rt.SINK.finish_step(list(model.parameters()))
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    ng = 0
    gworst, gworst_matt = 0.0, 0.0
    gtol = (8e-2 if c.get("cmfp") == "score" else GTOL_BF16) if precision in BF16_BWD else tol
    for k in z.files:
        if k.startswith("grad:"):
            g = params[k[5:]].grad
            assert g is not None, k
            e = rel_l2(g.cpu(), torch.from_numpy(z[k]))
            if ".fuser.matt." in k or ".mapping." in k:
                gworst_matt = max(gworst_matt, e)
            else:
                gworst = max(gworst, e)
            # MATT (two tiny ReLU layers feeding a softmax) and the mapping layers that only feed it: a bf16 rounding
            # that flips one ReLU gate moves their gradients
            kt = gtol * 2 if (precision in BF16_BWD and c.get("cmfp") == "score" and (".fuser.matt." in k or ".mapping." in k)) else gtol
            assert e < kt, (k, e)
            ng += 1
    assert ng >= 5
    names = [str(s) for s in z["gradnames"]]
    for nm, gn in zip(names, z["gradnorm"]):
        g = params[nm].grad
        assert g is not None, nm
        kt = gtol * 2 if (precision in BF16_BWD and c.get("cmfp") == "score" and (".fuser.matt." in nm or ".mapping." in nm)) else gtol
        assert abs(float(g.norm()) - gn) < kt * max(gn, 1e-3) * 2, (nm, float(g.norm()), gn)
    print(f"[{name}/{precision}] worst output error {worst:.2e} worst gradient error {gworst:.2e} (matt/mapping {gworst_matt:.2e})")


def test_autograd_grad_mode_equals_sink():
    """AFFT_GRAD_MODE=autograd (weight grads returned through autograd, e.g. under torch DDP) gives the
    same gradients as the default sink mode."""
    from afft_amd import runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    name = "t0_sa"
    c, state, data, tgt, sub = case_tensors(name)
    dev = torch.device("cuda:0")
    grads = {}
    for mode in ("sink", "autograd"):
        model = build(c, "fp32")
        rt.set_grad_mode(mode)
        model.load_state_dict(state)
        model = model.cuda().eval()
        rt.SINK.begin_step()
        out, out_t = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                           target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
        losses, _ = BasicLossAccuracy(False)(out, out_t["target"], out_t["target_subclips"])
        total, _ = Runner._reduce_loss(losses, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, sync=False)
        total.backward()
        rt.SINK.finish_step(list(model.parameters()))
        grads[mode] = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    rt.set_grad_mode("sink")
    for k in grads["sink"]:
        assert rel_l2(grads["autograd"][k], grads["sink"][k]) < 1e-5, k


@pytest.mark.parametrize("name,train", [("t0_sa", True), ("t0_sa", False), ("t1_ca", True), ("t3_m5", False)])
def test_gradient_handover_equals_separate_kernels(name, train):
    """The LayerNorm-backward kernel emitting the upstream sub-layer's bf16 operand (dropout mask replayed) and its
    output-bias gradient must give the same parameter gradients as the separate cast / column-sum kernels."""
    import afft_amd
    from afft_amd import dropout as D_, functional as F_, runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    c, state, data, tgt, sub = case_tensors(name)
    dev = torch.device("cuda:0")
    grads = {}
    taken = {}
    real_take = F_._take_shadow
    try:
        for on in (True, False):
            rt.set_handover(on)
            rt.set_grad_mode("sink")
            model = build(c, "bf16")
            model.load_state_dict(state)
            model = model.cuda()
            model.train(train)
            D_.manual_seed(11)
            hits = []

            def counting_take(dy, od, bias, _hits=hits):
                sh = real_take(dy, od, bias)
                _hits.append(sh is not None)
                return sh
            F_._take_shadow = counting_take
            rt.SINK.begin_step()
            out, out_t = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                               target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
            losses, _ = BasicLossAccuracy(False)(out, out_t["target"], out_t["target_subclips"])
            total, _ = Runner._reduce_loss(losses, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, sync=False)
            total.backward()
            rt.SINK.finish_step(list(model.parameters()))
            grads[on] = {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters()}
            taken[on] = sum(hits)
    finally:
        F_._take_shadow = real_take
        rt.set_handover(True)
    assert taken[True] > 0 and taken[False] == 0      # the fused path really ran (and only when enabled)
    for k in grads[True]:
        tol = 3e-3 if k.endswith("bias") else 2e-5    # bias: fp32 sums of the masked row vs sums of its bf16 rounding
        assert rel_l2(grads[True][k], grads[False][k]) < tol, (k, rel_l2(grads[True][k], grads[False][k]))


def test_train_mode_dropout_statistics():
    """Train mode: dropout/DropPath are active (outputs differ from eval, differ between steps), finite, and the
    backward pass replays the forward masks (checked on a Linear with input dropout by finite differences)."""
    from afft_amd import dropout as D_, functional as F_, runtime as rt
    import afft_amd
    afft_amd.set_precision("fp32")
    dev = torch.device("cuda:0")
    D_.manual_seed(7)
    x = torch.randn(64, 128, device=dev)
    desc = D_.elementwise(0.25)
    y = F_.ElementDropout.apply(x, desc)
    frac = float((y == 0).float().mean())
    assert 0.2 < frac < 0.3
    kept = y != 0
    assert torch.allclose(y[kept], x[kept] / 0.75, rtol=1e-6)
    y2 = F_.ElementDropout.apply(x, D_.elementwise(0.25))
    assert not torch.equal(y, y2)                              # new key per call
    y3 = F_.ElementDropout.apply(x, desc)
    assert torch.equal(y, y3)                                  # same key -> same mask (what backward relies on)
    # full model in train mode
    c, state, data, tgt, sub = case_tensors("t0_sa")
    model = build(c, "fp32")
    model.load_state_dict(state)
    model = model.cuda().train()
    # reference drop rates (0.1) are already in the cfg built by make_model_cfg
    outs = []
    for _ in range(2):
        rt.SINK.begin_step()
        out, _ = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                       target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
        lg = out["logits/action"]["all-fused"]
        assert torch.isfinite(lg).all()
        outs.append(lg.detach().clone())
        (lg.pow(2).mean() + out["past_logits/action"]["all-fused"].pow(2).mean()).backward()
    assert not torch.equal(outs[0], outs[1])
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", ["t3_m5", "t1_ca", "t2_flt"])
def test_composite_entry_points_equal_call_by_call_path(name, train):
    """afft_{attn,mlp,cross_attn}_sublayer_{fwd,bwd} (one C-ABI call per sub-layer) enqueue the same kernels with the same
    arguments in the same order as the call-by-call path of afft_amd/functional.py: outputs, loss and every gradient are
    BITWISE equal, in eval mode and in train mode (dropout / DropPath keys are drawn by the modules, before either path)."""
    import afft_amd
    from afft_amd import dropout as D_, runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    c, state, data, tgt, sub = case_tensors(name)
    dev = torch.device("cuda:0")
    res = {}
    for comp in (True, False):
        rt.set_composite(comp)
        D_.manual_seed(123)
        model = build(c, "bf16")
        model.load_state_dict(state)
        model = model.cuda().train(train)
        rt.SINK.begin_step()
        out, out_t = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                           target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
        losses, _ = BasicLossAccuracy(False)(out, out_t["target"], out_t["target_subclips"])
        total, _ = Runner._reduce_loss(losses, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, sync=False)
        total.backward()
        rt.SINK.finish_step(list(model.parameters()))
        torch.cuda.synchronize()
        res[comp] = (flatten_outputs(out), float(total), {k: p.grad.clone() for k, p in model.named_parameters()})
    rt.set_composite(True)
    (o1, l1, g1), (o0, l0, g0) = res[True], res[False]
    assert l1 == l0
    for k in o0:
        assert torch.equal(o1[k], o0[k]), k
    assert g1.keys() == g0.keys()
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


@pytest.mark.parametrize("name", ["t2_flt", "t3_m5", "t1_ca"])
def test_total_loss_is_bit_stable_over_200_forwards(name):
    """forward + the three-term loss 200 times on the same batch: ONE bit pattern for the total and for each term (every
    reduction of the path is ordered; round 2's MSE scalar was a float atomicAdd over workgroups and flipped its last bit)"""
    from afft_amd import runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    c, state, data, tgt, sub = case_tensors(name)
    dev = torch.device("cuda:0")
    model = build(c, "bf16")
    model.load_state_dict(state)
    model = model.cuda().eval()
    batch = {m: d.to(dev) for m, d in data.items()}
    crit = BasicLossAccuracy(False)
    seen = set()
    with torch.no_grad():
        for _ in range(200):
            out, out_t = model(batch, mixup_fn=None, target={"action": tgt.to(dev)}, target_subclips={"action": sub.to(dev)},
                               target_subclips_ignore_index=None)
            losses, _ = crit(out, out_t["target"], out_t["target_subclips"])
            total, means = Runner._reduce_loss(losses, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, sync=False)
            assert len(means) == 3
            bits = tuple(int(v.detach().reshape(1).view(torch.int32).item()) for v in [total] + [means[k] for k in sorted(means)])
            seen.add(bits)
    assert len(seen) == 1, seen


def test_marginalize_verb_noun_matches_reference_golden():
    """afft_amd.challenge.marginalize_verb_noun (row softmax kernel + two exact-fp32 MFMA GEMMs on the device, then the
    host-side accuracy bookkeeping) against tests/golden/m0_marginalize.npz, which the reference's own
    challenge.marginalize_verb_noun (challenge.py:196-210) produced on the same closed-form inputs."""
    import os
    import numpy as np
    import pandas as pd
    from afft_amd import challenge as CH
    from closed_form import eval_inputs
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "m0_marginalize.npz"))
    logits, mv, mn, a_lab, v_lab, n_lab = eval_inputs()

    class _DS:
        class_mappings = {("verb", "action"): torch.from_numpy(mv), ("noun", "action"): torch.from_numpy(mn)}
        df = pd.DataFrame(dict(verb_class=v_lab, noun_class=n_lab, action_class=a_lab))
        classes_manyshot = {}
    acc, scores = CH.marginalize_verb_noun(torch.from_numpy(logits).cuda(), _DS, to_prob=True)
    for got, key in zip(scores, ("verb", "noun", "action")):
        assert got.shape == z[key].shape
        assert rel_l2(torch.from_numpy(got), torch.from_numpy(z[key])) < 1e-6, key
    for k, v in zip([str(k) for k in z["acc_names"]], z["acc_values"]):
        assert (np.isnan(v) and np.isnan(acc[k])) or abs(acc[k] - v) < 1e-9, (k, acc[k], v)


@pytest.mark.parametrize("name", ["t3_m5", "t1_ca"])
def test_fused_optimizer_epilogue_equals_separate_update(name):
    """Trainer on one GPU: from step 2 on the Nesterov update of every sub-layer GEMM weight runs in the epilogue of that
    weight's gradient GEMM (afft_sgd_fused_t; the gradient never goes to HBM) and the bucket update kernel only walks the small
    parameters (afft_sgd_nesterov_runs).  Parameters, momentum and bf16 images after 4 steps are BITWISE those of the separate
    update kernels (one shared device function, pinned roundings)."""
    import afft_amd
    from afft_amd import dropout as D_, runtime as rt
    from afft_amd.parallel import Trainer
    c, state, data, tgt, sub = case_tensors(name)
    dev = torch.device("cuda:0")
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    feats = {m: d.to(dev) for m, d in data.items()}
    res = {}
    for fused in (True, False):
        rt.set_fused_sgd(fused)
        D_.manual_seed(5)
        model = build(c, "bf16")
        model.load_state_dict(state)
        model = model.cuda().train()
        tr = Trainer(model, wts, lr=1e-2, momentum=0.9, weight_decay=1e-4, bucket_elems=1 << 15)
        for _ in range(4):
            loss, _ = tr.step(feats, {"action": tgt.to(dev)}, {"action": sub.to(dev)})
        torch.cuda.synchronize()
        if fused:
            assert tr._fused and len(tr._fused) >= 8, "no weight took the fused path"
            assert any(r.shape[0] for r in tr.opt.runs.values())
        else:
            assert tr._fused is None
        res[fused] = (tr.flat.flat_p.clone(), tr.opt.buf.clone(), tr.flat.flat_p16.clone(), float(loss))
    rt.set_fused_sgd(True)
    for a, b, what in zip(res[True], res[False], ("parameters", "momentum", "bf16 images", "loss")):
        assert (a == b) if isinstance(a, float) else torch.equal(a, b), what


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["t0_sa", "t2_flt", "t3_m5"])
def test_last_block_on_token_rows_equals_all_rows(name, precision):
    """runtime.skip_dead_rows (default on): the SA-Fuser's last block runs its MLP half on token 0 of every frame only -- the
    rows models/fusion.py:362-365 keeps.  Against the reference's full row set (skip off): every output and the three losses agree
    to rounding (the token-0 rows go through the same arithmetic; GEMM tile shapes differ) and so does every gradient, including
    the last block's own MLP weights (the dropped rows contribute exact zeros).  The goldens themselves are checked with the
    default (on) by test_model_matches_reference_golden."""
    from afft_amd import runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    c, state, data, tgt, sub = case_tensors(name)
    dev = torch.device("cuda:0")
    res = {}
    for skip in (True, False):
        rt.set_skip_dead_rows(skip)
        model = build(c, precision)
        model.load_state_dict(state)
        model = model.cuda().eval()
        rt.SINK.begin_step()
        out, out_t = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                           target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
        losses, _ = BasicLossAccuracy(False)(out, out_t["target"], out_t["target_subclips"])
        total, _ = Runner._reduce_loss(losses, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, sync=False)
        total.backward()
        rt.SINK.finish_step(list(model.parameters()))
        torch.cuda.synchronize()
        res[skip] = (flatten_outputs(out), float(total), {k: p.grad.clone() for k, p in model.named_parameters()})
    rt.set_skip_dead_rows(True)
    import afft_amd
    afft_amd.set_precision("bf16")
    tol = 1e-5 if precision == "fp32" else 5e-3
    (o1, l1, g1), (o0, l0, g0) = res[True], res[False]
    assert abs(l1 - l0) <= tol * abs(l0)
    for k in o0:
        assert rel_l2(o1[k], o0[k]) <= tol, k
    worst = max((rel_l2(g1[k], g0[k]), k) for k in g0 if float(g0[k].abs().max()) > 0)
    assert worst[0] <= (1e-4 if precision == "fp32" else 2e-2), worst


def test_fused_optimizer_audit_when_the_graph_changes_between_steps():
    """The fused set is learned on one step: a later step that routes a weight differently must not lose its
    update.  (1) A step that SKIPS a sub-layer (its weights get no gradient): the audit applies the regular update to them
    (momentum decay + weight decay, as the bucket kernel would), drops them from the set, and parameters / momentum / bf16
    images stay BITWISE those of a Trainer that never fused.  (2) A step that gives fused weights a SECOND contribution
    (a block applied twice in one forward) raises instead of training on half a gradient."""
    import types
    from afft_amd import dropout as D_, functional as F_, runtime as rt
    from afft_amd.parallel import Trainer
    c, state, data, tgt, sub = case_tensors("t3_m5")
    dev = torch.device("cuda:0")
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    feats = {m: d.to(dev) for m, d in data.items()}
    res = {}
    for fused in (True, False):
        rt.set_fused_sgd(fused)
        D_.manual_seed(5)
        model = build(c, "bf16")
        model.load_state_dict(state)
        model = model.cuda().eval()
        tr = Trainer(model, wts, lr=1e-2, momentum=0.9, weight_decay=1e-4, bucket_elems=1 << 15)
        from afft_amd.models.transformerblock import Block
        blk = [m for m in model.modules() if isinstance(m, Block)][0]      # not the last block: that one runs forward_rows_first_token
        mlp_ids = {id(blk.mlp.mlp[0].weight), id(blk.mlp.mlp[2].weight)}
        orig = blk.forward_rows

        def attention_only(self, x2, L, mask, probs_out=None):
            a = self.attn
            return F_.AttnSublayer.apply(x2, self.norm1.weight, self.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight,
                                         a.proj.bias, L, a.num_heads, mask, self.norm1.eps, False, True, a.scale, None, probs_out)
        for step in range(5):
            if step == 2:
                if fused:
                    assert mlp_ids <= set(tr._fused)
                blk.forward_rows = types.MethodType(attention_only, blk)
            elif step == 3:
                blk.forward_rows = orig
                if fused:
                    assert not (mlp_ids & set(tr._fused)) and len(tr._fused) >= 6
            tr.step(feats, {"action": tgt.to(dev)}, {"action": sub.to(dev)})
        torch.cuda.synchronize()
        res[fused] = (tr.flat.flat_p.clone(), tr.opt.buf.clone(), tr.flat.flat_p16.clone())
        if fused:       # (2) a second gradient contribution to weights already updated in an epilogue
            def twice(self, x2, L, mask, probs_out=None):
                return orig(orig(x2, L, mask)[0], L, mask, probs_out)
            blk.forward_rows = types.MethodType(twice, blk)
            with pytest.raises(RuntimeError, match="fused optimizer"):
                tr.step(feats, {"action": tgt.to(dev)}, {"action": sub.to(dev)})
            torch.cuda.synchronize()
            # the backward pass that raised had queued its end-of-pass join of the auxiliary stream; the engine dropped the
            # callback: the next step must not inherit the "already queued" flag (every later backward would skip its join)
            tr.reducer.begin_step()
            assert not any(d.get("join_queued") for _, d in F_._ALL_STATES)
            assert not any(d.get("pending_ready") for _, d in F_._ALL_STATES)
    rt.set_fused_sgd(True)
    rt.SINK.fused = None
    for a, b, what in zip(res[True], res[False], ("parameters", "momentum", "bf16 images")):
        assert torch.equal(a, b), what


@pytest.mark.parametrize("name", ["cfg2", "ek100"])
def test_full_size_training_is_bitwise_reproducible_and_fused_update_bitwise_equal(name):
    """At the bench's full size (64 clips, dropout on, three streams busy: 256x256 and split-K weight-gradient epilogues updating
    388-614 M parameters beside the data-gradient chain) every reduction of the path is ordered (split-K slices are added up in
    slice order by the last workgroup to arrive, bias column sums in block order by a second kernel; no float atomics), so: (1) two runs of three
    training steps give BIT-IDENTICAL parameters and momentum, and (2) so does the optimizer fused into the weight-gradient
    epilogues against the separate update kernels -- a fused update that started before the data gradient of the same layer had
    read the weight's bf16 image would show up here."""
    import afft_amd
    from afft_amd import dropout as D_, runtime as rt
    from afft_amd.config import BASELINE_CONFIGS, make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.parallel import Trainer
    c = BASELINE_CONFIGS[name]
    B, T, K = 64, c["T"], 3806
    afft_amd.set_precision("bf16")
    rt.set_grad_mode("sink")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(8)
    feats = {m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(dev) for m, C in c["modal_dims"].items()}
    tgt = {"action": torch.randint(0, K, (B,), generator=g).to(dev)}
    sub = {"action": torch.randint(0, K, (B, T, 1), generator=g).to(dev)}
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}

    def run(fused):
        rt.set_fused_sgd(fused)
        D_.manual_seed(17)
        torch.manual_seed(9)
        cfg = make_model_cfg(c["modal_dims"], c["common_dim"], c["fp_inter_dim"], fuser=c["fuser"], T=T)
        model = BaseModel(cfg, {"action": K}, {}).to(dev).train()
        tr = Trainer(model, wts, lr=1e-2)
        for _ in range(3):
            tr.step(feats, tgt, sub)
        torch.cuda.synchronize()
        assert (tr._fused is not None) == fused
        out = tr.flat.flat_p.clone(), tr.opt.buf.clone()
        del tr, model
        torch.cuda.empty_cache()
        return out

    try:
        s1, s2, f1 = run(False), run(False), run(True)
    finally:
        rt.set_fused_sgd(True)
    for i, what in enumerate(("parameters", "momentum")):
        assert torch.equal(s1[i], s2[i]), f"{what}: two runs of the separate update differ"
        assert torch.equal(f1[i], s1[i]), f"{what}: fused update differs from the separate update"


def test_gemm_trace_hook_records_the_kernel_each_launch_ran():
    """afft_gemm_trace_begin / _end (bench.py's roofline source): one record per bf16 fast-path launch, from afft_gemm and from
    inside a composite call alike, with plausible durations, and the variant of the kernel that launch ran (set by its launcher):
    whole 128x128 tiles with an even K-tile count run the steady-state kernel (12, gemm_bf16_g2_kernel), ragged tiles the general
    128x128 kernel (1)."""
    from afft_amd import _lib, ops
    dev = torch.device("cuda:0")
    a = torch.randn(512, 256, device=dev).to(torch.bfloat16)
    b = torch.randn(384, 256, device=dev).to(torch.bfloat16)
    out = torch.empty(512, 384, dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.lib().afft_gemm_trace_begin(16))
    for _ in range(3):
        ops.gemm(a, b, out, b_t=True)
    ops.gemm(a[:500], b, out[:500], b_t=True)                    # 500 rows: a partial tile row
    ops.gemm(a.float(), b.float(), out.float(), b_t=True)      # exact-fp32 path: not traced
    buf = (_lib.GemmTraceRec * 16)()
    n = _lib.lib().afft_gemm_trace_end(buf, 16)
    assert n == 4
    for i in range(3):
        r = buf[i]
        assert (r.M, r.N, r.K, r.a_kstrided, r.b_kstrided, r.variant) == (512, 384, 256, 0, 0, 12) and 0.0 < r.ms < 5.0
    r = buf[3]
    assert (r.M, r.N, r.K, r.a_kstrided, r.b_kstrided, r.variant) == (500, 384, 256, 0, 0, 1) and 0.0 < r.ms < 5.0
    assert _lib.lib().afft_gemm_trace_end(buf, 16) < 0       # no trace open


def test_public_drop_path_module_is_differentiable():
    """models.transformerblock.DropPath in train mode (the standalone form; inside Block it is fused into the GEMM epilogue):
    one keep/drop decision per dim-0 sample, survivors scaled by 1/(1-p), and the gradient flows back through the SAME mask
    (it used to be cut: the output had no grad_fn)."""
    from afft_amd import dropout as D_
    from afft_amd.models.transformerblock import DropPath
    D_.manual_seed(11)
    dev = torch.device("cuda:0")
    x = torch.randn(256, 5, 24, device=dev, requires_grad=True)
    dp = DropPath(0.3).train()
    y = dp(x)
    assert y.grad_fn is not None and y.shape == x.shape
    dropped = (y.detach().abs().sum(dim=(1, 2)) == 0)
    assert 0.15 < float(dropped.float().mean()) < 0.45
    assert torch.allclose(y.detach()[~dropped], x.detach()[~dropped] / 0.7, rtol=1e-6)
    y.sum().backward()
    assert torch.equal(x.grad[dropped], torch.zeros_like(x.grad[dropped]))
    assert torch.allclose(x.grad[~dropped], torch.full_like(x.grad[~dropped], 1 / 0.7), rtol=1e-6)
    assert dp.eval()(x) is x


def test_trainer_fused_sgd_and_weight_images():
    """Trainer on one GPU: flat parameter/gradient buffers, fused Nesterov SGD equal to torch.optim.SGD on the same
    gradients, bf16 weight images refreshed by the SGD kernel, loss goes down."""
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.parallel import Trainer
    afft_amd.set_precision("bf16")
    rt.set_grad_mode("sink")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mods = {"rgb": 128, "objects": 40, "flow": 128}
    cfg = make_model_cfg(mods, 128, 256, depth=2, fp_layers=2, fp_heads=4, drop=0.0)
    model = BaseModel(cfg, {"action": 50}, {}).to(dev).eval()
    B, T = 8, 8
    feats = {m: torch.randn(B, T, C, 1, 1, 1, device=dev) for m, C in mods.items()}
    tgt = {"action": torch.randint(0, 50, (B,), device=dev)}
    sub = {"action": torch.randint(0, 50, (B, T, 1), device=dev)}
    tr = Trainer(model, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, lr=0.01, momentum=0.9,
                 weight_decay=1e-4)
    p0 = tr.flat.flat_p.clone()
    ref_p = torch.nn.Parameter(p0.clone())
    ref_opt = torch.optim.SGD([ref_p], lr=0.01, momentum=0.9, nesterov=True, weight_decay=1e-4)
    losses = []
    for step in range(6):
        loss, _ = tr.forward_backward(feats, tgt, sub)
        losses.append(float(loss))
        if step < 2:   # replay the same gradients through torch's optimizer
            ref_p.data.copy_(tr.flat.flat_p)
            ref_p.grad = tr.flat.flat_g.clone()
        g, scale = tr.reducer.grad_for_optimizer()
        tr.opt.step(g, scale)
        if step < 2:
            if step == 0:
                ref_opt.step()
            else:  # momentum buffer continuity
                ref_opt.state[ref_p]["momentum_buffer"] = tr_prev_buf
                ref_opt.step()
            assert rel_l2(tr.flat.flat_p, ref_p.detach()) < 1e-6
        tr_prev_buf = tr.opt.buf.clone()
        # images written by the SGD kernel match a fresh cast of the weights
        w = model.future_predictor.fuser.blocks[0].attn.qkv.weight
        img = rt.weight_images(w)
        assert torch.equal(img[:w.shape[0], :w.shape[1]], w.detach().to(torch.bfloat16))
        wc = model.future_predictor.classifiers["action"]["all-fused"][1].weight   # 50 x 128: padded cast image
        imgc = rt.weight_images(wc)
        assert torch.equal(imgc[:50, :128], wc.detach().to(torch.bfloat16)) and float(imgc[50:].float().abs().max()) == 0
    assert losses[-1] < losses[0], losses


def test_runner_async_metrics_equal_synchronous():
    """Runner(async_metrics=True): the loss scalars reach the host through one pinned non-blocking copy; same values as
    the reference-style synchronous path."""
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.common.runner import PendingScalars, Runner
    c, state, data, tgt, sub = case_tensors("t0_sa")
    model = build(c, "fp32")
    model.load_state_dict(state)
    model = model.cuda().eval()
    dev = torch.device("cuda:0")
    batch = ({"data_dict": data, "target": {"action": tgt}, "target_subclips": {"action": sub}}, {})
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    rt.SINK.begin_step()
    loss_s, m_s = Runner(model, dev, wts, compute_metrics=False, async_metrics=False)(batch)       # the reference's blocking .item() fetches
    rt.SINK.begin_step()
    loss_l, m_l = Runner(model, dev, wts, compute_metrics=False)(batch)                            # default: lazy values under the same keys
    for k, v in m_s.items():
        assert abs(m_l[k] - v) < 1e-6 * max(1.0, abs(v)), k
    rt.SINK.begin_step()
    loss_a, m_a = Runner(model, dev, wts, compute_metrics=False, async_metrics=True)(batch)
    pend = m_a["losses"]
    assert isinstance(pend, PendingScalars)
    vals = pend.result()
    assert pend.ready()
    assert abs(vals["total_loss"] - float(loss_s)) < 1e-6 * max(1.0, abs(float(loss_s)))
    for k, v in vals.items():
        assert abs(v - m_s[k]) < 1e-6 * max(1.0, abs(m_s[k])), k


FULL_WIDTH = {
    # BASELINE.json config -> (oracle fuser kind, gradient keys checked); B = 2 clips so that the CPU oracle finishes in seconds
    "cfg2": ("sa", ["future_predictor.fuser.blocks.0.attn.qkv.weight", "future_predictor.fuser.blocks.5.mlp.mlp.2.weight",
                    "future_predictor.future_predictor.gpt_model.h.3.mlp.c_fc.weight",
                    "future_predictor.classifiers.action.all-fused.1.weight", "future_predictor.fuser.modal_token"]),
    # cfg4: CA-Fuser (models/fusion.py:218-270), 3 DecoderBlocks, head dim 512, causal 16 x 16 self + cross attention
    "cfg4": ("ca", ["future_predictor.fuser.blocks.0.attn.qkv.weight", "future_predictor.fuser.blocks.2.cross_attn.w_k.weight",
                    "future_predictor.fuser.blocks.1.cross_attn.proj.weight", "future_predictor.fuser.blocks.2.mlp.mlp.0.weight",
                    "future_predictor.fuser.position_embeddings.weight", "future_predictor.future_predictor.gpt_model.h.0.attn.c_attn.weight",
                    "future_predictor.classifiers.action.all-fused.1.bias"]),
    # cfg5: 5 modalities (S = 6 tokens per frame: 2 frames per 16-row MFMA tile, ragged last group), T = 32 (two-tile causal path)
    "cfg5": ("sa", ["future_predictor.fuser.blocks.0.attn.qkv.weight", "future_predictor.fuser.blocks.3.attn.proj.weight",
                    "future_predictor.fuser.blocks.5.mlp.mlp.2.weight", "future_predictor.fuser.norm.weight",
                    "future_predictor.future_predictor.gpt_model.h.5.attn.c_proj.weight",
                    "future_predictor.future_predictor.gpt_model.wpe.weight", "future_predictor.fuser.modal_token"]),
    # the widths expts/01_SA-Fuser_ek100_train.txt trains: 1024 / 352 / 1024 / 1024 -> d = 1024 (mapping GEMM with K = 352),
    # head dim 256, dim_encoder / dim_decoder 1024 <-> 2048
    "ek100": ("sa", ["future_predictor.mapping.objects.mapping.0.weight", "future_predictor.fuser.blocks.0.attn.qkv.weight",
                     "future_predictor.fuser.blocks.5.mlp.mlp.0.weight", "future_predictor.dim_encoder.weight",
                     "future_predictor.dim_decoder.weight", "future_predictor.future_predictor.gpt_model.h.2.mlp.c_proj.weight",
                     "future_predictor.classifiers.action.all-fused.1.weight"]),
}


_FULL_CACHE = {}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16", "fp16x2"])
@pytest.mark.parametrize("name", list(FULL_CASES))
def test_full_size_matches_reference_fixture(name, precision):
    """The HIP path against the REFERENCE ITSELF at the real widths (tests/golden/f_*.npz, made by running the reference on
    closed-form weights: BASELINE cfg1, the EK100 widths of expts/01, cfg2 = the bench workload, cfg4 = CA-Fuser, cfg5 = five modalities at T = 32; 388-614 M
    parameters): every output tensor, the three losses, and the gradient of EVERY parameter (norm + 256-element strided sample).
    fp32 and bf16x3 modes within the north-star 1e-3 (measured: outputs 2.7e-6 / 1.4e-5, worst gradient 4.3e-6 / 2.8e-5); bf16
    within the bf16 bars (measured 5.7e-3..8.1e-3 and 9.3e-3..1.45e-2)."""
    from afft_amd import runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    import afft_amd
    if _FULL_CACHE.get("name") != name:
        _FULL_CACHE.clear()
        _FULL_CACHE.update(name=name, t=full_case_tensors(name))
    c, z, state, data, tgt, sub = _FULL_CACHE["t"]
    model = build(c, precision)
    res = model.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    dev = torch.device("cuda:0")
    model = model.to(dev).eval()
    rt.SINK.begin_step()
    out, out_t = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                       target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
    losses, _ = BasicLossAccuracy(False)(out, out_t["target"], out_t["target_subclips"])
    total, _ = Runner._reduce_loss(losses, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, sync=False)
    total.backward()
    rt.SINK.finish_step(list(model.parameters()))
    torch.cuda.synchronize()
    tol = TOL[precision]
    flat = flatten_outputs(out)
    keys = sorted({k.split(":")[1] for k in z.files if k.startswith("out:")})
    assert len(keys) >= 6
    worst = 0.0
    for key in keys:
        e = compact_error(flat[key].float(), z, "out:" + key)
        worst = max(worst, e)
        assert e < tol, (key, e)
    lt = float(z["loss:total"])
    assert abs(float(total) - lt) < tol * max(1.0, abs(lt)), (float(total), lt)
    for k, v in losses.items():
        assert abs(float(v.mean()) - float(z["loss:" + k])) < tol * max(1.0, abs(float(z["loss:" + k]))), k
    errs = full_gradient_errors({k: p.grad for k, p in model.named_parameters() if p.grad is not None}, z)
    assert len(errs) >= 140
    gw = max(errs, key=errs.get)
    print(f"[{name}/{precision}] vs reference fixture: worst output error {worst:.2e}, worst gradient error {errs[gw]:.2e} ({gw})")
    assert errs[gw] < (GTOL_BF16 if precision in BF16_BWD else tol), (gw, errs[gw])
    del model
    torch.cuda.empty_cache()
    afft_amd.set_precision("bf16")


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3", "fp16x2"])
@pytest.mark.parametrize("name", list(FULL_WIDTH))
def test_full_width_matches_oracle(name, precision):
    """Parity at the FULL widths of every 1-GPU BASELINE.json configuration and of the reference's own EK100 experiment
    (d = D = 2048 or 1024 / 2048, head dims 512 / 256, 6 + 6 layers or 3 DecoderBlocks + 6, 3806 classes, 388-614 M parameters;
    B = 2 clips so that the CPU oracle finishes in seconds): outputs, the three losses and gradients of weights spread over the
    fuser, the predictor, the mappings and the classifier against the oracle on the same random weights."""
    _compare_with_oracle(name, precision, 2)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16x2"])
def test_bench_workload_matches_oracle_at_full_batch(precision):
    """The bench workload ITSELF (BASELINE configs[1]: cfg2, 64 clips, every width 2048, 614 M parameters -- the 256x256 kernels,
    5120-row GEMMs, packed attention groups and token-0 rows of the last block exactly as bench.py runs them) against the CPU
    oracle on the same random weights and inputs: every output, the three losses and seven gradients.  The oracle's fwd + bwd of
    64 clips takes ~15 s on 16 host threads."""
    _compare_with_oracle("cfg2", precision, 64)


def _compare_with_oracle(name, precision, B):
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    from afft_amd.config import BASELINE_CONFIGS, make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from oracle import afft_oracle as O
    c = BASELINE_CONFIGS[name]
    fuser, gkeys = FULL_WIDTH[name]
    T, K = c["T"], 3806
    afft_amd.set_precision(precision)
    rt.set_grad_mode("sink")
    torch.manual_seed(1)
    cfg = make_model_cfg(c["modal_dims"], c["common_dim"], c["fp_inter_dim"], fuser=fuser, T=T, drop=0.0)
    model = BaseModel(cfg, {"action": K}, {}).eval()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k in gkeys:
        assert k in state, k
    g = torch.Generator().manual_seed(2)
    data = {m: torch.randn(B, T, C, 1, 1, 1, generator=g) for m, C in c["modal_dims"].items()}
    tgt = torch.randint(0, K, (B,), generator=g)
    sub = torch.randint(0, K, (B, T, 1), generator=g)
    sub[0, :5] = -1
    dev = torch.device("cuda:0")
    model = model.to(dev)
    rt.SINK.begin_step()
    out, out_t = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target={"action": tgt.to(dev)},
                       target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
    losses, _ = BasicLossAccuracy(False)(out, out_t["target"], out_t["target_subclips"])
    total, _ = Runner._reduce_loss(losses, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, sync=False)
    total.backward()
    rt.SINK.finish_step(list(model.parameters()))
    torch.cuda.synchronize()
    P = {k: (v.clone().requires_grad_(True) if k in gkeys else v) for k, v in state.items()}
    ocfg = dict(fuser=fuser, depth=6, num_heads=4, fp_layers=6, fp_heads=4, fp_output_len=1, num_classes={"action": K})
    nthreads = torch.get_num_threads()
    if B > 8:       # the host of the GPU box has 256 logical cores; torch's CPU kernels are fastest on 16 of them (bench.py's sweep)
        torch.set_num_threads(min(16, nthreads))
    try:
        oout = O.base_model_forward(P, data, ocfg)
        ototal, olosses = O.loss(oout, tgt, sub)
        ototal.backward()
    finally:
        torch.set_num_threads(nthreads)
    tol = TOL[precision]
    worst = 0.0
    for key in ("logits/action", "past_logits/action", "past_futures", "orig_past", "future"):
        e = rel_l2(out[key]["all-fused"].float().cpu(), oout[key]["all-fused"])
        worst = max(worst, e)
        assert e < tol, (key, e)
    if fuser == "sa":   # attention weights (B, depth, T, H, S, S) returned like the reference
        e = rel_l2(out["attentions"]["all-fused"]["modality_attns"].float().cpu(), oout["attentions"]["all-fused"]["modality_attns"])
        worst = max(worst, e)
        assert e < tol, ("modality_attns", e)
    assert abs(float(total) - float(ototal)) < tol * max(1.0, abs(float(ototal)))
    for k, v in olosses.items():
        assert abs(float(losses[k].mean()) - float(v)) < tol * max(1.0, abs(float(v))), k
    params = dict(model.named_parameters())
    gtol = GTOL_BF16 if precision in BF16_BWD else tol
    gworst = 0.0
    for k in gkeys:
        e = rel_l2(params[k].grad.cpu(), P[k].grad)
        gworst = max(gworst, e)
        assert e < gtol, (k, e)
    print(f"[{name} B={B}/{precision}] vs oracle: worst output error {worst:.2e} worst gradient error {gworst:.2e}")
    del model, P, state
    torch.cuda.empty_cache()
    afft_amd.set_precision("bf16")


@pytest.mark.parametrize("name", ["cfg2", "cfg4", "cfg5", "ek100"])
def test_full_size_batch_split_invariants(name):
    """Size-independent properties at the FULL bench size of every 1-GPU BASELINE configuration and of the reference's EK100
    widths (64 clips, bf16 operands, dropout off; cfg2: 4 modalities x T=16 x d=D=2048, 6+6 layers), no oracle involved.  Clips are independent, so (1) a clip's logits do not depend on which batch it
    sits in -- the batch of 64 runs on the 256x256 GEMM kernels, batches of 32 / 8 on other tile paths and split-K -- and (2) the
    data-parallel identity holds: the gradient of the mean loss over 64 clips is the average of the gradients over its two halves
    (what an all-reduce over two ranks computes)."""
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    from afft_amd.config import BASELINE_CONFIGS, make_model_cfg
    from afft_amd.models.base_model import BaseModel
    c = BASELINE_CONFIGS[name]
    B, T, K = 64, c["T"], 3806
    afft_amd.set_precision("bf16")
    rt.set_grad_mode("sink")
    torch.manual_seed(3)
    dev = torch.device("cuda:0")
    cfg = make_model_cfg(c["modal_dims"], c["common_dim"], c["fp_inter_dim"], fuser=c["fuser"], T=T, drop=0.0)
    model = BaseModel(cfg, {"action": K}, {}).to(dev).eval()
    g = torch.Generator().manual_seed(4)
    data = {m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(dev) for m, C in c["modal_dims"].items()}
    tgt = torch.randint(0, K, (B,), generator=g).to(dev)
    sub = torch.randint(0, K, (B, T, 1), generator=g).to(dev)       # no ignored rows: every half has the same number of terms
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    params = [p for p in model.parameters() if p.requires_grad]

    def run(lo, hi):
        rt.SINK.begin_step()
        out, out_t = model({m: d[lo:hi] for m, d in data.items()}, mixup_fn=None, target={"action": tgt[lo:hi]},
                           target_subclips={"action": sub[lo:hi]}, target_subclips_ignore_index=None)
        losses, _ = BasicLossAccuracy(False)(out, out_t["target"], out_t["target_subclips"])
        total, _ = Runner._reduce_loss(losses, wts, sync=False)
        total.backward()
        rt.SINK.finish_step(params)
        torch.cuda.synchronize()
        return (out["logits/action"]["all-fused"].float().clone(), out["past_logits/action"]["all-fused"].float().clone(),
                float(total.detach()), [p.grad.clone() for p in params])

    lg, plg, loss, grads = run(0, B)
    lg_a, plg_a, loss_a, grads_a = run(0, B // 2)
    lg_b, plg_b, loss_b, grads_b = run(B // 2, B)
    lg_s, plg_s, _, _ = run(40, 48)
    # (1) batch independence (different GEMM kernels / tile paths; bf16 operand rounding is the only difference)
    assert rel_l2(torch.cat([lg_a, lg_b]), lg) < 2e-2
    assert rel_l2(torch.cat([plg_a, plg_b]), plg) < 2e-2
    assert rel_l2(lg_s, lg[40:48]) < 2e-2 and rel_l2(plg_s, plg[40:48]) < 2e-2
    # (2) data-parallel identity: loss and gradient of the whole batch = mean over the halves
    assert abs(loss - 0.5 * (loss_a + loss_b)) < 2e-3 * max(1.0, abs(loss))
    num = sum(float(((ga + gb) * 0.5 - gf).double().pow(2).sum()) for gf, ga, gb in zip(grads, grads_a, grads_b))
    den = sum(float(gf.double().pow(2).sum()) for gf in grads)
    assert (num / den) ** 0.5 < 3e-2, (num / den) ** 0.5
    big = max(range(len(params)), key=lambda i: params[i].numel())
    assert rel_l2((grads_a[big] + grads_b[big]) * 0.5, grads[big]) < 5e-2
    del model, grads, grads_a, grads_b
    torch.cuda.empty_cache()


def test_evaluate_loop_scores_and_logit_store(tmp_path):
    """test.py's evaluate / save_logits without per-batch host copies: the collected logits equal the per-batch model
    outputs, the verb / noun scores equal softmax @ mapping, the stored file appends across calls."""
    import numpy as np
    from afft_amd import evaluate as E
    c, state, data, tgt, sub = case_tensors("t0_sa")
    model = build(c, "fp32")
    model.load_state_dict(state)
    model = model.cuda().eval()
    dev = torch.device("cuda:0")
    K = c["num_classes"]
    loader = [({"data_dict": {m: d[i:i + 2] for m, d in data.items()}}, {}) for i in range(0, c["B"], 2)]   # ragged last batch
    key, logits = E.collect_logits(model, loader, dev)
    assert key == "logits/action_all-fused" and logits.shape == (c["B"], K) and logits.is_cuda
    with torch.no_grad():
        ref, _ = model({m: d.to(dev) for m, d in data.items()}, mixup_fn=None, target=None, target_subclips=None,
                       target_subclips_ignore_index=None)
    assert rel_l2(logits, ref["logits/action"]["all-fused"][:, 0, :]) < 1e-5
    g = torch.Generator().manual_seed(3)
    maps = {("verb", "action"): (torch.rand(K, 4, generator=g) < 0.3).float(),
            ("noun", "action"): (torch.rand(K, 5, generator=g) < 0.3).float()}
    sc = E.evaluate_scores(model, maps, loader, dev)
    p = logits.double().softmax(-1).cpu()
    assert rel_l2(torch.from_numpy(sc["verb"]), (p @ maps[("verb", "action")].double()).float()) < 2e-5
    assert rel_l2(torch.from_numpy(sc["noun"]), (p @ maps[("noun", "action")].double()).float()) < 2e-5
    assert np.array_equal(sc["action"], logits.cpu().numpy())
    # the evaluation loops in the evaluation-forward precision: within 1e-3 of the fp32 logits, and the mode is restored
    import afft_amd
    key2, lg2 = E.collect_logits(model, loader, dev, precision="fp16x2")
    assert key2 == key and afft_amd.runtime.precision() == "fp32"
    assert 1e-6 < rel_l2(lg2, logits) < 1e-3, rel_l2(lg2, logits)
    sc2 = E.evaluate_scores(model, maps, loader, dev, precision="fp16x2")
    assert rel_l2(torch.from_numpy(sc2["verb"]), torch.from_numpy(sc["verb"])) < 1e-3
    path = E.save_logits(model, loader, dev, save_dir=str(tmp_path), save_file_name="run1")
    path = E.save_logits(model, loader, dev, save_dir=str(tmp_path), save_file_name="run1")    # appends
    with open(path, "rb") as fh:
        assert fh.read(8) == b"\x89HDF\r\n\x1a\n"          # an HDF5 file, whichever writer made it (h5py or afft_amd.h5lite)
    arr = E.load_logits(path, "logits/action_all-fused")
    assert arr.shape == (2 * c["B"], K) and arr.dtype == np.float32
    assert np.array_equal(arr[:c["B"]], logits.cpu().numpy()) and np.array_equal(arr[:c["B"]], arr[c["B"]:])


def test_trainer_gradient_clipping_matches_torch():
    """opt.grad_clip (train.py:254-260): global-norm clipping with the coefficient kept on the device equals
    torch.nn.utils.clip_grad_norm_ followed by torch's Nesterov SGD."""
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.parallel import Trainer
    afft_amd.set_precision("bf16")
    rt.set_grad_mode("sink")
    dev = torch.device("cuda:0")
    mods = {"rgb": 128, "flow": 128}
    B, T = 8, 8
    g = torch.Generator().manual_seed(21)
    feats = {m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(dev) for m, C in mods.items()}
    tgt = {"action": torch.randint(0, 31, (B,), generator=g).to(dev)}
    sub = {"action": torch.randint(0, 31, (B, T, 1), generator=g).to(dev)}
    torch.manual_seed(6)
    model = BaseModel(make_model_cfg(mods, 128, 256, depth=2, fp_layers=2, fp_heads=4, drop=0.0), {"action": 31}, {}).to(dev).eval()
    clip = 0.05
    tr = Trainer(model, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, lr=0.05, momentum=0.9,
                 weight_decay=1e-4, grad_clip=clip)
    assert not tr.overlap_optimizer            # the whole gradient is needed before the first update
    p0 = tr.flat.flat_p.clone()
    tr.forward_backward(feats, tgt, sub)
    grad = tr.flat.flat_g.clone()
    assert float(grad.norm()) > clip           # the clip is active
    ref_p = torch.nn.Parameter(p0.clone())
    ref_p.grad = grad.clone()
    torch.nn.utils.clip_grad_norm_([ref_p], clip)
    torch.optim.SGD([ref_p], lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4).step()
    gflat, scale = tr.reducer.grad_for_optimizer()
    tr.opt.step(gflat, scale, grad_clip=clip)
    assert rel_l2(tr.flat.flat_p, ref_p.detach()) < 1e-6
    assert abs(float(tr.opt.last_grad_norm) - float(grad.norm())) < 1e-4 * float(grad.norm())


def test_captured_step_graph_equals_eager_and_masks_change():
    """Trainer.capture(): the replayed hipGraph of a whole step (3 streams, fused SGD) gives the same parameters as eager steps
    (dropout off: exact same kernels), and with dropout on the device salt changes the masks from replay to replay."""
    import afft_amd
    from afft_amd import dropout as D_, runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.parallel import Trainer
    afft_amd.set_precision("bf16")
    rt.set_grad_mode("sink")
    dev = torch.device("cuda:0")
    mods = {"rgb": 256, "objects": 96, "audio": 256, "flow": 256}
    B, T = 16, 16
    g = torch.Generator().manual_seed(13)
    feats = {m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(dev) for m, C in mods.items()}
    tgt = {"action": torch.randint(0, 97, (B,), generator=g).to(dev)}
    sub = {"action": torch.randint(0, 97, (B, T, 1), generator=g).to(dev)}
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    try:
        res = {}
        for mode in ("eager", "graph"):
            torch.manual_seed(5)
            cfg = make_model_cfg(mods, 256, 512, depth=2, fp_layers=2, fp_heads=4, drop=0.0)
            model = BaseModel(cfg, {"action": 97}, {}).to(dev).eval()
            tr = Trainer(model, wts, lr=0.01, bucket_elems=1 << 18)
            if mode == "graph":
                tr.capture(feats, tgt, sub, warmup=3)
                for _ in range(4):
                    loss, _ = tr.step(feats, tgt, sub)          # replays
            else:
                for _ in range(7):
                    loss, _ = tr.step(feats, tgt, sub)
            torch.cuda.synchronize()
            res[mode] = (tr.flat.flat_p.clone(), float(loss))
        d = rel_l2(res["graph"][0], res["eager"][0])
        assert d < 5e-5, d                     # same kernels; only the float atomics of the bias column sums differ
        assert abs(res["graph"][1] - res["eager"][1]) < 1e-3 * max(1.0, abs(res["eager"][1]))
        # dropout on, learning rate 0: the parameters never move, yet every replay sees other masks
        torch.manual_seed(5)
        cfg = make_model_cfg(mods, 256, 512, depth=2, fp_layers=2, fp_heads=4, drop=0.1)
        model = BaseModel(cfg, {"action": 97}, {}).to(dev).train()
        tr = Trainer(model, wts, lr=0.0, momentum=0.0, weight_decay=0.0, bucket_elems=1 << 18)
        tr.capture(feats, tgt, sub, warmup=2)
        losses = []
        for _ in range(4):
            loss, _ = tr.step(feats, tgt, sub)
            losses.append(float(loss))
        assert all(l == l for l in losses) and len({round(l, 6) for l in losses}) == 4, losses
        assert max(losses) - min(losses) < 0.2 * abs(losses[0])      # ... masks, not garbage
    finally:
        D_.disable_device_salt()


def test_captured_graph_takes_new_batches_by_copy():
    """Trainer.step() with a captured graph and FRESH tensors (the normal data-loader pattern: new feature and label tensors every
    step): every incoming tensor is copied into the tensors the graph reads -- labels included (the round-1 replay compared only the
    ids of the feature tensors and silently trained on the labels frozen at capture time) -- and a batch of another shape falls
    back to an eager step."""
    import afft_amd
    from afft_amd import dropout as D_, runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.parallel import Trainer
    afft_amd.set_precision("bf16")
    rt.set_grad_mode("sink")
    dev = torch.device("cuda:0")
    mods = {"rgb": 128, "flow": 128}
    B, T, K = 8, 8, 31
    g = torch.Generator().manual_seed(21)
    mk = lambda: ({m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(dev) for m, C in mods.items()},       # noqa: E731
                  {"action": torch.randint(0, K, (B,), generator=g).to(dev)},
                  {"action": torch.randint(0, K, (B, T, 1), generator=g).to(dev)})
    batches = [mk() for _ in range(4)]
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    try:
        out = {}
        for mode in ("eager", "graph"):
            torch.manual_seed(3)
            cfg = make_model_cfg(mods, 128, 256, depth=1, fp_layers=1, fp_heads=4, drop=0.0)
            model = BaseModel(cfg, {"action": K}, {}).to(dev).eval()
            tr = Trainer(model, wts, lr=0.05, bucket_elems=1 << 16)
            if mode == "graph":
                f0, t0, s0 = (dict((k, v.clone()) for k, v in d.items()) for d in batches[0])
                tr.capture(f0, t0, s0, warmup=2)           # 2 eager steps on batch 0
            else:
                for _ in range(2):
                    tr.step(*batches[0])
            losses = [float(tr.step(*b)[0]) for b in batches[1:]]          # fresh tensors every step
            torch.cuda.synchronize()
            out[mode] = (losses, tr.flat.flat_p.clone())
        assert rel_l2(out["graph"][1], out["eager"][1]) < 5e-5
        for a, b in zip(out["graph"][0], out["eager"][0]):
            assert abs(a - b) < 1e-3 * max(1.0, abs(b)), (out["graph"][0], out["eager"][0])
        small = ({m: v[:4].contiguous() for m, v in batches[1][0].items()}, {"action": batches[1][1]["action"][:4].contiguous()},
                 {"action": batches[1][2]["action"][:4].contiguous()})
        loss, _ = tr.step(*small)                          # other shapes: eager fall-back, no replay on stale tensors
        assert torch.isfinite(loss)
    finally:
        D_.disable_device_salt()


def test_overlapped_optimizer_and_wgrad_streams_equal_serial():
    """Per-bucket SGD on the side stream (under backward) and weight-gradient GEMMs on the auxiliary stream must give
    the same parameters as the fully serial schedule (same kernels, same order of accumulation)."""
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.parallel import Trainer
    afft_amd.set_precision("bf16")
    rt.set_grad_mode("sink")
    dev = torch.device("cuda:0")
    mods = {"rgb": 256, "objects": 96, "audio": 256, "flow": 256}
    B, T = 16, 16
    g = torch.Generator().manual_seed(3)
    feats = {m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(dev) for m, C in mods.items()}
    tgt = {"action": torch.randint(0, 97, (B,), generator=g).to(dev)}
    sub = {"action": torch.randint(0, 97, (B, T, 1), generator=g).to(dev)}
    results = {}
    for mode in ("serial", "serial2", "overlap", "overlap2"):
        rt.set_overlap_wgrad(mode.startswith("overlap"))
        torch.manual_seed(5)
        cfg = make_model_cfg(mods, 256, 512, depth=3, fp_layers=3, fp_heads=4, drop=0.0)
        model = BaseModel(cfg, {"action": 97}, {}).to(dev).eval()
        tr = Trainer(model, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, lr=0.01,
                     bucket_elems=1 << 18, overlap_optimizer=mode.startswith("overlap"))
        assert len(tr.reducer.buckets) >= 4
        for _ in range(3):
            loss, _ = tr.step(feats, tgt, sub)
        torch.cuda.synchronize()
        results[mode] = (tr.flat.flat_p.clone(), float(loss))
    rt.set_overlap_wgrad(True)
    p_s, l_s = results["serial"]
    p_o, l_o = results["overlap"]
    # bias-gradient column sums and loss sums use fp32 atomics, so two runs of the SAME schedule differ in the last
    # bits, and one flipped bf16 rounding of a weight image turns that into a ~1e-5 relative difference (observed
    # bimodal: 1e-10 or 1e-5 between identical schedules); calibrate on serial-vs-serial with that floor.  A missing
    # stream dependency shows up orders of magnitude above it.
    noise = max(rel_l2(results["serial2"][0], p_s), rel_l2(results["overlap2"][0], p_o), 1e-7)
    d = rel_l2(p_o, p_s)
    print(f"serial-vs-serial noise {noise:.2e}, overlap-vs-serial {d:.2e}")
    assert d < 5 * noise + 3e-5, (d, noise)
    assert abs(l_s - l_o) < 1e-3 * max(1.0, abs(l_s)), (l_s, l_o)


def test_rccl_path_single_rank():
    """The collective path of the trainer (bucket -> side stream -> bf16 cast -> RCCL all-reduce -> per-bucket SGD on
    bf16 gradients) run in a 1-rank "nccl" (= RCCL) group on one GPU: must equal the no-communication result up to the
    bf16 rounding of the gradient payload."""
    import os
    import torch.distributed as dist
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.parallel import Trainer
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    dev = torch.device("cuda:0")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        created = True
    try:
        afft_amd.set_precision("bf16")
        rt.set_grad_mode("sink")
        mods = {"rgb": 128, "flow": 128}
        g = torch.Generator().manual_seed(9)
        B, T = 8, 8
        feats = {m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(dev) for m, C in mods.items()}
        tgt = {"action": torch.randint(0, 31, (B,), generator=g).to(dev)}
        sub = {"action": torch.randint(0, 31, (B, T, 1), generator=g).to(dev)}
        out = {}
        for mode in ("none", "fp32", "bf16"):
            torch.manual_seed(1)
            cfg = make_model_cfg(mods, 128, 128, depth=2, fp_layers=2, fp_heads=4, drop=0.0)
            model = BaseModel(cfg, {"action": 31}, {}).to(dev).eval()
            tr = Trainer(model, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, lr=0.01,
                         bucket_elems=1 << 16, comm_dtype="fp32" if mode == "none" else mode, force_comm=(mode != "none"))
            for _ in range(3):
                loss, _ = tr.step(feats, tgt, sub)
            torch.cuda.synchronize()
            out[mode] = tr.flat.flat_p.clone()
        assert rel_l2(out["fp32"], out["none"]) < 5e-5
        assert rel_l2(out["bf16"], out["none"]) < 2e-3      # bf16 rounding of the gradient payload
    finally:
        if created:
            dist.destroy_process_group()


def test_bench_two_ranks_rehearsal_on_one_gpu():
    """The N > 1 leg of bench.py as the driver launches it (python -m torch.distributed.run, one process per rank), rehearsed
    on this one-GPU box: both ranks on cuda:0, gradient exchange over gloo (RCCL refuses two ranks on a device).  Everything but
    the RCCL calls themselves is the 8-GPU path: parameter broadcast, bucketed reducer on its side stream with the optimizer
    behind it, barriers, max-over-ranks timing, the communication report.  Checks the JSON line's bookkeeping (whole-job value =
    2 ranks' clips), that the exchange really ran (world size 2, >= 1 bucket, finite losses for both payload types), and that
    the line is marked as a rehearsal."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AFFT_BENCH_BACKEND="gloo", AFFT_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2",
           "--config", "ek100", "--batch", "8", "--no-parity-mode", "--no-cpu-baseline", "--no-roofline", "--full"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and "REHEARSAL" in d["data"]
    assert d["config"]["global_batch"] == 16 and d["config"]["parallelism"] == "dp2"
    assert abs(d["value"] - 16 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
    comm = d["comm"]
    assert comm["world_size"] == 2 and comm["backend"] == "gloo" and comm["buckets"] >= 1
    # headline = the all-reduce form (north star / train.py:364-368); the sharded step is timed beside it in the same job
    assert d["config"]["grad_comm_algo"] == "allreduce" and d["optimizer_path"] == "separate"
    sh = comm["sharded"]
    assert "error" not in sh and sh["ms_per_step"] > 0 and sh["sharded_buckets"] >= 1 and sh["optimizer_path"] == "sharded", sh
    losses = comm["loss_after_20_steps"]
    assert all(v == v and abs(v) < 1e4 for v in losses.values())
    assert abs(comm["loss_delta_bf16_vs_fp32_payload"]) < 0.05 * abs(losses["fp32"])


def test_bench_launches_itself_for_two_ranks():
    """The BARE form `python bench.py --gpus 2` (no launcher, no WORLD_SIZE): bench.py starts `python -m torch.distributed.run`
    itself as a child process (reference: run.py:34-51 does the same with torchrun), relays rank 0's JSON line and the return
    code.  Rehearsal mode on this one-GPU box (both ranks on cuda:0, gloo).  `--gpus 1` stays a plain single process."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AFFT_BENCH_BACKEND="gloo", AFFT_BENCH_SHARE_GPU="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR", "LOCAL_WORLD_SIZE", "GROUP_RANK"):
        env.pop(k, None)
    common = ["--steps", "2", "--warmup", "1", "--config", "ek100", "--batch", "8", "--no-parity-mode", "--no-cpu-baseline", "--full"]
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--no-roofline", "--no-comm-report"] + common,
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 16
    assert d["optimizer_path"] == "separate" and d["config"]["grad_comm_algo"] == "allreduce" and "REHEARSAL" in d["data"]      # the N > 1 headline: all-reduce
    assert d["comm"]["sharded"]["ms_per_step"] > 0      # ... with the sharded step timed beside it
    r1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + common, cwd=root, env=env,
                        capture_output=True, text=True, timeout=900)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-4000:]
    d1 = json.loads([ln for ln in r1.stdout.splitlines() if ln.startswith("{")][0])
    assert d1["n_gpus"] == 1 and d1["optimizer_path"] == "fused-epilogue" and d1["roofline"]["frac"] > 0
    assert d1["separate_update"]["ms_per_step"] > 0      # the N = 1 anchor on the N > 1 ranks' code path
    assert d1["roofline"]["traffic"] is None              # no committed --pmc profile of THIS workload (ek100, 8 clips): null, not cfg2's bytes
    # a failing rank's return code comes back through the launcher
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", "no_such_config"] + common[:4],
                         cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert bad.returncode != 0


def test_bench_plain_run_is_the_headline_and_dumps_outputs(tmp_path):
    """`python bench.py --gpus 1` without --full: the headline line alone (no side measurement) over exactly --steps timed steps,
    and with --dump-outputs the last timed step's loss (the line's final_loss), its terms and the parameter / momentum samples as
    finite float64 / float32 .npy files, under 64 MB in all."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR", "LOCAL_WORLD_SIZE", "GROUP_RANK"):
        env.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "ek100",
                        "--batch", "8", "--dump-outputs", str(out)], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "bf16" and d["higher_is_better"] is True and d["unit"] == "clips/s"
    assert abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
    side = {"separate_update", "reference_row_set", "roofline", "hbm_kernels", "power", "fwd_p50_ms", "parity_mode", "ek100", "small_batch",
            "reference_loop", "cpu_baseline", "comm"}
    assert not side & set(d), side & set(d)
    files = {f.name: np.load(f) for f in out.iterdir()}
    assert {"loss.npy", "params_sample.npy", "momentum_sample.npy"} <= set(files) and any(k.startswith("loss_") for k in files)
    assert sum(f.stat().st_size for f in out.iterdir()) < 64 << 20
    for k, v in files.items():
        assert v.dtype == (np.float64 if k.startswith("loss") else np.float32) and v.size > 0 and np.isfinite(v).all(), k
    assert abs(float(files["loss.npy"][0]) - d["final_loss"]) < 1e-4 * max(1.0, abs(d["final_loss"]))
    assert files["params_sample.npy"].shape == files["momentum_sample.npy"].shape and np.abs(files["momentum_sample.npy"]).max() > 0


@pytest.mark.parametrize("fail", ["sharded", "sharded_hang", "headline_sharded"])
def test_bench_two_ranks_headline_survives_a_failing_side_leg(fail):
    """The first 8-GPU contact must not be losable (VERDICT r5 #3b).  Rehearsed on this box (two gloo ranks on cuda:0) with the test
    hooks of bench.py: the sharded leg RAISES on every rank ('sharded': caught, recorded, the all-reduce headline line is printed),
    it HANGS ('sharded_hang': after --side-leg-budget seconds rank 0 prints the headline as it stood and every rank exits 0), or the
    whole first child fails ('headline_sharded' with --comm-algo sharded: the launcher, which never touched a GPU, starts a fresh
    all-reduce-only child and relays ITS line, marked `fallback_after`).  Exactly one JSON line each time, rc 0."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AFFT_BENCH_BACKEND="gloo", AFFT_BENCH_SHARE_GPU="1", AFFT_BENCH_FAIL_LEG=fail)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR", "LOCAL_WORLD_SIZE", "GROUP_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--config", "ek100", "--batch", "8",
           "--no-parity-mode", "--no-cpu-baseline", "--no-roofline", "--no-comm-report", "--full"]
    if fail == "sharded_hang":
        cmd += ["--side-leg-budget", "8"]
    if fail == "headline_sharded":
        cmd += ["--comm-algo", "sharded"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["grad_comm_algo"] == "allreduce"
    if fail == "sharded":
        assert "AFFT_BENCH_FAIL_LEG" in d["comm"]["sharded"]["error"]
    elif fail == "sharded_hang":
        assert d["side_leg_cut"].startswith("sharded leg")
    else:
        assert "fallback_after" in d and "code" in d["fallback_after"]


def _run_two_rank_worker(tmp_path, case, precision, algo, steps=3):
    """tests/scripts/two_rank_gpu.py: two gloo ranks on cuda:0 (algo 'allreduce' | 'sharded') or one process (algo 'none')"""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tests", "scripts", "two_rank_gpu.py")
    out = str(tmp_path / f"{case}_{precision}_{algo}.pt")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "LOCAL_WORLD_SIZE", "GROUP_RANK"):
        env.pop(k, None)
    tail = [script, case, precision, algo, str(steps), out]
    if algo == "none":
        cmd = [sys.executable] + tail
    else:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port)] + tail
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(out)


@pytest.mark.parametrize("case", ["t0_sa", "t3_m5"])
def test_two_ranks_on_one_gpu_match_single_process_and_each_other(tmp_path, case):
    """D1 (train.py:364-368 DDP wrap, :252 backward-time all-reduce) on the REAL HIP path: two ranks (gloo, both on cuda:0) step
    three times on half-batches in the exact-fp32 mode with comm_algo 'allreduce' and 'sharded'.  Checked: (1) the two replicas of
    a run hold bitwise-equal parameters, momentum, bf16 images and evaluation logits (rank 1 started from perturbed weights: the
    construction-time broadcast); (2) parameters and momentum of both forms equal one process stepping on the whole batch to 1e-6
    (summation order of the two halves), logits to 1e-5; (3) the two forms agree BITWISE by name (a + b is the same sum in an
    all-reduce and in a reduce-scatter; the sliced update kernel is elementwise) -- which it would not if the sharded replicas had
    read stale fp32 masters anywhere (embedding tables stay replicated, 'fp32' precision gathers the masters: ADVICE r5);
    (4) state_dict() on stale masters raises instead of communicating, the evaluation forward refreshes them."""
    one = _run_two_rank_worker(tmp_path, case, "fp32", "none")
    runs = {a: _run_two_rank_worker(tmp_path, case, "fp32", a) for a in ("allreduce", "sharded")}
    for a, r in runs.items():
        assert r["info"]["replicas_bitwise_equal"], a
        assert r["info"]["buckets"] >= 3, r["info"]
        assert r["state_dict_keys"] == one["state_dict_keys"]
        for grp, tol in (("params", 1e-6), ("momentum", 2e-5)):
            ref = torch.cat([one[grp][k].reshape(-1) for k in sorted(one[grp])])
            got = torch.cat([r[grp][k].reshape(-1) for k in sorted(one[grp])])
            assert rel_l2(got, ref) < tol, (a, grp, rel_l2(got, ref))
        assert rel_l2(r["logits"], one["logits"]) < 1e-5, (a, rel_l2(r["logits"], one["logits"]))
    sh = runs["sharded"]["info"]
    assert 0 < sh["split"] < sh["total"] and 2 <= sh["sharded_buckets"] < sh["buckets"], sh
    assert sh["stale_before_sync"] and sh["state_dict_on_stale_masters"] == "raised" and not sh["stale_after_eval_forward"], sh
    a, b = runs["allreduce"], runs["sharded"]
    for grp in ("params", "momentum", "images"):
        assert a[grp].keys() == b[grp].keys()
        for k in a[grp]:
            assert torch.equal(a[grp][k], b[grp][k]), (grp, k)
    assert torch.equal(a["logits"], b["logits"])


@pytest.mark.parametrize("precision", ["bf16", "fp16x2"])
def test_two_ranks_on_one_gpu_sharded_equals_allreduce_in_the_16_bit_modes(tmp_path, precision):
    """The same two forms in the precisions the sharded update was built for (only the 16-bit IMAGES of the other rank's slice are
    gathered per step; fp32 masters lazily): parameters, momentum, images and evaluation logits bitwise equal between the forms and
    between the replicas, after sync_masters().  The all-reduce form never has stale state, so any fp32 read of a sharded
    parameter in a forward pass (GPT-2 wpe, position embeddings: ADVICE r5 high) shows up here as a difference."""
    runs = {a: _run_two_rank_worker(tmp_path, "t0_sa", precision, a, steps=4) for a in ("allreduce", "sharded")}
    a, b = runs["allreduce"], runs["sharded"]
    assert a["info"]["replicas_bitwise_equal"] and b["info"]["replicas_bitwise_equal"]
    assert b["info"]["stale_before_sync"] and not b["info"]["stale_after_eval_forward"]
    for grp in ("params", "momentum", "images"):
        for k in a[grp]:
            assert torch.equal(a[grp][k], b[grp][k]), (grp, k)
    assert torch.equal(a["logits"], b["logits"])
    assert all(x == y for x, y in zip(a["info"]["losses"], b["info"]["losses"])), (a["info"]["losses"], b["info"]["losses"])


def test_forward_under_no_grad_equals_forward_with_grad():
    """A forward nobody will differentiate skips what only backward reads (the MLP's pre-activation store, u = NULL in
    afft_mlp_sublayer_fwd): every output must be bit-identical to the forward of a differentiated pass."""
    c, state, data, tgt, sub = case_tensors("t0_sa")
    model = build(c, "bf16")
    model.load_state_dict(state)
    dev = torch.device("cuda:0")
    model = model.to(dev).eval()
    kw = dict(mixup_fn=None, target={"action": tgt.to(dev)}, target_subclips={"action": sub.to(dev)}, target_subclips_ignore_index=None)
    feats = {m: d.to(dev) for m, d in data.items()}
    with_grad, _ = model(feats, **kw)
    with torch.no_grad():
        without, _ = model(feats, **kw)
    fa, fb = flatten_outputs(with_grad), flatten_outputs(without)
    assert fa["logits/action/all-fused"].requires_grad and not fb["logits/action/all-fused"].requires_grad
    for k in fa:
        assert torch.equal(fa[k].detach(), fb[k]), k


# ----------------------------------------------------------------------------- round 4: the reference's own loop on the fast path
def _reference_loop(model, opt, sched, feats, tgt, sub, steps, mixup_fn=None, async_metrics=False):
    """train.py:241-265: runner -> zero_grad -> backward -> step -> scheduler.step"""
    from afft_amd.common.runner import Runner
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    runner = Runner(model, torch.device("cuda:0"), wts, compute_metrics=False, async_metrics=async_metrics)
    batch = ({"data_dict": feats, "target": {"action": tgt}, "target_subclips": {"action": sub}}, {})
    for _ in range(steps):
        loss, _ = runner(batch, mixup_fn, True)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if sched is not None:
            sched.step()
    return loss


@pytest.mark.parametrize("name", ["t3_m5", "t0_sa"])
def test_reference_loop_with_dropin_sgd_equals_trainer_bitwise(name):
    """the reference-shaped loop (Runner + afft_amd.optim.SGD over prepare_params' per-parameter groups, with
    dropout on) == Trainer.step, bit for bit, after 4 steps -- parameters, momentum, bf16 images -- and the optimizer took the
    fused-epilogue path; a Warmup(CosineLR) scheduler on both sides (Trainer's lr set by hand) keeps them equal."""
    from afft_amd import dropout as D_, runtime as rt
    from afft_amd.common.scheduler import CosineLR, Warmup, prepare_params
    from afft_amd.optim import SGD
    from afft_amd.parallel import Trainer
    c, state, data, tgt, sub = case_tensors(name)
    dev = torch.device("cuda:0")
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    feats = {m: d.to(dev) for m, d in data.items()}
    tgt, sub = tgt.to(dev), sub.to(dev)

    def fresh():
        D_.manual_seed(5)
        model = build(c, "bf16")
        model.load_state_dict(state)
        return model.cuda().train()

    # (a) Trainer, lr driven by the same schedule by hand
    model = fresh()
    tr = Trainer(model, wts, lr=1e-2, momentum=0.9, weight_decay=1e-4, bucket_elems=1 << 15)
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    sch = Warmup(dummy, CosineLR(dummy, num_epochs=2, iters_per_epoch=2, world_size=1, eta_min=1e-6), init_lr_ratio=0.1,
                 num_epochs=1, iters_per_epoch=2, world_size=1)
    for _ in range(4):
        tr.opt.lr = dummy.param_groups[0]["lr"]
        tr.step(feats, {"action": tgt}, {"action": sub})
        dummy.step()
        sch.step()
    torch.cuda.synchronize()
    want = (tr.flat.flat_p.clone(), tr.opt.buf.clone(), tr.flat.flat_p16.clone())
    assert tr._fused and len(tr._fused) >= 8
    # (b) the reference's loop with the drop-in optimizer
    model = fresh()
    opt = SGD(prepare_params(model, None, 1e-2, 1e-4), lr=1e-2, momentum=0.9, nesterov=True, bucket_elems=1 << 15)
    sched = Warmup(opt, CosineLR(opt, num_epochs=2, iters_per_epoch=2, world_size=1, eta_min=1e-6), init_lr_ratio=0.1,
                   num_epochs=1, iters_per_epoch=2, world_size=1)
    _reference_loop(model, opt, sched, feats, tgt, sub, 4)
    torch.cuda.synchronize()
    assert opt._fused and len(opt._fused) == len(tr._fused)
    assert opt.in_backward and len(opt.param_groups) == len(list(model.parameters()))
    for a, b, what in zip((opt.flat.flat_p, opt.opt.buf, opt.flat.flat_p16), want, ("parameters", "momentum", "bf16 images")):
        assert torch.equal(a, b), what
    # the momentum buffers are torch-shaped state
    p0 = next(iter(model.parameters()))
    assert opt.state[p0]["momentum_buffer"].data_ptr() == opt.opt.buf.data_ptr()


def test_dropin_sgd_matches_torch_sgd_on_the_gpu_and_with_mixup():
    """afft_amd.optim.SGD vs torch.optim.SGD on the same groups (both through the gradient sink), MixUp on as in expts/01,
    dropout off (so the two runs see the same network): parameters agree to the bf16 path's tolerance after 3 steps; a
    grad_clip run (in_backward off) clips on the device and matches clip_grad_norm_ + torch.optim.SGD."""
    from afft_amd import dropout as D_
    from afft_amd.common.mixup import MixUp
    from afft_amd.common.scheduler import prepare_params
    from afft_amd.optim import SGD
    c, state, data, tgt, sub = case_tensors("t0_sa")
    dev = torch.device("cuda:0")
    feats = {m: d.to(dev) for m, d in data.items()}
    tgt, sub = tgt.to(dev), sub.to(dev)
    sub = sub.clamp(min=0)          # no ignored frames: every sample takes part in MixUp

    class FixedLam(MixUp):          # MixUp with the Beta draw pinned, so both runs mix alike
        def __init__(self):
            super().__init__(alpha=0.1, label_smoothing={"action": 0.4}, num_classes={"action": c["num_classes"]})
            self.mixup_beta_sampler = type("S", (), {"sample": staticmethod(lambda: torch.tensor(0.7))})()

    def run(kind, clip=None):
        D_.manual_seed(5)
        model = build(c, "bf16")
        model.load_state_dict(state)
        model = model.cuda().eval()
        groups = prepare_params(model, None, 1e-2, 1e-4)
        if kind == "afft":
            opt = SGD(groups, lr=1e-2, momentum=0.9, nesterov=True, bucket_elems=1 << 15, grad_clip=clip)
            assert opt.in_backward == (clip is None)
            _reference_loop(model, opt, None, feats, tgt, sub, 3, mixup_fn=FixedLam())
        else:
            opt = torch.optim.SGD(groups, lr=1e-2, momentum=0.9, nesterov=True)
            from afft_amd.common.runner import Runner
            runner = Runner(model, dev, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, compute_metrics=False)
            batch = ({"data_dict": feats, "target": {"action": tgt}, "target_subclips": {"action": sub}}, {})
            for _ in range(3):
                loss, _ = runner(batch, FixedLam(), True)
                opt.zero_grad()
                loss.backward()
                if clip is not None:
                    torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], clip)
                opt.step()
        torch.cuda.synchronize()
        return torch.cat([p.detach().reshape(-1) for p in model.parameters()])

    for clip in (None, 0.05):
        a, b = run("afft", clip), run("torch", clip)
        assert rel_l2(a, b) < 2e-6, (clip, rel_l2(a, b))


def test_packed_weight_images_stay_coherent_and_feed_the_forward():
    """Fragment-packed weight images (FlatParams.flat_pk16): at the bench's cfg2 widths with 64 clips the fuser's projection / fc2
    forward GEMMs run on the B-direct kernel from them.  After fused-epilogue steps AND after separate-update steps every packed
    image equals afft_pack_weight of its fp32 master; the logits with the B-direct forward agree with the ping-pong forward to the
    bf16 path's rounding (same products, another summation order inside a tile)."""
    import bench as B
    from afft_amd import _lib, dropout as D_, ops, runtime as rt
    from afft_amd.parallel import Trainer
    dev = torch.device("cuda:0")
    D_.manual_seed(7)
    model, c = B.build_model("cfg2", dev)
    feats, tgt, sub = B.make_inputs(c, 64, c["T"], 0, dev)
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    tr = Trainer(model, wts)
    assert tr.flat.flat_pk16 is not None and len(tr.flat.packed) >= 24
    assert not any(rt.packed_live(p) for _, p, _ in tr.flat.packed), "images come to life on demand (the first forward GEMM that wants one)"
    model.train()

    def coherent():
        torch.cuda.synchronize()
        live = [(o, p, pk) for o, p, pk in tr.flat.packed if rt.packed_live(p)]
        assert len(live) >= 10      # the fuser's 5 projection + 5 fc2 weights (one-round grids at 5120 rows; the last block's projection and MLP run on the 1024 token-0 rows)
        for o, p, pk in live:
            want = torch.empty_like(pk)
            ops.pack_weight(p.detach(), want)
            assert torch.equal(pk, want), o
        return live
    for _ in range(3):
        tr.step(feats, tgt, sub)          # step 1 separate (learns the fused set), then fused epilogues
    live = coherent()
    assert len(live) < len(tr.flat.packed) // 2, "only the weights the dispatcher runs on the B-direct kernel pay for an image"
    ids = {id(p) for _, p, _ in live}
    for p in tr.flat.params:              # the epilogue writes the image of exactly those
        d = tr._fused_desc(p) if id(p) in tr._fused else None
        if d is not None:
            assert bool(d.p_pk16) == (id(p) in ids)
    rt.set_fused_sgd(False)
    try:
        tr2_steps = 2
        tr._fused = None
        tr.opt.runs = None
        for _ in range(tr2_steps):
            tr.step(feats, tgt, sub)      # per-bucket update kernels + re-pack
        coherent()
    finally:
        rt.set_fused_sgd(True)
    # forward: B-direct (default dispatch) against ping-pong everywhere
    model.eval()
    with torch.no_grad():
        with B.GemmTimer() as gt:
            o1, _ = model(feats, mixup_fn=None, target=tgt, target_subclips=sub, target_subclips_ignore_index=None)
        assert sum(1 for r in gt.records if r.variant == 10) >= 10, "the B-direct kernel was not dispatched"
        lib = _lib.lib()
        saved = [rt.weight_packed]
        rt.weight_packed = lambda p, rows=None: None          # no packed copies handed to the GEMMs: the ping-pong forward
        try:
            o2, _ = model(feats, mixup_fn=None, target=tgt, target_subclips=sub, target_subclips_ignore_index=None)
        finally:
            rt.weight_packed = saved[0]
    a, b = o1["logits/action"]["all-fused"].float(), o2["logits/action"]["all-fused"].float()
    assert rel_l2(a, b) < 2e-3, rel_l2(a, b)
    del lib


def test_weight_images_follow_a_state_dict_load():
    """after training with live fragment-packed (and, in 'fp16x2', FP16) images, model.load_state_dict() -- an in-place
    write into the flat views that no optimizer kernel sees -- must not leave any image behind: the next forward equals the forward
    of a FRESH model built from the same state, bitwise, in the bf16 mode (B-direct forward GEMMs on packed images) and in fp16x2."""
    import afft_amd
    import bench as B
    from afft_amd import dropout as D_, runtime as rt
    from afft_amd.parallel import Trainer
    dev = torch.device("cuda:0")
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    try:
        for precision in ("bf16", "fp16x2"):
            afft_amd.set_precision(precision)
            D_.manual_seed(7)
            model, c = B.build_model("cfg2", dev)
            feats, tgt, sub = B.make_inputs(c, 64, c["T"], 0, dev)
            # the state that is loaded later: every GEMM weight 5 % larger than what the model trains from (an image left behind
            # shows as a percent-level difference of the logits, far above the comparison's tolerance)
            state0 = {k: (v.detach() * 1.05 if v.dim() == 2 else v.detach().clone()) for k, v in model.state_dict().items()}
            tr = Trainer(model, wts)
            model.train()
            for _ in range(3):
                tr.step(feats, tgt, sub)
            torch.cuda.synchronize()
            if precision == "bf16":
                assert sum(rt.packed_live(p) for _, p, _ in tr.flat.packed) >= 10
            else:
                assert tr.flat.flat_h16 is not None
            model.load_state_dict(state0)          # weights move under the images
            model.eval()
            with torch.no_grad():
                o1, _ = model(feats, mixup_fn=None, target=tgt, target_subclips=sub, target_subclips_ignore_index=None)
            a = o1["logits/action"]["all-fused"].float().clone()
            del tr, model, o1
            torch.cuda.empty_cache()
            fresh, _ = B.build_model("cfg2", dev)
            fresh.load_state_dict(state0)
            fresh.eval()
            with torch.no_grad():
                o2, _ = fresh(feats, mixup_fn=None, target=tgt, target_subclips=sub, target_subclips_ignore_index=None)
            b = o2["logits/action"]["all-fused"].float()
            # the fresh model has no packed images (ping-pong forward GEMMs): same products, another summation order inside a tile
            tol = 2e-3 if precision == "bf16" else 1e-6
            assert rel_l2(a, b) < tol, (precision, rel_l2(a, b))
            del fresh, o2
            torch.cuda.empty_cache()
    finally:
        afft_amd.set_precision("bf16")


@pytest.mark.parametrize("precision", ["bf16", "fp16x2"])
@pytest.mark.parametrize("dim,heads,S,nseq", [(256, 4, 5, 128), (2048, 4, 5, 1024)])
def test_last_block_projection_on_token_rows_equals_all_rows(precision, dim, heads, S, nseq):
    """AttnSublayer(take = S) -- the SA-Fuser's last block (models/fusion.py:362-365 keeps token 0 of every frame): attention over all
    rows, the output projection / residual / everything behind them in backward on the token-0 rows only -- against the full-row
    sub-layer followed by the row selection: the rows that leave agree to GEMM-tile rounding, and so does every gradient (input,
    LayerNorm, qkv and projection weights and biases; the dropped rows contribute exact zeros in the full-row run).  cfg2's own
    geometry (1024 frames x 5 tokens x 2048) and a small one; a row count whose quotient is not a multiple of 64 takes the old path."""
    import afft_amd
    from afft_amd import functional as F_, runtime as rt
    from afft_amd.models.transformerblock import Block
    afft_amd.set_precision(precision)
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    blk = Block(dim, heads, mlp_ratio=2.0, qkv_bias=True).to(dev).eval()
    x = (torch.randn(nseq * S, dim, generator=torch.Generator().manual_seed(4)) * 0.5).to(dev)
    assert F_.attn_take_ok(x, S, heads) and not F_.attn_take_ok(x[:S * 65], S, heads)
    gy = torch.randn(nseq, dim, generator=torch.Generator().manual_seed(5)).to(dev)
    a = blk.attn
    res = {}
    for take in (S, 0):
        for p in blk.parameters():
            p.grad = None
        rt.SINK.begin_step()
        xi = x.clone().requires_grad_(True)
        y, probs = F_.AttnSublayer.apply(xi, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias,
                                         S, heads, "none", blk.norm1.eps, False, True, a.scale, None, None, take)
        if not take:
            y = F_.TakeRows.apply(y, S)
        assert y.shape == (nseq, dim)
        (y * gy).sum().backward()
        rt.SINK.finish_step(list(blk.parameters()))
        torch.cuda.synchronize()
        res[take] = (y.detach().clone(), probs.clone(), xi.grad.clone(),
                     {k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None})
    afft_amd.set_precision("bf16")
    (y1, p1, dx1, g1), (y0, p0, dx0, g0) = res[S], res[0]
    assert rel_l2(p1, p0) < 1e-5      # bit-equal unless the two runs differ in where the fp8 lo pass is eligible (fp16x2)
    assert rel_l2(y1, y0) < 1e-5, rel_l2(y1, y0)
    assert rel_l2(dx1, dx0) < 5e-3, rel_l2(dx1, dx0)
    assert set(g1) == set(g0) and {"attn.proj.weight", "attn.proj.bias", "attn.qkv.weight", "norm1.weight"} <= set(g1)
    for k in g0:
        assert rel_l2(g1[k], g0[k]) < 5e-3, (k, rel_l2(g1[k], g0[k]))


def test_capture_stream_never_comes_back_as_the_auxiliary_stream():
    """torch hands out 32 pooled streams per device round-robin.  With the pool positioned so that the NEXT draw is the auxiliary
    stream's own HIP stream (what a long session does by itself), Trainer.capture() must still capture on a different one
    (runtime.new_stream): a capture whose origin stream was also its auxiliary stream made hip::Stream::EndCapture recurse until the
    stack ran out (round 5) -- without the guard this test takes the process down."""
    import afft_amd
    from afft_amd import dropout as D_, runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.parallel import Trainer
    afft_amd.set_precision("bf16")
    rt.set_grad_mode("sink")
    dev = torch.device("cuda:0")
    aux = rt.aux_stream(dev)
    others = [rt.new_stream(dev) for _ in range(70)]
    assert all(s.cuda_stream not in (aux.cuda_stream, torch.cuda.current_stream().cuda_stream) for s in others)
    mods = {"rgb": 256, "objects": 96, "audio": 256, "flow": 256}
    B, T = 16, 16
    g = torch.Generator().manual_seed(13)
    feats = {m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(dev) for m, C in mods.items()}
    tgt = {"action": torch.randint(0, 97, (B,), generator=g).to(dev)}
    sub = {"action": torch.randint(0, 97, (B, T, 1), generator=g).to(dev)}
    torch.manual_seed(5)
    model = BaseModel(make_model_cfg(mods, 256, 512, depth=2, fp_layers=2, fp_heads=4, drop=0.0), {"action": 97}, {}).to(dev).eval()
    tr = Trainer(model, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, lr=0.01, bucket_elems=1 << 18)
    assert tr.reducer.side_stream.cuda_stream != aux.cuda_stream
    for _ in range(40):      # walk the pool until its next stream is the auxiliary one
        if torch.cuda.Stream().cuda_stream == aux.cuda_stream:
            break
    for _ in range(31):
        torch.cuda.Stream()
    try:
        tr.capture(feats, tgt, sub, warmup=2)
        for _ in range(2):
            loss, _ = tr.step(feats, tgt, sub)
        torch.cuda.synchronize()
        assert float(loss) == float(loss)
    finally:
        D_.disable_device_salt()


@pytest.mark.parametrize("precision", ["bf16", "fp16x2"])
def test_a_non_finite_loss_leaves_parameters_momentum_and_images_untouched(precision):
    """The device-side form of the reference's 'The loss is NaN!' check (common/runner.py:209 raises before backward): the first backward
    kernel writes isfinite(loss) into FusedSGD.ok and every update of the step -- the weight-gradient EPILOGUES of the fused optimizer and
    the per-bucket kernels -- skips on 0.  After a poisoned batch parameters, momentum, bf16 / fp16 / e4m3 / packed images are bit-identical
    to before it; the next clean step trains on."""
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from afft_amd.parallel import Trainer
    afft_amd.set_precision(precision)
    rt.set_grad_mode("sink")
    dev = torch.device("cuda:0")
    mods = {"rgb": 256, "objects": 96, "audio": 256, "flow": 256}
    B, T = 16, 16
    g = torch.Generator().manual_seed(13)
    feats = {m: torch.randn(B, T, C, 1, 1, 1, generator=g).to(dev) for m, C in mods.items()}
    bad = {m: f.clone() for m, f in feats.items()}
    bad["rgb"][3, 5, 7] = float("nan")
    tgt = {"action": torch.randint(0, 97, (B,), generator=g).to(dev)}
    sub = {"action": torch.randint(0, 97, (B, T, 1), generator=g).to(dev)}
    torch.manual_seed(5)
    model = BaseModel(make_model_cfg(mods, 256, 512, depth=2, fp_layers=2, fp_heads=4, drop=0.0), {"action": 97}, {}).to(dev).train()
    tr = Trainer(model, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, lr=0.01, bucket_elems=1 << 18)
    try:
        for _ in range(3):
            tr.step(feats, tgt, sub)
        assert tr._fused, "the fused optimizer epilogues are on from step 2"
        torch.cuda.synchronize()
        snap = lambda: [t.clone() for t in (tr.flat.flat_p, tr.opt.buf, tr.flat.flat_p16, tr.flat.flat_h16, tr.flat.flat_p8, tr.flat.flat_pk16)
                        if t is not None]
        before = snap()
        loss, _ = tr.step(bad, tgt, sub)
        torch.cuda.synchronize()
        assert float(loss) != float(loss) and float(tr.opt.ok) == 0.0
        for a, b in zip(before, snap()):
            assert torch.equal(a, b)
        loss, _ = tr.step(feats, tgt, sub)
        torch.cuda.synchronize()
        assert float(loss) == float(loss) and float(tr.opt.ok) == 1.0
        after = snap()
        assert not torch.equal(before[0], after[0]) and bool(torch.isfinite(after[0]).all()) and bool(torch.isfinite(after[1]).all())
    finally:
        afft_amd.set_precision("bf16")


@pytest.mark.parametrize("handover", [False, True])
def test_token_row_projection_replays_its_dropout_masks_in_backward(handover):
    """Training mode, output dropout + DropPath on the token-row form of the attention sub-layer (take = S): the masks are functions of
    (key, compact row, column) forward and backward.  The forward's mask is read off two forwards that differ by +1 in the projection
    bias (y' - y = mask * scale, exactly, since y = x + drop(proj + b)); the projection-bias gradient of the backward pass must then be
    the column sums of gy * mask -- and with the MLP half behind it, the same block gives the same gradients with the gradient
    hand-over across the boundary on and off (the LayerNorm backward replays the mask instead of the cast kernel)."""
    import afft_amd
    from afft_amd import dropout as D_, functional as F_, runtime as rt
    from afft_amd.models.transformerblock import Block
    afft_amd.set_precision("bf16")
    dev = torch.device("cuda:0")
    dim, heads, S, nseq = 256, 4, 5, 128
    torch.manual_seed(3)
    blk = Block(dim, heads, mlp_ratio=2.0, qkv_bias=True, drop=0.3, drop_path=0.2).to(dev).train()
    a = blk.attn
    x = (torch.randn(nseq * S, dim, generator=torch.Generator().manual_seed(4)) * 0.5).to(dev)
    gy = torch.randn(nseq, dim, generator=torch.Generator().manual_seed(5)).to(dev)
    was = rt.handover()
    rt.set_handover(handover)
    try:
        def attn_only(bias):
            D_.manual_seed(11)
            cfg = D_.with_path(a.drop_cfg(), 0.2, 1)
            return F_.AttnSublayer.apply(x, blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.qkv.bias, a.proj.weight, bias,
                                         S, heads, "none", blk.norm1.eps, False, True, a.scale, cfg, None, S)[0]
        with torch.no_grad():
            y0 = attn_only(a.proj.bias)
            y1 = attn_only(a.proj.bias + 1.0)
        mask = (y1 - y0)                                   # 0 where dropped, 1 / (keep * keep_path) where kept
        kept = float((mask != 0).float().mean())
        assert 0.45 < kept < 0.67, kept                      # (1 - 0.3) * (1 - 0.2) = 0.56
        for p in blk.parameters():
            p.grad = None
        rt.SINK.begin_step()
        y = attn_only(a.proj.bias)
        (y * gy).sum().backward()
        rt.SINK.finish_step(list(blk.parameters()))
        torch.cuda.synchronize()
        want = (gy * mask).sum(0)
        assert rel_l2(a.proj.bias.grad, want) < 1e-2, rel_l2(a.proj.bias.grad, want)
        # the whole block (attention take + MLP on the token rows): the same masks with the hand-over on and off
        res = {}
        for ho in (True, False):
            rt.set_handover(ho)
            for p in blk.parameters():
                p.grad = None
            rt.SINK.begin_step()
            D_.manual_seed(21)
            xi = x.clone().requires_grad_(True)
            yb, _ = blk.forward_rows_first_token(xi, S, "none")
            (yb * gy).sum().backward()
            rt.SINK.finish_step(list(blk.parameters()))
            torch.cuda.synchronize()
            res[ho] = (yb.detach().clone(), xi.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None})
        assert torch.equal(res[True][0], res[False][0])
        assert rel_l2(res[True][1], res[False][1]) < 2e-3
        for k in res[False][2]:
            assert rel_l2(res[True][2][k], res[False][2][k]) < 5e-3, k
    finally:
        rt.set_handover(was)


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16x3", 1e-3), ("bf16", 3e-2)])
def test_interface_edges_arbitrary_mask_mem_dim_qkv_bias_on_the_hip_path(precision, tol):
    """Block with an arbitrary additive (N, N) mask (afft_attention_fwd_table: models/transformerblock.py:26-28) and
    DecoderBlock(mem_dim != dim, qkv_bias=True) (:41-50, :66-68) through the C-ABI against the reference's own outputs, attention maps
    and gradients (tests/golden/e0_edges.npz)."""
    import afft_amd
    from afft_amd import runtime as rt
    from helpers import edge_error, edge_fixture, run_edge_modules
    z, meta, states, inputs = edge_fixture()
    afft_amd.set_precision(precision)
    rt.set_grad_mode("sink")
    try:
        got = run_edge_modules(torch.device("cuda:0"), states, inputs, meta)
    finally:
        afft_amd.set_precision("bf16")
    worst = {}
    for k, t in got.items():
        assert t is not None, k
        worst[k] = edge_error(t, torch.from_numpy(z[k]))
    bad = {k: v for k, v in worst.items() if not v < tol}
    assert not bad, bad
