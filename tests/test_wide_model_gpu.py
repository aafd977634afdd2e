"""GPU: a model whose rows are wider than 2048 columns (common_dim = fp_inter_dim = 2560) trains: outputs, the three losses and
gradients against the CPU oracle on the same random weights, after the pattern of test_model_gpu.py::_compare_with_oracle.  The
LayerNorm backward over 2560 columns runs inside the composite sub-layer calls, on the call-by-call path and standalone (the
fuser's final norm on token 0, GPT-2's ln_f)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_l2  # noqa: E402

# the bars of tests/test_model_gpu.py (TOL, GTOL_BF16): parity (fp32) mode 1e-3 on every output, loss and gradient; the bf16 speed
# mode 2e-2 on outputs and 2.5e-2 on gradients (bf16 operand rounding)
TOL = {"fp32": 1e-3, "bf16": 2e-2}
GTOL_BF16 = 2.5e-2

WIDTH, HEADS, T, CLASSES, B = 2560, 5, 4, 11, 2     # head dimension 512; ~160 M parameters; 24 fuser rows
MODAL_DIMS = {"rgb": WIDTH, "flow": WIDTH}
GKEYS = ["future_predictor.fuser.blocks.0.norm1.weight",                       # LayerNorm weights: inside the sub-layers ..
         "future_predictor.fuser.norm.weight",                                  # .. and standalone, on token 0 of every frame
         "future_predictor.fuser.blocks.0.mlp.mlp.2.weight",
         "future_predictor.future_predictor.gpt_model.h.0.ln_2.weight",
         "future_predictor.future_predictor.gpt_model.ln_f.weight",
         "future_predictor.future_predictor.gpt_model.h.0.mlp.c_fc.weight"]

_ORACLE = {}


def _oracle():
    """weights, inputs and the oracle's outputs, losses and gradients: computed once, shared by the four runs, never modified"""
    if _ORACLE:
        return _ORACLE
    from afft_amd.config import make_model_cfg
    from afft_amd.models.base_model import BaseModel
    from oracle import afft_oracle as O
    torch.manual_seed(1)
    cfg = make_model_cfg(MODAL_DIMS, WIDTH, WIDTH, fuser="sa", depth=1, num_heads=HEADS, fp_layers=1, fp_heads=HEADS, T=T, drop=0.0)
    state = {k: v.detach().clone() for k, v in BaseModel(cfg, {"action": CLASSES}, {}).state_dict().items()}
    for k in GKEYS:
        assert k in state, k
    g = torch.Generator().manual_seed(2)
    data = {m: torch.randn(B, T, C, 1, 1, 1, generator=g) for m, C in MODAL_DIMS.items()}
    tgt = torch.randint(0, CLASSES, (B,), generator=g)
    sub = torch.randint(0, CLASSES, (B, T, 1), generator=g)
    sub[0, :2] = -1
    P = {k: (v.clone().requires_grad_(True) if k in GKEYS else v) for k, v in state.items()}
    ocfg = dict(fuser="sa", depth=1, num_heads=HEADS, fp_layers=1, fp_heads=HEADS, fp_output_len=1, num_classes={"action": CLASSES})
    oout = O.base_model_forward(P, data, ocfg)
    ototal, olosses = O.loss(oout, tgt, sub)
    ototal.backward()
    _ORACLE.update(cfg=cfg, state=state, data=data, tgt=tgt, sub=sub, out=oout, total=float(ototal.detach()),
                   losses={k: float(v.detach()) for k, v in olosses.items()}, grads={k: P[k].grad for k in GKEYS})
    return _ORACLE


@pytest.mark.parametrize("composite", [True, False], ids=["composite", "call_by_call"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_wide_model_matches_oracle(precision, composite):
    import afft_amd
    from afft_amd import runtime as rt
    from afft_amd.common.runner import BasicLossAccuracy, Runner
    from afft_amd.models.base_model import BaseModel
    o = _oracle()
    was = rt.composite()
    afft_amd.set_precision(precision)
    rt.set_grad_mode("sink")
    rt.set_composite(composite)
    try:
        model = BaseModel(o["cfg"], {"action": CLASSES}, {}).eval()
        model.load_state_dict(o["state"], strict=True)
        dev = torch.device("cuda:0")
        model = model.to(dev)
        rt.SINK.begin_step()
        out, out_t = model({m: d.to(dev) for m, d in o["data"].items()}, mixup_fn=None, target={"action": o["tgt"].to(dev)},
                           target_subclips={"action": o["sub"].to(dev)}, target_subclips_ignore_index=None)
        losses, _ = BasicLossAccuracy(False)(out, out_t["target"], out_t["target_subclips"])
        total, _ = Runner._reduce_loss(losses, {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}, sync=False)
        total.backward()
        rt.SINK.finish_step(list(model.parameters()))
        torch.cuda.synchronize()
        tol = TOL[precision]
        worst = 0.0
        for key in ("logits/action", "past_logits/action", "past_futures", "orig_past", "future"):
            e = rel_l2(out[key]["all-fused"].float().cpu(), o["out"][key]["all-fused"])
            worst = max(worst, e)
            assert e < tol, (key, e)
        e = rel_l2(out["attentions"]["all-fused"]["modality_attns"].float().cpu(), o["out"]["attentions"]["all-fused"]["modality_attns"])
        assert e < tol, ("modality_attns", e)
        assert abs(float(total.detach()) - o["total"]) < tol * max(1.0, abs(o["total"]))
        for k, v in o["losses"].items():
            assert abs(float(losses[k].mean()) - v) < tol * max(1.0, abs(v)), k
        params = dict(model.named_parameters())
        gtol = GTOL_BF16 if precision == "bf16" else tol
        gworst = 0.0
        for k in GKEYS:
            e = rel_l2(params[k].grad.cpu(), o["grads"][k])
            gworst = max(gworst, e)
            assert e < gtol, (k, e)
        print(f"[wide {precision} composite={composite}] vs oracle: worst output error {worst:.2e} worst gradient error {gworst:.2e}")
    finally:
        rt.set_composite(was)
        afft_amd.set_precision("bf16")
        model = None
        torch.cuda.empty_cache()
