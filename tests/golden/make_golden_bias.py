"""Generate b0_attn_bias.npz by running the REFERENCE itself (build container only; see make_golden.py): its transformerblock.Block and
DecoderBlock with attention masks that broadcast over batch and heads, and with masks that require grad (models/transformerblock.py:26-28,
:66-68 add whatever tensor they are given).  Closed-form weights and inputs (closed_form.py), all drop rates 0, loss = mean(y^2).
Stored per case: the mask, the output, the returned attention (Block), the gradients of x (and mem), attn.qkv.weight and
attn.proj.weight, and the gradient of the mask where it requires grad.

    python tests/golden/make_golden_bias.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                        # tests/helpers.py
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # oracle/

import closed_form as cf  # noqa: E402
import make_golden  # noqa: E402
from bias_cases import B, D, H, N, GRAD_KEYS, make_mask, BLOCK_CASES  # noqa: E402


def fill(mod, tag):
    state = {k: cf.tensor_for(f"b0.{tag}.{k}", tuple(v.shape)) for k, v in mod.state_dict().items()}
    mod.load_state_dict(state)
    return state


def main():
    make_golden.install_stubs()
    from models.transformerblock import Block, DecoderBlock
    out = {}
    blk = Block(D, H).eval()
    st = fill(blk, "block")
    for case in BLOCK_CASES:
        blk.zero_grad(set_to_none=True)
        x = cf.tensor_for("b0.block.x", (B, N, D), "input").requires_grad_(True)
        m, needs_grad = make_mask(case)
        m.requires_grad_(needs_grad)
        y, attn = blk(x, m)
        y.pow(2).mean().backward()
        assert tuple(attn.shape) == (B, H, N, N) and bool(torch.isfinite(attn).all())
        out.update({f"{case}.mask": m, f"{case}.y": y, f"{case}.attn": attn, f"{case}.dx": x.grad})
        params = dict(blk.named_parameters())
        out.update({f"{case}.grad.{k}": params[k].grad for k in GRAD_KEYS})
        if needs_grad:
            out[f"{case}.dmask"] = m.grad
    dec = DecoderBlock(D, num_heads=H).eval()
    st2 = fill(dec, "dec")
    x = cf.tensor_for("b0.dec.x", (B, N, D), "input").requires_grad_(True)
    mem = cf.tensor_for("b0.dec.mem", (B, N, D), "input").requires_grad_(True)
    m, needs_grad = make_mask("dec")
    m.requires_grad_(needs_grad)
    y = dec(x, mem, m)
    y.pow(2).mean().backward()
    out.update({"dec.mask": m, "dec.y": y, "dec.dx": x.grad, "dec.dmem": mem.grad})
    params = dict(dec.named_parameters())
    out.update({f"dec.grad.{k}": params[k].grad for k in GRAD_KEYS})
    if needs_grad:
        out["dec.dmask"] = m.grad
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()) or k.endswith(".mask"), k
    shapes = {"block": {k: list(v.shape) for k, v in st.items()}, "dec": {k: list(v.shape) for k, v in st2.items()}}
    path = os.path.join(HERE, "b0_attn_bias.npz")
    np.savez_compressed(path, **{k: v.detach().float().numpy() for k, v in out.items()}, shapes=np.asarray(json.dumps(shapes)),
                        meta=np.asarray(json.dumps(dict(case="b0_attn_bias", B=B, N=N, d=D, heads=H, torch=torch.__version__,
                                                        reference="zeyun-zhong/AFFT (v1)"))))
    print("[b0_attn_bias]", len(out), "tensors,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
