"""The cases of b0_attn_bias.npz (make_golden_bias.py; tests/test_attention_bias_*.py): the reference's Block / DecoderBlock, dim 64,
4 heads, B = 3 sequences of N = 5 tokens, with attention masks that broadcast over batch and heads.  Masks are closed-form; no mask
hides every key of a row (the precondition of the table tests: a row of -inf has no softmax)."""
import torch

import closed_form as cf

B, N, D, H = 3, 5, 64, 4
NEG = float("-inf")
GRAD_KEYS = ("attn.qkv.weight", "attn.proj.weight")
# case -> (mask shape, requires grad)
BLOCK_CASES = {"pad": ((B, 1, 1, N), False), "head": ((1, H, N, N), False), "sample": ((B, 1, N, N), False),
               "full": ((B, H, N, N), False), "grad2d": ((N, N), True)}
DEC_CASE = ((B, 1, N, N), True)


def make_mask(case: str):
    """(fp32 mask, requires grad?)"""
    if case == "pad":          # key padding: sample 1 has lost its last key, sample 2 its last two
        m = torch.zeros(B, 1, 1, N)
        m[1, 0, 0, N - 1:] = NEG
        m[2, 0, 0, N - 2:] = NEG
        return m, False
    shape, grad = DEC_CASE if case == "dec" else BLOCK_CASES[case]
    m = 0.5 * cf.tensor_for(f"b0.{case}.mask", shape, "input")             # values in [-1, 1)
    if case == "dec":          # causal self-attention and cross-attention, one bias per sample on top
        return m + torch.triu(torch.full((N, N), NEG), diagonal=1), grad
    kill = cf.tensor_for(f"b0.{case}.kill", shape, "input") > 1.2            # ~ 20 % of the entries: -inf
    kill[..., 0] = False                                                      # key 0 stays visible to every query
    return m.masked_fill(kill, NEG), grad
