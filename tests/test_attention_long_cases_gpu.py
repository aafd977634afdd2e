"""Every case of tests/attention_long_cases.py -- every instantiation of the kernels of attention_long.hip: attention over 129..512
tokens, and the gradient of an additive attention bias at every L from 1 -- ELEMENTWISE against float64 (attention_double.reference()),
with every operand (q, k, v, dout, bias) in a NaN frame of its own and every result (out, dq, dk, dv, probs, dbias) in a sentinel frame.

The test asserts |got - ref| <= c * u * S for every element, S the magnitude sum of the reference and u the unit roundoff of the
narrowest rounding on the path: 2^-24 fp32 kernels, every probs and every dbias (fp32, accumulated in fp32 from storage-exact inputs);
2^-9 bf16 out and gradients.  Masked and -inf entries of probs and dbias must be exactly 0 (S is 0 there).  The relative-L2 bars of
test_attention_long_gpu.py and test_attention_bias_gpu.py are kept as a second assertion.

The backward and the bias gradient run twice: on the kernel's own probs, and on the float64 probabilities rounded to fp32, both held
to the same bars.  A bias gradient that sums over a broadcast dimension runs twice more into a second buffer: equal bits.  The forward
of a bias case of L <= 128 is a short kernel (afft_attention_fwd_bias), here only to supply the probabilities: it keeps its L2 bars.

c: the short kernels' constants (test_attention_short_gpu.py: C; generic_f32, generic_bf16, mfma_fwd / mfma_bwd; dbias takes the fp32 dq
constant in every family) times 4 are the CEILING -- the long sums have up to 512 terms against 128, and worst-case fp32 accumulation
error grows linearly in the term count.  The bars are twice the worst |got - ref| / (u S) measured over the table on an MI355X, rounded
up to a power of two (MEASURED: the worst per family and output kind, gradients over both probs sources), and every bar is asserted to
stay within its ceiling.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from attention_double import (SENTINEL, banned_pairs, flat_framed, flat_untouched, frame_untouched, framed, heads,  # noqa: E402
                              keep_scale, reference, rows, worst_ratio)
from attention_long_cases import CASES, frame_cols, make_bias  # noqa: E402
from helpers import rel_l2  # noqa: E402
from test_attention_short_gpu import C as SHORT_C  # noqa: E402

pytestmark = pytest.mark.gpu

U = {"f32": 2.0 ** -24, "bf16": 2.0 ** -9}
PATHS = {"f32": "generic_f32", "bf16": "generic_bf16", "mfma": "mfma"}

# worst |got - ref| / (u S) over the table, MI355X: path -> kind -> value
MEASURED = {
    "generic_f32": dict(out=7.22, probs=2.76, dq=1.52, dk=1.57, dv=7.02, dbias=13.4),
    "generic_bf16": dict(out=1.9, probs=1.42, dq=0.296, dk=0.376, dv=1.96, dbias=3.49),
    "mfma": dict(out=3.21, probs=1.26, dq=0.395, dk=0.589, dv=3.41, dbias=1.71),
}
# The largest, dbias of generic_f32 (13.4, against 2.5 on the float64 probabilities in the same case), is bf_L160_full_hd1_drop on its
# own probs: at hd = 1 a score is ONE product, so A = |q| |k| reaches 10 and the forward's rounding of p (2.4 u p (1 + 2 A) there, a
# bar of its own) is carried into dbias = p (dP - sum p dP), whose S knows only the rounding of dP.  It stays within the ceiling.
C = {path: {kind: 2.0 ** math.ceil(math.log2(2.0 * w)) for kind, w in kinds.items()} for path, kinds in MEASURED.items()}
# the ceilings: 4 x the short constants (512 terms against 128); a condition on the bars, not a measurement
CEILING = {"generic_f32": {k: 4.0 * v for k, v in SHORT_C["generic_f32"].items()},
           "generic_bf16": {k: 4.0 * v for k, v in SHORT_C["generic_bf16"].items()},
           "mfma": {k: 4.0 * v for k, v in {**SHORT_C["mfma_fwd"], **SHORT_C["mfma_bwd"]}.items()}}
for _path in CEILING:
    CEILING[_path]["dbias"] = 4.0 * SHORT_C["generic_f32"]["dq"]
assert CEILING["mfma"] == dict(out=32.0, probs=8.0, dq=8.0, dk=16.0, dv=32.0, dbias=32.0)
assert all(C[p][k] <= CEILING[p][k] for p in C for k in C[p]), (C, CEILING)
# relative L2, as test_attention_long_gpu.py and test_attention_bias_gpu.py hold them (dbias: the gradients' bar)
L2 = {"f32": dict(out=2e-5, probs=2e-5, grads=3e-5, dbias=3e-5), "bf16": dict(out=1e-2, probs=2e-3, grads=2e-2, dbias=2e-2)}


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def written(*ts):
    """no element is NaN, infinite or still the sentinel"""
    return all(bool(torch.isfinite(t.float()).all()) and not bool((t.float() == SENTINEL).any()) for t in ts)


def run_case(c):
    """runs case c -> (ratios {kind: worst |got - ref| / (u S)}, l2 {kind: relative L2}, facts {name: bool})"""
    from afft_amd import ops
    nseq, L, H, hd = c.nseq, c.L, c.H, c.hd
    d, R = H * hd, nseq * L
    scale = hd ** -0.5
    tdt = torch.float32 if c.storage == "f32" else torch.bfloat16
    ci, co = frame_cols(c, False, d), frame_cols(c, True, d)
    drop = dict(drop_p=c.drop_p, drop_key=c.key)
    ratios, l2, facts = {}, {}, {"frames": True, "written": True}

    # ---- operands: seeded on the CPU, rounded to the storage type; the reference sees the rounded values
    qkv, dout = rnd(R, 3 * d, seed=1), rnd(R, d, seed=2)
    if c.storage == "bf16":
        qkv, dout = qkv.to(tdt).float(), dout.to(tdt).float()
    ins = []
    for t in (qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], dout):      # q, k, v, dout: each in a NaN frame of its own
        _, view, _ = framed(R, d, float("nan"), tdt, ci)
        view.copy_(t.to(tdt))
        ins.append(view)
    q, k, v, do = ins
    b = make_bias(c)
    bias = None
    if b is not None:
        _, bflat = flat_framed(b.size, float("nan"))
        bflat.copy_(torch.from_numpy(b).flatten())
        bias = bflat.view(b.shape)
    q64, k64, v64 = (heads(qkv[:, i * d:(i + 1) * d].double().numpy(), nseq, L, H, hd) for i in range(3))
    ks, _ = keep_scale(nseq, H, L, c.drop_p, c.key)
    banned = banned_pairs(L, c.mask, c.period)
    ref = reference(q64, k64, v64, heads(dout.double().numpy(), nseq, L, H, hd), float(np.float32(scale)), banned, ks,
                    None if b is None else b.astype(np.float64))
    hidden = np.broadcast_to(banned, (nseq, H, L, L))
    if b is not None:
        hidden = hidden | ~np.isfinite(b.reshape((1,) * (4 - b.ndim) + b.shape))

    # ---- forward
    long_ = c.entry == "fwd_bwd" or c.long
    pbuf, pflat = flat_framed(nseq * H * L * L)
    probs = pflat.view(nseq, H, L, L)
    obuf, out, _ = framed(R, d, SENTINEL, tdt, co)
    if c.entry == "fwd_bwd":
        ops.attention_long_fwd(q, k, v, nseq, L, H, hd, scale, c.mask, out, probs, mask_period=c.period, table=bias, **drop)
    else:
        (ops.attention_long_fwd_bias if long_ else ops.attention_fwd_bias)(q, k, v, nseq, L, H, hd, scale, bias, out, probs, **drop)
    torch.cuda.synchronize()
    if long_:
        ratios["out"] = worst_ratio(out.float(), rows(ref["out"][0]), rows(ref["out"][1]), U[c.storage])
        ratios["probs"] = worst_ratio(probs, ref["probs"][0], ref["probs"][1], U["f32"])
    l2["out"] = rel_l2(out.float().cpu(), torch.from_numpy(rows(ref["out"][0])))
    l2["probs"] = rel_l2(probs.cpu(), torch.from_numpy(ref["probs"][0]))
    facts["masked_probs_zero"] = float(probs.cpu()[torch.from_numpy(hidden.copy())].abs().sum()) == 0.0
    facts["frames"] = frame_untouched(obuf, R, d) and flat_untouched(pbuf)
    facts["written"] = written(out, probs)

    # ---- backward and bias gradient: on the kernel's own probs, then on the float64 probabilities rounded to fp32
    rbuf, rflat = flat_framed(nseq * H * L * L)
    rflat.copy_(torch.from_numpy(ref["probs"][0]).float().flatten())
    for tag, pr in (("own", probs), ("ref", rflat.view(nseq, H, L, L))):
        if long_:
            bufs = [framed(R, d, SENTINEL, tdt, co) for _ in range(3)]
            ops.attention_long_bwd(do, q, k, v, pr, nseq, L, H, hd, scale, bufs[0][1], bufs[1][1], bufs[2][1], **drop)
            torch.cuda.synchronize()
            for kind, (buf, g, _) in zip(("dq", "dk", "dv"), bufs):
                ratios[f"{kind}/{tag}"] = worst_ratio(g.float(), rows(ref[kind][0]), rows(ref[kind][1]), U[c.storage])
                facts["frames"] = facts["frames"] and frame_untouched(buf, R, d)
                facts["written"] = facts["written"] and written(g)
            got = torch.cat([x[1].float().cpu() for x in bufs], dim=1)
            l2["grads/" + tag] = rel_l2(got, torch.from_numpy(np.concatenate([rows(ref[kd_][0]) for kd_ in ("dq", "dk", "dv")], axis=1)))
        if c.entry == "bias":
            dbs = []
            for _ in range(2 if c.reduces() else 1):
                dbuf, dflat = flat_framed(b.size)
                ops.attention_bias_bwd(do, v, pr, nseq, L, H, hd, dflat.view(b.shape), **drop)
                torch.cuda.synchronize()
                facts["frames"] = facts["frames"] and flat_untouched(dbuf)
                dbs.append(dflat.cpu())
            ratios["dbias/" + tag] = worst_ratio(dbs[0], ref["dbias"][0], ref["dbias"][1], U["f32"])
            l2["dbias/" + tag] = rel_l2(dbs[0].view(b.shape), torch.from_numpy(ref["dbias"][0]))
            facts["written"] = facts["written"] and written(dbs[0])
            facts["hidden_dbias_zero/" + tag] = float(dbs[0][torch.from_numpy(~np.isfinite(b)).flatten()].abs().sum()) == 0.0
            if c.reduces():
                facts["dbias_same_bits/" + tag] = torch.equal(dbs[0], dbs[1])
    facts["frames"] = facts["frames"] and flat_untouched(pbuf) and flat_untouched(rbuf)
    return ratios, l2, facts


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_attention_long_case(c):
    ratios, l2, facts = run_case(c)
    print(f"attention_long_case {c.name}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + " | L2 "
          + " ".join(f"{k} {v:.2e}" for k, v in l2.items()))
    for kind, r in ratios.items():
        bar = C[PATHS[c.family]][kind.split("/")[0]]
        assert r <= bar, f"{c.name}: {kind} is off by {r:.3g} u S, the bar is {bar}"
    for kind, e in l2.items():
        assert e < L2[c.storage][kind.split("/")[0]], (c.name, kind, e)
    assert all(facts.values()), (c.name, facts)
