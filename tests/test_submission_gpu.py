"""GPU: the submission path of afft_amd.challenge through the real kernels -- row softmax and the two mapping GEMMs per run
(marginalize_verb_noun), ops.weighted_sum_fwd for the combination of complete runs, ops.topk_rows for the 100 best actions -- against
tests/golden/s0_submission.npz, which the reference's own get_struct_outputs_per_dataset produced on tie-free rows; and
evaluate.top_predictions on the small t0_sa model."""
import os

import numpy as np
import pytest
import torch

import submission_cases as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "s0_submission.npz")))


@pytest.fixture(scope="module")
def runs():
    """run i -> (accuracies, [verb, noun, action]) from challenge.marginalize_verb_noun on the device; computed once"""
    from afft_amd import challenge
    ds = S.make_dataset()
    out = {}
    for i in range(len(S.SEEDS)):
        acc, scores = challenge.marginalize_verb_noun(torch.from_numpy(S.run_inputs(i)[0]).to(DEV), ds)
        for s in scores:
            s.setflags(write=False)
        out[i] = (acc, scores)
    return out


@pytest.mark.parametrize("case", sorted(S.CASES))
def test_struct_outputs_match_reference_golden(case, golden, runs, monkeypatch):
    from afft_amd import challenge, ops
    ds = S.make_dataset()
    monkeypatch.setattr(challenge, "get_epic_marginalize_verb_noun",
                        S.served({f"run{i}": S.cut(case, i, runs[i][1]) for i in S.CASES[case]["runs"]}, runs[0][0]))
    calls = {"weighted_sum_fwd": 0, "topk_rows": 0}

    def counted(name):
        real = getattr(ops, name)

        def f(*a, **kw):
            calls[name] += 1
            return real(*a, **kw)
        return f
    for name in calls:
        monkeypatch.setattr(ops, name, counted(name))
    res = challenge.get_struct_outputs_per_dataset(S.resdirs(case), S.CASES[case]["weights"], dataset=ds)
    S.check_results(res, golden, case, exact_action=case == "a")
    # complete runs are combined on the device, one launch per space; the run that is five rows short forces the per-uid union
    assert calls["weighted_sum_fwd"] == (0 if case == "c" else 3), calls
    assert calls["topk_rows"] == 1, calls
    if case == "a":                                              # one run, weight 1.0: its scores come back bit for bit
        for r, u in enumerate(S.uids()):
            assert list(res["results"][u]["verb"].values()) == runs[0][1][0][r].tolist()
            assert list(res["results"][u]["noun"].values()) == runs[0][1][1][r].tolist()


def test_top_actions_and_struct_outputs_take_device_tensors(golden, runs):
    from afft_amd import challenge
    ds = S.make_dataset()
    scores = [torch.from_numpy(np.array(s)).to(DEV) for s in runs[0][1]]
    vals, idx = challenge.top_actions(scores[2], k=1000)         # clamped to the 211 classes
    assert vals.shape == idx.shape == (S.N, S.A) and idx.dtype == np.int32
    assert np.array_equal(np.sort(idx, axis=1), np.tile(np.arange(S.A), (S.N, 1))) and (np.diff(vals, axis=1) <= 0).all()
    results = challenge.struct_outputs_from_scores(scores, ds)
    S.check_results(dict(version=str(S.VERSION), challenge=S.CHALLENGE,
                         results=dict(results, **{u: {"verb": {str(j): 0.0 for j in range(S.V)}, "noun": {str(j): 0.0 for j in range(S.NN)},
                                                      "action": {f"0,{j}": 0.0 for j in range(100)}}
                                                  for u in S.discarded_uids() if u not in results})), golden, "a", exact_action=True)


def test_top_predictions_on_the_small_model():
    from helpers import case_tensors
    from test_model_gpu import build
    from afft_amd import evaluate as E
    c, state, data, _, _ = case_tensors("t0_sa")
    model = build(c, "fp32")
    model.load_state_dict(state)
    model = model.cuda().eval()
    dev = torch.device(DEV)
    loader = [({"data_dict": {m: d[i:i + 2] for m, d in data.items()}}, {}) for i in range(0, c["B"], 2)]
    key, logits = E.collect_logits(model, loader, dev)
    key2, vals, idx = E.top_predictions(model, loader, dev, k=5)
    K = c["num_classes"]
    k = min(5, K)
    assert key2 == key and vals.is_cuda and idx.is_cuda and vals.shape == idx.shape == (c["B"], k)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int32
    assert torch.equal(idx[:, 0].long(), logits.argmax(dim=1))
    assert torch.equal(vals.view(torch.int32), torch.gather(logits, 1, idx.long()).view(torch.int32))
    assert (vals[:, :-1] >= vals[:, 1:]).all()
    assert E.top_predictions(model, loader, dev, k=10 * K)[2].shape == (c["B"], K)          # k is clamped to the classes
