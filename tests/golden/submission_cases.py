"""The late-fusion / submission fixture s0_submission.npz: sizes, runs, weights and the stub dataset object, shared by the generator
(make_golden_submission.py, which feeds them to the reference) and by the tests (which feed them to afft_amd.challenge).

N = 24 segments, A = 211 actions over V = 13 verbs x Nn = 17 nouns: V * Nn = 221 >= A with V and Nn coprime, so closed_form.eval_inputs'
maps a -> ((3a + 1) % V, (5a + 2) % Nn) give 211 DISTINCT (verb, noun) pairs and the inverse of verb_noun_to_action is a function.
A >= 100, which the reference's np.argpartition(row, -100) needs."""
import numpy as np

N, A, V, NN = 24, 211, 13, 17
SEEDS = (0, 1)                      # run i has the action logits closed_form.eval_inputs(..., seed=SEEDS[i])
SHORT = 5                           # case c: the second run lacks the last SHORT segments
CASES = {
    "a": dict(runs=(0,), weights=1.0, short=()),                 # one run: its scores come back bit for bit
    "b": dict(runs=(0, 1), weights=[0.7, 1.5], short=()),        # two complete runs: one weighted sum per space on the device
    "c": dict(runs=(0, 1), weights=[0.7, 1.5], short=(1,)),      # the second run five rows short: the per-uid union
}
VERSION, CHALLENGE = 0.2, "action_anticipation"


def run_inputs(i):
    from closed_form import eval_inputs
    return eval_inputs(N=N, A=A, V=V, Nn=NN, seed=SEEDS[i])


def uids():
    return [f"P{1 + i % 7:02d}_{101 + i % 3}_{i}" for i in range(N)]


def discarded_uids():
    """three discarded segments; the middle one repeats a kept uid and must not overwrite it"""
    return ["P40_101_0", uids()[3], "P41_102_7"]


def make_dataset():
    """the attributes of the reference's EPIC-KITCHENS dataset object that challenge.py reads; labels of run 0"""
    import pandas as pd
    import torch
    _, mv, mn, a_lab, v_lab, n_lab = run_inputs(0)
    verb_of, noun_of = mv.argmax(1), mn.argmax(1)
    pairs = {(int(v), int(n)): a for a, (v, n) in enumerate(zip(verb_of, noun_of))}
    assert len(pairs) == A, "the (verb, noun) pairs must be distinct"

    class _DS:
        class_mappings = {("verb", "action"): torch.from_numpy(mv), ("noun", "action"): torch.from_numpy(mn)}
        df = pd.DataFrame(dict(narration_id=uids(), verb_class=v_lab, noun_class=n_lab, action_class=a_lab))
        classes_manyshot = {}
        verb_noun_to_action = pairs
        verb_classes = {f"v{j}": j for j in range(V)}
        noun_classes = {f"n{j}": j for j in range(NN)}
        version = VERSION
        challenge_type = CHALLENGE
        discarded_df = pd.DataFrame(dict(narration_id=discarded_uids()))
    return _DS


def served(runs_scores, accuracies):
    """stand-in for get_epic_marginalize_verb_noun(resdir, dataset): resdir 'run<i>' -> (accuracies, [verb, noun, action] of run i)"""
    def get(resdir, dataset=None):
        return accuracies, [np.array(s) for s in runs_scores[resdir]]
    return get


# Every combined score is below 8.8 in magnitude, where one fp32 ulp is 9.5e-7; a product and a sum round once each and a fused
# multiply-add moves the result by at most one ulp more; 4e-6 is also a quarter of the smallest gap (1.6e-5) between two of the 101
# best action scores of a row, so a value inside the bound cannot change places with its neighbour's.
ATOL = 4e-6


def check_results(res, golden, case, exact_action=False):
    """the structure get_struct_outputs_per_dataset returned against case `case` of s0_submission.npz: every key, the ORDER of the
    (verb, noun) keys of 'action' (the ranking), every value within ATOL (exactly, for the action scores, with exact_action)"""
    g = golden
    assert res["version"] == str(g[f"{case}_version"]) and res["challenge"] == str(g[f"{case}_challenge"])
    assert set(res) == {"version", "challenge", "results"}
    results = res["results"]
    extra = [u for u in discarded_uids() if u not in uids()]
    assert list(results) == uids() + extra                      # dataset.df order, then the discarded rows
    assert sorted(extra) == sorted(str(u) for u in g[f"{case}_discarded"])
    row_of = {str(u): r for r, u in enumerate(g[f"{case}_uids"])}
    assert sorted(row_of) == sorted(uids())
    worst = 0.0
    for u in uids():
        r, got = row_of[u], results[u]
        assert list(got) == ["verb", "noun", "action"]
        assert list(got["action"]) == [f"{v},{n}" for v, n in g[f"{case}_pairs"][r]], u
        for space, want in (("verb", g[f"{case}_verb"][r]), ("noun", g[f"{case}_noun"][r])):
            assert list(got[space]) == [str(j) for j in range(len(want))]
        for space, want in (("verb", g[f"{case}_verb"][r]), ("noun", g[f"{case}_noun"][r]), ("action", g[f"{case}_action"][r])):
            have = list(got[space].values())
            assert all(type(v) is float for v in have), (u, space)
            err = float(np.max(np.abs(np.asarray(have, np.float64) - want)))
            worst = max(worst, err)
            assert err <= ATOL, (case, u, space, err)
            if exact_action and space == "action":
                assert err == 0.0, (case, u, err)
    for u in extra:
        got = results[u]
        assert got["verb"] == {str(j): 0.0 for j in range(V)} and got["noun"] == {str(j): 0.0 for j in range(NN)}
        assert got["action"] == {f"0,{j}": 0.0 for j in range(100)} and list(got["action"]) == [f"0,{j}" for j in range(100)]
    print(f"[s0_submission {case}] largest |value - reference| = {worst:.3g} (bound {ATOL})")
    return worst


def resdirs(case):
    return [f"run{i}" for i in CASES[case]["runs"]]


def cut(case, i, scores):
    """run i's [verb, noun, action] as case `case` sees them"""
    return [s[:N - SHORT] for s in scores] if i in CASES[case]["short"] else list(scores)
