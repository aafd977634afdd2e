"""Generate tests/golden/s0_submission.npz by running the REFERENCE's late fusion and submission code (build container only).

    python tests/golden/make_golden_submission.py

Imports the reference's challenge.py the way make_golden.run_eval_case does (same stubs), sets its module global `dataset` to the stub
of submission_cases.make_dataset, replaces its get_epic_marginalize_verb_noun by a function that serves in-memory runs (the scores the
reference's own marginalize_verb_noun gives for the closed-form logits) and calls the reference's get_struct_outputs_per_dataset for
the three cases of submission_cases.CASES.  Nothing else of the reference is touched.

TIE CONDITION, asserted below: in every combined action row the first 101 sorted values differ from their neighbours by at least
1e-5, and every verb / noun / action row is NaN-free.  On such rows "the 100 best, best first" has one meaning, so the reference alone
decides every stored index.  Nothing of the reference (source, bytecode, pickles) is written: the .npz holds numeric and string arrays.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

MIN_GAP = 1e-5


def main():
    import make_golden
    make_golden.install_stubs()
    make_golden._mod("h5py")
    make_golden._mod("numpyencoder", NumpyEncoder=object)
    import challenge as RC
    import submission_cases as S

    ds = S.make_dataset()
    RC.dataset = ds
    full, acc0 = {}, None
    for i in range(len(S.SEEDS)):
        acc, scores = RC.marginalize_verb_noun(S.run_inputs(i)[0].copy(), ds, to_prob=True)
        full[i] = [np.asarray(s, np.float32) for s in scores]
        acc0 = acc if acc0 is None else acc0
    inverse = {a: vn for vn, a in ds.verb_noun_to_action.items()}
    out, gaps = {}, {}
    for case, spec in S.CASES.items():
        RC.get_epic_marginalize_verb_noun = S.served({f"run{i}": S.cut(case, i, full[i]) for i in spec["runs"]}, acc0)
        _, combined, _ = RC.get_epic_marginalize_late_fuse(S.resdirs(case), spec["weights"])
        gap = np.inf
        for space in combined:
            for row in space.values():
                assert not np.isnan(row).any(), "NaN in a combined row"
        for row in combined[2].values():
            top = np.sort(np.asarray(row, np.float64))[::-1][:101]
            gap = min(gap, float(np.min(top[:-1] - top[1:])))
        assert gap >= MIN_GAP, f"case {case}: two of the 101 best action scores of a row are {gap} apart"
        gaps[case] = gap
        res = RC.get_struct_outputs_per_dataset(S.resdirs(case), spec["weights"])
        results = res["results"]
        kept = [u for u in results if u in combined[0]]
        added = [u for u in results if u not in combined[0]]
        assert sorted(kept) == sorted(S.uids()) and sorted(added) == sorted(set(S.discarded_uids()) - set(S.uids()))
        pairs = np.zeros((len(kept), 100, 2), np.int64)
        vals = np.zeros((len(kept), 100), np.float64)
        for r, u in enumerate(kept):
            items = list(results[u]["action"].items())
            assert len(items) == 100
            for j, (name, v) in enumerate(items):
                pairs[r, j] = [int(t) for t in name.split(",")]
                vals[r, j] = float(v)
                assert inverse[ds.verb_noun_to_action[tuple(pairs[r, j])]] == tuple(pairs[r, j])
            assert (np.diff(vals[r]) < 0).all()
            assert list(results[u]["verb"]) == [str(j) for j in range(S.V)] and list(results[u]["noun"]) == [str(j) for j in range(S.NN)]
        for u in added:
            assert list(results[u]["action"]) == [f"0,{j}" for j in range(100)] and set(results[u]["action"].values()) == {0.0}
            assert list(results[u]["verb"].values()) == [0.0] * S.V and list(results[u]["noun"].values()) == [0.0] * S.NN
        out.update({f"{case}_uids": np.asarray(kept), f"{case}_pairs": pairs, f"{case}_action": vals,
                    f"{case}_verb": np.asarray([[float(v) for v in results[u]["verb"].values()] for u in kept], np.float64),
                    f"{case}_noun": np.asarray([[float(v) for v in results[u]["noun"].values()] for u in kept], np.float64),
                    f"{case}_discarded": np.asarray(added), f"{case}_version": np.asarray(res["version"]),
                    f"{case}_challenge": np.asarray(res["challenge"])})
    out["meta"] = np.asarray(json.dumps(dict(case="s0_submission", N=S.N, A=S.A, V=S.V, Nn=S.NN, seeds=list(S.SEEDS), short=S.SHORT,
                                             cases={k: dict(v, runs=list(v["runs"]), short=list(v["short"])) for k, v in S.CASES.items()},
                                             smallest_gap=gaps, torch=torch.__version__, numpy=np.__version__,
                                             reference="zeyun-zhong/AFFT (v1)")))
    path = os.path.join(HERE, "s0_submission.npz")
    np.savez_compressed(path, **out)
    print("[s0_submission] smallest gap among the 101 best:", gaps, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
