"""CPU: the host logic of the submission path of afft_amd.challenge (late fusion, the submission structure, test.json / submit.zip)
against tests/golden/s0_submission.npz, which the reference's own get_struct_outputs_per_dataset produced on tie-free rows, with the
numpy doubles of tests/topk_double.py in place of ops.topk_rows / ops.weighted_sum_fwd.  The kernels themselves are tested on the GPU
(tests/test_topk_rows_gpu.py, tests/test_submission_gpu.py)."""
import json
import os
import zipfile

import numpy as np
import pandas as pd
import pytest
import torch

import submission_cases as S
import topk_double

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "s0_submission.npz")))


@pytest.fixture(scope="module")
def runs():
    """run i -> [verb, noun, action]: fp32 softmax of the closed-form logits times the one-hot maps, in numpy; computed once"""
    out = {}
    for i in range(len(S.SEEDS)):
        logits, mv, mn = S.run_inputs(i)[:3]
        e = np.exp(logits - logits.max(axis=1, keepdims=True))
        p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        out[i] = [p @ mv, p @ mn, logits]
        for s in out[i]:
            s.setflags(write=False)
    return out


@pytest.fixture()
def serve(runs, monkeypatch):
    """get_epic_marginalize_verb_noun served from memory for one case; the doubles installed"""
    from afft_amd import challenge
    ds = S.make_dataset()
    acc = challenge.compute_accuracies_epic(runs[0], ds)

    def _serve(case):
        monkeypatch.setattr(challenge, "get_epic_marginalize_verb_noun",
                            S.served({f"run{i}": S.cut(case, i, runs[i]) for i in S.CASES[case]["runs"]}, acc))
        return ds
    with topk_double.installed():
        yield _serve


def test_export_and_derived_signature():
    from afft_amd import _cabi, _lib
    assert "afft_topk_rows" in _lib.EXPORTS
    args, res = _cabi.protos["afft_topk_rows"]
    assert len(args) == 10 and _cabi.consts["AFFT_TOPK_MAX_C"] == 8192 == _lib.TOPK_MAX_C


@pytest.mark.parametrize("case", sorted(S.CASES))
def test_struct_outputs_match_reference_golden(case, golden, runs, serve):
    from afft_amd import challenge
    ds = serve(case)
    res = challenge.get_struct_outputs_per_dataset(S.resdirs(case), S.CASES[case]["weights"], dataset=ds)
    S.check_results(res, golden, case, exact_action=case == "a")
    kept = res["results"][S.discarded_uids()[1]]                # the discarded row that repeats a kept uid is not overwritten
    assert any(v != 0.0 for v in kept["action"].values()) and len(kept["verb"]) == S.V
    if case == "a":                                             # one run, weight 1.0: what was served comes back bit for bit
        for r, u in enumerate(S.uids()):
            assert list(res["results"][u]["verb"].values()) == runs[0][0][r].tolist()
            assert list(res["results"][u]["noun"].values()) == runs[0][1][r].tolist()
    json.dumps(res)                                             # Python numbers only: no encoder needed


def test_dataset_falls_back_to_the_module_attribute(golden, serve, monkeypatch):
    from afft_amd import challenge
    ds = serve("a")
    with pytest.raises(ValueError, match="dataset"):
        challenge.get_struct_outputs_per_dataset(S.resdirs("a"), 1.0)
    monkeypatch.setattr(challenge, "dataset", ds)
    S.check_results(challenge.get_struct_outputs_per_dataset(S.resdirs("a"), 1.0), golden, "a", exact_action=True)


def test_device_combine_is_taken_for_complete_runs_only(serve, monkeypatch):
    from afft_amd import challenge, ops
    calls = []
    real = ops.weighted_sum_fwd
    monkeypatch.setattr(ops, "weighted_sum_fwd", lambda xs, w, out: (calls.append((len(xs), tuple(w.shape))), real(xs, w, out))[1])
    for case, want in (("b", [(2, (S.N, 2))] * 3), ("c", [])):
        del calls[:]
        ds = serve(case)
        _, combined, back = challenge.get_epic_marginalize_late_fuse(S.resdirs(case), S.CASES[case]["weights"], dataset=ds)
        assert calls == want and back is ds
        assert [len(c) for c in combined] == [S.N] * 3 and list(combined[2]) == S.uids()
        assert all(isinstance(row, np.ndarray) and row.shape == (S.A,) for row in combined[2].values())
    # more than 8 complete runs: the per-uid sum again
    del calls[:]
    ds = serve("a")
    challenge.get_epic_marginalize_late_fuse(["run0"] * 9, 1.0, dataset=ds)
    assert calls == []


def test_weight_forms_accepted_and_refused(serve):
    from afft_amd import challenge
    ds = serve("b")
    dirs = S.resdirs("b")
    fuse = lambda w, **kw: challenge.get_epic_marginalize_late_fuse(dirs, w, dataset=ds, **kw)      # noqa: E731
    a_float = fuse(2.0)[1]
    a_list = fuse([2.0, 2.0])[1]
    a_lists = fuse([[1.0, 0.0], (2.0, 2.0)])[1]                 # a sweep returns the LAST combination
    a_array = fuse(np.asarray([[2.0, 2.0]]))[1]
    for u in S.uids():
        for other in (a_list, a_lists, a_array):
            assert np.array_equal(a_float[2][u], other[2][u])
    for bad in ([1.0], [1.0, 2.0, 3.0], [[1.0, 2.0], [1.0]], np.ones((2, 3))):
        with pytest.raises(AssertionError):
            fuse(bad)
    # a single directory that is not a list
    ds = serve("a")
    assert len(challenge.get_epic_marginalize_late_fuse("run0", 1.0, dataset=ds)[1][0]) == S.N


def test_best_weights_bookkeeping_keeps_the_n_best(serve, monkeypatch):
    from afft_amd import challenge
    ds = serve("b")
    metrics = iter([3.0, 1.0, 4.0, 1.5, 5.0, 2.0])
    plain = challenge.compute_accuracies_epic
    monkeypatch.setattr(challenge, "compute_accuracies_epic", lambda probs, d: dict(plain(probs, d), amt5r=next(metrics)))
    sweep = [[float(i), 1.0] for i in range(6)]
    best = []
    acc, _, _ = challenge.get_epic_marginalize_late_fuse(S.resdirs("b"), sweep, mp_best_weights=best, n_best=3, dataset=ds)
    # 3.0 enters; 1.0 is below the worst kept and does not; 4.0 enters; 1.5 is below 3.0; 5.0 enters (three kept); 2.0 is below 3.0
    assert best == [(3.0, sweep[0]), (4.0, sweep[2]), (5.0, sweep[4])]
    assert acc["amt5r"] == 2.0                                  # the accuracies returned are the last combination's
    metrics = iter([6.0, 7.0])
    challenge.get_epic_marginalize_late_fuse(S.resdirs("b"), sweep[:2], mp_best_weights=best, n_best=3, dataset=ds)
    assert [m for m, _ in best] == [5.0, 6.0, 7.0]              # the list is carried from call to call, the worst drops out


def test_normalize_and_concat_helpers():
    from afft_amd import challenge
    ds = S.make_dataset()
    m = np.arange(12, dtype=np.float32).reshape(4, 3) + 1
    d = challenge._concat_with_uids([m, m[:, :2], m[:2]], ds, "narration_id")
    assert [len(x) for x in d] == [4, 4, 2] and list(d[0]) == S.uids()[:4] and np.array_equal(d[2][S.uids()[1]], m[1])
    n1, n2 = challenge._normalize_scores(d[:1], 1)[0], challenge._normalize_scores(d[:1], 2)[0]
    for r, u in enumerate(S.uids()[:4]):
        assert np.allclose(n1[u], m[r] / (np.abs(m[r]).sum() + 0.000001), rtol=1e-6)
        assert np.allclose(n2[u], m[r] / (np.sqrt((m[r] ** 2).sum()) + 0.000001), rtol=1e-6)


def test_package_writes_test_json_and_submit_zip(golden, serve, tmp_path):
    from afft_amd import challenge
    ds = serve("b")
    out = tmp_path / "sub"
    res = challenge.package_results_for_submission_ek100(S.resdirs("b"), S.CASES["b"]["weights"], dataset=ds, output_dir=str(out))
    assert (res["sls_pt"], res["sls_tl"], res["sls_td"]) == (1, 4, 3)
    with open(out / "test.json") as fh:
        text = fh.read()
    back = json.loads(text)
    assert back == res and text.startswith('{\n    "version": "0.2"')         # indent=4
    assert [list(back["results"][u]["action"]) for u in S.uids()] == [list(res["results"][u]["action"]) for u in S.uids()]
    S.check_results({k: back[k] for k in ("version", "challenge", "results")}, golden, "b")
    with zipfile.ZipFile(out / "submit.zip") as z:
        assert z.namelist() == ["test.json"] and z.read("test.json").decode() == text
    res2 = challenge.package_results_for_submission_ek100(S.resdirs("b"), S.CASES["b"]["weights"], sls=(2, 3, 5), dataset=ds,
                                                          output_dir=str(out))
    assert (res2["sls_pt"], res2["sls_tl"], res2["sls_td"]) == (2, 3, 5)
    with zipfile.ZipFile(out / "submit.zip") as z:
        assert z.namelist() == ["test.json"]                    # written anew, not appended to


def test_generate_test_json_and_parse_args(serve, tmp_path, monkeypatch):
    from afft_amd import challenge
    ds = serve("b")
    monkeypatch.setattr(challenge, "LOGITS_DIR", str(tmp_path))
    seen = []
    plain = challenge.get_epic_marginalize_verb_noun
    monkeypatch.setattr(challenge, "get_epic_marginalize_verb_noun", lambda d, dataset: (seen.append(d), plain(os.path.basename(d)))[1])
    args = challenge.parse_args(["--models", "run0", "run1", "--weights", "0.7", "1.5"])
    assert args.prefix_h5 == "test" and args.models == ["run0", "run1"]
    challenge.generate_test_json(args, dataset=ds)
    assert seen == [os.path.join(str(tmp_path), "run0"), os.path.join(str(tmp_path), "run1")]
    assert sorted(os.listdir(tmp_path)) == ["submit.zip", "test.json"]


def test_top_actions_clamps_k_and_struct_outputs_take_fewer_than_100_classes(serve):
    from afft_amd import challenge
    serve("a")
    x = np.asarray([[1.0, 3.0, 2.0, 3.0, -1.0], [0.0, -0.0, 5.0, np.nan, 5.0]], np.float32)
    vals, idx = challenge.top_actions(x, k=100)
    assert vals.shape == idx.shape == (2, 5) and vals.dtype == np.float32 and idx.dtype == np.int32
    assert idx.tolist() == [[1, 3, 2, 0, 4], [2, 4, 0, 1, 3]]   # equal scores: the lower class first; NaN last
    assert vals[0].tolist() == [3.0, 3.0, 2.0, 1.0, -1.0] and np.isnan(vals[1, 4]) and np.signbit(vals[1, 3]) and not np.signbit(vals[1, 2])
    assert challenge.top_actions(x, k=2)[1].tolist() == [[1, 3], [2, 4]]
    assert challenge.top_actions(torch.from_numpy(x).reshape(2, 1, 5), k=1)[1].tolist() == [[1], [2]]

    class _DS:
        verb_noun_to_action = {(a % 2, a // 2): a for a in range(5)}
        df = pd.DataFrame(dict(narration_id=["s0", "s1"]))
    res = challenge.struct_outputs_from_scores([x[:, :2], x[:, :3], x[:1].repeat(2, 0)], _DS)
    assert list(res) == ["s0", "s1"] and list(res["s0"]["action"]) == ["1,0", "1,1", "0,1", "0,0", "0,2"]
    assert res["s0"]["verb"] == {"0": 1.0, "1": 3.0} and list(res["s1"]["noun"]) == ["0", "1", "2"]
