"""CPU: the host logic of the late-fusion weight search of afft_amd.challenge (device_sweep, late_fuse_sweep) on the fixture runs of
tests/golden/submission_cases.py, with the numpy doubles of tests/sweep_double.py in place of ops.fused_label_rank /
ops.rank_counts_sets, against get_epic_marginalize_late_fuse called once per weight combination.  The kernels themselves are tested
on the GPU (tests/test_fuse_sweep_gpu.py)."""
import math

import numpy as np
import pytest
import torch

import submission_cases as S
import sweep_double

# Six combinations of the two runs of case "b" (the fixture's own among them).  tie_free() below asserts what they were picked for.
COMBOS = [[1.0, 0.0], [0.7, 1.5], [0.5, 0.5], [1.0, 2.0], [0.25, 1.0], [1.5, 0.3]]
NINE = [f"{s}{m}" for s in "vna" for m in ("top1", "top5", "mt5r")]


def tie_free(xs, weights, labels):
    """no combined label score ties with, or sits within 4 fp32 ulp of, another score of its row: neither the tie rule nor one rounding
    more or less per run (a fused multiply-add against a product and a sum) can then move a rank"""
    labels = np.asarray(labels)
    rows = np.arange(len(labels))
    for wj in np.asarray(weights, np.float32):
        s = sweep_double.combine(xs, wj)
        sl = s[rows, labels][:, None]
        gap = np.abs(s - sl)
        gap[rows, labels] = np.inf
        if not (gap > 4 * np.spacing(np.maximum(np.abs(s), np.abs(sl)))).all():
            return False
    return True


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

    def _serve(case, order=None):
        order = S.CASES[case]["runs"] if order is None else order
        monkeypatch.setattr(challenge, "get_epic_marginalize_verb_noun",
                            S.served({f"run{i}": S.cut(case, i, runs[i]) for i in order}, acc))
        return ds
    with sweep_double.installed():
        yield _serve


def _labels(ds):
    return [getattr(ds.df, f"{key}_class").values for key in ("verb", "noun", "action")]


def test_exports_and_derived_signatures():
    from afft_amd import _cabi, _lib
    assert "afft_fused_label_rank" in _lib.EXPORTS and "afft_rank_counts_sets" in _lib.EXPORTS
    assert len(_cabi.protos["afft_fused_label_rank"][0]) == 12
    assert len(_cabi.protos["afft_rank_counts_sets"][0]) == 11


def test_sweep_gives_the_numbers_of_late_fuse_per_combination(runs, serve):
    from afft_amd import challenge
    ds = serve("b")
    for space, labels in enumerate(_labels(ds)):
        assert tie_free([runs[0][space], runs[1][space]], COMBOS, labels), space
    got = challenge.late_fuse_sweep(S.resdirs("b"), COMBOS, dataset=ds)
    assert len(got) == len(COMBOS)
    for weight, have in zip(COMBOS, got):
        want = challenge.get_epic_marginalize_late_fuse(S.resdirs("b"), [weight], dataset=ds)[0]
        assert list(have) == list(want)                         # compute_accuracies_epic's keys, in its order
        for key in NINE:
            # the same integer counts, a different order of float64 operations
            assert have[key] == pytest.approx(want[key], rel=1e-12), (weight, key)
        assert all(math.isnan(have[f"{s}mt5r_ms"]) and math.isnan(want[f"{s}mt5r_ms"]) for s in "vna")
    assert len({tuple(res[key] for key in NINE) for res in got}) > 1      # the combinations do not all score alike


def test_best_weights_are_those_of_late_fuse_and_carry_over(serve):
    from afft_amd import challenge
    ds = serve("b")
    old, new = [], []
    challenge.get_epic_marginalize_late_fuse(S.resdirs("b"), COMBOS[:4], mp_best_weights=old, n_best=3, dataset=ds)
    challenge.late_fuse_sweep(S.resdirs("b"), COMBOS[:4], mp_best_weights=new, n_best=3, dataset=ds)
    assert new == old and 1 <= len(new) <= 3                    # (float, list) pairs: == is bit for bit on the metric
    assert all(any(w is c for c in COMBOS) for _, w in new)     # the caller's own weight objects, as the existing function keeps them
    challenge.get_epic_marginalize_late_fuse(S.resdirs("b"), COMBOS[4:], mp_best_weights=old, n_best=3, dataset=ds)
    challenge.late_fuse_sweep(S.resdirs("b"), COMBOS[4:], mp_best_weights=new, n_best=3, dataset=ds)
    assert new == old and [m for m, _ in new] == sorted(m for m, _ in new)
    # the rule itself, on metrics that are given: ascending, the n_best kept, the list carried from call to call
    metrics = iter([3.0, 1.0, 4.0, 1.5, 5.0, 2.0, 6.0, 7.0])
    real = challenge.device_sweep

    def sweep(xs, labels, weights, **kw):
        top1, top5, mt5r = real(xs, labels, weights, **kw)
        if np.asarray(xs[0]).shape[1] == S.A:                   # the action space decides
            mt5r = np.asarray([next(metrics) for _ in mt5r])
        return top1, top5, mt5r
    challenge.device_sweep = sweep
    try:
        best = []
        res = challenge.late_fuse_sweep(S.resdirs("b"), COMBOS, mp_best_weights=best, n_best=3, dataset=ds)
        assert best == [(3.0, COMBOS[0]), (4.0, COMBOS[2]), (5.0, COMBOS[4])] and res[-1]["amt5r"] == 2.0
        challenge.late_fuse_sweep(S.resdirs("b"), COMBOS[:2], mp_best_weights=best, n_best=3, dataset=ds)
        assert [m for m, _ in best] == [5.0, 6.0, 7.0]
    finally:
        challenge.device_sweep = real


def test_weight_forms_accepted_and_refused(serve):
    from afft_amd import challenge
    ds = serve("b")
    dirs = S.resdirs("b")
    fuse = lambda w, **kw: challenge.late_fuse_sweep(dirs, w, dataset=ds, **kw)      # noqa: E731
    a_float = fuse(2.0)
    a_list = fuse([2.0, 2.0])
    a_lists = fuse([[1.0, 0.0], (2.0, 2.0)])
    a_array = fuse(np.asarray([[2.0, 2.0]]))
    assert len(a_float) == len(a_list) == len(a_array) == 1 and len(a_lists) == 2
    for other in (a_list[0], a_lists[1], a_array[0]):
        assert [other[k] for k in NINE] == [a_float[0][k] for k in NINE]
    for bad in ([1.0], [1.0, 2.0, 3.0], [[1.0, 2.0], [1.0]], np.ones((2, 3))):
        with pytest.raises(AssertionError):
            fuse(bad)
    # a single directory that is not a list
    ds = serve("a")
    one = challenge.late_fuse_sweep("run0", 1.0, dataset=ds)
    want = challenge.get_epic_marginalize_late_fuse("run0", 1.0, dataset=ds)[0]
    assert [one[0][k] for k in NINE] == pytest.approx([want[k] for k in NINE], rel=1e-12)


def test_short_runs_and_more_than_eight_runs_are_refused(serve):
    from afft_amd import challenge
    ds = serve("c")
    with pytest.raises(ValueError, match="complete runs.*get_epic_marginalize_late_fuse"):
        challenge.late_fuse_sweep(S.resdirs("c"), S.CASES["c"]["weights"], dataset=ds)
    ds = serve("a")
    with pytest.raises(ValueError, match="at most 8 runs.*get_epic_marginalize_late_fuse"):
        challenge.late_fuse_sweep(["run0"] * 9, 1.0, dataset=ds)
    assert len(challenge.late_fuse_sweep(["run0"] * 8, 1.0, dataset=ds)) == 1


def test_sets_per_call_does_not_change_the_result(runs, serve):
    from afft_amd import challenge, ops
    ds = serve("b")
    xs, labels = [runs[0][2], runs[1][2]], _labels(ds)[2]
    calls = []
    real = ops.fused_label_rank
    ops.fused_label_rank = lambda xs, w, lab, rank=None: (calls.append(w.shape[0]), real(xs, w, lab, rank=rank))[1]
    try:
        out = {n: challenge.device_sweep(xs, labels, COMBOS, sets_per_call=n) for n in (1, 4, 512)}
    finally:
        ops.fused_label_rank = real
    assert calls == [1] * 6 + [4, 2] + [6]
    for n in (4, 512):
        for a, b in zip(out[1], out[n]):
            assert a.dtype == np.float64 and a.shape == (len(COMBOS),) and np.array_equal(a, b)


def test_labels_outside_the_classes_leave_the_recall_and_stay_in_the_denominators(serve):
    from afft_amd import challenge
    serve("a")
    # class 2 is best in rows 0-2, class 0 in rows 3-5; rows 1 and 4 have no label
    x = np.asarray([[0.1, 0.2, 0.9, 0.0]] * 3 + [[0.9, 0.2, 0.1, 0.0]] * 3, np.float32)
    labels = np.asarray([2, -1, 1, 0, -1, 2])
    top1, top2, rec = challenge.device_sweep([x, x], labels, [[1.0, 1.0], [-1.0, 0.0]], k=2)
    # set 0: top-1 hits in rows 0 and 3, top-2 adds row 2 (class 1 is second): 2 and 3 of SIX rows
    assert top1[0] == 2 / 6 * 100 and top2[0] == 3 / 6 * 100
    # classes 0, 1, 2 have rows (1, 1, 2 of them); class 2: row 0 hits, row 5 (third of four) does not
    assert rec[0] == pytest.approx((1 / 1 + 1 / 1 + 1 / 2) / 3 * 100, rel=1e-15)
    # set 1 turns the order round: class 3 (score 0) is best everywhere and is nobody's label; only row 5's label comes second
    assert top1[1] == 0.0 and top2[1] == 1 / 6 * 100
    assert rec[1] == pytest.approx((0 / 1 + 0 / 1 + 1 / 2) / 3 * 100, rel=1e-15)
    # a subset of the classes restricts the recall mean, as device_accuracy does
    sub = challenge.device_sweep([x, x], labels, [[1.0, 1.0]], k=2, classes={"a": 0, "c": 2, "z": 99})[2]
    assert sub[0] == pytest.approx((1 / 1 + 1 / 2) / 2 * 100, rel=1e-15)
    # device tensors are taken as they are
    again = challenge.device_sweep([torch.from_numpy(x), torch.from_numpy(x)], torch.from_numpy(labels), np.asarray([[1.0, 1.0]]), k=2)
    assert again[0][0] == top1[0] and again[2][0] == rec[0]
