"""CPU: the EPIC-KITCHENS-100 validation report from integer counters per row group (afft_amd.challenge.row_groups,
device_accuracies_epic, the grouped device_sweep / late_fuse_sweep) with the numpy doubles of tests/report_double.py in place of the
kernels, against the reference's own 18 numbers (tests/golden/m1_unseen_tail.npz) and against the host compute_accuracies_epic.  The
kernel itself, afft_rank_counts_groups, is tested on the GPU (tests/test_eval_report_gpu.py)."""
import ctypes
import functools
import math
import re

import numpy as np
import pytest
import torch

import report_cases as RC
import report_double
import submission_cases as S
import sweep_double
from test_cabi_cpu import _gcc, built_lib  # noqa: F401  (the fixture the C-ABI tests use)
from test_fuse_sweep_cpu import COMBOS, NINE, tie_free


def _close(got, want, tol=1e-9):
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) < tol


# ---------------------------------------------------------------- row groups

def test_row_groups_are_the_hand_built_masks(tmp_path):
    from afft_amd import challenge
    ds, _, _, ids, tables = RC.reference_fixture(tmp_path)
    got = challenge.row_groups(ds)
    assert list(got) == ["verb", "noun", "action"]
    i = np.arange(len(ids))
    unseen = i % 5 == 0
    tail = {"verb": i % 3 != 0, "noun": (i % 4 == 1) | (i > 40), "action": i % 2 == 1}
    for key in RC.SPACES:
        assert got[key].dtype == np.uint32 and got[key].shape == (len(ids),)
        assert np.array_equal(got[key] & 1, np.ones(len(ids), np.uint32))
        assert np.array_equal((got[key] >> 1) & 1, unseen.astype(np.uint32)), key
        assert np.array_equal((got[key] >> 2) & 1, tail[key].astype(np.uint32)), key
        assert not (got[key] >> 3).any()
    # the ids of the tables that are in no split select nothing, and the masks are the ones epic100_unseen_tail_eval matches
    assert int(((got["verb"] >> 1) & 1).sum()) == len(tables["validation_unseen_participants_ids.csv"]) - 1
    assert 0 < int(((got["noun"] >> 2) & 1).sum()) == len(tables["validation_tail_nouns_ids.csv"]) - 1


def test_epic55_counts_one_group_and_reads_no_table(tmp_path, monkeypatch):
    from afft_amd import challenge, ops
    ds, scores, _, _, _ = RC.reference_fixture(tmp_path)
    ds.version = 0.1
    ds.rulstm_annotation_dir = str(tmp_path / "not_there")
    monkeypatch.setattr(challenge, "_read_id_column", lambda path: pytest.fail(f"read {path}"))
    seen = []
    with report_double.installed(), monkeypatch.context() as m:      # m is undone first: the doubles never outlive the block
        real = ops.rank_counts_groups
        m.setattr(ops, "rank_counts_groups", lambda rank, lab, C, k, member, ngroups, *bufs:
                  (seen.append((member, ngroups, tuple(rank.shape))), real(rank, lab, C, k, member, ngroups, *bufs))[1])
        got = challenge.device_accuracies_epic(scores, ds, compute_manyshot_unseen_tail=True)
        off = challenge.device_accuracies_epic(scores, ds)
    assert seen == [(None, 1, (1, 48))] * 6
    want = challenge.compute_accuracies_epic(scores, ds, True)
    assert list(got) == list(want) == RC.TWELVE                 # many-shot, no unseen / tail keys (challenge.py:190)
    assert all(_close(got[k], want[k]) for k in want) and not any(math.isnan(got[f"{s}mt5r_ms"]) for s in "vna")
    assert list(off) == RC.TWELVE and all(math.isnan(off[f"{s}mt5r_ms"]) for s in "vna")
    assert [off[k] for k in NINE] == [got[k] for k in NINE]


# ---------------------------------------------------------------- the double against the reference's numbers

def _double_report(scores, ds, groups, report, grouped):
    per_space = {}
    for key, x in zip(RC.SPACES, scores):
        labels = getattr(ds.df, f"{key}_class").values
        rank = report_double.label_ranks(x, labels)
        G = 3 if grouped else 1
        hits, tps, nums, rows = report_double.counts(rank[None], labels, groups[key] if grouped else None, G, x.shape[1], min(5, x.shape[1]))
        assert rows[0] == len(labels)
        per_space[key] = (len(labels), hits[0], tps[0], nums)
    return report_double.accuracies(per_space, ds.classes_manyshot, report, grouped)


def test_double_gives_the_references_eighteen_numbers(tmp_path):
    """counters from the integer restatement, fed with ranks computed in numpy from the m0 matrices -> all 18 numbers of
    m1_unseen_tail.npz.  The fixture's rows have no tie at the label's score among the best five (asserted), so the tie rule of
    include/afft_hip.h and numpy's argsort count the same hits and every row is compared with the reference."""
    from afft_amd import challenge
    ds, scores, want, _, _ = RC.reference_fixture(tmp_path)
    for key, x in zip(RC.SPACES, scores):
        assert RC.no_tie_at_the_label_among_the_best(x, getattr(ds.df, f"{key}_class").values), key
    got = _double_report(scores, ds, challenge.row_groups(ds), True, True)
    assert list(got) == RC.EIGHTEEN and set(want) == set(got) and len(want) == 18
    for key, v in want.items():
        assert abs(got[key] - v) < 1e-9, (key, got[key], v)
    # without the option: the twelve keys, many-shot NaN, the nine numbers unchanged
    plain = _double_report(scores, ds, None, False, False)
    assert list(plain) == RC.TWELVE and [plain[k] for k in NINE] == [got[k] for k in NINE]
    assert all(math.isnan(plain[f"{s}mt5r_ms"]) for s in "vna")


def test_device_accuracies_epic_on_the_references_fixture_with_the_doubles(tmp_path):
    from afft_amd import challenge
    ds, scores, want, _, _ = RC.reference_fixture(tmp_path)
    with report_double.installed():
        got = challenge.device_accuracies_epic([torch.from_numpy(x) for x in scores], ds, compute_manyshot_unseen_tail=True)
        plain = challenge.device_accuracies_epic(scores, ds)
    host = challenge.compute_accuracies_epic(scores, ds, True)
    assert list(got) == list(host) == RC.EIGHTEEN
    for key, v in want.items():
        assert type(got[key]) is float and abs(got[key] - v) < 1e-9, (key, got[key], v)
    assert got == _double_report(scores, ds, challenge.row_groups(ds), True, True)      # the same integers, the same float64 steps
    assert list(plain) == list(challenge.compute_accuracies_epic(scores, ds)) == RC.TWELVE


def test_labels_outside_the_classes_and_an_empty_group(tmp_path):
    """rows without a label stay in the accuracy denominators and out of every recall; a group without rows has a NaN recall"""
    import pandas as pd
    from afft_amd import challenge
    x = np.asarray([[0.1, 0.2, 0.9, 0.0]] * 3 + [[0.9, 0.2, 0.1, 0.0]] * 3, np.float32)
    labels = np.asarray([2, -1, 1, 0, 7, 2])
    ids = [f"s{i}" for i in range(6)]
    RC.write_tables({"validation_unseen_participants_ids.csv": ["elsewhere"], "validation_tail_verbs_ids.csv": ids[:3],
                     "validation_tail_nouns_ids.csv": ids[3:], "validation_tail_actions_ids.csv": ids[1:2]}, tmp_path)

    class _DS:
        df = pd.DataFrame(dict(verb_class=labels, noun_class=labels, action_class=labels, narration_id=ids))
        classes_manyshot = {"verb": {"a": 0, "c": 2, "z": 99}}
        version = challenge.EPIC100_VERSION
        rulstm_annotation_dir = str(tmp_path)
    with report_double.installed():
        got = challenge.device_accuracies_epic([x, x, x], _DS, True)
    # top-1 hits in rows 0 and 3; top-4 (k = min(5, C)) hits in every row with a label: 2 and 4 of SIX rows
    assert got["vtop1"] == 2 / 6 * 100 and got["vtop5"] == 4 / 6 * 100
    assert got["vmt5r"] == 100.0 and got["vmt5r_ms"] == 100.0 and math.isnan(got["nmt5r_ms"])
    assert all(math.isnan(got[f"{s}mt5r_unseen"]) for s in "vna")                # nobody is an unseen participant
    assert got["vmt5r_tail"] == 100.0 and got["nmt5r_tail"] == 100.0
    assert math.isnan(got["amt5r_tail"])                                          # its only row has no label: no class has a row


# ---------------------------------------------------------------- the C ABI

def test_symbol_is_exported_with_the_compilers_signature(built_lib):  # noqa: F811
    from afft_amd import _cabi
    assert "afft_rank_counts_groups" in built_lib.EXPORTS
    assert hasattr(ctypes.CDLL(built_lib.LIB_PATH), "afft_rank_counts_groups")
    (args,) = re.findall(r"\*/ extern int afft_rank_counts_groups \((.*)\);", _gcc('#include "afft_hip.h"\n'))
    scalars = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32}
    want = [ctypes.c_void_p if "*" in a else scalars[a.strip()] for a in args.split(",")]
    have, res = _cabi.protos["afft_rank_counts_groups"]
    assert len(want) == 14 and have == want and res is ctypes.c_int
    assert [i for i, t in enumerate(want) if t is ctypes.c_void_p] == [0, 3, 4, 9, 10, 11, 12, 13]
    assert built_lib._SIGS["afft_rank_counts_groups"] == (have, res)


# ---------------------------------------------------------------- the sweep with the report

@pytest.fixture(scope="module")
def runs():
    """run i -> [verb, noun, action] in numpy, as tests/test_fuse_sweep_cpu.py builds them"""
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
def recorded(runs, monkeypatch):
    """the doubles installed, the runs of case "b" served from memory, every call of the sweep's ops recorded by name"""
    from afft_amd import challenge, ops
    calls = []
    with report_double.installed(), monkeypatch.context() as m:      # m is undone first: the doubles never outlive the block
        m.setattr(challenge, "get_epic_marginalize_verb_noun", S.served({f"run{i}": list(runs[i]) for i in S.CASES["b"]["runs"]}, {}))
        m.setattr(challenge, "print_accuracies_epic", lambda *a, **kw: None)
        for name in ("fused_label_rank", "rank_counts_sets", "rank_counts_groups", "weighted_sum_fwd", "label_rank", "recall_accumulate"):
            m.setattr(ops, name, (lambda real, name: lambda *a, **kw: (calls.append(name), real(*a, **kw))[1])(getattr(ops, name), name))
        yield calls


def _host_report(runs, weight, ds):
    from afft_amd import challenge
    combo = [sweep_double.combine([runs[0][space], runs[1][space]], np.asarray(weight, np.float32)) for space in range(3)]
    return challenge.compute_accuracies_epic(combo, ds, True)


def test_sweep_call_sequence_with_and_without_the_report(runs, recorded, tmp_path, monkeypatch):
    from afft_amd import challenge
    ds = RC.sweep_dataset(tmp_path)
    dirs = S.resdirs("b")
    off = challenge.late_fuse_sweep(dirs, COMBOS, dataset=ds)
    assert recorded == ["fused_label_rank", "rank_counts_sets"] * 3              # today's sequence: one chunk per space
    del recorded[:]
    on = challenge.late_fuse_sweep(dirs, COMBOS, dataset=ds, compute_manyshot_unseen_tail=True)
    assert recorded == ["fused_label_rank", "rank_counts_groups"] * 3
    del recorded[:]
    monkeypatch.setattr(challenge, "device_sweep", functools.partial(challenge.device_sweep, sets_per_call=4))
    chunked = challenge.late_fuse_sweep(dirs, COMBOS, dataset=ds, compute_manyshot_unseen_tail=True)
    assert recorded == ["fused_label_rank", "rank_counts_groups"] * 6            # 6 sets in chunks of 4: two chunks per space
    assert chunked == on
    assert all(list(d) == RC.TWELVE for d in off) and all(list(d) == RC.EIGHTEEN for d in on)
    for a, b in zip(off, on):
        assert [a[k] for k in NINE] == [b[k] for k in NINE] and all(math.isnan(a[f"{s}mt5r_ms"]) for s in "vna")


def test_sweep_report_equals_the_host_report_of_every_combination(runs, recorded, tmp_path):
    from afft_amd import challenge
    ds = RC.sweep_dataset(tmp_path)
    for space, key in enumerate(RC.SPACES):
        assert tie_free([runs[0][space], runs[1][space]], COMBOS, getattr(ds.df, f"{key}_class").values), key
    best = []
    got = challenge.late_fuse_sweep(S.resdirs("b"), COMBOS, mp_best_weights=best, n_best=3, dataset=ds, compute_manyshot_unseen_tail=True)
    for weight, have in zip(COMBOS, got):
        want = _host_report(runs, weight, ds)
        assert list(have) == list(want) == RC.EIGHTEEN
        for key, v in want.items():
            assert not math.isnan(v) and abs(have[key] - v) < 1e-9, (weight, key, have[key], v)
    assert len({tuple(d.values()) for d in got}) > 1 and [m for m, _ in best] == sorted(m for m, _ in best)
    # EPIC-55: the many-shot numbers only, one group, no table read
    ds55 = RC.sweep_dataset(tmp_path, version=0.1)
    ds55.rulstm_annotation_dir = str(tmp_path / "not_there")
    got55 = challenge.late_fuse_sweep(S.resdirs("b"), COMBOS[:2], dataset=ds55, compute_manyshot_unseen_tail=True)
    for have, full in zip(got55, got):
        assert list(have) == RC.TWELVE and [have[k] for k in RC.TWELVE] == [full[k] for k in RC.TWELVE]


def test_grouped_device_sweep_return_form(runs, recorded):
    """four float64 arrays [nsets, ngroups]; column 0 of a group that holds every row is the ungrouped call's vector, bit for bit"""
    from afft_amd import challenge
    labels = S.make_dataset().df.noun_class.values
    xs = [runs[0][1], runs[1][1]]
    member = np.asarray([1 | (2 if r % 2 else 0) | 0x100 for r in range(S.N)], np.uint32)      # group 2 is empty; bit 8 is ignored
    plain = challenge.device_sweep(xs, labels, COMBOS)
    sub = challenge.device_sweep(xs, labels, COMBOS, classes={"a": 1, "b": 4})
    out = challenge.device_sweep(xs, labels, COMBOS, classes={"a": 1, "b": 4}, member=member, ngroups=3)
    assert len(plain) == 3 and len(out) == 4 and all(a.dtype == np.float64 and a.shape == (len(COMBOS), 3) for a in out)
    for i in range(3):
        assert np.array_equal(out[i][:, 0], plain[i])
    assert np.array_equal(out[3][:, 0], sub[2], equal_nan=True)
    odd = [x[1::2] for x in xs]
    for i, want in enumerate(challenge.device_sweep(odd, labels[1::2], COMBOS)):
        assert np.array_equal(out[i][:, 1], want)
    assert all(np.isnan(a[:, 2]).all() for a in out)
    with pytest.raises(ValueError, match="member"):
        challenge.device_sweep(xs, labels, COMBOS, ngroups=3)
