"""Stub datasets for the EPIC-KITCHENS-100 validation report tests (CPU and GPU): the reference's own fixture (m0_marginalize.npz scores,
m1_unseen_tail.npz numbers, closed_form.unseen_tail_tables) and the late-fusion fixture runs of submission_cases with id tables and
many-shot subsets of their own.  The id tables are written where the caller says (tmp_path), as test_oracle_golden.py does."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPACES = ("verb", "noun", "action")
TWELVE = [f"{s}{m}" for s in "vna" for m in ("top1", "top5", "mt5r", "mt5r_ms")]
EIGHTEEN = TWELVE + [f"{s}mt5r_{g}" for g in ("tail", "unseen") for s in "vna"]      # compute_accuracies_epic's key order


def write_tables(tables, where):
    for name, rows in tables.items():
        with open(os.path.join(str(where), name), "w", encoding="utf-8") as fh:
            fh.write("\n".join(rows) + "\n")


def reference_fixture(where):
    """(dataset stub, [verb, noun, action] fp32 matrices of m0_marginalize.npz, the 18 numbers of m1_unseen_tail.npz as a dict,
    ids, tables): what the reference's compute_accuracies_epic(..., True) was run on"""
    import pandas as pd
    from afft_amd import challenge
    from closed_form import eval_inputs, unseen_tail_tables
    z = np.load(os.path.join(GOLDEN, "m0_marginalize.npz"))
    g = np.load(os.path.join(GOLDEN, "m1_unseen_tail.npz"))
    logits, mv, mn, a_lab, v_lab, n_lab = eval_inputs()
    ids, tables, manyshot = unseen_tail_tables(len(a_lab), logits.shape[1])
    write_tables(tables, where)

    class _DS:
        df = pd.DataFrame(dict(verb_class=v_lab, noun_class=n_lab, action_class=a_lab, narration_id=ids))
        classes_manyshot = manyshot
        version = challenge.EPIC100_VERSION
        rulstm_annotation_dir = str(where)
    want = dict(zip([str(k) for k in g["acc_names"]], [float(v) for v in g["acc_values"]]))
    return _DS, [np.asarray(z[k], np.float32) for k in SPACES], want, ids, tables


def sweep_tables():
    """id tables and many-shot subsets for the 24 segments of submission_cases (each table also holds an id that is in no split)"""
    import submission_cases as S
    ids = np.asarray(S.uids())
    i = np.arange(S.N)
    tables = {"validation_unseen_participants_ids.csv": list(ids[i % 5 == 0]) + ["P35_105_7"],
              "validation_tail_verbs_ids.csv": list(ids[i % 3 != 0]),
              "validation_tail_nouns_ids.csv": list(ids[(i % 4 == 1) | (i > 18)]) + ["P01_101_999"],
              "validation_tail_actions_ids.csv": list(ids[i % 2 == 1])}
    return tables


def sweep_dataset(where, version=None):
    """submission_cases.make_dataset() with many-shot subsets (the classes of every third segment: present by construction) and the
    id tables of sweep_tables() on disk"""
    import submission_cases as S
    ds = S.make_dataset()
    write_tables(sweep_tables(), where)
    ds.classes_manyshot = {key: {f"{key[0]}{int(c)}": int(c) for c in sorted(set(getattr(ds.df, f"{key}_class").values[::3].tolist()))}
                           for key in SPACES}
    ds.rulstm_annotation_dir = str(where)
    if version is not None:
        ds.version = version
    return ds


def no_tie_at_the_label_among_the_best(scores, labels, k=5):
    """True when in no row another score EQUALS the label's score while the label's rank is below k + 1: only there could the tie rule
    of include/afft_hip.h (the lower class first) and numpy's argsort (the higher class first) count a hit differently"""
    scores, labels = np.asarray(scores), np.asarray(labels)
    for r, l in enumerate(labels.tolist()):
        sl = scores[r, l]
        equal = int((scores[r] == sl).sum()) - 1
        if equal and int((scores[r] > sl).sum()) <= k:
            return False
    return True
