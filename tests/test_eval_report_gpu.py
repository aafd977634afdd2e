"""GPU: afft_rank_counts_groups (include/afft_hip.h) against the integer restatement of tests/report_double.py, and the
EPIC-KITCHENS-100 validation report through it (afft_amd.challenge.device_accuracies_epic, marginalize_verb_noun(device_metrics=True),
afft_amd.evaluate.evaluate, late_fuse_sweep(compute_manyshot_unseen_tail=True)) against the reference's own 18 numbers
(tests/golden/m1_unseen_tail.npz) and the host compute_accuracies_epic."""
import math

import numpy as np
import pytest
import torch

import report_cases as RC
import report_double
import submission_cases as S
from test_fuse_sweep_cpu import COMBOS, NINE, tie_free

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = (1, 255, 256, 257, 700)                                  # 257: one live row in the second workgroup
CS = (1, 5, 97)
NSETS = (1, 3, 9)
NGROUPS = (1, 3, 8)
PATTERNS = ("all", "absent", "last", "random")


def _cases():
    """5 x 3 x 3 cases: every (rows, C, nsets); ngroups and the choice of k run through their three values along each of the three axes,
    so that every pair of values of two parameters occurs.  Each case runs all four membership patterns."""
    out = []
    for ri, rows in enumerate(ROWS):
        for ci, C in enumerate(CS):
            for si, nsets in enumerate(NSETS):
                k = (1, min(5, C), C)[(ri + 2 * ci + si) % 3]
                out.append((rows, C, nsets, NGROUPS[(ri + ci + si) % 3], k))
    return out


def _member(pattern, rows, G, gen):
    """uint32 [rows] membership words"""
    full = (1 << G) - 1
    if pattern == "all":
        return np.full(rows, full, np.uint32)
    words = torch.randint(0, 2 ** 32, (rows,), generator=gen).numpy().astype(np.uint32)      # bits at or above G included
    if pattern == "random":
        words[0] |= np.uint32(0x80000000)
        return words
    last = np.uint32(1 << (G - 1))
    words &= ~last                                              # "absent": no row of group G - 1
    if pattern == "last":                                       # group G - 1 lives in the last (partial) workgroup only
        words[(rows - 1) // 256 * 256:] |= last
    return words


def _buffers(nsets, G, C):
    return [torch.zeros(s, dtype=torch.int32, device=DEV) for s in ((nsets, G, 2), (nsets, G, C), (G, C), (G,))]


@pytest.mark.parametrize("rows,C,nsets,G,k", _cases())
def test_kernel_equals_the_integer_restatement(rows, C, nsets, G, k):
    from afft_amd import ops
    gen = torch.Generator().manual_seed(100000 * rows + 1000 * C + 10 * nsets + G)
    host_rank = torch.randint(0, C + 1, (nsets, rows), generator=gen, dtype=torch.int32)
    buf = torch.zeros(nsets, rows + 3, dtype=torch.int32)       # ldr > rows; the padding (rank 0) would count as a hit if it were read
    buf[:, :rows] = host_rank
    rank = buf.to(DEV)[:, :rows]
    labels = torch.randint(-1, C + 2, (rows,), generator=gen)
    if rows >= 3:
        labels[0], labels[1], labels[2] = -1, C, C - 1
    lab_dev = labels.to(DEV)
    for pattern in PATTERNS:
        words = _member(pattern, rows, G, gen)
        member = torch.from_numpy(words.view(np.int32)).to(DEV)
        want = report_double.counts(host_rank.numpy(), labels.numpy(), words, G, C, k)
        got = _buffers(nsets, G, C)
        ops.rank_counts_groups(rank, lab_dev, C, k, member, G, *got)
        for name, g, w in zip(("hits", "tps", "nums", "group_rows"), got, want):
            assert np.array_equal(g.cpu().numpy().astype(np.int64), w), (pattern, name)
        ops.rank_counts_groups(rank, lab_dev, C, k, member, G, *got)      # the counters are ADDED to
        for name, g, w in zip(("hits", "tps", "nums", "group_rows"), got, want):
            assert np.array_equal(g.cpu().numpy().astype(np.int64), 2 * w), (pattern, name, "second call")
        if pattern in ("absent", "last"):
            assert int(want[3][G - 1]) == (0 if pattern == "absent" else rows - (rows - 1) // 256 * 256)
    if G == 1:                                                  # member = None: afft_rank_counts_sets, integer for integer
        got = _buffers(nsets, 1, C)
        ops.rank_counts_groups(rank, lab_dev, C, k, None, 1, *got)
        sets = [torch.zeros(s, dtype=torch.int32, device=DEV) for s in ((nsets, 2), (nsets, C), (C,))]
        ops.rank_counts_sets(rank, lab_dev, C, k, *sets)
        assert torch.equal(got[0].reshape(nsets, 2), sets[0]) and torch.equal(got[1].reshape(nsets, C), sets[1])
        assert torch.equal(got[2].reshape(C), sets[2]) and int(got[3][0]) == rows


def test_argument_errors_raise_before_any_launch():
    from afft_amd import ops
    rows, C, nsets = 6, 10, 2
    rank = torch.zeros(nsets, rows, dtype=torch.int32, device=DEV)
    labels = torch.zeros(rows, dtype=torch.int64, device=DEV)
    member = torch.ones(rows, dtype=torch.int32, device=DEV)
    bufs = [torch.zeros(n, dtype=torch.int32, device=DEV) for n in (nsets * 9 * 2, nsets * 9 * C, 9 * C, 9)]
    for G in (0, 9):
        with pytest.raises(RuntimeError, match="1 <= ngroups <= 8"):
            ops.rank_counts_groups(rank, labels, C, 5, member, G, *bufs)
    three = _buffers(nsets, 3, C)
    with pytest.raises(RuntimeError, match="k <= C"):
        ops.rank_counts_groups(rank, labels, C, C + 1, member, 3, *three)
    with pytest.raises(RuntimeError, match="null member"):
        ops.rank_counts_groups(rank, labels, C, 5, None, 3, *three)
    short = torch.as_strided(rank, (nsets, rows), (rows - 1, 1))
    with pytest.raises(RuntimeError, match="ldr"):
        ops.rank_counts_groups(short, labels, C, 5, member, 3, *three)
    torch.cuda.synchronize()
    assert not any(bool(b.any()) for b in bufs + three)


# ---------------------------------------------------------------- the report on the reference's fixture

def _assert_reference_numbers(got, want):
    assert list(got) == RC.EIGHTEEN and set(want) == set(got) and len(want) == 18
    for key, v in want.items():
        print(f"{key}: device {got[key]!r} reference {v!r}")
        assert abs(got[key] - v) < 1e-9, (key, got[key], v)


def test_report_reproduces_the_references_eighteen_numbers(tmp_path):
    """the m0 matrices on the device, the m1 stub dataset: all 18 numbers to 1e-9.  No row of the fixture has a tie at the label's
    score among the best five (asserted), so every row is compared with the reference and none with the double alone."""
    from afft_amd import challenge
    ds, scores, want, _, _ = RC.reference_fixture(tmp_path)
    for key, x in zip(RC.SPACES, scores):
        assert RC.no_tie_at_the_label_among_the_best(x, getattr(ds.df, f"{key}_class").values), key
    got = challenge.device_accuracies_epic([torch.from_numpy(x).to(DEV) for x in scores], ds, compute_manyshot_unseen_tail=True)
    _assert_reference_numbers(got, want)
    plain = challenge.device_accuracies_epic(scores, ds)        # host arrays go to the device; one group, many-shot NaN
    assert list(plain) == RC.TWELVE and [plain[k] for k in NINE] == [got[k] for k in NINE]
    assert all(math.isnan(plain[f"{s}mt5r_ms"]) for s in "vna")


def test_marginalize_and_evaluate_give_the_same_report(tmp_path, capsys):
    from afft_amd import challenge, evaluate
    from closed_form import eval_inputs
    ds, _, want, _, _ = RC.reference_fixture(tmp_path)
    logits, mv, mn = eval_inputs()[:3]
    ds.class_mappings = {("verb", "action"): torch.from_numpy(mv), ("noun", "action"): torch.from_numpy(mn)}
    x = torch.from_numpy(logits).to(DEV)
    got, scores = challenge.marginalize_verb_noun(x, ds, compute_manyshot_unseen_tail=True, device_metrics=True)
    _assert_reference_numbers(got, want)
    host, host_scores = challenge.marginalize_verb_noun(x, ds, compute_manyshot_unseen_tail=True)
    assert all(np.array_equal(a, b) for a, b in zip(scores, host_scores))      # the returned scores do not depend on the switch
    assert list(host) == list(got) and all(abs(host[k] - got[k]) < 1e-9 for k in got)

    class _Model:
        def eval(self):
            return self

        def __call__(self, feats, **kw):
            return {evaluate.LOGITS_KEY: {"rgb": feats["rgb"][:, None, :]}}, None
    loader = [({"data_dict": {"rgb": torch.from_numpy(logits[at:at + 20])}}, None) for at in range(0, len(logits), 20)]
    capsys.readouterr()
    report = evaluate.evaluate(_Model(), ds, loader, DEV)
    assert report == got
    printed = capsys.readouterr().out
    assert "Mean top 5 tail" in printed and "Mean top 5 unseen" in printed and "many shot" in printed


# ---------------------------------------------------------------- the sweep with the report

def test_sweep_report_equals_the_host_report_of_the_materialised_combination(tmp_path, monkeypatch):
    from afft_amd import challenge, ops
    ds = RC.sweep_dataset(tmp_path)
    runs = {i: challenge.marginalize_verb_noun(torch.from_numpy(S.run_inputs(i)[0]).to(DEV), ds)[1] for i in range(len(S.SEEDS))}
    monkeypatch.setattr(challenge, "get_epic_marginalize_verb_noun", S.served({f"run{i}": list(runs[i]) for i in S.CASES["b"]["runs"]}, {}))
    monkeypatch.setattr(challenge, "print_accuracies_epic", lambda *a, **kw: None)
    combos = COMBOS[:4]
    for space, key in enumerate(RC.SPACES):
        assert tie_free([runs[0][space], runs[1][space]], combos, getattr(ds.df, f"{key}_class").values), key
    calls = []
    with monkeypatch.context() as m:
        for name in ("fused_label_rank", "rank_counts_sets", "rank_counts_groups", "weighted_sum_fwd"):
            m.setattr(ops, name, (lambda real, name: lambda *a, **kw: (calls.append(name), real(*a, **kw))[1])(getattr(ops, name), name))
        got = challenge.late_fuse_sweep(S.resdirs("b"), combos, dataset=ds, compute_manyshot_unseen_tail=True)
        assert calls == ["fused_label_rank", "rank_counts_groups"] * 3
        del calls[:]
        off = challenge.late_fuse_sweep(S.resdirs("b"), combos, dataset=ds, compute_manyshot_unseen_tail=False)
        assert calls == ["fused_label_rank", "rank_counts_sets"] * 3
    N = S.N
    for weight, have in zip(combos, got):
        combo = []
        for space in range(3):
            xs = [torch.from_numpy(np.ascontiguousarray(runs[i][space])).to(DEV) for i in (0, 1)]
            out = torch.empty_like(xs[0])
            ops.weighted_sum_fwd(xs, torch.tensor([weight], dtype=torch.float32, device=DEV).expand(N, 2), out)
            combo.append(out.cpu().numpy())
        want = challenge.compute_accuracies_epic(combo, ds, True)
        assert list(have) == list(want) == RC.EIGHTEEN
        for key, v in want.items():
            print(f"{weight} {key}: sweep {have[key]!r} host {v!r}")
            assert not math.isnan(v) and abs(have[key] - v) < 1e-9, (weight, key, have[key], v)
    # the option off: today's result exactly -- the default call, and the numbers of the ungrouped device_sweep
    default = challenge.late_fuse_sweep(S.resdirs("b"), combos, dataset=ds)
    assert len(default) == len(off) == len(combos)
    for a, b in zip(off, default):
        assert list(a) == list(b) and all(a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])) for k in a)
    for space, (short, key) in enumerate((("v", "verb"), ("n", "noun"), ("a", "action"))):
        top1, top5, mt5r = challenge.device_sweep([runs[0][space], runs[1][space]], getattr(ds.df, f"{key}_class").values, combos)
        for j, d in enumerate(off):
            assert list(d) == RC.TWELVE and math.isnan(d[f"{short}mt5r_ms"])
            assert (d[f"{short}top1"], d[f"{short}top5"], d[f"{short}mt5r"]) == (float(top1[j]), float(top5[j]), float(mt5r[j]))
            assert [got[j][k] for k in NINE] == [d[k] for k in NINE]
