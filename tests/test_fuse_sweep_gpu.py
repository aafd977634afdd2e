"""GPU: afft_fused_label_rank and afft_rank_counts_sets (include/afft_hip.h) and the weight search of afft_amd.challenge through them.
The fused kernel is held to the composition it replaces, bit for bit -- ops.label_rank of ops.weighted_sum_fwd's output, set by set --
and, on scores whose products and sums are exact, to the numpy restatement of tests/sweep_double.py."""
import numpy as np
import pytest
import torch

import submission_cases as S
import sweep_double
from test_fuse_sweep_cpu import COMBOS, NINE, tie_free

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WT = 8                                                          # FLR_WT of afft_amd/csrc/metrics.hip: weight sets per workgroup
CS = (1, 3, 255, 256, 257, 1024, 1027, 3806)
NSETS = (1, WT - 1, WT, WT + 1, 2 * WT + 3)
NS = (1, 3, 8)
ROWS = (1, 5)
LAYOUTS = ("contiguous", "padded", "offset", "odd")


def _cases():
    """8 x 5 cases that cover every PAIR of values of (C, nsets, n, rows): with t = ci + si, n takes NS[t % 3] and rows ROWS[t % 2], so
    that along every C (si = 0..4) and along every nsets (ci = 0..7) t runs through all residues, and t mod 6 through all (n, rows)"""
    out = []
    for ci, C in enumerate(CS):
        for si, nsets in enumerate(NSETS):
            t = ci + si
            out.append((C, nsets, NS[t % 3], ROWS[t % 2], LAYOUTS[(ci + 2 * si) % 4]))
    return out


def _views(n, rows, C, layout, gen):
    """n fp32 [rows, C] views of random normal scores with one row stride"""
    if layout == "contiguous":                                  # 16-byte loads when C is a multiple of 4
        ld, off = C, 0
    elif layout == "padded":                                    # ldx > C, rows 16-byte aligned: 16-byte loads and a scalar tail
        ld, off = (C + 3) // 4 * 4 + 4, 0
    elif layout == "offset":                                    # x[:, 1:]: the base pointer is 4 bytes off, the scalar path
        ld, off = (C + 1 + 3) // 4 * 4, 1
    else:                                                       # a row stride that is no multiple of 4: the scalar path
        ld, off = (C + 1) | 1, 0
    base = torch.randn(n, rows, ld, generator=gen).to(DEV)
    xs = [base[i][:, off:off + C] for i in range(n)]
    if layout == "offset":
        assert all(x.data_ptr() % 16 == 4 for x in xs)
    return xs


def _composition(xs, w, labels):
    """rank[j] = label_rank(weighted_sum_fwd(xs, w[j] for every row)): what the parent commit runs per weight set"""
    from afft_amd import ops
    rows, C = xs[0].shape
    out = torch.empty(rows, C, device=DEV)
    lab = torch.empty(rows, dtype=torch.int64, device=DEV)
    want = torch.empty(w.shape[0], rows, dtype=torch.int32, device=DEV)
    for j in range(w.shape[0]):
        ops.weighted_sum_fwd(xs, w[j:j + 1].expand(rows, len(xs)), out)
        ops.label_rank(out, C, labels=labels, k=1, rank=want[j], label_out=lab)
    return want


@pytest.mark.parametrize("C,nsets,n,rows,layout", _cases())
def test_equals_label_rank_of_weighted_sum_bit_for_bit(C, nsets, n, rows, layout):
    from afft_amd import ops
    gen = torch.Generator().manual_seed(1000 * C + 10 * nsets + n + rows)
    xs = _views(n, rows, C, layout, gen)
    w = torch.randn(nsets, n, generator=gen).to(DEV)
    if nsets > 1:
        w[nsets - 1] = 0.0                                      # a weight set of zeros: every finite score ties at 0
    edge = [0, C - 1, -1, C, int(torch.randint(0, C, (1,), generator=gen))]
    labels = torch.tensor(edge if rows == 5 else [edge[(C + nsets) % 5]], dtype=torch.int64, device=DEV)
    if rows == 5 and C >= 4:
        l = edge[4]                                             # row 4: NaN at the label, +inf, -inf and one more NaN beside it
        xs[0][4, l] = float("nan")
        xs[n - 1][4, (l + 1) % C] = float("inf")
        xs[0][4, (l + 2) % C] = float("-inf")
        xs[n // 2][4, (l + 3) % C] = float("nan")
        xs[0][0, C - 1] = float("nan")                          # row 0 (label 0): a finite label score among NaN, +inf and -inf
        xs[n - 1][0, 1] = float("inf")
        xs[0][0, 2] = float("-inf")
    buf = torch.full((nsets, rows + 3), -7, dtype=torch.int32, device=DEV)      # ldr > rows: the padding is a canary
    got = ops.fused_label_rank(xs, w, labels, rank=buf[:, :rows])
    want = _composition(xs, w, labels)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    assert bool((buf[:, rows:] == -7).all())
    outside = (labels < 0) | (labels >= C)
    assert bool((got[:, outside] == C).all())
    if nsets > 1 and not (rows == 5 and C >= 4):                # zeros, finite scores: everything ties and the lower classes come first
        inside = ~outside
        assert torch.equal(got[nsets - 1][inside], labels[inside].to(torch.int32))
    assert torch.equal(ops.fused_label_rank(xs, w, labels), want)               # the rank buffer the call makes itself


@pytest.mark.parametrize("C,n,nsets,rows", [(37, 3, 11, 6), (260, 8, 9, 4), (1027, 2, 3, 3)])
def test_exact_arithmetic_and_ties_against_the_restatement(C, n, nsets, rows):
    """scores from {-2 .. 2} / 8 and weights from {-1, 0, 0.5, 1, 2}: every product and every sum is exact, so a fused multiply-add
    and a product plus a sum agree, and the rows are full of equal scores (the lower class wins; -0.0 == +0.0)"""
    from afft_amd import ops
    gen = torch.Generator().manual_seed(C + n)
    xs = [(torch.randint(-2, 3, (rows, C), generator=gen).float() / 8).to(DEV) for _ in range(n)]
    xs[0] = torch.where(xs[0] == 0, -xs[0], xs[0])              # run 0 has its zeros negative
    assert bool(torch.signbit(xs[0]).logical_and(xs[0] == 0).any())
    w = torch.tensor([-1.0, 0.0, 0.5, 1.0, 2.0])[torch.randint(0, 5, (nsets, n), generator=gen)].to(DEV)
    labels = torch.randint(0, C, (rows,), generator=gen)
    labels[0], labels[1] = -1, C
    labels = labels.to(DEV)
    got = ops.fused_label_rank(xs, w, labels).cpu().numpy()
    want = sweep_double.label_ranks([x.cpu().numpy() for x in xs], w.cpu().numpy(), labels.cpu().numpy())
    assert np.array_equal(got, want)
    assert (want[:, 2:] > 0).any() and (want[:, :1] == C).all()


@pytest.mark.parametrize("rows", [1, 255, 257])
@pytest.mark.parametrize("k", [1, 5, 7])
def test_rank_counts_sets_equals_recall_accumulate_per_set(rows, k):
    from afft_amd import ops
    C, nsets = 7, 3
    gen = torch.Generator().manual_seed(rows + k)
    buf = torch.full((nsets, rows + 2), -1, dtype=torch.int32)
    buf[:, :rows] = torch.randint(0, C + 1, (nsets, rows), generator=gen, dtype=torch.int32)
    rank = buf.to(DEV)[:, :rows]                                # ldr > rows; the padding would count as a hit if it were read
    labels = torch.randint(-1, C + 1, (rows,), generator=gen).to(DEV)
    hits = torch.full((nsets, 2), 3, dtype=torch.int32, device=DEV)
    tps = torch.full((nsets, C), 5, dtype=torch.int32, device=DEV)
    nums = torch.full((C,), 11, dtype=torch.int32, device=DEV)
    want_hits, want_tps, want_nums = hits.clone(), tps.clone(), nums.clone()
    spare = torch.zeros(C, dtype=torch.int32, device=DEV)
    for j in range(nsets):
        ops.recall_accumulate(rank[j].contiguous(), labels, k, want_tps[j], want_nums if j == 0 else spare)
        want_hits[j, 0] += int((rank[j] < 1).sum())
        want_hits[j, 1] += int((rank[j] < k).sum())
    ops.rank_counts_sets(rank, labels, C, k, hits, tps, nums)
    assert torch.equal(hits, want_hits) and torch.equal(tps, want_tps)
    assert torch.equal(nums, want_nums)                         # every row once, not once per set
    h, t, n = sweep_double.counts(rank.cpu().numpy(), labels.cpu().numpy(), C, k)
    assert np.array_equal(hits.cpu().numpy() - 3, h) and np.array_equal(tps.cpu().numpy() - 5, t) and np.array_equal(nums.cpu().numpy() - 11, n)


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


def test_late_fuse_sweep_end_to_end_against_late_fuse_per_combination(runs, monkeypatch):
    from afft_amd import challenge, ops
    ds = S.make_dataset()
    monkeypatch.setattr(challenge, "get_epic_marginalize_verb_noun",
                        S.served({f"run{i}": list(runs[i][1]) for i in S.CASES["b"]["runs"]}, runs[0][0]))
    for space, key in enumerate(("verb", "noun", "action")):
        assert tie_free([runs[0][1][space], runs[1][1][space]], COMBOS, getattr(ds.df, f"{key}_class").values), key
    calls = {"weighted_sum_fwd": 0, "topk_rows": 0, "fused_label_rank": 0, "rank_counts_sets": 0}
    with monkeypatch.context() as m:
        for name in calls:
            m.setattr(ops, name, (lambda real, name: lambda *a, **kw: (calls.__setitem__(name, calls[name] + 1), real(*a, **kw))[1])(
                getattr(ops, name), name))
        best = []
        got = challenge.late_fuse_sweep(S.resdirs("b"), COMBOS, mp_best_weights=best, n_best=3, dataset=ds)
    # no combination is formed and nothing is sorted; one launch of each kernel per space
    assert calls == {"weighted_sum_fwd": 0, "topk_rows": 0, "fused_label_rank": 3, "rank_counts_sets": 3}, calls
    old = []
    for weight, have in zip(COMBOS, got):
        want = challenge.get_epic_marginalize_late_fuse(S.resdirs("b"), [weight], mp_best_weights=old, n_best=3, dataset=ds)[0]
        assert list(have) == list(want)
        for key in NINE:
            assert have[key] == pytest.approx(want[key], rel=1e-12), (weight, key)
    assert best == old and 1 <= len(best) <= 3                  # a metric below the worst kept never enters: the list may stay short


def test_two_runs_give_the_same_bits():
    from afft_amd import ops
    gen = torch.Generator().manual_seed(7)
    xs = _views(3, 5, 3806, "padded", gen)
    w = torch.randn(2 * WT + 3, 3, generator=gen).to(DEV)
    labels = torch.randint(0, 3806, (5,), generator=gen).to(DEV)
    a, b = ops.fused_label_rank(xs, w, labels), ops.fused_label_rank(xs, w, labels)
    assert torch.equal(a, b)
    out = []
    for _ in range(2):
        counters = [torch.zeros(w.shape[0], 2, dtype=torch.int32, device=DEV), torch.zeros(w.shape[0], 3806, dtype=torch.int32, device=DEV),
                    torch.zeros(3806, dtype=torch.int32, device=DEV)]
        ops.rank_counts_sets(a, labels, 3806, 5, *counters)
        out.append(counters)
    assert all(torch.equal(p, q) for p, q in zip(*out))


def test_refusals_raise_on_the_host_before_any_launch():
    from afft_amd import ops
    rows, C = 4, 10
    x = torch.randn(rows, C, device=DEV)
    labels = torch.zeros(rows, dtype=torch.int64, device=DEV)
    rank = torch.full((3, rows), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="n <= 8"):
        ops.fused_label_rank([x] * 9, torch.ones(3, 9, device=DEV), labels, rank=rank)
    with pytest.raises(RuntimeError, match="nsets"):
        ops.fused_label_rank([x], torch.ones(0, 1, device=DEV), labels)
    short = torch.as_strided(rank, (3, rows), (rows - 1, 1))
    with pytest.raises(RuntimeError, match="ldr"):
        ops.fused_label_rank([x], torch.ones(3, 1, device=DEV), labels, rank=short)
    wide = torch.randn(rows, C + 4, device=DEV)[:, :C]
    with pytest.raises(RuntimeError, match="row stride"):
        ops.fused_label_rank([x, wide], torch.ones(3, 2, device=DEV), labels, rank=rank)
    hits, tps, nums = (torch.zeros(s, dtype=torch.int32, device=DEV) for s in ((3, 2), (3, C), (C,)))
    with pytest.raises(RuntimeError, match="k <= C"):
        ops.rank_counts_sets(rank, labels, C, C + 1, hits, tps, nums)
    with pytest.raises(RuntimeError, match="ldr"):
        ops.rank_counts_sets(short, labels, C, 1, hits, tps, nums)
    torch.cuda.synchronize()
    assert bool((rank == -7).all()) and not bool(hits.any()) and not bool(tps.any()) and not bool(nums.any())
