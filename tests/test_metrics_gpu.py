"""GPU: afft_label_rank / afft_recall_accumulate (afft_amd/csrc/metrics.hip) against a float64 / int64 numpy restatement of their
contract (include/afft_hip.h) written here, against tests/golden/k0_metrics.npz (the reference's own accuracy, MixUp adjustment and
recall meter on tie-free inputs), and end to end: Runner(device_metrics=True) + afft_amd.common.metric_tracking against the host
path, challenge.device_accuracy against challenge.compute_accuracy.

Every comparison of ranks, labels and counters is exact: they are integers, and the restatement applies the same tie rule (the lower
class index wins).  acc is float(count) * float32(100 / rows) on both sides, so it is compared bit for bit as well; only the
comparison with runner.accuracy (torch's own reduction) uses the rtol of 1e-6 the arithmetic allows."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "k0_metrics.npz")))


# ----------------------------------------------------------------------------- the restatement
def _argmax_low(t):
    return int(np.flatnonzero(t == t.max())[0])


def ref_rank(x, C, labels=None, soft=None):
    """rank int64 [rows], label int64 [rows] by the definition: one row at a time, scores in float64 (the fold s[i1] += s[i2] is one
    fp32 addition, as in the reference's fp32 clone of the logits)"""
    rows = x.shape[0]
    rank, lab = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    idx = np.arange(C)
    for r in range(rows):
        s = x[r, :C].astype(np.float32).copy()
        if soft is not None:
            t = soft[r, :C].astype(np.float64).copy()
            i1 = _argmax_low(t)
            if C > 1:
                t[i1] = -np.inf
                i2 = _argmax_low(t)
                s[i1] = np.float32(s[i1] + s[i2])
                s[i2] = 0.0
            l = i1
        else:
            l = int(labels[r])
        lab[r] = l
        if not 0 <= l < C:
            rank[r] = C
            continue
        s = s.astype(np.float64)
        rank[r] = int((((s > s[l]) | ((s == s[l]) & (idx < l))) & (idx != l)).sum())
    return rank, lab


def ref_acc(rank, k):
    scale = np.float32(100.0 / len(rank))
    return np.asarray([np.float32((rank < 1).sum()) * scale, np.float32((rank < k).sum()) * scale], np.float32)


def ref_counters(rank, lab, C, k):
    keep = (lab >= 0) & (lab < C)
    return (np.bincount(lab[keep][rank[keep] < k], minlength=C).astype(np.int64), np.bincount(lab[keep], minlength=C).astype(np.int64))


def run(x, C, k, labels=None, soft=None, with_acc=True):
    """x: device tensor / view [rows, >= C]; returns numpy (rank, label_out, acc)"""
    from afft_amd import ops
    rows = x.shape[0]
    rank = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    lab = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    acc = torch.full((2,), -7.0, device=DEV) if with_acc else None
    ops.label_rank(x, C, labels=labels, soft=soft, k=k, rank=rank, label_out=lab, acc=acc)
    return rank, lab, acc


def counters(rank, lab, C, k, times=1):
    from afft_amd import ops
    cnt = torch.zeros(2, C, dtype=torch.int32, device=DEV)
    for _ in range(times):
        ops.recall_accumulate(rank, lab, k, cnt[0], cnt[1])
    return cnt.cpu().numpy()


def _inputs(rows, C, seed):
    """tie-free rows (a permutation of distinct values each), labels with the edge cases where there is room, soft targets of a
    mixed pair (0.7 / 0.3 over a smoothing floor)"""
    g = np.random.default_rng(seed)
    x = np.stack([g.permutation(C) for _ in range(rows)]).astype(np.float32) * np.float32(0.37) - np.float32(0.1 * C)
    labels = g.integers(0, C, rows).astype(np.int64)
    if rows >= 4:
        labels[:4] = [0, C - 1, -1, C]
    if rows >= 6:
        labels[4:6] = [C + 1000, -5]
    soft = np.full((rows, C), 0.1 / C, np.float32)
    a = g.integers(0, C, rows)
    b = (a + 1 + g.integers(0, max(C - 1, 1), rows)) % C
    soft[np.arange(rows), a] += 0.63
    if C > 1:
        soft[np.arange(rows), b] += 0.27
    return x, labels, soft


# ----------------------------------------------------------------------------- kernels against the restatement
@pytest.mark.parametrize("rows", [1, 2, 48, 300])
@pytest.mark.parametrize("C", [1, 3, 5, 211, 257, 3806])
def test_rank_acc_and_counters_match_the_restatement(C, rows):
    k = min(5, C)
    x, labels, soft = _inputs(rows, C, seed=1000 * C + rows)
    xd = torch.from_numpy(x).to(DEV)
    for kw_ref, kw_dev in ((dict(labels=labels), dict(labels=torch.from_numpy(labels).to(DEV))),
                           (dict(soft=soft), dict(soft=torch.from_numpy(soft).to(DEV)))):
        want_rank, want_lab = ref_rank(x, C, **kw_ref)
        rank, lab, acc = run(xd, C, k, **kw_dev)
        assert np.array_equal(rank.cpu().numpy(), want_rank), kw_ref.keys()
        assert np.array_equal(lab.cpu().numpy(), want_lab)
        assert np.array_equal(acc.cpu().numpy(), ref_acc(want_rank, k)), (acc, ref_acc(want_rank, k))
        want_tps, want_nums = ref_counters(want_rank, want_lab, C, k)
        got = counters(rank, lab, C, k, times=2)                     # two calls accumulate
        assert np.array_equal(got[0], 2 * want_tps) and np.array_equal(got[1], 2 * want_nums)
        assert want_nums.sum() == ((want_lab >= 0) & (want_lab < C)).sum()
    # without acc: one launch, the same ranks
    rank2, _, _ = run(xd, C, k, soft=torch.from_numpy(soft).to(DEV), with_acc=False)
    assert torch.equal(rank2, rank)


def test_rows_are_walked_where_they_lie():
    """logits[:, 0, :] of a (B, 2, 3840-pitch) buffer (row_stride = 2 * 3840, 16-byte loads), and a view whose rows are not 16-byte
    aligned (odd pitch, base off by one element: the scalar path); the soft targets strided as well"""
    C, rows, k = 3806, 48, 5
    x, labels, soft = _inputs(rows, C, seed=7)
    want_h, want_s = ref_rank(x, C, labels=labels), ref_rank(x, C, soft=soft)
    big = torch.full((rows, 2, 3840), float("nan"), device=DEV)
    big[:, 0, :C] = torch.from_numpy(x).to(DEV)
    view = big[:, 0, :C]
    assert view.stride(0) == 2 * 3840
    odd = torch.full((rows * 3811 + 1,), float("nan"), device=DEV)
    oview = odd[1:].view(rows, 3811)[:, :C]
    oview.copy_(torch.from_numpy(x).to(DEV))
    sbig = torch.zeros(rows, 3811, device=DEV)
    sbig[:, :C] = torch.from_numpy(soft).to(DEV)
    lab_d = torch.from_numpy(labels).to(DEV)
    for v in (view, oview):
        rank, lab, acc = run(v, C, k, labels=lab_d)
        assert np.array_equal(rank.cpu().numpy(), want_h[0]) and np.array_equal(lab.cpu().numpy(), want_h[1])
        assert np.array_equal(acc.cpu().numpy(), ref_acc(want_h[0], k))
        rank, lab, _ = run(v, C, k, soft=sbig[:, :C])
        assert np.array_equal(rank.cpu().numpy(), want_s[0]) and np.array_equal(lab.cpu().numpy(), want_s[1])


def test_label_edges_and_colliding_counters():
    C, rows, k = 5, 300, 5
    x, _, _ = _inputs(rows, C, seed=3)
    xd = torch.from_numpy(x).to(DEV)
    # every row the same label: 300 updates of one counter pair
    labels = np.full(rows, 3, np.int64)
    rank, lab, acc = run(xd, C, 2, labels=torch.from_numpy(labels).to(DEV))
    want_rank, want_lab = ref_rank(x, C, labels=labels)
    assert np.array_equal(rank.cpu().numpy(), want_rank)
    got = counters(rank, lab, C, 2)
    assert got[1].tolist() == [0, 0, 0, rows, 0] and got[0].tolist() == [0, 0, 0, int((want_rank < 2).sum()), 0]
    # labels outside [0, C): rank = C, out of the counters, inside the accuracy's denominator
    labels = np.asarray([0, C - 1, -1, C, 2 ** 40, -2 ** 40], np.int64)
    x6 = np.tile(np.asarray([5, 4, 3, 2, 1], np.float32), (6, 1))
    rank, lab, acc = run(torch.from_numpy(x6).to(DEV), C, 5, labels=torch.from_numpy(labels).to(DEV))
    assert rank.tolist() == [0, 4, C, C, C, C] and lab.tolist() == labels.tolist()
    assert np.array_equal(acc.cpu().numpy(), np.asarray([np.float32(1) * np.float32(100.0 / 6), np.float32(2) * np.float32(100.0 / 6)]))
    got = counters(rank, lab, C, 5)
    assert got[1].tolist() == [1, 0, 0, 0, 1] and got[0].tolist() == [1, 0, 0, 0, 1]


@pytest.mark.parametrize("C,k", [(3, 3), (5, 5), (211, 5), (3806, 5)])
def test_rank_boundary(C, k):
    """rows whose label ranks exactly k - 1 (the last hit) and exactly k (the first miss; k = C: no such row exists)"""
    x = np.tile(np.arange(C, 0, -1, dtype=np.float32), (2, 1))       # class c has rank c
    labels = np.asarray([k - 1, min(k, C - 1)], np.int64)
    rank, lab, acc = run(torch.from_numpy(x).to(DEV), C, k, labels=torch.from_numpy(labels).to(DEV))
    assert rank.tolist() == labels.tolist()
    hits = 1 + (labels[1] < k)
    assert acc.tolist() == [float(np.float32(1 if k == 1 else 0) * np.float32(50.0)), float(np.float32(hits) * np.float32(50.0))]
    got = counters(rank, lab, C, k)
    assert got[0].sum() == hits and got[1].sum() == 2


def test_soft_targets_fold_the_second_label_into_the_first():
    C, k = 257, 5
    g = np.random.default_rng(11)
    pairs = [(100, 101), (101, 100), (0, C - 1), (C - 1, 0), (7, 200)]      # adjacent, the two ends, far apart
    x = (g.permutation(len(pairs) * C).reshape(len(pairs), C).astype(np.float32) - 600.0) * np.float32(0.01)
    soft = np.full((len(pairs), C), 1e-4, np.float32)
    for r, (i1, i2) in enumerate(pairs):
        soft[r, i1], soft[r, i2] = 0.7, 0.3
    # last row: the second label carries by far the largest logit.  It is folded into the first label's score and scores 0 itself:
    # the first label ranks 0, and would not with the logits as they are
    x[4, 200], x[4, 7] = 50.0, -1.0
    want_rank, want_lab = ref_rank(x, C, soft=soft)
    rank, lab, _ = run(torch.from_numpy(x).to(DEV), C, k, soft=torch.from_numpy(soft).to(DEV))
    assert lab.tolist() == [p[0] for p in pairs] == want_lab.tolist()
    assert np.array_equal(rank.cpu().numpy(), want_rank)
    assert rank[4].item() == 0 and ref_rank(x[4:5], C, labels=np.asarray([7]))[0][0] > 0
    # by hand for row 2: s[0] = x[0] + x[C - 1], s[C - 1] = 0
    s = x[2].astype(np.float64)
    s[0] = np.float32(x[2, 0] + x[2, C - 1])
    s[C - 1] = 0.0
    assert rank[2].item() == int((s[1:] > s[0]).sum())


def test_tie_rule_lowest_index_wins():
    """the project's definition (include/afft_hip.h), tested against itself: equal scores rank by class index; a single-peak target
    (MixUp of two samples with the same label: every other entry equal) takes the lowest other class as its second label"""
    C, k = 211, 5
    labels = np.asarray([0, 1, 4, 5, 100, C - 1], np.int64)
    x = np.full((len(labels), C), 1.5, np.float32)
    rank, lab, acc = run(torch.from_numpy(x).to(DEV), C, k, labels=torch.from_numpy(labels).to(DEV))
    assert rank.tolist() == labels.tolist()                  # every lower class is ahead, no higher one
    assert acc.tolist() == [float(np.float32(1) * np.float32(100.0 / 6)), float(np.float32(3) * np.float32(100.0 / 6))]
    g = np.random.default_rng(5)
    x = g.permutation(3 * C).reshape(3, C).astype(np.float32)
    soft = np.full((3, C), 0.1 / C, np.float32)
    peaks = [0, 17, C - 1]
    for r, p in enumerate(peaks):
        soft[r, p] = 0.9
    rank, lab, _ = run(torch.from_numpy(x).to(DEV), C, k, soft=torch.from_numpy(soft).to(DEV))
    assert lab.tolist() == peaks
    for r, p in enumerate(peaks):
        i2 = 1 if p == 0 else 0
        s = x[r].astype(np.float64)
        s[p] = np.float32(x[r, p] + x[r, i2])
        s[i2] = 0.0
        assert rank[r].item() == int(((s > s[p]) & (np.arange(C) != p)).sum()), r
    # two equal peaks: the lower one is the label, the higher one is folded in
    soft = np.full((1, C), 0.0, np.float32)
    soft[0, 30] = soft[0, 20] = 0.5
    _, lab, _ = run(torch.from_numpy(x[:1]).to(DEV), C, k, soft=torch.from_numpy(soft).to(DEV))
    assert lab.tolist() == [20]
    assert np.array_equal(ref_rank(x[:1], C, soft=soft)[1], [20])


# ----------------------------------------------------------------------------- against the reference's own numbers
@pytest.mark.parametrize("tag", ["hard", "soft"])
def test_matches_reference_golden(golden, tag):
    from afft_amd.common.runner import accuracy
    g = golden
    B, C = g["logits"].shape
    xd = torch.from_numpy(g["logits"]).to(DEV)
    kw = dict(labels=torch.from_numpy(g["labels"]).to(DEV)) if tag == "hard" else dict(soft=torch.from_numpy(g["soft"]).to(DEV))
    rank, lab, acc = run(xd, C, 5, **kw)
    want_lab = g["labels"] if tag == "hard" else g["soft_labels"]
    assert np.array_equal(lab.cpu().numpy(), want_lab)
    assert np.array_equal((rank.cpu().numpy() < 5).astype(np.int64), g[f"{tag}_tp"])
    got = np.zeros((2, C), np.int64)
    for sl in (slice(0, B // 2), slice(B // 2, B)):                 # the two update calls of the golden
        got += counters(rank[sl].contiguous(), lab[sl].contiguous(), C, 5)
    assert np.array_equal(got[0], g[f"{tag}_tps"]) and np.array_equal(got[1], g[f"{tag}_nums"])
    ref = np.asarray([g[f"{tag}_acc1"], g[f"{tag}_acc5"]], np.float32)
    a = acc.cpu().numpy()
    print(f"[{tag}] acc {a.tolist()} reference {ref.tolist()} bit-equal {np.array_equal(a, ref)}")
    np.testing.assert_allclose(a, ref, rtol=1e-6, atol=0)
    if tag == "hard":
        # runner.accuracy (torch.topk on the GPU) on the same tie-free input
        t1, t5 = accuracy(xd[:, None, :], torch.from_numpy(g["labels"]).to(DEV)[:, None], topk=(1, 5))
        t = np.asarray([t1.item(), t5.item()], np.float32)
        print(f"[{tag}] runner.accuracy {t.tolist()} bit-equal {np.array_equal(a, t)}")
        np.testing.assert_allclose(a, t, rtol=1e-6, atol=0)


def test_two_runs_are_bitwise_equal():
    C, rows, k = 3806, 300, 5
    x, labels, soft = _inputs(rows, C, seed=21)
    labels[:] = labels % 7                       # heavy collisions in the counters
    xd, ld, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(labels).to(DEV), torch.from_numpy(soft).to(DEV)
    outs = []
    for _ in range(2):
        rank, lab, acc = run(xd, C, k, labels=ld)
        rank_s, lab_s, acc_s = run(xd, C, k, soft=sd)
        outs.append([t.cpu().numpy() for t in (rank, lab, acc, rank_s, lab_s, acc_s)] + [counters(rank, lab, C, k), counters(rank_s, lab_s, C, k)])
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


def test_errors_are_reported():
    """bad arguments come back as error codes with text; nothing is launched"""
    from afft_amd import _lib as L
    from afft_amd import ops
    C, rows = 5, 4
    x = torch.zeros(rows, C, device=DEV)
    labels = torch.zeros(rows, dtype=torch.int64, device=DEV)
    soft = torch.zeros(rows, C, device=DEV)
    rank, lab = torch.empty(rows, dtype=torch.int32, device=DEV), torch.empty(rows, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(2, C, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="1 <= k <= C"):
        ops.label_rank(x, C, labels=labels, k=C + 1, rank=rank, label_out=lab)
    with pytest.raises(RuntimeError, match="1 <= k <= C"):
        ops.label_rank(x, C, labels=labels, k=0, rank=rank, label_out=lab)
    with pytest.raises(RuntimeError, match="exactly one of labels / soft"):
        ops.label_rank(x, C, labels=labels, soft=soft, k=1, rank=rank, label_out=lab)
    with pytest.raises(RuntimeError, match="exactly one of labels / soft"):
        ops.label_rank(x, C, k=1, rank=rank, label_out=lab)
    with pytest.raises(RuntimeError, match="1 <= k <= C"):
        ops.recall_accumulate(rank, lab, C + 1, cnt[0], cnt[1])
    s = torch.cuda.current_stream().cuda_stream
    rc = L.lib().afft_label_rank(x.data_ptr(), C - 1, rows, C, labels.data_ptr(), None, 0, 1, 25.0, rank.data_ptr(), lab.data_ptr(), None, s)
    assert rc != 0
    with pytest.raises(RuntimeError, match="row_stride 4 < C = 5"):
        L.check(rc, "label_rank")
    rc = L.lib().afft_label_rank(x.data_ptr(), C, 0, C, labels.data_ptr(), None, 0, 1, 25.0, rank.data_ptr(), lab.data_ptr(), None, s)
    assert rc != 0 and b"rows >= 1" in L.lib().afft_last_error()
    torch.cuda.synchronize()
    assert int(cnt.sum()) == 0


# ----------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("mixup", [False, True])
def test_runner_and_tracker_device_metrics_equal_the_host_path(mixup):
    """3 steps of the small t0_sa model: Runner(device_metrics=True) + the mirrored tracker against Runner(async_metrics=False) +
    the host form of the same tracker.  Labels within a batch are distinct, so the MixUp targets have two distinct peaks."""
    from helpers import case_tensors
    from test_model_gpu import build
    from afft_amd import runtime as rt
    from afft_amd.common.metric_tracking import MetricTracker
    from afft_amd.common.mixup import MixUp
    from afft_amd.common.runner import Runner
    c, state, _, _, _ = case_tensors("t0_sa")
    model = build(c, "fp32")
    model.load_state_dict(state)
    model = model.cuda().eval()
    dev = torch.device(DEV)
    K, B = c["num_classes"], 6
    wts = {"cls_action": 1.0, "past_cls_action": 1.0, "past_reg": 1.0}
    mix = None
    if mixup:
        mix = MixUp(alpha=0.1, label_smoothing={"action": 0.1}, num_classes={"action": K})
        mix.mixup_beta_sampler = type("S", (), {"sample": staticmethod(lambda: torch.tensor(0.3))})()
    dev_runner = Runner(model, dev, wts, device_metrics=True)
    host_runner = Runner(model, dev, wts, async_metrics=False, device_metrics=False)
    trackers = MetricTracker({"action": K}), MetricTracker({"action": K})
    g = torch.Generator().manual_seed(3)
    for step in range(3):
        data = {m: torch.randn(B, c["T"], C, 1, 1, 1, generator=g) for m, C in c["modal_dims"].items()}
        tgt = (torch.randperm(K, generator=g)[:B]).to(torch.int64)
        sub = torch.randint(0, K, (B, c["T"], 1), generator=g)
        batch = ({"data_dict": data, "target": {"action": tgt}, "target_subclips": {"action": sub}}, {})
        for runner, tracker in zip((dev_runner, host_runner), trackers):
            rt.SINK.begin_step()
            _, m = runner(batch, mix, True)
            tracker.update(m, B, True)
        key = next(k for k in m if k.startswith("mt5r_action_"))
    entry_d = None
    rt.SINK.begin_step()
    _, m_d = dev_runner(batch, mix, True)
    entry_d = m_d[key]
    assert set(entry_d) == {"rank", "labels", "k"} and entry_d["k"] == 5
    assert entry_d["rank"].is_cuda and entry_d["rank"].dtype == torch.int32 and entry_d["rank"].shape == (B,)
    assert entry_d["labels"].is_cuda and entry_d["labels"].dtype == torch.int64
    a1 = m_d[key.replace("mt5r", "acc1")]
    assert a1.is_cuda and a1.dim() == 0 and a1._base is not None and a1._base.numel() == 2
    md, mh = (t.training_metrics["train_" + key] for t in trackers)
    tps, nums = md._counters.cpu().numpy()
    assert nums.sum() == 3 * B
    assert np.array_equal(tps, mh.tps) and np.array_equal(nums, mh.nums)
    assert md.value == mh.value
    for name in ("acc1", "acc5"):
        kk = "train_" + key.replace("mt5r", name)
        d, h = float(trackers[0].get_data(kk, True)), float(trackers[1].get_data(kk, True))
        assert abs(d - h) <= 1e-6 * max(1.0, abs(h)), (name, d, h)
    for kk in trackers[1].training_metrics:
        if "acc" not in kk and "mt5r" not in kk:
            d, h = float(trackers[0].get_data(kk, True)), float(trackers[1].get_data(kk, True))
            assert abs(d - h) <= 1e-6 * max(1.0, abs(h)), kk


@pytest.mark.parametrize("subset", [False, True])
def test_device_accuracy_equals_compute_accuracy(subset):
    from afft_amd import challenge
    N, C = 300, 97
    g = np.random.default_rng(9)
    scores = np.stack([g.permutation(C) for _ in range(N)]).astype(np.float32) * np.float32(0.25)      # tie-free
    labels = g.integers(0, 40, N).astype(np.int64)                  # classes 40.. never occur
    scores[np.arange(N), labels] += np.float32(0.125) + (np.arange(N) % 5 == 0) * np.float32(20.0)     # still tie-free: odd multiples of 1/8
    classes = {f"c{i}": i for i in (0, 3, 5, 39, 41, 96)} if subset else None
    want = challenge.compute_accuracy(scores, labels, classes=classes)
    got = challenge.device_accuracy(torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV), classes=classes)
    assert abs(got[0] - want[0]) <= 1e-6 * want[0] and abs(got[1] - want[1]) <= 1e-6 * want[1]
    assert abs(got[2] - want[2]) <= 1e-12 * want[2]
