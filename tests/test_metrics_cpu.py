"""Host logic of the device-side metrics in the build container: afft_amd.common.metric_tracking, the Runner switch and
install_as_models(device_metrics=...), with tests/metrics_double.py standing in for the two kernels (ops.label_rank,
ops.recall_accumulate) and tests/cpu_ops.py for the rest.  Expected values: tests/golden/k0_metrics.npz, written by the reference's
own accuracy / MixUp adjustment / MeanTopKRecallMeter on tie-free inputs (tests/golden/make_golden_metrics.py)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metrics_double

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "k0_metrics.npz")))


def _device_form(g, tag, sl=slice(None)):
    """what Runner(device_metrics=True) hands the meter, from the double"""
    logits = torch.from_numpy(g["logits"])[sl]
    B, C = logits.shape
    rank, lab, acc = torch.empty(B, dtype=torch.int32), torch.empty(B, dtype=torch.int64), torch.empty(2)
    kw = dict(labels=torch.from_numpy(g["labels"])[sl]) if tag == "hard" else dict(soft=torch.from_numpy(g["soft"])[sl])
    metrics_double.label_rank(logits, C, k=5, rank=rank, label_out=lab, acc=acc, **kw)
    return {"rank": rank, "labels": lab, "k": 5}, acc


def _host_form(g, tag, sl=slice(None)):
    """the reference's form: (adjusted) logits and labels as numpy arrays"""
    x, lab = g["logits"][sl].copy(), g["labels"][sl]
    if tag == "soft":
        order = np.argsort(-g["soft"][sl], axis=1, kind="stable")
        r = np.arange(len(x))
        x[r, order[:, 0]] += x[r, order[:, 1]]
        x[r, order[:, 1]] = 0.0
        lab = order[:, 0]
    return {"logits": x, "labels": lab}


@pytest.mark.parametrize("tag", ["hard", "soft"])
@pytest.mark.parametrize("form", ["host", "device"])
def test_tracker_reproduces_the_references_counters(golden, tag, form):
    from afft_amd.common.metric_tracking import MetricTracker
    g = golden
    tracker = MetricTracker({"action": 211})
    make = _host_form if form == "host" else _device_form
    with metrics_double.installed():
        for sl in (slice(0, 24), slice(24, 48)):
            entry = make(g, tag, sl)
            entry = entry[0] if form == "device" else entry
            tracker.update({"mt5r_action_all-fused": entry}, 24, True)
        meter = tracker.training_metrics["train_mt5r_action_all-fused"]
        if form == "device":
            tps, nums = meter._counters.numpy()
        else:
            tps, nums = meter.tps, meter.nums
        assert np.array_equal(tps, g[f"{tag}_tps"]) and np.array_equal(nums, g[f"{tag}_nums"])
        assert abs(tracker.get_data("train_mt5r_action_all-fused", True) - float(g[f"{tag}_value"])) <= 1e-12
        assert tracker.to_string(True).count(f"{float(g[f'{tag}_value']):.3f}") == 1
    if form == "device":
        entry, acc = _device_form(g, tag)
        assert np.array_equal((entry["rank"].numpy() < 5).astype(np.int64), g[f"{tag}_tp"])
        assert np.array_equal(entry["labels"].numpy(), g["labels"] if tag == "hard" else g["soft_labels"])
        assert acc[0].item() == g[f"{tag}_acc1"] and acc[1].item() == g[f"{tag}_acc5"]


def test_host_form_equals_device_form_and_mixing_raises(golden):
    from afft_amd.common.metric_tracking import MeanTopKRecallMeter
    host, dev = MeanTopKRecallMeter("h", 211), MeanTopKRecallMeter("d", 211)
    host.reset()
    dev.reset()
    assert host.value is None and dev.value is None
    with metrics_double.installed():
        for tag in ("hard", "soft"):
            host.update(_host_form(golden, tag))
            dev.update(_device_form(golden, tag)[0])
        assert np.array_equal(host.tps, dev._counters[0].numpy()) and np.array_equal(host.nums, dev._counters[1].numpy())
        assert host.value == dev.value
        with pytest.raises(ValueError, match="one epoch takes one form"):
            host.update(_device_form(golden, "hard")[0])
        with pytest.raises(ValueError, match="one epoch takes one form"):
            dev.update(_host_form(golden, "hard"))
        # reset() starts the next epoch: either form again, device counters zeroed where they were first used
        dev.reset()
        assert dev._counters is not None and int(dev._counters.sum()) == 0 and dev.value is None
        dev.update(_host_form(golden, "hard"))
        assert abs(dev.value - float(golden["hard_value"])) <= 1e-12
        wrong_k = dict(_device_form(golden, "hard")[0], k=3)
        host.reset()
        with pytest.raises(ValueError, match="k = 3"):
            host.update(wrong_k)


def test_labels_outside_the_classes_are_left_out(golden):
    from afft_amd.common.metric_tracking import MeanTopKRecallMeter
    m = MeanTopKRecallMeter("d", 211)
    m.reset()
    entry = {"rank": torch.tensor([0, 211, 211, 7], dtype=torch.int32), "labels": torch.tensor([3, -1, 400, 3]), "k": 5}
    with metrics_double.installed():
        m.update(entry)
    assert int(m._counters[1].sum()) == 2 and int(m._counters[0, 3]) == 1 and m.value == 50.0


def test_average_meter_and_tracker_interface():
    from afft_amd.common.metric_tracking import AverageMeter, MetricTracker
    a = AverageMeter("acc1")
    a.reset()
    a.update(torch.tensor(50.0), 4)
    a.update(25.0, 12)
    assert float(a.value) == (50.0 * 4 + 25.0 * 12) / 16 and a.to_string() == "31.250"
    t = MetricTracker({"action": 5, "verb": 3})
    t.update({"acc1_action": 10.0, "total_loss": 2.0}, 8, True)
    t.update({"acc1_action": 20.0}, 8, False)
    assert set(t.training_metrics) == {"train_acc1_action", "train_total_loss"} and set(t.validation_metrics) == {"val_acc1_action"}
    assert t.get_all_data(True) == {"train_acc1_action": 10.0, "train_total_loss": 2.0} and t.get_data("val_acc1_action", False) == 20.0
    assert t.to_string(True) == "\33[0;36;40mTraining:    train_acc1_action: 10.000   train_total_loss: 2.000   \033[0m"
    assert t.to_string(False) == "\33[0;32;40mValidation:  val_acc1_action: 20.000   \033[0m"
    t.reset()
    assert t.training_metrics["train_acc1_action"].count == 0
    with pytest.raises(ValueError):
        t.add_metric("mt5r_noun")
    t.add_metric("val_mt5r_verb_rgb", is_training=False)
    assert t.validation_metrics["val_mt5r_verb_rgb"].num_classes == 3


def test_install_as_models_registers_the_tracker_only_on_request(monkeypatch):
    import afft_amd
    from afft_amd.common import runner
    monkeypatch.delenv("AFFT_DEVICE_METRICS", raising=False)
    saved = {k: v for k, v in sys.modules.items() if k in ("models", "common") or k.startswith(("models.", "common."))}
    for k in saved:
        del sys.modules[k]
    try:
        afft_amd.install_as_models()
        assert "common.metric_tracking" not in sys.modules and runner.DEVICE_METRICS_DEFAULT is None
        assert runner.Runner(None, torch.device("cpu"), {}).device_metrics is False
        afft_amd.install_as_models(device_metrics=True)
        import common.metric_tracking as mt
        assert mt.__name__ == "afft_amd.common.metric_tracking" and sys.modules["common"].metric_tracking is mt
        assert runner.Runner(None, torch.device("cpu"), {}).device_metrics is True
        assert runner.Runner(None, torch.device("cpu"), {}, device_metrics=False).device_metrics is False
    finally:
        runner.DEVICE_METRICS_DEFAULT = None
        common = sys.modules.get("common")
        if common is not None and hasattr(common, "metric_tracking"):
            delattr(common, "metric_tracking")
        for k in [k for k in sys.modules if k in ("models", "common") or k.startswith(("models.", "common."))]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_runner_reads_the_environment_switch(monkeypatch):
    from afft_amd.common.runner import Runner
    monkeypatch.setenv("AFFT_DEVICE_METRICS", "1")
    assert Runner(None, torch.device("cpu"), {}).device_metrics is True
    monkeypatch.setenv("AFFT_DEVICE_METRICS", "0")
    assert Runner(None, torch.device("cpu"), {}).device_metrics is False


def test_runner_without_device_metrics_returns_todays_keys_and_types(monkeypatch):
    """device_metrics=False (and the default) is the path of the parent commit: numpy logits / labels for the meter, 0-dim accuracy
    tensors, floats for the losses; logits that are not on the GPU take that path even with the switch on"""
    import cpu_ops
    from test_parallel_cpu import WTS, _afft_case, _afft_model
    from afft_amd.common.metric_tracking import MetricTracker
    from afft_amd.common.runner import Runner
    monkeypatch.delenv("AFFT_DEVICE_METRICS", raising=False)
    c, state, data, tgt, sub = _afft_case()
    batch = ({"data_dict": data, "target": {"action": tgt}, "target_subclips": {"action": sub}}, {})
    with cpu_ops.installed(), metrics_double.installed():
        model = _afft_model(c, state, "fp32")
        got = {}
        for name, kw in (("off", dict(device_metrics=False)), ("default", {}), ("on_cpu", dict(device_metrics=True))):
            _, got[name] = Runner(model, torch.device("cpu"), WTS, async_metrics=False, **kw)(batch, None, True)
    m = got["off"]
    B, C = len(tgt), c["num_classes"]
    mt5r = [k for k in m if k.startswith("mt5r_action_")]
    assert len(mt5r) == 1
    modk = mt5r[0][len("mt5r_action_"):]
    assert set(m) == {f"acc1_action_{modk}", f"acc5_action_{modk}", f"mt5r_action_{modk}", f"cls_action_{modk}",
                      f"past_cls_action_{modk}", f"past_reg_{modk}", "total_loss"}
    entry = m[mt5r[0]]
    assert set(entry) == {"logits", "labels"} and isinstance(entry["logits"], np.ndarray) and entry["logits"].shape == (B, C)
    assert isinstance(entry["labels"], np.ndarray) and np.array_equal(entry["labels"], tgt.numpy())
    for k in (f"acc1_action_{modk}", f"acc5_action_{modk}"):
        assert torch.is_tensor(m[k]) and m[k].dim() == 0 and m[k].dtype == torch.float32
    assert isinstance(m["total_loss"], float)
    for other in ("default", "on_cpu"):
        assert set(got[other]) == set(m)
        assert np.array_equal(got[other][mt5r[0]]["logits"], entry["logits"])
    # the mirrored tracker takes the whole dictionary, as train.py hands it over
    tracker = MetricTracker({"action": C})
    tracker.update(m, B, True)
    assert tracker.get_data(f"train_acc1_action_{modk}", True) == m[f"acc1_action_{modk}"]
    assert tracker.training_metrics[f"train_mt5r_action_{modk}"].nums.sum() == B


# ----------------------------------------------------------------------------- world_size 2 over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sync_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    for p in (HERE, os.path.dirname(HERE)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import metrics_double as md
    from afft_amd.common.metric_tracking import MeanTopKRecallMeter
    g = dict(np.load(os.path.join(HERE, "golden", "k0_metrics.npz")))
    sl = slice(0, 24) if rank == 0 else slice(24, 48)
    meter = MeanTopKRecallMeter("mt5r_action", 211)
    meter.reset()
    with md.installed():
        meter.update(_device_form(g, "hard", sl)[0])
        counters = meter._counters
        meter.synchronize_between_processes()
        assert meter._counters is counters, "the all-reduce is in place"
        if rank == 0:
            torch.save({"tps": meter._counters[0].clone(), "nums": meter._counters[1].clone(), "value": meter.value}, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_sum_their_device_counters(golden, tmp_path):
    out = str(tmp_path / "sync.pt")
    mp.spawn(_sync_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out, weights_only=False)
    assert got["tps"].dtype == torch.int32
    assert np.array_equal(got["tps"].numpy(), golden["hard_tps"]) and np.array_equal(got["nums"].numpy(), golden["hard_nums"])
    assert abs(got["value"] - float(golden["hard_value"])) <= 1e-12
