"""MI355X mirror of the reference's ``common/metric_tracking.py``: the meters of the training loop.

  MeanTopKRecallMeter  <- common/metric_tracking.py:10-53   two input forms, see below
  AverageMeter         <- common/metric_tracking.py:56-88   same behaviour (device scalars and runner.LazyScalar both work with it)
  MetricTracker        <- common/metric_tracking.py:91-185  same behaviour: constructor, methods, key prefixes, to_string format

``MeanTopKRecallMeter.update`` takes what ``Runner`` puts under the ``mt5r_*`` keys, in either form:

  host    {'logits': (B, C), 'labels': (B,)} as numpy arrays or runner.LazyHostArray: the reference's arithmetic (an argsort of
          every row and a loop over the labels present), on the host;
  device  {'rank': int32 (B,), 'labels': int64 (B,), 'k': int} as device tensors (Runner(device_metrics=True)): one
          ops.recall_accumulate launch into int32 per-class counters that live on the device.  Nothing is copied to the host
          until ``value`` is read.  A label outside [0, num_classes) is left out (include/afft_hip.h).

Mixing the two forms between two ``reset()`` calls raises: their counters live in different places.
"""
from typing import Dict

import numpy as np
import torch
import torch.distributed as dist

from .. import ops


def is_dist_avail_and_initialized():
    return dist.is_available() and dist.is_initialized()


class MeanTopKRecallMeter:
    """Mean over the classes seen of their top-k recall: per-class hit and row counters, filled batch by batch."""

    def __init__(self, name, num_classes: int, k=5, string_format='{:.3f}'):
        self.name, self.num_classes, self.k, self.string_format = name, num_classes, k, string_format
        self._device = None       # where the device form was first seen: reset() allocates its counters there from then on

    def reset(self):
        self.tps = np.zeros(self.num_classes)
        self.nums = np.zeros(self.num_classes)
        self._form = None         # 'host' / 'device' once update() has been called
        self._counters = None     # device form: int32 [2, num_classes] = (tps, nums)
        if self._device is not None:
            self._counters = torch.zeros(2, self.num_classes, dtype=torch.int32, device=self._device)

    def _enter(self, form):
        if self._form not in (None, form):
            raise ValueError(f'MeanTopKRecallMeter {self.name}: a {form}-form update after a {self._form}-form update; one epoch '
                             f'takes one form (reset() starts the next)')
        self._form = form

    def update(self, logits_labels_dict, n=1):
        """n (the batch size the tracker passes to every meter) plays no part: the counters count rows"""
        d = logits_labels_dict
        if 'rank' in d:
            self._enter('device')
            if d['k'] != min(self.k, self.num_classes):
                raise ValueError(f"MeanTopKRecallMeter {self.name}: the ranks come with k = {d['k']}, the meter counts "
                                 f"top-{min(self.k, self.num_classes)}")
            if self._counters is None:
                self._device = d['rank'].device
                self._counters = torch.zeros(2, self.num_classes, dtype=torch.int32, device=self._device)
            ops.recall_accumulate(d['rank'], d['labels'], d['k'], self._counters[0], self._counters[1])
            return
        self._enter('host')
        scores, labels = d['logits'], d['labels']
        # the reference's arithmetic: a row hits when its label is among the last k entries of the row's ascending argsort
        hit = (np.argsort(scores, axis=1)[:, -self.k:] == labels.reshape(-1, 1)).max(1)
        for cls in np.unique(labels):
            rows = labels == cls
            self.tps[cls] += hit[rows].sum()
            self.nums[cls] += rows.sum()

    def synchronize_between_processes(self):
        if not is_dist_avail_and_initialized():
            return
        if self._counters is not None and self._form != 'host':
            dist.all_reduce(self._counters)      # in place, in stream order behind the kernels: no barrier, no host-built tensor
            return
        # host form, as the reference does it: the float64 counters become tensors and stay tensors
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
        self.tps, self.nums = torch.tensor(self.tps, device=device), torch.tensor(self.nums, device=device)
        dist.barrier()
        dist.all_reduce(self.tps)
        dist.all_reduce(self.nums)

    @property
    def value(self):
        tps, nums = self.tps, self.nums
        if self._form == 'device':
            tps, nums = self._counters.cpu().numpy().astype(np.float64)      # the one fetch; finished in float64 like the host form
        seen = nums > 0
        recalls = tps[seen] / nums[seen]
        return recalls.mean() * 100 if len(recalls) > 0 else None

    def to_string(self):
        return self.string_format.format(self.value)


class AverageMeter:
    """Running mean of a scalar weighted by the batch size.  val may be a float, a 0-dim device tensor (acc1 / acc5) or a
    runner.LazyScalar: only `val * n` and `+=` are asked of it."""

    def __init__(self, name, string_format='{:.3f}'):
        self.name, self.string_format = name, string_format

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n

    def synchronize_between_processes(self):
        if not is_dist_avail_and_initialized():
            return
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
        totals = [torch.as_tensor(v, device=device) for v in (self.count, self.sum)]
        dist.barrier()
        for t in totals:
            dist.all_reduce(t)
        self.count, self.sum = totals

    @property
    def value(self):
        self.avg = self.sum / self.count
        return self.avg

    def to_string(self):
        return self.string_format.format(self.value)


class MetricTracker:
    """All meters of a run, by name, one set for training and one for validation: a name containing 'mt5r' gets a
    MeanTopKRecallMeter (its class count looked up by the target type in the name), every other an AverageMeter."""
    training_prefix, validation_prefix = 'train_', 'val_'

    def __init__(self, num_classes: Dict[str, int]):
        self.num_classes = num_classes
        self.training_metrics, self.validation_metrics = {}, {}

    def _meters(self, is_training):
        return self.training_metrics if is_training else self.validation_metrics

    def _get_num_classes(self, name):
        found = [n for key, n in self.num_classes.items() if key in name]
        if not found:
            raise ValueError(f'mt5r metric {name!r} names none of the target types {list(self.num_classes)}')
        return found[-1]

    def add_metric(self, name, is_training=None):
        meter = MeanTopKRecallMeter(name, self._get_num_classes(name)) if 'mt5r' in name else AverageMeter(name)
        meter.reset()
        if is_training is None or is_training:
            self.training_metrics[name] = meter
        if is_training is None or not is_training:
            self.validation_metrics[name] = meter

    def update(self, metric_dict: Dict, batch_size: int, is_training: bool):
        meters = self._meters(is_training)
        prefix = self.training_prefix if is_training else self.validation_prefix
        for key, value in metric_dict.items():
            if prefix + key not in meters:
                self.add_metric(prefix + key, is_training)
            meters[prefix + key].update(value, batch_size)

    def synchronize_between_processes(self, is_training):
        for meter in self._meters(is_training).values():
            meter.synchronize_between_processes()

    def reset(self):
        for meter in list(self.training_metrics.values()) + list(self.validation_metrics.values()):
            meter.reset()

    def get_all_data(self, is_training):
        return {name: meter.value for name, meter in self._meters(is_training).items()}

    def get_data(self, metric_name, is_training):
        return self._meters(is_training)[metric_name].value

    def to_string(self, is_training):
        colour, title = ('\33[0;36;40m', 'Training:    ') if is_training else ('\33[0;32;40m', 'Validation:  ')
        body = ''.join(f'{m.name}: {m.to_string()}   ' for m in self._meters(is_training).values())
        return colour + title + body + '\033[0m'
