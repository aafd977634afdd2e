#!/usr/bin/env python
"""Time the EPIC-KITCHENS-100 validation report on the device (afft_rank_counts_groups, challenge.device_accuracies_epic, the grouped
device_sweep) at validation size against what the parent commit offers: N = 9668 segments, R = 3 runs, 64 weight sets, for the action
(C = 3806), noun (300) and verb (97) spaces; three row groups (all rows, unseen participants, tail classes).

    python tools/eval_report_bench.py [--out profiles/eval_report.txt] [--sets 64] [--reps 5]

Per space it reports:
  counting   the sweep's counting launch on the [sets, N] ranks of afft_fused_label_rank: afft_rank_counts_groups with ngroups = 3
             against afft_rank_counts_sets (the parent's launch: one group) -- device events around the one launch, medians;
  report     device_sweep with the membership words over all sets (fused_label_rank + rank_counts_groups + the copy of the counters +
             the float64 arithmetic), per weight set, against the ungrouped device_sweep -- host clock, medians;
and once, for the three spaces together:
  host       compute_accuracies_epic(combination, dataset, True) on ONE materialised combination already on the host, the parent's only
             route to the many-shot / unseen / tail numbers of a combination -- ONE window, not a median (it takes seconds);
  single     the metric stage of evaluate.evaluate (device_accuracies_epic(..., True) on three device matrices; median) against the
             bookkeeping of marginalize_verb_noun (the copy of the three matrices to the host + compute_accuracies_epic(..., True); ONE
             window).
Every timed window ends in a device synchronise and is warmed up first.  The device report is checked against the host's before
anything is timed (scores are random normal: tie-free)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _median_ms(fn, reps, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def _event_ms(fn, reps, warmup=2):
    import torch
    ev = []
    for _ in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    return statistics.median(ev[warmup:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--N", type=int, default=9668)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import pandas as pd
    import torch
    from afft_amd import challenge, ops
    if not torch.cuda.is_available():
        raise SystemExit("eval_report_bench: no GPU visible (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    N, R = a.N, a.runs
    spaces = (("action", 3806), ("noun", 300), ("verb", 97))
    weights = (torch.rand(a.sets, R, generator=gen) * 2).numpy().astype(np.float32)
    ids = np.asarray([f"P{1 + i % 37:02d}_{100 + i % 11}_{i}" for i in range(N)])
    pick = lambda share: ids[torch.rand(N, generator=gen).numpy() < share]      # noqa: E731
    tmp = tempfile.TemporaryDirectory()
    for name, share in (("validation_unseen_participants_ids.csv", 0.2), ("validation_tail_verbs_ids.csv", 0.3),
                        ("validation_tail_nouns_ids.csv", 0.3), ("validation_tail_actions_ids.csv", 0.3)):
        with open(os.path.join(tmp.name, name), "w", encoding="utf-8") as fh:
            fh.write("\n".join(pick(share)) + "\n")
    xs, labels = {}, {}
    for name, C in spaces:
        xs[name] = [torch.randn(N, C, generator=gen).to(dev) for _ in range(R)]
        labels[name] = torch.randint(0, C, (N,), generator=gen)

    class _DS:
        df = pd.DataFrame(dict(narration_id=ids, **{f"{name}_class": labels[name].numpy() for name, _ in spaces}))
        classes_manyshot = {name: {f"{name}{c}": c for c in range(0, C, 3)} for name, C in spaces}
        version = challenge.EPIC100_VERSION
        rulstm_annotation_dir = tmp.name
    groups = challenge.row_groups(_DS)
    lines = [f"EPIC-KITCHENS-100 validation report: N = {N} segments, R = {R} runs, {a.sets} weight sets, 3 row groups (all, unseen "
             f"{int(((groups['verb'] >> 1) & 1).sum())} rows, tail ~30 %); medians of {a.reps} windows unless a line says otherwise; every "
             f"window ends in a device synchronise", f"device: {torch.cuda.get_device_name(0)}", ""]
    w_dev = torch.from_numpy(weights).to(dev)
    for name, C in spaces:
        lab = labels[name].to(dev)
        member = torch.from_numpy(groups[name].view(np.int32)).to(dev)
        rank = ops.fused_label_rank(xs[name], w_dev, lab)
        k = min(5, C)
        g3 = [torch.zeros(n, dtype=torch.int32, device=dev) for n in (a.sets * 3 * 2, a.sets * 3 * C, 3 * C, 3)]
        g1 = [torch.zeros(n, dtype=torch.int32, device=dev) for n in (a.sets * 2, a.sets * C, C, 1)]
        s1 = [torch.zeros(n, dtype=torch.int32, device=dev) for n in (a.sets * 2, a.sets * C, C)]
        t_g3 = _event_ms(lambda: ops.rank_counts_groups(rank, lab, C, k, member, 3, *g3), a.reps)
        t_g1 = _event_ms(lambda: ops.rank_counts_groups(rank, lab, C, k, None, 1, *g1), a.reps)
        t_s1 = _event_ms(lambda: ops.rank_counts_sets(rank, lab, C, k, *s1), a.reps)
        many = _DS.classes_manyshot[name]
        t_rep = _median_ms(lambda: challenge.device_sweep(xs[name], lab, weights, classes=many, member=groups[name], ngroups=3), a.reps)
        t_plain = _median_ms(lambda: challenge.device_sweep(xs[name], lab, weights), a.reps)
        lines += [f"{name} (C = {C}):",
                  f"  counting  rank_counts_groups, 3 groups {1e3 * t_g3:9.1f} us   | 1 group, no member {1e3 * t_g1:9.1f} us   | rank_counts_sets "
                  f"(parent) {1e3 * t_s1:9.1f} us   for {a.sets} sets; groups(3) / sets = {t_g3 / t_s1:.2f}",
                  f"  report    {t_rep / a.sets:9.4f} ms per set   ({t_rep:.3f} ms for {a.sets} sets: device_sweep with 3 groups and the many-shot "
                  f"classes)   | ungrouped device_sweep {t_plain / a.sets:9.4f} ms per set ({t_plain:.3f} ms)", ""]
        print("\n".join(lines[-4:]), flush=True)
    # one combination, materialised and on the host: the parent's route to the full report of a combination
    combo = []
    for name in ("verb", "noun", "action"):
        out = torch.empty_like(xs[name][0])
        ops.weighted_sum_fwd(xs[name], w_dev[:1].expand(N, R), out)
        combo.append(out)
    host_combo = [c.cpu().numpy() for c in combo]
    t0 = time.perf_counter()
    want = challenge.compute_accuracies_epic(host_combo, _DS, True)
    t_host = time.perf_counter() - t0
    got = challenge.device_accuracies_epic(combo, _DS, True)
    assert list(got) == list(want) and all(abs(got[key] - want[key]) < 1e-9 for key in want), (got, want)
    sweep = {name: challenge.device_sweep(xs[name], labels[name], weights[:1], classes=_DS.classes_manyshot[name], member=groups[name],
                                          ngroups=3) for name, _ in spaces}
    for name, _ in spaces:
        s = name[0]
        assert abs(sweep[name][2][0, 0] - want[f"{s}mt5r"]) < 1e-9 and abs(sweep[name][3][0, 0] - want[f"{s}mt5r_ms"]) < 1e-9
        assert abs(sweep[name][2][0, 1] - want[f"{s}mt5r_unseen"]) < 1e-9 and abs(sweep[name][2][0, 2] - want[f"{s}mt5r_tail"]) < 1e-9
    t_dev = _median_ms(lambda: challenge.device_accuracies_epic(combo, _DS, True), a.reps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    challenge.compute_accuracies_epic([c.cpu().numpy() for c in combo], _DS, True)
    t_book = time.perf_counter() - t0
    lines += ["all three spaces together (device report checked against the host's to 1e-9 first):",
              f"  host      {1e3 * t_host:10.1f} ms per combination   (compute_accuracies_epic(..., True) on one materialised combination on the host; "
              f"ONE window)",
              f"  single    {t_dev:10.3f} ms   (device_accuracies_epic(..., True): evaluate.evaluate's metric stage, id tables read each call; "
              f"median)   | {1e3 * t_book:10.1f} ms   (marginalize_verb_noun's bookkeeping: three copies to the host + "
              f"compute_accuracies_epic(..., True); ONE window)", ""]
    print("\n".join(lines[-4:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))
    tmp.cleanup()


if __name__ == "__main__":
    main()
