#!/usr/bin/env python3
"""The stream-batched GRU scan of the multi-stream model (fdlp_mmod_compute) against what it replaces, on a batch
resident in HBM.  Reported, not gated.

Workload: the TIMIT recipe's multimod model, 3 modulation streams of 13 columns -> +-4 context (117) -> 1 GRU x 100
per stream -> 1 trunk GRU x 300 -> 40 classes (column, context and class counts are the benchmark's choice), global
CMVN with variances per stream, utterances of U(2, 8) s at 100 frames/s, 32 and 2048 utterances per batch, seeded;
weights are torch's default init range times 3.

For the same weights and batch, the way to the concatenated [rows, 300] sub-network output is timed twice:
  (a) batched   MultimodPlan.compute(tap = the concatenation): the three chain launches, then ONE scan launch on
                the grid (groups, 3) that writes stream s at column 100 s of the concatenated buffer;
  (b) separate  three one-stream RnnPlan.compute (the same chain launch and the same gru_scan_kernel, grid
                (groups, 1), into compact [rows, 100] buffers), then the copy into the concatenated layout
                (torch.cat with out=).
Both ways give the same bits, which is asserted.  Per way: the median of --reps windows of --calls calls between two
device events, the two ways alternating window by window after warm-up calls; and, in a pass of its own with the
plans' profiling on, the HIP-event time of the scan launches alone (fdlp_mmod_times / fdlp_rnn_times), with the
copy's between two events of its own.  Last, the whole model (tap 0) in frames/s and audio-hours/s.

Each batch size is one step, run in a child process under --step-timeout seconds.

    python benchmarks/multimod_throughput.py [--reps 5] [--calls 2] [--out profiles/multimod_throughput.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

DIM, CTX, M, HS, LS, LT, CLASSES = 13, 4, 3, 100, 1, 1, 40
FPS, GU = 100, 32


def window(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def summary(ms):
    return dict(ms=round(float(np.median(ms)), 4), ms_min=round(float(min(ms)), 4), ms_max=round(float(max(ms)), 4))


def step(n_utts, reps, calls):
    import post_numpy as PN
    import torch
    from speech_recognition_tools_amd.multimod import MultimodPlan
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    from test_multimod import make_model
    from xform_throughput import stats_of
    rng = np.random.default_rng(2027)
    sub, trunk, reg = make_model(rng, DIM * (2 * CTX + 1), M, LS, HS, LT, CLASSES)
    lens = [int(v) for v in rng.integers(2 * FPS, 8 * FPS + 1, n_utts)]
    rows = sum(lens)
    cfg = PostConfig(dim=DIM, left_context=CTX, right_context=CTX)
    xs = [np.round(rng.standard_normal((rows, DIM)) * (3.0 - s) + 1.0 + s, 3).astype(np.float32) for s in range(M)]
    feats = [torch.from_numpy(x).cuda() for x in xs]
    norms = [torch.from_numpy(PN.cmvn_norm(stats_of(x), norm_vars=True)).cuda() for x in xs]
    mm = MultimodPlan([cfg] * M, sub, trunk, reg, max_rows=rows, max_utts=n_utts)
    ones = [RnnPlan(cfg, [("gru",) + tuple(l) for l in sub[s]], max_rows=rows, max_utts=n_utts) for s in range(M)]
    cat_a = torch.empty((rows, M * HS), dtype=torch.float32, device="cuda")
    cat_b = torch.empty((rows, M * HS), dtype=torch.float32, device="cuda")
    compact = [torch.empty((rows, HS), dtype=torch.float32, device="cuda") for _ in range(M)]
    logits = torch.empty((rows, CLASSES), dtype=torch.float32, device="cuda")

    def batched():
        mm.compute(feats, lens, norms=norms, tap=LT + 1, out=cat_a)

    def scans_separate():
        for s in range(M):
            ones[s].compute(feats[s], lens, norm=norms[s], norm_vars=True, out=compact[s])

    def copy():
        torch.cat(compact, dim=1, out=cat_b)

    def separate():
        scans_separate()
        copy()

    def whole():
        mm.compute(feats, lens, norms=norms, tap=0, out=logits)

    res = dict(bench="multimod_throughput", utts=n_utts, rows=rows, streams=M, hidden_sub=HS, trunk=M * HS,
               sub_layers=LS, trunk_layers=LT, classes=CLASSES, reps=reps, calls=calls,
               device=torch.cuda.get_device_name(0), groups=-(-n_utts // GU), workgroups_batched=-(-n_utts // GU) * M,
               workgroups_per_separate_launch=-(-n_utts // GU), workspace_bytes=mm.workspace_bytes)
    for fn in (batched, separate, whole):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res["bit_identical"] = bool(torch.equal(cat_a.view(torch.int32), cat_b.view(torch.int32)))
    assert res["bit_identical"], "the two ways to the concatenated output differ"
    a_ms, b_ms = [], []
    for _ in range(reps):                   # alternating, so that what else the machine does falls on both
        a_ms.append(window(batched, calls))
        b_ms.append(window(separate, calls))
    res["to_concat_batched"], res["to_concat_separate"] = summary(a_ms), summary(b_ms)
    res["to_concat_speedup"] = round(res["to_concat_separate"]["ms"] / res["to_concat_batched"]["ms"], 3)
    # the scan launches alone, from the plans' own events around them; the copy between two events
    mm.set_profiling(True)
    for p in ones:
        p.set_profiling(True)
    a_scan, b_scan, b_copy = [], [], []
    for _ in range(reps):
        batched()
        a_scan.append(mm.times()[1])
        scans_separate()
        b_scan.append(sum(p.times()[1] for p in ones))
        b_copy.append(window(copy, 1))
    mm.set_profiling(False)
    for p in ones:
        p.set_profiling(False)
    res["scan_batched"], res["scan_separate"], res["concat_copy"] = summary(a_scan), summary(b_scan), summary(b_copy)
    res["scan_speedup"] = round((res["scan_separate"]["ms"] + res["concat_copy"]["ms"]) / res["scan_batched"]["ms"], 3)
    res["whole_model"] = summary([window(whole, calls) for _ in range(reps)])
    ms = res["whole_model"]["ms"]
    res["frames_per_s"] = round(rows / ms * 1e3)
    res["audio_hours_per_s"] = round(rows / FPS / 3600 / ms * 1e3, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multimod_throughput.jsonl"))
    ap.add_argument("--one", type=int, default=0, help="(internal) run the step with this many utterances")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.one:
        print(json.dumps(step(args.one, args.reps, args.calls)))
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for n in (32, 2048):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--reps", str(args.reps),
                            "--calls", str(args.calls)], capture_output=True, text=True, timeout=args.step_timeout)
        if r.returncode != 0:       # nothing more is started on the device after a step that failed
            print(r.stderr[-3000:], file=sys.stderr)
            return r.returncode
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
