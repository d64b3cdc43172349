#!/usr/bin/env python3
"""Throughput of the GRU acoustic model after the chain (fdlp_rnn_compute: the input projections in xform_kernel /
dense_kernel, the time scans in gru_scan_kernel) on a batch resident in HBM, next to the same model as torch.nn.GRU
on 16 CPU threads, which is how the reference's dump_genclassifier_outputs.py runs it.  Reported, not gated.

Workload: the recipe's nnet_gru_3lenc_1lclas_1lae_256nodes, 13 columns -> +-4 context (117) -> 3 GRU x 256 ->
bottleneck 50 (ReLU) -> 1 GRU x 256 -> 1936 classes (bottleneck and class count are the benchmark's choice), global
CMVN with variances, utterances of U(2, 8) s at 100 frames/s, 64 and 2048 utterances per batch, seeded; weights are
torch's default init range times 3.

Each batch size is one step, run in a child process under --step-timeout seconds.  Reported per step: frames/s and
audio-hours/s of the whole compute (median of --reps windows of --calls calls between two device events, after
warm-up calls); the HIP-event times of the input projections and linear stages versus the scans
(fdlp_rnn_set_profiling); the scans' fraction of the float32 MFMA peak (157.3 TFLOP/s) on the FLOPs they execute
(every group runs 2 x 32 x 3H x ceil(H / 16) 16 per step up to its longest utterance, occupied slots or not); and,
for the 64-utterance batch, the CPU side on a padded, packed batch.

    python benchmarks/gru_throughput.py [--reps 5] [--calls 2] [--out profiles/gru_throughput.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DIM, CTX, HIDDEN, ENC, BN, CLS, CLASSES = 13, 4, 256, 3, 50, 1, 1936
FPS, PEAK_TFLOPS, GU, CPU_THREADS = 100, 157.3, 32, 16


def model(rng):
    from test_rnn import make_stages
    spec = [("gru", HIDDEN)] * ENC + [("linear_relu", BN)] + [("gru", HIDDEN)] * CLS + [("linear", CLASSES)]
    return make_stages(rng, DIM * (2 * CTX + 1), spec)


def scan_flops(lens, stages):
    srt = sorted(lens, reverse=True)
    steps = sum(srt[i] for i in range(0, len(srt), GU))      # the longest utterance of every group
    per = sum(2 * GU * 3 * s[2].shape[1] * (-(-s[2].shape[1] // 16) * 16) for s in stages if s[0] == "gru")
    return steps * per


def torch_cpu(stages, rows_per_utt):
    """the reference's way: nn.GRU layers on a padded batch, packed, then the 1 x 1 convolutions as matmuls"""
    import torch
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    torch.set_num_threads(CPU_THREADS)
    mods = []
    for st in stages:
        if st[0] == "gru":
            g = torch.nn.GRU(st[1].shape[1], st[2].shape[1], batch_first=True)
            with torch.no_grad():
                for p, a in zip((g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0), st[1:]):
                    p.copy_(torch.from_numpy(a))
            mods.append(g.eval())
        else:
            mods.append((st[0], torch.from_numpy(st[1]), torch.from_numpy(st[2])))
    order = np.argsort([-r.shape[0] for r in rows_per_utt], kind="stable")
    lens = torch.tensor([rows_per_utt[i].shape[0] for i in order])
    x = torch.nn.utils.rnn.pad_sequence([torch.from_numpy(rows_per_utt[i]) for i in order], batch_first=True)

    def run():
        with torch.no_grad():
            h, relu = x, False
            for m in mods:
                if isinstance(m, tuple):
                    h = torch.nn.functional.linear(torch.relu(h) if relu else h, m[1], m[2])
                    relu = m[0] == "linear_relu"
                else:
                    h, _ = pad_packed_sequence(m(pack_padded_sequence(torch.relu(h) if relu else h, lens, True))[0], True)
                    relu = False
            return h

    run()
    t0 = time.perf_counter()
    out = run()
    return time.perf_counter() - t0, out, order


def step(n_utts, reps, calls, cpu):
    import post_numpy as PN
    import torch
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    from xform_throughput import stats_of, time_calls
    rng = np.random.default_rng(2026)
    stages = model(rng)
    lens = [int(v) for v in rng.integers(2 * FPS, 8 * FPS + 1, n_utts)]
    rows = sum(lens)
    x = np.round(rng.standard_normal((rows, DIM)) * 3.0 + 1.0, 3).astype(np.float32)
    cfg = PostConfig(dim=DIM, left_context=CTX, right_context=CTX)
    plan = RnnPlan(cfg, stages, max_rows=rows, max_utts=n_utts)
    feats = torch.from_numpy(x).cuda()
    normh = PN.cmvn_norm(stats_of(x), norm_vars=True)
    norm = torch.from_numpy(normh).cuda()
    out = torch.empty((rows, CLASSES), dtype=torch.float32, device="cuda")

    def native():
        return plan.compute(feats, lens, norm=norm, norm_vars=True, out=out)

    res = dict(bench="gru_throughput", utts=n_utts, rows=rows, dims=plan.dims, kinds=plan.kinds, reps=reps, calls=calls,
               device=torch.cuda.get_device_name(0), group_utts=plan.group_utts, groups=-(-n_utts // GU),
               scan_lds_bytes=plan.lds_bytes, workspace_bytes=plan.workspace_bytes)
    res["native"] = time_calls(native, reps, calls)
    ms = res["native"]["ms"]
    res["frames_per_s"] = round(rows / ms * 1e3)
    res["audio_hours_per_s"] = round(rows / FPS / 3600 / ms * 1e3, 3)
    plan.set_profiling(True)
    for _ in range(calls):
        native()
    proj, scan = plan.times()
    plan.set_profiling(False)
    res["projection_ms"], res["scan_ms"] = round(proj / calls, 3), round(scan / calls, 3)
    fl = scan_flops(lens, stages)
    res["scan_executed_gflop"] = round(fl / 1e9, 2)
    res["scan_fraction_of_f32_mfma_peak"] = round(fl / (scan / calls * 1e-3) / (PEAK_TFLOPS * 1e12), 4)
    if cpu:
        ends = np.cumsum(lens)
        per = [PN.post(x[e - n:e], normh, True, 0, 2, 0, CTX, CTX) for e, n in zip(ends, lens)]
        sec, ref, order = torch_cpu(stages, per)
        res["torch_cpu"] = dict(threads=CPU_THREADS, ms=round(sec * 1e3, 1), frames_per_s=round(rows / sec),
                                audio_hours_per_s=round(rows / FPS / 3600 / sec, 4))
        res["speedup_vs_torch_cpu"] = round(sec * 1e3 / ms, 1)
        got = out.cpu().numpy()
        res["max_abs_diff_native_torch_cpu"] = float(max(
            np.abs(got[ends[u] - lens[u]:ends[u]] - ref[k, :lens[u]].numpy()).max() for k, u in enumerate(order)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_throughput.jsonl"))
    ap.add_argument("--one", type=int, default=0, help="(internal) run the step with this many utterances")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.one:
        print(json.dumps(step(args.one, args.reps, args.calls, cpu=args.one <= 64)))
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for n in (64, 2048):
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
