#!/usr/bin/env python3
"""Throughput of the VAE-encoded GRU model after the chain (fdlp_venc_compute: the convolutions in
conv2d_same_kernel, `means` and the projections in dense_kernel, the normaliser in utt_norm_kernel, the scans in
gru_scan_kernel) on a batch resident in HBM, next to the same model as torch modules on 16 CPU threads, one utterance
at a time, which is how the reference's compute_vae_encoded_likelihood.py runs it.  Reported, not gated: there is no
target number.

Workload: the CNN trainer's default encoder 1 -> 32 -> 64 -> 128, kernel (3, 5), on 13 columns, bn 30, then 3 GRU x
256 -> 1936 classes, global CMVN with variances, 2048 utterances of U(2, 8) s at 100 frames/s, seeded; weights are
torch's default init range times 3.

Reported: frames/s and audio-hours/s of the whole compute (median of --reps windows of --calls calls between two
device events, after warm-up calls); the HIP-event times of the convolutions, of the scans and of the rest
(fdlp_venc_set_profiling); the convolutions' share of the time and their fraction of the float32 MFMA peak
(157.3 TFLOP/s) on the model's 2 x 13 x 15 x (1 x 32 + 32 x 64 + 64 x 128) = 4.0 MFLOP per frame; and the CPU side on
the first --cpu-utts utterances of the same batch.

    python benchmarks/vaeenc_throughput.py [--reps 5] [--calls 2] [--out profiles/vaeenc_throughput.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

DIM, CHANNELS, KERNEL, BN, HIDDEN, CLS, CLASSES = 13, [1, 32, 64, 128], (3, 5), 30, 256, 3, 1936
FPS, PEAK_TFLOPS, CPU_THREADS = 100, 157.3, 16


def model(rng):
    from test_vaeenc import make_vstages
    return make_vstages(rng, "cnn", DIM, (CHANNELS, KERNEL), BN, [("gru", HIDDEN)] * CLS + [("linear", CLASSES)])


def conv_flop_per_frame():
    kh, kw = KERNEL
    return 2 * DIM * kh * kw * sum(ci * co for ci, co in zip(CHANNELS[:-1], CHANNELS[1:]))


def torch_cpu(stages, rows_per_utt):
    """the reference's way: per utterance, Conv2d + ReLU layers on the [1, 1, F, T] image, means, the normaliser
    (mean, then unbiased variance over time), nn.GRU layers and the regression"""
    import torch
    torch.set_num_threads(CPU_THREADS)
    mods = []
    for st in stages:
        if st[0] == "conv":
            co, ci, kh, kw = st[1].shape
            m = torch.nn.Conv2d(ci, co, (kh, kw), padding=((kh - 1) // 2, (kw - 1) // 2))
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(st[1]))
                m.bias.copy_(torch.from_numpy(st[2]))
            mods.append(("conv", m.eval()))
        elif st[0] == "gru":
            g = torch.nn.GRU(st[1].shape[1], st[2].shape[1], batch_first=True)
            with torch.no_grad():
                for p, a in zip((g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0), st[1:]):
                    p.copy_(torch.from_numpy(a))
            mods.append(("gru", g.eval()))
        elif st[0] == "norm":
            mods.append(("norm", None))
        else:
            mods.append(("linear", (torch.from_numpy(st[1]), torch.from_numpy(st[2]))))

    def run():
        outs = []
        with torch.no_grad():
            for rows in rows_per_utt:
                h = torch.transpose(torch.from_numpy(rows)[None, None, :, :], 2, 3)
                for kind, m in mods:
                    if kind == "conv":
                        h = torch.relu(m(h))
                    elif kind == "linear":
                        if h.dim() == 4:
                            h = torch.transpose(h.reshape(1, -1, h.shape[3]), 1, 2)
                        h = torch.nn.functional.linear(h, m[0], m[1])
                    elif kind == "norm":
                        h = h - torch.mean(h, dim=1, keepdim=True)
                        h = h / torch.sqrt(torch.var(h, dim=1, keepdim=True))
                    else:
                        h, _ = m(h)
                outs.append(h[0])
        return outs

    run()
    t0 = time.perf_counter()
    outs = run()
    return time.perf_counter() - t0, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--utts", type=int, default=2048)
    ap.add_argument("--cpu-utts", type=int, default=32, help="utterances of the batch the CPU side runs (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vaeenc_throughput.jsonl"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import post_numpy as PN
    import torch
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.vaeenc import VaeEncPlan
    from xform_throughput import stats_of, time_calls
    rng = np.random.default_rng(2026)
    stages = model(rng)
    n_utts = args.utts
    lens = [int(v) for v in rng.integers(2 * FPS, 8 * FPS + 1, n_utts)]
    rows = sum(lens)
    x = np.round(rng.standard_normal((rows, DIM)) * 3.0 + 1.0, 3).astype(np.float32)
    plan = VaeEncPlan(PostConfig(dim=DIM), stages, max_rows=rows, max_utts=n_utts)
    feats = torch.from_numpy(x).cuda()
    normh = PN.cmvn_norm(stats_of(x), norm_vars=True)
    norm = torch.from_numpy(normh).cuda()
    out = torch.empty((rows, CLASSES), dtype=torch.float32, device="cuda")

    def native():
        return plan.compute(feats, lens, norm=norm, norm_vars=True, out=out)

    res = dict(bench="vaeenc_throughput", utts=n_utts, rows=rows, dims=plan.dims, kinds=plan.kinds, reps=args.reps,
               calls=args.calls, device=torch.cuda.get_device_name(0), scan_lds_bytes=plan.lds_bytes[0],
               conv_lds_bytes=plan.lds_bytes[1], workspace_bytes=plan.workspace_bytes)
    res["native"] = time_calls(native, args.reps, args.calls)
    ms = res["native"]["ms"]
    res["frames_per_s"] = round(rows / ms * 1e3)
    res["audio_hours_per_s"] = round(rows / FPS / 3600 / ms * 1e3, 3)
    plan.set_profiling(True)
    for _ in range(args.calls):
        native()
    other, scan, conv = (t / args.calls for t in plan.times())
    plan.set_profiling(False)
    res["conv_ms"], res["scan_ms"], res["other_ms"] = round(conv, 3), round(scan, 3), round(other, 3)
    res["conv_share_of_time"] = round(conv / (conv + scan + other), 4)
    fl = conv_flop_per_frame()
    res["conv_mflop_per_frame"] = round(fl / 1e6, 3)
    res["conv_fraction_of_f32_mfma_peak"] = round(fl * rows / (conv * 1e-3) / (PEAK_TFLOPS * 1e12), 4)
    if args.cpu_utts > 0:
        n = min(args.cpu_utts, n_utts)
        ends = np.cumsum(lens)
        per = [PN.post(x[e - t:e], normh, True, 0, 2, 0, 0, 0) for e, t in zip(ends[:n], lens[:n])]
        sec, ref = torch_cpu(stages, per)
        crows = int(ends[n - 1])
        res["torch_cpu"] = dict(threads=CPU_THREADS, utts=n, rows=crows, ms=round(sec * 1e3, 1),
                                frames_per_s=round(crows / sec), audio_hours_per_s=round(crows / FPS / 3600 / sec, 4))
        res["speedup_vs_torch_cpu"] = round((rows / ms * 1e3) / (crows / sec), 1)   # frames/s over frames/s
        got = out[:crows].cpu().numpy()
        res["max_abs_diff_native_torch_cpu"] = float(max(
            np.abs(got[ends[u] - lens[u]:ends[u]] - ref[u].numpy()).max() for u in range(n)))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
