#!/usr/bin/env python3
"""Throughput of the MFCC kernel (fdlp_mfcc_compute) on a resident batch, next to the mel kernel on the same
batch and a numpy/scipy CPU restatement of the reference's per-frame chain on 16 processes.

Workload: 65,536 frames of seeded 4 s utterances (163 x 400 frames + one shorter tail), int16 PCM resident in
HBM, reference defaults (30 filters, 20 ms frames, 100 Hz, nfft 1024 -> a 513-point DFT).  Warm-up calls, then
`--reps` timed windows of `--calls` calls each between two device events; the median window is reported with
the spread.  Prints one JSON line.

    python benchmarks/mfcc_throughput.py [--reps 7] [--calls 20] [--cpu_utts 64]

Stage ablation: build a variant library with a stage of mfcc_kernel removed and time it through FDLP_LIB,
    python speech_recognition_tools_amd/_build.py --out /tmp/libfdlp_nogather.so -DFDLP_MFCC_SKIP=1   (2: no MFMA loop)
    FDLP_LIB=/tmp/libfdlp_nogather.so python benchmarks/mfcc_throughput.py --cpu_utts 0
(the variant's outputs are wrong on purpose; only its time means anything).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SRATE, HOP, L, NFFT, NFILT = 16000, 160, 320, 1024, 30
FRAMES = 65536
MFMA_F64_SPEC_TFLOPS = 78.6  # MI355X fp64 matrix peak (spec sheet)


def make_batch():
    rng = np.random.default_rng(2024)
    per = (4 * SRATE - 2) // HOP + 1                      # frames of a 4 s utterance
    n_full = FRAMES // per
    tail = FRAMES - n_full * per
    lens = [4 * SRATE] * n_full + ([HOP * (tail - 1) + 50] if tail else [])
    pcm = np.clip(np.round(rng.standard_normal(sum(lens)) * 2000), -32768, 32767).astype(np.int16)
    return pcm, lens


def _cpu_tables():
    n = NFFT // 2 + 1
    mel_max = 2595 * np.log10(1 + SRATE / 1400)
    fw = np.linspace(0, mel_max, NFILT + 2)
    fb = np.zeros((NFILT, n))
    edge = np.floor((NFFT + 1) * (700 * (10 ** (fw / 2595) - 1)) / SRATE)
    for m in range(1, NFILT + 1):
        a, c, r = int(edge[m - 1]), int(edge[m]), int(edge[m + 1])
        for k in range(a, c):
            fb[m - 1, k] = (k - edge[m - 1]) / (edge[m] - edge[m - 1])
        for k in range(c, r):
            fb[m - 1, k] = (edge[m + 1] - k) / (edge[m + 1] - edge[m])
    return n, fb


def cpu_utterance(x):
    """getFrames + |fft(frame, 513)| @ fbank.T, log10, dct[:, :13] of one utterance (reference items 4-6)."""
    from scipy.fftpack import dct, fft
    n, fb = _cpu_tables()
    sig = np.pad(x / 2.0 ** 15, L // 2 - 1, "reflect")
    F = (x.size - 2) // HOP + 1
    idx = np.arange(F)[:, None] * HOP + np.arange(L)[None, :]
    fr = sig[idx] * np.hamming(L)
    mel = np.log10(np.abs(fft(fr, n, axis=1)) @ fb.T)
    return dct(mel, axis=1)[:, :13].shape[0]


def cpu_rate(pcm, lens, n_utts, procs=16):
    import multiprocessing as mp
    offs = np.concatenate([[0], np.cumsum(lens)])
    utts = [pcm[offs[i]:offs[i + 1]] for i in range(min(n_utts, len(lens)))]
    with mp.get_context("spawn").Pool(procs) as pool:
        pool.map(cpu_utterance, utts[:procs])             # start the workers, import scipy
        t0 = time.perf_counter()
        frames = sum(pool.map(cpu_utterance, utts, chunksize=1))
        dt = time.perf_counter() - t0
    return frames / dt, frames


def time_calls(fn, reps, calls, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--cpu_utts", type=int, default=64)
    args = ap.parse_args()
    pcm, lens = make_batch()
    # before the GPU is opened: the workers never touch it
    cpu_fps, cpu_frames = cpu_rate(pcm, lens, args.cpu_utts) if args.cpu_utts > 0 else (None, 0)
    variant = os.environ.get("FDLP_LIB")

    import torch
    from speech_recognition_tools_amd.melspec import MelConfig, MelPlan
    from speech_recognition_tools_amd.mfcc import MfccConfig, MfccPlan
    dev_pcm = torch.from_numpy(pcm).cuda()
    audio_s = sum(lens) / SRATE
    res = dict(bench="mfcc_throughput", frames=FRAMES, utts=len(lens), audio_seconds=audio_s, reps=args.reps,
               calls=args.calls, device=torch.cuda.get_device_name(0))
    if variant:
        res["variant_lib"] = os.path.basename(variant)
    plans = {"mfcc": MfccPlan(MfccConfig(), device=0, max_frames=FRAMES),
             "mfcc_context3": MfccPlan(MfccConfig(context=3), device=0, max_frames=FRAMES),
             "mel": MelPlan(MelConfig(), device=0, max_frames=FRAMES)}
    t = plans["mfcc"].tables()
    res["tile_frames"] = t["tile"]
    for name, plan in plans.items():
        out, rows, _ = plan.compute(dev_pcm, lens)
        assert int(rows[-1]) == FRAMES and (variant or bool(torch.isfinite(out).all()))
        med, lo, hi = time_calls(lambda: plan.compute(dev_pcm, lens), args.reps, args.calls)
        res[name] = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                         frames_per_s=round(FRAMES / med * 1e3), audio_hours_per_s=round(audio_s / 3600 / med * 1e3, 3))
    # useful DFT work: Re and Im of K x nb bins per frame, 2 FLOP per FMA; issued: the padded tiles
    useful = 4.0 * t["K"] * t["nb"] * FRAMES
    issued = 4.0 * t["Kpad"] * t["nbpad"] * FRAMES
    s = res["mfcc"]["ms"] * 1e-3
    res["dft_useful_tflops"] = round(useful / s / 1e12, 2)
    res["dft_issued_tflops"] = round(issued / s / 1e12, 2)
    res["fraction_of_fp64_mfma_spec_peak"] = round(useful / s / 1e12 / MFMA_F64_SPEC_TFLOPS, 3)
    if cpu_fps:
        res["cpu_restatement_16proc"] = dict(frames=cpu_frames, frames_per_s=round(cpu_fps),
                                             audio_hours_per_s=round(cpu_fps / 100 / 3600, 3))
        res["speedup_vs_cpu_16proc"] = round(res["mfcc"]["frames_per_s"] / cpu_fps, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
