#!/usr/bin/env python3
"""Throughput of the fused cmvn | deltas | splice | transform-feats launch (fdlp_xform_compute) on a batch resident
in HBM, next to what the same result costs without it: the plain PostPlan writing the spliced rows to HBM, then
torch.matmul (plus the offset add) on those rows.

Workload: 2^20 frames in utterances of 200 frames, one global CMVN pair with variance normalisation, one global
matrix drawn from a seeded normal over sqrt(K).  Two shapes:
    lda13   13 columns, delta order 2, +-4 context (K = 351) -> 40, affine
    lda80   80 columns, +-4 context (K = 720) -> 40, linear
The HBM floor of the fused launch is 4 (D + N) bytes per row, every input row read once and every output row written
once; its fraction is taken against a device-to-device copy of that many bytes timed in the same run (read half,
write half).  The two-step form moves 4 (D + 2 K + N) bytes per row.  The MFMA floor is ceil(K / 4) * ceil(N / 16)
v_mfma_f32_16x16x4_f32 (32 cycles each on one of 1024 SIMDs) per 16 rows.

Timing: warm-up calls, then `--reps` (>= 5) windows of `--calls` calls between two device events; the median
window is reported with its range.  One JSON line is printed and appended to --out.

    python benchmarks/xform_throughput.py [--reps 7] [--calls 5] [--utt-frames 200] [--out profiles/xform_throughput.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES, UTT = 1 << 20, 200
SHAPES = {"lda13": dict(dim=13, cfg=dict(delta_order=2, left_context=4, right_context=4), out_dim=40, affine=True),
          "lda80": dict(dim=80, cfg=dict(left_context=4, right_context=4), out_dim=40, affine=False)}


def stats_of(x):
    st = np.zeros((2, x.shape[1] + 1))
    st[0, :-1] = x.astype(np.float64).sum(0)
    st[1, :-1] = (x.astype(np.float64) ** 2).sum(0)
    st[0, -1] = x.shape[0]
    return st


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
    return dict(ms=round(float(np.median(ms)), 4), ms_min=round(float(min(ms)), 4), ms_max=round(float(max(ms)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--utt-frames", type=int, default=UTT, help="frames per utterance (256: every tile is full)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xform_throughput.jsonl"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import post_numpy as PN
    import torch
    from speech_recognition_tools_amd.post import PostConfig, PostPlan, XformPlan
    utt = args.utt_frames
    lens = [utt] * (FRAMES // utt) + ([FRAMES % utt] if FRAMES % utt else [])
    res = dict(bench="xform_throughput", frames=FRAMES, utts=len(lens), utt_frames=utt, reps=args.reps,
               calls=args.calls, device=torch.cuda.get_device_name(0))
    rng = np.random.default_rng(2026)
    for name, sh in SHAPES.items():
        D, N, affine = sh["dim"], sh["out_dim"], sh["affine"]
        x = np.round(rng.standard_normal((FRAMES, D)) * 3.0 + 1.0, 3).astype(np.float32)
        cfg = PostConfig(dim=D, **sh["cfg"])
        fused = XformPlan(cfg, N, affine)
        K = fused.in_dim
        M = (rng.standard_normal((N, K + int(affine))) / np.sqrt(K)).astype(np.float32)
        feats = torch.from_numpy(x).cuda()
        norm = torch.from_numpy(PN.cmvn_norm(stats_of(x), norm_vars=True)).cuda()
        Md = torch.from_numpy(M).cuda()
        out = torch.empty((FRAMES, N), dtype=torch.float32, device="cuda")
        floor_bytes = FRAMES * 4 * (D + N)
        r = dict(dim=D, K=K, out_dim=N, affine=affine, tile_frames=fused.tile, lds_bytes=fused.lds_bytes,
                 floor_bytes=floor_bytes, two_step_bytes=FRAMES * 4 * (D + 2 * K + N))
        r["fused"] = time_calls(lambda: fused.compute(feats, lens, Md, norm=norm, out=out), args.reps, args.calls)
        r["fused"]["rows_per_s"] = round(FRAMES / r["fused"]["ms"] * 1e3)
        got = out.clone()
        # the parent's way to the same result: spliced rows to HBM, then the product
        post = PostPlan(cfg)
        rows = torch.empty((FRAMES, K), dtype=torch.float32, device="cuda")
        Wt = Md[:, :K].T.contiguous()
        off = Md[:, K].contiguous() if affine else None

        def two_step():
            post.compute(feats, lens, norm=norm, out=rows)
            torch.matmul(rows, Wt, out=out)
            if affine:
                out.add_(off)
        r["two_step"] = time_calls(two_step, args.reps, args.calls)
        r["two_step"]["rows_per_s"] = round(FRAMES / r["two_step"]["ms"] * 1e3)
        r["post_only"] = time_calls(lambda: post.compute(feats, lens, norm=norm, out=rows), args.reps, args.calls)
        r["max_abs_diff_fused_two_step"] = float((got - out).abs().max())
        r["fused_speedup_vs_two_step"] = round(r["two_step"]["ms"] / r["fused"]["ms"], 2)
        # a device-to-device copy moving the floor's traffic, in the same run
        src = torch.empty(floor_bytes // 8, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        r["copy_floor"] = time_calls(lambda: dst.copy_(src), args.reps, args.calls)
        r["fused_fraction_of_hbm_floor"] = round(r["copy_floor"]["ms"] / r["fused"]["ms"], 3)
        mfma = -(-K // 4) * -(-N // 16) * (FRAMES // 16)
        r["mfma_floor_ms"] = round(mfma * 32 / 1024 / 2.4e6, 4)     # 1024 SIMDs at 2.4 GHz
        r["fused_fraction_of_mfma_floor"] = round(r["mfma_floor_ms"] / r["fused"]["ms"], 3)
        res[name] = r
        del src, dst, rows, out, got, feats, fused, post
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
