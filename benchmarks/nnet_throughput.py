#!/usr/bin/env python3
"""Throughput of the feed-forward network after the chain (fdlp_nnet_compute: layer 0 in the chain's launch, one
dense_kernel launch per further layer) on a batch resident in HBM, next to what the parent commit can do for the
same result: the plain PostPlan writing the spliced rows to HBM, then a chain of torch.nn.functional.linear + relu
on the device, timed with the same events.

Workload: the recipe's model (recipes/timit/run_hybrid_mvector.sh), 13 columns -> +-4 context (117) -> 4 x 512 -> 38,
global CMVN (means only), 2^18 rows in utterances of 200, weights drawn from a seeded normal over sqrt(K).

Reported: the whole chain; the network cut after each layer (tap), whose increments are the layers' own times --
`dense_512x512` is the mean increment of the three 512 -> 512 layers -- next to torch's linear(relu(x)) on a
[2^18, 512] tensor alone; each also as a fraction of the float32 MFMA floor, sum over layers of
ceil(K / 4) * ceil(N / 16) v_mfma_f32_16x16x4_f32 of 32 cycles per 16 rows on 1024 SIMDs at 2.4 GHz (the clock
DESIGN.md section 7d uses).

Timing: warm-up calls, then `--reps` (>= 5) windows of `--calls` calls between two device events; the median
window is reported with its range.  One JSON line is printed and appended to --out.

    python benchmarks/nnet_throughput.py [--reps 7] [--calls 5] [--out profiles/nnet_throughput.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from xform_throughput import stats_of, time_calls  # noqa: E402

ROWS, UTT = 1 << 18, 200
DIM, CTX, HIDDEN, LAYERS, CLASSES = 13, 4, 512, 4, 38


def mfma_floor_ms(rows, pairs):
    n = sum(-(-k // 4) * -(-n // 16) for k, n in pairs) * (rows // 16)
    return n * 32 / 1024 / 2.4e6     # 1024 SIMDs at 2.4 GHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nnet_throughput.jsonl"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import post_numpy as PN
    import torch
    import torch.nn.functional as F
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig, PostPlan
    lens = [UTT] * (ROWS // UTT) + ([ROWS % UTT] if ROWS % UTT else [])
    K0 = DIM * (2 * CTX + 1)
    dims = [K0] + [HIDDEN] * LAYERS + [CLASSES]
    pairs = list(zip(dims[:-1], dims[1:]))
    rng = np.random.default_rng(2026)
    x = np.round(rng.standard_normal((ROWS, DIM)) * 3.0 + 1.0, 3).astype(np.float32)
    ws = [(rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32) for k, n in pairs]
    bs = [(rng.standard_normal(n) * 0.5).astype(np.float32) for _, n in pairs]
    cfg = PostConfig(dim=DIM, left_context=CTX, right_context=CTX)
    plan = NnetPlan(cfg, ws, bs, max_rows=ROWS)
    feats = torch.from_numpy(x).cuda()
    norm = torch.from_numpy(PN.cmvn_norm(stats_of(x), norm_vars=False)).cuda()
    res = dict(bench="nnet_throughput", rows=ROWS, utts=len(lens), utt_frames=UTT, dims=dims, reps=args.reps,
               calls=args.calls, device=torch.cuda.get_device_name(0), dense_tile=list(plan.tile),
               dense_lds_bytes=plan.lds_bytes, workspace_bytes=plan.workspace_bytes)
    n = len(pairs)
    outs = [torch.empty((ROWS, plan.tap_dim(t)), dtype=torch.float32, device="cuda") for t in range(n)]

    def native(tap):
        return lambda: plan.compute(feats, lens, norm=norm, norm_vars=False, tap=tap, out=outs[tap])

    res["native"] = time_calls(native(0), args.reps, args.calls)
    res["native"]["rows_per_s"] = round(ROWS / res["native"]["ms"] * 1e3)
    got = outs[0].clone()
    # the network cut after layer l (tap n - 1 - l): the increments are the layers' own times
    upto = [time_calls(native(n - 1 - l), args.reps, args.calls)["ms"] for l in range(n)]
    res["native_up_to_layer_ms"] = upto
    res["native_layer_ms"] = [round(upto[0], 4)] + [round(upto[l] - upto[l - 1], 4) for l in range(1, n)]
    mid = [res["native_layer_ms"][l] for l in range(1, n) if pairs[l] == (HIDDEN, HIDDEN)]
    res["dense_512x512"] = dict(ms=round(float(np.mean(mid)), 4), layers=len(mid))

    # the parent's way to the same result: spliced rows to HBM, then torch
    post = PostPlan(cfg)
    rows = torch.empty((ROWS, K0), dtype=torch.float32, device="cuda")
    Wd = [torch.from_numpy(w).cuda() for w in ws]
    bd = [torch.from_numpy(b).cuda() for b in bs]

    def baseline():
        post.compute(feats, lens, norm=norm, norm_vars=False, out=rows)
        h = F.linear(rows, Wd[0], bd[0])
        for W, b in zip(Wd[1:], bd[1:]):
            h = F.linear(F.relu(h), W, b)
        return h

    res["torch_chain"] = time_calls(baseline, args.reps, args.calls)
    res["torch_chain"]["rows_per_s"] = round(ROWS / res["torch_chain"]["ms"] * 1e3)
    res["post_only"] = time_calls(lambda: post.compute(feats, lens, norm=norm, norm_vars=False, out=rows), args.reps,
                                  args.calls)
    ref = baseline()
    res["max_abs_diff_native_torch"] = float((got - ref).abs().max())
    hid = torch.empty((ROWS, HIDDEN), dtype=torch.float32, device="cuda").normal_()
    res["torch_linear_relu_512x512"] = time_calls(lambda: F.linear(F.relu(hid), Wd[1], bd[1]), args.reps, args.calls)
    res["torch_linear_512x512"] = time_calls(lambda: F.linear(hid, Wd[1], bd[1]), args.reps, args.calls)
    res["native_speedup_vs_torch_chain"] = round(res["torch_chain"]["ms"] / res["native"]["ms"], 3)
    res["dense_speedup_vs_torch_linear_relu"] = round(res["torch_linear_relu_512x512"]["ms"] / res["dense_512x512"]["ms"], 3)
    res["mfma_floor_ms"] = round(mfma_floor_ms(ROWS, pairs), 4)
    res["mfma_floor_512x512_ms"] = round(mfma_floor_ms(ROWS, [(HIDDEN, HIDDEN)]), 4)
    res["native_fraction_of_mfma_floor"] = round(res["mfma_floor_ms"] / res["native"]["ms"], 3)
    res["torch_chain_fraction_of_mfma_floor"] = round(res["mfma_floor_ms"] / res["torch_chain"]["ms"], 3)
    res["dense_fraction_of_mfma_floor"] = round(res["mfma_floor_512x512_ms"] / res["dense_512x512"]["ms"], 3)
    res["torch_linear_relu_fraction_of_mfma_floor"] = round(
        res["mfma_floor_512x512_ms"] / res["torch_linear_relu_512x512"]["ms"], 3)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
