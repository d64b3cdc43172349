#!/usr/bin/env python3
"""Throughput of one batch of compute-lifelong-likelihood on the device, resident in HBM: D = 3 of the README's GRU
model (13 x 9 -> 3 GRU x 256 -> 1936 classes, global CMVN with variances, splice -4..+4) in mode softmax, then what
speech_recognition_tools_amd/lifelong.py runs after the logits, for task_prior `mm` (mmeasure_kernel, the host's
weights, lifelong_fuse_kernel) and `dp` (per model: an encoder plan 117 -> 2 GRU x 256 -> [means; vars] of bn 30,
vae_sample_kernel, a decoder plan 30 -> 1 GRU x 256 -> 117, vae_elbo_kernel against the spliced rows; then the
weights and the fusion).  2048 utterances of U(2, 8) s at 100 frames/s, seeded; weights are torch's default init range
times 3 (the VAEs' times 1).  Reported, not gated: there is no target number.

Reported per task_prior: the step's time (median of --reps steps between two device events, the one copy-back and
the host's weights included), HIP-event times per kernel family in one further step, the new kernels' share of the
step, and for mmeasure_kernel the achieved rate against its one-read floor of D rows C 4 bytes.

    python benchmarks/lifelong_throughput.py [--reps 5] [--out profiles/lifelong_throughput.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

D, DIM, CTX, HIDDEN, LAYERS, CLASSES, BN = 3, 13, 4, 256, 3, 1936, 30
FPS, HBM_TBS = 100, 8.0   # HBM3E peak of the MI355X data sheet, TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--utts", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lifelong_throughput.jsonl"))
    args = ap.parse_args()
    import post_numpy as PN
    import torch
    from speech_recognition_tools_amd import lifelong as L
    from speech_recognition_tools_amd.post import PostConfig, PostPlan
    from speech_recognition_tools_amd.rnn import RnnPlan
    from test_rnn import make_stages
    from xform_throughput import stats_of
    rng = np.random.default_rng(2026)
    K = DIM * (2 * CTX + 1)
    cls = [make_stages(rng, K, [("gru", HIDDEN)] * LAYERS + [("linear", CLASSES)], 3.0) for _ in range(D)]
    enc = [make_stages(rng, K, [("gru", HIDDEN)] * 2 + [("linear", 2 * BN)], 1.0) for _ in range(D)]
    dec = [make_stages(rng, BN, [("gru", HIDDEN), ("linear", K)], 1.0) for _ in range(D)]
    lens = [int(v) for v in rng.integers(2 * FPS, 8 * FPS + 1, args.utts)]
    rows, U = sum(lens), len(lens)
    x = np.round(rng.standard_normal((rows, DIM)) * 3.0 + 1.0, 3).astype(np.float32)
    dev = torch.device("cuda", 0)
    cfg = PostConfig(dim=DIM, left_context=CTX, right_context=CTX)
    mk = dict(max_rows=rows, max_utts=U)
    cls_p = [RnnPlan(cfg, s, **mk) for s in cls]
    enc_p = [RnnPlan(cfg, s, **mk) for s in enc]
    dec_p = [RnnPlan(PostConfig(dim=BN), s, **mk) for s in dec]
    post_p = PostPlan(cfg, 0)
    feats = torch.from_numpy(x).to(dev)
    norm = torch.from_numpy(PN.cmvn_norm(stats_of(x), norm_vars=True)).to(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    P = torch.empty((D, rows, CLASSES), **f32)
    out = torch.empty((rows, CLASSES), **f32)
    X, XH, ML, Z = (torch.empty((rows, n), **f32) for n in (K, K, 2 * BN, BN))
    ELBO = torch.empty((rows,), **f32)
    eps = [torch.randn((rows, BN), generator=torch.Generator().manual_seed(i)).to(dev) for i in range(D)]
    priors = np.log(rng.dirichlet(np.ones(CLASSES) * 5.0, D))
    tab = torch.from_numpy(np.exp(priors)).to(dev)
    tables = L.utt_tables(lens, dev)
    chain = dict(norm=norm, norm_vars=True)
    ev = []

    def timed(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        ev.append((name, a, b))
        return r

    def step(kind):
        for i in range(D):
            timed("classifiers", lambda: cls_p[i].compute(feats, lens, mode="softmax", out=P[i], **chain))
        both = torch.full((2, U, D), float("nan"), dtype=torch.float64, device=dev)
        if kind == "mm":
            timed("mmeasure_kernel", lambda: L.mmeasure(P, tables, out=both[0]))
        else:
            timed("post_kernel", lambda: post_p.compute(feats, lens, out=X, **chain))
            for i in range(D):
                timed("vae_plans", lambda: enc_p[i].compute(feats, lens, out=ML, **chain))
                timed("vae_sample_kernel", lambda: L.vae_sample(ML, eps[i], out=Z))
                timed("vae_plans", lambda: dec_p[i].compute(Z, lens, out=XH))
                timed("vae_elbo_kernel", lambda: L.vae_elbo(X, XH, ML, tables, "lifelong", out=both[1, :, i], elbo=ELBO))
        host = both.cpu().numpy()
        w = np.stack([L.task_weights("lifelong", kind, host[0, u], host[1, u]) for u in range(U)])
        wd = torch.from_numpy(w).to(dev)
        timed("lifelong_fuse_kernel", lambda: L.fuse(P, tables, max(lens), wd, tab, 0.8, "lifelong", out=out))
        return w

    res = dict(bench="lifelong_throughput", D=D, utts=U, rows=rows, classes=CLASSES, reps=args.reps,
               device=torch.cuda.get_device_name(0))
    new = ("mmeasure_kernel", "vae_sample_kernel", "vae_elbo_kernel", "lifelong_fuse_kernel")
    for kind in ("mm", "dp"):
        step(kind)                                                    # warm-up: code objects, the pool's first blocks
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            w = step(kind)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        ev.clear()
        step(kind)
        torch.cuda.synchronize()
        fam = {}
        for name, a, b in ev:
            fam[name] = fam.get(name, 0.0) + a.elapsed_time(b)
        ev.clear()
        med = float(np.median(ms))
        r = dict(step_ms=round(med, 2), step_ms_min=round(min(ms), 2), step_ms_max=round(max(ms), 2),
                 frames_per_s=round(rows / med * 1e3), audio_hours_per_s=round(rows / FPS / 3600 / med * 1e3, 3),
                 kernel_ms={k: round(v, 3) for k, v in fam.items()},
                 new_kernels_share_of_step=round(sum(fam.get(k, 0.0) for k in new) / med, 4),
                 nan_weight_rows=int(np.isnan(w).any(1).sum()))
        if kind == "mm":
            floor_bytes = D * rows * CLASSES * 4
            r["mmeasure_floor_bytes"] = floor_bytes
            r["mmeasure_tb_per_s"] = round(floor_bytes / (fam["mmeasure_kernel"] * 1e-3) / 1e12, 3)
            r["mmeasure_fraction_of_hbm_peak"] = round(r["mmeasure_tb_per_s"] / HBM_TBS, 4)
        res[kind] = r
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
