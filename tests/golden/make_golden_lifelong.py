"""Golden fixtures of the multi-domain tools (tests/test_lifelong.py), produced by the REAL reference classes
src/nnet/nnet_models.py nnetRNN and nnetVAE and the REAL functions mmeasure_loss, sym_kld and vae_loss of
src/nnet/compute_lifelong_likelihood.py (imported from the reference checkout at generation time only; kaldi_io and
the reference's `features` module, which that script imports and these functions do not use, are stubbed in
sys.modules), on torch's CPU path, doing what the loops of compute_lifelong_likelihood.py:127-201 and
compute_incremental_likelihood.py:125-187 do, in this project's own code.

  lifelong_models       D = 3 pairs: 7 columns, cmvn with vars, splice -1..+1 (21) -> 2 GRU x 33 -> 10 classes, and
                        nnetVAE 21 -> 2 GRU x 33 -> bn 11 -> 1 GRU x 33 -> 21; three log priors; the CMVN stats;
                        utterances of 1, 65, 66, 67 and 131 frames; the sampler's noise eps<i>_<utt> [T, 11], drawn
                        per utterance in order and per model in order from torch's default generator
  lifelong_mm           task_prior mm, and the same with --stream_selection (keys sel_*)
  lifelong_dp           task_prior dp
  lifelong_lowent       task_prior lowent
  lifelong_fixed        task_prior 0.5,0.0,1.5
  lifelong_incremental  compute_incremental_likelihood.py, task_prior lowent
As in make_golden_rnn.py every `weight*` tensor of the freshly initialised classifiers is multiplied by 3.  The VAEs
keep torch's initialisation: the reference's dp weights are exp(300 p(x)) / sum, which is 0 / 0 once every p(x) lies
below -2.48, and VAEs with tripled weights reconstruct badly enough (p(x) of -3 to -5) for every dp output to be NaN.

Per utterance a result file stores mm_ and px_ [3] (float64 run; NaN where the reference has NaN; px_ only where the
kind uses it here, mm_ likewise), w_ the weights, out64_ and out32_ the float64 and float32 runs' outputs and
text3_ the float32 output as a '%.3f' text ark holds it.  The float64 run is the same loop on .double() models and
float64 rows with the SAME float32 noise; mmeasure_loss accumulates into a FloatTensor, so the float64 M-measure is
the same expression, sum_d (sym_kld + KLDivLoss) / 4, on the script's own functions without that accumulator.

A fixture is REFUSED unless the reference's own float32 run lies within LIMITS of its float64 run, separately at the
M-measure, at p(x), at the weights and at the output (meta d32_mm, d32_px, d32_w, d32_out), the NaN patterns of the two
runs agree, and no near-tie decides anything: 1e-3 between the two largest values an argmax picks from and between the
two entropies lowent compares.  dp and lowent weights amplify p(x) by 200-500, so their output d32 can exceed what a
'%.3f' text is stable under: meta text_ok says whether the text may be asserted (d32_out <= 1e-4).

Run from the repository root:  python tests/golden/make_golden_lifelong.py
"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch
from scipy.stats import entropy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
from make_golden_nnet import text3  # noqa: E402
import post_numpy as PN  # noqa: E402

LIMITS = dict(mm=1e-4, px=1e-5, w=1e-2, out=1e-2)
MARGIN = 1e-3
LENS = (1, 65, 66, 67, 131)
D, FDIM, LEFT, RIGHT, LAYERS, HID, BN, NCLS = 3, 7, 1, 1, 2, 33, 11, 10


def reference():
    sys.path.insert(0, os.path.join(REF, "src/nnet"))
    for name in ("kaldi_io", "features"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.dict2Ark = None
            sys.modules[name] = m
    import compute_lifelong_likelihood as S
    import compute_incremental_likelihood as SI
    import inspect
    for fn in ("vae_loss", "sym_kld", "mmeasure_loss"):      # the two scripts carry the same functions
        assert inspect.getsource(getattr(S, fn)) == inspect.getsource(getattr(SI, fn)), fn
    from nnet_models import nnetRNN, nnetVAE
    return S, nnetRNN, nnetVAE


def mm64(S, X):
    kld = torch.nn.KLDivLoss()
    acc = 0
    for d in [5, 25, 45, 65]:
        acc = acc + S.sym_kld(X[d:, :], X[0:-d, :]) + kld(X[0:-d:, :], X[d:, :])
    return (acc / 4).item()


def run_utt(S, tool, kind, models, vaes, rows, eps, priors, pw, fixed, sel, dtype):
    """one pass of the script's loop body; eps[i]: the noise model i's sampler sees (torch.randn is replaced for its
    one call, so the float32 and the float64 run get the same values)"""
    mat = torch.from_numpy(np.asarray(rows)).to(dtype)[None, :, :]
    batch_l = torch.IntTensor([mat.size(1)])
    sm = torch.nn.Softmax(1)
    num_domains = len(models)
    px_save, all_pcx, all_tp, all_tp_2, mms = [], [], [], [], []
    with torch.no_grad():
        for idx, model in enumerate(models):
            out = model(mat, batch_l)
            real = torch.randn

            def fixed_randn(shape, _e=eps[idx]):
                assert tuple(shape) == (1,) + _e.shape
                return torch.from_numpy(_e)[None]

            torch.randn = fixed_randn      # the sampler's one call: it must see the stored noise in both precisions
            try:
                ae_out, latent_out = vaes[idx](mat, batch_l)
            finally:
                torch.randn = real
            latent_out = (latent_out[0][0, :, :], latent_out[1][0, :, :])
            px = S.vae_loss(mat[0, :, :], ae_out[0, :, :], latent_out).data.numpy()
            if tool == "incremental":
                px = np.exp(px)
            px_save.append(np.mean(px))
            pcx = sm(out[0, :, :])
            all_pcx.append(pcx.data.numpy())
            mm = S.mmeasure_loss(pcx).item() if dtype == torch.float32 else mm64(S, pcx)
            mms.append(mm)
            if kind == "mm":
                all_tp.append(mm)
            elif kind == "dp":
                all_tp.append(px_save[idx])
            elif kind == "lowent":
                all_tp.append(mm)
                all_tp_2.append(px_save[idx])
            else:
                all_tp.append(fixed[idx])
    margins = []
    with np.errstate(all="ignore"):
        k_dp = 300 if tool == "lifelong" else 500
        k_le = 300 if tool == "lifelong" else 200
        if kind == "mm":
            all_tp = np.asarray(all_tp, dtype=np.float64)
            if sel and tool == "lifelong":
                if not np.isnan(all_tp).any():
                    s = np.sort(all_tp)
                    margins.append(s[-1] - s[-2])
                temp = np.zeros(all_tp.shape)
                temp[np.argmax(all_tp)] = 1
                all_tp = temp
            else:
                all_tp = np.exp(all_tp) / np.sum(np.exp(all_tp))
            if np.isnan(all_tp[0]):
                all_tp = np.ones(num_domains) / num_domains
        elif kind == "dp":
            all_tp = np.asarray(all_tp, dtype=np.float64)
            all_tp = np.exp(k_dp * all_tp) / np.sum(np.exp(k_dp * all_tp))
        elif kind == "lowent":
            all_tp = np.asarray(all_tp)
            all_tp = np.exp(all_tp) / np.sum(np.exp(all_tp))
            if np.isnan(all_tp[0]):
                all_tp = np.ones(num_domains) / num_domains
            # compute_lifelong_likelihood.py:187 has no dtype here, so its float32 p(x) stay float32, exp(300 p(x))
            # underflows to 0 for p(x) < -0.34 -- always, as p(x) <= -0.5 log(2 pi) -- and lowent is mm with a NaN
            # printed.  Its float64 run does what the line means; that is what the port and this fixture do.
            all_tp_2 = np.asarray(all_tp_2, dtype=np.float64 if tool == "lifelong" else None)
            all_tp_2 = np.exp(k_le * all_tp_2) / np.sum(np.exp(k_le * all_tp_2))
            margins.append(abs(entropy(all_tp_2) - entropy(all_tp)))
            if entropy(all_tp_2) < entropy(all_tp):
                all_tp = all_tp_2
        else:
            all_tp = np.asarray(all_tp, dtype=np.float64)
        post = np.zeros((mat.shape[1], all_pcx[0].shape[1]))
        if tool == "lifelong":
            prior_acc = np.zeros(post.shape[1])
            for idx, pcx in enumerate(all_pcx):
                post += pcx * np.ones(pcx.shape) * all_tp[idx]
                prior_acc += np.exp(priors[idx]) * all_tp[idx]
            out = np.log(post) - pw * np.log(prior_acc)
        else:
            for idx, pcx in enumerate(all_pcx):
                post += (np.log(pcx) - pw * priors[idx]) * all_tp[idx]
            out = post / num_domains
    return dict(mm=np.array(mms, dtype=np.float64), px=np.array(px_save, dtype=np.float64), w=np.asarray(all_tp),
                out=out, margins=margins)


def dmax(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        raise SystemExit("%s: the NaN patterns of the float32 and float64 runs differ" % what)
    fin = np.isfinite(a) & np.isfinite(b)
    if not np.array_equal(a[~fin & ~np.isnan(a)], b[~fin & ~np.isnan(b)]):
        raise SystemExit("%s: the infinities of the float32 and float64 runs differ" % what)
    return float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0


def main():
    S, nnetRNN, nnetVAE = reference()
    seed = 41
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    K = FDIM * (LEFT + RIGHT + 1)
    models = [nnetRNN(K, LAYERS, HID, NCLS, 0) for _ in range(D)]
    vaes = [nnetVAE(K, LAYERS, 1, HID, BN, 0, False) for _ in range(D)]
    with torch.no_grad():
        for m in models:
            for k, p in m.named_parameters():
                if k.split(".")[-1].startswith("weight"):
                    p.mul_(3.0)
        for m in models + vaes:
            m.eval()
    models64 = [copy.deepcopy(m).double() for m in models]
    vaes64 = [copy.deepcopy(m).double() for m in vaes]
    utts = ["utt%d" % i for i in range(len(LENS))]
    xs = {n: np.round(rng.standard_normal((T, FDIM)) * 3.0 + 1.0, 3).astype(np.float32) for n, T in zip(utts, LENS)}
    allx = np.concatenate(list(xs.values())).astype(np.float64)
    st = np.zeros((2, FDIM + 1))
    st[0, :FDIM], st[1, :FDIM], st[0, FDIM] = allx.sum(0), (allx ** 2).sum(0), allx.shape[0]
    norm = PN.cmvn_norm(st, norm_vars=True)
    priors = [np.log(rng.dirichlet(np.ones(NCLS) * 5.0)) for _ in range(D)]
    # the noise, in the reference's draw order: per utterance in order, per model in order
    torch.manual_seed(seed + 1)
    eps = {n: [torch.randn(1, xs[n].shape[0], BN)[0].numpy().copy() for _ in range(D)] for n in utts}
    base = dict(stats=st)
    hdr = dict(feature_dim=FDIM, num_frames=LEFT + RIGHT + 1, num_layers=LAYERS, hidden_dim=HID, num_classes=NCLS,
               dropout=0.0)
    vhdr = dict(feature_dim=FDIM, num_frames=LEFT + RIGHT + 1, encoder_num_layers=LAYERS, decoder_num_layers=1,
                hidden_dim=HID, bn_dim=BN)
    for i in range(D):
        for k, v in models[i].state_dict().items():
            base["sd%d_%s" % (i, k)] = v.detach().numpy().copy()
        for k, v in vaes[i].state_dict().items():
            base["vsd%d_%s" % (i, k)] = v.detach().numpy().copy()
        base["prior%d" % i] = priors[i]
    for n in utts:
        base["in_" + n] = xs[n]
        for i in range(D):
            base["eps%d_%s" % (i, n)] = eps[n][i]
    base["meta"] = np.array(json.dumps(dict(D=D, left=LEFT, right=RIGHT, feat_type="cmvn", utts=utts, lens=list(LENS),
                                            seed=seed, header=hdr, vae_header=vhdr, torch=torch.__version__,
                                            numpy=np.__version__)))
    path = os.path.join(HERE, "lifelong_models.npz")
    np.savez_compressed(path, **base)
    print("wrote %s, %d KiB" % (path, os.path.getsize(path) // 1024))

    rows = {n: PN.post(xs[n], norm, True, 0, 2, 0, LEFT, RIGHT) for n in utts}
    pw = 0.8
    cases = [("lifelong_mm", "lifelong", "mm", None, (False, True)), ("lifelong_dp", "lifelong", "dp", None, (False,)),
             ("lifelong_lowent", "lifelong", "lowent", None, (False,)),
             ("lifelong_fixed", "lifelong", "fixed", [0.5, 0.0, 1.5], (False,)),
             ("lifelong_incremental", "incremental", "lowent", None, (False,))]
    for name, tool, kind, fixed, sels in cases:
        arrays, d32, margin = {}, dict(mm=0.0, px=0.0, w=0.0, out=0.0), np.inf
        for sel in sels:
            pre = "sel_" if sel else ""
            for n in utts:
                r64 = run_utt(S, tool, kind, models64, vaes64, rows[n], eps[n], priors, pw, fixed, sel, torch.float64)
                r32 = run_utt(S, tool, kind, models, vaes, rows[n], eps[n], priors, pw, fixed, sel, torch.float32)
                for k in ("mm", "px", "w", "out"):
                    if (k == "mm" and kind not in ("mm", "lowent")) or (k == "px" and kind not in ("dp", "lowent")):
                        continue
                    d32[k] = max(d32[k], dmax(r32[k], r64[k], "%s %s %s" % (name, n, k)))
                    if k != "out":
                        arrays["%s%s_%s" % (pre, k, n)] = r64[k]
                margin = min([margin] + r64["margins"] + r32["margins"])
                arrays[pre + "out64_" + n] = r64["out"]
                arrays[pre + "out32_" + n] = r32["out"].astype(np.float32)
                arrays[pre + "text3_" + n] = text3(r32["out"].astype(np.float32))
        for k, v in d32.items():
            if not v <= LIMITS[k]:
                raise SystemExit("%s: the reference's float32 run is %.3g from its float64 run at %s (limit %g): not "
                                 "written" % (name, v, k, LIMITS[k]))
        if not margin >= MARGIN:
            raise SystemExit("%s: a near-tie (margin %.3g) decides an argmax or the entropy comparison" % (name, margin))
        meta = dict(tool=tool, kind=kind, fixed=fixed, prior_weight=pw, stream_selection=list(sels), utts=utts,
                    d32_mm=d32["mm"], d32_px=d32["px"], d32_w=d32["w"], d32_out=d32["out"],
                    margin=None if np.isinf(margin) else float(margin), text_ok=bool(d32["out"] <= 1e-4),
                    limits=LIMITS)
        arrays["meta"] = np.array(json.dumps(meta))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print("wrote %s, %d KiB, d32 %s, margin %s, text_ok %s" % (path, os.path.getsize(path) // 1024, d32, margin,
                                                                   meta["text_ok"]))
    cli_options_fixture()


def cli_options_fixture():
    import ast
    out = {}
    for script in ("compute_lifelong_likelihood", "compute_incremental_likelihood"):
        src = open(os.path.join(REF, "src/nnet/%s.py" % script)).read()
        opts = []
        for node in ast.walk(ast.parse(src)):
            if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
                kw = {}
                for k in node.keywords:
                    if k.arg in ("default", "action"):
                        kw[k.arg] = ast.literal_eval(k.value)
                    elif k.arg == "type":
                        kw["type"] = k.value.id
                opts.append(dict(name=ast.literal_eval(node.args[0]), **kw))
        out[script] = opts
    with open(os.path.join(HERE, "cli_options_lifelong.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote cli_options_lifelong.json", {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
