"""Golden fixtures of the multi-stream GRU model (tests/test_multimod.py), produced by the REAL reference class
src/nnet/nnet_models.py nnetRNNMultimod (imported from the reference checkout at generation time only) on torch's
CPU path, the way dump_multimod_outputs.py runs it: one utterance at a time,
`model([mat_0[None], .., mat_{M-1}[None]], IntTensor([T]))`.

  multimod_3     3 streams of 9 columns, each with its own global cmvn (with vars) and splice -1..+1 (27) ->
                 1 GRU x 20 per stream -> 1 trunk GRU x 60 -> 10; utterances of 1, 2, 23, 70 frames
  multimod_deep  2 streams of 27 columns, raw, no splice -> 2 GRU x 17 per stream -> 2 trunk GRU x 34 -> 7;
                 utterances of 1, 5, 40 frames
  multimod_tiny  1 stream of 5 columns, raw, no splice -> 1 GRU x 3 -> 1 trunk GRU x 3 -> 2; utterances of 1, 6 frames

As in make_golden_rnn.py every `weight*` tensor of the freshly initialised model is multiplied by 3 (saturated
gates, a recurrence that matters), and a fixture is REFUSED unless the reference's own float32 forward lies within
1e-5 of its float64 forward (d32, stored in meta).  The rows entering the model are those of tests/post_numpy.py.

Stored per fixture: the settings (meta), the state dict (sd_<key>), per stream the CMVN stats (stats_<s>), per
utterance and stream the input (in_<s>_<utt>), and per utterance the float64 forward of the real class (f64_, which
is also the regression's tap), its float32 forward (f32_), the logits as dict2Ark's '%.3f' text ark holds them
(logits3_) and the float64 taps from forward hooks on the real modules: each sub-network's last layer
(sub<s>_<utt>) and each trunk GRU (trunk<l>_<utt>).  A fixture whose taps would push the file past the size of
rnn_noae.npz keeps them in a second file, <name>_taps.npz.  cli_options_multimod.json is the reference's argparse
table, names and defaults only, read from its source with ast.

Run from the repository root:  python tests/golden/make_golden_multimod.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
from make_golden_nnet import text3  # noqa: E402
import post_numpy as PN  # noqa: E402

D32_LIMIT = 1e-5
SIZE_LIMIT = os.path.getsize(os.path.join(HERE, "rnn_noae.npz"))


def run(model, rows, dtype):
    """(logits [T, C], sub-network outputs [M][T, Hs], trunk GRU outputs [Lt][T, M Hs]) of one utterance"""
    sub, trunk = [], []
    hs = [m.register_forward_hook(lambda mod, inp, out: sub.append(out[0].detach().numpy().copy()))
          for m in model.subnets]
    hs += [m.register_forward_hook(lambda mod, inp, out: trunk.append(out[0].data.detach().numpy().copy()))
           for m in model.layers]
    with torch.no_grad():
        xs = [torch.from_numpy(np.asarray(r)).to(dtype)[None, :, :] for r in rows]
        out = model(xs, torch.IntTensor([xs[0].size(1)]))
    for h in hs:
        h.remove()
    return out[0].numpy().copy(), sub, trunk


def make(name, M, feature_dim, left, right, Ls, Hs, Lt, num_classes, lens, cmvn, seed):
    sys.path.insert(0, os.path.join(REF, "src/nnet"))
    from nnet_models import nnetRNNMultimod  # noqa: E402
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    num_frames = left + right + 1
    model = nnetRNNMultimod(feature_dim * num_frames, Ls, Lt, Hs, num_classes, M)
    hdr = dict(feature_dim=feature_dim, num_frames=num_frames, num_classes=num_classes, num_layers_subband=Ls,
               num_layers=Lt, hidden_dim_subband=Hs, mod_num=M)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.split(".")[-1].startswith("weight"):
                p.mul_(3.0)
    model.eval()
    model64 = copy.deepcopy(model).double()
    utts = ["utt%d" % i for i in range(len(lens))]
    # stream s sits at another offset and scale, as the modulation streams of one utterance do
    xs = [{u: np.round(rng.standard_normal((T, feature_dim)) * (3.0 - s) + 1.0 + s, 3).astype(np.float32)
           for u, T in zip(utts, lens)} for s in range(M)]
    arrays, taps, norms = {}, {}, [None] * M
    for s in range(M):
        if cmvn:
            allx = np.concatenate(list(xs[s].values())).astype(np.float64)
            st = np.zeros((2, feature_dim + 1))
            st[0, :feature_dim], st[1, :feature_dim], st[0, feature_dim] = allx.sum(0), (allx ** 2).sum(0), allx.shape[0]
            arrays["stats_%d" % s] = st
            norms[s] = PN.cmvn_norm(st, norm_vars=True)
    for k, v in model.state_dict().items():
        arrays["sd_" + k] = v.detach().numpy().copy()
    d32 = 0.0
    for u in utts:
        rows = [PN.post(xs[s][u], norms[s], cmvn, 0, 2, 0, left, right) for s in range(M)]
        f64, sub64, trunk64 = run(model64, rows, torch.float64)
        f32, _, _ = run(model, rows, torch.float32)
        assert len(sub64) == M and len(trunk64) == Lt and f64.dtype == np.float64
        d32 = max(d32, float(np.abs(f32.astype(np.float64) - f64).max()))
        for s in range(M):
            arrays["in_%d_%s" % (s, u)] = xs[s][u]
            taps["sub%d_%s" % (s, u)] = sub64[s]
        for l in range(Lt):
            taps["trunk%d_%s" % (l, u)] = trunk64[l]
        arrays["f64_" + u] = f64
        arrays["f32_" + u] = f32
        arrays["logits3_" + u] = text3(f32)
    if not d32 <= D32_LIMIT:
        raise SystemExit("%s: the reference's float32 forward is %.3g from its float64 forward (limit %g): not written"
                         % (name, d32, D32_LIMIT))
    meta = dict(hdr, left=left, right=right, feat_type="cmvn" if cmvn else None, utts=utts, seed=seed, d32=d32,
                header=sorted(hdr), torch=torch.__version__, numpy=np.__version__)
    path, tpath = os.path.join(HERE, name + ".npz"), os.path.join(HERE, name + "_taps.npz")
    meta["taps_file"] = None
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays, **taps)
    if os.path.getsize(path) > SIZE_LIMIT:
        meta["taps_file"] = os.path.basename(tpath)
        np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
        np.savez_compressed(tpath, **taps)
    elif os.path.exists(tpath):
        os.unlink(tpath)
    for f in (path, tpath):
        if os.path.exists(f):
            assert os.path.getsize(f) <= SIZE_LIMIT, (f, os.path.getsize(f), SIZE_LIMIT)
            print("wrote %s, %d KiB, d32 %.3g" % (f, os.path.getsize(f) // 1024, d32))


def cli_options_fixture():
    import ast
    src = open(os.path.join(REF, "src/nnet/dump_multimod_outputs.py")).read()
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
    with open(os.path.join(HERE, "cli_options_multimod.json"), "w") as f:
        json.dump(opts, f, indent=1)
    print("wrote cli_options_multimod.json", len(opts))


if __name__ == "__main__":
    make("multimod_3", 3, 9, 1, 1, 1, 20, 1, 10, (1, 2, 23, 70), True, 31)
    make("multimod_deep", 2, 27, 0, 0, 2, 17, 2, 7, (1, 5, 40), False, 32)
    make("multimod_tiny", 1, 5, 0, 0, 1, 3, 1, 2, (1, 6), False, 33)
    cli_options_fixture()
