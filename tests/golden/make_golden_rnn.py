"""Golden fixtures of the GRU models (tests/test_rnn.py), produced by the REAL reference model classes
src/nnet/nnet_models.py nnetRNN and nnetAEClassifierMultitask (imported from the reference checkout at generation
time only) on torch's CPU path, the way dump_genclassifier_outputs.py runs them: model.eval(), one utterance at a
time, `model(mat[None], IntTensor([T]))`.

  rnn_noae    9 columns, cmvn with vars, splice -1..+1 (27) -> 2 GRU x 40 -> 10; utterances of 1, 2, 23, 70 frames
  rnn_normal  9 columns, cmvn with vars, splice -1..+1 -> enc 2 GRU x 33 -> bn 12 (ReLU) -> 1 GRU x 33 -> 7;
              utterances of 1, 5, 40 frames; the state dict holds the `ae` branch too
  rnn_tiny    5 columns, raw, no splice -> 1 GRU x 3 -> 2; utterances of 1, 6 frames

Every `weight*` tensor of the freshly initialised model is multiplied by 3: with torch's default init the gates stay
near 1/2 and the recurrence barely matters; x 3 saturates gates.  Each fixture is REFUSED unless the reference's own
float32 forward lies within 1e-5 of its float64 forward (d32, stored in meta): that keeps the fixture on the
non-chaotic side, where a tolerance against it means something (x 6 at H 256 gives 6.1 and is out).

Kaldi is absent, so the rows entering the model are those of tests/post_numpy.py (apply-cmvn --norm-vars=true, then
splice-feats), which tests/test_post.py holds the device to.  Stored per fixture: the settings (meta), the state
dict (sd_<key>), the CMVN stats, and per utterance the input (in_), the float64 forward of the real class
(f64_), its float32 forward (f32_), the logits as dict2Ark's '%.3f' text ark holds them (logits3_) and every
stage's float64 output (stage<i>_, from forward hooks on the real modules).  cli_options_rnn.json is the
reference's argparse table, names and defaults only, read from its source with ast.

Run from the repository root:  python tests/golden/make_golden_rnn.py
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


def stage_modules(model, ae_type):
    """the modules whose outputs are the stages' outputs, in order (a bottleneck's is its pre-activation)"""
    if ae_type == "noae":
        return list(model.layers) + [model.regression]
    return (list(model.encoder.layers) + [model.encoder.bottleneck] + list(model.classifier.layers)
            + [model.classifier.regression])


def run(model, ae_type, rows, dtype):
    """(logits [T, C], [stage outputs [T, width]]) of one utterance"""
    taps = []

    def hook(mod, inp, out):
        if isinstance(out, tuple):       # nn.GRU on a packed sequence
            taps.append(out[0].data.detach().numpy().copy())
        else:                            # Conv1d: [1, C, T]
            taps.append(out[0].detach().numpy().T.copy())

    # the classifier branch runs first; the `ae` branch re-runs the encoder, whose taps are dropped below
    mods = stage_modules(model, ae_type)
    hs = [m.register_forward_hook(hook) for m in mods]
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(rows)).to(dtype)[None, :, :]
        out = model(x, torch.IntTensor([x.size(1)]))
    for h in hs:
        h.remove()
    if ae_type == "normal":
        out = out[0]
    return out[0].numpy().copy(), taps[:len(mods)]


def make(name, ae_type, feature_dim, left, right, hidden, num_classes, lens, cmvn, seed, enc=0, cls=0, bn=0, layers=0):
    sys.path.insert(0, os.path.join(REF, "src/nnet"))
    from nnet_models import nnetAEClassifierMultitask, nnetRNN  # noqa: E402
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    num_frames = left + right + 1
    K0 = feature_dim * num_frames
    if ae_type == "noae":
        model = nnetRNN(K0, layers, hidden, num_classes, 0.2)
        hdr = dict(feature_dim=feature_dim, num_frames=num_frames, num_layers=layers, hidden_dim=hidden,
                   num_classes=num_classes, dropout=0.2)
    else:
        model = nnetAEClassifierMultitask(K0, num_classes, enc, cls, 1, hidden, bn, 0.2)
        hdr = dict(feature_dim=feature_dim, num_frames=num_frames, num_classes=num_classes, encoder_num_layers=enc,
                   classifier_num_layers=cls, ae_num_layers=1, hidden_dim=hidden, bn_dim=bn, enc_dropout=0.2)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.split(".")[-1].startswith("weight"):
                p.mul_(3.0)
    model.eval()
    model64 = copy.deepcopy(model).double()
    utts = ["utt%d" % i for i in range(len(lens))]
    xs = {u: np.round(rng.standard_normal((T, feature_dim)) * 3.0 + 1.0, 3).astype(np.float32)
          for u, T in zip(utts, lens)}
    arrays = {}
    norm = None
    if cmvn:
        allx = np.concatenate(list(xs.values())).astype(np.float64)
        st = np.zeros((2, feature_dim + 1))
        st[0, :feature_dim], st[1, :feature_dim], st[0, feature_dim] = allx.sum(0), (allx ** 2).sum(0), allx.shape[0]
        arrays["stats"] = st
        norm = PN.cmvn_norm(st, norm_vars=True)
    for k, v in model.state_dict().items():
        arrays["sd_" + k] = v.detach().numpy().copy()
    d32 = 0.0
    for u in utts:
        rows = PN.post(xs[u], norm, cmvn, 0, 2, 0, left, right)
        f64, st64 = run(model64, ae_type, rows, torch.float64)
        f32, _ = run(model, ae_type, rows, torch.float32)
        assert np.array_equal(st64[-1], f64)
        d32 = max(d32, float(np.abs(f32.astype(np.float64) - f64).max()))
        arrays["in_" + u] = xs[u]
        arrays["f64_" + u] = f64
        arrays["f32_" + u] = f32
        arrays["logits3_" + u] = text3(f32)
        for i, s in enumerate(st64):
            arrays["stage%d_%s" % (i, u)] = s
    if not d32 <= D32_LIMIT:
        raise SystemExit("%s: the reference's float32 forward is %.3g from its float64 forward (limit %g): not written"
                         % (name, d32, D32_LIMIT))
    meta = dict(hdr, ae_type=ae_type, left=left, right=right, feat_type="cmvn" if cmvn else None, utts=utts,
                seed=seed, d32=d32, header=sorted(hdr), torch=torch.__version__, numpy=np.__version__)
    arrays["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s, %d KiB, d32 %.3g" % (path, os.path.getsize(path) // 1024, d32))


def cli_options_fixture():
    import ast
    src = open(os.path.join(REF, "src/nnet/dump_genclassifier_outputs.py")).read()
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
    with open(os.path.join(HERE, "cli_options_rnn.json"), "w") as f:
        json.dump(opts, f, indent=1)
    print("wrote cli_options_rnn.json", len(opts))


if __name__ == "__main__":
    make("rnn_noae", "noae", 9, 1, 1, 40, 10, (1, 2, 23, 70), True, 21, layers=2)
    make("rnn_normal", "normal", 9, 1, 1, 33, 7, (1, 5, 40), True, 22, enc=2, cls=1, bn=12)
    make("rnn_tiny", "noae", 5, 0, 0, 3, 2, (1, 6), False, 23, layers=1)
    cli_options_fixture()
