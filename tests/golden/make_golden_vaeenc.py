"""Golden fixtures of the VAE-encoded GRU models (tests/test_vaeenc.py), produced by the REAL reference model classes
src/nnet/nnet_models.py nnetVAE and nnetRNN and src/nnet/nnet_models_cnn.py nnetVAECNNNopool (imported from the
reference checkout at generation time only) on torch's CPU path, doing what the loop of
compute_vae_encoded_likelihood.py:112-131 does, in this project's own code: one utterance at a time through the VAE
model, the means of its latent centred over time and divided by the root of their unbiased variance over time, then
the classifier on that with the utterance's length.

  vaeenc_rnn  7 columns, cmvn with vars, splice -1..+1 (21) -> 2 GRU x 33 -> bn 11 -> norm -> 2 GRU x 33 -> 10
  vaeenc_cnn  7 columns, cmvn with vars, no splice -> conv 1 -> 5 -> 6 -> 9, kernel (3, 5) -> bn 11 -> norm ->
              2 GRU x 33 -> 10
  vaeenc_mod  vae_type "modulation": the GRU encoder of vaeenc_rnn with a latent of nfilters 4 x nrepeats 3
Utterances of 2, 3 and 40 frames each.  The generator also runs an utterance of ONE frame through the same loop and
asserts that the reference's output is all NaN (0 / 0 in the unbiased variance); meta["t1_all_nan"] records it.

As in make_golden_rnn.py, every `weight*` tensor of the freshly initialised models is multiplied by 3, and a fixture
is REFUSED unless the reference's own float32 forward lies within 1e-5 of its float64 forward (d32, stored in meta).
The sampled decoder output the script throws away is thrown away here too; the sampler's noise reaches nothing stored.

Stored per fixture: the settings (meta: the classifier header `header`, the encoder file's `enc_header`), the
classifier's state dict (sd_<key>), the encoder file's (esd_<key>, decoder and vars included), the CMVN stats, and
per utterance the input (in_), the float64 and float32 forwards (f64_, f32_), the logits as a '%.3f' text ark holds
them (logits3_), every stage's float64 output from forward hooks on the real modules (stage<i>_; a conv stage's is
its pre-activation in rows [t][c F + f]; the norm stage's is the normalised latent the loop computes).
cli_options_vaeenc.json is the reference's argparse table, names and defaults only, read from its source with ast.

Run from the repository root:  python tests/golden/make_golden_vaeenc.py
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


def run(vae_model, model, arch, rows, dtype):
    """(output [T, C], [stage outputs [T, width]]) of one utterance"""
    taps = []

    def hook(mod, inp, out):
        if isinstance(out, tuple):                    # nn.GRU on a packed sequence
            taps.append(out[0].data.detach().numpy().copy())
        elif out.dim() == 4:                          # Conv2d: [1, C, F, T] -> rows [t][c F + f]
            taps.append(out[0].detach().permute(2, 0, 1).reshape(out.shape[3], -1).numpy().copy())
        else:                                         # Conv1d: [1, C, T]
            taps.append(out[0].detach().numpy().T.copy())

    enc = vae_model.vae_encoder
    enc_mods = (list(enc.cnn_layers) if arch == "cnn" else list(enc.layers)) + [enc.means]
    cls_mods = list(model.layers) + [model.regression]
    hs = [m.register_forward_hook(hook) for m in enc_mods + cls_mods]
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(rows)).to(dtype)
        T = torch.IntTensor([x.shape[0]])
        if arch == "cnn":
            # the (feature x time) image of the utterance, one channel: [1, 1, F, T]
            latent = vae_model(x.t().reshape(1, 1, x.shape[1], x.shape[0]))[1]
            means = latent[0].permute(0, 2, 1)        # [1, bn, T] -> [1, T, bn]
        else:
            latent = vae_model(x.unsqueeze(0), T)[1]
            means = latent[0]                         # [1, T, bn]
        n_enc = len(taps)                             # the decoder has no hooks; the encoder ran once
        centred = means - means.mean(dim=1, keepdim=True)
        normed = centred / centred.var(dim=1, keepdim=True).sqrt()   # unbiased, as torch.var is by default
        z = normed[0].numpy().copy()
        out = model(normed, T)
    for h in hs:
        h.remove()
    assert n_enc == len(enc_mods) and len(taps) == len(enc_mods) + len(cls_mods)
    return out[0].numpy().copy(), taps[:n_enc] + [z] + taps[n_enc:]


def make(name, arch, vae_type, feature_dim, left, right, lens, seed, enc_layers=0, enc_hidden=0, channels=None,
         kernel=None, bn=0, nfilters=0, nrepeats=0, layers=2, hidden=33, num_classes=10):
    sys.path.insert(0, os.path.join(REF, "src/nnet"))
    from nnet_models import nnetRNN, nnetVAE  # noqa: E402
    from nnet_models_cnn import nnetVAECNNNopool  # noqa: E402
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    num_frames = left + right + 1
    latent = nfilters * nrepeats if vae_type == "modulation" else bn
    if arch == "cnn":
        assert num_frames == 1
        # the script: nnetVAECNNNopool(vae['feature_dim'], vae['num_frames'], in_channels, out_channels, kernel, bn, False)
        ehdr = dict(feature_dim=feature_dim, num_frames=40, in_channels=",".join(map(str, channels[:-1])),
                    out_channels=",".join(map(str, channels[1:])), kernel="%d,%d" % kernel)
        vae_model = nnetVAECNNNopool(feature_dim, 40, list(channels[:-1]), list(channels[1:]), tuple(kernel), latent,
                                     False)
    else:
        ehdr = dict(feature_dim=feature_dim, num_frames=num_frames, encoder_num_layers=enc_layers,
                    decoder_num_layers=1, hidden_dim=enc_hidden)
        vae_model = nnetVAE(feature_dim * num_frames, enc_layers, 1, enc_hidden, latent, 0, False)
    ehdr.update(dict(nfilters=nfilters, nrepeats=nrepeats) if vae_type == "modulation" else dict(bn_dim=bn))
    model = nnetRNN(latent, layers, hidden, num_classes, 0)
    hdr = dict(vaeenc="exp/vae/final.model", vae_type=vae_type, feature_dim=feature_dim, num_frames=ehdr["num_frames"],
               num_classes=num_classes, num_layers=layers, hidden_dim=hidden, dropout=0.0)
    with torch.no_grad():
        for m in (vae_model, model):
            for k, p in m.named_parameters():
                if k.split(".")[-1].startswith("weight"):
                    p.mul_(3.0)
    vae_model.eval()
    model.eval()
    vae64, model64 = copy.deepcopy(vae_model).double(), copy.deepcopy(model).double()
    utts = ["utt%d" % i for i in range(len(lens))]
    xs = {u: np.round(rng.standard_normal((T, feature_dim)) * 3.0 + 1.0, 3).astype(np.float32)
          for u, T in zip(utts, lens)}
    arrays = {}
    allx = np.concatenate(list(xs.values())).astype(np.float64)
    st = np.zeros((2, feature_dim + 1))
    st[0, :feature_dim], st[1, :feature_dim], st[0, feature_dim] = allx.sum(0), (allx ** 2).sum(0), allx.shape[0]
    arrays["stats"] = st
    norm = PN.cmvn_norm(st, norm_vars=True)
    for k, v in model.state_dict().items():
        arrays["sd_" + k] = v.detach().numpy().copy()
    for k, v in vae_model.state_dict().items():
        arrays["esd_" + k] = v.detach().numpy().copy()
    d32 = 0.0
    for u in utts:
        rows = PN.post(xs[u], norm, True, 0, 2, 0, left, right)
        f64, st64 = run(vae64, model64, arch, rows, torch.float64)
        f32, _ = run(vae_model, model, arch, rows, torch.float32)
        assert np.array_equal(st64[-1], f64) and np.isfinite(f64).all()
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
    # one frame: the unbiased variance is 0 / 0 and the reference's output is NaN everywhere
    one = PN.post(xs[utts[0]][:1], norm, True, 0, 2, 0, left, right)
    t1_64, _ = run(vae64, model64, arch, one, torch.float64)
    t1_32, _ = run(vae_model, model, arch, one, torch.float32)
    assert np.isnan(t1_64).all() and np.isnan(t1_32).all(), "the reference's one-frame output is not all-NaN"
    meta = dict(hdr, vae_arch=arch, left=left, right=right, feat_type="cmvn", utts=utts, seed=seed, d32=d32,
                header=sorted(hdr), enc_header=ehdr, t1_all_nan=True, n_stages=len(st64),
                torch=torch.__version__, numpy=np.__version__)
    arrays["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s, %d KiB, d32 %.3g" % (path, os.path.getsize(path) // 1024, d32))


def cli_options_fixture():
    import ast
    src = open(os.path.join(REF, "src/nnet/compute_vae_encoded_likelihood.py")).read()
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
    with open(os.path.join(HERE, "cli_options_vaeenc.json"), "w") as f:
        json.dump(opts, f, indent=1)
    print("wrote cli_options_vaeenc.json", len(opts))


if __name__ == "__main__":
    make("vaeenc_rnn", "rnn", "normal", 7, 1, 1, (2, 3, 40), 31, enc_layers=2, enc_hidden=33, bn=11)
    make("vaeenc_cnn", "cnn", "normal", 7, 0, 0, (2, 3, 40), 32, channels=(1, 5, 6, 9), kernel=(3, 5), bn=11)
    make("vaeenc_mod", "rnn", "modulation", 7, 1, 1, (2, 3, 40), 33, enc_layers=2, enc_hidden=33, nfilters=4,
         nrepeats=3)
    cli_options_fixture()
