"""Golden fixtures of the feed-forward network (tests/test_nnet.py), produced by the REAL reference model class
src/nnet/nnet_models.py nnetFeedforward (imported from the reference checkout at generation time only) on torch's
CPU float32 path, the way extract_posterior.py runs it: one utterance at a time, `embeds` tapped before the ReLU.

  nnet_small   9 columns, cmvn, splice -1..+1 (27) -> 2 x 40 -> 10; utterances of 1, 2, 23 and 70 frames
  nnet_tiny    5 columns, raw, no splice -> 1 x 3 -> 2   (num_layers 1)
  nnet_single  7 columns, raw, no splice -> 3            (num_layers 0: a single Linear)

Kaldi is absent, so the rows entering the network are those of tests/post_numpy.py (apply-cmvn with Kaldi's defaults,
means only, then splice-feats), which tests/test_post.py holds the device to.  Stored per fixture: the settings
(meta), the weights w<i> / biases b<i> of model.state_dict(), the CMVN stats, and per utterance the input, every
embeds[i] (tap<i>_), the logits (logits_) and the logits as dict2Ark's '%.3f' text ark holds them (logits3_).

Run from the repository root:  python tests/golden/make_golden_nnet.py
"""
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
import post_numpy as PN  # noqa: E402


def text3(a):
    """the values np.savetxt(fmt='%.3f') writes (features.py dict2Ark), read back as float32 like copy-feats does"""
    s = io.StringIO()
    np.savetxt(s, a, fmt="%.3f")
    return np.loadtxt(io.StringIO(s.getvalue()), dtype=np.float64, ndmin=2).astype(np.float32).reshape(a.shape)


def make(name, feature_dim, left, right, num_layers, hidden_dim, num_classes, lens, cmvn, seed):
    sys.path.insert(0, os.path.join(REF, "src/nnet"))
    from nnet_models import nnetFeedforward  # noqa: E402
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    num_frames = left + right + 1
    model = nnetFeedforward(feature_dim * num_frames, num_layers, hidden_dim, num_classes)
    model.eval()
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
        norm = PN.cmvn_norm(st, norm_vars=False)
    for i, layer in enumerate(model.layers):
        arrays["w%d" % i] = layer.weight.detach().numpy().copy()
        arrays["b%d" % i] = layer.bias.detach().numpy().copy()
    with torch.no_grad():
        for u in utts:
            rows = PN.post(xs[u], norm, False, 0, 2, 0, left, right)
            embeds, logits = model(torch.FloatTensor(rows))
            arrays["in_" + u] = xs[u]
            for i, e in enumerate(embeds):
                arrays["tap%d_%s" % (i, u)] = e.numpy().copy()
            arrays["logits_" + u] = logits.numpy().copy()
            arrays["logits3_" + u] = text3(logits.numpy())
    meta = dict(feature_dim=feature_dim, num_frames=num_frames, num_layers=num_layers, hidden_dim=hidden_dim,
                num_classes=num_classes, left=left, right=right, feat_type="cmvn" if cmvn else None, utts=utts,
                seed=seed, torch=torch.__version__, numpy=np.__version__)
    arrays["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    make("nnet_small", 9, 1, 1, 2, 40, 10, (1, 2, 23, 70), True, 11)
    make("nnet_tiny", 5, 0, 0, 1, 3, 2, (1, 6, 33), False, 12)
    make("nnet_single", 7, 0, 0, 0, 5, 3, (4, 17), False, 13)
