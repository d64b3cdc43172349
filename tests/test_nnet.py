"""extract-posterior: the feed-forward acoustic model after the chain (speech_recognition_tools_amd/nnet.py,
dense_kernel and row_epilogue_kernel of csrc/fdlp_nnet.hip, layer 0 in xform_kernel of csrc/fdlp_post.hip).

Kaldi is absent, so the rows entering the network are those of tests/post_numpy.post, which tests/test_post.py
holds the device to.  Bounds, none of them fitted to what the device gives:

  * a layer against its own input: y = f(A) W^T + b is one float32 dot product of K terms in some order plus one
    add, so elementwise, for K <= 4096,  |got - ref64| <= (K + 2) 2^-24 (|f(A)| |W|^T + |b|)  (the bound
    tests/test_transform.py asserts), with A the float32 values the device itself produced for the layer below: no
    error propagates, which keeps the bound tight at any width;
  * against the reference's outputs (tests/golden/nnet_*.npz, torch's CPU float32 forward of the reference's model
    class): both sides lie within E of the float64 forward pass, E_l = (K + 2) 2^-24 ((|a| + E_{l-1}) |W|^T + |b|)
    + E_{l-1} |W|^T with E_0 = 0 (ReLU is 1-Lipschitz), so |got - golden| <= 2 E;
  * softmax of the device's own float32 logits x, m = max x, T = max_j (m - x_j): relative error at most
    (C + 8 + T) 2^-23 plus an absolute 1e-37 -- the subtraction moves the exponent's argument by |x_j - m| 2^-24,
    exp is within 3 ulp (OCML documents 1 ulp for exp and log in float32; 3 leaves room and is what the bound was
    written with), the C-term sum, one division; the absolute term covers results below the normal range;
  * loglike: absolute error at most (C + 16 + 2 |x_j - m| + |log S| + |w prior_j|) 2^-23.
Every claim of independence (batch composition, position, neighbours, taps) is asserted bitwise.
"""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import post_numpy as PN
from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "bin")
TM, TN, KC = 128, 128, 32     # dense_kernel's row tile, column tile and k chunk (kDenseTM, kDenseTN, kDenseKC)
TN_SMALL = 64                 # the column tile of the instantiation for N <= 64
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits_equal(a, b, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(bits(a), bits(b)), what


def ark_like(rng, T, D, shift=0.0):
    return np.round(rng.standard_normal((T, D)) * 3.0 + shift, 3).astype(np.float32)


def stats_of(x):
    D = x.shape[1]
    st = np.zeros((2, D + 1))
    st[0, :D] = x.astype(np.float64).sum(0)
    st[1, :D] = (x.astype(np.float64) ** 2).sum(0)
    st[0, D] = x.shape[0]
    return st


def make_net(rng, dims):
    ws = [(rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32) for k, n in zip(dims[:-1], dims[1:])]
    bs = [(rng.standard_normal(n) * 0.5).astype(np.float32) for n in dims[1:]]
    return ws, bs


def layer_ref_and_bound(A, W, b):
    """float64 A W^T + b and the elementwise float32 dot-product bound for float32 A (already through f), W, b"""
    K = A.shape[1]
    assert K <= 4096 and W.shape[1] == K
    A64, W64, b64 = A.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    return A64 @ W64.T + b64, (K + 2) * U * (np.abs(A64) @ np.abs(W64).T + np.abs(b64))


def forward64(rows, ws, bs):
    """float64 forward pass of float32 rows: the pre-activations y_l and the propagated bounds E_l"""
    a, E = rows.astype(np.float64), np.zeros(rows.shape)
    ys, Es = [], []
    for l, (W, b) in enumerate(zip(ws, bs)):
        W64, b64 = W.astype(np.float64), b.astype(np.float64)
        x = a if l == 0 else np.maximum(a, 0.0)
        K = W.shape[1]
        y = x @ W64.T + b64
        E = (K + 2) * U * ((np.abs(x) + E) @ np.abs(W64).T + np.abs(b64)) + E @ np.abs(W64).T
        ys.append(y)
        Es.append(E)
        a = y
    return ys, Es


def load_nnet_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    n = meta["num_layers"] + 1
    ws = [z["w%d" % i] for i in range(n)]
    bs = [z["b%d" % i] for i in range(n)]
    return meta, z, ws, bs


def golden_rows(meta, z, u):
    norm = PN.cmvn_norm(z["stats"], norm_vars=False) if meta["feat_type"] == "cmvn" else None
    return PN.post(z["in_" + u], norm, False, 0, 2, 0, meta["left"], meta["right"])


def save_checkpoint(path, meta, ws, bs):
    import torch
    from collections import OrderedDict
    sd = OrderedDict()
    for i, (w, b) in enumerate(zip(ws, bs)):
        sd["layers.%d.weight" % i] = torch.from_numpy(np.array(w))
        sd["layers.%d.bias" % i] = torch.from_numpy(np.array(b))
    torch.save({k: meta[k] for k in ("feature_dim", "num_frames", "num_layers", "hidden_dim", "num_classes")}
               | {"model_state_dict": sd}, path)


GOLDENS = ["nnet_small", "nnet_tiny", "nnet_single"]


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_cli_argparse_surface():
    from speech_recognition_tools_amd import nnet
    a = nnet.extract_posterior_parser().parse_args(["final.mdl", "feats.scp", "egs.config", "post"])
    assert (a.model, a.scp, a.egs_config, a.save_file) == ("final.mdl", "feats.scp", "egs.config", "post")
    assert (a.layer, a.add_softmax) == (0, False)                       # the reference's defaults
    assert (a.prior, a.prior_weight, a.ark_precision, a.batch_rows) == (None, 0.8, 3, 16384)
    a = nnet.extract_posterior_parser().parse_args(["m", "scp:f.scp", "e", "ark:-", "--layer", "2", "--add_softmax",
                                                    "--prior", "p.pkl", "--prior_weight", "0.2", "--device", "1",
                                                    "--batch-rows", "64", "--ark_precision", "-1"])
    assert (a.layer, a.add_softmax, a.prior, a.prior_weight, a.device, a.batch_rows, a.ark_precision) == (
        2, True, "p.pkl", 0.2, 1, 64, -1)
    with pytest.raises(SystemExit):
        nnet.extract_posterior_parser().parse_args(["m", "s", "e"])     # four positionals, as in the reference
    assert os.access(os.path.join(BIN, "extract-posterior"), os.X_OK)


@pytest.mark.parametrize("num_layers", [0, 1, 4])
def test_checkpoint_round_trip(tmp_path, num_layers):
    from speech_recognition_tools_amd.nnet import load_feedforward_checkpoint
    rng = np.random.default_rng(num_layers)
    meta = dict(feature_dim=5, num_frames=3, num_layers=num_layers, hidden_dim=7, num_classes=4)
    dims = [15] + [7] * num_layers + [4]
    ws, bs = make_net(rng, dims)
    p = str(tmp_path / "m.pt")
    save_checkpoint(p, meta, ws, bs)
    c = load_feedforward_checkpoint(p)
    assert (c.feature_dim, c.num_frames, c.num_layers, c.hidden_dim, c.num_classes) == (5, 3, num_layers, 7, 4)
    assert c.dims == dims and len(c.weights) == len(c.biases) == num_layers + 1
    for a, b in zip(c.weights + c.biases, ws + bs):
        assert a.dtype == np.float32
        assert_bits_equal(a, b)


def test_checkpoint_errors_name_the_key(tmp_path):
    import torch
    from speech_recognition_tools_amd.nnet import load_feedforward_checkpoint
    rng = np.random.default_rng(1)
    meta = dict(feature_dim=5, num_frames=3, num_layers=2, hidden_dim=7, num_classes=4)
    ws, bs = make_net(rng, [15, 7, 7, 4])
    p = str(tmp_path / "m.pt")
    # a shape that contradicts the header
    save_checkpoint(p, dict(meta, hidden_dim=8), ws, bs)
    with pytest.raises(ValueError, match=r"layers\.0\.weight"):
        load_feedforward_checkpoint(p)
    save_checkpoint(p, meta, ws, [bs[0], bs[1][:-1], bs[2]])
    with pytest.raises(ValueError, match=r"layers\.1\.bias"):
        load_feedforward_checkpoint(p)
    save_checkpoint(p, dict(meta, num_layers=1), ws, bs)                # a layer beyond the header's count
    with pytest.raises(ValueError, match=r"layers\.1\.weight|layers\.2"):
        load_feedforward_checkpoint(p)
    # missing keys, in the header and in the state dict
    save_checkpoint(p, meta, ws, bs)
    d = torch.load(p, map_location="cpu")
    for k in ("feature_dim", "num_classes", "model_state_dict"):
        torch.save({q: v for q, v in d.items() if q != k}, p)
        with pytest.raises(ValueError, match=k):
            load_feedforward_checkpoint(p)
    save_checkpoint(p, dict(meta, num_layers=3), ws, bs)
    with pytest.raises(ValueError, match=r"layers\.2\.weight|layers\.3"):
        load_feedforward_checkpoint(p)
    # not a dict, not a checkpoint, not there
    torch.save([1, 2, 3], p)
    with pytest.raises(ValueError, match="not a dict"):
        load_feedforward_checkpoint(p)
    open(p, "wb").write(b"garbage")
    with pytest.raises(ValueError, match="m.pt"):
        load_feedforward_checkpoint(p)
    with pytest.raises(OSError):
        load_feedforward_checkpoint(str(tmp_path / "absent.pt"))


def test_egs_config_reader(tmp_path):
    from speech_recognition_tools_amd.nnet import load_egs_config
    p = str(tmp_path / "egs.config")

    def dump(d):
        pickle.dump(d, open(p, "wb"))

    dump({"feat_type": "cmvn,/data/cmvn.ark", "concat_feats": "4,4"})
    c = load_egs_config(p)
    assert (c.feat_type, c.feat_path, c.left, c.right) == ("cmvn", "/data/cmvn.ark", 4, 4)
    dump({"feat_type": "pca,exp/pca.mat", "concat_feats": "3,1"})
    c = load_egs_config(p)
    assert (c.feat_type, c.feat_path, c.left, c.right) == ("pca", "exp/pca.mat", 3, 1)
    dump({"feat_type": None, "concat_feats": None})
    c = load_egs_config(p)
    assert (c.feat_type, c.feat_path, c.left, c.right) == (None, None, 0, 0)
    dump({"feat_type": None, "concat_feats": "0,2"})
    assert (load_egs_config(p).left, load_egs_config(p).right) == (0, 2)
    for bad in ({"feat_type": "cmvn", "concat_feats": None}, {"feat_type": "lda,x", "concat_feats": None},
                {"feat_type": "cmvn,", "concat_feats": None}, {"feat_type": None, "concat_feats": "4"},
                {"feat_type": None, "concat_feats": "a,b"}, {"feat_type": None, "concat_feats": "1,2,3"},
                {"feat_type": None, "concat_feats": "-1,2"}, {"feat_type": None}, ["cmvn"]):
        dump(bad)
        with pytest.raises(ValueError, match="egs.config"):
            load_egs_config(p)
    open(p, "wb").write(b"not a pickle")
    with pytest.raises(ValueError, match="egs.config"):
        load_egs_config(p)


def test_host_only_plan_info_and_refusals():
    from speech_recognition_tools_amd._lib import FDLP_E_INVALID, FdlpError
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    cfg = PostConfig(dim=13, left_context=4, right_context=4)
    p = NnetPlan(cfg, None, None, max_rows=1000, device=-1, dims=[117, 512, 512, 300, 38])
    assert (p.in_dim, p.n_linear, p.dims, p.out_dim) == (117, 4, [117, 512, 512, 300, 38], 38)
    assert p.workspace_bytes == 2 * 1000 * 512 * 4                      # two [max_rows, widest hidden] float32
    assert p.tile == (TM, TN, KC)
    assert p.lds_bytes == 2 * (TM + TN) * (KC + 4) * 4                  # two buffers of an A and a W chunk
    assert [p.tap_dim(t) for t in range(4)] == [38, 300, 512, 512]
    one = NnetPlan(cfg, None, None, max_rows=7, device=-1, dims=[117, 38])
    assert (one.n_linear, one.workspace_bytes, one.tap_dim(0)) == (1, 0, 38)
    with pytest.raises(ValueError):
        one.tap_dim(1)
    # shapes taken from the arrays
    ws, bs = make_net(np.random.default_rng(0), [117, 6, 3])
    assert NnetPlan(cfg, ws, bs, max_rows=5, device=-1).dims == [117, 6, 3]
    # refusals: FDLP_E_INVALID with the sizes in the message
    with pytest.raises(FdlpError) as e:
        NnetPlan(cfg, None, None, device=-1, dims=[116, 512, 38])       # dims[0] is not the stages' out_dim
    assert e.value.code == FDLP_E_INVALID and "116" in str(e.value) and "117" in str(e.value)
    with pytest.raises(FdlpError) as e:
        NnetPlan(cfg, None, None, device=-1, dims=[117])                # n_linear = 0
    assert e.value.code == FDLP_E_INVALID and "n_linear = 0" in str(e.value)
    with pytest.raises(FdlpError) as e:
        NnetPlan(cfg, None, None, device=-1, dims=[117, 512, 0, 38])    # a dimension < 1
    assert e.value.code == FDLP_E_INVALID and "117 -> 512 -> 0 -> 38" in str(e.value)
    with pytest.raises(FdlpError) as e:
        NnetPlan(cfg, None, None, device=-1, dims=[117, -4])
    assert e.value.code == FDLP_E_INVALID and "-4" in str(e.value)
    with pytest.raises(FdlpError) as e:
        NnetPlan(cfg, None, None, max_rows=0, device=-1, dims=[117, 4])
    assert e.value.code == FDLP_E_INVALID and "max_rows" in str(e.value)
    with pytest.raises(FdlpError) as e:
        NnetPlan(cfg, None, None, device=-1, dims=[117] + [8] * 33)     # more than FDLP_NNET_MAX_LINEAR layers
    assert e.value.code == FDLP_E_INVALID and "33" in str(e.value)


def test_entry_points_are_declared_and_exported():
    import ctypes
    import re
    from speech_recognition_tools_amd import _lib
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    names = ["fdlp_nnet_plan_create", "fdlp_nnet_plan_destroy", "fdlp_nnet_plan_info", "fdlp_nnet_compute"]
    src = open(os.path.join(ROOT, "include", "fdlp.h")).read()
    declared = set(re.findall(r"\b(fdlp_[a-z0-9_]+)\s*\(", src))
    for n in names:
        assert n in declared and n in _lib.SIGNATURES and hasattr(_lib.lib, n), n
    assert "#define FDLP_ABI_VERSION 13" in src and _lib.lib.fdlp_abi_version() == 13
    p = NnetPlan(PostConfig(dim=4), None, None, device=-1, dims=[4, 3])
    with pytest.raises(_lib.FdlpError):                                  # a host-only plan refuses to compute
        _lib.check(_lib.lib.fdlp_nnet_compute(p._h, ctypes.byref(_lib.FdlpPostBatchC()), 0, 0, None, 0.8, None))
    with pytest.raises(_lib.FdlpError):
        _lib.check(_lib.lib.fdlp_nnet_plan_info(None, None, None, None, None, None, None))


def test_round_ark_rule():
    from speech_recognition_tools_amd.nnet import round_ark
    v = np.array([0.0005, 0.0015, -0.0004, 1.23449, -7.0006, 123.4565], dtype=np.float32)
    want = (np.rint(v.astype(np.float64) * 1e3) / 1e3).astype(np.float32)
    assert_bits_equal(round_ark(v, 3), want)
    assert_bits_equal(round_ark(v, -1), v)
    assert np.signbit(round_ark(v, 3)[2])                               # -0.0, as nearbyint gives it


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_self_check(name):
    """the fixtures and the propagated bound agree before any GPU is involved: torch's CPU float32 forward of the
    reference's class lies within E of the float64 forward pass of the same weights"""
    meta, z, ws, bs = load_nnet_golden(name)
    assert len(ws) == meta["num_layers"] + 1
    assert ws[0].shape[1] == meta["feature_dim"] * meta["num_frames"] and ws[-1].shape[0] == meta["num_classes"]
    worst = 0.0
    for u in meta["utts"]:
        ys, Es = forward64(golden_rows(meta, z, u), ws, bs)
        stored = [z["tap%d_%s" % (i, u)] for i in range(meta["num_layers"])] + [z["logits_" + u]]
        for y, E, g in zip(ys, Es, stored):
            assert g.dtype == np.float32 and g.shape == y.shape
            err = np.abs(g.astype(np.float64) - y)
            worst = max(worst, float((err / E).max()))
            assert np.all(err <= E)
        assert np.all(np.abs(z["logits3_" + u] - z["logits_" + u]) <= 0.0005 + 1e-6)
    print("%s: reference float32 forward at %.3g of E, 2E of the logits up to %.3g" % (name, worst, 2 * float(Es[-1].max())))


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def run_nnet(plan, xs, norms=None, idx=None, offsets=None, out=None, n_rows=None, **kw):
    import torch
    if offsets is None:
        host = np.concatenate(xs)
    else:
        host = np.full((n_rows, xs[0].shape[1]), np.nan, dtype=np.float32)   # rows of no utterance hold NaN
        for o, x in zip(offsets, xs):
            host[o:o + x.shape[0]] = x
    feats = torch.from_numpy(host).cuda()
    nt = torch.from_numpy(np.stack(norms)).cuda() if norms is not None else None
    if "prior" in kw and kw["prior"] is not None:
        kw["prior"] = torch.from_numpy(kw["prior"]).cuda()
    o = plan.compute(feats, [x.shape[0] for x in xs], norm=nt, norm_index=idx, offsets=offsets, out=out, **kw)
    torch.cuda.synchronize()
    return o.cpu().numpy()


def run_post(plan, xs, norms=None, idx=None):
    import torch
    feats = torch.from_numpy(np.concatenate(xs)).cuda()
    nt = torch.from_numpy(np.stack(norms)).cuda() if norms is not None else None
    o = plan.compute(feats, [x.shape[0] for x in xs], norm=nt, norm_index=idx)
    torch.cuda.synchronize()
    return o.cpu().numpy()


def split_rows(a, xs):
    ends = np.cumsum([x.shape[0] for x in xs])
    return [a[e - x.shape[0]:e] for e, x in zip(ends, xs)]


def two_norms(xs):
    """two CMVN pairs interleaved over the utterances (one pair when there is one utterance)"""
    if len(xs) < 2:
        return [PN.cmvn_norm(stats_of(np.concatenate(xs + [xs[0] + 1])), norm_vars=True)], [0] * len(xs)
    return [PN.cmvn_norm(stats_of(np.concatenate(xs[k::2])), norm_vars=True) for k in (0, 1)], [i % 2 for i in range(len(xs))]


# D, L, R, dims[1:], utterance lengths.  Dense layers see K in {1, 3, KC-1, KC, KC+1, 117, 512} and others, N in
# {1, 15, 17, 38, TN_SMALL, TN_SMALL+1, TN+1, 512}; the batches have 1, 15, 17, TM-1, TM+1 and 2 TM + 3 rows;
# n_linear is 1, 2 and 5; lengths include 1 and 2 under a context of 4.
LAYER_CASES = [
    (1, 0, 0, [1, 3, KC - 1, KC, KC + 1], [1]),                      # K = 1, 3, 31, 32 of the dense layers; 1 row
    (1, 0, 0, [1, 3, KC - 1, KC, KC + 1], [TM - 1]),
    (5, 0, 0, [17, TN_SMALL + 1, TN_SMALL, 1, 38], [15]),            # K = 17, 65, 64, 1;  N = 65, 64, 1, 38
    (5, 1, 1, [17, TN_SMALL + 1, TN_SMALL, 1, 38], [1, 2, TM, TM]),  # 2 TM + 3 rows
    (13, 4, 4, [KC + 1, 117, 512, TN + 1, 15], [17]),                # K = 33, 117, 512, 129;  N = 117, 512, 129, 15
    (13, 4, 4, [KC + 1, 117, 512, TN + 1, 15], [1, 2, 3, TM - 5]),   # TM + 1 rows, lengths under the context
    (9, 1, 1, [512, 38], [1, 60, 2, 70]),                            # n_linear 2: K = 512, N = 38
    (9, 1, 1, [40], [1, 2, 30]),                                     # n_linear 1: layer 0 alone
    (13, 4, 4, [512, 512, 512, 512, 38], [1, 90, 3, 106]),           # the recipe's 117 -> 4 x 512 -> 38, 200 rows
]


@pytest.mark.gpu
@pytest.mark.parametrize("D,L,R,widths,lens", LAYER_CASES)
def test_gpu_every_layer_against_its_own_input(D, L, R, widths, lens):
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig, PostPlan
    rng = np.random.default_rng(D * 1000 + sum(widths) + sum(lens))
    cfg = PostConfig(dim=D, left_context=L, right_context=R)
    dims = [D * (L + R + 1)] + widths
    ws, bs = make_net(rng, dims)
    xs = [ark_like(rng, T, D, 2.0 * (i % 2)) for i, T in enumerate(lens)]
    norms, idx = two_norms(xs)
    rows = sum(lens)
    plan = NnetPlan(cfg, ws, bs, max_rows=rows)
    assert plan.dims == dims
    prev = run_post(PostPlan(cfg), xs, norms, idx)                   # the float32 rows entering the network
    for i, (a, x) in enumerate(zip(split_rows(prev, xs), xs)):
        assert_bits_equal(a, PN.post(x, norms[idx[i]], True, 0, 2, 0, L, R), "rows entering the network")
    n = len(widths)
    for l in range(n):
        got = run_nnet(plan, xs, norms, idx, tap=n - 1 - l)
        assert got.shape == (rows, widths[l])
        A = prev if l == 0 else np.maximum(prev, 0.0)
        ref, bound = layer_ref_and_bound(A, ws[l], bs[l])
        err = np.abs(got.astype(np.float64) - ref)
        print("layer %d, K %d N %d rows %d: max err %.3g, max err/bound %.3g"
              % (l, dims[l], widths[l], rows, float(err.max()), float((err / bound).max())))
        assert np.all(err <= bound), (l, float((err - bound).max()))
        prev = got


def chain_f32(a, W, b, order):
    """acc = fl32(a[k] W[n][k] + acc) over k in `order`, then fl32(acc + b[n]), for integer-valued data: every exact
    sum below is an integer under 2^53, so the float64 arithmetic is exact and each step rounds once, to float32"""
    acc = np.zeros((a.shape[0], W.shape[0]), dtype=np.float32)
    a64, W64 = a.astype(np.float64), W.astype(np.float64)
    for k in order:
        acc = (np.outer(a64[:, k], W64[:, k]) + acc.astype(np.float64)).astype(np.float32)
    return (acc.astype(np.float64) + b.astype(np.float64)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [70, 64])
def test_gpu_dense_chain_order_is_the_documented_one(K):
    """include/fdlp.h and DESIGN.md 7e give the k order of a dense result; integers large enough to round in
    float32 make the order visible, and layer 0 as the identity hands them to the dense layer unchanged"""
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    rng = np.random.default_rng(K)
    N, rows = 45, 19
    x = rng.integers(-2048, 2048, (rows, K)).astype(np.float32)
    W1 = rng.integers(-2048, 2048, (N, K)).astype(np.float32)
    b1 = rng.integers(-2048, 2048, N).astype(np.float32)
    plan = NnetPlan(PostConfig(dim=K), [np.eye(K, dtype=np.float32), W1], [np.zeros(K, dtype=np.float32), b1],
                    max_rows=rows)
    assert_bits_equal(run_nnet(plan, [x], tap=1), x, "layer 0 as the identity")
    got = run_nnet(plan, [x])
    order = [k for g in range(0, -(-K // KC) * KC, 8) for i in range(4) for k in (g + i, g + 4 + i) if k < K]
    assert sorted(order) == list(range(K))
    a = np.maximum(x, 0.0)
    assert_bits_equal(got, chain_f32(a, W1, b1, order), "the documented order")
    assert not np.array_equal(bits(got), bits(chain_f32(a, W1, b1, range(K)))), "the data does not show the order"


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDENS)
def test_gpu_against_reference_goldens(name):
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    meta, z, ws, bs = load_nnet_golden(name)
    cfg = PostConfig(dim=meta["feature_dim"], left_context=meta["left"], right_context=meta["right"])
    xs = [z["in_" + u] for u in meta["utts"]]
    norms = [PN.cmvn_norm(z["stats"], norm_vars=False)] if meta["feat_type"] == "cmvn" else None
    plan = NnetPlan(cfg, ws, bs, max_rows=sum(x.shape[0] for x in xs))
    n = meta["num_layers"] + 1
    got = [split_rows(run_nnet(plan, xs, norms, None, norm_vars=False, tap=n - 1 - l), xs) for l in range(n)]
    for ui, u in enumerate(meta["utts"]):
        _, Es = forward64(golden_rows(meta, z, u), ws, bs)
        stored = [z["tap%d_%s" % (i, u)] for i in range(meta["num_layers"])] + [z["logits_" + u]]
        for l in range(n):
            err = np.abs(got[l][ui].astype(np.float64) - stored[l].astype(np.float64))
            print("%s %s layer %d: max err %.3g, max err/2E %.3g" % (name, u, l, float(err.max()),
                                                                    float((err / (2 * Es[l])).max())))
            assert np.all(err <= 2 * Es[l]), (u, l)


def epilogue_logits(C):
    """a one-layer network 2 -> C whose input rows choose the logits: W[:, 0] a random pattern, W[:, 1] picks
    logit 0, no bias.  Rows: constant, the pattern, logit 0 200 above the rest, the pattern spread past +-1e4, both."""
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    rng = np.random.default_rng(C)
    W = np.zeros((C, 2), dtype=np.float32)
    W[:, 0] = rng.standard_normal(C)
    W[0, 1] = 1.0
    x = np.array([[0, 0], [1, 0], [0, 200], [6000, 0], [-6000, 0], [2.5, 200], [40, -7]], dtype=np.float32)
    plan = NnetPlan(PostConfig(dim=2), [W], [np.zeros(C, dtype=np.float32)], max_rows=x.shape[0])
    return plan, x, run_nnet(plan, [x])


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 38, 65, 2000])
def test_gpu_softmax_epilogue(C):
    plan, x, logits = epilogue_logits(C)
    assert logits.shape == (x.shape[0], C) and np.all(logits[0] == 0)
    if C >= 2:
        assert logits[2, 0] == 200 and np.all(logits[2, 1:] == 0)        # np.exp(200) overflows float32: NaN there
    if C >= 38:
        assert min(logits[3].min(), logits[4].min()) <= -1e4             # logits down to -1e4
    got = run_nnet(plan, [x], mode="softmax")
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    x64 = logits.astype(np.float64)
    m = x64.max(1, keepdims=True)
    e = np.exp(x64 - m)
    ref = e / e.sum(1, keepdims=True)
    T = (m - x64).max(1, keepdims=True)
    err = np.abs(got.astype(np.float64) - ref)
    bound = (C + 8 + T) * 2.0 ** -23 * ref + 1e-37
    print("softmax C %d: max err/bound %.3g" % (C, float((err / bound).max())))
    assert np.all(err <= bound)
    assert np.all(np.abs(got.astype(np.float64).sum(1) - 1.0) <= C * 2.0 ** -23)
    assert_bits_equal(got[0], np.full(C, np.float32(1.0) / np.float32(C), dtype=np.float32), "a constant row")
    # raw mode is the default and leaves the logits alone; softmax of a hidden layer is refused
    assert_bits_equal(run_nnet(plan, [x], mode="raw"), logits)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 38, 65, 2000])
def test_gpu_loglike_epilogue(C):
    plan, x, logits = epilogue_logits(C)
    rng = np.random.default_rng(C + 1)
    prior = np.log(rng.dirichlet(np.ones(C))).astype(np.float32)
    for w in (0.8, 0.2):
        got = run_nnet(plan, [x], mode="loglike", prior=prior, prior_weight=w)
        assert np.all(np.isfinite(got))
        x64, w32 = logits.astype(np.float64), float(np.float32(w))
        m = x64.max(1, keepdims=True)
        S = np.exp(x64 - m).sum(1, keepdims=True)
        ref = x64 - m - np.log(S) - w32 * prior.astype(np.float64)
        bound = (C + 16 + 2 * np.abs(x64 - m) + np.abs(np.log(S)) + np.abs(w32 * prior.astype(np.float64))) * 2.0 ** -23
        err = np.abs(got.astype(np.float64) - ref)
        print("loglike C %d w %.1f: max err/bound %.3g" % (C, w, float((err / bound).max())))
        assert np.all(err <= bound)


@pytest.mark.gpu
def test_gpu_mode_and_tap_refusals():
    import torch
    from speech_recognition_tools_amd._lib import FDLP_E_CAPACITY, FDLP_E_INVALID, FdlpError
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    rng = np.random.default_rng(5)
    ws, bs = make_net(rng, [4, 6, 3])
    plan = NnetPlan(PostConfig(dim=4), ws, bs, max_rows=8)
    x = ark_like(rng, 5, 4)
    with pytest.raises(FdlpError) as e:
        run_nnet(plan, [x], tap=1, mode="softmax")
    assert e.value.code == FDLP_E_INVALID and "tap" in str(e.value)
    with pytest.raises(ValueError):
        run_nnet(plan, [x], tap=2)
    with pytest.raises(ValueError):
        run_nnet(plan, [x], mode="loglike")                          # no prior
    with pytest.raises(ValueError):
        run_nnet(plan, [x], mode="logsoftmax")
    with pytest.raises(FdlpError) as e:
        run_nnet(plan, [ark_like(rng, 9, 4)])
    assert e.value.code == FDLP_E_CAPACITY and "9" in str(e.value) and "8" in str(e.value)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def indep():
    """13 columns, context 4, 117 -> 130 -> 70 -> 20: two column tiles in layer 1, both dense instantiations"""
    rng = np.random.default_rng(40)
    Ts = [1, 1, 7, 300, 2, 129, 128, 127, 3, 64]
    xs = [ark_like(rng, T, 13, 1.5 * (i % 2)) for i, T in enumerate(Ts)]
    norms = [PN.cmvn_norm(stats_of(np.concatenate(xs[k::2])), norm_vars=True) for k in (0, 1)]
    idx = [i % 2 for i in range(len(xs))]
    ws, bs = make_net(rng, [117, 130, 70, 20])
    return xs, norms, idx, ws, bs


@pytest.mark.gpu
def test_gpu_rows_do_not_depend_on_the_batch(indep):
    import torch
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    xs, norms, idx, ws, bs = indep
    cfg = PostConfig(dim=13, left_context=4, right_context=4)
    rows = sum(x.shape[0] for x in xs)
    plan = NnetPlan(cfg, ws, bs, max_rows=rows + 400)
    # the NaN batch runs first, so that NaNs are what the workspaces and the LDS hold afterwards
    xn = [np.full_like(x, np.nan) if i % 2 else x for i, x in enumerate(xs)]
    gn = run_nnet(plan, xn, norms, idx)
    gn2 = run_nnet(plan, xn, norms, idx, tap=2)
    SENT = np.float32(-12345.5)
    out = torch.full((rows + 5, 20), float(SENT), dtype=torch.float32, device="cuda")
    got = run_nnet(plan, xs, norms, idx, out=out)
    assert np.all(got[rows:] == SENT), "rows after the batch were written"
    got = got[:rows]
    assert np.all(np.isfinite(got))
    assert_bits_equal(run_nnet(plan, xs, norms, idx), got, "two calls")
    for i, (a, b, a2) in enumerate(zip(split_rows(gn, xs), split_rows(got, xs), split_rows(gn2, xs))):
        if i % 2:
            assert np.all(np.isnan(a2)), "layer 0 of a NaN utterance"
        else:
            assert_bits_equal(a, b, "neighbour of a NaN utterance")
    per = split_rows(got, xs)
    for g, x, k in zip(per, xs, idx):                                 # the utterance alone
        assert_bits_equal(run_nnet(plan, [x], [norms[k]], None), g, "one per call")
    for pre in (1, 17, 127):                                         # after prefixes of other lengths
        both = run_nnet(plan, [xs[5][:pre], xs[3]], norms, [idx[5], idx[3]])
        assert_bits_equal(both[pre:], per[3], "after a prefix of %d rows" % pre)
    # at offsets that move the utterances across the row tiles, with rows of no utterance in between
    offs = [5, 5 + 300 + 120, 5 + 300 + 120 + 129 + 1]
    sel = [3, 5, 7]
    n_rows = offs[-1] + 127 + 9
    o = run_nnet(plan, [xs[i] for i in sel], norms, [idx[i] for i in sel], offsets=offs, n_rows=n_rows)
    for off, i in zip(offs, sel):
        assert_bits_equal(o[off:off + xs[i].shape[0]], per[i], "at offset %d" % off)


@pytest.mark.gpu
def test_gpu_taps_do_not_depend_on_later_layers(indep):
    """a layer's values are the same whether or not later layers exist or are asked for: every tap of the full
    network equals, bit for bit, the output of the network cut after that layer"""
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    xs, norms, idx, ws, bs = indep
    cfg = PostConfig(dim=13, left_context=4, right_context=4)
    rows = sum(x.shape[0] for x in xs)
    plan = NnetPlan(cfg, ws, bs, max_rows=rows)
    full = run_nnet(plan, xs, norms, idx)
    for l in (0, 1):
        tap = run_nnet(plan, xs, norms, idx, tap=2 - l)
        cut = NnetPlan(cfg, ws[:l + 1], bs[:l + 1], max_rows=rows)
        assert_bits_equal(run_nnet(cut, xs, norms, idx), tap, "layer %d" % l)
    assert_bits_equal(run_nnet(plan, xs, norms, idx), full, "after the taps")


CHECKS_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import test_nnet as TN_
from speech_recognition_tools_amd.nnet import NnetPlan
from speech_recognition_tools_amd.plan import device_checks
from speech_recognition_tools_amd.post import PostConfig
assert device_checks(reset=True)[0], "not a checks build"
rng = np.random.default_rng(2)
D, L, R, widths, lens = TN_.CHECK_CASE
ws, bs = TN_.make_net(rng, [D * (L + R + 1)] + widths)
xs = [TN_.ark_like(rng, T, D) for T in lens]
norms, idx = TN_.two_norms(xs)
plan = NnetPlan(PostConfig(dim=D, left_context=L, right_context=R), ws, bs, max_rows=sum(lens))
prior = np.log(rng.dirichlet(np.ones(widths[-1]))).astype(np.float32)
runs = 0
for kw in (dict(), dict(tap=1), dict(tap=2), dict(mode="softmax"), dict(mode="loglike", prior=prior)):
    assert np.all(np.isfinite(TN_.run_nnet(plan, xs, norms, idx, **kw)))
    runs += 1
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": runs}))
"""
CHECK_CASE = (5, 1, 1, [TN_SMALL + 1, KC + 1, 38], [1, 2, TM, 9])    # both instantiations, k and row tails


@pytest.mark.gpu
def test_gpu_device_range_checks_silent():
    """the FDLP_DEVICE_CHECKS build of dense_kernel and row_epilogue_kernel: LDS and global indices stay in range"""
    lib = os.path.join(ROOT, "speech_recognition_tools_amd", "lib", "libfdlp_checks.so")
    assert os.path.exists(lib), "build() compiles libfdlp_checks.so"
    r = subprocess.run([sys.executable, "-c", CHECKS_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=dict(os.environ, FDLP_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["enabled"] and res["runs"] == 5
    assert res["violations"] == 0, res


# ---------------------------------------------------------------------------------------------
# the command, in child processes
# ---------------------------------------------------------------------------------------------
def _write_feats(d, name, items):
    from speech_recognition_tools_amd.post import FeatWriter
    w = FeatWriter("ark,scp:%s/%s.ark,%s/%s.scp" % (d, name, d, name))
    for k, m in items:
        w.write(k, m)
    w.close()
    return "%s/%s.scp" % (d, name)


def _read_scp(path):
    from speech_recognition_tools_amd.cmvn import MatReader
    return [(k, m.copy()) for k, m in MatReader("scp:" + path)]


def _cli(args, timeout=300):
    return subprocess.run([os.path.join(BIN, "extract-posterior")] + [str(a) for a in args], capture_output=True,
                          text=True, timeout=timeout)


@pytest.fixture(scope="module")
def cli_small(tmp_path_factory):
    """nnet_small as the files the command reads: checkpoint, egs.config (cmvn + splice), stats, feats, prior"""
    from speech_recognition_tools_amd.cmvn import write_kaldi_dmatrix
    d = str(tmp_path_factory.mktemp("cli_small"))
    meta, z, ws, bs = load_nnet_golden("nnet_small")
    save_checkpoint(d + "/final.mdl", meta, ws, bs)
    write_kaldi_dmatrix(d + "/cmvn.stats", z["stats"])
    pickle.dump({"feat_type": "cmvn," + d + "/cmvn.stats", "concat_feats": "%d,%d" % (meta["left"], meta["right"])},
                open(d + "/egs.config", "wb"))
    utts = [(u, z["in_" + u]) for u in meta["utts"]]
    scp = _write_feats(d, "feats", utts)
    prior = np.log(np.random.default_rng(3).dirichlet(np.ones(meta["num_classes"])))
    pickle.dump(prior, open(d + "/prior.pkl", "wb"))
    return dict(d=d, meta=meta, z=z, ws=ws, bs=bs, utts=utts, scp=scp, prior=prior.astype(np.float32))


def _expected(c, **kw):
    """NnetPlan.compute of the fixture's utterances, per utterance"""
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    meta = c["meta"]
    xs = [x for _, x in c["utts"]]
    plan = NnetPlan(PostConfig(dim=meta["feature_dim"], left_context=meta["left"], right_context=meta["right"]),
                    c["ws"], c["bs"], max_rows=sum(x.shape[0] for x in xs))
    norms = [PN.cmvn_norm(c["z"]["stats"], norm_vars=False)]
    return split_rows(run_nnet(plan, xs, norms, None, norm_vars=False, **kw), xs)


@pytest.mark.gpu
def test_gpu_cli_logits_and_batches(cli_small):
    from speech_recognition_tools_amd.nnet import round_ark
    c, d = cli_small, cli_small["d"]
    r = _cli([d + "/final.mdl", c["scp"], d + "/egs.config", d + "/post"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr.strip().splitlines()[-1] == "LOG (extract-posterior) Extracted posteriors for 4 utterances, errors on 0"
    got = _read_scp(d + "/post.scp")
    assert [k for k, _ in got] == [k for k, _ in c["utts"]]              # keys and order of the scp
    assert os.path.exists(d + "/post.ark") and not [f for f in os.listdir(d) if f.endswith(".tmp")]
    want = _expected(c)
    for (k, g), w in zip(got, want):
        assert_bits_equal(g, round_ark(w, 3), k)                        # the stated rounding, bit for bit
        _, Es = forward64(golden_rows(c["meta"], c["z"], k), c["ws"], c["bs"])
        assert np.all(np.abs(g.astype(np.float64) - c["z"]["logits3_" + k]) <= 0.001 + 2 * Es[-1]), k
    # several batches, one utterance (70 frames) longer than a batch: byte-identical files
    r = _cli([d + "/final.mdl", "scp:" + c["scp"], d + "/egs.config", d + "/post_b", "--batch-rows", "24"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(d + "/post_b.ark", "rb").read() == open(d + "/post.ark", "rb").read()


@pytest.mark.gpu
def test_gpu_cli_float32_values_to_an_ark_specifier(cli_small):
    """--ark_precision -1 keeps the float32 values; an rspecifier for the scp and an ark wspecifier as save_file"""
    from speech_recognition_tools_amd.cmvn import MatReader
    c, d = cli_small, cli_small["d"]
    r = _cli([d + "/final.mdl", "ark:" + d + "/feats.ark", d + "/egs.config", "ark:" + d + "/raw.ark",
              "--ark_precision", "-1"])
    assert r.returncode == 0, r.stderr[-2000:]
    got = [(k, m.copy()) for k, m in MatReader("ark:" + d + "/raw.ark")]
    assert [k for k, _ in got] == [k for k, _ in c["utts"]] and not os.path.exists(d + "/raw.ark.scp")
    for (k, g), w in zip(got, _expected(c)):
        assert_bits_equal(g, w, k)


@pytest.mark.gpu
@pytest.mark.parametrize("layer", [1, 2])
def test_gpu_cli_hidden_layers(cli_small, layer):
    from speech_recognition_tools_amd.nnet import round_ark
    c, d = cli_small, cli_small["d"]
    out = "%s/hid%d" % (d, layer)
    r = _cli([d + "/final.mdl", c["scp"], d + "/egs.config", out, "--layer", layer, "--add_softmax"])
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = _read_scp(out + ".scp"), _expected(c, tap=layer)
    for (k, g), w in zip(got, want):
        assert g.shape == (w.shape[0], 40)
        assert_bits_equal(g, round_ark(w, 3), k)                        # --add_softmax applies to layer 0 only
        _, Es = forward64(golden_rows(c["meta"], c["z"], k), c["ws"], c["bs"])
        gold = c["z"]["tap%d_%s" % (2 - layer, k)]                      # embeds[-layer], not rounded to 3 decimals
        # the ark's rounding moves a value by at most 0.0005, its float32 storage by |v| 2^-24 < 1e-6 for |v| < 16
        assert np.all(np.abs(g.astype(np.float64) - gold) <= 0.0005 + 1e-6 + 2 * Es[2 - layer]), k


@pytest.mark.gpu
def test_gpu_cli_softmax_and_prior(cli_small):
    from speech_recognition_tools_amd.nnet import round_ark
    c, d = cli_small, cli_small["d"]
    r = _cli([d + "/final.mdl", c["scp"], d + "/egs.config", d + "/sm", "--add_softmax"])
    assert r.returncode == 0, r.stderr[-2000:]
    for (k, g), w in zip(_read_scp(d + "/sm.scp"), _expected(c, mode="softmax")):
        assert_bits_equal(g, round_ark(w, 3), k)
        assert np.all(np.abs(g.sum(1) - 1.0) <= 10 * 0.0005 + 1e-6)
    r = _cli([d + "/final.mdl", c["scp"], d + "/egs.config", d + "/ll", "--prior", d + "/prior.pkl", "--prior_weight",
              "0.2"])
    assert r.returncode == 0, r.stderr[-2000:]
    for (k, g), w in zip(_read_scp(d + "/ll.scp"), _expected(c, mode="loglike", prior=c["prior"], prior_weight=0.2)):
        assert_bits_equal(g, round_ark(w, 3), k)


@pytest.mark.gpu
def test_gpu_cli_pca_and_raw_feat_types(tmp_path):
    from speech_recognition_tools_amd.nnet import NnetPlan, round_ark
    from speech_recognition_tools_amd.post import PostConfig, XformPlan
    import torch
    d = str(tmp_path)
    rng = np.random.default_rng(21)
    # pca,<mat>: transform-feats 12 -> 9 BEFORE the splice, then nnet_small's network
    meta, z, ws, bs = load_nnet_golden("nnet_small")
    save_checkpoint(d + "/small.mdl", meta, ws, bs)
    M = (rng.standard_normal((9, 12)) / 3.0).astype(np.float32)
    from test_transform import write_fm
    write_fm(d + "/pca.mat", M)
    pickle.dump({"feat_type": "pca," + d + "/pca.mat", "concat_feats": "1,1"}, open(d + "/egs_pca", "wb"))
    utts = [("a", ark_like(rng, 31, 12)), ("b", ark_like(rng, 1, 12)), ("c", ark_like(rng, 50, 12))]
    scp = _write_feats(d, "f12", utts)
    r = _cli([d + "/small.mdl", scp, d + "/egs_pca", d + "/pca"])
    assert r.returncode == 0, r.stderr[-2000:]
    lens = [x.shape[0] for _, x in utts]
    feats = torch.from_numpy(np.concatenate([x for _, x in utts])).cuda()
    mid = XformPlan(PostConfig(dim=12), 9, False).compute(feats, lens, torch.from_numpy(M).cuda())
    want = NnetPlan(PostConfig(dim=9, left_context=1, right_context=1), ws, bs, max_rows=sum(lens)).compute(mid, lens)
    torch.cuda.synchronize()
    got = _read_scp(d + "/pca.scp")
    assert [k for k, _ in got] == ["a", "b", "c"]
    for (k, g), w in zip(got, split_rows(want.cpu().numpy(), [x for _, x in utts])):
        assert_bits_equal(g, round_ark(w, 3), k)
    # None: raw features (nnet_tiny), against the golden as well
    meta, z, ws, bs = load_nnet_golden("nnet_tiny")
    save_checkpoint(d + "/tiny.mdl", meta, ws, bs)
    pickle.dump({"feat_type": None, "concat_feats": None}, open(d + "/egs_raw", "wb"))
    scp = _write_feats(d, "f5", [(u, z["in_" + u]) for u in meta["utts"]])
    r = _cli([d + "/tiny.mdl", scp, d + "/egs_raw", d + "/tiny"])
    assert r.returncode == 0, r.stderr[-2000:]
    for k, g in _read_scp(d + "/tiny.scp"):
        _, Es = forward64(golden_rows(meta, z, k), ws, bs)
        assert np.all(np.abs(g.astype(np.float64) - z["logits3_" + k]) <= 0.001 + 2 * Es[-1]), k


@pytest.mark.gpu
def test_gpu_cli_failures_leave_nothing_behind(cli_small, tmp_path):
    from speech_recognition_tools_amd.cmvn import write_kaldi_dmatrix
    c, d, t = cli_small, cli_small["d"], str(tmp_path)
    r = _cli([t + "/absent.mdl", c["scp"], d + "/egs.config", t + "/o1"])
    assert r.returncode != 0 and "absent.mdl" in r.stderr, r.stderr[-2000:]
    write_kaldi_dmatrix(t + "/bad.stats", np.ones((2, 12)))              # 11 columns of stats for 9 of features
    pickle.dump({"feat_type": "cmvn," + t + "/bad.stats", "concat_feats": "1,1"}, open(t + "/egs_bad", "wb"))
    r = _cli([d + "/final.mdl", c["scp"], t + "/egs_bad", t + "/o2"])
    assert r.returncode != 0 and "bad.stats" in r.stderr and "2 x 12" in r.stderr, r.stderr[-2000:]
    assert sorted(os.listdir(t)) == ["bad.stats", "egs_bad"]             # no output, partial or temporary
