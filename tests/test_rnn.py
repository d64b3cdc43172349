"""dump-genclassifier-outputs: the GRU acoustic models after the chain (speech_recognition_tools_amd/rnn.py,
gru_scan_kernel of csrc/fdlp_nnet.hip, the input projections in xform_kernel and dense_kernel).

Bounds, none of them fitted to what the device gives (U = 2^-24):

  * a GRU stage, every step against ITS OWN input (tests/gru_numpy.gru_step_ref_and_bound): x_t is the stage
    below, tapped, h_{t-1} this stage's own tapped output, so no error propagates through time or depth.  With
    e_i = (K + 2) U (|x| |W_ih|^T + |b_ih|), e_h = (H + 2) U (|h| |W_hh|^T + |b_hh|) the dot-product bound
    tests/test_nnet.py uses, q = W_hn h + b_hn and a_r, a_z, a_n the gate arguments:
        dr = (e_i,r + e_h,r + 2U |a_r|) / 4 + 8U, dz likewise            (s' <= 1/4; 8U: a few-ulp expf and the division)
        dn = e_i,n + r e_h,n + (|q| + e_h,n) dr + 2U (|a_n| + |r q|) + 8U   (tanh' <= 1)
        dh = (|n - h| + dn) dz + (1 - z) dn + 4U (|n| + |h|)
    A numpy float32 forward sits at 0.01-0.07 of dh; a wrong gate, stale state or misplaced row is >= 1e-2.
  * a linear stage: test_nnet.layer_ref_and_bound;
  * against the reference (tests/golden/rnn_*.npz, the float64 forward of the reference's model classes):
    16 x d32, d32 the reference's own float32-vs-float64 gap from the fixture's meta; 16 because a gh element here
    is one sequential K-term chain where torch's BLAS adds blocked partial sums;
  * softmax and loglike: the bounds of tests/test_nnet.py, on the device's own logits.
Every claim of independence (group, slot, other lengths, batch, taps) is asserted bitwise.
"""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import gru_numpy as GN
import post_numpy as PN
import test_nnet as TN_
from conftest import GOLDEN, ROOT
from test_nnet import ark_like, assert_bits_equal, layer_ref_and_bound, split_rows, stats_of, two_norms

BIN = os.path.join(ROOT, "bin")
GU = 32          # kGruGU: utterances per group of gru_scan_kernel
KC = 32          # dense_kernel's k chunk
GKC = 16         # gru_scan_kernel's k chunk
U = 2.0 ** -24
GOLDENS = ["rnn_noae", "rnn_normal", "rnn_tiny"]


def make_stages(rng, k0, spec, gain=3.0):
    """spec: [(kind, width)]; weights U(-1, 1) gain / sqrt(width), torch's init times `gain` (3 saturates gates)"""
    out, k = [], k0
    for kind, n in spec:
        s = gain / np.sqrt(n)
        if kind == "gru":
            out.append(("gru", (rng.uniform(-s, s, (3 * n, k))).astype(np.float32),
                        (rng.uniform(-s, s, (3 * n, n))).astype(np.float32),
                        (rng.uniform(-s, s, 3 * n) / gain).astype(np.float32),
                        (rng.uniform(-s, s, 3 * n) / gain).astype(np.float32)))
        else:
            s = gain / np.sqrt(k)
            out.append((kind, rng.uniform(-s, s, (n, k)).astype(np.float32),
                        (rng.uniform(-s, s, n) / gain).astype(np.float32)))
        k = n
    return out


def golden_checkpoint(meta, z):
    from collections import OrderedDict
    import torch
    sd = OrderedDict((k[3:], torch.from_numpy(np.array(z[k]))) for k in z.files if k.startswith("sd_"))
    return dict({k: meta[k] for k in meta["header"]}, model_state_dict=sd)


def load_rnn_golden(name, tmp):
    import torch
    from speech_recognition_tools_amd.rnn import load_rnn_checkpoint
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    p = os.path.join(str(tmp), name + ".mdl")
    torch.save(golden_checkpoint(meta, z), p)
    return meta, z, load_rnn_checkpoint(p, meta["ae_type"]), p


def golden_rows(meta, z, u):
    norm = PN.cmvn_norm(z["stats"], norm_vars=True) if meta["feat_type"] == "cmvn" else None
    return PN.post(z["in_" + u], norm, norm is not None, 0, 2, 0, meta["left"], meta["right"])


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_cli_argparse_surface_matches_reference():
    from speech_recognition_tools_amd import rnn
    ref = json.load(open(os.path.join(GOLDEN, "cli_options_rnn.json")))
    assert [o["name"] for o in ref][:4] == ["model", "scp", "egs_config", "save_file"] and len(ref) == 10
    a = rnn.dump_genclassifier_outputs_parser().parse_args(["final.mdl", "feats.scp", "egs.config", "post"])
    for o in ref:
        dest = o["name"].lstrip("-")
        assert hasattr(a, dest), o
        if o["name"].startswith("--"):
            assert getattr(a, dest) == (False if o.get("action") == "store_true" else o.get("default")), o
    assert (a.model, a.scp, a.egs_config, a.save_file) == ("final.mdl", "feats.scp", "egs.config", "post")
    assert (a.ark_precision, a.batch_rows) == (3, 131072)
    a = rnn.dump_genclassifier_outputs_parser().parse_args(
        ["m", "s", "e", "o", "--ae_type", "noae", "--prior", "p", "--prior_weight", "0.2", "--add_softmax",
         "--override_trans", "cmvn_utt,x.scp", "--vae", "v", "--device", "1", "--batch-rows", "8", "--ark_precision", "-1"])
    assert (a.ae_type, a.prior, a.prior_weight, a.add_softmax, a.override_trans, a.vae, a.device, a.batch_rows,
            a.ark_precision) == ("noae", "p", 0.2, True, "cmvn_utt,x.scp", "v", 1, 8, -1)
    with pytest.raises(SystemExit):
        rnn.dump_genclassifier_outputs_parser().parse_args(["m", "s", "e"])
    assert os.access(os.path.join(BIN, "dump-genclassifier-outputs"), os.X_OK)


@pytest.mark.parametrize("ae_type", ["vae", "vaeenc", "lstm"])
def test_unsupported_model_types_exit_1(tmp_path, capsys, ae_type):
    from speech_recognition_tools_amd.rnn import main_dump_genclassifier_outputs
    rc = main_dump_genclassifier_outputs(["m", "s", "e", str(tmp_path / "out"), "--ae_type=" + ae_type])
    assert rc == 1 and "--ae_type=%s is not supported" % ae_type in capsys.readouterr().err
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("name", GOLDENS)
def test_checkpoint_round_trip(tmp_path, name):
    meta, z, c, _ = load_rnn_golden(name, tmp_path)
    assert (c.ae_type, c.feature_dim, c.num_frames, c.num_classes) == (
        meta["ae_type"], meta["feature_dim"], meta["num_frames"], meta["num_classes"])
    H = meta["hidden_dim"]
    if meta["ae_type"] == "noae":
        assert [s[0] for s in c.stages] == ["gru"] * meta["num_layers"] + ["linear"]
        assert c.dims == [meta["feature_dim"] * meta["num_frames"]] + [H] * meta["num_layers"] + [meta["num_classes"]]
        assert_bits_equal(c.stages[0][2], z["sd_layers.0.weight_hh_l0"])
        assert_bits_equal(c.stages[-1][1], z["sd_regression.weight"][:, :, 0])      # the Conv1d weight, squeezed
    else:
        ne, nc = meta["encoder_num_layers"], meta["classifier_num_layers"]
        assert [s[0] for s in c.stages] == ["gru"] * ne + ["linear_relu"] + ["gru"] * nc + ["linear"]
        assert c.dims == ([meta["feature_dim"] * meta["num_frames"]] + [H] * ne + [meta["bn_dim"]] + [H] * nc
                          + [meta["num_classes"]])
        assert any(k.startswith("sd_ae.") for k in z.files)                        # present, and ignored
        assert_bits_equal(c.stages[ne][1], z["sd_encoder.bottleneck.weight"][:, :, 0])
        assert_bits_equal(c.stages[ne + 1][1], z["sd_classifier.layers.0.weight_ih_l0"])
    for st in c.stages:
        assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in st[1:])


def test_checkpoint_errors_name_the_key(tmp_path):
    import torch
    from speech_recognition_tools_amd.rnn import load_rnn_checkpoint
    p = str(tmp_path / "m.pt")
    z = np.load(os.path.join(GOLDEN, "rnn_noae.npz"))
    meta = json.loads(str(z["meta"]))
    good = golden_checkpoint(meta, z)

    def variant(hdr=None, drop=None, put=None):
        d = dict(good, model_state_dict=dict(good["model_state_dict"]))
        d.update(hdr or {})
        for k in drop or ():
            (d if k in d else d["model_state_dict"]).pop(k)
        if put:
            d["model_state_dict"].update(put)
        torch.save(d, p)

    variant(hdr={"hidden_dim": 41})                                     # a shape that contradicts the header
    with pytest.raises(ValueError, match=r"layers\.0\.weight_ih_l0"):
        load_rnn_checkpoint(p, "noae")
    variant(put={"layers.1.bias_hh_l0": torch.zeros(119)})
    with pytest.raises(ValueError, match=r"layers\.1\.bias_hh_l0"):
        load_rnn_checkpoint(p, "noae")
    variant(put={"regression.weight": torch.zeros(10, 40, 2)})          # a Conv1d of kernel size 2
    with pytest.raises(ValueError, match=r"regression\.weight"):
        load_rnn_checkpoint(p, "noae")
    variant(hdr={"num_layers": 1})                                      # a layer beyond the header's count
    with pytest.raises(ValueError, match=r"layers\.1\."):
        load_rnn_checkpoint(p, "noae")
    variant(hdr={"num_layers": 3})
    with pytest.raises(ValueError, match=r"layers\.2\.weight_ih_l0"):
        load_rnn_checkpoint(p, "noae")
    for k in ("feature_dim", "hidden_dim", "model_state_dict", "layers.0.weight_hh_l0", "regression.bias"):
        variant(drop=[k])
        with pytest.raises(ValueError, match=k.replace(".", r"\.")):
            load_rnn_checkpoint(p, "noae")
    variant()
    with pytest.raises(ValueError, match="encoder_num_layers"):         # a noae checkpoint read as normal
        load_rnn_checkpoint(p, "normal")
    with pytest.raises(ValueError, match="vae"):
        load_rnn_checkpoint(p, "vae")
    # normal: a missing classifier key, a wrong bottleneck, ae.* of any shape ignored
    z = np.load(os.path.join(GOLDEN, "rnn_normal.npz"))
    meta = json.loads(str(z["meta"]))
    good = golden_checkpoint(meta, z)
    variant(drop=["classifier.regression.weight"])
    with pytest.raises(ValueError, match=r"classifier\.regression\.weight"):
        load_rnn_checkpoint(p, "normal")
    variant(hdr={"bn_dim": 13})
    with pytest.raises(ValueError, match=r"encoder\.bottleneck\.weight"):
        load_rnn_checkpoint(p, "normal")
    variant(hdr={"encoder_num_layers": 1})
    with pytest.raises(ValueError, match=r"encoder\.layers\.1\."):
        load_rnn_checkpoint(p, "normal")
    variant(put={"ae.layers.0.weight_ih_l0": torch.zeros(2, 2)}, drop=["ae.regression.bias"])
    assert len(load_rnn_checkpoint(p, "normal").stages) == 5
    torch.save([1, 2, 3], p)
    with pytest.raises(ValueError, match="not a dict"):
        load_rnn_checkpoint(p, "noae")
    open(p, "wb").write(b"garbage")
    with pytest.raises(ValueError, match="m.pt"):
        load_rnn_checkpoint(p, "noae")
    variant()
    blob = open(p, "rb").read()
    open(p, "wb").write(blob[:len(blob) // 2])                          # a truncated file
    with pytest.raises(ValueError, match="m.pt"):
        load_rnn_checkpoint(p, "noae")
    with pytest.raises(OSError, match="absent.pt"):
        load_rnn_checkpoint(str(tmp_path / "absent.pt"), "noae")


def test_egs_config_and_override(tmp_path):
    from speech_recognition_tools_amd.rnn import load_rnn_egs_config
    p = str(tmp_path / "egs.config")
    pickle.dump({"feat_type": "cmvn,/d/cmvn.ark", "concat_feats": "4,4"}, open(p, "wb"))
    c = load_rnn_egs_config(p)
    assert (c.feat_type, c.feat_path, c.left, c.right) == ("cmvn", "/d/cmvn.ark", 4, 4)
    c = load_rnn_egs_config(p, "cmvn_utt,/d/utt.scp")
    assert (c.feat_type, c.feat_path, c.left, c.right) == ("cmvn_utt", "/d/utt.scp", 4, 4)
    assert load_rnn_egs_config(p, "pca,/d/p.mat").feat_type == "pca"
    assert load_rnn_egs_config(p, "none").feat_type is None             # anything else is raw
    pickle.dump({"feat_type": None, "concat_feats": None}, open(p, "wb"))
    c = load_rnn_egs_config(p)
    assert (c.feat_type, c.feat_path, c.left, c.right) == (None, None, 0, 0)
    for bad in ({"feat_type": "cmvn,", "concat_feats": None}, {"feat_type": None, "concat_feats": "4"}, ["x"],
                {"feat_type": None}):
        pickle.dump(bad, open(p, "wb"))
        with pytest.raises(ValueError, match="egs.config"):
            load_rnn_egs_config(p)


RECIPE_KINDS = ["gru"] * 3 + ["linear_relu", "gru", "linear"]          # 3 enc + bn + 1 class + regression
RECIPE_DIMS = [117, 256, 256, 256, 40, 256, 1900]


def test_host_only_plan_info_and_refusals():
    from speech_recognition_tools_amd._lib import FDLP_E_INVALID, FdlpError
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    cfg = PostConfig(dim=13, left_context=4, right_context=4)
    p = RnnPlan(cfg, None, max_rows=1000, max_utts=70, device=-1, kinds=RECIPE_KINDS, dims=RECIPE_DIMS)
    assert (p.in_dim, p.n_stages, p.dims, p.out_dim, p.kinds) == (117, 6, RECIPE_DIMS, 1900, RECIPE_KINDS)
    assert p.group_utts == GU
    # G [max_rows, 3 max H], two [max_rows, widest of dims[1 .. n - 1]], ceil(max_utts / GU) groups of GU 16-byte slots
    assert p.workspace_bytes == 4 * 1000 * 3 * 256 + 2 * 4 * 1000 * 256 + 16 * GU * 3
    # slot table, two [GU, ceil(H / 16) 16 + 4] state buffers, four waves x two [96, 16 + 4] chunk buffers
    assert p.lds_bytes == 4 * (3 * GU + 2 * GU * (256 + 4) + 4 * 2 * 96 * (GKC + 4))
    assert [p.tap_dim(t) for t in range(6)] == [1900, 256, 40, 256, 256, 256]
    with pytest.raises(ValueError):
        p.tap_dim(6)
    one = RnnPlan(cfg, None, max_rows=7, max_utts=1, device=-1, kinds=["linear"], dims=[117, 5])
    assert (one.workspace_bytes, one.lds_bytes) == (16 * GU, 0)
    odd = RnnPlan(cfg, None, max_rows=3, max_utts=33, device=-1, kinds=["gru", "linear"], dims=[117, 33, 5])
    assert odd.workspace_bytes == 4 * 3 * 3 * 33 + 2 * 4 * 3 * 33 + 16 * GU * 2
    assert odd.lds_bytes == 4 * (3 * GU + 2 * GU * (48 + 4) + 4 * 2 * 96 * (GKC + 4))
    # shapes taken from the arrays
    st = make_stages(np.random.default_rng(0), 117, [("gru", 6), ("linear_relu", 4), ("gru", 5), ("linear", 3)])
    q = RnnPlan(cfg, st, max_rows=5, device=-1)
    assert (q.dims, q.kinds) == ([117, 6, 4, 5, 3], ["gru", "linear_relu", "gru", "linear"])

    def refused(*need, **kw):
        a = dict(max_rows=10, max_utts=4, device=-1, kinds=["gru", "linear"], dims=[117, 8, 3])
        a.update(kw)
        with pytest.raises(FdlpError) as e:
            RnnPlan(cfg, None, **a)
        assert e.value.code == FDLP_E_INVALID and all(n in str(e.value) for n in need), str(e.value)

    refused("kind 7", "stage 1", kinds=["gru", 7])                      # an unknown kind
    refused("117 -> 0 -> 3", dims=[117, 0, 3])                          # a dimension < 1
    refused("-4", dims=[117, 8, -4])
    refused("116", "117", dims=[116, 8, 3])                             # dims[0] is not the stages' out_dim
    refused("n_stages = 33", kinds=["linear"] * 33, dims=[117] + [4] * 33)
    refused("n_stages = 0", kinds=[], dims=[117])
    refused("max_rows", "0", max_rows=0)
    refused("max_utts", "0", max_utts=0)
    refused("400", "384", "163840", dims=[117, 400, 3])                 # a GRU too wide for the LDS
    RnnPlan(cfg, None, max_rows=10, device=-1, kinds=["gru", "linear"], dims=[117, 384, 3])


FF_KINDS = ["linear_relu", "linear_relu", "linear"]                    # a feed-forward net as stages


def test_feedforward_net_is_the_linear_only_stage_plan():
    """one plan behind both fronts: the same shapes, and workspaces that differ by the group table alone"""
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    cfg, dims = PostConfig(dim=13, left_context=4, right_context=4), [117, 70, 9, 5]
    for max_rows, max_utts in ((1000, 70), (7, 1), (33, GU), (33, GU + 1)):
        a = NnetPlan(cfg, None, None, max_rows=max_rows, device=-1, dims=dims)
        b = RnnPlan(cfg, None, max_rows=max_rows, max_utts=max_utts, device=-1, kinds=FF_KINDS, dims=dims)
        assert a.dims == b.dims == dims and a.n_linear == b.n_stages == 3 and b.kinds == FF_KINDS
        assert [a.tap_dim(t) for t in range(3)] == [b.tap_dim(t) for t in range(3)] == [5, 9, 70]
        assert a.workspace_bytes == 2 * 4 * max_rows * 70
        assert b.workspace_bytes - a.workspace_bytes == 16 * GU * -(-max_utts // GU)
        assert b.lds_bytes == 0                                         # no scan


def test_group_table():
    from speech_recognition_tools_amd._lib import FDLP_E_INVALID, FdlpError
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    p = RnnPlan(PostConfig(dim=4), None, max_rows=500, max_utts=64, device=-1, kinds=["gru"], dims=[4, 3])
    lens = [5, 1, 9, 9, 2] + [3] * GU
    n = len(lens)
    g, s, ng = p.groups(lens)
    assert ng == -(-n // GU) == 2
    pos = g.astype(np.int64) * GU + s
    assert sorted(pos.tolist()) == list(range(n))                       # every utterance exactly once, groups filled
    order = np.argsort(pos)
    sorted_lens = [lens[i] for i in order]
    assert all(a >= b for a, b in zip(sorted_lens, sorted_lens[1:]))    # lengths do not increase across (group, slot)
    for L in set(lens):                                                 # equal lengths keep their input order
        same = [i for i in order if lens[i] == L]
        assert same == sorted(same)
    assert (g[2], s[2], g[3], s[3]) == (0, 0, 0, 1) and g[1] == 1 and s[1] == n - GU - 1
    assert p.groups([])[2] == 0 and p.groups([7])[2] == 1
    with pytest.raises(FdlpError) as e:
        p.groups([3, 0, 2])                                             # a zero-length utterance
    assert e.value.code == FDLP_E_INVALID and "utterance 1" in str(e.value) and "length 0" in str(e.value)


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_self_check(tmp_path, name):
    """the restatement and the fixtures agree before any GPU is involved: gru_numpy in float64 reproduces the real
    classes' float64 outputs at every stage, and in float32 stays within 4 x d32"""
    meta, z, c, _ = load_rnn_golden(name, tmp_path)
    d32 = meta["d32"]
    assert 0 < d32 <= 1e-5
    w64 = w32 = 0.0
    for u in meta["utts"]:
        rows = golden_rows(meta, z, u)
        o64, o32 = GN.forward(rows, c.stages, np.float64), GN.forward(rows, c.stages, np.float32)
        assert len(o64) == len(c.stages)
        for i, (a, b) in enumerate(zip(o64, o32)):
            ref = z["stage%d_%s" % (i, u)]
            assert ref.dtype == np.float64 and ref.shape == a.shape and b.dtype == np.float32
            w64 = max(w64, float(np.abs(a - ref).max()))
            w32 = max(w32, float(np.abs(b - ref).max()))
        assert np.array_equal(z["stage%d_%s" % (len(c.stages) - 1, u)], z["f64_" + u])
        assert float(np.abs(z["f32_" + u] - z["f64_" + u]).max()) <= d32
        assert np.all(np.abs(z["logits3_" + u] - z["f32_" + u]) <= 0.0005 + 1e-6)
    print("%s: float64 restatement within %.3g, float32 within %.3g = %.2f d32" % (name, w64, w32, w32 / d32))
    assert w64 <= 1e-12 and w32 <= 4 * d32


def test_entry_points_are_declared_and_exported():
    import ctypes
    import re
    from speech_recognition_tools_amd import _lib
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    names = ["fdlp_rnn_plan_create", "fdlp_rnn_plan_destroy", "fdlp_rnn_plan_info", "fdlp_rnn_plan_groups",
             "fdlp_rnn_compute", "fdlp_rnn_set_profiling", "fdlp_rnn_times"]
    src = open(os.path.join(ROOT, "include", "fdlp.h")).read()
    declared = set(re.findall(r"\b(fdlp_[a-z0-9_]+)\s*\(", src))
    for n in names:
        assert n in declared and n in _lib.SIGNATURES and hasattr(_lib.lib, n), n
    assert "#define FDLP_ABI_VERSION 13" in src and _lib.lib.fdlp_abi_version() == 13
    assert "#define FDLP_RNN_MAX_STAGES 32" in src and _lib.FDLP_RNN_MAX_STAGES == 32
    p = RnnPlan(PostConfig(dim=4), None, device=-1, kinds=["gru"], dims=[4, 3])
    with pytest.raises(_lib.FdlpError, match="host-only"):               # a host-only plan refuses to compute
        _lib.check(_lib.lib.fdlp_rnn_compute(p._h, ctypes.byref(_lib.FdlpPostBatchC()), 0, 0, None, 0.8, None))
    with pytest.raises(_lib.FdlpError):
        _lib.check(_lib.lib.fdlp_rnn_plan_info(None, None, None, None, None, None, None))


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def run_rnn(plan, xs, norms=None, idx=None, **kw):
    import torch
    feats = torch.from_numpy(np.concatenate(xs)).cuda()
    nt = torch.from_numpy(np.stack(norms)).cuda() if norms is not None else None
    if kw.get("prior") is not None:
        kw["prior"] = torch.from_numpy(kw["prior"]).cuda()
    o = plan.compute(feats, [x.shape[0] for x in xs], norm=nt, norm_index=idx, **kw)
    torch.cuda.synchronize()
    return o.cpu().numpy()


def check_every_stage(what, D, L, R, spec, lens, seed):
    """GPU test 1 for one case; returns the worst err/bound over the stages"""
    from speech_recognition_tools_amd.post import PostConfig, PostPlan
    from speech_recognition_tools_amd.rnn import RnnPlan
    rng = np.random.default_rng(seed)
    cfg = PostConfig(dim=D, left_context=L, right_context=R)
    stages = make_stages(rng, D * (L + R + 1), spec)
    xs = [ark_like(rng, T, D, 2.0 * (i % 2)) for i, T in enumerate(lens)]
    norms, idx = two_norms(xs)
    rows = sum(lens)
    plan = RnnPlan(cfg, stages, max_rows=rows, max_utts=len(lens))
    prev = TN_.run_post(PostPlan(cfg), xs, norms, idx)                 # the float32 rows entering the model
    for i, (a, x) in enumerate(zip(split_rows(prev, xs), xs)):
        assert_bits_equal(a, PN.post(x, norms[idx[i]], True, 0, 2, 0, L, R), "rows entering the model")
    n, kind, worst = len(stages), None, 0.0
    for s, st in enumerate(stages):
        got = run_rnn(plan, xs, norms, idx, tap=n - 1 - s)
        assert got.shape == (rows, spec[s][1]) and np.all(np.isfinite(got))
        A = GN.stage_input(prev, kind)
        kind = st[0]
        if kind == "gru":
            pairs = [GN.gru_step_ref_and_bound(a, g, *st[1:]) for a, g in zip(split_rows(A, xs), split_rows(got, xs))]
            ref, bound = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
        else:
            ref, bound = layer_ref_and_bound(A, st[1], st[2])
        err = np.abs(got.astype(np.float64) - ref)
        ratio = float((err / bound).max())
        print("%s stage %d %s, K %d N %d, %d utterances %d rows: max err %.3g, median bound %.3g, max err/bound %.3g"
              % (what, s, kind, A.shape[1], spec[s][1], len(lens), rows, float(err.max()), float(np.median(bound)), ratio))
        assert np.all(err <= bound), (what, s, float((err - bound).max()))
        worst, prev = max(worst, ratio), got
    return worst


CYCLE = [1, 9, 4, 17]
STAGE_CASES = {
    # unit and k tails: H 33 (two unit blocks, three k chunks), in 27
    "a_tails": (9, 1, 1, [("gru", 33), ("linear", 5)], [1, 2, 37]),
    # two groups, ragged
    "b_two_groups": (5, 1, 1, [("gru", 40), ("gru", 40), ("linear", 6)], [CYCLE[i % 4] for i in range(GU + 1)]),
    # 16 k chunks, every wave owning two unit blocks; in KC + 1
    "c_h256": (KC + 1, 0, 0, [("gru", 256), ("linear", 4)], [1 + (5 * i) % 12 for i in range(GU + 1)]),
    # the `normal` topology: ReLU-on-load into a GRU's projection
    "d_normal": (9, 1, 1, [("gru", 64), ("linear_relu", 12), ("gru", 64), ("linear", 7)], [3, 11, 1, 6]),
    "e_one_frame": (9, 1, 1, [("gru", 40), ("linear", 3)], [1]),
    "f_h1": (4, 0, 0, [("gru", 1), ("gru", 1), ("linear", 3)], [6, 1, 3]),
    # the widest GRU the LDS holds: 24 k chunks, three unit blocks per wave
    "g_h384": (4, 0, 0, [("gru", 384), ("linear", 3)], [3, 1, 2]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(STAGE_CASES))
def test_gpu_every_stage_every_step_against_its_own_input(case):
    D, L, R, spec, lens = STAGE_CASES[case]
    check_every_stage(case, D, L, R, spec, lens, seed=sum(map(ord, case)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDENS)
def test_gpu_against_reference_goldens(tmp_path, name):
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    meta, z, c, _ = load_rnn_golden(name, tmp_path)
    d32 = meta["d32"]
    cfg = PostConfig(dim=meta["feature_dim"], left_context=meta["left"], right_context=meta["right"])
    xs = [z["in_" + u] for u in meta["utts"]]
    norms = [PN.cmvn_norm(z["stats"], norm_vars=True)] if meta["feat_type"] == "cmvn" else None
    plan = RnnPlan(cfg, c.stages, max_rows=sum(x.shape[0] for x in xs), max_utts=len(xs))
    n = len(c.stages)
    worst = 0.0
    for s in range(n):
        got = split_rows(run_rnn(plan, xs, norms, None, tap=n - 1 - s), xs)
        for g, u in zip(got, meta["utts"]):
            err = float(np.abs(g.astype(np.float64) - z["stage%d_%s" % (s, u)]).max())
            print("%s %s stage %d (%s): max err %.3g = %.3g d32" % (name, u, s, c.stages[s][0], err, err / d32))
            worst = max(worst, err / d32)
    assert worst <= 16, worst


def indep_case(H):
    rng = np.random.default_rng(H)
    stages = make_stages(rng, 15, [("gru", H), ("gru", H), ("linear", 5)])
    # the longest, one in the middle of the first group, one that sorts into the second group
    targets = [ark_like(rng, T, 5) for T in (12, 5, 1)]
    others = [ark_like(rng, 1 + (7 * i) % 11, 5, 1.0) for i in range(GU + 5)]
    return stages, targets, others


@pytest.mark.gpu
@pytest.mark.parametrize("H", [40, 256])
def test_gpu_an_utterance_does_not_depend_on_its_batch(H):
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    stages, targets, others = indep_case(H)
    norm = [PN.cmvn_norm(stats_of(np.concatenate(others)), norm_vars=True)]
    cfg = PostConfig(dim=5, left_context=1, right_context=1)
    rows = sum(o.shape[0] for o in others) + 2 * 12
    plan = RnnPlan(cfg, stages, max_rows=rows, max_utts=len(others) + 2)
    lens = [o.shape[0] for o in others]
    for x in targets:
        T = x.shape[0]
        g, s, _ = plan.groups(lens[:9] + [T] + lens[9:])
        g2, s2, _ = plan.groups(lens + [T])
        print("H %d, T %d: group %d slot %d inside the batch, group %d slot %d at its end" % (H, T, g[9], s[9], g2[-1], s2[-1]))
        for tap in (0, 1):
            alone = run_rnn(plan, [x], norm, tap=tap)
            assert np.all(np.isfinite(alone))

            def at(batch, k):
                o = run_rnn(plan, batch, norm, tap=tap)
                off = sum(b.shape[0] for b in batch[:k])
                return o[off:off + T]

            assert_bits_equal(at(others[:9] + [x] + others[9:], 9), alone, "inside a batch of others")
            assert_bits_equal(at([x] + others, 0), alone, "at another position: first")
            nans = [np.full_like(o, np.nan) for o in others]             # nothing of a neighbour is read
            assert_bits_equal(at(nans[:9] + [x] + nans[9:], 9), alone, "among NaN utterances")
            assert_bits_equal(at(others + [x], len(others)), alone, "at another position: last")
            rev = (others[:9] + [x] + others[9:])[::-1]
            assert_bits_equal(at(rev, len(others) - 9), alone, "the batch reversed")
            twice = [x] + others[:20] + [x] + others[20:]
            assert_bits_equal(at(twice, 0), alone, "twice in a batch: the first")
            assert_bits_equal(at(twice, 21), alone, "twice in a batch: the second (h_0 = 0, no carry-over)")
            assert_bits_equal(run_rnn(plan, [x], norm, tap=tap), alone, "a second compute on the plan")
            # the recurrence is causal: what follows reaches frame T - 1 through the splice's right context only
            longer = np.concatenate([x, others[3]])
            assert_bits_equal(run_rnn(plan, [longer], norm, tap=tap)[:T - 1], alone[:T - 1], "as a longer one's prefix")
    assert plan.groups(lens + [1])[0][-1] == 1                           # the one-frame target was in the second group


@pytest.mark.gpu
def test_gpu_taps_do_not_depend_on_later_stages():
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    rng = np.random.default_rng(8)
    stages = make_stages(rng, 15, [("gru", 40), ("linear_relu", 12), ("gru", 33), ("linear", 5)])
    xs = [ark_like(rng, T, 5) for T in (7, 1, 19, 4)]
    cfg = PostConfig(dim=5, left_context=1, right_context=1)
    rows = sum(x.shape[0] for x in xs)
    plan = RnnPlan(cfg, stages, max_rows=rows, max_utts=4)
    full = run_rnn(plan, xs)
    for l in range(3):
        cut = RnnPlan(cfg, stages[:l + 1], max_rows=rows, max_utts=4)
        assert_bits_equal(run_rnn(cut, xs), run_rnn(plan, xs, tap=3 - l), "stage %d" % l)
    assert_bits_equal(run_rnn(plan, xs), full, "after the taps")


@pytest.mark.gpu
def test_gpu_epilogues_and_refusals():
    import torch
    from speech_recognition_tools_amd._lib import FDLP_E_CAPACITY, FDLP_E_INVALID, FdlpError
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    rng = np.random.default_rng(5)
    C = 38
    stages = make_stages(rng, 4, [("gru", 20), ("linear", C)], gain=6.0)
    plan = RnnPlan(PostConfig(dim=4), stages, max_rows=40, max_utts=3)
    xs = [ark_like(rng, T, 4) for T in (9, 1, 17)]
    logits = run_rnn(plan, xs)
    x64 = logits.astype(np.float64)
    m = x64.max(1, keepdims=True)
    got = run_rnn(plan, xs, mode="softmax")
    ref = GN.softmax(logits)
    err = np.abs(got.astype(np.float64) - ref)
    bound = (C + 8 + (m - x64).max(1, keepdims=True)) * 2.0 ** -23 * ref + 1e-37
    print("softmax: max err/bound %.3g" % float((err / bound).max()))
    assert np.all(err <= bound)
    prior = np.log(rng.dirichlet(np.ones(C))).astype(np.float32)
    for w in (0.8, 0.2):
        got = run_rnn(plan, xs, mode="loglike", prior=prior, prior_weight=w)
        w32 = float(np.float32(w))
        ref = GN.loglike(logits, prior, w32)
        S = np.exp(x64 - m).sum(1, keepdims=True)
        bound = (C + 16 + 2 * np.abs(x64 - m) + np.abs(np.log(S)) + np.abs(w32 * prior.astype(np.float64))) * 2.0 ** -23
        err = np.abs(got.astype(np.float64) - ref)
        print("loglike w %.1f: max err/bound %.3g" % (w, float((err / bound).max())))
        assert np.all(err <= bound)
    assert_bits_equal(run_rnn(plan, xs, mode="raw"), logits)
    with pytest.raises(FdlpError) as e:
        run_rnn(plan, xs, tap=1, mode="softmax")                        # a mode on a hidden tap
    assert e.value.code == FDLP_E_INVALID and "tap" in str(e.value)
    with pytest.raises(ValueError):
        run_rnn(plan, xs, tap=2)                                        # a tap out of range
    with pytest.raises(ValueError):
        run_rnn(plan, xs, mode="loglike")                               # no prior
    with pytest.raises(FdlpError) as e:
        run_rnn(plan, [ark_like(rng, 2, 4)] * 4)                        # over max_utts
    assert e.value.code == FDLP_E_INVALID and "4" in str(e.value) and "max_utts 3" in str(e.value)
    with pytest.raises(FdlpError) as e:
        run_rnn(plan, [ark_like(rng, 41, 4)])                           # over max_rows
    assert e.value.code == FDLP_E_CAPACITY and "41" in str(e.value) and "40" in str(e.value)
    feats = torch.from_numpy(np.concatenate(xs)).cuda()
    with pytest.raises(FdlpError) as e:
        plan.compute(feats, [9, 0, 18])                                 # a zero-length utterance
    assert e.value.code == FDLP_E_INVALID and "utterance 1" in str(e.value)
    torch.cuda.synchronize()
    assert_bits_equal(run_rnn(plan, xs), logits, "after the refusals")


@pytest.mark.gpu
def test_gpu_feedforward_net_through_both_fronts_is_bit_identical():
    """the same network as an NnetPlan and as the stages linear_relu, linear_relu, linear of an RnnPlan: K_0 = 20,
    widths 70, 9, 5 (three layers, so both workspaces and the ReLU flag; N on both sides of 64), utterances of 1, 37
    and 130 rows (more than one 128-row tile, the last partial) with NaN rows between them.  Every tap raw, and tap 0
    in softmax and in loglike with a random prior, bit for bit."""
    from speech_recognition_tools_amd.nnet import NnetPlan
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    rng = np.random.default_rng(11)
    cfg = PostConfig(dim=5, left_context=1, right_context=2)
    ws, bs = TN_.make_net(rng, [20, 70, 9, 5])
    lens, offsets, n_rows = [1, 37, 130], [2, 5, 45], 180
    xs = [ark_like(rng, T, 5, 2.0 * (i % 2)) for i, T in enumerate(lens)]
    norms, idx = two_norms(xs)
    prior = np.log(rng.dirichlet(np.ones(5))).astype(np.float32)
    nnet = NnetPlan(cfg, ws, bs, max_rows=n_rows)
    rnn = RnnPlan(cfg, [(k, w, b) for k, w, b in zip(FF_KINDS, ws, bs)], max_rows=n_rows, max_utts=3)
    assert nnet.dims == rnn.dims == [20, 70, 9, 5]
    cases = [dict(tap=t) for t in range(3)] + [dict(mode="softmax"), dict(mode="loglike", prior=prior, prior_weight=0.3)]
    for kw in cases:
        a = TN_.run_nnet(nnet, xs, norms, idx, offsets=offsets, n_rows=n_rows, **dict(kw))
        b = TN_.run_nnet(rnn, xs, norms, idx, offsets=offsets, n_rows=n_rows, **dict(kw))
        assert a.shape == b.shape == (n_rows, nnet.tap_dim(kw.get("tap", 0)))
        for o, T in zip(offsets, lens):
            assert np.all(np.isfinite(a[o:o + T])), kw
            assert_bits_equal(a[o:o + T], b[o:o + T], "%s rows %d..%d" % (sorted(kw), o, o + T))


CHECKS_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import test_rnn as TR
from speech_recognition_tools_amd.plan import device_checks
assert device_checks(reset=True)[0], "not a checks build"
worst = [TR.check_every_stage(c, *TR.STAGE_CASES[c], seed=3) for c in TR.CHECK_CASES]
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": len(worst)}))
"""
CHECK_CASES = ["b_two_groups", "c_h256"]


@pytest.mark.gpu
def test_gpu_device_range_checks_silent():
    """the FDLP_DEVICE_CHECKS build of gru_scan_kernel (and the kernels around it): LDS and global indices in range"""
    lib = os.path.join(ROOT, "speech_recognition_tools_amd", "lib", "libfdlp_checks.so")
    assert os.path.exists(lib), "build() compiles libfdlp_checks.so"
    r = subprocess.run([sys.executable, "-c", CHECKS_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=dict(os.environ, FDLP_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["enabled"] and res["runs"] == 2
    assert res["violations"] == 0, res


# ---------------------------------------------------------------------------------------------
# the command, in child processes
# ---------------------------------------------------------------------------------------------
def _cli_all(*arglists, timeout=300):
    """the command once per argument list, the child processes side by side (each spends most of its seconds
    starting up); every one is waited for"""
    ps = [subprocess.Popen([os.path.join(BIN, "dump-genclassifier-outputs")] + [str(a) for a in args],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for args in arglists]
    out = []
    for p in ps:
        try:
            so, se = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
        out.append(subprocess.CompletedProcess(p.args, p.returncode, so, se))
    return out


@pytest.fixture(scope="module", params=["rnn_noae", "rnn_normal"])
def cli_fix(request, tmp_path_factory):
    """a fixture as the files the command reads: checkpoint, egs.config (cmvn + splice), stats, feats, prior"""
    from speech_recognition_tools_amd.cmvn import write_kaldi_dmatrix, write_table
    name = request.param
    d = str(tmp_path_factory.mktemp("cli_" + name))
    meta, z, c, mdl = load_rnn_golden(name, d)
    write_kaldi_dmatrix(d + "/cmvn.stats", z["stats"])
    pickle.dump({"feat_type": "cmvn," + d + "/cmvn.stats", "concat_feats": "%d,%d" % (meta["left"], meta["right"])},
                open(d + "/egs.config", "wb"))
    utts = [(u, z["in_" + u]) for u in meta["utts"]]
    scp = TN_._write_feats(d, "feats", utts)
    prior = np.log(np.random.default_rng(3).dirichlet(np.ones(meta["num_classes"])))
    pickle.dump(prior, open(d + "/prior.pkl", "wb"))
    # per-utterance stats for all but the second utterance
    write_table("ark,scp:%s/utt.ark,%s/utt.scp" % (d, d), [(u, stats_of(np.concatenate([x, x[::-1] + 1.0])))
                                                          for i, (u, x) in enumerate(utts) if i != 1])
    return dict(d=d, meta=meta, z=z, c=c, mdl=mdl, utts=utts, scp=scp, prior=prior.astype(np.float32),
                ae=["--ae_type", meta["ae_type"]])


def _expected(c, norms=None, idx=None, utts=None, **kw):
    """RnnPlan.compute of the fixture's utterances, per utterance"""
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    meta = c["meta"]
    xs = [x for _, x in (utts or c["utts"])]
    plan = RnnPlan(PostConfig(dim=meta["feature_dim"], left_context=meta["left"], right_context=meta["right"]),
                   c["c"].stages, max_rows=sum(x.shape[0] for x in xs), max_utts=len(xs))
    if norms is None:
        norms = [PN.cmvn_norm(c["z"]["stats"], norm_vars=True)]
    return split_rows(run_rnn(plan, xs, norms, idx, **kw), xs)


@pytest.mark.gpu
def test_gpu_cli_logits_batches_and_ark(cli_fix):
    from speech_recognition_tools_amd.cmvn import MatReader
    from speech_recognition_tools_amd.nnet import round_ark
    c, d = cli_fix, cli_fix["d"]
    # the default; --batch-rows 8: many launches, utterances longer than a batch; an ark wspecifier, float32 values
    r, rb, ra = _cli_all(
        [c["mdl"], c["scp"], d + "/egs.config", d + "/post"] + c["ae"],
        [c["mdl"], "scp:" + c["scp"], d + "/egs.config", d + "/post_b", "--batch-rows", "8"] + c["ae"],
        [c["mdl"], "ark:" + d + "/feats.ark", d + "/egs.config", "ark:" + d + "/raw.ark", "--ark_precision", "-1"] + c["ae"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr.strip().splitlines()[-1] == ("LOG (dump-genclassifier-outputs) Dumped outputs for %d utterances, "
                                                 "errors on 0" % len(c["utts"]))
    got = TN_._read_scp(d + "/post.scp")
    assert [k for k, _ in got] == [k for k, _ in c["utts"]]              # keys and order of the scp
    assert not [f for f in os.listdir(d) if f.endswith(".tmp")]
    want = _expected(c)
    for (k, g), w in zip(got, want):
        assert_bits_equal(g, round_ark(w, 3), k)                        # the stated rounding, bit for bit
        assert np.all(np.abs(g.astype(np.float64) - c["z"]["logits3_" + k]) <= 0.001 + 16 * c["meta"]["d32"]), k
    assert rb.returncode == 0, rb.stderr[-2000:]                        # byte-identical files
    assert open(d + "/post_b.ark", "rb").read() == open(d + "/post.ark", "rb").read()
    assert (open(d + "/post_b.scp").read().replace("post_b.ark", "post.ark") == open(d + "/post.scp").read())
    assert ra.returncode == 0, ra.stderr[-2000:]
    got = [(k, m.copy()) for k, m in MatReader("ark:" + d + "/raw.ark")]
    assert [k for k, _ in got] == [k for k, _ in c["utts"]]
    for (k, g), w in zip(got, want):
        assert_bits_equal(g, w, k)


@pytest.mark.gpu
def test_gpu_cli_prior_softmax_and_utterance_cmvn(cli_fix):
    from speech_recognition_tools_amd.nnet import round_ark
    c, d = cli_fix, cli_fix["d"]
    # the second utterance has no per-utterance stats: skipped, counted, exit 0
    r, rs, ru = _cli_all(
        [c["mdl"], c["scp"], d + "/egs.config", d + "/ll", "--prior", d + "/prior.pkl", "--prior_weight", "0.2"] + c["ae"],
        [c["mdl"], c["scp"], d + "/egs.config", d + "/sm", "--add_softmax"] + c["ae"],
        [c["mdl"], c["scp"], d + "/egs.config", d + "/pu", "--override_trans=cmvn_utt," + d + "/utt.scp"] + c["ae"])
    assert r.returncode == 0, r.stderr[-2000:]
    for (k, g), w in zip(TN_._read_scp(d + "/ll.scp"), _expected(c, mode="loglike", prior=c["prior"], prior_weight=0.2)):
        assert_bits_equal(g, round_ark(w, 3), k)
    assert rs.returncode == 0, rs.stderr[-2000:]
    for (k, g), w in zip(TN_._read_scp(d + "/sm.scp"), _expected(c, mode="softmax")):
        assert_bits_equal(g, round_ark(w, 3), k)
        assert np.all(np.abs(g.sum(1) - 1.0) <= c["meta"]["num_classes"] * 0.0005 + 1e-6)
    r = ru
    assert r.returncode == 0, r.stderr[-2000:]
    n = len(c["utts"])
    assert "No normalization statistics available for key utt1" in r.stderr
    assert r.stderr.strip().splitlines()[-1].endswith("for %d utterances, errors on 1" % (n - 1))
    kept = [kv for i, kv in enumerate(c["utts"]) if i != 1]
    norms = [PN.cmvn_norm(stats_of(np.concatenate([x, x[::-1] + 1.0])), norm_vars=True) for _, x in kept]
    got = TN_._read_scp(d + "/pu.scp")
    assert [k for k, _ in got] == [k for k, _ in kept]
    for (k, g), w in zip(got, _expected(c, norms, list(range(len(kept))), kept)):
        assert_bits_equal(g, round_ark(w, 3), k)


@pytest.mark.gpu
def test_gpu_cli_failures_leave_nothing_behind(cli_fix, tmp_path):
    c, d, t = cli_fix, cli_fix["d"], str(tmp_path)
    blob = open(c["mdl"], "rb").read()
    open(t + "/cut.mdl", "wb").write(blob[:len(blob) // 2])              # a truncated model file
    rv, rc = _cli_all([c["mdl"], c["scp"], d + "/egs.config", t + "/o1", "--ae_type=vae"],
                      [t + "/cut.mdl", c["scp"], d + "/egs.config", t + "/o3"] + c["ae"])
    assert rv.returncode == 1 and "--ae_type=vae is not supported" in rv.stderr, rv.stderr[-2000:]
    assert rc.returncode == 1 and "cut.mdl" in rc.stderr, rc.stderr[-2000:]
    assert os.listdir(t) == ["cut.mdl"]                                  # no output, partial or temporary
