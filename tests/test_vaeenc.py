"""compute-vae-encoded-likelihood: the VAE-encoded GRU models after the chain (speech_recognition_tools_amd/vaeenc.py,
conv2d_same_kernel and utt_norm_kernel of csrc/fdlp_vaeenc.hip, around the stages tests/test_rnn.py holds).

Bounds, none of them fitted to what the device gives (U = 2^-24):

  * a conv stage is held BITWISE to dense_kernel: the im2col rows of the tapped stage below (zeros outside the
    utterance and outside 0 .. F, k in the order (ci, dh, dw)) through an RnnPlan of an identity stage (exact: every
    chain is x 1 + zeros) and the stage ("linear", W.reshape(Co, -1), b) -- the identity being "linear_relu" for the
    layers after the first, whose input goes through the ReLU on load;
  * every stage against ITS OWN input: conv and linear stages by test_nnet.layer_ref_and_bound on the im2col or the
    rows, GRU stages by gru_numpy.gru_step_ref_and_bound, the normaliser by vaeenc_numpy.utt_norm_ref_and_bound,
    2U (|d| + |m|) / s + 4U |out|, on the device's own tapped latent;
  * against the reference (tests/golden/vaeenc_*.npz): 16 x d32 at every stage, test_rnn.py's rule and reasoning;
  * T = 1: finite before the normaliser, NaN from it on, as the reference (meta["t1_all_nan"]).
Every claim of independence (tile, place in the batch, batch, taps) is asserted bitwise.
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
import vaeenc_numpy as VN
from conftest import GOLDEN, ROOT
from test_nnet import ark_like, assert_bits_equal, layer_ref_and_bound, split_rows, stats_of, two_norms
from test_rnn import make_stages, run_rnn

BIN = os.path.join(ROOT, "bin")
GU, GKC, TM, KC = 32, 16, 128, 32     # kGruGU, kGruKC, kDenseTM (positions per conv tile), kDenseKC
U = 2.0 ** -24
GOLDENS = ["vaeenc_rnn", "vaeenc_cnn", "vaeenc_mod"]


def golden_checkpoints(meta, z):
    """(the classifier's dict, the encoder file's dict) of a fixture, as the reference's trainers save them"""
    from collections import OrderedDict
    import torch
    sd = OrderedDict((k[3:], torch.from_numpy(np.array(z[k]))) for k in z.files if k.startswith("sd_"))
    esd = OrderedDict((k[4:], torch.from_numpy(np.array(z[k]))) for k in z.files if k.startswith("esd_"))
    return (dict({k: meta[k] for k in meta["header"]}, model_state_dict=sd),
            dict(meta["enc_header"], model_state_dict=esd))


def load_vaeenc_golden(name, tmp):
    import torch
    from speech_recognition_tools_amd.vaeenc import load_vaeenc_checkpoint
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    cls, enc = golden_checkpoints(meta, z)
    mdl, encp = os.path.join(str(tmp), name + ".mdl"), os.path.join(str(tmp), name + ".enc")
    cls["vaeenc"] = encp
    torch.save(cls, mdl)
    torch.save(enc, encp)
    return meta, z, load_vaeenc_checkpoint(mdl, meta["vae_arch"]), mdl, encp


def golden_rows(meta, z, u):
    return PN.post(z["in_" + u], PN.cmvn_norm(z["stats"], norm_vars=True), True, 0, 2, 0, meta["left"], meta["right"])


def make_vstages(rng, arch, k0, enc, bn, cls, gain=3.0):
    """enc: [channels..] with a kernel for "cnn" (k0 = F), [(\"gru\", H)..] for "rnn"; cls: [("gru", H).., ("linear", C)]"""
    if arch == "cnn":
        channels, (kh, kw) = enc
        st = []
        for ci, co in zip(channels[:-1], channels[1:]):
            s = gain / np.sqrt(ci * kh * kw)
            st.append(("conv", rng.uniform(-s, s, (co, ci, kh, kw)).astype(np.float32),
                       (rng.uniform(-s, s, co) / gain).astype(np.float32)))
        k = channels[-1] * k0
    else:
        st = make_stages(rng, k0, enc, gain)
        k = enc[-1][1]
    st += make_stages(rng, k, [("linear", bn)], gain) + [("norm",)]
    return st + make_stages(rng, bn, cls, gain)


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_cli_argparse_surface_matches_reference():
    from speech_recognition_tools_amd import vaeenc
    ref = json.load(open(os.path.join(GOLDEN, "cli_options_vaeenc.json")))
    assert [o["name"] for o in ref][:4] == ["model", "scp", "egs_config", "save_file"] and len(ref) == 10
    a = vaeenc.compute_vae_encoded_likelihood_parser().parse_args(["final.mdl", "feats.scp", "egs.config", "post"])
    for o in ref:
        dest = o["name"].lstrip("-")
        assert hasattr(a, dest), o
        if o["name"].startswith("--"):
            assert getattr(a, dest) == (False if o.get("action") == "store_true" else o.get("default")), o
    assert (a.model, a.scp, a.egs_config, a.save_file) == ("final.mdl", "feats.scp", "egs.config", "post")
    assert (a.ark_precision, a.batch_rows, a.vaeenc, a.vae_arch) == (3, 32768, None, "cnn")
    a = vaeenc.compute_vae_encoded_likelihood_parser().parse_args(
        ["m", "s", "e", "o", "--vae_arch", "rnn", "--max_seq_len", "7", "--prior", "p", "--prior_weight", "0.2",
         "--add_softmax", "--override_trans", "cmvn_utt,x.scp", "--vaeenc", "v", "--device", "1", "--batch-rows", "8",
         "--ark_precision", "-1"])
    assert (a.vae_arch, a.max_seq_len, a.prior, a.prior_weight, a.add_softmax, a.override_trans, a.vaeenc, a.device,
            a.batch_rows, a.ark_precision) == ("rnn", 7, "p", 0.2, True, "cmvn_utt,x.scp", "v", 1, 8, -1)
    with pytest.raises(SystemExit):
        vaeenc.compute_vae_encoded_likelihood_parser().parse_args(["m", "s", "e"])
    assert os.access(os.path.join(BIN, "compute-vae-encoded-likelihood"), os.X_OK)


@pytest.mark.parametrize("name", GOLDENS)
def test_checkpoint_round_trip(tmp_path, name):
    meta, z, c, mdl, encp = load_vaeenc_golden(name, tmp_path)
    eh = meta["enc_header"]
    bn = eh["nfilters"] * eh["nrepeats"] if meta["vae_type"] == "modulation" else eh["bn_dim"]
    assert (bn, meta["vae_type"]) == ((12, "modulation") if name == "vaeenc_mod" else (11, "normal"))
    H, nl, C = meta["hidden_dim"], meta["num_layers"], meta["num_classes"]
    assert (c.vae_arch, c.vae_type, c.num_classes, c.vaeenc) == (meta["vae_arch"], meta["vae_type"], C, encp)
    tail = ["linear", "norm"] + ["gru"] * nl + ["linear"]
    if meta["vae_arch"] == "cnn":
        cout = [int(x) for x in eh["out_channels"].split(",")]
        F = eh["feature_dim"]
        assert [s[0] for s in c.stages] == ["conv"] * len(cout) + tail
        assert (c.feature_dim, c.num_frames) == (F, 1)                  # num_frames of the header is the chunk width
        assert c.dims == [F] + [co * F for co in cout] + [bn, bn] + [H] * nl + [C]
        assert_bits_equal(c.stages[1][1], z["esd_vae_encoder.cnn_layers.1.weight"])
        ne = len(cout)
    else:
        ne, He = eh["encoder_num_layers"], eh["hidden_dim"]
        assert [s[0] for s in c.stages] == ["gru"] * ne + tail
        assert (c.feature_dim, c.num_frames) == (eh["feature_dim"], eh["num_frames"])
        assert c.dims == [eh["feature_dim"] * eh["num_frames"]] + [He] * ne + [bn, bn] + [H] * nl + [C]
        assert_bits_equal(c.stages[0][2], z["esd_vae_encoder.layers.0.weight_hh_l0"])
    # the ignored keys are there, and the Conv1d weights are squeezed
    assert any(k.startswith("esd_vae_decoder.") for k in z.files) and "esd_vae_encoder.vars.weight" in z.files
    assert z["esd_vae_encoder.means.weight"].ndim == 3
    assert_bits_equal(c.stages[ne][1], z["esd_vae_encoder.means.weight"][:, :, 0])
    assert_bits_equal(c.stages[ne + 2][1], z["sd_layers.0.weight_ih_l0"])
    assert_bits_equal(c.stages[-1][1], z["sd_regression.weight"][:, :, 0])
    for st in c.stages:
        assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in st[1:])


def _variants(tmp_path, name):
    import torch
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    mdl, encp = str(tmp_path / "m.pt"), str(tmp_path / "e.pt")

    def variant(hdr=None, ehdr=None, drop=(), edrop=(), put=None, eput=None):
        cls, enc = golden_checkpoints(meta, z)
        cls["vaeenc"] = encp
        for d, h, dr, pu in ((cls, hdr, drop, put), (enc, ehdr, edrop, eput)):
            d.update(h or {})
            for k in dr:
                (d if k in d else d["model_state_dict"]).pop(k)
            d["model_state_dict"].update(pu or {})
        torch.save(cls, mdl)
        torch.save(enc, encp)

    return meta, mdl, encp, variant


def test_checkpoint_errors_name_the_key(tmp_path):
    import torch
    from speech_recognition_tools_amd.vaeenc import load_vaeenc_checkpoint
    meta, mdl, encp, variant = _variants(tmp_path, "vaeenc_rnn")
    variant(ehdr={"hidden_dim": 41})                                    # a shape that contradicts the header
    with pytest.raises(ValueError, match=r"e\.pt.*vae_encoder\.layers\.0\.weight_ih_l0"):
        load_vaeenc_checkpoint(mdl, "rnn")
    variant(ehdr={"bn_dim": 13})
    with pytest.raises(ValueError, match=r"vae_encoder\.means\.weight"):
        load_vaeenc_checkpoint(mdl, "rnn")
    variant(ehdr={"encoder_num_layers": 1})                             # a layer beyond the header's count
    with pytest.raises(ValueError, match=r"vae_encoder\.layers\.1\."):
        load_vaeenc_checkpoint(mdl, "rnn")
    variant(eput={"vae_encoder.means.weight": torch.zeros(11, 33, 2)})  # a Conv1d of kernel size 2
    with pytest.raises(ValueError, match=r"vae_encoder\.means\.weight"):
        load_vaeenc_checkpoint(mdl, "rnn")
    variant(hdr={"hidden_dim": 40})                                     # the classifier's own keys
    with pytest.raises(ValueError, match=r"m\.pt.*layers\.0\.weight_ih_l0"):
        load_vaeenc_checkpoint(mdl, "rnn")
    for k in ("vaeenc", "vae_type", "num_layers", "regression.bias"):
        variant(drop=[k])
        with pytest.raises(ValueError, match=k.replace(".", r"\.")):
            load_vaeenc_checkpoint(mdl, "rnn")
    for k in ("feature_dim", "bn_dim", "encoder_num_layers", "vae_encoder.means.bias", "vae_encoder.layers.1.bias_hh_l0"):
        variant(edrop=[k])
        with pytest.raises(ValueError, match=k.replace(".", r"\.")):
            load_vaeenc_checkpoint(mdl, "rnn")
    # every vae_decoder.* key and vae_encoder.vars.* of any shape, or absent: ignored
    variant(eput={"vae_decoder.layers.0.weight_ih_l0": torch.zeros(2, 2)}, edrop=["vae_encoder.vars.weight"])
    assert len(load_vaeenc_checkpoint(mdl, "rnn").stages) == 7
    variant()
    with pytest.raises(ValueError, match="in_channels|kernel"):         # a GRU encoder file read as a CNN's
        load_vaeenc_checkpoint(mdl, "cnn")
    os.unlink(encp)
    with pytest.raises(OSError, match="e.pt"):
        load_vaeenc_checkpoint(mdl, "rnn")
    # modulation: the latent is nfilters * nrepeats
    meta, mdl, encp, variant = _variants(tmp_path, "vaeenc_mod")
    variant(ehdr={"nrepeats": 2})
    with pytest.raises(ValueError, match=r"vae_encoder\.means\.weight.*\(8, 33\)"):
        load_vaeenc_checkpoint(mdl, "rnn")
    variant(edrop=["nfilters"])
    with pytest.raises(ValueError, match="nfilters"):
        load_vaeenc_checkpoint(mdl, "rnn")
    # arvae: the GRU encoder under another vae_type, its ar_steps ignored
    meta, mdl, encp, variant = _variants(tmp_path, "vaeenc_rnn")
    variant(hdr={"vae_type": "arvae"}, ehdr={"ar_steps": "1,2"})
    c = load_vaeenc_checkpoint(mdl, "rnn")
    assert (c.vae_type, [s[0] for s in c.stages]) == ("arvae", ["gru", "gru", "linear", "norm", "gru", "gru", "linear"])
    # cnn: the comma strings and the layers
    meta, mdl, encp, variant = _variants(tmp_path, "vaeenc_cnn")
    variant(ehdr={"kernel": "3,5,1"})
    with pytest.raises(ValueError, match="kernel"):
        load_vaeenc_checkpoint(mdl, "cnn")
    variant(ehdr={"out_channels": "5,6,8"})
    with pytest.raises(ValueError, match=r"vae_encoder\.cnn_layers\.2\.weight"):
        load_vaeenc_checkpoint(mdl, "cnn")
    variant(ehdr={"in_channels": "1,5,7"})
    with pytest.raises(ValueError, match="in_channels"):
        load_vaeenc_checkpoint(mdl, "cnn")
    variant(ehdr={"in_channels": "1,5", "out_channels": "5,6"})
    with pytest.raises(ValueError, match=r"vae_encoder\.cnn_layers\.2\."):
        load_vaeenc_checkpoint(mdl, "cnn")
    variant(ehdr={"feature_dim": 8})
    with pytest.raises(ValueError, match=r"vae_encoder\.means\.weight"):
        load_vaeenc_checkpoint(mdl, "cnn")
    variant(edrop=["vae_encoder.cnn_layers.0.bias"])
    with pytest.raises(ValueError, match=r"vae_encoder\.cnn_layers\.0\.bias"):
        load_vaeenc_checkpoint(mdl, "cnn")


def test_arvae_with_cnn_exits_1(tmp_path, capsys):
    from speech_recognition_tools_amd.vaeenc import main_compute_vae_encoded_likelihood
    meta, mdl, encp, variant = _variants(tmp_path, "vaeenc_cnn")
    variant(hdr={"vae_type": "arvae"})
    out = tmp_path / "out"
    out.mkdir()
    rc = main_compute_vae_encoded_likelihood([mdl, "s", "e", str(out / "post"), "--vae_arch=cnn"])
    err = capsys.readouterr().err
    assert rc == 1 and "ERROR (compute-vae-encoded-likelihood)" in err and "arvae" in err and "cnn" in err
    assert os.listdir(str(out)) == []


def test_vaeenc_path_from_the_header_or_the_option(tmp_path, monkeypatch):
    import torch
    from speech_recognition_tools_amd.vaeenc import load_vaeenc_checkpoint
    z = np.load(os.path.join(GOLDEN, "vaeenc_rnn.npz"))
    meta = json.loads(str(z["meta"]))
    cls, enc = golden_checkpoints(meta, z)
    assert cls["vaeenc"] == "exp/vae/final.model"                       # a path relative to the working directory
    os.makedirs(str(tmp_path / "run" / "exp" / "vae"))
    torch.save(cls, str(tmp_path / "m.pt"))
    torch.save(enc, str(tmp_path / "run" / "exp" / "vae" / "final.model"))
    monkeypatch.chdir(str(tmp_path / "run"))
    a = load_vaeenc_checkpoint(str(tmp_path / "m.pt"), "rnn")
    assert a.vaeenc == "exp/vae/final.model"
    monkeypatch.chdir(str(tmp_path))
    with pytest.raises(OSError, match="final.model"):
        load_vaeenc_checkpoint(str(tmp_path / "m.pt"), "rnn")
    b = load_vaeenc_checkpoint(str(tmp_path / "m.pt"), "rnn", vaeenc=str(tmp_path / "run" / "exp" / "vae" / "final.model"))
    assert b.vaeenc.endswith("run/exp/vae/final.model") and len(a.stages) == len(b.stages)
    for sa, sb in zip(a.stages, b.stages):
        for x, y in zip(sa[1:], sb[1:]):
            assert_bits_equal(x, y)
    enc["bn_dim"] = 12                                                   # --vaeenc wins over the header's path
    torch.save(enc, str(tmp_path / "other.model"))
    with pytest.raises(ValueError, match="other.model"):
        load_vaeenc_checkpoint(str(tmp_path / "m.pt"), "rnn", vaeenc=str(tmp_path / "other.model"))


def conv_lds(F, Ci, Co, kh, kw):
    """conv2d_same_kernel's LDS bytes: the koff table, the patch, dense_kernel's two chunk buffers"""
    K = Ci * kh * kw
    patch = -(-(((TM - 1) // F + kw + 1) * Ci * (F + kh - 1)) // 4) * 4
    return 4 * (-(-K // KC) * KC + patch) + 4 * 2 * (TM + (64 if Co <= 64 else 128)) * (KC + 4)


def test_host_only_plan_info_and_refusals():
    from speech_recognition_tools_amd._lib import FDLP_E_INVALID, FdlpError
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.vaeenc import VaeEncPlan, VaeEncShape
    # the trainer's default encoder in front of a classifier that fits the scan
    cnn = VaeEncShape("cnn", 30, 3, 256, 1936, channels=[1, 32, 64, 128], kh=3, kw=5, feat_h=13)
    p = VaeEncPlan(PostConfig(dim=13), None, max_rows=1000, max_utts=70, device=-1, shape=cnn)
    assert p.kinds == ["conv"] * 3 + ["linear", "norm"] + ["gru"] * 3 + ["linear"]
    assert (p.in_dim, p.n_stages, p.out_dim) == (13, 9, 1936)
    assert p.dims == [13, 32 * 13, 64 * 13, 128 * 13, 30, 30, 256, 256, 256, 1936]
    assert p.group_utts == GU
    # G [max_rows, 3 max H], two [max_rows, max_l C_l F] (the widest stage INPUT, the image included), the group table
    assert p.workspace_bytes == 4 * 1000 * 3 * 256 + 2 * 4 * 1000 * 128 * 13 + 16 * GU * 3
    assert p.lds_bytes == (4 * (3 * GU + 2 * GU * (256 + 4) + 4 * 2 * 96 * (GKC + 4)),
                           max(conv_lds(13, 1, 32, 3, 5), conv_lds(13, 32, 64, 3, 5), conv_lds(13, 64, 128, 3, 5)))
    assert p.lds_bytes[1] == conv_lds(13, 64, 128, 3, 5) <= 163840
    assert [p.tap_dim(t) for t in range(9)] == [1936, 256, 256, 256, 30, 30, 1664, 832, 416]
    g, s, ng = p.groups([5, 1, 9])
    assert (ng, g.tolist(), s.tolist()) == (1, [0, 0, 0], [1, 2, 0])
    rnn = VaeEncShape("rnn", 11, 2, 33, 10, in_dim=21, n_enc_layers=2, enc_hidden=40)
    q = VaeEncPlan(PostConfig(dim=7, left_context=1, right_context=1), None, max_rows=10, max_utts=33, device=-1, shape=rnn)
    assert (q.dims, q.kinds) == ([21, 40, 40, 11, 11, 33, 33, 10], ["gru", "gru", "linear", "norm", "gru", "gru", "linear"])
    assert q.workspace_bytes == 4 * 10 * 3 * 40 + 2 * 4 * 10 * 40 + 16 * GU * 2
    assert q.lds_bytes == (4 * (3 * GU + 2 * GU * (48 + 4) + 4 * 2 * 96 * (GKC + 4)), 0)
    # shapes taken from the arrays
    st = make_vstages(np.random.default_rng(0), "cnn", 7, ([1, 5, 6], (3, 5)), 4, [("gru", 8), ("linear", 3)])
    r = VaeEncPlan(PostConfig(dim=7), st, max_rows=5, device=-1)
    assert r.dims == [7, 35, 42, 4, 4, 8, 3] and (r.shape.kh, r.shape.kw, r.shape.feat_h) == (3, 5, 7)

    def refused(cfg, shape, *need, **kw):
        a = dict(max_rows=10, max_utts=4, device=-1)
        a.update(kw)
        with pytest.raises(FdlpError) as e:
            VaeEncPlan(cfg, None, shape=shape, **a)
        assert e.value.code == FDLP_E_INVALID and all(n in str(e.value) for n in need), str(e.value)

    import dataclasses
    c13 = PostConfig(dim=13)
    refused(c13, dataclasses.replace(cnn, kh=4), "odd", "(4, 5)")       # an even kernel
    refused(c13, dataclasses.replace(cnn, kw=2), "odd", "(3, 2)")
    refused(c13, dataclasses.replace(cnn, channels=[2, 32]), "channels[0] = 2")
    refused(PostConfig(dim=13, left_context=1, right_context=1), cnn, "13", "39")   # the chain gives 39 columns
    refused(PostConfig(dim=7), rnn, "21", "7")                          # the first GRU takes 21
    refused(c13, dataclasses.replace(cnn, cls_hidden=512), "512", "384", "163840")  # the trainer's default hidden_dim
    refused(PostConfig(dim=7, left_context=1, right_context=1), dataclasses.replace(rnn, enc_hidden=400), "400", "384")
    # a convolution the LDS cannot hold: the patch of 256 channels at F 13 alone is 15 frames x 256 x 15 floats
    refused(c13, dataclasses.replace(cnn, channels=[1, 256, 8]), "256 -> 8", "163840", str(conv_lds(13, 256, 8, 3, 5)))
    refused(c13, dataclasses.replace(cnn, channels=[1]), "n_conv = 0")
    refused(c13, dataclasses.replace(cnn, n_cls_layers=0), "classifier")
    refused(c13, dataclasses.replace(cnn, latent_dim=0), "0")
    refused(c13, cnn, "max_rows", max_rows=0)
    refused(c13, cnn, "max_utts", max_utts=0)
    VaeEncPlan(c13, None, max_rows=10, device=-1, shape=dataclasses.replace(cnn, cls_hidden=384))


def _venc_create(arch, in_dim=40, feat_h=40, **post):
    from speech_recognition_tools_amd import _lib
    import ctypes
    c = _lib.FdlpVencConfigC()
    c.post.dim, c.post.device = 40, -1
    for k, v in post.items():
        setattr(c.post, k, v)
    c.arch, c.in_dim, c.n_enc_layers, c.enc_hidden = arch, in_dim, 1, 8
    c.n_conv, c.kh, c.kw, c.feat_h = 1, 3, 5, feat_h
    c.channels[0], c.channels[1] = 1, 2
    c.latent_dim, c.n_cls_layers, c.cls_hidden, c.n_classes = 4, 1, 8, 5
    return lambda out: _lib.lib.fdlp_venc_create(ctypes.byref(c), None, 16, 1, out)


# the rejections that fire after the plan object exists (after and inside the nested chain create), as
# tests/test_plan_errors.py lists them for the other create functions: code, the whole message, no plan left behind
_HUGE = dict(dim=1000, left_context=100000, right_context=100000)
_POST_MSG = ("post plan does not fit the 160 KB LDS at one frame per tile: dim 1000, delta order 0 window 0, "
             "context -100000..+100000 give 200001000 output columns and need %d bytes")
_WIDTH_MSG = "the model's input dimension dims[0] = 39 differs from the 40 columns the stages before it give"
_XFORM_EXTRA = 4 * 2 * 32 * (min((24 + 15) // 16, 4) * 16 + 4)         # the staged chunk of a transform to 3 x 8 columns
CREATE_CASES = {
    "width": (lambda: _venc_create(0, in_dim=39), _WIDTH_MSG),
    "chain": (lambda: _venc_create(0, in_dim=1000, **_HUGE),
              (_POST_MSG % (800004000 + _XFORM_EXTRA)) + " (with a transform to 24 columns, %d of the bytes)" % _XFORM_EXTRA),
    "cnn-width": (lambda: _venc_create(1, feat_h=39), _WIDTH_MSG),
    "cnn-chain": (lambda: _venc_create(1, feat_h=1000, **_HUGE), _POST_MSG % 800004000),
}


@pytest.mark.parametrize("case", sorted(CREATE_CASES))
def test_create_refuses_and_leaves_no_plan(case):
    import ctypes
    from speech_recognition_tools_amd import _lib
    make, message = CREATE_CASES[case]
    out = ctypes.c_void_p(0xdead)                                       # create clears it before anything else
    assert make()(ctypes.byref(out)) == _lib.FDLP_E_INVALID
    assert _lib.lib.fdlp_last_error().decode() == message
    assert not out.value


def test_entry_points_are_declared_and_exported():
    import ctypes
    import re
    from speech_recognition_tools_amd import _lib
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.vaeenc import VaeEncPlan, VaeEncShape
    names = ["fdlp_venc_create", "fdlp_venc_plan_destroy", "fdlp_venc_plan_info", "fdlp_venc_plan_groups",
             "fdlp_venc_compute", "fdlp_venc_set_profiling", "fdlp_venc_times"]
    src = open(os.path.join(ROOT, "include", "fdlp.h")).read()
    declared = set(re.findall(r"\b(fdlp_[a-z0-9_]+)\s*\(", src))
    for n in names:
        assert n in declared and n in _lib.SIGNATURES and hasattr(_lib.lib, n), n
    assert "#define FDLP_ABI_VERSION 13" in src and _lib.lib.fdlp_abi_version() == 13 and _lib.ABI_VERSION == 13
    assert "#define FDLP_VENC_MAX_CONV 8" in src and _lib.FDLP_VENC_MAX_CONV == 8
    # the stage kinds of the public plan did not grow: the internal ones are refused there
    from speech_recognition_tools_amd.rnn import RnnPlan
    for k in (3, 4):
        with pytest.raises(_lib.FdlpError, match="unknown kind %d" % k):
            RnnPlan(PostConfig(dim=4), None, device=-1, kinds=["gru", k], dims=[4, 4, 4])
    p = VaeEncPlan(PostConfig(dim=4), None, device=-1,
                   shape=VaeEncShape("rnn", 3, 1, 5, 2, in_dim=4, n_enc_layers=1, enc_hidden=6))
    with pytest.raises(_lib.FdlpError, match="host-only"):
        _lib.check(_lib.lib.fdlp_venc_compute(p._h, ctypes.byref(_lib.FdlpPostBatchC()), 0, 0, None, 0.8, None))
    with pytest.raises(_lib.FdlpError):
        _lib.check(_lib.lib.fdlp_venc_plan_info(None, None, None, None, None, None, None))


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_self_check(tmp_path, name):
    """the twin and the fixtures agree before any GPU is involved: vaeenc_numpy in float64 reproduces the real
    classes' float64 outputs at every stage (this holds the twin, not the device)"""
    meta, z, c, _, _ = load_vaeenc_golden(name, tmp_path)
    d32 = meta["d32"]
    assert 0 < d32 <= 1e-5 and meta["t1_all_nan"] is True and meta["n_stages"] == len(c.stages)
    w64 = 0.0
    for u in meta["utts"]:
        rows = golden_rows(meta, z, u)
        o64 = VN.forward(rows, c.stages, dtype=np.float64)
        assert len(o64) == len(c.stages)
        for i, a in enumerate(o64):
            ref = z["stage%d_%s" % (i, u)]
            assert ref.dtype == np.float64 and ref.shape == a.shape, (i, ref.shape, a.shape)
            w64 = max(w64, float(np.abs(a - ref).max()))
        assert np.array_equal(z["stage%d_%s" % (len(c.stages) - 1, u)], z["f64_" + u])
        assert float(np.abs(z["f32_" + u] - z["f64_" + u]).max()) <= d32
        assert np.all(np.abs(z["logits3_" + u] - z["f32_" + u]) <= 0.0005 + 1e-6)
    print("%s: float64 restatement within %.3g" % (name, w64))
    assert w64 <= 1e-12
    one = VN.forward(golden_rows(meta, z, meta["utts"][0])[:1], c.stages, dtype=np.float64)
    n = [s[0] for s in c.stages].index("norm")
    assert all(np.isfinite(o).all() for o in one[:n]) and all(np.isnan(o).all() for o in one[n:])


def test_im2col_twin_is_the_definition():
    """vaeenc_numpy.im2col against the sum written out, on a shape with both paddings wider than the image"""
    rng = np.random.default_rng(2)
    F, Ci, kh, kw, T = 3, 2, 5, 3, 4
    rows = rng.standard_normal((T, Ci * F))
    cols = VN.im2col(rows, F, Ci, kh, kw)
    ph, pw = 2, 1
    for t in range(T):
        for f in range(F):
            for ci in range(Ci):
                for dh in range(kh):
                    for dw in range(kw):
                        tt, ff = t + dw - pw, f + dh - ph
                        want = rows[tt, ci * F + ff] if 0 <= tt < T and 0 <= ff < F else 0.0
                        assert cols[t, f, (ci * kh + dh) * kw + dw] == want


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def prev_of(plan, cfg, xs, norms, idx, s):
    """the float32 rows stage s loads, before the ReLU: the tapped stage below, or the chain's rows for stage 0"""
    from speech_recognition_tools_amd.post import PostPlan
    if s == 0:
        return TN_.run_post(PostPlan(cfg), xs, norms, idx)
    return run_rnn(plan, xs, norms, idx, tap=plan.n_stages - s)


# F, kernel, channels, utterance lengths.  A tile is TM = 128 positions p = t F + f of one utterance.
CONV_CASES = {
    # K = 15 / 75 / 90: below one k chunk, chunk tails; T < kw and T <= pw; 40 x 7 = 280 positions, three tiles
    "a_tails": (7, (3, 5), [1, 5, 6, 9], [1, 2, 3, 40]),
    # K = 480 at layer 2, N = 64 at a tile edge; 10 x 13 = 130 positions cross a tile by 2, 20 x 13 = 2 tiles + 4,
    # and the tile edge falls inside a frame
    "b_k480": (13, (3, 5), [1, 32, 64], [5, 10, 20]),
    "c_kh_over_f": (3, (5, 3), [1, 4], [1, 43, 5]),                      # 43 x 3 = 129: one position past a tile
    "d_1x1": (3, (1, 1), [1, 4], [43, 2]),
    # N = 130 past one column tile (three, the last of 2 channels); kw = 9: T <= pw; 32 x 4 = one tile exactly
    "e_n130": (4, (3, 9), [1, 3, 130], [32, 3, 33]),
}


def check_conv_case(what, F, kernel, channels, lens, seed):
    """GPU test 1 for one case: every conv stage against dense_kernel on its im2col rows, bitwise"""
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.rnn import RnnPlan
    from speech_recognition_tools_amd.vaeenc import VaeEncPlan
    rng = np.random.default_rng(seed)
    kh, kw = kernel
    cfg = PostConfig(dim=F)
    stages = make_vstages(rng, "cnn", F, (channels, kernel), 4, [("gru", 8), ("linear", 3)])
    xs = [ark_like(rng, T, F, 2.0 * (i % 2)) for i, T in enumerate(lens)]
    norms, idx = two_norms(xs)
    rows = sum(lens)
    plan = VaeEncPlan(cfg, stages, max_rows=rows, max_utts=len(lens))
    for s in range(len(channels) - 1):
        Ci, Co = channels[s], channels[s + 1]
        K = Ci * kh * kw
        got = run_rnn(plan, xs, norms, idx, tap=plan.n_stages - 1 - s)
        assert got.shape == (rows, Co * F) and np.all(np.isfinite(got))
        prev = prev_of(plan, cfg, xs, norms, idx, s)
        cols = [VN.im2col(a, F, Ci, kh, kw).reshape(-1, K) for a in split_rows(prev, xs)]
        w, b = stages[s][1], stages[s][2]
        eye = ("linear" if s == 0 else "linear_relu", np.eye(K, dtype=np.float32), np.zeros(K, dtype=np.float32))
        dense = RnnPlan(PostConfig(dim=K), [eye, ("linear", w.reshape(Co, K), b)], max_rows=rows * F,
                        max_utts=len(lens))
        want = run_rnn(dense, cols)                                      # [positions, Co]
        for u, (g, wv) in enumerate(zip(split_rows(got, xs), split_rows(want, cols))):
            T = xs[u].shape[0]
            assert_bits_equal(np.ascontiguousarray(g.reshape(T, Co, F).transpose(0, 2, 1)).reshape(T * F, Co), wv,
                              "%s layer %d (K %d, N %d) utterance %d of %d frames" % (what, s, K, Co, u, T))
        print("%s layer %d: K %d N %d, %d positions, bit-identical to dense_kernel" % (what, s, K, Co, rows * F))
    return len(channels) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_gpu_conv_is_dense_kernel_on_the_im2col_rows_bitwise(case):
    check_conv_case(case, *CONV_CASES[case], seed=sum(map(ord, case)))


def check_every_stage(what, arch, D, L, R, enc, bn, cls, lens, seed):
    """GPU test 2 for one case; returns the worst err/bound over the stages"""
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.vaeenc import VaeEncPlan
    rng = np.random.default_rng(seed)
    cfg = PostConfig(dim=D, left_context=L, right_context=R)
    k0 = D * (L + R + 1)
    stages = make_vstages(rng, arch, k0, enc, bn, cls)
    xs = [ark_like(rng, T, D, 2.0 * (i % 2)) for i, T in enumerate(lens)]
    norms, idx = two_norms(xs)
    rows = sum(lens)
    plan = VaeEncPlan(cfg, stages, max_rows=rows, max_utts=len(lens))
    prev = prev_of(plan, cfg, xs, norms, idx, 0)
    n, kind, worst = len(stages), None, 0.0
    i_norm = plan.kinds.index("norm")
    one = [u for u, T in enumerate(lens) if T == 1]
    for s, st in enumerate(stages):
        got = run_rnn(plan, xs, norms, idx, tap=n - 1 - s)
        assert got.shape == (rows, plan.dims[s + 1])
        parts = split_rows(got, xs)
        for u, g in enumerate(parts):                                    # T = 1: NaN from the normaliser on, as IEEE gives
            assert np.all(np.isnan(g)) if (u in one and s >= i_norm) else np.all(np.isfinite(g)), (what, s, u)
        A = VN.stage_input(prev, kind)
        kind = st[0]
        keep = [u for u in range(len(lens)) if not (u in one and s >= i_norm)]
        if kind == "gru":
            pairs = [GN.gru_step_ref_and_bound(a, g, *st[1:]) for a, g in zip(split_rows(A, xs), parts)]
        elif kind == "conv":
            Co, Ci, kh, kw = st[1].shape
            pairs = []
            for a in split_rows(A, xs):
                r, b = layer_ref_and_bound(VN.im2col(a, k0, Ci, kh, kw).reshape(-1, Ci * kh * kw),
                                           st[1].reshape(Co, -1), st[2])
                T = a.shape[0]
                pairs.append(tuple(np.ascontiguousarray(v.reshape(T, k0, Co).transpose(0, 2, 1)).reshape(T, Co * k0)
                                   for v in (r, b)))
        elif kind == "norm":
            pairs = [VN.utt_norm_ref_and_bound(a) if a.shape[0] >= 2 else (a, a) for a in split_rows(A, xs)]
        else:
            pairs = [layer_ref_and_bound(a, st[1], st[2]) for a in split_rows(A, xs)]
        for u in keep:
            # a later stage of a one-frame utterance has NaN input: nothing to hold it to
            ref, bound = pairs[u]
            err = np.abs(parts[u].astype(np.float64) - ref)
            ratio = float((err / bound).max())
            assert np.all(err <= bound), (what, s, kind, u, float((err - bound).max()), ratio)
            worst = max(worst, ratio)
        print("%s stage %d %s -> %d columns, %d utterances %d rows: max err/bound %.3g so far"
              % (what, s, kind, plan.dims[s + 1], len(lens), rows, worst))
        prev = got
    return worst


STAGE_CASES = {
    # the fixture's CNN shape; lengths under and over the kernel's width, three position tiles, one frame
    "cnn_a": ("cnn", 7, 0, 0, ([1, 5, 6, 9], (3, 5)), 11, [("gru", 33), ("gru", 33), ("linear", 10)], [2, 3, 40, 1, 5]),
    # a splice in front of the image (height 3 x 3 = 9), K = 288 at layer 2, 33 utterances: two scan groups
    "cnn_b": ("cnn", 3, 1, 1, ([1, 32, 7], (3, 3)), 5, [("gru", 40), ("linear", 6)], [2 + (5 * i) % 17 for i in range(GU + 1)]),
    "rnn_a": ("rnn", 7, 1, 1, [("gru", 33), ("gru", 33)], 11, [("gru", 33), ("gru", 33), ("linear", 10)], [2, 3, 40, 1]),
    "rnn_b": ("rnn", 5, 0, 0, [("gru", 64)], 30, [("gru", 40), ("linear", 7)], [2 + (5 * i) % 17 for i in range(GU + 1)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(STAGE_CASES))
def test_gpu_every_stage_against_its_own_input(case):
    check_every_stage(case, *STAGE_CASES[case], seed=sum(map(ord, case)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDENS)
def test_gpu_against_reference_goldens(tmp_path, name):
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.vaeenc import VaeEncPlan
    meta, z, c, _, _ = load_vaeenc_golden(name, tmp_path)
    d32 = meta["d32"]
    cfg = PostConfig(dim=meta["enc_header"]["feature_dim"], left_context=meta["left"], right_context=meta["right"])
    xs = [z["in_" + u] for u in meta["utts"]]
    norms = [PN.cmvn_norm(z["stats"], norm_vars=True)]
    plan = VaeEncPlan(cfg, c.stages, max_rows=sum(x.shape[0] for x in xs), max_utts=len(xs))
    n = len(c.stages)
    worst = 0.0
    for s in range(n):
        got = split_rows(run_rnn(plan, xs, norms, None, tap=n - 1 - s), xs)
        for g, u in zip(got, meta["utts"]):
            err = float(np.abs(g.astype(np.float64) - z["stage%d_%s" % (s, u)]).max())
            print("%s %s stage %d (%s): max err %.3g = %.3g d32" % (name, u, s, c.stages[s][0], err, err / d32))
            worst = max(worst, err / d32)
    assert worst <= 16, worst


INDEP = {
    "cnn": ("cnn", 5, ([1, 5, 33], (3, 5)), 6, [("gru", 40), ("linear", 5)]),
    "rnn": ("rnn", 5, [("gru", 40)], 6, [("gru", 40), ("linear", 5)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("arch", sorted(INDEP))
def test_gpu_an_utterance_does_not_depend_on_its_batch(arch):
    """an utterance's output at every tap, bit for bit: alone, first, last and in the middle of a batch of 33 ragged
    utterances (two scan groups; for the CNN its tiles start at other rows and other neighbours fill its halo)"""
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.vaeenc import VaeEncPlan
    _, D, enc, bn, cls = INDEP[arch]
    rng = np.random.default_rng(len(arch) + D)
    stages = make_vstages(rng, arch, D, enc, bn, cls)
    others = [ark_like(rng, 2 + (7 * i) % 11, D, 1.0) for i in range(GU)]
    norm = [PN.cmvn_norm(stats_of(np.concatenate(others)), norm_vars=True)]
    plan = VaeEncPlan(PostConfig(dim=D), stages, max_rows=sum(o.shape[0] for o in others) + 30, max_utts=GU + 1)
    assert plan.groups([o.shape[0] for o in others] + [2])[2] == 2
    for T in (27, 2):                                                    # 27 x 5 = 135 positions: two tiles
        x = ark_like(rng, T, D)
        for tap in range(plan.n_stages):
            alone = run_rnn(plan, [x], norm, tap=tap)
            assert np.all(np.isfinite(alone))

            def at(batch, k):
                o = run_rnn(plan, batch, norm, tap=tap)
                off = sum(b.shape[0] for b in batch[:k])
                return o[off:off + T]

            assert_bits_equal(at([x] + others, 0), alone, "first (tap %d)" % tap)
            assert_bits_equal(at(others + [x], GU), alone, "last (tap %d)" % tap)
            assert_bits_equal(at(others[:9] + [x] + others[9:], 9), alone, "in the middle (tap %d)" % tap)
            nans = [np.full_like(o, np.nan) for o in others]             # nothing of a neighbour is read as data
            assert_bits_equal(at(nans[:9] + [x] + nans[9:], 9), alone, "among NaN utterances (tap %d)" % tap)


@pytest.mark.gpu
def test_gpu_taps_do_not_depend_on_later_stages():
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.vaeenc import VaeEncPlan
    rng = np.random.default_rng(8)
    a = make_vstages(rng, "cnn", 5, ([1, 4, 6], (3, 3)), 6, [("gru", 33), ("gru", 33), ("linear", 5)])
    # the same encoder, means and first classifier GRU under another tail
    b = a[:5] + make_stages(np.random.default_rng(9), 33, [("gru", 20), ("linear", 3)])
    xs = [ark_like(rng, T, 5) for T in (7, 2, 30, 4)]
    rows = sum(x.shape[0] for x in xs)
    pa = VaeEncPlan(PostConfig(dim=5), a, max_rows=rows, max_utts=4)
    pb = VaeEncPlan(PostConfig(dim=5), b, max_rows=rows, max_utts=4)
    full = run_rnn(pa, xs)
    for s in range(5):
        assert_bits_equal(run_rnn(pa, xs, tap=6 - s), run_rnn(pb, xs, tap=6 - s), "stage %d" % s)
    assert_bits_equal(run_rnn(pa, xs), full, "after the taps")


CHECKS_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import test_vaeenc as TV
from speech_recognition_tools_amd.plan import device_checks
assert device_checks(reset=True)[0], "not a checks build"
runs = sum(TV.check_conv_case(c, *TV.CONV_CASES[c], seed=3) for c in TV.CHECK_CASES)
runs += TV.check_every_stage("cnn_a", *TV.STAGE_CASES["cnn_a"], seed=3) >= 0
en, v, line = device_checks()
print(json.dumps({"enabled": en, "violations": v, "last_line": line, "runs": int(runs)}))
"""
CHECK_CASES = ["a_tails", "b_k480"]


@pytest.mark.gpu
def test_gpu_device_range_checks_silent():
    """the FDLP_DEVICE_CHECKS build of conv2d_same_kernel and utt_norm_kernel (and the kernels around them): LDS and
    global indices in range over conv cases a and b and one pass through every stage"""
    lib = os.path.join(ROOT, "speech_recognition_tools_amd", "lib", "libfdlp_checks.so")
    assert os.path.exists(lib), "build() compiles libfdlp_checks.so"
    r = subprocess.run([sys.executable, "-c", CHECKS_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}],
                       cwd=ROOT, env=dict(os.environ, FDLP_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["enabled"] and res["runs"] == 3 + 2 + 1
    assert res["violations"] == 0, res


# ---------------------------------------------------------------------------------------------
# the command, in child processes
# ---------------------------------------------------------------------------------------------
PROG = "compute-vae-encoded-likelihood"


def _cli_all(*arglists, timeout=300):
    """the command once per argument list, the child processes side by side; every one is waited for"""
    ps = [subprocess.Popen([os.path.join(BIN, PROG)] + [str(a) for a in args], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True) for args in arglists]
    out = []
    for p in ps:
        try:
            so, se = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
        out.append(subprocess.CompletedProcess(p.args, p.returncode, so, se))
    return out


@pytest.fixture(scope="module", params=["vaeenc_rnn", "vaeenc_cnn"])
def cli_fix(request, tmp_path_factory):
    """a fixture as the files the command reads: the classifier (its header names the encoder file), the encoder file,
    egs.config (cmvn + splice), stats, feats with a one-frame utterance among them, prior, per-utterance stats"""
    from speech_recognition_tools_amd.cmvn import write_kaldi_dmatrix, write_table
    name = request.param
    d = str(tmp_path_factory.mktemp("cli_" + name))
    meta, z, c, mdl, encp = load_vaeenc_golden(name, d)
    write_kaldi_dmatrix(d + "/cmvn.stats", z["stats"])
    pickle.dump({"feat_type": "cmvn," + d + "/cmvn.stats",
                 "concat_feats": "%d,%d" % (meta["left"], meta["right"]) if meta["left"] + meta["right"] else None},
                open(d + "/egs.config", "wb"))
    utts = [(u, z["in_" + u]) for u in meta["utts"]]
    one = ("one_frame", z["in_" + meta["utts"][2]][5:6].copy())
    scp = TN_._write_feats(d, "feats", utts[:2] + [one] + utts[2:])
    prior = np.log(np.random.default_rng(3).dirichlet(np.ones(meta["num_classes"])))
    pickle.dump(prior, open(d + "/prior.pkl", "wb"))
    # per-utterance stats for all but the second utterance
    write_table("ark,scp:%s/utt.ark,%s/utt.scp" % (d, d),
                [(u, stats_of(np.concatenate([x, x[::-1] + 1.0]))) for i, (u, x) in enumerate(utts + [one]) if i != 1])
    return dict(d=d, meta=meta, z=z, c=c, mdl=mdl, enc=encp, utts=utts, scp=scp, prior=prior.astype(np.float32),
                arch=["--vae_arch", meta["vae_arch"]])


def _expected(c, norms=None, idx=None, utts=None, **kw):
    """VaeEncPlan.compute of the fixture's utterances, per utterance"""
    from speech_recognition_tools_amd.post import PostConfig
    from speech_recognition_tools_amd.vaeenc import VaeEncPlan
    meta = c["meta"]
    xs = [x for _, x in (utts or c["utts"])]
    plan = VaeEncPlan(PostConfig(dim=meta["enc_header"]["feature_dim"], left_context=meta["left"],
                                 right_context=meta["right"]),
                      c["c"].stages, max_rows=sum(x.shape[0] for x in xs), max_utts=len(xs))
    if norms is None:
        norms = [PN.cmvn_norm(c["z"]["stats"], norm_vars=True)]
    return split_rows(run_rnn(plan, xs, norms, idx, **kw), xs)


@pytest.mark.gpu
def test_gpu_cli_logits_batches_and_ark(cli_fix):
    from speech_recognition_tools_amd.cmvn import MatReader
    from speech_recognition_tools_amd.nnet import round_ark
    c, d = cli_fix, cli_fix["d"]
    # the default (the encoder's path from the header); --batch-rows 8: many launches, utterances longer than a
    # batch; an ark wspecifier with float32 values and the encoder named on the command line
    r, rb, ra = _cli_all(
        [c["mdl"], c["scp"], d + "/egs.config", d + "/post"] + c["arch"],
        [c["mdl"], "scp:" + c["scp"], d + "/egs.config", d + "/post_b", "--batch-rows", "8"] + c["arch"],
        [c["mdl"], "ark:" + d + "/feats.ark", d + "/egs.config", "ark:" + d + "/raw.ark", "--ark_precision=-1",
         "--vaeenc", c["enc"], "--max_seq_len", "9"] + c["arch"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == ""                                               # no print(batch_x.shape)
    assert "WARNING (%s) Utterance one_frame has one frame" % PROG in r.stderr
    assert r.stderr.strip().splitlines()[-1] == ("LOG (%s) Computed likelihoods for %d utterances, errors on 1"
                                                 % (PROG, len(c["utts"])))
    got = TN_._read_scp(d + "/post.scp")
    assert [k for k, _ in got] == [k for k, _ in c["utts"]]              # keys and order; the one-frame one is not there
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
        [c["mdl"], c["scp"], d + "/egs.config", d + "/ll", "--prior", d + "/prior.pkl", "--prior_weight", "0.2"] + c["arch"],
        [c["mdl"], c["scp"], d + "/egs.config", d + "/sm", "--add_softmax"] + c["arch"],
        [c["mdl"], c["scp"], d + "/egs.config", d + "/pu", "--override_trans=cmvn_utt," + d + "/utt.scp"] + c["arch"])
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
    assert "Utterance one_frame has one frame" in r.stderr
    assert r.stderr.strip().splitlines()[-1].endswith("for %d utterances, errors on 2" % (n - 1))
    kept = [kv for i, kv in enumerate(c["utts"]) if i != 1]
    norms = [PN.cmvn_norm(stats_of(np.concatenate([x, x[::-1] + 1.0])), norm_vars=True) for _, x in kept]
    got = TN_._read_scp(d + "/pu.scp")
    assert [k for k, _ in got] == [k for k, _ in kept]
    for (k, g), w in zip(got, _expected(c, norms, list(range(len(kept))), kept)):
        assert_bits_equal(g, round_ark(w, 3), k)


@pytest.mark.gpu
def test_gpu_cli_failures_leave_nothing_behind(cli_fix, tmp_path):
    import torch
    c, d, t = cli_fix, cli_fix["d"], str(tmp_path)
    cls, enc = golden_checkpoints(c["meta"], c["z"])
    key = "feature_dim" if c["meta"]["vae_arch"] == "cnn" else "hidden_dim"
    torch.save(dict(enc, **{key: enc[key] + 1}), t + "/bad.enc")         # a header its tensors contradict
    cls["vaeenc"], cls["vae_type"] = c["enc"], "arvae"
    torch.save(cls, t + "/arvae.mdl")
    rm, rs, ra = _cli_all(
        [c["mdl"], c["scp"], d + "/egs.config", t + "/o1", "--vaeenc", t + "/absent.enc"] + c["arch"],
        [c["mdl"], c["scp"], d + "/egs.config", t + "/o2", "--vaeenc", t + "/bad.enc"] + c["arch"],
        [t + "/arvae.mdl", c["scp"], d + "/egs.config", t + "/o3", "--vae_arch=cnn"])
    assert rm.returncode == 1 and "absent.enc" in rm.stderr, rm.stderr[-2000:]
    assert rs.returncode == 1 and "bad.enc" in rs.stderr and "vae_encoder." in rs.stderr, rs.stderr[-2000:]
    assert ra.returncode == 1 and "arvae" in ra.stderr, ra.stderr[-2000:]
    assert sorted(os.listdir(t)) == ["arvae.mdl", "bad.enc"]             # no output, partial or temporary
