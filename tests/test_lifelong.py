"""compute-lifelong-likelihood and compute-incremental-likelihood: what speech_recognition_tools_amd/lifelong.py runs
after the logits of its D (classifier, VAE) pairs -- mmeasure_kernel, vae_sample_kernel, vae_elbo_kernel and
lifelong_fuse_kernel of csrc/fdlp_lifelong.hip -- around the stage plans tests/test_rnn.py holds.

Bounds, none of them fitted to what the device gives (tests/lifelong_numpy.py derives each):
  * every kernel against ITS OWN float32 inputs in float64: the M-measure and the fusion by the length of their
    float64 sums and the sum of the magnitudes added (plus the one float32 rounding of the fusion's result), the
    sampler by expf's ulp alone, the ELBO by its float32 rounding; NaN exactly where the oracle has NaN;
  * against the reference (tests/golden/lifelong_*.npz): 16 x d32 at the M-measure, at p(x), at the weights and at the
    output, test_rnn.py's rule, each with the d32 the generator measured for it;
  * every claim of independence (place in the batch, batch, --batch-rows) is asserted bitwise.

Figures of the run these tests were written against are in DESIGN.md 7i.
"""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import gru_numpy as GN
import lifelong_numpy as LN
import post_numpy as PN
import test_nnet as TN_
from conftest import GOLDEN, ROOT
from test_nnet import ark_like, assert_bits_equal

BIN = os.path.join(ROOT, "bin")
FIXTURES = ["lifelong_mm", "lifelong_dp", "lifelong_lowent", "lifelong_fixed", "lifelong_incremental"]


# ---------------------------------------------------------------------------------------------
# the fixtures as the files the tools read
# ---------------------------------------------------------------------------------------------
def models_golden():
    z = np.load(os.path.join(GOLDEN, "lifelong_models.npz"))
    return json.loads(str(z["meta"])), z


def result_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return json.loads(str(z["meta"])), z


def checkpoint_dicts(meta, z, i):
    from collections import OrderedDict
    import torch
    sd = OrderedDict((k[len("sd%d_" % i):], torch.from_numpy(np.array(z[k]))) for k in z.files
                     if k.startswith("sd%d_" % i))
    vsd = OrderedDict((k[len("vsd%d_" % i):], torch.from_numpy(np.array(z[k]))) for k in z.files
                      if k.startswith("vsd%d_" % i))
    return dict(meta["header"], model_state_dict=sd), dict(meta["vae_header"], model_state_dict=vsd)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """checkpoints, priors, egs.config, stats and feats of lifelong_models.npz in a directory"""
    import torch
    from speech_recognition_tools_amd.cmvn import write_kaldi_dmatrix
    d = str(tmp_path_factory.mktemp("lifelong"))
    meta, z = models_golden()
    pcx, px, pri = [], [], []
    for i in range(meta["D"]):
        c, v = checkpoint_dicts(meta, z, i)
        pcx.append("%s/cls%d.mdl" % (d, i))
        px.append("%s/vae%d.mdl" % (d, i))
        pri.append("%s/prior%d.pkl" % (d, i))
        torch.save(c, pcx[-1])
        torch.save(v, px[-1])
        pickle.dump(np.array(z["prior%d" % i]), open(pri[-1], "wb"))
    write_kaldi_dmatrix(d + "/cmvn.stats", z["stats"])
    pickle.dump({"feat_type": "cmvn," + d + "/cmvn.stats", "concat_feats": "%d,%d" % (meta["left"], meta["right"])},
                open(d + "/egs.config", "wb"))
    utts = [(u, np.array(z["in_" + u])) for u in meta["utts"]]
    scp = TN_._write_feats(d, "feats", utts)
    noise = {u: [np.array(z["eps%d_%s" % (i, u)]) for i in range(meta["D"])] for u in meta["utts"]}
    return dict(d=d, meta=meta, z=z, pcx=pcx, px=px, pri=pri, scp=scp, utts=utts, noise=noise, egs=d + "/egs.config")


def argv_of(f, task_prior, save, px=None):
    return [",".join(f["pcx"]), ",".join(px or f["px"]), f["scp"], f["egs"], ",".join(f["pri"]), task_prior, save]


def run_runner(f, tool, task_prior, tmp, utts=None, sel=False, batch_rows=None, noise="golden", seed=None, tag="o"):
    """the tool's runner in this process on `utts` (default: the fixture's); returns (runner, {utt: float32 rows})"""
    from speech_recognition_tools_amd import lifelong as L
    from speech_recognition_tools_amd.cmvn import MatReader
    from speech_recognition_tools_amd.post import FeatWriter
    tmp = str(tmp)
    scp = f["scp"] if utts is None else TN_._write_feats(tmp, "feats_" + tag, utts)
    ap = L.compute_lifelong_likelihood_parser() if tool == "lifelong" else L.compute_incremental_likelihood_parser()
    args = argv_of(f, task_prior, tmp + "/" + tag) + ["--ark_precision", "-1"]
    if batch_rows:
        args += ["--batch-rows", str(batch_rows)]
    if sel:
        args += ["--stream_selection"]
    if seed is not None:
        args += ["--seed", str(seed)]
    a = ap.parse_args(args)
    a.scp = scp
    lines = []
    r = L.make_runner(a, tool, "test", noise=f["noise"] if noise == "golden" else noise, keep=True, say=lines.append)
    w = FeatWriter("ark:%s/%s.ark" % (tmp, tag))
    done, err = r.run("scp:" + scp, w)
    w.close()
    r.close()
    r.lines = lines
    return r, {k: m.copy() for k, m in MatReader("ark:%s/%s.ark" % (tmp, tag))}


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_cli_argparse_surface_matches_reference():
    from speech_recognition_tools_amd import lifelong as L
    ref = json.load(open(os.path.join(GOLDEN, "cli_options_lifelong.json")))
    pos = ["models_pcx", "models_px", "scp", "egs_config", "priors", "task_prior", "save_file"]
    for script, parser, n in (("compute_lifelong_likelihood", L.compute_lifelong_likelihood_parser, 10),
                              ("compute_incremental_likelihood", L.compute_incremental_likelihood_parser, 9)):
        opts = ref[script]
        assert [o["name"] for o in opts][:7] == pos and len(opts) == n
        a = parser().parse_args(["a,b", "c,d", "s", "e", "p,q", "mm", "out"])
        for o in opts:
            dest = o["name"].lstrip("-")
            assert hasattr(a, dest), o
            if o["name"].startswith("--"):
                assert getattr(a, dest) == (False if o.get("action") == "store_true" else o.get("default")), o
        assert (a.ark_precision, a.batch_rows, a.seed) == (3, 32768, None)
        with pytest.raises(SystemExit):
            parser().parse_args(["a", "b", "s", "e", "p", "mm"])
    assert not hasattr(L.compute_incremental_likelihood_parser().parse_args(["a", "b", "s", "e", "p", "mm", "o"]),
                       "stream_selection")
    a = L.compute_lifelong_likelihood_parser().parse_args(
        ["a", "b", "s", "e", "p", "0.5", "o", "--stream_selection", "--prior_weight", "0.2", "--override_trans",
         "cmvn_utt,x.scp", "--seed", "7", "--device", "1", "--batch-rows", "8", "--ark_precision", "-1"])
    assert (a.stream_selection, a.prior_weight, a.override_trans, a.seed, a.device, a.batch_rows, a.ark_precision) == \
        (True, 0.2, "cmvn_utt,x.scp", 7, 1, 8, -1)
    for prog in ("compute-lifelong-likelihood", "compute-incremental-likelihood"):
        assert os.access(os.path.join(BIN, prog), os.X_OK)


def test_entry_points_are_declared_and_exported():
    from speech_recognition_tools_amd import _lib
    names = ["fdlp_life_mmeasure", "fdlp_life_vae_sample", "fdlp_life_vae_elbo", "fdlp_life_fuse"]
    src = open(os.path.join(ROOT, "include", "fdlp.h")).read()
    for n in names:
        assert ("int %s(" % n) in src and n in _lib.SIGNATURES and hasattr(_lib.lib, n), n
    assert sorted(n for n in _lib.SIGNATURES if "_life_" in n) == sorted(names)
    assert not [n for n in names if n.endswith("_plan_create")]


def _refusal(f, tmp, **change):
    """the message make_runner refuses the changed argument lists with"""
    from speech_recognition_tools_amd import lifelong as L
    c = dict(pcx=f["pcx"], px=f["px"], pri=f["pri"], task="dp")
    c.update(change)
    a = L.compute_lifelong_likelihood_parser().parse_args(
        [",".join(c["pcx"]), ",".join(c["px"]), f["scp"], f["egs"], ",".join(c["pri"]), c["task"], str(tmp) + "/o"])
    with pytest.raises(ValueError) as e:
        L.make_runner(a, "lifelong", "test")
    return str(e.value)


def test_refusals_name_the_file_and_the_key(files, tmp_path):
    import torch
    f, t = files, str(tmp_path)
    meta, z = f["meta"], f["z"]
    # list lengths that differ
    m = _refusal(f, t, px=f["px"][:2])
    assert "models_pcx names 3 models, models_px 2 and priors 3" in m
    assert "lists 2 weights for 3 models" in _refusal(f, t, task="0.5,0.5")
    # a classifier with another num_classes
    c, v = checkpoint_dicts(meta, z, 1)
    c["num_classes"] = 9
    c["model_state_dict"]["regression.weight"] = c["model_state_dict"]["regression.weight"][:9]
    c["model_state_dict"]["regression.bias"] = c["model_state_dict"]["regression.bias"][:9]
    torch.save(c, t + "/c9.mdl")
    m = _refusal(f, t, pcx=[f["pcx"][0], t + "/c9.mdl", f["pcx"][2]])
    assert "c9.mdl" in m and "'num_classes' is 9" in m and "cls0.mdl has 10" in m
    # a prior of another length
    pickle.dump(np.zeros(9), open(t + "/p9.pkl", "wb"))
    m = _refusal(f, t, pri=[f["pri"][0], t + "/p9.pkl", f["pri"][2]])
    assert "p9.pkl" in m and "9 entries" in m and "'num_classes' 10" in m
    # a VAE whose feature_dim * num_frames is not the spliced width
    c, v = checkpoint_dicts(meta, z, 2)
    v["num_frames"] = 1
    w = v["model_state_dict"]["vae_encoder.layers.0.weight_ih_l0"]
    v["model_state_dict"]["vae_encoder.layers.0.weight_ih_l0"] = w[:, :7].clone()
    v["model_state_dict"]["vae_decoder.means.weight"] = v["model_state_dict"]["vae_decoder.means.weight"][:7].clone()
    v["model_state_dict"]["vae_decoder.means.bias"] = v["model_state_dict"]["vae_decoder.means.bias"][:7].clone()
    torch.save(v, t + "/v7.mdl")
    m = _refusal(f, t, px=[f["px"][0], f["px"][1], t + "/v7.mdl"])
    assert "v7.mdl" in m and "'feature_dim' * 'num_frames' give 7 columns" in m and "have 21" in m
    # GRU widths above the scan's 384, in either model
    c, v = checkpoint_dicts(meta, z, 0)
    torch.save(dict(c, hidden_dim=385), t + "/wide.mdl")
    torch.save(dict(v, hidden_dim=512), t + "/widev.mdl")
    m = _refusal(f, t, pcx=[t + "/wide.mdl"] + f["pcx"][1:])
    assert "wide.mdl" in m and "'hidden_dim' is 385" in m and "384" in m
    m = _refusal(f, t, px=[t + "/widev.mdl"] + f["px"][1:])
    assert "widev.mdl" in m and "'hidden_dim' is 512" in m and "384" in m
    # a transformer VAE; a shape the header contradicts names the prefixed key
    torch.save(dict(v, use_transformer=True), t + "/tr.mdl")
    assert "transformer" in _refusal(f, t, px=[t + "/tr.mdl"] + f["px"][1:])
    torch.save(dict(v, bn_dim=12), t + "/bn.mdl")
    m = _refusal(f, t, px=[t + "/bn.mdl"] + f["px"][1:])
    assert "bn.mdl" in m and "'vae_encoder.means.weight'" in m
    # with mm or a list of floats models_px is counted and never opened
    from speech_recognition_tools_amd import lifelong as L
    for task in ("mm", "1,2,3"):
        a = L.compute_lifelong_likelihood_parser().parse_args(argv_of(f, task, t + "/o", px=["no/such"] * 3))
        assert L.make_runner(a, "lifelong", "test", say=lambda s: None).vaes is None
    with pytest.raises(OSError):
        a = L.compute_lifelong_likelihood_parser().parse_args(argv_of(f, "dp", t + "/o", px=["no/such"] * 3))
        L.make_runner(a, "lifelong", "test")


def test_vae_checkpoint_stacks_means_on_vars(files):
    from speech_recognition_tools_amd.lifelong import load_vae_checkpoint
    v = load_vae_checkpoint(files["px"][1])
    z = files["z"]
    assert [s[0] for s in v.enc_stages] == ["gru", "gru", "linear"] and [s[0] for s in v.dec_stages] == ["gru", "linear"]
    w, b = v.enc_stages[-1][1:]
    assert w.shape == (22, 33) and b.shape == (22,)
    np.testing.assert_array_equal(w[:11], z["vsd1_vae_encoder.means.weight"][:, :, 0])
    np.testing.assert_array_equal(w[11:], z["vsd1_vae_encoder.vars.weight"][:, :, 0])
    np.testing.assert_array_equal(b[11:], z["vsd1_vae_encoder.vars.bias"])
    np.testing.assert_array_equal(v.dec_stages[-1][1], z["vsd1_vae_decoder.means.weight"][:, :, 0])


def test_weight_rules():
    from scipy.stats import entropy
    from speech_recognition_tools_amd import lifelong as L
    nan = float("nan")
    said = []
    # mm: softmax; a NaN gives uniform weights and the reference's line
    w = L.task_weights("lifelong", "mm", mm=[0.5, 1.0, 0.25], say=said.append)
    np.testing.assert_array_equal(w, np.exp([0.5, 1.0, 0.25]) / np.sum(np.exp([0.5, 1.0, 0.25])))
    assert said == ["task 0 , mm=0.50", "task 1 , mm=1.00", "task 2 , mm=0.25"]
    said.clear()
    np.testing.assert_array_equal(L.task_weights("lifelong", "mm", mm=[0.5, nan, 0.25], say=said.append), np.ones(3) / 3)
    assert said[-1] == "Switching to uniform priors"
    # --stream_selection: one-hot at argmax; an all-NaN argmax is index 0, a one-hot, so no switch
    np.testing.assert_array_equal(L.task_weights("lifelong", "mm", mm=[0.5, 1.0, 0.25], stream_selection=True), [0, 1, 0])
    said.clear()
    np.testing.assert_array_equal(L.task_weights("lifelong", "mm", mm=[nan] * 3, stream_selection=True, say=said.append),
                                  [1, 0, 0])
    assert "Switching to uniform priors" not in said
    # a NaN that is not first wins numpy's argmax, as in the reference
    np.testing.assert_array_equal(L.task_weights("lifelong", "mm", mm=[0.5, nan, 2.0], stream_selection=True), [0, 1, 0])
    # the incremental tool has no stream selection
    w = L.task_weights("incremental", "mm", mm=[0.5, 1.0, 0.25], stream_selection=True)
    assert np.all(w > 0) and abs(w.sum() - 1) < 1e-15
    # dp: exp(300 px) (500 in the incremental tool), normalised; all far below gives the reference's 0 / 0
    px = np.array([-1.30, -1.31, -1.29])
    np.testing.assert_array_equal(L.task_weights("lifelong", "dp", px=px), np.exp(300 * px) / np.sum(np.exp(300 * px)))
    np.testing.assert_array_equal(L.task_weights("incremental", "dp", px=px), np.exp(500 * px) / np.sum(np.exp(500 * px)))
    assert np.isnan(L.task_weights("lifelong", "dp", px=[-3.0, -4.0, -5.0])).all()
    np.testing.assert_array_equal(L.task_weights("lifelong", "dp", px=px, stream_selection=True), [0, 0, 1])
    # lowent: the lower entropy of the two; 300 in the lifelong tool, 200 in the incremental one
    mm = np.array([0.5, 1.0, 0.25])
    w_mm = np.exp(mm) / np.sum(np.exp(mm))
    for tool, k in (("lifelong", 300.0), ("incremental", 200.0)):
        w_dp = np.exp(k * px) / np.sum(np.exp(k * px))
        assert entropy(w_dp) < entropy(w_mm)
        said.clear()
        np.testing.assert_array_equal(L.task_weights(tool, "lowent", mm=mm, px=px, say=said.append), w_dp)
        assert said == ["Entropy dp:{:.2f} and Entropy mm:{:.2f}".format(entropy(w_dp), entropy(w_mm))]
    flat = np.array([-1.3, -1.3, -1.3])                                   # dp uniform: the mm weights stay
    np.testing.assert_array_equal(L.task_weights("lifelong", "lowent", mm=mm, px=flat), w_mm)
    np.testing.assert_array_equal(L.task_weights("lifelong", "lowent", mm=mm, px=[-3.0, -4.0, -5.0]), w_mm)  # NaN entropy
    np.testing.assert_array_equal(L.task_weights("lifelong", "lowent", mm=[nan] * 3, px=flat), np.ones(3) / 3)
    # a list of floats is used as given
    np.testing.assert_array_equal(L.task_weights("lifelong", "fixed", fixed=[0.5, 0.0, 1.5]), [0.5, 0.0, 1.5])
    # the module's entropy is scipy's
    for v in ([0.2, 0.3, 0.5], [1.0, 0.0, 0.0], [2.0, 2.0], [nan, 0.5], [0.0, 0.0]):
        a, b = L.entropy(v), float(entropy(v))
        assert (np.isnan(a) and np.isnan(b)) or a == pytest.approx(b, rel=1e-15, abs=0), v
    # and the oracle's weights are the module's
    for kind, kw in (("mm", dict(mm=mm)), ("dp", dict(px=px)), ("lowent", dict(mm=mm, px=px))):
        for tool in ("lifelong", "incremental"):
            np.testing.assert_array_equal(L.task_weights(tool, kind, **kw), LN.weights(tool, kind, **kw))


def stages_of(f):
    from speech_recognition_tools_amd.lifelong import load_classifier, load_vae_checkpoint
    cls = [load_classifier(p).stages for p in f["pcx"]]
    vae = [load_vae_checkpoint(p) for p in f["px"]]
    return cls, [(v.enc_stages, v.dec_stages) for v in vae]


def golden_rows(f, u):
    meta, z = f["meta"], f["z"]
    return PN.post(np.array(z["in_" + u]), PN.cmvn_norm(z["stats"], norm_vars=True), True, 0, 2, 0, meta["left"],
                   meta["right"])


@pytest.fixture(scope="module")
def oracle64(files):
    """the float64 oracle on every fixture, computed once: {(fixture, sel): {utt: dict}}"""
    cls, vae = stages_of(files)
    priors = np.stack([files["z"]["prior%d" % i] for i in range(3)])
    out = {}
    for name in FIXTURES:
        meta, _ = result_golden(name)
        for sel in meta["stream_selection"]:
            out[name, sel] = {
                u: LN.utterance(golden_rows(files, u), cls, vae, files["noise"][u], priors, meta["prior_weight"],
                                meta["tool"], meta["kind"], meta["fixed"], sel, round32=False) for u in meta["utts"]}
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_self_check(oracle64, name):
    """lifelong_numpy, float64 throughout, against the reference's float64 run: 1e-9, NaN where it has NaN"""
    meta, z = result_golden(name)
    for sel in meta["stream_selection"]:
        pre = "sel_" if sel else ""
        for u in meta["utts"]:
            r = oracle64[name, sel][u]
            for k in ("mm", "px", "w"):
                if pre + k + "_" + u in z.files and r[k] is not None:
                    np.testing.assert_allclose(r[k], z[pre + k + "_" + u], rtol=0, atol=1e-9, equal_nan=True, err_msg=k + u)
            np.testing.assert_allclose(r["out"], z[pre + "out64_" + u], rtol=0, atol=1e-9, equal_nan=True, err_msg=u)
    if meta["kind"] in ("mm", "lowent"):       # T <= 65: NaN in the reference's M-measure
        assert all(np.isnan(z["mm_utt%d" % i]).all() for i in (0, 1)) and np.isfinite(z["mm_utt2"]).all()
    if name == "lifelong_mm":
        np.testing.assert_array_equal(z["w_utt0"], np.ones(3) / 3)
        assert sorted(z["sel_w_utt4"]) == [0, 0, 1]


def test_mmeasure_oracle_nan_rules():
    rng = np.random.default_rng(5)
    for T in (1, 5, 6, 65):
        assert np.isnan(LN.mmeasure(rng.dirichlet(np.ones(4), T)))
    P = rng.dirichlet(np.ones(4), 70).astype(np.float32)
    assert np.isfinite(LN.mmeasure(P))
    for t in (2, 40, 69):                      # a zero that is only ever Y, both, only ever X
        Q = P.copy()
        Q[t, 1] = 0.0
        assert np.isnan(LN.mmeasure(Q)), t


# ---------------------------------------------------------------------------------------------
# GPU: every kernel against its own inputs
# ---------------------------------------------------------------------------------------------
def _posts(rng, D, lens, C, sharp=3.0):
    x = rng.standard_normal((D, sum(lens), C)) * sharp
    e = np.exp(x - x.max(2, keepdims=True))
    return (e / e.sum(2, keepdims=True)).astype(np.float32)


def _split(lens):
    ends = np.cumsum(lens)
    return [(int(e - n), int(e)) for e, n in zip(ends, lens)]


MM_LENS = [1, 65, 66, 67, 71, 131, 200]


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("C", [1, 10, 70, 1936])
def test_gpu_mmeasure_against_its_own_input(C, D):
    import torch
    from speech_recognition_tools_amd import lifelong as L
    rng = np.random.default_rng(C + D)
    lens = MM_LENS + [70]
    P = _posts(rng, D, lens, C)
    zero_at = _split(lens)[-1][0] + 3                                     # the last utterance holds an exact 0
    P[D - 1, zero_at, C // 2] = 0.0
    dev = torch.device("cuda", 0)
    got = L.mmeasure(torch.from_numpy(P).to(dev), L.utt_tables(lens, dev)).cpu().numpy()
    assert got.shape == (len(lens), D)
    worst = 0.0
    for u, (a, b) in enumerate(_split(lens)):
        for m in range(D):
            ref, bound = LN.mmeasure(P[m, a:b], with_bound=True)
            if np.isnan(ref):
                assert np.isnan(got[u, m]), (u, m)
            else:
                err = abs(got[u, m] - ref)
                print("T %d C %d model %d: M %.6g err %.3g bound %.3g" % (b - a, C, m, ref, err, bound))
                assert err <= bound, (lens[u], C, m, err, bound)
                worst = max(worst, err / bound)
    assert [bool(np.isnan(got[u]).all()) for u in range(3)] == [True, True, False]   # T = 1, 65 | 66
    assert np.isnan(got[-1, D - 1])
    assert C == 1 or np.isfinite(got[:, 0][2:-1]).all()


@pytest.mark.gpu
def test_gpu_vae_sample_and_elbo_against_their_own_inputs():
    import torch
    from speech_recognition_tools_amd import lifelong as L
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    for K, bn, lens in ((21, 11, [1, 2, 67]), (117, 70, [5, 300]), (1, 1, [3]), (130, 64, [9])):
        rows = sum(lens)
        ml = np.concatenate([rng.standard_normal((rows, bn)), rng.standard_normal((rows, bn)) * 0.7 - 0.5], 1)
        ml = ml.astype(np.float32)
        eps = rng.standard_normal((rows, bn)).astype(np.float32)
        z = L.vae_sample(torch.from_numpy(ml).to(dev), torch.from_numpy(eps).to(dev)).cpu().numpy()
        ref, bound = LN.vae_sample_ref_and_bound(ml, eps)
        err = np.abs(z.astype(np.float64) - ref.astype(np.float64))
        print("sample K %d bn %d: max err / bound %.3g, exact in %.3f" % (K, bn, (err / bound).max(), (err == 0).mean()))
        assert np.all(err <= bound)
        x = rng.standard_normal((rows, K)).astype(np.float32)
        xh = (x + rng.standard_normal((rows, K)) * 0.8).astype(np.float32)
        tab = L.utt_tables(lens, dev)
        for tool in ("lifelong", "incremental"):
            px, elbo = L.vae_elbo(torch.from_numpy(x).to(dev), torch.from_numpy(xh).to(dev), torch.from_numpy(ml).to(dev),
                                  tab, tool)
            px, elbo = px.cpu().numpy(), elbo.cpu().numpy()
            ref, bound = LN.vae_elbo(x, xh, ml, with_bound=True)
            err = np.abs(elbo.astype(np.float64) - ref)
            print("elbo K %d bn %d: max err / bound %.3g" % (K, bn, (err / bound).max()))
            assert np.all(err <= bound)
            for u, (a, b) in enumerate(_split(lens)):
                ref, bound = LN.px_of(elbo[a:b], tool, with_bound=True)        # against the device's own rows
                assert abs(px[u] - ref) <= bound, (tool, K, u, px[u], ref, bound)
        # a column view of a table as the output: the stride is passed on
        table = torch.full((len(lens), 3), -7.0, dtype=torch.float64, device=dev)
        L.vae_elbo(torch.from_numpy(x).to(dev), torch.from_numpy(xh).to(dev), torch.from_numpy(ml).to(dev), tab,
                   "incremental", out=table[:, 1])
        t = table.cpu().numpy()
        np.testing.assert_array_equal(t[:, 1], px)
        assert np.all(t[:, [0, 2]] == -7.0)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [10, 70, 1936])
@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_gpu_fuse_against_its_own_input(D, C):
    import torch
    from speech_recognition_tools_amd import lifelong as L
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(100 * D + C)
    lens = [1, 63, 64, 65, 130]
    P = _posts(rng, D, lens, C)
    priors = np.log(rng.dirichlet(np.ones(C) * 5.0, D))
    w = rng.dirichlet(np.ones(D), len(lens))
    w[0] = np.eye(D)[D - 1]                                               # a one-hot row
    w[1, 0] = 0.0                                                         # a zero among the weights (all zero for D = 1)
    w[2] = rng.uniform(0.1, 2.0, D)                                       # a list of floats: need not sum to 1
    tab = L.utt_tables(lens, dev)
    Pd, wd = torch.from_numpy(P).to(dev), torch.from_numpy(w).to(dev)
    for tool, table in (("lifelong", np.exp(priors)), ("incremental", priors)):
        out = L.fuse(Pd, tab, max(lens), wd, torch.from_numpy(np.ascontiguousarray(table)).to(dev), 0.8, tool)
        out = out.cpu().numpy().astype(np.float64)
        worst = 0.0
        for u, (a, b) in enumerate(_split(lens)):
            ref, bound = LN.fuse(P[:, a:b], w[u], priors, 0.8, tool, with_bound=True)
            fin = np.isfinite(ref)
            np.testing.assert_array_equal(out[a:b][~fin], ref[~fin])          # -inf - (-inf), log 0: as IEEE gives
            err = np.abs(out[a:b][fin] - ref[fin])
            assert np.all(err <= bound[fin]), (tool, D, C, u, float((err / bound[fin]).max()))
            worst = max(worst, float((err / bound[fin]).max()) if fin.any() else 0.0)
        print("fuse %s D %d C %d: max err / bound %.3g" % (tool, D, C, worst))


# ---------------------------------------------------------------------------------------------
# GPU: the tools
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_against_reference_goldens(files, tmp_path, name):
    """16 x d32 at the M-measure, at p(x), at the weights and at the output, with the golden's noise injected"""
    meta, z = result_golden(name)
    task = ",".join(map(str, meta["fixed"])) if meta["kind"] == "fixed" else meta["kind"]
    worst = {}
    for sel in meta["stream_selection"]:
        pre = "sel_" if sel else ""
        r, outs = run_runner(files, meta["tool"], task, tmp_path, sel=sel, tag="g%d" % sel)
        for u in meta["utts"]:
            for k, got in (("mm", r.mm[u]), ("px", r.px[u]), ("w", r.weights[u])):
                key = pre + k + "_" + u
                if key not in z.files or got is None:
                    continue
                want = z[key]
                assert np.array_equal(np.isnan(got), np.isnan(want)), (key, got, want)
                fin = ~np.isnan(want)
                err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
                print("%s %s: err %.3g, d32 %.3g" % (name, key, err, meta["d32_" + k]))
                assert err <= 16 * meta["d32_" + k], (key, err, meta["d32_" + k])
                worst[k] = max(worst.get(k, 0.0), err)
            want = z[pre + "out64_" + u]
            got = outs[u].astype(np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(want)), u
            err = float(np.nanmax(np.abs(got - want)))
            print("%s %sout_%s: err %.3g, d32 %.3g" % (name, pre, u, err, meta["d32_out"]))
            assert err <= 16 * meta["d32_out"], (u, err, meta["d32_out"])
        if meta["kind"] == "mm" and not sel:        # T <= 65: the reference's uniform-prior rows
            for u in ("utt0", "utt1"):
                np.testing.assert_array_equal(r.weights[u], np.ones(3) / 3)
            assert r.lines.count("Switching to uniform priors") == 2
            assert "task 0 , mm=nan" in r.lines


@pytest.mark.gpu
@pytest.mark.parametrize("tool,task", [("lifelong", "lowent"), ("incremental", "lowent")])
def test_gpu_an_utterance_does_not_depend_on_its_batch(files, tmp_path, tool, task):
    """the same utterance alone, last of a batch of 40, and with --batch-rows cutting the batch elsewhere: identical
    bits at the M-measure, at p(x) and in the output"""
    rng = np.random.default_rng(17)
    x = ark_like(rng, 71, 7, 1.0)
    others = [("o%02d" % i, ark_like(rng, 2 + (7 * i) % 23, 7, 1.0)) for i in range(39)]
    noise = {k: [rng.standard_normal((m.shape[0], 11)).astype(np.float32) for _ in range(3)]
             for k, m in others + [("x", x)]}
    alone, oa = run_runner(files, tool, task, tmp_path, utts=[("x", x)], noise=noise, tag="a")
    assert np.isfinite(alone.mm["x"]).all() and np.isfinite(alone.px["x"]).all() and np.isfinite(oa["x"]).all()
    for tag, rows in (("b", None), ("c", 100), ("d", 71)):
        r, o = run_runner(files, tool, task, tmp_path, utts=others + [("x", x)], noise=noise, batch_rows=rows, tag=tag)
        assert len(o) == 40
        assert_bits_equal(r.mm["x"], alone.mm["x"], "M " + tag)
        assert_bits_equal(r.px["x"], alone.px["x"], "p(x) " + tag)
        assert_bits_equal(o["x"], oa["x"], "output " + tag)


@pytest.mark.gpu
def test_gpu_seed_gives_the_reference_draw_order(files, tmp_path):
    """--seed 7 with dp: the noise the runner used is torch.randn(1, T, bn) per utterance in scp order and per model
    in list order after torch.manual_seed(7)"""
    import torch
    r, _ = run_runner(files, "lifelong", "dp", tmp_path, noise=None, seed=7)
    torch.manual_seed(7)
    for u, x in files["utts"]:
        for i in range(3):
            want = torch.randn(1, x.shape[0], 11)[0].numpy()
            assert_bits_equal(r.noise_used[u][i], want, "%s model %d" % (u, i))
    r2, _ = run_runner(files, "lifelong", "mm", tmp_path, noise=None, seed=7, tag="m")
    assert r2.noise_used == {}


def _cli_all(*calls, timeout=300):
    """the commands (prog, args) side by side in child processes; every one is waited for"""
    ps = [subprocess.Popen([os.path.join(BIN, prog)] + [str(a) for a in args], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True) for prog, args in calls]
    out = []
    for p in ps:
        try:
            so, se = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
        out.append(subprocess.CompletedProcess(p.args, p.returncode, so, se))
    return out


@pytest.mark.gpu
def test_gpu_cli_both_commands_end_to_end(files, tmp_path):
    from speech_recognition_tools_amd.nnet import round_ark
    f, t = files, str(tmp_path)
    absent = ["no/such/vae%d.mdl" % i for i in range(3)]                  # accepted: counted, never opened
    # a list of floats; mm with --stream_selection; the incremental tool with lowent; two refusals
    r, rsel, rinc, rbad, rbad2 = _cli_all(
        ("compute-lifelong-likelihood", argv_of(f, "0.5,0.0,1.5", t + "/fx", px=absent)),
        ("compute-lifelong-likelihood", argv_of(f, "mm", t + "/sel", px=absent) + ["--stream_selection", "--batch-rows", "70"]),
        ("compute-incremental-likelihood", argv_of(f, "lowent", t + "/inc") + ["--seed", "3"]),
        ("compute-incremental-likelihood", argv_of(f, "dp", t + "/bad", px=absent)),
        ("compute-lifelong-likelihood", argv_of(f, "mm", t + "/bad2", px=absent[:2])))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr.strip().splitlines()[-1] == ("LOG (compute-lifelong-likelihood) Computed likelihoods for 5 "
                                                 "utterances, errors on 0")
    meta, z = result_golden("lifelong_fixed")
    got = TN_._read_scp(t + "/fx.scp")
    assert [k for k, _ in got] == meta["utts"] and meta["text_ok"]
    for k, g in got:
        assert np.all(np.abs(g.astype(np.float64) - z["text3_" + k]) <= 0.001 + 16 * meta["d32_out"]), k
        assert_bits_equal(g, round_ark(g, 3), k)
    assert not [n for n in os.listdir(t) if n.endswith(".tmp")]
    r = rsel
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines()[0] == "using mm-measure based task priors"
    assert "task 0 , mm=nan" in r.stdout and "Task 0 prior =1.000000 Task 1 prior =0.000000" in r.stdout
    meta, z = result_golden("lifelong_mm")
    for k, g in TN_._read_scp(t + "/sel.scp"):
        assert np.all(np.abs(g.astype(np.float64) - z["sel_text3_" + k]) <= 0.001 + 16 * meta["d32_out"]), k
    r = rinc
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines()[0] == "Using low-entropy prior" and "Entropy dp:" in r.stdout
    assert "p(x) for Task 0 =" in r.stdout and len(TN_._read_scp(t + "/inc.scp")) == 5
    # refusals exit 1 with the message and leave nothing behind
    r = rbad
    assert r.returncode == 1 and "no/such/vae0.mdl" in r.stderr and not os.path.exists(t + "/bad.ark")
    r = rbad2
    assert r.returncode == 1 and "models_px 2" in r.stderr
