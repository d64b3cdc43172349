"""Parity of the HIP path (through the C ABI) against the reference's golden outputs and the
CPU oracle.  Tolerance: 1e-4 max-abs on the fp64 log features (BASELINE.json north_star),
checked before the '%.3f' ark quantisation; the quantised float32 output may differ from the
reference's by one 0.001 step at rounding boundaries."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN_SETS, feature_cfg, load_golden, oracle_cfg

pytestmark = pytest.mark.gpu
TOL = 1e-4
# 'short2' is a 2-sample utterance: reflect padding turns it into an alternating sequence whose
# band energies away from DC and Nyquist sit at the fp64 rounding floor of the DCT, so its features
# are ill-conditioned at the rounding level: perturbing every autocorrelation by 1e-15 r0 (a few
# ulps of a 24000-term sum) moves them by 1.4e-3 in the oracle (tests/test_oracle_golden.py::
# test_short2_is_rounding_ill_conditioned).  It is held to 3e-3; every other utterance to TOL.
TOL_UTT = {"short2": 3e-3}


def _batch_inputs(meta, sig, z):
    from oracle import fdlp_oracle as O
    from speech_recognition_tools_amd import NpRandom
    from speech_recognition_tools_amd.augment import noise_params
    utts = meta["utts"]
    an = meta["opts"].get("add_noise", "clean")
    kw = {}
    # other WAV dtypes (wav_kinds_*) go to the device as their float64 values (FDLP_PCM_F64)
    wide = any(sig[u].dtype != np.int16 for u in utts)
    pcm = np.concatenate([sig[u].astype(np.float64) if wide else sig[u] for u in utts])
    if an == "diff":
        kw = dict(preprocess="diff")
    else:
        if an != "clean":
            noise = z["noise_babble"]
            snr = float(an.split(",")[1])
            nr = NpRandom(meta["extra"]["noise_seed"])
            offs, alps = [], []
            for u in utts:
                o, a = noise_params(sig[u], noise, snr, nr.rand())
                offs.append(o)
                alps.append(a)
            kw = dict(noise=torch.from_numpy(noise).cuda(), noise_off=offs, noise_alpha=alps)
    return pcm, kw


def run_gpu(meta, sig, z, support_eps=None, max_frames=256, debug=False, path="auto", lpc="auto", dct="auto"):
    from speech_recognition_tools_amd import FdlpPlan, PyRandom
    cfg = feature_cfg(meta, support_eps)
    plan = FdlpPlan(cfg, device=0, max_frames=max_frames)
    plan.set_autocorr_path(path)
    plan.set_lpc_path(lpc)
    plan.set_dct_path(dct)
    if debug:
        plan.set_debug(True)
    utts = meta["utts"]
    lens = [sig[u].size for u in utts]
    pcm, kw = _batch_inputs(meta, sig, z)
    pcm = torch.from_numpy(pcm).cuda()
    if meta["opts"].get("add_reverb", "clean") != "clean":  # addReverb on the device (fdlp_reverb)
        from oracle import fdlp_oracle as O
        from speech_recognition_tools_amd.augment import reverb
        rir = torch.from_numpy(O.load_rir(z["rir"])).cuda()
        pcm, lens = reverb(pcm, lens, rir, **kw)
        kw = {}
    nj = sum(max(plan.geometry(int(T))[0] - 1, 0) for T in lens)
    jit = PyRandom(meta["seed"]).randbits2(nj)
    out, rows, out64 = plan.compute(pcm, lens, jit, want_f64=True, **kw)
    torch.cuda.synchronize()
    out, out64 = out.cpu().numpy(), out64.cpu().numpy()
    res = {u: (out64[rows[i]:rows[i + 1]], out[rows[i]:rows[i + 1]]) for i, u in enumerate(utts)}
    return plan, res


@pytest.mark.parametrize("path", ["auto", "direct"])
@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_pipeline_vs_reference_golden(name, path):
    meta, sig, ref, z = load_golden(name)
    _, res = run_gpu(meta, sig, z, path=path)
    for u in meta["utts"]:
        f64, f32 = res[u]
        assert f64.shape == ref[u].shape, u
        err = np.abs(f64 - ref[u]).max()
        assert err <= TOL_UTT.get(u, TOL), (name, u, err)
        q = np.round(ref[u], 3).astype(np.float32)
        assert np.abs(f32 - q).max() <= max(1.0011e-3, 2 * TOL_UTT.get(u, 0)), (name, u)


@pytest.mark.parametrize("eps", [0.0, 1e-20, 1e-16])
def test_support_eps_variants(eps):
    meta, sig, ref, z = load_golden("wsj")
    _, res = run_gpu(meta, sig, z, support_eps=eps, path="direct")
    for u in meta["utts"]:
        assert np.abs(res[u][0] - ref[u]).max() <= TOL_UTT.get(u, TOL), (eps, u)


def test_batching_independent_of_grouping():
    """Utterances computed one batch at a time give the same features as one big batch."""
    meta, sig, ref, z = load_golden("wsj")
    _, res_all = run_gpu(meta, sig, z)
    from speech_recognition_tools_amd import FdlpPlan, PyRandom
    plan = FdlpPlan(feature_cfg(meta), device=0, max_frames=64)
    rng = PyRandom(meta["seed"])
    for u in meta["utts"]:
        T = sig[u].size
        jit = rng.randbits2(plan.geometry(T)[0] - 1)
        out, rows, out64 = plan.compute(torch.from_numpy(sig[u]).cuda(), [T], jit, want_f64=True)
        np.testing.assert_array_equal(out64.cpu().numpy(), res_all[u][0])


def test_stage_dct_and_lpc_vs_reference_stages():
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig
    z = np.load("tests/golden/stages_wsj.npz")
    plan = FdlpPlan(FeatureConfig.wsj(), device=0, max_frames=8)
    from oracle import fdlp_oracle as O
    cfg = O.FdlpConfig.wsj()
    fr = O.frames(z["x"], cfg, O.geometry(cfg))
    D = plan.dct_rows(torch.from_numpy(fr).cuda()).cpu().numpy()
    assert np.abs(D - z["dct"]).max() <= 1e-12 * np.abs(z["dct"]).max()
    fb, _, _ = plan.fbank()
    bands = np.stack([fb[j, :-1] * z["dct"][1] for j in (0, 37, 79)])
    r, a, gg = plan.lpc_rows(torch.from_numpy(bands).cuda())
    r, a, gg = r.cpu().numpy(), a.cpu().numpy(), gg.cpu().numpy()
    for i, tag in enumerate(("b0", "b37", "b79")):
        rr = z[tag + "_r"]
        assert np.abs(r[i] - rr).max() <= 1e-12 * abs(rr[0]), tag
        assert np.abs(a[i] - z[tag + "_a"]).max() <= 1e-6 * np.abs(z[tag + "_a"]).max(), tag
        assert abs(gg[i] - z[tag + "_gg"]) <= 1e-8 * abs(z[tag + "_gg"]), tag
    for lim in (100, 450):
        c = plan.cepstrum_rows(torch.from_numpy(np.stack([z[t + "_a"] for t in ("b0", "b37", "b79")])).cuda(),
                               torch.tensor([float(z[t + "_gg"]) for t in ("b0", "b37", "b79")],
                                            dtype=torch.float64).cuda(), lim).cpu().numpy()
        for i, tag in enumerate(("b0", "b37", "b79")):
            np.testing.assert_allclose(c[i], z["%s_c%d" % (tag, lim)], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("path", ["structured", "structured_mfma", "direct"])
def test_intermediates_vs_oracle(path):
    """Every stage of one utterance against the oracle's intermediates."""
    from oracle import fdlp_oracle as O
    meta, sig, ref, z = load_golden("wsj")
    sub = {"s4p0": sig["s4p0"]}
    plan, res = run_gpu(dict(meta, utts=["s4p0"]), sub, z, debug=True, path=path)
    d = plan.debug_fetch(4)
    keep = O.Intermediates()
    O.FdlpOracle(oracle_cfg(meta)).band_envelopes(sig["s4p0"], keep)
    assert np.abs(d["dct"] - keep.dct).max() <= 1e-10 * np.abs(keep.dct).max()
    rel = np.abs(d["r"] - keep.r).max(axis=-1) / np.abs(keep.r[..., 0])
    assert rel.max() <= 1e-12
    assert np.abs(d["cep"] - keep.cep).max() <= 1e-5
    assert np.abs(np.log(d["env"][..., 1:-1]) - np.log(keep.env[..., 1:-1])).max() <= 1e-5


STRUCT_CFGS = [
    # (fbank_type, nfilters, fduration, order, coeff_num)
    ("cochlear,1,1,1,2.5,1", 80, 1.5, 150, 100),     # WSJ / REVERB / CHiME-4 recipes
    ("cochlear,0.5,2.5,1,1.5,1", 40, 1.0, 60, 60),   # narrow flat top, steep lower skirt
    ("cochlear,2,0.5,1,4,1.2", 20, 0.5, 30, 40),     # wide flat top, warped axis, short frames
    ("cochlear,1,1,1,2.5,1", 7, 1.5, 238, 100),      # few wide bands, the largest order
    ("cochlear,0.02,1,1,2.5,1", 30, 0.5, 40, 40),    # (near-)empty flat tops
    ("cochlear,3,1,1,2.5,1", 60, 0.5, 20, 20),       # wide overlapping flat tops (many chains)
    ("cochlear,1,0.05,1,0.05,1", 24, 1.0, 50, 50),   # shallow skirts: the shared wrap straddle carries weight
]


@pytest.mark.parametrize("path", ["structured", "structured_mfma"])
@pytest.mark.parametrize("fb,nf,fd,order,cn", STRUCT_CFGS)
def test_structured_autocorr_matches_oracle(fb, nf, fd, order, cn, path):
    """The skirt-factorised autocorrelation equals the oracle's FFT autocorrelation of every band
    (features.py:223-226) to fp64 rounding, on speech-like and on white input, with the edge bands
    whose lower skirt (band 0) or upper skirt (last band) is empty; for both the lag-parallel VALU
    sweeps ('structured') and the MFMA lag-tile sweeps ('structured_mfma')."""
    from oracle import fdlp_oracle as O
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig, PyRandom
    cfg = FeatureConfig(fbank_type=fb, nfilters=nf, fduration=fd, order=order, coeff_num=cn,
                        coeff_range="0,%d" % cn)
    plan = FdlpPlan(cfg, device=0, max_frames=64)
    assert plan.autocorr_path in ("structured", "structured_mfma")
    plan.set_autocorr_path(path)
    plan.set_debug(True)
    rng = np.random.default_rng(nf + order)
    T = 16000 + 123
    t = np.arange(T) / 16000.0
    speechy = (3000 * np.sin(2 * np.pi * 180 * t) * (1 + np.sin(2 * np.pi * 3 * t))
               + 200 * rng.standard_normal(T)).astype(np.int16)
    white = (rng.standard_normal(T) * 8000).astype(np.int16)
    ocfg = O.FdlpConfig(fbank_type=fb, nfilters=nf, fduration=fd, order=order, coeff_num=cn,
                        coeff_range="0,%d" % cn)
    for x in (speechy, white):
        F, _ = plan.geometry(T)
        plan.compute(torch.from_numpy(x).cuda(), [T], PyRandom(0).randbits2(F - 1))
        torch.cuda.synchronize()
        d = plan.debug_fetch(F)
        keep = O.Intermediates()
        O.FdlpOracle(ocfg).band_envelopes(x, keep)
        rel = np.abs(d["r"] - keep.r).max(axis=-1) / np.abs(keep.r[..., 0])
        assert rel.max() <= 1e-12, rel.max()


def test_pipelined_sub_batches_match_serial():
    """Sub-batches on two streams (fdlp_set_pipeline) give bit-identical features."""
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig, PyRandom
    rng = np.random.default_rng(5)
    lens = [int(v) for v in rng.integers(8000, 300000, size=200)]
    pcm = (rng.standard_normal(sum(lens)) * 2000).astype(np.int16)
    plan = FdlpPlan(FeatureConfig.wsj(), device=0, max_frames=4096)
    nj = sum(plan.geometry(T)[0] - 1 for T in lens)
    assert sum(plan.geometry(T)[0] for T in lens) >= 1024
    jit = PyRandom(3).randbits2(nj)
    res = []
    for n in (1, 2, 4):
        plan.set_pipeline(n)
        out, rows, out64 = plan.compute(torch.from_numpy(pcm).cuda(), lens, jit, want_f64=True)
        torch.cuda.synchronize()
        res.append(out64.cpu().numpy())
    np.testing.assert_array_equal(res[0], res[1])
    np.testing.assert_array_equal(res[0], res[2])


@pytest.mark.parametrize("fduration", [0.5, 0.5315625, 1.5])
def test_dct_rows_even_and_odd_lengths(fduration):
    """fdlp_dct_rows == scipy dct-II / sqrt(2N) (computeFDLPSpectrogram.py:178) for an even N
    (packed half-length FFT: 8000, 24000) and an odd N (full-length complex FFT: 8505)."""
    import scipy.fft
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig
    cfg = FeatureConfig(fduration=fduration, nfilters=20, order=30, coeff_num=30, coeff_range="0,30")
    plan = FdlpPlan(cfg, device=0, max_frames=8)
    N = plan.N
    rng = np.random.default_rng(N)
    x = rng.standard_normal((5, N)) * np.linspace(1, 100, N)
    y = plan.dct_rows(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = scipy.fft.dct(x, type=2, axis=-1) / np.sqrt(2 * N)
    assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("name", ["wsj", "wsj_diff", "chime4_noise", "reverb_rir_noise"])
def test_dct_frame_kernel_matches_four_step(name):
    """The single-kernel DCT (dct_frame_kernel, default at N = 24000) against the four-step kernel pair
    on every frame of a golden set: plain int16 frames (the direct gather), reflect-padded edges, the
    diff filter, noise mixing and fp64 (reverberated) input (the staged gather); then the features."""
    meta, sig, ref, z = load_golden(name)
    plan_f, res_f = run_gpu(meta, sig, z, debug=True)
    assert plan_f.dct_path == "frame"
    plan_4, res_4 = run_gpu(meta, sig, z, debug=True, dct="four_step")
    assert plan_4.dct_path == "four_step"
    # frames of the batch (a reverberated utterance may come out one sample shorter: a lower bound)
    nf = sum(plan_f.geometry(sig[u].size - 1)[0] for u in meta["utts"])
    d_f = plan_f.debug_fetch(nf, keys=("dct",))["dct"]
    d_4 = plan_4.debug_fetch(nf, keys=("dct",))["dct"]
    scale = np.abs(d_4).max(axis=-1, keepdims=True)
    assert (np.abs(d_f - d_4) / scale).max() <= 1e-13
    for u in meta["utts"]:
        # the two DCTs round differently (<= 1e-13 of the frame maximum, above); Levinson amplifies that
        # to ~4e-8 on the wsj set's least well-conditioned frames (measured), the same order as the
        # lattice-vs-LDS Durbin bar; each path is held to the reference at 1e-4 by the golden tests
        np.testing.assert_allclose(res_f[u][0], res_4[u][0], rtol=0, atol=TOL_UTT.get(u, 1e-6), err_msg=u)


@pytest.mark.parametrize("name", ["wsj", "reverb", "cli_default_mel"])
def test_lattice_durbin_matches_lds_durbin(name, monkeypatch):
    """The register-resident lattice Durbin (default for order <= 255) and the LDS Durbin
    (fallback for larger orders, selected here by fdlp_set_lpc_path) give the same features and a."""
    meta, sig, ref, z = load_golden(name)
    plan, res_lat = run_gpu(meta, sig, z)
    _, res_lds = run_gpu(meta, sig, z, lpc="lds")
    for u in meta["utts"]:
        a, b = res_lat[u][0], res_lds[u][0]
        fin = np.isfinite(b)
        np.testing.assert_array_equal(np.isfinite(a), fin)
        # The two differ only in the summation order of the order-k dot products; Levinson at p = 150
        # amplifies that in the near-empty 4-8 kHz bands of the upsampled PESQ clips (1.4e-8 measured)
        # and in the degenerate short2 (its own tolerance).  Both stay within TOL of the reference.
        assert np.abs(a[fin] - b[fin]).max() <= TOL_UTT.get(u, 1e-6), (name, u)


def durbin_errors(plans, nf):
    """Per-item errors of each plan's Durbin against scipy's solve_toeplitz on the same r (the oracle,
    features.py:226-228): a as max |a - a_ref| / max |a_ref|, gg as |gg - gg_ref| / gg_ref, over the items
    with r_0 > 0."""
    from oracle import fdlp_oracle as O
    d = [pl.debug_fetch(nf, keys=("r", "a", "gg")) for pl in plans]
    r = d[0]["r"].reshape(-1, d[0]["r"].shape[-1])
    p = d[0]["a"].shape[-1] - 1
    live = np.flatnonzero(r[:, 0] > 0)
    ea = np.empty((len(plans), live.size))
    eg = np.empty((len(plans), live.size))
    for n, i in enumerate(live):
        a_ref, gg_ref = O.lpc_from_autocorr(r[i], p)
        sc = np.abs(a_ref).max()
        for k, dk in enumerate(d):
            ea[k, n] = np.abs(dk["a"].reshape(-1, p + 1)[i] - a_ref).max() / sc
            eg[k, n] = abs(dk["gg"].reshape(-1)[i] - gg_ref) / abs(gg_ref)
    return ea, eg


def assert_durbin4_accuracy(ea4, ea8, eg4, eg8, what):
    """durbin4 (the default) at least as accurate as durbin8 (the kernel it replaced) against solve_toeplitz.
    The two differ only in rounding (the order-k dot products summed over 4 lanes x 1 chain instead of 8
    lanes x 4 chains), which Levinson amplifies by each item's conditioning, so per item either kernel can
    be the more accurate one by a random factor: over the golden sets and orders 128-150 the ratio e4 / e8
    has median 0.81-0.83, p99 3.8-4.6 and maximum 6.3-10.2, and 6-7.5 % of the items exceed 2
    (tests/data/durbin4_accuracy_r05c.jsonl, benchmarks/durbin4_accuracy.py).  So the bars are on the
    distribution -- median, p99 and worst item no worse than durbin8's -- plus a per-item bound of 16x
    durbin8's error (above the measured maximum) or 1e-9, and gg within 1e-11 of the oracle's gain."""
    for q in (0.5, 0.99, 1.0):
        assert np.quantile(ea4, q) <= max(1e-13, 1.25 * np.quantile(ea8, q)), (what, q, np.quantile(ea4, q),
                                                                             np.quantile(ea8, q))
    assert np.all(ea4 <= np.maximum(1e-9, 16 * ea8)), (what, float((ea4 / np.maximum(ea8, 1e-300)).max()))
    assert eg4.max() <= 1e-11 and eg8.max() <= 1e-11, (what, float(eg4.max()), float(eg8.max()))


@pytest.mark.parametrize("name", ["wsj", "reverb", "mel80"])
def test_durbin4_matches_durbin8(name):
    """durbin4_kernel (4 lanes per item, the default for 128 <= p <= 150) against durbin8_kernel (8 lanes,
    FDLP_LPC_LATTICE8): the same lattice recursion with the order-k dot products summed over 4 lanes x 1
    chain instead of 8 lanes x 4 chains.  Features within 1e-6 (the ill-conditioned short2 / PESQ bands
    as for the LDS cross-check), gg of every item within 1e-9 of durbin8's, and a / gg of every item as
    accurate against solve_toeplitz as durbin8's (assert_durbin4_accuracy)."""
    meta, sig, ref, z = load_golden(name)
    p4, res4 = run_gpu(meta, sig, z, debug=True)
    p8, res8 = run_gpu(meta, sig, z, debug=True, lpc="lattice8")
    for u in meta["utts"]:
        a, b = res4[u][0], res8[u][0]
        fin = np.isfinite(b)
        np.testing.assert_array_equal(np.isfinite(a), fin)
        assert np.abs(a[fin] - b[fin]).max() <= TOL_UTT.get(u, 1e-6), (name, u)
        assert np.abs(a - ref[u]).max() <= TOL_UTT.get(u, TOL), (name, u)
    nf = sum(p4.geometry(sig[u].size)[0] for u in meta["utts"])
    g4 = p4.debug_fetch(nf, keys=("gg",))["gg"].reshape(-1)
    g8 = p8.debug_fetch(nf, keys=("gg",))["gg"].reshape(-1)
    live = g8 > 0
    assert live.sum() >= 80
    np.testing.assert_allclose(g4[live], g8[live], rtol=1e-9, atol=0)  # gg feeds c0 = log(sqrt(gg))
    (e4, e8), (eg4, eg8) = durbin_errors([p4, p8], nf)
    assert_durbin4_accuracy(e4, e8, eg4, eg8, name)


@pytest.mark.parametrize("order", [128, 130, 146, 149])
def test_durbin4_orders_below_150(order):
    """durbin4_kernel at the orders where it stops at an earlier phase than at the recipes' 150 (the per-item
    copy of a row shorter than its capacity, and the zero margins the select-free relayout relies on:
    ADVICE round 4): WSJ golden signals with --order changed, against the oracle at TOL (the jitter of
    O.compute_utterances), against durbin8_kernel and the LDS Durbin within 1e-6 (short2 3e-3), and a / gg
    per item against solve_toeplitz as for p = 150."""
    from oracle import fdlp_oracle as O
    meta, sig, ref, z = load_golden("wsj")
    meta = dict(meta, opts=dict(meta["opts"], order=order), seed=5)
    runs = {k: run_gpu(meta, sig, z, debug=True, lpc=k) for k in ("auto", "lattice8", "lds")}
    oref = O.compute_utterances(oracle_cfg(meta), {u: sig[u] for u in meta["utts"]}, 5)
    for u in meta["utts"]:
        got = runs["auto"][1][u][0]
        assert got.shape == oref[u].shape, u
        assert np.abs(got - oref[u]).max() <= TOL_UTT.get(u, TOL), (order, u, np.abs(got - oref[u]).max())
        for k in ("lattice8", "lds"):
            other = runs[k][1][u][0]
            assert np.abs(got - other).max() <= TOL_UTT.get(u, 1e-6), (order, k, u)
    nf = sum(runs["auto"][0].geometry(sig[u].size)[0] for u in meta["utts"])
    (e4, e8), (eg4, eg8) = durbin_errors([runs["auto"][0], runs["lattice8"][0]], nf)
    assert_durbin4_accuracy(e4, e8, eg4, eg8, order)


def test_reverb_kernel_vs_oracle():
    """fdlp_reverb (preprocessing + full convolution + xcorr argmax alignment) against the oracle's
    restatement of addReverb (features.py:110-115) on random int16 signals, with and without the diff
    preprocessing, including an RIR longer than one kernel tile and an utterance shorter than the RIR."""
    from oracle import fdlp_oracle as O
    from speech_recognition_tools_amd.augment import reverb
    rng = np.random.default_rng(3)
    rir = np.concatenate([[0.7, 0.0, -0.2], rng.standard_normal(1500) * np.exp(-np.arange(1500) / 300.0) * 0.2])
    sigs = [np.clip(rng.standard_normal(T) * 2000, -32768, 32767).astype(np.int16) for T in (5000, 1200, 777, 17000)]
    lens = [s.size for s in sigs]
    pcm = torch.from_numpy(np.concatenate(sigs)).cuda()
    for pre in (None, "diff"):
        out, ol = reverb(pcm, lens, torch.from_numpy(rir).cuda(), preprocess=pre)
        out = out.cpu().numpy()
        off = 0
        for s, T, L in zip(sigs, lens, ol):
            x = O.diff_signal(s) if pre == "diff" else s
            ref = O.add_reverb(x, rir)
            assert L == ref.size
            got = out[off:off + L]
            assert np.abs(got - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
            off += T


def test_librispeech_scale_lengths_vs_oracle():
    """BASELINE configs[4] shape: utterances of U(1, 30) s (seeded) plus the 1 s / 30 s extremes, WSJ
    feature settings, one batch (split over the plan's two-stream sub-batches), against the oracle at
    TOL: parity at the LibriSpeech-scale length distribution."""
    from collections import OrderedDict
    from oracle import fdlp_oracle as O
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig, PyRandom
    import bench
    rs = np.random.RandomState(960)
    lens = [int(rs.uniform(1.0, 30.0) * 16000) for _ in range(4)] + [16000, 30 * 16000 - 1]
    pcm = bench.speech_like_batch(1, sum(lens), 961).reshape(-1)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    sig = OrderedDict(("u%d" % i, pcm[o:o + t]) for i, (o, t) in enumerate(zip(offs, lens)))
    plan = FdlpPlan(FeatureConfig.wsj(), device=0, max_frames=256)
    nj = sum(plan.geometry(t)[0] - 1 for t in lens)
    _, rows, out64 = plan.compute(torch.from_numpy(pcm).cuda(), lens, PyRandom(5).randbits2(nj), want_f64=True)
    out64 = out64.cpu().numpy()
    ref = O.compute_utterances(O.FdlpConfig.wsj(), sig, 5)
    for i, u in enumerate(sig):
        got = out64[rows[i]:rows[i + 1]]
        assert got.shape == ref[u].shape, u
        assert np.abs(got - ref[u]).max() <= TOL, (u, lens[i], np.abs(got - ref[u]).max())


def test_torch_op_matches_plan_compute():
    """torch.ops.fdlp.spectrogram (the PyTorch-ROCm operator over fdlp_compute) == FdlpPlan.compute."""
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig, PyRandom
    meta, sig, ref, z = load_golden("wsj")
    utts = meta["utts"]
    lens = [sig[u].size for u in utts]
    pcm = torch.from_numpy(np.concatenate([sig[u] for u in utts])).cuda()
    plan = FdlpPlan(FeatureConfig.wsj(), device=0, max_frames=256)
    nj = sum(plan.geometry(T)[0] - 1 for T in lens)
    jit = PyRandom(meta["seed"]).randbits2(nj)
    got = torch.ops.fdlp.spectrogram(plan.op_id, pcm, torch.tensor(lens, dtype=torch.int64),
                                     torch.from_numpy(jit), 3)
    want, rows, _ = plan.compute(pcm, lens, jit)
    torch.cuda.synchronize()
    assert got.shape == (int(rows[-1]), 80) and got.dtype == torch.float32
    assert torch.equal(got, want)


def test_batches_in_flight_on_streams_match_serial():
    """Three plans featurising three batches concurrently on three HIP streams (bench.py --inflight)
    give bit-identical features to one plan computing the batches in turn."""
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig, PyRandom
    rng = np.random.default_rng(9)
    lens = [int(v) for v in rng.integers(16000, 120000, size=64)]
    pcm = torch.from_numpy(np.clip(rng.standard_normal(sum(lens)) * 2000, -32768, 32767).astype(np.int16)).cuda()
    plans = [FdlpPlan(FeatureConfig.wsj(), device=0, max_frames=512) for _ in range(3)]
    nj = sum(plans[0].geometry(T)[0] - 1 for T in lens)
    jits = [PyRandom(s).randbits2(nj) for s in (1, 2, 3)]
    ref = []
    for k in range(3):
        _, _, o64 = plans[0].compute(pcm, lens, jits[k], want_f64=True)
        torch.cuda.synchronize()
        ref.append(o64.cpu().numpy())
    streams = [torch.cuda.Stream() for _ in range(3)]
    res = []
    for k in range(3):
        with torch.cuda.stream(streams[k]):
            res.append(plans[k].compute(pcm, lens, jits[k], want_f64=True)[2])
    torch.cuda.synchronize()
    for k in range(3):
        np.testing.assert_array_equal(res[k].cpu().numpy(), ref[k])


def test_features_into_pinned_host_memory_match_device_output():
    """fdlp_compute with out_dev = the device mapping of a pinned host buffer (fdlp_mapped_ptr: the OLA
    kernel stores the features straight into host memory, the JOB runner's and bench's PCIe path) gives
    bit-identical features to a device output buffer."""
    from speech_recognition_tools_amd import FdlpPlan, PyRandom
    meta, sig, ref, z = load_golden("wsj")
    plan = FdlpPlan(feature_cfg(meta), device=0, max_frames=256)
    utts = meta["utts"]
    lens = [sig[u].size for u in utts]
    pcm = torch.from_numpy(np.concatenate([sig[u] for u in utts])).cuda()
    nj = sum(max(plan.geometry(int(T))[0] - 1, 0) for T in lens)
    jit = PyRandom(meta["seed"]).randbits2(nj)
    dev_out, rows, _ = plan.compute(pcm, lens, jit)
    host = torch.full(tuple(dev_out.shape), float("nan"), dtype=torch.float32).pin_memory()
    plan.compute(pcm, lens, jit, out=host)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host.numpy(), dev_out.cpu().numpy())
    with pytest.raises(ValueError):
        plan.compute(pcm, lens, jit, out=torch.empty(tuple(dev_out.shape), dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------
# addReverb edges: ties of the cross-correlation maximum and outputs shorter than the input
# ---------------------------------------------------------------------------------------------------------
def _tie_rir(last_peak):
    """Equal peaks at 5 and 5 + 256 (one thread's scan of rev_select_kernel, 256 apart) and `last_peak` at
    5 + 1024 (the second rev_xcorr_kernel block), and a smaller tap after each so the aligned output is not all zero."""
    rir = np.zeros(1300)
    rir[[5, 5 + 256]] = 0.5
    rir[5 + 1024] = last_peak
    rir[[300, 1100]] = 0.125
    return rir


def _impulse(T, a=1000):
    x = np.zeros(T, dtype=np.int16)
    x[0] = a
    return x


REVERB_EDGES = {
    # name: (signal, rir, output length); with x = a delta_0 the correlation at shift s is a^2 rir[s], products of
    # powers of two and 1000: exact in fp64, so equal peaks tie on the device as they do in numpy
    "tie_across_blocks": (_impulse(400), _tie_rir(0.5), 400),       # largest tied shift 1029 wins
    "tie_in_one_thread": (_impulse(400), _tie_rir(0.25), 400),      # 5 and 261 tie, 261 wins
    "all_zero": (np.zeros(300, dtype=np.int16), _tie_rir(0.5), 299),  # every shift ties: sh* = R - 1
    "rir_of_one_tap": (np.arange(-250, 250).astype(np.int16), np.array([0.5]), 499),
    "one_sample_long_rir": (_impulse(1, 1234), np.cos(np.arange(1300.0)) * np.exp(-np.arange(1300.0) / 200), 1),
    "one_sample_one_tap": (_impulse(1, 77), np.array([0.75]), 0),
}


@pytest.mark.parametrize("case", sorted(REVERB_EDGES))
def test_reverb_edges_vs_oracle(case):
    """rev_select_kernel keeps the LARGEST shift attaining the maximum (numpy's first argmax over the reversed
    correlation) through its strided scan, its LDS tree and the shifts of the second rev_xcorr_kernel block, and
    the output is one sample short when that shift is the last one: lengths and samples against O.add_reverb.
    The empty output of a one-sample utterance under a one-tap RIR is then refused by the plan."""
    from oracle import fdlp_oracle as O
    from speech_recognition_tools_amd import FdlpError, FdlpPlan, FeatureConfig
    from speech_recognition_tools_amd.augment import reverb
    x, rir, want_len = REVERB_EDGES[case]
    ref = O.add_reverb(x, rir)
    assert ref.size == want_len, (case, ref.size)
    # a neighbour on either side: the edge utterance is neither the first nor the last of the batch
    pad = np.arange(1, 600, dtype=np.int16)
    lens = [pad.size, x.size, pad.size]
    pcm = torch.from_numpy(np.concatenate([pad, x, pad])).cuda()
    out, ol = reverb(pcm, lens, torch.from_numpy(rir).cuda())
    assert [int(v) for v in ol] == [O.add_reverb(pad, rir).size, want_len, O.add_reverb(pad, rir).size]
    got = out.cpu().numpy()[pad.size:pad.size + want_len]
    assert got.shape == ref.shape
    if want_len:
        assert np.abs(got - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        if case.startswith("tie"):
            assert np.abs(ref).max() > 0
            np.testing.assert_array_equal(got, ref)  # exact products: the device's samples are numpy's
    else:  # the batch as augment.reverb hands it on: the emptied utterance between its two neighbours
        plan = FdlpPlan(FeatureConfig(), device=0, max_frames=16)
        with pytest.raises(FdlpError, match="too short"):
            plan.compute(out, [int(v) for v in ol], None, offsets=[0, pad.size, pad.size + x.size])


# ---------------------------------------------------------------------------------------------------------
# input kinds: every entry point x PCM kind x preprocessing either matches its oracle or says why not
# ---------------------------------------------------------------------------------------------------------
KIND_ENTRIES = ("spectrogram", "modspec", "modspec_complex", "mel", "mfcc", "reverb")
KIND_PCM = ("int16", "float64")
KIND_PRE = ("none", "noise", "diff")
# (entry, kind, pre) -> what the FdlpError has to say.  float64 PCM is the sample values of a non-16-bit WAV (or a
# reverberated signal); mel's diff filter, the MFCC script's own noise mixing and fdlp_reverb's preprocessing are
# written for int16 samples only, and computeMfccFeatures.py has no diff option at all (so no oracle either).
KIND_REFUSED = {
    ("mel", "float64", "diff"): "int16",
    ("mfcc", "float64", "noise"): "int16",
    ("mfcc", "int16", "diff"): "no diff",
    ("mfcc", "float64", "diff"): "no diff",
    ("reverb", "float64", "noise"): "int16",
    ("reverb", "float64", "diff"): "int16",
}
KIND_SNR, KIND_SEED, KIND_NOISE_SEED = 10.0, 4, 6
KIND_FDLP = dict(nfilters=5, order=20, fduration=0.5, frate=100, fbank_type="mel,1")
_KIND_DATA = {}


def _kind_data():
    if not _KIND_DATA:
        rng = np.random.default_rng(77)
        t = np.arange(9000) / 16000.0
        tone = 2500 * np.sin(2 * np.pi * 310 * t) * (1 + 0.5 * np.sin(2 * np.pi * 4 * t))
        sig = []
        for T, base, amp in ((9000, tone, 300), (5003, 0.0, 1500)):
            while True:  # the reference squares int16 in int16 (features.py:24-31): keep a positive wrapped mean
                s = np.round(base + amp * rng.standard_normal(T)).astype(np.int16)
                if np.mean(s ** 2) > 1.0:
                    break
            sig.append(s)
        _KIND_DATA["sig"] = sig
        _KIND_DATA["noise"] = np.round(rng.standard_normal(12000) * 60).astype(np.int16)  # squares stay in int16
        _KIND_DATA["rir"] = np.concatenate([[0.8], rng.standard_normal(299) * np.exp(-np.arange(299) / 60.0) * 0.2])
    return _KIND_DATA["sig"], _KIND_DATA["noise"], _KIND_DATA["rir"]


def _kind_cell(entry, kind, pre):
    """(device call -> list of fp64 outputs per utterance, oracle outputs, error bound per output) of one cell."""
    import random
    from oracle import fdlp_oracle as O
    from oracle import mel_oracle as MO
    from oracle import modspec_oracle as MS
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig, NpRandom, PyRandom
    from speech_recognition_tools_amd.augment import noise_params, noise_params_f64, reverb
    from speech_recognition_tools_amd.melspec import MelConfig, MelPlan
    from speech_recognition_tools_amd.mfcc import MfccConfig, MfccPlan
    sigs, noise, rir = _kind_data()
    xs = [s.astype(np.float64) if kind == "float64" else s for s in sigs]   # what the caller holds
    lens = [x.size for x in xs]
    nr = NpRandom(KIND_NOISE_SEED)
    draws = [nr.rand() for _ in xs]
    assert draws == list(np.random.RandomState(KIND_NOISE_SEED).rand(len(xs)))
    # host side: the reference's preprocessing of each signal in its own dtype
    if entry == "mfcc":  # computeMfccFeatures.py: / 2**15 first, its own add_noise_to_wav on the float64 arrays
        params = [noise_params_f64(x, noise, KIND_SNR, u) for x, u in zip(xs, draws)]
        pres = [x / np.power(2, 15) + (a * (noise[o:o + x.size] / np.power(2, 15)) if pre == "noise" else 0.0)
                for x, (o, a) in zip(xs, params)]
    else:
        params = [noise_params(x, noise, KIND_SNR, u) for x, u in zip(xs, draws)]
        pres = [O.diff_signal(x) if pre == "diff" else O.add_noise(x, noise, KIND_SNR, u) if pre == "noise" else x
                for x, u in zip(xs, draws)]
        if pre == "noise":
            for x, u, (o, a) in zip(xs, draws, params):  # the device's (offset, alpha) are the oracle's
                ro, ra = O.noise_mix_params(x, noise, KIND_SNR, u)
                assert o == ro and a == float(ra)
    assert all(np.isfinite(a) and a > 0 for _, a in params)
    kw = {}
    if pre == "diff":
        kw = dict(preprocess="diff")
    elif pre == "noise":
        kw = dict(noise=torch.from_numpy(noise).cuda(), noise_off=[o for o, _ in params],
                  noise_alpha=[a for _, a in params])
    pcm = torch.from_numpy(np.concatenate(xs)).cuda()

    def split(out64, rows):
        out64 = out64.cpu().numpy()
        return [out64[rows[i]:rows[i + 1]] for i in range(len(xs))]

    if entry in ("spectrogram", "modspec", "modspec_complex"):
        if entry == "spectrogram":
            cfg = FeatureConfig(coeff_num=20, coeff_range="1,20", overlap_fraction=0.25, **KIND_FDLP)
            orc = O.FdlpOracle(O.FdlpConfig(coeff_num=20, coeff_range="1,20", overlap_fraction=0.25, **KIND_FDLP))
            prng = random.Random(KIND_SEED)
            want = [orc.utterance(x, prng) for x in pres]
            bound = [TOL * np.ones_like(w) for w in want]                         # this module's bar
        else:
            cfg = FeatureConfig(mode=entry, window="hanning", coeff_num=20, coeff_0=2, **KIND_FDLP)
            f = MS.modspec_features if entry == "modspec" else MS.modspec_complex_features
            want = [f(np.asarray(x, dtype=np.float64), coeff_0=2, coeff_n=20, **KIND_FDLP) for x in pres]
            bound = [1e-7 * np.maximum(1.0, np.abs(w)) for w in want]             # tests/test_modspec.py TOL
        plan = FdlpPlan(cfg, device=0, max_frames=128)

        def run():
            jit = PyRandom(KIND_SEED).randbits2(sum(max(plan.geometry(T)[0] - 1, 0) for T in lens))
            _, rows, out64 = plan.compute(pcm, lens, jit, want_f64=True, **kw)
            return split(out64, rows)
    elif entry == "mel":
        plan = MelPlan(MelConfig(), device=0, max_frames=128)
        want = [MO.mel_spectrum(x) for x in pres]
        bound = [1e-9 * np.maximum(1.0, np.abs(w)) for w in want]                 # tests/test_melspec.py

        def run():
            _, rows, out64 = plan.compute(pcm, lens, want_f64=True, **kw)
            return split(out64, rows)
    elif entry == "mfcc":
        plan = MfccPlan(MfccConfig(), device=0, max_frames=128)
        t = plan.tables()
        K, nb, nbp = t["K"], t["nb"], t["nbpad"]
        want = []
        for x in pres:  # the reference chain on the plan's tables (tests/test_mfcc.py holds them to the reference)
            fr = MO.get_frames(x, 16000, 100, 0.02)[:, :K]
            mag = np.hypot(fr @ t["tw"][:K, :nb], fr @ t["tw"][:K, nbp:nbp + nb])
            want.append(np.log10(mag @ t["fold"].T) @ t["dct"])
        bound = [1e-6 * np.ones_like(w) for w in want]                            # tests/test_mfcc.py

        def run():
            _, rows, out64 = plan.compute(pcm, lens, want_f64=True, **kw)
            return split(out64, rows)
    else:
        want = [O.add_reverb(x, rir) for x in pres]
        bound = [1e-9 * max(1.0, np.abs(w).max()) * np.ones_like(w) for w in want]  # test_reverb_kernel_vs_oracle

        def run():
            out, ol = reverb(pcm, lens, torch.from_numpy(rir).cuda(), **kw)
            out = out.cpu().numpy()
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
            return [out[o:o + n] for o, n in zip(offs, ol)]
    return run, want, bound


@pytest.mark.parametrize("pre", KIND_PRE)
@pytest.mark.parametrize("kind", KIND_PCM)
@pytest.mark.parametrize("entry", KIND_ENTRIES)
def test_input_kind_table(entry, kind, pre):
    """Every (entry point, PCM kind, preprocessing) cell computes its oracle's features at that entry's own bar,
    or raises FdlpError naming the cause; KIND_REFUSED lists the refusals, and nothing is computed silently
    without its preprocessing (mel float64 + noise did: mel_kernel ignored the noise for float64 PCM)."""
    from speech_recognition_tools_amd import FdlpError
    assert set(KIND_REFUSED) <= {(e, k, p) for e in KIND_ENTRIES for k in KIND_PCM for p in KIND_PRE}
    run, want, bound = _kind_cell(entry, kind, pre)
    assert all(np.isfinite(w).all() and w.size for w in want)
    if (entry, kind, pre) in KIND_REFUSED:
        with pytest.raises(FdlpError, match=KIND_REFUSED[(entry, kind, pre)]):
            run()
        return
    got = run()
    for i, (g, w, b) in enumerate(zip(got, want, bound)):
        assert g.shape == w.shape, (entry, kind, pre, i, g.shape, w.shape)
        excess = np.abs(g - w) / b
        assert excess.max() <= 1.0, (entry, kind, pre, i, float(np.abs(g - w).max()))


# One smallest batch per plan family, as (make_plan, run(plan) -> output tensor): one utterance of two analysis
# frames for the featurisers, one utterance of tile + 1 rows (two tiles, the second of one row) for the chain plans.
def _two_frame_pcm(frames_of):
    T = next(t for t in range(1, 1 << 20) if frames_of(t) == 2)
    return torch.from_numpy(np.random.RandomState(T).randint(-3000, 3000, T).astype(np.int16)).cuda(), T


def _destroy_fdlp():
    from speech_recognition_tools_amd import FdlpPlan, FeatureConfig, PyRandom
    def run(plan):
        pcm, T = _two_frame_pcm(lambda t: plan.geometry(t)[0])
        return plan.compute(pcm, [T], PyRandom(3).randbits2(1))[0]
    return (lambda: FdlpPlan(FeatureConfig(**KIND_FDLP), device=0, max_frames=4)), run


def _destroy_feat(kind):
    from speech_recognition_tools_amd.melspec import MelConfig, MelPlan
    from speech_recognition_tools_amd.mfcc import MfccConfig, MfccPlan
    Plan, cfg = (MelPlan, MelConfig()) if kind == "mel" else (MfccPlan, MfccConfig(context=1))
    def run(plan):
        pcm, T = _two_frame_pcm(plan.frames)
        return plan.compute(pcm, [T])[0]
    return (lambda: Plan(cfg, device=0, max_frames=4)), run


def _destroy_chain(kind):
    from speech_recognition_tools_amd.post import PostConfig, PostPlan, XformPlan
    from speech_recognition_tools_amd.rnn import RnnPlan
    cfg = PostConfig(dim=8, delta_order=2, left_context=1, right_context=1)
    K, H, C = 8 * 3 * 3, 16, 5
    rs = np.random.RandomState(11)
    w = lambda *shape: (0.1 * rs.randn(*shape)).astype(np.float32)
    if kind == "post":
        make, tile, extra = (lambda: PostPlan(cfg, device=0)), PostPlan(cfg, device=-1).tile, ()
    elif kind == "xform":
        make, tile = (lambda: XformPlan(cfg, C, affine=True, device=0)), XformPlan(cfg, C, affine=True, device=-1).tile
        extra = (torch.from_numpy(w(C, K + 1)).cuda(),)
    else:
        stages = [("gru", w(3 * H, K), w(3 * H, H), w(3 * H), w(3 * H)), ("linear", w(C, H), w(C))]
        make, extra = (lambda: RnnPlan(cfg, stages, max_rows=1024, max_utts=4, device=0)), ()
        tile = XformPlan(cfg, 3 * H, affine=True, device=-1).tile  # stage 0's chain
    feats = torch.from_numpy(w(tile + 1, 8)).cuda()
    return make, (lambda plan: plan.compute(feats, [tile + 1], *extra))


DESTROY_FAMILIES = {"fdlp": _destroy_fdlp, "mel": lambda: _destroy_feat("mel"), "mfcc": lambda: _destroy_feat("mfcc"),
                    "post": lambda: _destroy_chain("post"), "xform": lambda: _destroy_chain("xform"),
                    "rnn": lambda: _destroy_chain("rnn")}


def test_destroy_right_after_compute():
    """A plan destroyed straight after its compute call, with the batch still in flight, leaves the same output as
    one that is synchronised first: destroy waits for the device before it frees what the kernels read."""
    for name, family in DESTROY_FAMILIES.items():
        make, run = family()
        outs = []
        for sync_first in (False, True):
            plan = make()
            out = run(plan)
            if sync_first:
                torch.cuda.synchronize()
            plan.close()
            torch.cuda.synchronize()
            outs.append(out.cpu())
        assert outs[0].numel() > 0 and torch.isfinite(outs[1]).all(), name
        assert torch.equal(outs[0], outs[1]), name
