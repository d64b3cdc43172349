"""FDLP modulation spectrum sibling feature: src/featgen/computeModulationSpectrum.py.

CPU: the oracle (oracle/modspec_oracle.py) against the real reference's outputs (tests/golden/modspec_*.npz,
made by tests/golden/make_golden.py --modspec-only), host-side geometry and option validation.  GPU: the FDLP
plan in its modspec mode against the goldens (fp64 cepstra, relative 1e-7: the reference computes in fp64, the
device differs only by summation order in the DCT/autocorrelation/Levinson), a reverberated batch against the
oracle, and the compute-modspec-feats CLI's ark ('%.3f' rounding, as dict2Ark).  The complex kernels are also held
to the reference at orders 65-236 and coeff_n 300 (EDGE_COMPLEX_SETS: more than one loop trip per lane), batching
invariance and float64 PCM input included."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import fdlp_oracle as O
from oracle import mel_oracle as MO
from oracle import modspec_oracle as MS

MODSPEC_SETS = ["modspec_default", "modspec_even_comp_abs", "modspec_cochlear_rect"]
COMPLEX_SETS = ["modspec_complex", "modspec_complex_even_comp_abs", "modspec_complex_cochlear_rect"]
# short-signal sets at the sizes where the 64-lane loops of cplx_autocorr_kernel / cplx_lpc_out_kernel run more
# than once per lane (make_golden.py --sibling-edges-only; DESIGN.md, parity section): order + 2 = 67 / 68 / 132 /
# 238 lags, 1 / 2 / 3 / 4 Durbin values per lane (the update of step k holds k - 1 values, so order 65 still has one
# per lane and order 66 is the first with two), and coeff_n = 300 > order + 1 = 41 (zero-extended a, 5 cepstrum trips)
EDGE_COMPLEX_SETS = ["modspec_complex_o65", "modspec_complex_o66", "modspec_complex_o130", "modspec_complex_o236",
                     "modspec_complex_c300"]
EDGE_MAX_FRAMES = 24  # the edge sets have 16 + 7 + 11 frames: two compute calls
TOL = 1e-7
# modspec_complex_o236 (order 236 on 2500 samples, values scaled by faxis up to 400) is not held to TOL: Levinson at
# that order amplifies a rounding-sized change of the autocorrelation far beyond it.  Its bar comes from the oracle
# alone (test_o236_bar_is_the_oracles_response_to_autocorr_rounding): every lag of every band's y moved by the direct
# sum's own error bound (hi - lo) 2^-53 sum|terms| with seeded signs moves the oracle's features of utterance e1
# (the worst of the three, seeds 1-3) by O236_RESPONSE relative to max(1, |ref|); four times that is allowed, the
# margin covering the recursion's own rounding.  The bound is a worst case (errors adding up over ~10^3 taps), so
# the bar is wide: the device's own deviation, printed by the GPU test, was 1.6e-6 when this was written.
O236_RESPONSE = 1.3346e-3
EDGE_TOL = {"modspec_complex_o236": 4 * O236_RESPONSE}


def _y_rounding_hook(seed):
    """y_hook of MS.modspec_complex_features: y[l] +- (hi - lo) 2^-53 sum_n |s[n + l]| |s[n]| in the real and the
    imaginary part (lag 0 stays real), the error bound of cplx_autocorr_kernel's direct sum over the band's taps."""
    rng = np.random.default_rng(seed)

    def hook(y, s):
        nz = np.flatnonzero(s)
        mags = np.abs(s)
        terms = np.real(np.fft.ifft(np.abs(np.fft.fft(mags)) ** 2))  # circular sum_n |s[n + l]| |s[n]|
        bound = (nz[-1] - nz[0] + 1) * 2.0 ** -53 * terms
        d = bound * (rng.choice([-1.0, 1.0], y.size) + 1j * rng.choice([-1.0, 1.0], y.size))
        d[0] = d[0].real
        return y + d
    return hook


def test_o236_bar_is_the_oracles_response_to_autocorr_rounding():
    meta, sig, ref, _ = load_golden("modspec_complex_o236")
    x = sig["e1"].astype(np.float64)
    base = MS.modspec_complex_features(x, **_opts(meta["opts"]))
    moved = MS.modspec_complex_features(x, y_hook=_y_rounding_hook(1), **_opts(meta["opts"]))
    response = np.max(np.abs(moved - base) / np.maximum(1.0, np.abs(ref["e1"])))
    assert response == pytest.approx(O236_RESPONSE, rel=0.02), response
    assert response > 1e3 * TOL


@pytest.mark.parametrize("name", MODSPEC_SETS)
def test_modspec_oracle_matches_reference(name):
    meta, sig, ref, _ = load_golden(name)
    for u in meta["utts"]:
        got = MS.modspec_features(sig[u].astype(np.float64), **meta["opts"])
        assert got.shape == ref[u].shape, u
        np.testing.assert_allclose(got, ref[u], rtol=1e-9, atol=1e-9)


def _opts(o):
    o = dict(o)
    o.pop("complex_modulation", None)
    return o


@pytest.mark.parametrize("name", COMPLEX_SETS + EDGE_COMPLEX_SETS)
def test_modspec_complex_oracle_matches_reference(name):
    meta, sig, ref, _ = load_golden(name)
    for u in meta["utts"]:
        got = MS.modspec_complex_features(sig[u].astype(np.float64), **_opts(meta["opts"]))
        assert got.shape == ref[u].shape, u
        np.testing.assert_allclose(got, ref[u], rtol=1e-9, atol=1e-9)


def test_modspec_complex_geometry_and_validation():
    from speech_recognition_tools_amd._lib import FdlpError
    from speech_recognition_tools_amd.plan import FdlpPlan, FeatureConfig
    for name in COMPLEX_SETS:
        meta, _, ref, _ = load_golden(name)
        plan = FdlpPlan(_cfg(meta["opts"]), device=-1, max_frames=16)
        assert plan.out_dim == ref[meta["utts"][0]].shape[1], name
    with pytest.raises(FdlpError):  # keep_even without abs: the reference's broadcast error
        FdlpPlan(FeatureConfig(mode="modspec_complex", nfilters=15, coeff_num=30, coeff_0=5, order=50,
                               keep_even=True), device=-1)


@pytest.mark.parametrize("name", EDGE_COMPLEX_SETS)
def test_modspec_complex_edge_plans_accept_and_size(name):
    """A host-only plan takes every edge configuration (order up to 236 < 238, coeff_n up to 300 <= 1024), and
    its width and frame counts are the reference's; the signals need two calls at EDGE_MAX_FRAMES."""
    from speech_recognition_tools_amd.plan import FdlpPlan
    meta, sig, ref, _ = load_golden(name)
    o = meta["opts"]
    plan = FdlpPlan(_cfg(o), device=-1, max_frames=EDGE_MAX_FRAMES)
    assert plan.nlags == o["order"] + 2
    assert plan.lpc_dispatch()["durbin"][0] == "cplx"
    frames = []
    for u in meta["utts"]:
        F, L = plan.geometry(sig[u].size)
        assert (L, plan.out_dim) == ref[u].shape and F == L, u
        frames.append(F)
    assert max(frames) <= EDGE_MAX_FRAMES < sum(frames)
    assert len(_groups(plan, sig, meta["utts"])) == 2


def _groups(plan, sig, utts):
    """Consecutive utterances per compute call, as the CLI fills a plan of max_frames analysis frames."""
    groups, n = [[]], 0
    for u in utts:
        F = plan.geometry(sig[u].size)[0]
        if groups[-1] and n + F > plan.max_frames:
            groups.append([])
            n = 0
        groups[-1].append(u)
        n += F
    return groups


def _cfg(o):
    from speech_recognition_tools_amd.plan import FeatureConfig
    return FeatureConfig(mode="modspec_complex" if o.get("complex_modulation") else "modspec",
                         window="rect" if o.get("no_window") else "hanning",
                         nfilters=o["nfilters"], coeff_num=o["coeff_n"], coeff_0=o["coeff_0"], order=o["order"],
                         fduration=o["fduration"], frate=o["frate"], fbank_type=o["fbank_type"],
                         keep_even=bool(o.get("keep_even")), compensate_noise=bool(o.get("compensate_noise")),
                         absolute_value=bool(o.get("absolute_value")))


def test_modspec_geometry_and_width():
    from speech_recognition_tools_amd.plan import FdlpPlan
    for name in MODSPEC_SETS:
        meta, _, ref, _ = load_golden(name)
        o = meta["opts"]
        plan = FdlpPlan(_cfg(o), device=-1, max_frames=16)
        assert plan.out_dim == ref[meta["utts"][0]].shape[1]
        for T in (2, 100, 3999, 4000, 4001, 8000, 23457):
            F, L = plan.geometry(T)
            assert F == L == MO.get_frames(np.zeros(T), 16000, o["frate"], o["fduration"], np.hanning).shape[0]


def test_modspec_option_validation():
    from speech_recognition_tools_amd._lib import FdlpError
    from speech_recognition_tools_amd.plan import FdlpPlan, FeatureConfig
    for bad in (dict(coeff_0=0), dict(coeff_0=31), dict(gamma_weight="1,2,3"), dict(odd_mod_zero=True)):
        kw = dict(mode="modspec", nfilters=15, coeff_num=30, coeff_0=5, order=50)
        kw.update(bad)
        with pytest.raises(FdlpError):
            FdlpPlan(FeatureConfig(**kw), device=-1)


def test_modspec_cli_args():
    from speech_recognition_tools_amd.featgen.computeModulationSpectrum import feature_config, get_args
    a = get_args(["s.scp", "out"])
    assert (a.nfilters, a.coeff_0, a.coeff_n, a.order, a.fduration, a.frate, a.fbank_type) == \
        (15, 5, 30, 50, 0.5, 100, "mel,1")
    c = feature_config(get_args(["s.scp", "out", "--no_window", "--keep_even", "--coeff_0=2"]))
    assert c.mode == "modspec" and c.window == "rect" and c.keep_even and c.coeff_0 == 2
    assert feature_config(get_args(["s.scp", "out", "--complex_modulation"])).mode == "modspec_complex"


def _modspec_gpu(cfg, sig, utts, rir=None, max_frames=4096, as_f64=False):
    import torch
    from speech_recognition_tools_amd.augment import reverb
    from speech_recognition_tools_amd.plan import FdlpPlan
    plan = FdlpPlan(cfg, device=0, max_frames=max_frames)
    lens = [sig[u].size for u in utts]
    x = np.concatenate([sig[u] for u in utts])
    pcm = torch.from_numpy(x.astype(np.float64) if as_f64 else x).cuda()
    offs = None
    if rir is not None:
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        pcm, lens = reverb(pcm, lens, torch.from_numpy(rir).cuda(), offsets=offs)
    out, rows, out64 = plan.compute(pcm, lens, None, offsets=offs, want_f64=True)
    out, out64 = out.cpu().numpy(), out64.cpu().numpy()
    return {u: (out64[rows[i]:rows[i + 1]], out[rows[i]:rows[i + 1]]) for i, u in enumerate(utts)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODSPEC_SETS)
def test_modspec_gpu_vs_reference_golden(name):
    meta, sig, ref, _ = load_golden(name)
    res = _modspec_gpu(_cfg(meta["opts"]), sig, meta["utts"])
    for u in meta["utts"]:
        f64, f32 = res[u]
        assert f64.shape == ref[u].shape, u
        scale = np.maximum(1.0, np.abs(ref[u]))
        assert np.max(np.abs(f64 - ref[u]) / scale) <= TOL, (name, u, np.max(np.abs(f64 - ref[u]) / scale))
        np.testing.assert_allclose(f32, np.round(ref[u], 3).astype(np.float32), rtol=0, atol=1.0011e-3 * scale.max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", COMPLEX_SETS)
def test_modspec_complex_gpu_vs_reference_golden(name):
    meta, sig, ref, _ = load_golden(name)
    res = _modspec_gpu(_cfg(meta["opts"]), sig, meta["utts"])
    for u in meta["utts"]:
        f64, f32 = res[u]
        assert f64.shape == ref[u].shape, u
        scale = np.maximum(1.0, np.abs(ref[u]))
        assert np.max(np.abs(f64 - ref[u]) / scale) <= TOL, (name, u, np.max(np.abs(f64 - ref[u]) / scale))
        np.testing.assert_allclose(f32, np.round(ref[u], 3).astype(np.float32), rtol=0, atol=1.0011e-3 * scale.max())


_EDGE_RUNS = {}


def _edge_gpu(name):
    """{utt: (f64, f32)} of an edge set computed as the CLI would at EDGE_MAX_FRAMES (two compute calls), once."""
    if name not in _EDGE_RUNS:
        from speech_recognition_tools_amd.plan import FdlpPlan
        meta, sig, _, _ = load_golden(name)
        cfg = _cfg(meta["opts"])
        res = {}
        for g in _groups(FdlpPlan(cfg, device=-1, max_frames=EDGE_MAX_FRAMES), sig, meta["utts"]):
            res.update(_modspec_gpu(cfg, sig, g, max_frames=EDGE_MAX_FRAMES))
        _EDGE_RUNS[name] = res
    return _EDGE_RUNS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_COMPLEX_SETS)
def test_modspec_complex_edge_gpu_vs_reference_golden(name):
    """cplx_autocorr_kernel's second to fourth lag trip and cplx_lpc_out_kernel with 2-4 Durbin values per lane,
    cepstrum sums over more than 64 terms and the zero-extended a, against the reference at the bar of
    test_modspec_complex_gpu_vs_reference_golden."""
    meta, sig, ref, _ = load_golden(name)
    res = _edge_gpu(name)
    for u in meta["utts"]:
        f64, f32 = res[u]
        assert f64.shape == ref[u].shape, u
        scale = np.maximum(1.0, np.abs(ref[u]))
        err = np.max(np.abs(f64 - ref[u]) / scale)
        print("%s %s: max relative error %.3g" % (name, u, err))
        assert err <= EDGE_TOL.get(name, TOL), (name, u, err)
        np.testing.assert_allclose(f32, np.round(ref[u], 3).astype(np.float32), rtol=0, atol=1.0011e-3 * scale.max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_COMPLEX_SETS)
def test_modspec_complex_edge_alone_equals_batch(name):
    """One wave per (frame, band) item and no state shared between items: every utterance alone, the two-call
    split and one batch of all three are bit-identical."""
    meta, sig, _, _ = load_golden(name)
    cfg = _cfg(meta["opts"])
    whole = _modspec_gpu(cfg, sig, meta["utts"])
    split = _edge_gpu(name)
    for u in meta["utts"]:
        alone = _modspec_gpu(cfg, sig, [u], max_frames=EDGE_MAX_FRAMES)[u]
        for other in (alone, split[u]):
            np.testing.assert_array_equal(whole[u][0], other[0], err_msg=u)
            np.testing.assert_array_equal(whole[u][1], other[1], err_msg=u)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_COMPLEX_SETS)
def test_modspec_complex_float64_pcm_equals_int16(name):
    """int16 samples handed over as float64.  Bit-identity, read from the code: with complex modulation the frames
    go through frames_dft1_kernel<false>, whose samples all come from makhoul_sample (fdlp_dct.hip); without
    noise its int16 branch is (double)pcm[t] and its float64 branch the load of that same double, and both are
    followed by the one __dmul_rn with the window."""
    meta, sig, _, _ = load_golden(name)
    cfg = _cfg(meta["opts"])
    a = _modspec_gpu(cfg, sig, meta["utts"])
    b = _modspec_gpu(cfg, sig, meta["utts"], as_f64=True)
    for u in meta["utts"]:
        np.testing.assert_array_equal(a[u][0], b[u][0], err_msg=u)
        np.testing.assert_array_equal(a[u][1], b[u][1], err_msg=u)


@pytest.mark.gpu
def test_modspec_gpu_reverb_vs_oracle():
    meta, sig, _, _ = load_golden("modspec_default")
    _, _, _, zr = load_golden("reverb_rir")
    rir = O.load_rir(zr["rir"])
    res = _modspec_gpu(_cfg(meta["opts"]), sig, meta["utts"], rir=rir)
    for u in meta["utts"]:
        want = MS.modspec_features(O.add_reverb(sig[u], rir), **meta["opts"])
        f64 = res[u][0]
        assert f64.shape == want.shape, u
        assert np.max(np.abs(f64 - want) / np.maximum(1.0, np.abs(want))) <= TOL, u


@pytest.mark.gpu
def test_modspec_cli_writes_reference_arks(tmp_path):
    from scipy.io import wavfile
    from speech_recognition_tools_amd.featgen.computeModulationSpectrum import get_args, get_feats
    from speech_recognition_tools_amd.featgen.features import read_ark
    meta, sig, ref, _ = load_golden("modspec_even_comp_abs")
    scp = tmp_path / "wav.scp"
    with open(scp, "w") as f:
        for u in meta["utts"]:
            p = tmp_path / (u + ".wav")
            wavfile.write(str(p), 16000, sig[u])
            f.write("%s %s\n" % (u, p))
    out = str(tmp_path / "modspec")
    get_feats(get_args([str(scp), out, "--keep_even", "--compensate_noise", "--absolute_value",
                        "--add_reverb=clean", "--kaldi_cmd=copy-feats"]))
    ark = read_ark(out + ".ark")
    assert list(ark) == meta["utts"]
    scp_keys = [l.split()[0] for l in open(out + ".scp")]
    assert scp_keys == meta["utts"]
    for u in meta["utts"]:
        q = np.round(ref[u], 3).astype(np.float32)
        assert ark[u].shape == q.shape
        assert np.abs(ark[u] - q).max() <= 1.0011e-3 * max(1.0, np.abs(ref[u]).max())


@pytest.mark.gpu
def test_modspec_complex_cli_writes_reference_arks(tmp_path):
    from scipy.io import wavfile
    from speech_recognition_tools_amd.featgen.computeModulationSpectrum import get_args, get_feats
    from speech_recognition_tools_amd.featgen.features import read_ark
    meta, sig, ref, _ = load_golden("modspec_complex")
    scp = tmp_path / "wav.scp"
    with open(scp, "w") as f:
        for u in meta["utts"]:
            p = tmp_path / (u + ".wav")
            wavfile.write(str(p), 16000, sig[u])
            f.write("%s %s\n" % (u, p))
    out = str(tmp_path / "modspec_c")
    get_feats(get_args([str(scp), out, "--complex_modulation"]))
    ark = read_ark(out + ".ark")
    assert list(ark) == meta["utts"]
    for u in meta["utts"]:
        q = np.round(ref[u], 3).astype(np.float32)
        assert ark[u].shape == q.shape
        assert np.abs(ark[u] - q).max() <= 1.0011e-3 * max(1.0, np.abs(ref[u]).max())
