"""Mel spectrum sibling feature: src/featgen/computeMelSpectrum.py.

CPU: the oracle (oracle/mel_oracle.py) against the real reference's outputs (tests/golden/mel_*.npz), and
the host-side geometry.  GPU: MelPlan (mel_kernel through fdlp_mel_compute) against the goldens at 1e-6
(fp64 log10 mel energies; the reference computes in fp64 too) and the CLI drop-in's ark output; EDGE_MEL_SETS add
frames longer than nfft, nfft/2 = 300, nfft = 4096 and noise mixing on non-16-bit WAVs (API and CLI child process)."""
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle import fdlp_oracle as O
from oracle import mel_oracle as MO

MEL_SETS = ["mel_default", "mel_recipe15", "mel_cochlear_power", "mel_diff", "mel_noise_reverb"]
# short-signal sets (make_golden.py --sibling-edges-only): a frame longer than nfft (fft truncates), an odd frame
# zero-padded into nfft/2 = 300 = 2.2.3.5.5, nfft = 4096 (128 KiB of LDS: launch_mel's attribute branch), and noise
# mixing on float32 / 8-bit / 24-bit WAVs (mel_kernel's float64 PCM branch)
EDGE_MEL_SETS = ["mel_trunc256", "mel_nfft600_odd", "mel_nfft4096", "mel_kinds_noise"]


def _oracle_inputs(meta, sig, z):
    """Preprocessed float64 / int signals per utterance exactly as the reference loop does."""
    o = meta["opts"]
    an = o.get("add_noise", "clean")
    rng = np.random.RandomState(meta["extra"]["noise_seed"]) if "noise_seed" in meta["extra"] else None
    out = {}
    for u in meta["utts"]:
        x = sig[u]
        if an == "diff":
            x = O.diff_signal(x)
        elif an != "clean":
            x = O.add_noise(x, z["noise_babble"], float(an.split(",")[1]), rng.rand())
        if o.get("add_reverb", "clean") != "clean":
            x = O.add_reverb(x, O.load_rir(z["rir"]))
        out[u] = x
    return out


def _kw(meta):
    o = meta["opts"]
    return dict(nfilters=o["nfilters"], fduration=o["fduration"], frate=o["frate"], nfft=o["nfft"],
                fbank_type=o["fbank_type"], spectrum_type=o.get("spectrum_type", "log"))


@pytest.mark.parametrize("name", MEL_SETS + EDGE_MEL_SETS)
def test_mel_oracle_matches_reference(name):
    meta, sig, ref, z = load_golden(name)
    xs = _oracle_inputs(meta, sig, z)
    for u in meta["utts"]:
        got = MO.mel_spectrum(xs[u], **_kw(meta))
        assert got.shape == ref[u].shape, u
        np.testing.assert_allclose(got, ref[u], rtol=1e-10, atol=1e-10)


def test_mel_geometry_matches_getframes():
    from speech_recognition_tools_amd.melspec import MelConfig, MelPlan
    for fd, fr in ((0.02, 100), (0.025, 100), (0.0251, 67)):
        plan = MelPlan(MelConfig(fduration=fd, frate=fr), device=-1)
        for T in (1, 2, 150, 319, 320, 321, 16000, 23457):
            assert plan.frames(T) == MO.get_frames(np.zeros(T), 16000, fr, fd).shape[0], (fd, fr, T)


@pytest.mark.parametrize("name", EDGE_MEL_SETS)
def test_mel_edge_plans_accept_and_size(name):
    """A host-only plan takes every edge configuration (nfft/2 = 128, 300, 2048, 512) and counts the reference's
    frames; the 300-sample utterance is shorter than one frame."""
    from speech_recognition_tools_amd.melspec import MelConfig, MelPlan
    meta, sig, ref, _ = load_golden(name)
    plan = MelPlan(MelConfig(**_kw(meta)), device=-1)
    for u in meta["utts"]:
        assert (plan.frames(sig[u].size), plan.B) == ref[u].shape, u
        assert np.isfinite(ref[u]).all(), u
    assert min(sig[u].size for u in meta["utts"]) < int(16000 * meta["opts"]["fduration"])


def test_mel_kinds_noise_fixture_is_not_int16():
    """mel_kinds_noise holds float32, uint8 and left-justified 24-bit signals, the WAV bytes the reference read,
    and the noise moves the features far more than any tolerance here (so a kernel that skips the mixing fails)."""
    from speech_recognition_tools_amd.featgen.features import read_wav_bytes
    meta, sig, ref, z = load_golden("mel_kinds_noise")
    assert [str(sig[u].dtype) for u in meta["utts"]] == ["float32", "uint8", "int32"]
    assert not (sig["ki24"] & 0xFF).any()
    for u in meta["utts"]:
        sr, x = read_wav_bytes(z["wav_" + u].tobytes())
        assert sr == 16000 and x.scipy_kind == str(sig[u].dtype), u
        np.testing.assert_array_equal(np.asarray(x), sig[u].astype(np.float64))
        clean = MO.mel_spectrum(sig[u], **_kw(meta))
        assert np.abs(clean - ref[u]).max() > 0.01, u  # ten '%.3f' ark steps, 1e7 times the GPU bar


def _mel_gpu(meta, sig, z, max_frames=4096, as_f64=False):
    import torch
    from speech_recognition_tools_amd import NpRandom
    from speech_recognition_tools_amd.augment import noise_params, reverb
    from speech_recognition_tools_amd.melspec import MelConfig, MelPlan
    plan = MelPlan(MelConfig(**_kw(meta)), device=0, max_frames=max_frames)
    utts = meta["utts"]
    lens = [sig[u].size for u in utts]
    # other WAV dtypes (mel_kinds_noise) go to the device as their float64 values; alpha is taken on the stored dtype
    wide = as_f64 or any(sig[u].dtype != np.int16 for u in utts)
    pcm = torch.from_numpy(np.concatenate([sig[u].astype(np.float64) if wide else sig[u] for u in utts])).cuda()
    an = meta["opts"].get("add_noise", "clean")
    kw = {}
    if an == "diff":
        kw["preprocess"] = "diff"
    elif an != "clean":
        noise = z["noise_babble"]
        nr = NpRandom(meta["extra"]["noise_seed"])
        offs, alps = zip(*[noise_params(sig[u], noise, float(an.split(",")[1]), nr.rand()) for u in utts])
        kw = dict(noise=torch.from_numpy(noise).cuda(), noise_off=list(offs), noise_alpha=list(alps))
    if meta["opts"].get("add_reverb", "clean") != "clean":
        pcm, lens = reverb(pcm, lens, torch.from_numpy(O.load_rir(z["rir"])).cuda(), **kw)
        kw = {}
    out, rows, out64 = plan.compute(pcm, lens, want_f64=True, **kw)
    out, out64 = out.cpu().numpy(), out64.cpu().numpy()
    return {u: (out64[rows[i]:rows[i + 1]], out[rows[i]:rows[i + 1]]) for i, u in enumerate(utts)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", MEL_SETS + EDGE_MEL_SETS)
def test_mel_gpu_vs_reference_golden(name):
    meta, sig, ref, z = load_golden(name)
    res = _mel_gpu(meta, sig, z)
    for u in meta["utts"]:
        f64, f32 = res[u]
        assert f64.shape == ref[u].shape, u
        scale = np.maximum(1.0, np.abs(ref[u]))
        assert np.max(np.abs(f64 - ref[u]) / scale) <= 1e-9, (name, u)
        np.testing.assert_allclose(f32, np.round(ref[u], 3).astype(np.float32), rtol=0, atol=1.0011e-3 * scale.max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mel_default", "mel_trunc256", "mel_nfft600_odd", "mel_nfft4096", "mel_noise_reverb"])
def test_mel_float64_pcm_equals_int16(name):
    """int16 samples handed over as float64.  Bit-identity, read from mel_kernel: its int16 branch is
    (double)pcm[t] and its float64 branch the load of that same double, each followed by the same
    __dadd_rn(sv, __dmul_rn(alpha, noise)) when noise is mixed and by the one __dmul_rn with the window.
    mel_noise_reverb runs without its reverberation (the noise mixing alone, same alpha for both kinds)."""
    meta, sig, _, z = load_golden(name)
    meta = dict(meta, opts=dict(meta["opts"], add_reverb="clean"))
    a, b = _mel_gpu(meta, sig, z), _mel_gpu(meta, sig, z, as_f64=True)
    for u in meta["utts"]:
        assert np.isfinite(a[u][0]).all(), u
        np.testing.assert_array_equal(a[u][0], b[u][0], err_msg=u)
        np.testing.assert_array_equal(a[u][1], b[u][1], err_msg=u)


@pytest.mark.gpu
def test_mel_cli_mixes_noise_into_other_wav_formats(tmp_path):
    """compute-mel-feats --add_noise babble,10 in a child process on the float32, 8-bit and 24-bit WAV files the
    reference read (mel_kinds_noise): the ark against the reference's features."""
    import subprocess
    from scipy.io import wavfile
    from conftest import ROOT
    from speech_recognition_tools_amd.featgen.features import read_ark
    meta, sig, ref, z = load_golden("mel_kinds_noise")
    (tmp_path / "noises").mkdir()
    wavfile.write(str(tmp_path / "noises" / "babble.wav"), 16000, z["noise_babble"])
    scp = tmp_path / "wav.scp"
    with open(scp, "w") as f:
        for u in meta["utts"]:
            p = tmp_path / (u + ".wav")
            p.write_bytes(z["wav_" + u].tobytes())
            f.write("%s %s\n" % (u, p))
    out = str(tmp_path / "melk")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([os.path.join(ROOT, "bin", "compute-mel-feats"), str(scp), out,
                        "--add_noise=" + meta["opts"]["add_noise"], "--noise_seed=%d" % meta["extra"]["noise_seed"]],
                       cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode("utf-8", "replace")
    ark = read_ark(out + ".ark")
    assert list(ark) == meta["utts"]
    for u in meta["utts"]:
        q = np.round(ref[u], 3).astype(np.float32)
        assert ark[u].shape == q.shape, u
        assert np.abs(ark[u] - q).max() <= 1.0011e-3, (u, np.abs(ark[u] - q).max())


@pytest.mark.gpu
def test_mel_cli_writes_reference_arks(tmp_path):
    from scipy.io import wavfile
    from speech_recognition_tools_amd.featgen.computeMelSpectrum import get_args, compute_mel_spectrum
    from speech_recognition_tools_amd.featgen.features import read_ark
    meta, sig, ref, z = load_golden("mel_recipe15")
    scp = tmp_path / "wav.scp"
    with open(scp, "w") as f:
        for u in meta["utts"]:
            p = tmp_path / (u + ".wav")
            wavfile.write(str(p), 16000, sig[u])
            f.write("%s %s\n" % (u, p))
    o = meta["opts"]
    out = str(tmp_path / "mel")
    compute_mel_spectrum(get_args([str(scp), out, "--nfilters=%d" % o["nfilters"], "--nfft=%d" % o["nfft"],
                                   "--fduration=%s" % o["fduration"], "--frate=%d" % o["frate"],
                                   "--fbank_type=" + o["fbank_type"], "--spectrum_type=log",
                                   "--add_noise=clean", "--add_reverb=clean", "--write_utt2num_frames"]))
    ark = read_ark(out + ".ark")
    assert list(ark) == meta["utts"]
    lens = dict(l.split() for l in open(out + ".len"))
    for u in meta["utts"]:
        q = np.round(ref[u], 3).astype(np.float32)
        assert ark[u].shape == q.shape and int(lens[u]) == q.shape[0]
        assert np.abs(ark[u] - q).max() <= 1.0011e-3
