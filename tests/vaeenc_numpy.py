"""numpy restatement of the stages speech_recognition_tools_amd/vaeenc.py runs (tests/test_vaeenc.py), in float64 or
float32: the same-padded Conv2d of VAECNNEncoderNopool over rows [t][c F + f], the per-utterance normaliser of
compute_vae_encoded_likelihood.py:128-129, and gru_numpy's GRU and linear stages around them.

Stages are tuples ("conv", w [Co, Ci, kh, kw], b), ("gru", w_ih, w_hh, b_ih, b_hh), ("linear", w, b) or ("norm",), as
VaeEncPlan takes them.  The ReLU after a conv stage is applied when the next stage loads its output.
"""
import numpy as np

import gru_numpy as GN

U = 2.0 ** -24


def im2col(rows, F, Ci, kh, kw, dtype=None):
    """[T, F, Ci kh kw] patches of one utterance's rows [T, Ci F] (channel-major): entry (t, f, k) with k the flat
    index of (ci, dh, dw) is rows[t + dw - pw][ci F + f + dh - ph], zero outside 0 <= f' < F and 0 <= t' < T"""
    rows = np.asarray(rows) if dtype is None else np.asarray(rows).astype(dtype)
    T = rows.shape[0]
    ph, pw = (kh - 1) // 2, (kw - 1) // 2
    img = np.zeros((T + kw - 1, Ci, F + kh - 1), dtype=rows.dtype)
    img[pw:pw + T, :, ph:ph + F] = rows.reshape(T, Ci, F)
    out = np.zeros((T, F, Ci, kh, kw), dtype=rows.dtype)
    for dh in range(kh):
        for dw in range(kw):
            out[:, :, :, dh, dw] = img[dw:dw + T, :, dh:dh + F].transpose(0, 2, 1)
    return out.reshape(T, F, Ci * kh * kw)


def conv_layer(rows, w, b, F, dtype=np.float64):
    """out [T, Co F] of one utterance's rows [T, Ci F] (already through the ReLU where one applies)"""
    w = np.asarray(w).astype(dtype)
    Co, Ci, kh, kw = w.shape
    cols = im2col(rows, F, Ci, kh, kw, dtype)                       # [T, F, K]
    out = cols @ w.reshape(Co, -1).T + np.asarray(b).astype(dtype)  # [T, F, Co]
    return np.ascontiguousarray(out.transpose(0, 2, 1)).reshape(rows.shape[0], Co * F)


def utt_norm(z, dtype=np.float64):
    """(z - mean_t z) / sqrt(var_t(z - mean_t z)), unbiased, per column; T = 1 gives NaN as IEEE does"""
    z = np.asarray(z).astype(dtype)
    T = z.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = z - z.sum(0) / dtype(T)
        e = d - d.sum(0) / dtype(T)
        return d / np.sqrt((e * e).sum(0) / dtype(T - 1))


def utt_norm_ref_and_bound(z):
    """The normaliser against ITS OWN input z [T, D] (float32, T >= 2), in float64, and the elementwise bound
        2U (|d| + |m|) / s + 4U |out|
    with m the mean, d = z - m, s the standard deviation.  The numerator: one rounding of m to float32 (<= U |m|; it
    moves every d_t alike, so the variance, taken about the mean of the d_t, does not see it) and one of z - m
    (<= U |d_t|), divided by s; the factor 2 is slack.  The denominator, relative to |out|: the roundings of the d_t
    move s by at most U s (d(s^2) <= 2 sum |e_t| U |d_t| / (T - 1) ~ 2U s^2), the float32 v by U / 2, the correctly
    rounded sqrt and the division by U each: 3.5U <= 4U.  The sums run in float64 and add nothing at this scale."""
    z = np.asarray(z).astype(np.float64)
    T = z.shape[0]
    m = z.sum(0) / T
    d = z - m
    s = np.sqrt(((d - d.sum(0) / T) ** 2).sum(0) / (T - 1))
    ref = d / s
    return ref, 2 * U * (np.abs(d) + np.abs(m)) / s + 4 * U * np.abs(ref)


def stage_input(prev, prev_kind):
    return np.maximum(prev, 0) if prev_kind in ("linear_relu", "conv") else prev


def forward(rows, stages, F=None, dtype=np.float64):
    """every stage's output for one utterance's rows [T, K] (a conv stage's is its pre-activation).  F: the image
    height of the conv stages (default: the width of `rows`, one input channel)"""
    outs, prev, kind = [], np.asarray(rows).astype(dtype), None
    F = prev.shape[1] if F is None else F
    for st in stages:
        a = stage_input(prev, kind)
        kind = st[0]
        if kind == "gru":
            prev = GN.gru_layer(a, *st[1:], dtype=dtype)
        elif kind == "conv":
            prev = conv_layer(a, st[1], st[2], F, dtype=dtype)
        elif kind == "norm":
            prev = utt_norm(a, dtype=dtype)
        else:
            prev = a @ np.asarray(st[1]).astype(dtype).T + np.asarray(st[2]).astype(dtype)
        outs.append(prev)
    return outs
