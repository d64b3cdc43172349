"""numpy restatement of the stages speech_recognition_tools_amd/rnn.py runs (tests/test_rnn.py), in float64 or
float32: nn.GRU as torch documents it (gate order r, z, n), a linear stage, the ReLU between a 'linear_relu' stage
and the next one, and the row epilogues.

  gh = W_hh h_{t-1} + b_hh,  r = s(G_r[t] + gh_r),  z = s(G_z[t] + gh_z),  n = tanh(G_n[t] + r gh_n),
  h_t = (1 - z) n + z h_{t-1},  G = x W_ih^T + b_ih,  h_{-1} = 0

Stages are tuples ("gru", w_ih, w_hh, b_ih, b_hh) or ("linear" | "linear_relu", w, b), as RnnPlan takes them.
"""
import numpy as np

U = 2.0 ** -24


def sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def gru_layer(x, w_ih, w_hh, b_ih, b_hh, dtype=np.float64):
    """h [T, H] of one utterance x [T, K]"""
    x, w_ih, w_hh, b_ih, b_hh = (np.asarray(a).astype(dtype) for a in (x, w_ih, w_hh, b_ih, b_hh))
    H = w_hh.shape[1]
    G = x @ w_ih.T + b_ih
    h = np.zeros(H, dtype=dtype)
    out = np.zeros((x.shape[0], H), dtype=dtype)
    one = dtype(1)
    for t in range(x.shape[0]):
        gh = w_hh @ h + b_hh
        r = one / (one + np.exp(-(G[t, :H] + gh[:H])))
        z = one / (one + np.exp(-(G[t, H:2 * H] + gh[H:2 * H])))
        n = np.tanh(G[t, 2 * H:] + r * gh[2 * H:])
        h = (one - z) * n + z * h
        out[t] = h
    return out


def stage_input(prev, prev_kind):
    """what a stage loads: the previous stage's output, through the ReLU after a 'linear_relu' stage"""
    return np.maximum(prev, 0) if prev_kind == "linear_relu" else prev


def forward(rows, stages, dtype=np.float64):
    """every stage's output for one utterance's rows [T, K] (a 'linear_relu' stage's is its pre-activation)"""
    outs, prev, kind = [], np.asarray(rows).astype(dtype), None
    for st in stages:
        a = stage_input(prev, kind)
        kind = st[0]
        if kind == "gru":
            prev = gru_layer(a, *st[1:], dtype=dtype)
        else:
            prev = a @ np.asarray(st[1]).astype(dtype).T + np.asarray(st[2]).astype(dtype)
        outs.append(prev)
    return outs


def gru_step_ref_and_bound(x, h_own, w_ih, w_hh, b_ih, b_hh):
    """Every step of a GRU stage against ITS OWN input, for one utterance: x [T, K] the float32 rows the stage
    loaded, h_own [T, H] the float32 states the device produced.  h_{t-1} is row t - 1 of h_own (0 at t = 0), so no
    error propagates through time.  Returns the float64 h_t [T, H] and the elementwise bound dh of tests/test_rnn.py:
      e_i = (K + 2) U (|x| |W_ih|^T + |b_ih|),  e_h = (H + 2) U (|h| |W_hh|^T + |b_hh|),  q = W_hn h + b_hn
      dr = (e_i,r + e_h,r + 2U |a_r|) / 4 + 8U, dz likewise
      dn = e_i,n + r e_h,n + (|q| + e_h,n) dr + 2U (|a_n| + |r q|) + 8U
      dh = (|n - h| + dn) dz + (1 - z) dn + 4U (|n| + |h|)"""
    x, h_own, w_ih, w_hh, b_ih, b_hh = (np.asarray(a).astype(np.float64) for a in (x, h_own, w_ih, w_hh, b_ih, b_hh))
    T, K = x.shape
    H = w_hh.shape[1]
    h = np.vstack([np.zeros((1, H)), h_own[:-1]])
    gi = x @ w_ih.T + b_ih
    gh = h @ w_hh.T + b_hh
    e_i = (K + 2) * U * (np.abs(x) @ np.abs(w_ih).T + np.abs(b_ih))
    e_h = (H + 2) * U * (np.abs(h) @ np.abs(w_hh).T + np.abs(b_hh))
    R, Z, N = slice(0, H), slice(H, 2 * H), slice(2 * H, 3 * H)
    a_r, a_z = gi[:, R] + gh[:, R], gi[:, Z] + gh[:, Z]
    r, z = sigmoid(a_r), sigmoid(a_z)
    q = gh[:, N]
    a_n = gi[:, N] + r * q
    n = np.tanh(a_n)
    ref = (1 - z) * n + z * h
    dr = (e_i[:, R] + e_h[:, R] + 2 * U * np.abs(a_r)) / 4 + 8 * U
    dz = (e_i[:, Z] + e_h[:, Z] + 2 * U * np.abs(a_z)) / 4 + 8 * U
    dn = e_i[:, N] + r * e_h[:, N] + (np.abs(q) + e_h[:, N]) * dr + 2 * U * (np.abs(a_n) + np.abs(r * q)) + 8 * U
    dh = (np.abs(n - h) + dn) * dz + (1 - z) * dn + 4 * U * (np.abs(n) + np.abs(h))
    return ref, dh


def softmax(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def loglike(x, prior, w):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(1, keepdims=True)) - w * np.asarray(prior, dtype=np.float64)
