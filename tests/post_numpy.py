"""numpy restatement of apply-cmvn | add-deltas | splice-feats as speech_recognition_tools_amd/post.py documents
them (Kaldi's transform/cmvn.cc ApplyCmvn, feature-functions.cc DeltaFeatures and SpliceFrames).  Written from
the documented behaviour, independently of the library: tests/test_post.py holds the device kernel and the C
host functions against it."""
import numpy as np


def scale_tables(order, window):
    """[scales[0] .. scales[order]] in float32.  scales[i][j + k] += j * scales[i-1][k] over j = -window..window,
    over sum j^2; kept as integer numerators over (sum j^2)^i and rounded once."""
    norm = sum(j * j for j in range(-window, window + 1))
    prev, out = [1], [np.array([1.0], dtype=np.float32)]
    for i in range(1, order + 1):
        po = (len(prev) - 1) // 2
        cur = [0] * (len(prev) + 2 * window)
        for j in range(-window, window + 1):
            for k in range(-po, po + 1):
                cur[j + k + po + window] += j * prev[k + po]
        out.append((np.array(cur, dtype=np.float64) / float(norm ** i)).astype(np.float32))
        prev = cur
    return out


def cmvn_norm(stats, norm_means=True, norm_vars=False, reverse=False, skip_dims=()):
    """float32 [2, D]: scale row and offset row, computed in double."""
    stats = np.asarray(stats, dtype=np.float64)
    D = stats.shape[1] - 1
    count = stats[0, D]
    if count < 1.0:
        raise ValueError("insufficient stats")
    if norm_vars and not norm_means:
        raise ValueError("You cannot normalize the variance but not the mean")
    scale, offset = np.ones(D), np.zeros(D)
    if norm_means:
        mean = stats[0, :D] / count
        if norm_vars:
            var = np.maximum(stats[1, :D] / count - mean * mean, 1e-20)
            scale = np.sqrt(var) if reverse else 1.0 / np.sqrt(var)
        offset = mean if reverse else -(mean * scale)
    for d in skip_dims:
        scale[d], offset[d] = 1.0, 0.0
    return np.stack([scale, offset]).astype(np.float32)


def apply_cmvn(x, norm, norm_vars=True):
    """fl32(fl32(x * scale) + offset): two float32 roundings; the multiply only when variances are normalised."""
    x = np.asarray(x, dtype=np.float32)
    if norm is None:
        return x.copy()
    y = x
    if norm_vars:
        y = (y * norm[0][None, :]).astype(np.float32)
    return (y + norm[1][None, :]).astype(np.float32)


def _clamped(T, j):
    return np.clip(np.arange(T) + j, 0, T - 1)


def add_deltas(y, order, window, truncate=0, dtype=np.float32):
    """[y | d | dd ..]: block i of frame t = sum_j scales[i][j] * y[clamp(t + j)], accumulated in `dtype` in
    ascending j (zero taps skipped).  Also returns sum_j |scales[i][j] * y[clamp(t + j)]| in float64."""
    y = np.asarray(y, dtype=np.float32)
    if truncate:
        y = y[:, :truncate]
    T = y.shape[0]
    blocks, mags = [y.astype(dtype)], [np.abs(y).astype(np.float64)]
    for i, s in enumerate(scale_tables(order, window)):
        if i == 0:
            continue
        hw = (len(s) - 1) // 2
        acc = np.zeros(y.shape, dtype=dtype)
        mag = np.zeros(y.shape, dtype=np.float64)
        for j in range(-hw, hw + 1):
            sj = s[j + hw]
            if sj == 0:
                continue
            term = (dtype(sj) * y[_clamped(T, j)].astype(dtype)).astype(dtype)
            acc = (acc + term).astype(dtype)
            mag += np.abs(np.float64(sj) * y[_clamped(T, j)].astype(np.float64))
        blocks.append(acc)
        mags.append(mag)
    return np.concatenate(blocks, axis=1), np.concatenate(mags, axis=1)


def splice(z, left, right):
    """row t = [z[clamp(t - left)] .. z[clamp(t + right)]] (edges replicated)."""
    T = z.shape[0]
    return np.concatenate([z[_clamped(T, j)] for j in range(-left, right + 1)], axis=1)


def post(x, norm=None, norm_vars=True, order=0, window=2, truncate=0, left=0, right=0):
    """The whole chain of one utterance in float32."""
    z, _ = add_deltas(apply_cmvn(x, norm, norm_vars), order, window, truncate)
    return splice(z, left, right)
