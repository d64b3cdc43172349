"""Feature post-processing on the MI355X: drop-ins for Kaldi's `apply-cmvn`, `add-deltas` and `splice-feats`,
the chain every consumer of the reference pipes its arks through (recipes/timit/local_pyspeech/decode.sh:84-90,
get_Tandem_feats.sh:31-35, make_mfcc_feats.sh:108-118, the `apply-cmvn ... | splice-feats ... |` strings of
src/nnet/data_prep_*.py), plus `post-feats`, the three fused into one launch per batch.

Kaldi semantics restated (transform/cmvn.cc ApplyCmvn / ApplyCmvnReverse, feat/feature-functions.cc
DeltaFeatures and SpliceFrames; Kaldi itself is not a dependency and parity with it is not pinned by a test):
  * CMVN: from the [2, D+1] double stats, scale and offset vectors in double, rounded to float32;
    y = fl32(fl32(x * scale) + offset), the multiply only with --norm-vars (cmvn_norm).
  * deltas: scales[0] = [1]; scales[i] = scales[i-1] convolved with j = -window..window over sum j^2;
    block i of frame t = sum_j scales[i][j] * y[clamp(t + j, 0, T-1)] in float32, ascending j.
  * splice: row t = rows clamp(t-L) .. clamp(t+R) concatenated (edges replicated).
All three stages run in post_kernel (csrc/fdlp_post.hip) with no intermediate in HBM.

`transform-feats` (featbin/transform-feats.cc: LDA / MLLT `final.mat`, per-speaker fMLLR) is the optional fourth
stage, fused after the splice (xform_kernel, same file): with K the row width entering it and M [N, C] float32,
  * C == K: out = row M^T;  C == K + 1: out = row M[:, :K]^T + M[:, K] (the offset added last, one float32 add);
  * any other C: the utterance is warned about, counted as an error and not written;
  * every product is one float32 fmaf chain over k in an order fixed by K alone (Kaldi leaves it to its BLAS);
  * the average-logdet log line is not reproduced.
"""
import argparse
import ctypes
import os
import struct
import sys
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import FdlpPostBatchC, FdlpPostConfigC, FdlpXformConfigC, check, lib, ptr
from .cmvn import MatReader, _bool, read_kaldi_dmatrix


@dataclass
class PostConfig:
    """dim: input columns; the rest are the Kaldi options (a stage left at its zero is not executed)."""
    dim: int
    truncate: int = 0
    delta_order: int = 0
    delta_window: int = 2
    left_context: int = 0
    right_context: int = 0

    def to_c(self, device: int) -> FdlpPostConfigC:
        c = FdlpPostConfigC()
        c.dim, c.truncate = int(self.dim), int(self.truncate)
        c.delta_order, c.delta_window = int(self.delta_order), int(self.delta_window)
        c.left_context, c.right_context = int(self.left_context), int(self.right_context)
        c.device = int(device)
        return c


def cmvn_norm(stats, norm_means: bool = True, norm_vars: bool = False, reverse: bool = False,
              skip_dims: Sequence[int] = ()) -> np.ndarray:
    """float32 [2, D] (scale row, offset row) of ApplyCmvn / ApplyCmvnReverse for [2, D+1] double stats."""
    st = np.ascontiguousarray(stats, dtype=np.float64)
    if st.ndim != 2 or st.shape[0] != 2 or st.shape[1] < 2:
        raise ValueError("CMVN stats must be a [2, D+1] matrix, got %s" % (st.shape,))
    dim = st.shape[1] - 1
    skip = np.ascontiguousarray(np.asarray(list(skip_dims), dtype=np.int32))
    out = np.zeros((2, dim), dtype=np.float32)
    check(lib.fdlp_cmvn_norm(ptr(st, ctypes.c_double), dim, int(bool(norm_means)), int(bool(norm_vars)),
                             int(bool(reverse)), ptr(skip, ctypes.c_int32) if skip.size else None, int(skip.size),
                             ptr(out, ctypes.c_float)))
    return out


def _make_batch(who, dim, out_dim, feats, lengths, norm, norm_index, norm_vars, offsets, out):
    """The fdlp_post_batch of a compute call, the output tensor and the host arrays the batch points into."""
    if feats.dtype != torch.float32 or not feats.is_cuda or feats.dim() != 2 or feats.shape[1] != dim:
        raise ValueError("%s: need a float32 [rows, %d] device tensor" % (who, dim))
    feats = feats.contiguous()
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64))
    n = lens.size
    if offsets is None:
        offs = np.zeros(n, dtype=np.int64)
        if n:
            offs[1:] = np.cumsum(lens)[:-1]
    else:
        offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    rows = feats.shape[0]
    if out is None:
        out = torch.empty((rows, out_dim), dtype=torch.float32, device=feats.device)
    elif (out.dtype != torch.float32 or out.device != feats.device or not out.is_contiguous()
          or out.dim() != 2 or out.shape[1] != out_dim or out.shape[0] < rows):
        raise ValueError("%s: out must be a contiguous float32 [>= rows, %d] tensor" % (who, out_dim))
    b = FdlpPostBatchC()
    b.n_utt, b.n_rows = n, rows
    b.in_dev, b.out_dev = feats.data_ptr(), out.data_ptr()
    b.row_off, b.utt_len = ptr(offs, ctypes.c_int64), ptr(lens, ctypes.c_int64)
    idx = None
    if norm is not None:
        if norm.dtype != torch.float32 or norm.device != feats.device:
            raise ValueError("%s: norm must be a float32 tensor on the features' device" % who)
        if norm.dim() == 2:
            norm = norm.unsqueeze(0)
        if norm.dim() != 3 or norm.shape[1] != 2 or norm.shape[2] != dim:
            raise ValueError("%s: norm must be [2, %d] or [n, 2, %d]" % (who, dim, dim))
        norm = norm.contiguous()
        b.norm_dev, b.n_norm, b.norm_mul = norm.data_ptr(), norm.shape[0], int(bool(norm_vars))
        if norm_index is not None:
            idx = np.ascontiguousarray(np.asarray(norm_index, dtype=np.int32))
            if idx.size != n:
                raise ValueError("one norm index per utterance")
            b.norm_index = ptr(idx, ctypes.c_int32)
    return b, out, (feats, lens, offs, norm, idx)


class PostPlan:
    """cmvn | deltas | splice of a batch of concatenated utterances in one kernel launch.  device=-1 gives a
    host-only plan (out_dim, tile, lds_bytes, scales())."""

    def __init__(self, cfg: PostConfig, device: int = 0):
        self.cfg = cfg
        self.device = int(device)
        c = cfg.to_c(device)
        h = ctypes.c_void_p()
        check(lib.fdlp_post_plan_create(ctypes.byref(c), ctypes.byref(h)))
        self._h = h
        od, tl, lb = _lib.c_i32(), _lib.c_i32(), _lib.c_i32()
        check(lib.fdlp_post_plan_info(self._h, ctypes.byref(od), ctypes.byref(tl), ctypes.byref(lb)))
        self.out_dim, self.tile, self.lds_bytes = od.value, tl.value, lb.value

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            lib.fdlp_post_plan_destroy(h)
            self._h = None

    def __del__(self):
        self.close()

    def scales(self):
        """[scales[0], .., scales[order]] as float32 arrays (2 i window + 1 taps)."""
        lens = np.zeros(self.cfg.delta_order + 1, dtype=np.int32)
        check(lib.fdlp_post_plan_scales(self._h, ptr(lens, ctypes.c_int32), None))
        flat = np.zeros(int(lens.sum()), dtype=np.float32)
        check(lib.fdlp_post_plan_scales(self._h, None, ptr(flat, ctypes.c_float)))
        ends = np.cumsum(lens)
        return [flat[e - n:e].copy() for e, n in zip(ends, lens)]

    def compute(self, feats: torch.Tensor, lengths: Sequence[int], norm: Optional[torch.Tensor] = None,
                norm_index: Optional[Sequence[int]] = None, stream=None, norm_vars: bool = True,
                offsets: Optional[Sequence[int]] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """feats: float32 [rows, dim] device tensor holding the utterances one after another (or at `offsets`);
        norm: float32 device tensor [2, dim] or [n, 2, dim] from cmvn_norm, norm_index[u] the pair of utterance u;
        norm_vars=False skips the multiply (the scale row is all ones then).  Returns out [rows, out_dim]; row r
        of the output belongs to input row r."""
        b, out, keep = _make_batch("PostPlan.compute", self.cfg.dim, self.out_dim, feats, lengths, norm, norm_index,
                                   norm_vars, offsets, out)
        s = stream if stream is not None else torch.cuda.current_stream(feats.device)
        check(lib.fdlp_post_compute(self._h, ctypes.byref(b), ctypes.c_void_p(s.cuda_stream)))
        return out


class XformPlan:
    """cmvn | deltas | splice | transform-feats in one kernel launch: the stages of `cfg`, then every row times
    an [out_dim, K (+ 1 when affine)] float32 matrix, K = in_dim being the row width the stages produce.  With
    every stage of cfg off it is the stand-alone transform-feats.  device=-1 gives a host-only plan (in_dim,
    out_dim, mat_cols, tile, lds_bytes)."""

    def __init__(self, cfg: PostConfig, out_dim: int, affine: bool = False, device: int = 0):
        self.cfg = cfg
        self.device = int(device)
        c = FdlpXformConfigC()
        c.post = cfg.to_c(device)
        c.out_dim, c.affine = int(out_dim), int(bool(affine))
        h = ctypes.c_void_p()
        check(lib.fdlp_xform_plan_create(ctypes.byref(c), ctypes.byref(h)))
        self._h = h
        v = [_lib.c_i32() for _ in range(5)]
        check(lib.fdlp_xform_plan_info(self._h, *[ctypes.byref(x) for x in v]))
        self.in_dim, self.out_dim, self.mat_cols, self.tile, self.lds_bytes = [x.value for x in v]
        self.affine = bool(affine)

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            lib.fdlp_xform_plan_destroy(h)
            self._h = None

    def __del__(self):
        self.close()

    def dispatch(self) -> dict:
        """What compute() launches, read from the function the launcher selects by: xform_kernel<mode, ncb>
        (mode -1 no deltas, 0 general, 1 and 2 = that order at window 2), the column `groups` of 16 ncb, the `tile`,
        `vec` (16-byte LDS reads of the rows), K = 32 full_chunks + tail, and big_lds (more than 64 KB of dynamic
        LDS).  Works on a host-only plan."""
        info = (_lib.c_i32 * 8)()
        check(lib.fdlp_xform_plan_dispatch(self._h, info))
        keys = ("mode", "ncb", "groups", "tile", "vec", "full_chunks", "tail", "big_lds")
        d = dict(zip(keys, (int(v) for v in info)))
        d["vec"], d["big_lds"] = bool(d["vec"]), bool(d["big_lds"])
        return d

    def compute(self, feats: torch.Tensor, lengths: Sequence[int], mats: torch.Tensor,
                mat_index: Optional[Sequence[int]] = None, norm: Optional[torch.Tensor] = None,
                norm_index: Optional[Sequence[int]] = None, norm_vars: bool = True,
                offsets: Optional[Sequence[int]] = None, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """feats, lengths, norm, norm_index, norm_vars, offsets as for PostPlan.compute; mats: float32 device tensor
        [out_dim, mat_cols] or [n, out_dim, mat_cols], mat_index[u] the matrix of utterance u (None: matrix 0).
        Returns out [rows, out_dim]."""
        b, out, keep = _make_batch("XformPlan.compute", self.cfg.dim, self.out_dim, feats, lengths, norm, norm_index,
                                   norm_vars, offsets, out)
        if not isinstance(mats, torch.Tensor) or mats.dtype != torch.float32 or mats.device != feats.device:
            raise ValueError("XformPlan.compute: mats must be a float32 tensor on the features' device")
        if mats.dim() == 2:
            mats = mats.unsqueeze(0)
        if mats.dim() != 3 or mats.shape[0] < 1 or tuple(mats.shape[1:]) != (self.out_dim, self.mat_cols):
            raise ValueError("XformPlan.compute: mats must be [%d, %d] or [n, %d, %d], got %s"
                             % (self.out_dim, self.mat_cols, self.out_dim, self.mat_cols, tuple(mats.shape)))
        mats = mats.contiguous()
        midx = None
        if mat_index is not None:
            midx = np.ascontiguousarray(np.asarray(mat_index, dtype=np.int32))
            if midx.size != b.n_utt:
                raise ValueError("one matrix index per utterance")
        s = stream if stream is not None else torch.cuda.current_stream(feats.device)
        check(lib.fdlp_xform_compute(self._h, ctypes.byref(b), ctypes.c_void_p(mats.data_ptr()), mats.shape[0],
                                     ptr(midx, ctypes.c_int32) if midx is not None else None,
                                     ctypes.c_void_p(s.cuda_stream)))
        return out


# ---------------------------------------------------------------------------------------------
# tables of Kaldi double matrices (per-speaker CMVN stats): kept in float64, never through MatReader
# ---------------------------------------------------------------------------------------------
def _split_specifier(spec: str):
    """("ark" | "scp", set of the other options, rest) of an r/wspecifier; (None, set(), spec) for a filename."""
    kind, sep, rest = spec.partition(":")
    opts = kind.split(",")
    if not sep or not ({"ark", "scp"} & set(opts)) or not all(o.isalpha() for o in opts):
        return None, set(), spec
    return ("ark" if "ark" in opts else "scp"), set(opts), rest


def _read_dmatrix(f, where: str) -> np.ndarray:
    hdr = f.read(5)
    if hdr[:2] != b"\0B":
        raise ValueError("expected a binary Kaldi object at %s" % where)
    if hdr[2:5] not in (b"DM ", b"FM "):
        raise ValueError("not a float/double matrix at %s" % where)
    sizes = f.read(10)
    if len(sizes) != 10 or sizes[0] != 4 or sizes[5] != 4:
        raise ValueError("bad matrix dimensions at %s" % where)
    r, c = struct.unpack("<i", sizes[1:5])[0], struct.unpack("<i", sizes[6:10])[0]
    dt = "<f8" if hdr[2:5] == b"DM " else "<f4"
    raw = f.read(r * c * np.dtype(dt).itemsize)
    if r < 0 or c < 0 or len(raw) != r * c * np.dtype(dt).itemsize:
        raise ValueError("truncated matrix at %s" % where)
    return np.frombuffer(raw, dtype=dt).reshape(r, c).astype(np.float64)


def read_dmatrix_table(rspecifier: str):
    """Iterator over (key, float64 ndarray) of "ark:<file>" / "scp:<file>" (binary; Kaldi's s, cs, p options are
    accepted and ignored).  Double matrices keep their 64 bits."""
    kind, _, path = _split_specifier(rspecifier)
    if kind is None:
        raise ValueError("not a table rspecifier: %s" % rspecifier)
    if kind == "ark":
        f = sys.stdin.buffer if path == "-" else open(path, "rb")
        try:
            while True:
                key = b""
                ch = f.read(1)
                while ch and ch in b" \n\t\r":
                    ch = f.read(1)
                if not ch:
                    return
                while ch and ch != b" ":
                    key += ch
                    ch = f.read(1)
                if not ch:
                    raise ValueError("truncated ark after key %s" % key.decode())
                yield key.decode(), _read_dmatrix(f, "ark key " + key.decode())
        finally:
            if path != "-":
                f.close()
    else:
        cur, cur_path = None, None
        try:
            for line in open(path):
                t = line.split(None, 1)
                if len(t) < 2:
                    if t:
                        raise ValueError("bad scp line: %s" % line.rstrip())
                    continue
                key, rx = t[0], t[1].strip()
                fn, _, off = rx.rpartition(":")
                if fn and off.isdigit():
                    off = int(off)
                else:
                    fn, off = rx, 0
                if fn != cur_path:
                    if cur:
                        cur.close()
                    cur, cur_path = open(fn, "rb"), fn
                cur.seek(off)
                yield key, _read_dmatrix(cur, rx)
        finally:
            if cur:
                cur.close()


def read_kaldi_matrix(path: str) -> np.ndarray:
    """A Kaldi matrix *file* (final.mat, an fMLLR matrix) as float32: binary "FM ", binary "DM " (rounded to float32
    once) or the text form " [ ... ]" with one row per line."""
    raw = open(path, "rb").read()
    if raw[:2] == b"\0B":
        tok = raw[2:5]
        if tok not in (b"FM ", b"DM "):
            raise ValueError("%s: not a float or double matrix" % path)
        if len(raw) < 15 or raw[5] != 4 or raw[10] != 4:
            raise ValueError("%s: bad matrix dimensions" % path)
        r, c = struct.unpack("<i", raw[6:10])[0], struct.unpack("<i", raw[11:15])[0]
        dt = np.dtype("<f4" if tok == b"FM " else "<f8")
        if r < 0 or c < 0 or len(raw) < 15 + dt.itemsize * r * c:
            raise ValueError("%s: truncated matrix (%d x %d expected)" % (path, r, c))
        return np.frombuffer(raw[15:15 + dt.itemsize * r * c], dtype=dt).reshape(r, c).astype(np.float32)
    try:
        txt = raw.decode("ascii").strip()
    except UnicodeDecodeError:
        raise ValueError("%s: not a Kaldi matrix" % path)
    if not (txt.startswith("[") and txt.endswith("]")):
        raise ValueError("%s: not a Kaldi matrix, or a truncated one" % path)
    try:
        rows = [[float(v) for v in l.split()] for l in txt[1:-1].split("\n") if l.strip()]
    except ValueError:
        raise ValueError("%s: not a Kaldi matrix" % path)
    if len(set(len(r) for r in rows)) > 1:
        raise ValueError("%s: rows of different lengths" % path)
    return np.array(rows, dtype=np.float64).reshape(len(rows), -1).astype(np.float32)


def read_utt2spk(rspecifier: str) -> dict:
    _, _, path = _split_specifier(rspecifier)
    out = {}
    for line in open(path):
        t = line.split()
        if len(t) >= 2:
            out[t[0]] = t[1]
    return out


# ---------------------------------------------------------------------------------------------
# writers: ark:<file>, ark,scp:<ark>,<scp> through fdlp_ark_* (atomic); ark:- as Kaldi binary on stdout
# ---------------------------------------------------------------------------------------------
class FeatWriter:
    def __init__(self, wspecifier: str):
        kind, opts, rest = _split_specifier(wspecifier)
        if kind is None or "ark" not in opts:
            raise ValueError("unsupported wspecifier %s (ark:<file>, ark,scp:<ark>,<scp> or ark:-)" % wspecifier)
        if "t" in opts:
            raise ValueError("text-mode arks are not supported (%s)" % wspecifier)
        self._h, self._out = None, None
        if "scp" in opts:
            first, _, second = rest.partition(",")
            ark, scp = (first, second) if wspecifier.index("ark") < wspecifier.index("scp") else (second, first)
            if not ark or not scp or ark == "-":
                raise ValueError("ark,scp needs two file names (%s)" % wspecifier)
        else:
            ark, scp = rest, None
        if ark == "-":
            self._out = sys.stdout.buffer
        else:
            h = ctypes.c_void_p()
            check(lib.fdlp_ark_open(ark.encode(), scp.encode() if scp else None, ctypes.byref(h)))
            self._h = h

    def write(self, key: str, m: np.ndarray):
        m = np.ascontiguousarray(m, dtype=np.float32)
        if self._out is not None:
            self._out.write(key.encode() + b" \0BFM \x04" + struct.pack("<i", m.shape[0]) + b"\x04" +
                            struct.pack("<i", m.shape[1]))
            self._out.write(m.data)
        else:
            check(lib.fdlp_ark_write(self._h, key.encode(), ptr(m, ctypes.c_float), m.shape[0], m.shape[1]))

    def close(self):
        if self._out is not None:
            self._out.flush()
            self._out = None
        elif self._h:
            h, self._h = self._h, None
            check(lib.fdlp_ark_close(h))

    def abort(self):
        if self._h:
            h, self._h = self._h, None
            lib.fdlp_ark_abort(h)


# ---------------------------------------------------------------------------------------------
# runner: MatReader -> pinned double-buffered staging -> one PostPlan.compute per batch -> writer
# ---------------------------------------------------------------------------------------------
class _Slot:
    def __init__(self, rows, dim, out_dim, dev):
        self.h_in = torch.empty((rows, dim), dtype=torch.float32, pin_memory=True)
        self.d_in = torch.empty((rows, dim), dtype=torch.float32, device=dev)
        self.d_out = torch.empty((rows, out_dim), dtype=torch.float32, device=dev)
        self.h_out = torch.empty((rows, out_dim), dtype=torch.float32, pin_memory=True)
        self.rows = rows
        self.reset()

    def reset(self):
        """empty, for the next batch"""
        self.keys, self.lens, self.norm_idx, self.norms = [], [], [], []
        self.where = {}  # stats key -> row of this batch's norm table
        self.mat_idx, self.mats, self.mwhere = [], [], {}  # the same for the transform table
        self.fill = 0
        self.done = None


class SlotRunner:
    """The two-slot loop of every table-to-table tool: while the device works on one slot's batch, the host fills
    the other and writes out the batch before.  A subclass sets dim, slots (None until _setup or _admit has made
    them), num_done, num_err and log, and provides
      _setup(dim)       called with the width of the first non-empty matrix
      _admit(utt)       False skips the utterance (the hook has logged and counted it); anything else goes to _added
      _added(sl, extra) the utterance _admit returned `extra` for has been appended to slot sl
      _launch(sl)       copy in, compute, copy out, record sl.done
      _grow(cur, rows)  replace slots[cur] by one of `rows` rows for an utterance longer than a slot
      _host(v)          what is written for the device's rows v of a batch (the identity here)
      _reader(rspec)    the (key, matrix) pairs of the table (MatReader here)"""

    def _admit(self, utt):
        return None

    def _added(self, sl, extra):
        pass

    def _host(self, v):
        return v

    def _reader(self, rspecifier):
        """hook: the (key, matrix) pairs the loop consumes"""
        return MatReader(rspecifier)

    def _drain(self, sl):
        if sl.done is None:
            return
        sl.done.synchronize()
        host = self._host(sl.h_out.numpy()[:sl.fill])
        pos = 0
        for k, n in zip(sl.keys, sl.lens):
            self.writer.write(k, host[pos:pos + n])
            pos += n
            self.num_done += 1
        sl.reset()

    def run(self, rspecifier: str, writer: "FeatWriter"):
        self.writer = writer
        cur = 0
        for utt, m in self._reader(rspecifier):
            if self.dim is None and m.shape[0] > 0:
                self._setup(m.shape[1])
            if m.shape[0] == 0 or m.shape[1] != self.dim:
                self.log("Empty or mismatched feature matrix for utterance %s (%d x %d)" % (utt, m.shape[0], m.shape[1]))
                self.num_err += 1
                continue
            extra = self._admit(utt)
            if extra is False:
                continue
            sl = self.slots[cur]
            if sl.fill and sl.fill + m.shape[0] > sl.rows:
                self._launch(sl)
                cur ^= 1
                sl = self.slots[cur]
                self._drain(sl)           # the batch before the one just launched
            if m.shape[0] > sl.rows:      # one utterance longer than a batch: the slot grows to hold it
                self._grow(cur, m.shape[0])
                sl = self.slots[cur]
            sl.h_in[sl.fill:sl.fill + m.shape[0]].numpy()[...] = m
            sl.fill += m.shape[0]
            sl.keys.append(utt)
            sl.lens.append(m.shape[0])
            self._added(sl, extra)
        if self.slots:
            if self.slots[cur].fill:
                self._launch(self.slots[cur])
            self._drain(self.slots[cur ^ 1])
            self._drain(self.slots[cur])
        return self.num_done, self.num_err


class PostRunner(SlotRunner):
    """opts: the PostConfig fields but dim (taken from the first matrix); stats: None, a [2, D+1] matrix (global)
    or a dict key -> matrix with utt2spk (None: looked up by the utterance id).  transform: None, one [N, C] matrix
    (global) or a dict key -> matrix looked up like the stats (the same utt2spk); the plan is made from the first
    usable matrix (C = K or K + 1 for the K columns the other stages give), and a matrix of another shape later
    on is an error for its utterances."""

    def __init__(self, opts: dict, stats=None, utt2spk=None, norm_means=True, norm_vars=False, reverse=False,
                 skip_dims=(), device=0, batch_rows=16384, max_out_bytes=256 << 20, prog="post-feats", log=None,
                 transform=None):
        self.opts, self.stats, self.utt2spk = opts, stats, utt2spk
        self.transform = transform
        self._mat_cache = {}
        self.cmvn = dict(norm_means=norm_means, norm_vars=norm_vars, reverse=reverse, skip_dims=tuple(skip_dims))
        if norm_vars and not norm_means:
            raise ValueError("You cannot normalize the variance but not the mean.")
        self.apply_norm = stats is not None and norm_means
        self.device, self.batch_rows, self.max_out_bytes = device, batch_rows, max_out_bytes
        self.prog = prog
        self.log = log or (lambda m: print("WARNING (%s) %s" % (prog, m), file=sys.stderr))
        self.plan, self.slots, self.dim = None, None, None
        self._norm_cache = {}
        self.num_done = self.num_err = 0

    def _norm_for(self, utt):
        """(cache key, float32 [2, D]) or None when the utterance has no usable stats."""
        if isinstance(self.stats, dict):
            key = utt if self.utt2spk is None else self.utt2spk.get(utt)
            if key is None or key not in self.stats:
                return None
            st = self.stats[key]
        else:
            key, st = "", self.stats
        if key not in self._norm_cache:
            if st.shape != (2, self.dim + 1):
                self.log("Dimension mismatch: CMVN stats %s for features of dimension %d" % (st.shape, self.dim))
                self._norm_cache[key] = None
            else:
                self._norm_cache[key] = cmvn_norm(st, **self.cmvn)
        v = self._norm_cache[key]
        return None if v is None else (key, v)

    def _mat_for(self, utt):
        """(cache key, float32 [N, C]) or None (after the warning) when the utterance has no usable transform."""
        if isinstance(self.transform, dict):
            key = utt if self.utt2spk is None else self.utt2spk.get(utt)
            if key is None or key not in self.transform:
                self.log("No fMLLR transform available for utterance %s, producing no output for this utterance" % utt)
                return None
            m = self.transform[key]
        else:
            key, m = "", self.transform
        if key not in self._mat_cache:
            m = np.ascontiguousarray(m, dtype=np.float32)   # a double matrix is rounded once
            ok = m.ndim == 2 and m.shape[0] >= 1 and m.shape[1] in (self.in_dim, self.in_dim + 1)
            if ok and self.xshape is None:
                self.xshape = m.shape
            self._mat_cache[key] = m if ok and m.shape == self.xshape else m.shape
        m = self._mat_cache[key]
        if isinstance(m, tuple):
            want = "%d or %d" % (self.in_dim, self.in_dim + 1) if self.xshape is None else "%d x %d" % self.xshape
            self.log("Transform matrix for utterance %s has bad dimension %s versus feat dim %d (need %s)"
                     % (utt, " x ".join(str(v) for v in m), self.in_dim, want))
            return None
        return key, m

    def _setup(self, dim):
        self.dim = dim
        cfg = PostConfig(dim=dim, **self.opts)
        if self.transform is not None:       # the device plan waits for the first usable matrix
            self.in_dim, self.xshape = PostPlan(cfg, -1).out_dim, None
            return
        self._make_plan(PostPlan(cfg, self.device))

    def _make_plan(self, plan):
        dim = self.dim
        torch.cuda.set_device(self.device)
        self.plan = plan
        rows = max(1, min(self.batch_rows, self.max_out_bytes // (4 * self.plan.out_dim)))
        self.rows = rows
        self.slots = [_Slot(rows, dim, self.plan.out_dim, torch.device("cuda", self.device)) for _ in range(2)]

    def _launch(self, sl):
        n = sl.fill
        d_in = sl.d_in[:n]
        d_in.copy_(sl.h_in[:n], non_blocking=True)
        norm = idx = None
        if self.apply_norm:
            norm = torch.from_numpy(np.stack(sl.norms)).to(d_in.device)
            idx = sl.norm_idx
        if self.transform is not None:
            self.plan.compute(d_in, sl.lens, torch.from_numpy(np.stack(sl.mats)).to(d_in.device), sl.mat_idx,
                              norm=norm, norm_index=idx, out=sl.d_out, norm_vars=self.cmvn["norm_vars"])
        else:
            self.plan.compute(d_in, sl.lens, norm=norm, norm_index=idx, out=sl.d_out,
                              norm_vars=self.cmvn["norm_vars"])
        sl.h_out[:n].copy_(sl.d_out[:n], non_blocking=True)
        sl.done = torch.cuda.Event()
        sl.done.record()

    def _admit(self, utt):
        nv = mv = None
        if self.apply_norm:
            nv = self._norm_for(utt)
            if nv is None:
                self.log("No normalization statistics available for key %s, producing no output for this "
                         "utterance" % utt)
                self.num_err += 1
                return False
        if self.transform is not None:
            mv = self._mat_for(utt)
            if mv is None:
                self.num_err += 1
                return False
            if self.plan is None:
                N, C = mv[1].shape
                self._make_plan(XformPlan(PostConfig(dim=self.dim, **self.opts), N, C == self.in_dim + 1,
                                          self.device))
        return nv, mv

    def _added(self, sl, extra):
        nv, mv = extra
        if nv is not None:
            key, vec = nv
            if key not in sl.where:
                sl.where[key] = len(sl.norms)
                sl.norms.append(vec)
            sl.norm_idx.append(sl.where[key])
        if mv is not None:
            key, mat = mv
            if key not in sl.mwhere:
                sl.mwhere[key] = len(sl.mats)
                sl.mats.append(mat)
            sl.mat_idx.append(sl.mwhere[key])

    def _grow(self, cur, rows):
        sl = self.slots[cur]
        self._drain(sl)
        self.slots[cur] = _Slot(rows, self.dim, self.plan.out_dim, sl.d_in.device)


# ---------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------
def _skip_dims(v):
    return tuple(int(t) for t in v.split(":") if t != "")


def _add_common(ap):
    ap.add_argument("--device", type=int, default=int(os.environ.get("FDLP_DEVICE", "0")))
    ap.add_argument("--batch-rows", type=int, default=16384, help="rows per device batch")


def _add_cmvn_opts(ap):
    ap.add_argument("--norm-means", type=_bool, default=True, help="You can set this to false to turn off mean "
                    "normalization (default true)")
    ap.add_argument("--norm-vars", type=_bool, default=False, help="If true, normalize variances (default false)")
    ap.add_argument("--reverse", type=_bool, default=False, help="If true, apply CMVN in a reverse sense")
    ap.add_argument("--skip-dims", type=_skip_dims, default=(), help="Dimensions to skip normalization of "
                    "(colon-separated list of integers)")
    ap.add_argument("--utt2spk", default="", help="rspecifier for utterance to speaker map")


def _add_delta_opts(ap, order):
    ap.add_argument("--delta-order", type=int, default=order, help="Order of delta computation")
    ap.add_argument("--delta-window", type=int, default=2, help="Parameter controlling window for delta "
                    "computation (actual window size for each delta order is 1 + 2*delta-window-size)")
    ap.add_argument("--truncate", type=int, default=0, help="If nonzero, first truncate features to this dimension")


def _add_splice_opts(ap, ctx):
    ap.add_argument("--left-context", type=int, default=ctx, help="Number of frames of left context")
    ap.add_argument("--right-context", type=int, default=ctx, help="Number of frames of right context")


def apply_cmvn_parser():
    ap = argparse.ArgumentParser(
        prog="apply-cmvn", description="Apply cepstral mean and (optionally) variance normalization (on the MI355X). "
        "Usage: apply-cmvn [options] (<cmvn-stats-rspecifier>|<cmvn-stats-rxfilename>) <feats-rspecifier> "
        "<feats-wspecifier>")
    _add_cmvn_opts(ap)
    _add_common(ap)
    ap.add_argument("cmvn")
    ap.add_argument("feats")
    ap.add_argument("out")
    return ap


def add_deltas_parser():
    ap = argparse.ArgumentParser(prog="add-deltas", description="Add deltas (typically to raw mfcc or plp features) "
                                 "(on the MI355X). Usage: add-deltas [options] <in-rspecifier> <out-wspecifier>")
    _add_delta_opts(ap, 2)
    _add_common(ap)
    ap.add_argument("feats")
    ap.add_argument("out")
    return ap


def splice_feats_parser():
    ap = argparse.ArgumentParser(prog="splice-feats", description="Splice features with left and right context "
                                 "(on the MI355X). Usage: splice-feats [options] <feature-rspecifier> "
                                 "<feature-wspecifier>")
    _add_splice_opts(ap, 4)
    _add_common(ap)
    ap.add_argument("feats")
    ap.add_argument("out")
    return ap


def transform_feats_parser():
    ap = argparse.ArgumentParser(
        prog="transform-feats", description="Apply transform (e.g. LDA; HLDA; fMLLR/CMLLR; MLLT/STC) (on the MI355X). "
        "Linear transform if transform-num-cols == feature-dim, affine if transform-num-cols == feature-dim+1 "
        "(->append 1.0 to features). Per-utterance by default, or per-speaker if utt2spk option provided. "
        "Global if transform-rxfilename provided. Usage: transform-feats [options] "
        "(<transform-rspecifier>|<transform-rxfilename>) <feats-rspecifier> <feats-wspecifier>")
    ap.add_argument("--utt2spk", default="", help="rspecifier for utterance to speaker map")
    _add_common(ap)
    ap.add_argument("transform")
    ap.add_argument("feats")
    ap.add_argument("out")
    return ap


def post_feats_parser():
    """apply-cmvn | add-deltas | splice-feats | transform-feats in one launch per batch; every stage is off by
    default."""
    ap = argparse.ArgumentParser(prog="post-feats", description="apply-cmvn | add-deltas | splice-feats | "
                                 "transform-feats fused into one kernel launch per batch (on the MI355X). Usage: "
                                 "post-feats [options] <feats-rspecifier> <feats-wspecifier>")
    ap.add_argument("--cmvn", default="", help="CMVN stats: a table rspecifier or the file of one global matrix")
    ap.add_argument("--transform", default="", help="transform-feats as the last stage: the file of one global "
                    "matrix (final.mat) or a table rspecifier (per utterance, per speaker with --utt2spk)")
    _add_cmvn_opts(ap)
    _add_delta_opts(ap, 0)
    _add_splice_opts(ap, 0)
    _add_common(ap)
    ap.add_argument("feats")
    ap.add_argument("out")
    return ap


def _load_stats(arg: str):
    kind, _, _ = _split_specifier(arg)
    if kind is None:
        return read_kaldi_dmatrix(arg)
    return dict(read_dmatrix_table(arg))


def _load_transform(arg: str):
    kind, _, _ = _split_specifier(arg)
    if kind is None:
        return read_kaldi_matrix(arg)
    return dict(read_dmatrix_table(arg))


def _run(prog, a, opts, cmvn_arg=None, transform_arg=None):
    stats = utt2spk = None
    kw = {}
    if transform_arg:
        kw["transform"] = _load_transform(transform_arg)
        if a.utt2spk:
            utt2spk = read_utt2spk(a.utt2spk)
    if cmvn_arg:
        kw.update(norm_means=a.norm_means, norm_vars=a.norm_vars, reverse=a.reverse, skip_dims=a.skip_dims)
        if a.norm_vars and not a.norm_means:
            print("ERROR (%s) You cannot normalize the variance but not the mean." % prog, file=sys.stderr)
            return 1
        stats = _load_stats(cmvn_arg)
        if a.utt2spk:
            utt2spk = read_utt2spk(a.utt2spk)
    runner = PostRunner(opts, stats=stats, utt2spk=utt2spk, device=a.device, batch_rows=a.batch_rows, prog=prog, **kw)
    writer = FeatWriter(a.out)
    try:
        done, err = runner.run(a.feats, writer)
    except BaseException:
        writer.abort()
        raise
    writer.close()
    what = {"apply-cmvn": "Applied cepstral mean %snormalization" % ("and variance " if kw.get("norm_vars") else ""),
            "add-deltas": "Added deltas", "splice-feats": "Spliced features",
            "post-feats": "Applied the feature post-processing chain", "transform-feats": "Applied transform"}[prog]
    if prog == "transform-feats":
        print("LOG (%s) Applied transform to %d utterances; %d had errors." % (prog, done, err), file=sys.stderr)
    else:
        print("LOG (%s) %s to %d utterances, errors on %d" % (prog, what, done, err), file=sys.stderr)
    return 0 if done else 1


def main_apply_cmvn(argv=None):
    a = apply_cmvn_parser().parse_args(argv)
    return _run("apply-cmvn", a, {}, a.cmvn)


def main_add_deltas(argv=None):
    a = add_deltas_parser().parse_args(argv)
    return _run("add-deltas", a, dict(truncate=a.truncate, delta_order=a.delta_order, delta_window=a.delta_window))


def main_splice_feats(argv=None):
    a = splice_feats_parser().parse_args(argv)
    return _run("splice-feats", a, dict(left_context=a.left_context, right_context=a.right_context))


def main_post_feats(argv=None):
    a = post_feats_parser().parse_args(argv)
    opts = dict(truncate=a.truncate, delta_order=a.delta_order, delta_window=a.delta_window,
                left_context=a.left_context, right_context=a.right_context)
    return _run("post-feats", a, opts, a.cmvn or None, a.transform or None)


def main_transform_feats(argv=None):
    a = transform_feats_parser().parse_args(argv)
    return _run("transform-feats", a, {}, None, a.transform)


MAINS = {"apply-cmvn": main_apply_cmvn, "add-deltas": main_add_deltas, "splice-feats": main_splice_feats,
         "post-feats": main_post_feats, "transform-feats": main_transform_feats}

if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in MAINS:
        sys.exit("usage: python -m speech_recognition_tools_amd.post (%s) [options] ..." % " | ".join(MAINS))
    sys.exit(MAINS[sys.argv[1]](sys.argv[2:]))
