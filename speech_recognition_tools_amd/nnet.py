"""The feed-forward acoustic model of the hybrid recipes on the MI355X: a drop-in for the reference's
src/nnet/extract_posterior.py (recipes/timit/run_hybrid_mvector.sh), which pushes `apply-cmvn | splice-feats` rows
through nnetFeedforward (src/nnet/nnet_models.py:9-31: nn.Linear layers with ReLU between them) one utterance at a
time on the CPU.

  * Layer 0 runs inside the chain's kernel launch (xform_kernel, csrc/fdlp_post.hip) as the affine transform
    [W_0 | b_0]: the spliced rows never reach HBM.  Every further layer is one dense_kernel launch
    (csrc/fdlp_nnet.hip) on the exact-float32 MFMA; it applies the ReLU as it loads its input, so each layer stores
    its pre-activation, which is what the reference taps (`embeds.append(inputs)` before the ReLU).
  * Every result is one float32 fmaf chain in an order fixed by the layer's input width alone (include/fdlp.h), so
    a row's bits do not depend on the batch it is computed in.  torch leaves the order to its BLAS; parity with the
    reference is therefore to rounding, not bitwise.
  * `--add_softmax`: p_j = exp(x_j - m) / sum_i exp(x_i - m) with m = max_i x_i.  The reference's
    `np.exp(X) / sum` (extract_posterior.py:13-14) has no max subtraction and overflows to NaN once a logit
    exceeds 88; that is NOT reproduced: the result here is finite for every finite row.
  * `--prior` / `--prior_weight` (an addition, off by default; extract_posterior.py has no such option):
    log_softmax(x) - prior_weight * prior, the pseudo log-likelihoods of dump_genclassifier_outputs.py:110 that
    latgen-faster-mapped consumes.
  * egs.config (data_prep_feedforward.py:132-135): `cmvn,<stats>` is a global apply-cmvn with Kaldi's defaults
    (means only), `pca,<mat>` a transform-feats BEFORE the splice (the reference's order), None raw features (the
    reference raises a NameError there, extract_posterior.py:42-51; the data-prep script plainly means raw).
  * The ark values are rounded like dict2Ark's '%.3f' text ark read back by copy-feats, by the rule include/fdlp.h
    documents for ark_decimals: k = nearbyint(v * 10^d), stored as (float)(k / 10^d).
Out of scope: training.  The GRU models of src/nnet (dump_genclassifier_outputs.py) are in rnn.py, on what this
module shares with it: StagePlan (the library has one stage plan; a feed-forward net is its linear-only case),
NnetRunner on post.py's two-slot loop, the checkpoint and egs.config readers, and run_model_tool, the body of both
command lines.
"""
import argparse
import ctypes
import os
import pickle
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import FdlpNnetConfigC, check, lib
from .cmvn import read_kaldi_dmatrix
from .post import (FeatWriter, PostConfig, SlotRunner, XformPlan, _make_batch, _Slot, _split_specifier, cmvn_norm,
                   read_dmatrix_table, read_kaldi_matrix)

MODES = {"raw": _lib.FDLP_NNET_RAW, "softmax": _lib.FDLP_NNET_SOFTMAX, "loglike": _lib.FDLP_NNET_LOGLIKE}


class StagePlan:
    """What NnetPlan and RnnPlan (rnn.py) share: one stage plan of the library under two names.  A constructor sets
    cfg, _h, dims and out_dim; the class names the C functions behind the handle and the words of its messages."""
    _DESTROY = _COMPUTE = None
    _WORDS = ("model", "stage")

    def close(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:   # lib is gone when the interpreter shuts down
            getattr(lib, self._DESTROY)(h)
            self._h = None

    def __del__(self):
        self.close()

    def tap_dim(self, tap: int) -> int:
        """columns of the output for `tap` (0: the last stage; s: stage n - 1 - s of n; for a network, tap l is the
        reference's embeds[-l])"""
        n, (model, stage) = len(self.dims) - 1, self._WORDS
        if not 0 <= tap < n:
            raise ValueError("tap %d is outside 0 .. %d (the %s has %d %ss)" % (tap, n - 1, model, n, stage))
        return self.dims[n - tap]

    def compute(self, feats: torch.Tensor, lengths: Sequence[int], norm: Optional[torch.Tensor] = None,
                norm_index: Optional[Sequence[int]] = None, norm_vars: bool = True, tap: int = 0, mode: str = "raw",
                prior: Optional[torch.Tensor] = None, prior_weight: float = 0.8,
                offsets: Optional[Sequence[int]] = None, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """feats, lengths, norm, norm_index, norm_vars, offsets, out as for PostPlan.compute.  tap 0: the last stage's
        output, in `mode` raw, softmax or loglike (the last with prior, a float32 device tensor [out_dim]); tap s > 0:
        the output of stage n - 1 - s, raw (of a linear_relu stage or a hidden layer, the pre-activation).  Returns
        out [rows, tap_dim(tap)]."""
        who = type(self).__name__ + ".compute"
        if mode not in MODES:
            raise ValueError("mode must be one of %s" % ", ".join(MODES))
        b, out, keep = _make_batch(who, self.cfg.dim, self.tap_dim(tap), feats, lengths, norm, norm_index, norm_vars,
                                   offsets, out)
        pp = None
        if mode == "loglike":
            if (not isinstance(prior, torch.Tensor) or prior.dtype != torch.float32 or prior.device != feats.device
                    or tuple(prior.shape) != (self.out_dim,)):
                raise ValueError("%s: loglike needs prior, a float32 [%d] tensor on the features' device"
                                 % (who, self.out_dim))
            prior = prior.contiguous()
            pp = ctypes.c_void_p(prior.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(feats.device)
        check(getattr(lib, self._COMPUTE)(self._h, ctypes.byref(b), int(tap), MODES[mode], pp, float(prior_weight),
                                          ctypes.c_void_p(s.cuda_stream)))
        return out


class NnetPlan(StagePlan):
    """cmvn | deltas | splice | feed-forward network: the stage plan with the stages linear_relu x (n_linear - 1),
    linear.  weights[l]: float32 [dims[l+1], dims[l]] (nn.Linear's layout),
    biases[l]: [dims[l+1]], dims[0] being the row width the stages of cfg give.  device=-1 gives a host-only plan
    (dims, workspace_bytes, tile, lds_bytes); it needs the shapes only, so the arrays may be None there and `dims`
    is given instead."""
    _DESTROY, _COMPUTE = "fdlp_nnet_plan_destroy", "fdlp_nnet_compute"
    _WORDS = ("network", "layer")

    def __init__(self, cfg: PostConfig, weights, biases, max_rows: int = 16384, device: int = 0,
                 dims: Optional[Sequence[int]] = None):
        self.cfg, self.device, self.max_rows = cfg, int(device), int(max_rows)
        if dims is None:
            if not weights or len(weights) != len(biases):
                raise ValueError("NnetPlan: one weight matrix and one bias vector per layer")
            ws = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
            bs = [np.ascontiguousarray(b, dtype=np.float32) for b in biases]
            for l, (w, b) in enumerate(zip(ws, bs)):
                if w.ndim != 2 or b.ndim != 1 or b.shape[0] != w.shape[0] or (l and w.shape[1] != ws[l - 1].shape[0]):
                    raise ValueError("NnetPlan: layer %d has weight %s and bias %s after a layer of %s outputs"
                                     % (l, w.shape, b.shape, ws[l - 1].shape[0] if l else "-"))
            dims = [ws[0].shape[1]] + [w.shape[0] for w in ws]
        else:
            ws = bs = None
            dims = [int(d) for d in dims]
        n_linear = len(dims) - 1
        c = FdlpNnetConfigC()
        c.post = cfg.to_c(device)
        c.n_linear = n_linear
        for i, d in enumerate(dims[:_lib.FDLP_NNET_MAX_LINEAR + 1]):
            c.dims[i] = d
        wp = bp = None
        if ws is not None:
            n = len(ws)
            wp = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws])
            bp = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
        h = ctypes.c_void_p()
        check(lib.fdlp_nnet_plan_create(ctypes.byref(c), wp, bp, self.max_rows, ctypes.byref(h)))
        self._h = h
        ind, nl, lds = _lib.c_i32(), _lib.c_i32(), _lib.c_i32()
        wsb = _lib.c_i64()
        tile = (_lib.c_i32 * 3)()
        od = (_lib.c_i32 * _lib.FDLP_NNET_MAX_LINEAR)()
        check(lib.fdlp_nnet_plan_info(self._h, ctypes.byref(ind), ctypes.byref(nl), od, ctypes.byref(wsb), tile,
                                      ctypes.byref(lds)))
        self.in_dim, self.n_linear = ind.value, nl.value
        self.dims = [ind.value] + [od[i] for i in range(nl.value)]
        self.out_dim = self.dims[-1]
        self.workspace_bytes, self.tile, self.lds_bytes = wsb.value, tuple(tile), lds.value


# ---------------------------------------------------------------------------------------------
# the reference's files: the checkpoint dict of train_feedforward*.py and egs.config
# ---------------------------------------------------------------------------------------------
@dataclass
class FeedforwardCheckpoint:
    feature_dim: int
    num_frames: int
    num_layers: int     # hidden layers: num_layers + 1 nn.Linear in all
    hidden_dim: int
    num_classes: int
    weights: List[np.ndarray]
    biases: List[np.ndarray]

    @property
    def dims(self):
        return [self.feature_dim * self.num_frames] + [self.hidden_dim] * self.num_layers + [self.num_classes]


HEADER_KEYS = ("feature_dim", "num_frames", "num_layers", "hidden_dim", "num_classes")


def open_checkpoint(path: str, keys: Sequence[str], zero_ok: Sequence[str] = (), hint: str = "", whole: bool = False):
    """(header, model_state_dict) of a dict the reference's trainers save: header[k] = int(d[k]) for k in keys, each
    >= 1, or >= 0 for those of zero_ok.  A missing file is an OSError that names it; everything else a ValueError
    that names the path and the key (`hint` is appended where a key is missing).  whole: the dict itself as a third
    value, for a caller whose header holds more than integers."""
    with open(path, "rb"):   # a missing or unreadable file is an OSError that names it
        pass
    try:
        d = torch.load(path, map_location="cpu")
    except Exception as e:  # an unpickling error of any kind; a truncated archive surfaces as an OSError without a name
        raise ValueError("%s: not a torch checkpoint (%s)" % (path, e))
    if not isinstance(d, dict):
        raise ValueError("%s: the checkpoint is a %s, not a dict" % (path, type(d).__name__))
    for k in tuple(keys) + ("model_state_dict",):
        if k not in d:
            raise ValueError("%s: the checkpoint has no key '%s'%s" % (path, k, hint))
    hdr = {}
    for k in keys:
        try:
            hdr[k] = int(d[k])
        except (TypeError, ValueError):
            raise ValueError("%s: key '%s' is not an integer (%r)" % (path, k, d[k]))
        if hdr[k] < (0 if k in zero_ok else 1):
            raise ValueError("%s: key '%s' is %d" % (path, k, hdr[k]))
    sd = d["model_state_dict"]
    if not hasattr(sd, "keys"):
        raise ValueError("%s: key 'model_state_dict' is a %s, not a dict" % (path, type(sd).__name__))
    return (hdr, sd, d) if whole else (hdr, sd)


def state_array(path, sd, name, want, hdr, conv1d=False):
    """float32 sd[name], of shape `want`; conv1d also takes a Conv1d weight of kernel size 1, [out, in, 1]"""
    if name not in sd:
        raise ValueError("%s: model_state_dict has no key '%s'" % (path, name))
    t = sd[name]
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if conv1d and a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if tuple(a.shape) != want:
        raise ValueError("%s: '%s' has shape %s where the header (%s) needs %s"
                         % (path, name, tuple(a.shape), ", ".join("%s %d" % kv for kv in hdr.items()), want))
    return np.ascontiguousarray(a, dtype=np.float32)


def load_feedforward_checkpoint(path: str) -> FeedforwardCheckpoint:
    """torch.load of the dict the reference's trainers save: feature_dim, num_frames, num_layers, hidden_dim,
    num_classes and model_state_dict with layers.{i}.weight / layers.{i}.bias, i = 0 .. num_layers.  Every shape is
    checked against the header; the errors name the key."""
    hdr, sd = open_checkpoint(path, HEADER_KEYS, zero_ok=("num_layers",))
    ins = [hdr["feature_dim"] * hdr["num_frames"]] + [hdr["hidden_dim"]] * hdr["num_layers"]
    outs = [hdr["hidden_dim"]] * hdr["num_layers"] + [hdr["num_classes"]]
    ws = [state_array(path, sd, "layers.%d.weight" % i, (n, k), hdr) for i, (k, n) in enumerate(zip(ins, outs))]
    bs = [state_array(path, sd, "layers.%d.bias" % i, (n,), hdr) for i, n in enumerate(outs)]
    extra = [k for k in sd.keys() if k.startswith("layers.") and k.split(".")[1].isdigit()
             and int(k.split(".")[1]) > hdr["num_layers"]]
    if extra:
        raise ValueError("%s: model_state_dict has '%s' beyond the num_layers = %d of the header"
                         % (path, extra[0], hdr["num_layers"]))
    return FeedforwardCheckpoint(weights=ws, biases=bs, **hdr)


@dataclass
class EgsConfig:
    feat_type: Optional[str]    # None (raw), "cmvn" or "pca"; "cmvn_utt" too from load_rnn_egs_config
    feat_path: Optional[str]    # the stats file / the transform matrix
    left: int
    right: int


def read_egs_config(path: str, need=("feat_type", "concat_feats")):
    """(d, left, right): the pickled dict of egs.config, holding the keys of `need`, and its concat_feats 'L,R'"""
    try:
        with open(path, "rb") as f:
            d = pickle.load(f)
    except (OSError, IOError):
        raise
    except Exception as e:
        raise ValueError("%s: not a pickled egs.config (%s)" % (path, e))
    if not isinstance(d, dict):
        raise ValueError("%s: egs.config is a %s, not a dict" % (path, type(d).__name__))
    for k in need:
        if k not in d:
            raise ValueError("%s: egs.config has no key '%s'" % (path, k))
    left = right = 0
    if d["concat_feats"]:
        try:
            t = d["concat_feats"].split(",")
            left, right = int(t[0]), int(t[1])
            if len(t) != 2 or left < 0 or right < 0:
                raise ValueError
        except (AttributeError, IndexError, ValueError):
            raise ValueError("%s: 'concat_feats' must be '<left>,<right>' or None, got %r" % (path, d["concat_feats"]))
    return d, left, right


def load_egs_config(path: str) -> EgsConfig:
    """The pickled dict {'feat_type': 'cmvn,<path>' | 'pca,<path>' | None, 'concat_feats': 'L,R' | None} that
    data_prep_feedforward.py:132-135 writes.  Any other feat_type is refused."""
    d, left, right = read_egs_config(path)
    ft, fp = None, None
    if d["feat_type"]:
        if not isinstance(d["feat_type"], str) or d["feat_type"].count(",") < 1:
            raise ValueError("%s: 'feat_type' must be '<cmvn|pca>,<path>' or None, got %r" % (path, d["feat_type"]))
        ft, fp = d["feat_type"].split(",", 1)
        if ft not in ("cmvn", "pca") or not fp:
            raise ValueError("%s: 'feat_type' must be '<cmvn|pca>,<path>' or None, got %r" % (path, d["feat_type"]))
    return EgsConfig(ft, fp, left, right)


def round_ark(v: np.ndarray, decimals: int) -> np.ndarray:
    """float32 ark values of `v` for ark_decimals = decimals (include/fdlp.h): k = nearbyint(v 10^d), (float)(k / 10^d);
    decimals < 0 keeps the float32 values."""
    v = np.asarray(v, dtype=np.float32)
    if decimals < 0:
        return v
    s = 10.0 ** decimals
    return (np.rint(v.astype(np.float64) * s) / s).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# runner: MatReader -> pinned double-buffered staging -> one NnetPlan.compute per batch -> writer
# ---------------------------------------------------------------------------------------------
class NnetRunner(SlotRunner):
    """post.py's two slots around a model plan.  `pca,<mat>` runs a stand-alone XformPlan first (the reference
    transforms before it splices), then the model plan with the splice only.  A tool differs (RnnRunner, rnn.py) in
    the class attributes, in _new_plan and in the hooks _admit, _added and _norm_args."""
    NORM_VARS = False                   # the apply-cmvn --norm-vars the tool's command line implies
    FEAT_TYPES = ("cmvn", "pca")        # egs.feat_type values that are not raw features
    BATCH_ROWS, PROG = 16384, "extract-posterior"

    def __init__(self, ckpt, egs: EgsConfig, layer: int = 0, mode: str = "raw", prior=None, prior_weight: float = 0.8,
                 device: int = 0, batch_rows: Optional[int] = None, decimals: int = 3, prog: Optional[str] = None,
                 log=None):
        prog = prog or self.PROG
        self.ckpt, self.egs, self.layer, self.mode = ckpt, egs, int(layer), mode
        self.device, self.decimals = int(device), int(decimals)
        self.batch_rows = max(1, int(self.BATCH_ROWS if batch_rows is None else batch_rows))
        self.prior_weight = float(prior_weight)
        self.log = log or (lambda m: print("WARNING (%s) %s" % (prog, m), file=sys.stderr))
        if egs.left + egs.right + 1 != ckpt.num_frames:
            raise ValueError("the model was trained on %d spliced frames but egs.config splices -%d..+%d"
                             % (ckpt.num_frames, egs.left, egs.right))
        if not 0 <= self.layer <= ckpt.num_layers:
            raise ValueError("--layer %d: the model has %d hidden layers" % (self.layer, ckpt.num_layers))
        self.norm_host = self.pca_host = self.utt_stats = None
        feat_type = egs.feat_type if egs.feat_type in self.FEAT_TYPES else None
        if feat_type == "cmvn":
            st = read_kaldi_dmatrix(egs.feat_path)
            if st.shape != (2, ckpt.feature_dim + 1):
                raise ValueError("%s: CMVN stats of shape %s for a model of feature dimension %d (need 2 x %d)"
                                 % (egs.feat_path, " x ".join(str(v) for v in st.shape), ckpt.feature_dim,
                                    ckpt.feature_dim + 1))
            self.norm_host = cmvn_norm(st, norm_means=True, norm_vars=self.NORM_VARS)
        elif feat_type == "cmvn_utt":
            self.utt_stats = dict(read_dmatrix_table("scp:" + egs.feat_path))
        elif feat_type == "pca":
            m = read_kaldi_matrix(egs.feat_path)
            if m.shape[0] != ckpt.feature_dim:
                raise ValueError("%s: a transform to %d columns for a model of feature dimension %d"
                                 % (egs.feat_path, m.shape[0], ckpt.feature_dim))
            self.pca_host = m
        self.prior_host = None
        if mode == "loglike":
            p = np.ascontiguousarray(prior, dtype=np.float32).reshape(-1)
            if p.shape[0] != ckpt.num_classes:
                raise ValueError("the prior has %d entries for %d classes" % (p.shape[0], ckpt.num_classes))
            self.prior_host = p
        self.dim, self.plan, self.pre, self.slots = None, None, None, None
        self.num_done = self.num_err = 0

    def _new_plan(self, cfg, rows):
        return NnetPlan(cfg, self.ckpt.weights, self.ckpt.biases, max_rows=rows, device=self.device)

    def _make_plan(self, rows):
        cfg = PostConfig(dim=self.ckpt.feature_dim, left_context=self.egs.left, right_context=self.egs.right)
        if self.plan is not None:
            self.plan.close()
        self.plan = self._new_plan(cfg, rows)

    def _setup(self, dim):
        self._setup_front(dim)
        self._make_plan(self.batch_rows)
        self.out_dim = self.plan.tap_dim(self.layer)
        self.slots = [self._slot(self.batch_rows) for _ in range(2)]

    def _setup_front(self, dim):
        """what lies before the model plan, for features of width dim: the transform, the norm and the prior"""
        self.dim = dim
        torch.cuda.set_device(self.device)
        dev = torch.device("cuda", self.device)
        if self.pca_host is not None:
            if self.pca_host.shape[1] not in (dim, dim + 1):
                raise ValueError("%s: transform of %d x %d for features of dimension %d"
                                 % (self.egs.feat_path, self.pca_host.shape[0], self.pca_host.shape[1], dim))
            self.pre = XformPlan(PostConfig(dim=dim), self.pca_host.shape[0], self.pca_host.shape[1] == dim + 1,
                                 self.device)
            self.pca = torch.from_numpy(self.pca_host).to(dev)
        elif dim != self.ckpt.feature_dim:
            raise ValueError("features of dimension %d for a model of feature dimension %d" % (dim, self.ckpt.feature_dim))
        self.norm = torch.from_numpy(self.norm_host).to(dev) if self.norm_host is not None else None
        self.prior = torch.from_numpy(self.prior_host).to(dev) if self.prior_host is not None else None

    def _slot(self, rows):
        sl = _Slot(rows, self.dim, self.out_dim, torch.device("cuda", self.device))
        sl.d_mid = (torch.empty((rows, self.ckpt.feature_dim), dtype=torch.float32, device=sl.d_in.device)
                    if self.pre is not None else None)
        return sl

    def _norm_args(self, sl):
        """hook: (norm, norm_index) of slot sl's batch"""
        return self.norm, None

    def _launch(self, sl):
        n = sl.fill
        d_in = sl.d_in[:n]
        d_in.copy_(sl.h_in[:n], non_blocking=True)
        if self.pre is not None:
            d_in = self.pre.compute(d_in, sl.lens, self.pca, out=sl.d_mid)[:n]
        norm, idx = self._norm_args(sl)
        self.plan.compute(d_in, sl.lens, norm=norm, norm_index=idx, norm_vars=self.NORM_VARS, tap=self.layer,
                          mode=self.mode, prior=self.prior, prior_weight=self.prior_weight, out=sl.d_out)
        sl.h_out[:n].copy_(sl.d_out[:n], non_blocking=True)
        sl.done = torch.cuda.Event()
        sl.done.record()

    def _host(self, v):
        return round_ark(v, self.decimals)

    def _grow(self, cur, rows):
        self._drain(self.slots[cur])
        self._drain(self.slots[cur ^ 1])   # the old plan's workspaces are still being read
        self._make_plan(rows)
        self.slots[cur] = self._slot(rows)


# ---------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------
def extract_posterior_parser():
    ap = argparse.ArgumentParser(prog="extract-posterior",
                                 description="Extract Posterior from a Feedforward nnet Model (on the MI355X)")
    ap.add_argument("model", help="Feedforward pytorch nnet model")
    ap.add_argument("scp", help="scp files for features (or an ark: / scp: rspecifier)")
    ap.add_argument("egs_config", help="config file for generating examples")
    ap.add_argument("save_file", help="file to save posteriors: <save_file>.ark and .scp (or an ark wspecifier)")
    ap.add_argument("--layer", type=int, default=0, help="layer from the end to get the posteriors from")
    ap.add_argument("--add_softmax", action="store_true", help="Add softmax to layer zero posteriors")
    ap.add_argument("--prior", default=None, help="pickle of a float array [num_classes]: write log_softmax - "
                    "prior_weight * prior instead of the logits (layer 0 only)")
    ap.add_argument("--prior_weight", type=float, default=0.8, help="weight of the prior (default 0.8)")
    ap.add_argument("--ark_precision", type=int, default=3, help="decimals of the written values, like the "
                    "reference's '%%.3f' text ark; negative keeps float32")
    ap.add_argument("--device", type=int, default=int(os.environ.get("FDLP_DEVICE", "0")))
    ap.add_argument("--batch-rows", type=int, default=16384, help="rows per device batch")
    return ap


def _load_prior(path):
    try:
        with open(path, "rb") as f:
            p = pickle.load(f)
        return np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1), dtype=np.float32)
    except (OSError, IOError):
        raise
    except Exception as e:
        raise ValueError("%s: not a pickled prior vector (%s)" % (path, e))


def _rspecifier(scp):
    return scp if _split_specifier(scp)[0] else "scp:" + scp


def run_model_tool(prog, a, make_runner, did, scps=None):
    """What the model tools do with their parsed arguments `a` (scp, save_file): make_runner() loads the files and
    returns the runner; `did` opens the final LOG line.  scps: the tables of a tool that reads several in step
    (dump-multimod-outputs), whose runner takes the list.  Returns the exit status."""
    writer = None
    try:
        runner = make_runner()
        rspec = _rspecifier(a.scp) if scps is None else [_rspecifier(s) for s in scps]
        if _split_specifier(a.save_file)[0]:
            wspec = a.save_file
        else:
            base = os.path.abspath(a.save_file)
            wspec = "ark,scp:%s.ark,%s.scp" % (base, base)
        writer = FeatWriter(wspec)
        done, err = runner.run(rspec, writer)
    except (OSError, ValueError, _lib.FdlpError) as e:
        if writer is not None:
            writer.abort()
        print("ERROR (%s) %s" % (prog, e), file=sys.stderr)
        return 1
    except BaseException:
        if writer is not None:
            writer.abort()
        raise
    writer.close()
    print("LOG (%s) %s for %d utterances, errors on %d" % (prog, did, done, err), file=sys.stderr)
    return 0 if done else 1


def main_extract_posterior(argv=None):
    prog = "extract-posterior"
    a = extract_posterior_parser().parse_args(argv)

    def make_runner():
        ckpt = load_feedforward_checkpoint(a.model)
        egs = load_egs_config(a.egs_config)
        mode, prior = "raw", None
        if a.layer == 0:           # as in the reference, the options of layer 0 are ignored for a hidden layer
            if a.prior:
                mode, prior = "loglike", _load_prior(a.prior)
            elif a.add_softmax:
                mode = "softmax"
        return NnetRunner(ckpt, egs, layer=a.layer, mode=mode, prior=prior, prior_weight=a.prior_weight,
                          device=a.device, batch_rows=a.batch_rows, decimals=a.ark_precision, prog=prog)

    return run_model_tool(prog, a, make_runner, "Extracted posteriors")


if __name__ == "__main__":
    sys.exit(main_extract_posterior(sys.argv[1:]))
