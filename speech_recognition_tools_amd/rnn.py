"""The GRU acoustic models of the hybrid recipes on the MI355X: a drop-in for the reference's
src/nnet/dump_genclassifier_outputs.py (recipes/timit/local_pyspeech/decode_dnn.sh), which pushes the
`apply-cmvn --norm-vars=true | splice-feats` rows of one utterance at a time through torch on the CPU and writes the
pseudo log-likelihoods latgen-faster-mapped consumes.

  * --ae_type=noae is nnetRNN (nnet_models.py:54-89): GRU layers, then a regression layer (a Conv1d of kernel size
    1).  --ae_type=normal, the recipe's default, is the classifier branch of nnetAEClassifierMultitask
    (nnet_models.py:164-240): encoder GRUs, a bottleneck with ReLU, classifier GRUs, the regression layer; the `ae`
    branch does not feed the output and its keys are ignored.  Dropout is the identity in eval().
  * A GRU layer is two launches (include/fdlp.h): the input projection of every row at once, a GEMM --
    stage 0's inside the chain's launch (xform_kernel), so the spliced rows never reach HBM, the others in
    dense_kernel -- and gru_scan_kernel (csrc/fdlp_nnet.hip), which walks time with a group of up to 32 utterances as
    the M dimension of the exact-float32 MFMA.  Every value is computed in an order fixed by the layer's widths
    alone, so an utterance's bits do not depend on the batch: the files do not depend on --batch-rows.
  * Feature types (egs.config, or --override_trans): `pca,<mat>` a transform-feats BEFORE the splice; `cmvn,<stats>`
    a global apply-cmvn --norm-vars=true (this script's command line says true, unlike extract_posterior.py);
    `cmvn_utt,<scp>` a table of per-utterance stats, --norm-vars=true, an utterance without stats is warned about,
    counted as an error and skipped, as Kaldi does; anything else is raw.
  * --ae_type=vae samples its latent and --ae_type=vaeenc loads a path hard-coded in the reference: neither is
    reproduced, both exit 1 with a message.  --add_softmax uses the max-subtracted form nnet.py documents.
Out of scope: training, and the CURL, multimod and CNN models.
"""
import argparse
import ctypes
import os
import pickle
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import FdlpRnnConfigC, check, lib, ptr
from .cmvn import read_kaldi_dmatrix
from .nnet import MODES, EgsConfig, NnetRunner, _load_prior
from .post import (FeatWriter, PostConfig, _make_batch, _split_specifier, cmvn_norm, read_dmatrix_table,
                   read_kaldi_matrix)

KINDS = {"gru": _lib.FDLP_RNN_GRU, "linear": _lib.FDLP_RNN_LINEAR, "linear_relu": _lib.FDLP_RNN_LINEAR_RELU}
KIND_NAMES = {v: k for k, v in KINDS.items()}


class RnnPlan:
    """cmvn | deltas | splice | a list of stages.  stages[s] is ("gru", w_ih [3H, K], w_hh [3H, H], b_ih [3H],
    b_hh [3H]) in nn.GRU's layout (gate order r, z, n), or ("linear" | "linear_relu", w [N, K], b [N]); the ReLU of
    "linear_relu" is applied when the next stage loads the output, so tapping it gives the pre-activation.
    device=-1 gives a host-only plan (dims, workspace_bytes, group_utts, lds_bytes, groups()); it needs the shapes
    only: pass stages=None with `kinds` and `dims` (dims[0] the row width the stages of cfg give)."""

    def __init__(self, cfg: PostConfig, stages, max_rows: int = 131072, max_utts: Optional[int] = None,
                 device: int = 0, kinds: Optional[Sequence] = None, dims: Optional[Sequence[int]] = None):
        self.cfg, self.device, self.max_rows = cfg, int(device), int(max_rows)
        self.max_utts = int(max_utts) if max_utts is not None else max(1, self.max_rows)
        arrays = None
        if stages is not None:
            if not stages:
                raise ValueError("RnnPlan: at least one stage")
            kinds, dims, arrays = [], None, []
            for s, st in enumerate(stages):
                kind = st[0]
                if kind not in KINDS or len(st) != (5 if kind == "gru" else 3):
                    raise ValueError("RnnPlan: stage %d must be ('gru', w_ih, w_hh, b_ih, b_hh) or "
                                     "('linear' | 'linear_relu', w, b)" % s)
                a = [np.ascontiguousarray(x, dtype=np.float32) for x in st[1:]]
                if kind == "gru":
                    w_ih, w_hh, b_ih, b_hh = a
                    H = w_hh.shape[1] if w_hh.ndim == 2 else -1
                    if (w_ih.ndim != 2 or w_ih.shape[0] != 3 * H or w_hh.shape != (3 * H, H)
                            or b_ih.shape != (3 * H,) or b_hh.shape != (3 * H,)):
                        raise ValueError("RnnPlan: GRU stage %d has shapes %s, %s, %s, %s"
                                         % (s, w_ih.shape, w_hh.shape, b_ih.shape, b_hh.shape))
                    k_in, n_out, four = w_ih.shape[1], H, [w_ih, w_hh, b_ih, b_hh]
                else:
                    w, b = a
                    if w.ndim != 2 or b.shape != (w.shape[0],):
                        raise ValueError("RnnPlan: linear stage %d has weight %s and bias %s" % (s, w.shape, b.shape))
                    k_in, n_out, four = w.shape[1], w.shape[0], [w, None, b, None]
                if dims is None:
                    dims = [k_in]
                elif dims[-1] != k_in:
                    raise ValueError("RnnPlan: stage %d takes %d columns after a stage of %d outputs"
                                     % (s, k_in, dims[-1]))
                dims.append(n_out)
                kinds.append(kind)
                arrays += four
        kinds = [KINDS.get(k, k) for k in kinds]
        dims = [int(d) for d in dims]
        if len(dims) != len(kinds) + 1:
            raise ValueError("RnnPlan: one dimension more than stages")
        c = FdlpRnnConfigC()
        c.post = cfg.to_c(device)
        c.n_stages = len(kinds)
        for i, k in enumerate(kinds[:_lib.FDLP_RNN_MAX_STAGES]):
            c.kind[i] = int(k)
        for i, d in enumerate(dims[:_lib.FDLP_RNN_MAX_STAGES + 1]):
            c.dims[i] = d
        pp = None
        if arrays is not None:
            pp = (ctypes.c_void_p * len(arrays))(*[a.ctypes.data if a is not None else None for a in arrays])
        h = ctypes.c_void_p()
        check(lib.fdlp_rnn_plan_create(ctypes.byref(c), pp, self.max_rows, self.max_utts, ctypes.byref(h)))
        self._h = h
        ind, ns, gu, lds = _lib.c_i32(), _lib.c_i32(), _lib.c_i32(), _lib.c_i32()
        wsb = _lib.c_i64()
        od = (_lib.c_i32 * _lib.FDLP_RNN_MAX_STAGES)()
        check(lib.fdlp_rnn_plan_info(self._h, ctypes.byref(ind), ctypes.byref(ns), od, ctypes.byref(wsb),
                                     ctypes.byref(gu), ctypes.byref(lds)))
        self.in_dim, self.n_stages = ind.value, ns.value
        self.dims = [ind.value] + [od[i] for i in range(ns.value)]
        self.kinds = [KIND_NAMES[k] for k in kinds]
        self.out_dim = self.dims[-1]
        self.workspace_bytes, self.group_utts, self.lds_bytes = wsb.value, gu.value, lds.value

    def close(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib.fdlp_rnn_plan_destroy(h)
            self._h = None

    def __del__(self):
        self.close()

    def tap_dim(self, tap: int) -> int:
        """columns of the output for `tap` (0: the last stage; s: stage n_stages - 1 - s)"""
        if not 0 <= tap < self.n_stages:
            raise ValueError("tap %d is outside 0 .. %d (the model has %d stages)" % (tap, self.n_stages - 1, self.n_stages))
        return self.dims[self.n_stages - tap]

    def groups(self, lengths: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, int]:
        """(group_of, slot_of, n_groups) of a batch with these lengths: the table gru_scan_kernel is launched with"""
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32))
        g, s = np.zeros(lens.size, dtype=np.int32), np.zeros(lens.size, dtype=np.int32)
        n = _lib.c_i32()
        check(lib.fdlp_rnn_plan_groups(self._h, ptr(lens, ctypes.c_int32), lens.size, ptr(g, ctypes.c_int32),
                                       ptr(s, ctypes.c_int32), ctypes.byref(n)))
        return g, s, n.value

    def set_profiling(self, on: bool):
        check(lib.fdlp_rnn_set_profiling(self._h, int(bool(on))))

    def times(self):
        """(ms in the input projections and linear stages, ms in the scans) since the last call; waits for them"""
        ms = (ctypes.c_double * 2)()
        check(lib.fdlp_rnn_times(self._h, ms))
        return ms[0], ms[1]

    def compute(self, feats: torch.Tensor, lengths: Sequence[int], norm: Optional[torch.Tensor] = None,
                norm_index: Optional[Sequence[int]] = None, norm_vars: bool = True, tap: int = 0, mode: str = "raw",
                prior: Optional[torch.Tensor] = None, prior_weight: float = 0.8,
                offsets: Optional[Sequence[int]] = None, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """As NnetPlan.compute.  tap 0: the last stage's output, in `mode` raw, softmax or loglike; tap s > 0: the
        output of stage n_stages - 1 - s, raw.  Returns out [rows, tap_dim(tap)]."""
        if mode not in MODES:
            raise ValueError("mode must be one of %s" % ", ".join(MODES))
        b, out, keep = _make_batch("RnnPlan.compute", self.cfg.dim, self.tap_dim(tap), feats, lengths, norm,
                                   norm_index, norm_vars, offsets, out)
        pp = None
        if mode == "loglike":
            if (not isinstance(prior, torch.Tensor) or prior.dtype != torch.float32 or prior.device != feats.device
                    or tuple(prior.shape) != (self.out_dim,)):
                raise ValueError("RnnPlan.compute: loglike needs prior, a float32 [%d] tensor on the features' device"
                                 % self.out_dim)
            prior = prior.contiguous()
            pp = ctypes.c_void_p(prior.data_ptr())
        s = stream if stream is not None else torch.cuda.current_stream(feats.device)
        check(lib.fdlp_rnn_compute(self._h, ctypes.byref(b), int(tap), MODES[mode], pp, float(prior_weight),
                                   ctypes.c_void_p(s.cuda_stream)))
        return out


# ---------------------------------------------------------------------------------------------
# the reference's checkpoints: the dicts train_*_hybrid / train_nnet_rnn save
# ---------------------------------------------------------------------------------------------
@dataclass
class RnnCheckpoint:
    ae_type: str
    feature_dim: int
    num_frames: int
    num_classes: int
    header: dict
    stages: List[tuple] = field(default_factory=list)

    num_layers = 0   # NnetRunner's --layer check: only the last stage is written

    @property
    def dims(self):
        return [self.feature_dim * self.num_frames] + [(s[2].shape[1] if s[0] == "gru" else s[1].shape[0])
                                                       for s in self.stages]


NOAE_KEYS = ("feature_dim", "num_frames", "num_layers", "hidden_dim", "num_classes")
NORMAL_KEYS = ("feature_dim", "num_frames", "num_classes", "encoder_num_layers", "classifier_num_layers",
               "ae_num_layers", "hidden_dim", "bn_dim")


def _state_array(path, sd, name, want, hdr):
    if name not in sd:
        raise ValueError("%s: model_state_dict has no key '%s'" % (path, name))
    t = sd[name]
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if a.ndim == 3 and a.shape[2] == 1:   # a Conv1d of kernel size 1: [out, in, 1]
        a = a[:, :, 0]
    if tuple(a.shape) != want:
        raise ValueError("%s: '%s' has shape %s where the header (%s) needs %s"
                         % (path, name, tuple(a.shape), ", ".join("%s %d" % kv for kv in hdr.items()), want))
    return np.ascontiguousarray(a, dtype=np.float32)


def _gru_stages(path, sd, prefix, n, k_in, H, hdr):
    out = []
    for i in range(n):
        p = "%s.%d." % (prefix, i)
        out.append(("gru", _state_array(path, sd, p + "weight_ih_l0", (3 * H, k_in if i == 0 else H), hdr),
                    _state_array(path, sd, p + "weight_hh_l0", (3 * H, H), hdr),
                    _state_array(path, sd, p + "bias_ih_l0", (3 * H,), hdr),
                    _state_array(path, sd, p + "bias_hh_l0", (3 * H,), hdr)))
    extra = [k for k in sd.keys() if k.startswith(prefix + ".") and k[len(prefix) + 1:].split(".")[0].isdigit()
             and int(k[len(prefix) + 1:].split(".")[0]) >= n]
    if extra:
        raise ValueError("%s: model_state_dict has '%s' beyond the %d layers of the header" % (path, extra[0], n))
    return out


def load_rnn_checkpoint(path: str, ae_type: str = "normal") -> RnnCheckpoint:
    """torch.load of the dict the reference's trainers save.  noae: feature_dim, num_frames, num_layers, hidden_dim,
    num_classes and model_state_dict with layers.{i}.{weight_ih,weight_hh,bias_ih,bias_hh}_l0 and
    regression.{weight,bias}.  normal: encoder_num_layers, classifier_num_layers, ae_num_layers, hidden_dim, bn_dim
    beside feature_dim, num_frames, num_classes, with encoder.layers.*, encoder.bottleneck.*, classifier.layers.*,
    classifier.regression.*; every ae.* key is ignored.  Every shape is checked against the header; the errors name
    the key."""
    if ae_type not in ("noae", "normal"):
        raise ValueError("ae_type %r: only 'noae' and 'normal' models are supported" % (ae_type,))
    with open(path, "rb"):   # a missing or unreadable file is an OSError that names it
        pass
    try:
        d = torch.load(path, map_location="cpu")
    except Exception as e:  # an unpickling error of any kind; a truncated archive surfaces as an OSError without a name
        raise ValueError("%s: not a torch checkpoint (%s)" % (path, e))
    if not isinstance(d, dict):
        raise ValueError("%s: the checkpoint is a %s, not a dict" % (path, type(d).__name__))
    keys = NOAE_KEYS if ae_type == "noae" else NORMAL_KEYS
    for k in keys + ("model_state_dict",):
        if k not in d:
            raise ValueError("%s: the checkpoint has no key '%s' (--ae_type=%s)" % (path, k, ae_type))
    hdr = {}
    for k in keys:
        try:
            hdr[k] = int(d[k])
        except (TypeError, ValueError):
            raise ValueError("%s: key '%s' is not an integer (%r)" % (path, k, d[k]))
        if hdr[k] < (0 if k == "ae_num_layers" else 1):
            raise ValueError("%s: key '%s' is %d" % (path, k, hdr[k]))
    sd = d["model_state_dict"]
    if not hasattr(sd, "keys"):
        raise ValueError("%s: key 'model_state_dict' is a %s, not a dict" % (path, type(sd).__name__))
    K0, H, C = hdr["feature_dim"] * hdr["num_frames"], hdr["hidden_dim"], hdr["num_classes"]
    if ae_type == "noae":
        stages = _gru_stages(path, sd, "layers", hdr["num_layers"], K0, H, hdr)
        stages.append(("linear", _state_array(path, sd, "regression.weight", (C, H), hdr),
                       _state_array(path, sd, "regression.bias", (C,), hdr)))
    else:
        bn = hdr["bn_dim"]
        stages = _gru_stages(path, sd, "encoder.layers", hdr["encoder_num_layers"], K0, H, hdr)
        stages.append(("linear_relu", _state_array(path, sd, "encoder.bottleneck.weight", (bn, H), hdr),
                       _state_array(path, sd, "encoder.bottleneck.bias", (bn,), hdr)))
        stages += _gru_stages(path, sd, "classifier.layers", hdr["classifier_num_layers"], bn, H, hdr)
        stages.append(("linear", _state_array(path, sd, "classifier.regression.weight", (C, H), hdr),
                       _state_array(path, sd, "classifier.regression.bias", (C,), hdr)))
    return RnnCheckpoint(ae_type, hdr["feature_dim"], hdr["num_frames"], C, hdr, stages)


def load_rnn_egs_config(path: str, override_trans: Optional[str] = None) -> EgsConfig:
    """egs.config as dump_genclassifier_outputs.py:68-91 reads it: feat_type '<type>,<path>' with type pca, cmvn or
    cmvn_utt (anything else, None included, is raw), replaced by --override_trans when given; concat_feats 'L,R'."""
    try:
        with open(path, "rb") as f:
            d = pickle.load(f)
    except (OSError, IOError):
        raise
    except Exception as e:
        raise ValueError("%s: not a pickled egs.config (%s)" % (path, e))
    if not isinstance(d, dict) or "concat_feats" not in d or (override_trans is None and "feat_type" not in d):
        raise ValueError("%s: egs.config must be a dict with the keys 'feat_type' and 'concat_feats'" % path)
    spec = override_trans if override_trans is not None else d["feat_type"]
    ft = fp = None
    if isinstance(spec, str) and spec.split(",")[0] in ("pca", "cmvn", "cmvn_utt"):
        ft, _, fp = spec.partition(",")
        fp = fp.split(",")[0]
        if not fp:
            raise ValueError("%s: '%s' names no file" % ("--override_trans" if override_trans is not None else path, spec))
    left = right = 0
    if d["concat_feats"]:
        try:
            t = d["concat_feats"].split(",")
            left, right = int(t[0]), int(t[1])
            if len(t) != 2 or left < 0 or right < 0:
                raise ValueError
        except (AttributeError, IndexError, ValueError):
            raise ValueError("%s: 'concat_feats' must be '<left>,<right>' or None, got %r" % (path, d["concat_feats"]))
    return EgsConfig(ft, fp, left, right)


# ---------------------------------------------------------------------------------------------
# runner: NnetRunner's two pinned slots around an RnnPlan; whole utterances, --norm-vars=true
# ---------------------------------------------------------------------------------------------
class RnnRunner(NnetRunner):
    def __init__(self, ckpt: RnnCheckpoint, egs: EgsConfig, mode: str = "raw", prior=None, prior_weight: float = 0.8,
                 device: int = 0, batch_rows: int = 131072, decimals: int = 3, prog: str = "dump-genclassifier-outputs",
                 log=None):
        self.ckpt, self.egs, self.layer, self.mode = ckpt, egs, 0, mode
        self.device, self.batch_rows, self.decimals = int(device), max(1, int(batch_rows)), int(decimals)
        self.prior_weight = float(prior_weight)
        self.log = log or (lambda m: print("WARNING (%s) %s" % (prog, m), file=sys.stderr))
        if egs.left + egs.right + 1 != ckpt.num_frames:
            raise ValueError("the model was trained on %d spliced frames but egs.config splices -%d..+%d"
                             % (ckpt.num_frames, egs.left, egs.right))
        self.norm_host = self.pca_host = self.utt_stats = None
        want = (2, ckpt.feature_dim + 1)
        if egs.feat_type == "cmvn":
            st = read_kaldi_dmatrix(egs.feat_path)
            if st.shape != want:
                raise ValueError("%s: CMVN stats of shape %s for a model of feature dimension %d (need 2 x %d)"
                                 % (egs.feat_path, " x ".join(str(v) for v in st.shape), ckpt.feature_dim, want[1]))
            self.norm_host = cmvn_norm(st, norm_means=True, norm_vars=True)
        elif egs.feat_type == "cmvn_utt":
            self.utt_stats = dict(read_dmatrix_table("scp:" + egs.feat_path))
        elif egs.feat_type == "pca":
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

    def _make_plan(self, rows):
        cfg = PostConfig(dim=self.ckpt.feature_dim, left_context=self.egs.left, right_context=self.egs.right)
        if self.plan is not None:
            self.plan.close()
        self.plan = RnnPlan(cfg, self.ckpt.stages, max_rows=rows, max_utts=rows, device=self.device)

    def _admit(self, utt):
        if self.utt_stats is None:
            return None
        st = self.utt_stats.get(utt)
        if st is None or st.shape != (2, self.ckpt.feature_dim + 1):
            self.log("No normalization statistics available for key %s, producing no output for this utterance" % utt
                     if st is None else "Dimension mismatch: CMVN stats %s for utterance %s" % (st.shape, utt))
            self.num_err += 1
            return False
        return cmvn_norm(st, norm_means=True, norm_vars=True)

    def _added(self, sl, extra):
        if extra is not None:
            sl.norms.append(extra)

    def _launch(self, sl):
        n = sl.fill
        d_in = sl.d_in[:n]
        d_in.copy_(sl.h_in[:n], non_blocking=True)
        if self.pre is not None:
            d_in = self.pre.compute(d_in, sl.lens, self.pca, out=sl.d_mid)[:n]
        norm, idx = self.norm, None
        if self.utt_stats is not None:
            norm, idx = torch.from_numpy(np.stack(sl.norms)).to(d_in.device), list(range(len(sl.norms)))
        self.plan.compute(d_in, sl.lens, norm=norm, norm_index=idx, norm_vars=True, tap=0, mode=self.mode,
                          prior=self.prior, prior_weight=self.prior_weight, out=sl.d_out)
        sl.h_out[:n].copy_(sl.d_out[:n], non_blocking=True)
        sl.done = torch.cuda.Event()
        sl.done.record()

    def _drain(self, sl, writer):
        if sl.done is not None:
            super()._drain(sl, writer)
            sl.norms = []


# ---------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------
def dump_genclassifier_outputs_parser():
    ap = argparse.ArgumentParser(prog="dump-genclassifier-outputs",
                                 description="Logits, posteriors or pseudo log-likelihoods of a GRU acoustic model, on the MI355X")
    ap.add_argument("model", help="checkpoint of the GRU model, as the reference's trainers save it")
    ap.add_argument("scp", help="feats.scp of the JOB (or an ark: / scp: rspecifier)")
    ap.add_argument("egs_config", help="the egs.config pickle written at data preparation")
    ap.add_argument("save_file", help="output base name: <save_file>.ark and .scp are written (or an ark wspecifier)")
    ap.add_argument("--ae_type", default="normal", help="model family: normal (encoder, bottleneck, classifier) or noae (plain "
                    "GRU stack); vae and vaeenc are refused")
    ap.add_argument("--vae", default=None, help="accepted and ignored, as in the reference")
    ap.add_argument("--prior", default=None, help="pickle of the log prior [num_classes]: write log_softmax - prior_weight * prior")
    ap.add_argument("--prior_weight", type=float, default=0.8, help="weight of the prior (default 0.8)")
    ap.add_argument("--add_softmax", action="store_true", help="write softmax posteriors instead of logits (ignored with --prior)")
    ap.add_argument("--override_trans", default=None, help="<pca|cmvn|cmvn_utt>,<path> to use instead of egs.config's feat_type")
    ap.add_argument("--ark_precision", type=int, default=3, help="decimals of the written values, like the "
                    "reference's '%%.3f' text ark; negative keeps float32")
    ap.add_argument("--device", type=int, default=int(os.environ.get("FDLP_DEVICE", "0")))
    ap.add_argument("--batch-rows", type=int, default=131072, help="rows per device batch (whole utterances)")
    return ap


def main_dump_genclassifier_outputs(argv=None):
    prog = "dump-genclassifier-outputs"
    a = dump_genclassifier_outputs_parser().parse_args(argv)
    if a.ae_type not in ("normal", "noae"):
        why = {"vae": "it samples its latent, so its outputs are random",
               "vaeenc": "the reference loads its encoder from a path hard-coded in the script"}.get(a.ae_type)
        print("ERROR (%s) --ae_type=%s is not supported%s" % (prog, a.ae_type, ": %s" % why if why else ""),
              file=sys.stderr)
        return 1
    writer = None
    try:
        ckpt = load_rnn_checkpoint(a.model, a.ae_type)
        egs = load_rnn_egs_config(a.egs_config, a.override_trans)
        mode, prior = "raw", None
        if a.prior:
            mode, prior = "loglike", _load_prior(a.prior)
        elif a.add_softmax:
            mode = "softmax"
        runner = RnnRunner(ckpt, egs, mode=mode, prior=prior, prior_weight=a.prior_weight, device=a.device,
                           batch_rows=a.batch_rows, decimals=a.ark_precision, prog=prog)
        rspec = a.scp if _split_specifier(a.scp)[0] else "scp:" + a.scp
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
    print("LOG (%s) Dumped outputs for %d utterances, errors on %d" % (prog, done, err), file=sys.stderr)
    return 0 if done else 1


if __name__ == "__main__":
    sys.exit(main_dump_genclassifier_outputs(sys.argv[1:]))
