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
    reproduced, both exit 1 with a message (the deterministic form of that family, which reads the encoder's path
    from the checkpoint, is compute-vae-encoded-likelihood, vaeenc.py).  --add_softmax uses the max-subtracted form
    nnet.py documents.
Out of scope: training, and the CURL and CNN models (the multi-stream model is multimod.py).

The plan's compute, the runner, the file readers and the command line's body are nnet.py's (StagePlan, NnetRunner,
open_checkpoint, read_egs_config, run_model_tool); this module adds the stage list, the GRU checkpoints, the
per-utterance stats and --override_trans.
"""
import argparse
import ctypes
import os
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import FdlpRnnConfigC, check, lib, ptr
from .nnet import (EgsConfig, NnetRunner, StagePlan, _load_prior, open_checkpoint, read_egs_config, run_model_tool,
                   state_array)
from .post import PostConfig, cmvn_norm

KINDS = {"gru": _lib.FDLP_RNN_GRU, "linear": _lib.FDLP_RNN_LINEAR, "linear_relu": _lib.FDLP_RNN_LINEAR_RELU}
KIND_NAMES = {v: k for k, v in KINDS.items()}


class RnnPlan(StagePlan):
    """cmvn | deltas | splice | a list of stages.  stages[s] is ("gru", w_ih [3H, K], w_hh [3H, H], b_ih [3H],
    b_hh [3H]) in nn.GRU's layout (gate order r, z, n), or ("linear" | "linear_relu", w [N, K], b [N]); the ReLU of
    "linear_relu" is applied when the next stage loads the output, so tapping it gives the pre-activation.
    device=-1 gives a host-only plan (dims, workspace_bytes, group_utts, lds_bytes, groups()); it needs the shapes
    only: pass stages=None with `kinds` and `dims` (dims[0] the row width the stages of cfg give)."""
    _DESTROY, _COMPUTE = "fdlp_rnn_plan_destroy", "fdlp_rnn_compute"

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
    return state_array(path, sd, name, want, hdr, conv1d=True)   # the regression layers are Conv1d of kernel size 1


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
    hdr, sd = open_checkpoint(path, NOAE_KEYS if ae_type == "noae" else NORMAL_KEYS, zero_ok=("ae_num_layers",),
                              hint=" (--ae_type=%s)" % ae_type)
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
    d, left, right = read_egs_config(path, ("feat_type", "concat_feats") if override_trans is None
                                     else ("concat_feats",))
    spec = override_trans if override_trans is not None else d["feat_type"]
    ft = fp = None
    if isinstance(spec, str) and spec.split(",")[0] in ("pca", "cmvn", "cmvn_utt"):
        ft, _, fp = spec.partition(",")
        fp = fp.split(",")[0]
        if not fp:
            raise ValueError("%s: '%s' names no file" % ("--override_trans" if override_trans is not None else path, spec))
    return EgsConfig(ft, fp, left, right)


# ---------------------------------------------------------------------------------------------
# runner: NnetRunner around an RnnPlan; whole utterances, --norm-vars=true, per-utterance stats as a norm table
# ---------------------------------------------------------------------------------------------
class RnnRunner(NnetRunner):
    NORM_VARS = True
    FEAT_TYPES = ("cmvn", "cmvn_utt", "pca")
    BATCH_ROWS, PROG = 131072, "dump-genclassifier-outputs"

    def _new_plan(self, cfg, rows):
        return RnnPlan(cfg, self.ckpt.stages, max_rows=rows, max_utts=rows, device=self.device)

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

    def _norm_args(self, sl):
        if self.utt_stats is None:
            return self.norm, None
        return torch.from_numpy(np.stack(sl.norms)).to(sl.d_in.device), list(range(len(sl.norms)))


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

    def make_runner():
        ckpt = load_rnn_checkpoint(a.model, a.ae_type)
        egs = load_rnn_egs_config(a.egs_config, a.override_trans)
        mode, prior = "raw", None
        if a.prior:
            mode, prior = "loglike", _load_prior(a.prior)
        elif a.add_softmax:
            mode = "softmax"
        return RnnRunner(ckpt, egs, mode=mode, prior=prior, prior_weight=a.prior_weight, device=a.device,
                         batch_rows=a.batch_rows, decimals=a.ark_precision, prog=prog)

    return run_model_tool(prog, a, make_runner, "Dumped outputs")


if __name__ == "__main__":
    sys.exit(main_dump_genclassifier_outputs(sys.argv[1:]))
