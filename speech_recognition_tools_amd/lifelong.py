"""The multi-domain decode tools of the hybrid recipes on the MI355X: drop-ins for the reference's
src/nnet/compute_lifelong_likelihood.py (recipes/timit/local_pyspeech/decode_lifelong.sh --pm_type px) and
src/nnet/compute_incremental_likelihood.py (decode_incremental.sh), which run D (classifier nnetRNN, likelihood model
nnetVAE) pairs on one feature stream, one utterance at a time in torch on the CPU, and fuse the D posterior streams
into one pseudo-log-likelihood matrix with per-utterance task weights.

Per batch of whole utterances, everything on the device but the D weights of an utterance:

  1. every classifier is an RnnPlan (rnn.py) in mode softmax into its slice of one [D, rows, C] float32 tensor;
  2. task_prior `mm` / `lowent`: mmeasure_kernel gives the M-measure of every (utterance, model) in one pass;
  3. task_prior `dp` / `lowent`: every VAE is an encoder RnnPlan (GRU stack, then ONE linear stage, `means` stacked on
     `vars`: [rows, 2 bn]), vae_sample_kernel (z = mu + exp(sigma) eps), a decoder RnnPlan on an identity chain (GRU
     stack, then vae_decoder.means; vae_decoder.vars is ignored, as in the reference) and vae_elbo_kernel against the
     spliced rows, which a PostPlan of the same chain gives.  It leaves p(x) per (utterance, model);
  4. the two [n_utts, D] float64 tables come back in ONE copy per batch and the weights are computed on the host in
     numpy float64 with the reference's own lines (task_weights), so NaN, tie and entropy behaviour stay literally the
     reference's, and its per-utterance lines are printed to stdout;
  5. lifelong_fuse_kernel writes the float32 output from the posteriors, the weights and exp(prior) (or the prior).
The kernels are csrc/fdlp_lifelong.hip; include/fdlp.h states their arithmetic.  Every value depends on the
utterance's own rows alone, so the files do not depend on --batch-rows.

The sampler's noise comes from the host: torch.randn(1, T, bn_i) from torch's default CPU generator, once per
utterance in scp order and per model in list order, which is the reference's draw order.  --seed S calls
torch.manual_seed(S) first, so a reference run after the same call sees the same noise; without it the run is
unseeded, as the reference is.

Divergences from the reference, on purpose:
  * With task_prior `mm` or a list of floats the VAE output reaches nothing that is written (the reference computes it
    and throws it away): models_px is checked for its count only and never opened, and the per-utterance line
    carries the weights without p(x).
  * Lists of different lengths, classifiers of different num_classes, a prior of another length, a VAE of another
    input width and a GRU wider than the scan's 384 units exit 1 with a message that names the file and the key (the
    reference warns, or fails later).  Transformer VAEs are refused.
  * The M-measure, the ELBO and the fusion are evaluated in float64 from the float32 posteriors (the reference mixes
    float32 torch and float64 numpy); parity is to rounding, as everywhere in this package.
  * lowent in the lifelong tool: compute_lifelong_likelihood.py:187 builds the dp weights from its float32 p(x)
    without the dtype=np.float64 its dp branch has, so exp(300 p(x)) underflows to 0 / 0 for every p(x) below -0.34
    (all of them: p(x) <= -0.5 log(2 pi)), the entropy is NaN and lowent is always mm.  Here p(x) is float64, which is
    what the line means and what the reference computes on float64 models.
  * scp and egs_config name ONE feature stream, as in the reference; a comma list there must repeat one entry.
"""
import argparse
import ctypes
import os
import pickle
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .nnet import open_checkpoint, run_model_tool, state_array
from .post import PostConfig, PostPlan, _split_specifier
from .rnn import RnnPlan, RnnRunner, _gru_stages, load_rnn_checkpoint, load_rnn_egs_config

MAX_MODELS = _lib.FDLP_LIFE_MAX_MODELS
GRU_MAX_HIDDEN = 384              # gru_scan_kernel's limit (include/fdlp.h)
TOOLS = {"lifelong": _lib.FDLP_LIFE_LIFELONG, "incremental": _lib.FDLP_LIFE_INCREMENTAL}
DP_SCALE = {"lifelong": 300.0, "incremental": 500.0}        # exp(300 px): compute_lifelong_likelihood.py:180
LOWENT_SCALE = {"lifelong": 300.0, "incremental": 200.0}    # :188; compute_incremental_likelihood.py:175


# ---------------------------------------------------------------------------------------------
# the four kernels
# ---------------------------------------------------------------------------------------------
def utt_tables(lengths: Sequence[int], device, offsets: Optional[Sequence[int]] = None) -> torch.Tensor:
    """the device int64 [2, n_utt] table (row_off, utt_len) the kernels of a batch share"""
    lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if offsets is None:
        offs = np.zeros(lens.size, dtype=np.int64)
        if lens.size:
            offs[1:] = np.cumsum(lens)[:-1]
    else:
        offs = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if offs.size != lens.size or (lens < 0).any() or (offs < 0).any():
        raise ValueError("one non-negative offset and length per utterance")
    return torch.from_numpy(np.stack([offs, lens])).to(device)


def _stream(t, stream):
    s = stream if stream is not None else torch.cuda.current_stream(t.device)
    return ctypes.c_void_p(s.cuda_stream)


def _f32(name, t, shape=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError("%s must be a contiguous float32 device tensor" % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def _check_tables(tab, post_rows):
    if (not isinstance(tab, torch.Tensor) or tab.dtype != torch.int64 or not tab.is_cuda or tab.dim() != 2
            or tab.shape[0] != 2 or not tab.is_contiguous()):
        raise ValueError("tables must be utt_tables' int64 [2, n_utt] device tensor")
    return tab.shape[1]


def mmeasure(post: torch.Tensor, tables: torch.Tensor, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """M-measure [n_utt, D] float64 of post [D, rows, C] (mmeasure_kernel); the utterances' rows must lie inside
    `rows`, which the caller vouches for, as for every table here"""
    _f32("post", post)
    if post.dim() != 3:
        raise ValueError("post must be [D, rows, C]")
    D, rows, C = post.shape
    n = _check_tables(tables, rows)
    if out is None:
        out = torch.empty((n, D), dtype=torch.float64, device=post.device)
    with torch.cuda.device(post.device):
        check(lib.fdlp_life_mmeasure(post.data_ptr(), D, rows, C, n, tables[0].data_ptr(), tables[1].data_ptr(),
                                     out.data_ptr(), _stream(post, stream)))
    return out


def vae_sample(ml: torch.Tensor, eps: torch.Tensor, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """z [rows, bn] = mu + expf(sigma) eps of ml [rows, 2 bn] (mu, then sigma) and eps [rows, bn] (vae_sample_kernel)"""
    _f32("ml", ml)
    if ml.dim() != 2 or ml.shape[1] % 2 or ml.shape[1] < 2:
        raise ValueError("ml must be [rows, 2 bn]")
    rows, bn = ml.shape[0], ml.shape[1] // 2
    _f32("eps", eps, (rows, bn))
    if out is None:
        out = torch.empty((rows, bn), dtype=torch.float32, device=ml.device)
    _f32("out", out)
    if out.dim() != 2 or out.shape[1] != bn or out.shape[0] < rows:
        raise ValueError("out must be [>= rows, bn]")
    with torch.cuda.device(ml.device):
        check(lib.fdlp_life_vae_sample(ml.data_ptr(), eps.data_ptr(), out.data_ptr(), rows, bn, _stream(ml, stream)))
    return out


def vae_elbo(x: torch.Tensor, xhat: torch.Tensor, ml: torch.Tensor, tables: torch.Tensor, tool: str = "lifelong",
             out: Optional[torch.Tensor] = None, elbo: Optional[torch.Tensor] = None, stream=None):
    """(p(x) per utterance, elbo per row) of x, xhat [rows, K] and ml [rows, 2 bn] (vae_elbo_kernel): float64 [n_utt]
    (or `out`, a float64 column view: its stride is passed on) and float32 [rows]"""
    _f32("x", x)
    rows, K = x.shape
    _f32("xhat", xhat, (rows, K))
    _f32("ml", ml)
    if ml.dim() != 2 or ml.shape[0] != rows or ml.shape[1] % 2 or ml.shape[1] < 2:
        raise ValueError("ml must be [rows, 2 bn]")
    n = _check_tables(tables, rows)
    if out is None:
        out = torch.empty((n,), dtype=torch.float64, device=x.device)
    if out.dtype != torch.float64 or out.dim() != 1 or out.shape[0] != n or out.device != x.device:
        raise ValueError("out must be a float64 [n_utt] device tensor (a column of a table is fine)")
    if elbo is None:
        elbo = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _f32("elbo", elbo)
    with torch.cuda.device(x.device):
        check(lib.fdlp_life_vae_elbo(x.data_ptr(), xhat.data_ptr(), ml.data_ptr(), rows, K, ml.shape[1] // 2, n,
                                     tables[0].data_ptr(), tables[1].data_ptr(), TOOLS[tool], elbo.data_ptr(),
                                     out.data_ptr(), max(int(out.stride(0)), 1) if n else 1, _stream(x, stream)))
    return out, elbo


def fuse(post: torch.Tensor, tables: torch.Tensor, max_len: int, w: torch.Tensor, tab: torch.Tensor,
         prior_weight: float, tool: str = "lifelong", out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """out [rows, C] float32 of post [D, rows, C], w [n_utt, D] float64 and tab [D, C] float64: exp(prior) for
    "lifelong", the prior for "incremental" (lifelong_fuse_kernel)"""
    _f32("post", post)
    D, rows, C = post.shape
    n = _check_tables(tables, rows)
    for name, t, shape in (("w", w, (n, D)), ("tab", tab, (D, C))):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != post.device
                or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous float64 %s tensor on the posteriors' device" % (name, shape))
    if out is None:
        out = torch.empty((rows, C), dtype=torch.float32, device=post.device)
    _f32("out", out)
    if out.dim() != 2 or out.shape[1] != C or out.shape[0] < int(max_len > 0):
        raise ValueError("out must be [rows, C]")
    with torch.cuda.device(post.device):
        check(lib.fdlp_life_fuse(post.data_ptr(), D, rows, C, n, int(max_len), tables[0].data_ptr(),
                                 tables[1].data_ptr(), w.data_ptr(), tab.data_ptr(), float(prior_weight), TOOLS[tool],
                                 out.data_ptr(), _stream(post, stream)))
    return out


# ---------------------------------------------------------------------------------------------
# the task weights: the reference's own lines, numpy float64 on the host
# ---------------------------------------------------------------------------------------------
def entropy(pk) -> float:
    """scipy.stats.entropy(pk): pk normalised to sum 1, then sum of -p log p with 0 for p = 0 and -inf for p < 0"""
    pk = np.asarray(pk, dtype=np.float64)
    with np.errstate(all="ignore"):
        pk = pk / np.sum(pk, axis=0)
        e = np.where(pk > 0, -pk * np.log(np.where(pk > 0, pk, 1.0)), np.where(pk == 0, 0.0, -np.inf))
        e = np.where(np.isnan(pk), np.nan, e)
        return float(np.sum(e))


def task_weights(tool: str, kind: str, mm=None, px=None, fixed=None, stream_selection: bool = False, say=None):
    """the D task weights of one utterance as compute_lifelong_likelihood.py:162-191 (tool "lifelong") or
    compute_incremental_likelihood.py:159-178 ("incremental") compute them.  kind: "mm" (mm: the M-measures), "dp"
    (px: the mean ELBOs, or mean likelihoods), "lowent" (both) or "fixed" (the list).  say: where the reference's
    printed lines go."""
    say = say or (lambda line: None)
    sel = stream_selection and tool == "lifelong"
    with np.errstate(all="ignore"):
        if kind == "fixed":
            return np.asarray(fixed, dtype=np.float64)
        if kind == "mm":
            all_tp = np.asarray(mm, dtype=np.float64)
            for i, v in enumerate(all_tp):
                say("task {:d} , mm={:.2f}".format(i, v))
            if sel:
                temp = np.zeros(all_tp.shape)
                temp[np.argmax(all_tp)] = 1
                all_tp = temp
            else:
                all_tp = np.exp(all_tp) / np.sum(np.exp(all_tp))
            if np.isnan(all_tp[0]):
                say("Switching to uniform priors")
                all_tp = np.ones(all_tp.size) / all_tp.size
            return all_tp
        if kind == "dp":
            all_tp = np.asarray(px, dtype=np.float64)
            if sel:
                temp = np.zeros(all_tp.shape)
                temp[np.argmax(all_tp)] = 1
                return temp
            k = DP_SCALE[tool]
            return np.exp(k * all_tp) / np.sum(np.exp(k * all_tp))
        if kind == "lowent":
            all_tp = np.asarray(mm, dtype=np.float64)
            all_tp = np.exp(all_tp) / np.sum(np.exp(all_tp))
            if np.isnan(all_tp[0]):
                say("Switching to uniform priors")
                all_tp = np.ones(all_tp.size) / all_tp.size
            k = LOWENT_SCALE[tool]
            all_tp_2 = np.asarray(px, dtype=np.float64)
            all_tp_2 = np.exp(k * all_tp_2) / np.sum(np.exp(k * all_tp_2))
            e2, e1 = entropy(all_tp_2), entropy(all_tp)
            say("Entropy dp:{:.2f} and Entropy mm:{:.2f}".format(e2, e1))
            if e2 < e1:
                all_tp = all_tp_2
            return all_tp
    raise ValueError("task_prior kind %r" % (kind,))


def parse_task_prior(text: str, n: int):
    """("mm" | "dp" | "lowent", None) or ("fixed", [D floats])"""
    if text in ("mm", "dp", "lowent"):
        return text, None
    try:
        v = [float(t) for t in text.split(",")]
    except ValueError:
        raise ValueError("task_prior must be mm, dp, lowent or %d comma-separated floats, got %r" % (n, text))
    if len(v) != n:
        raise ValueError("task_prior lists %d weights for %d models" % (len(v), n))
    return "fixed", v


# ---------------------------------------------------------------------------------------------
# the reference's nnetVAE checkpoints
# ---------------------------------------------------------------------------------------------
VAE_KEYS = ("feature_dim", "num_frames", "encoder_num_layers", "decoder_num_layers", "hidden_dim", "bn_dim")


@dataclass
class VaeCheckpoint:
    path: str
    feature_dim: int
    num_frames: int
    bn_dim: int
    header: dict
    enc_stages: List[tuple] = field(default_factory=list)   # GRUs, then ("linear", [means; vars] [2 bn, H], b)
    dec_stages: List[tuple] = field(default_factory=list)   # GRUs, then ("linear", vae_decoder.means [K, H], b)


def _check_width(path, hdr):
    if hdr["hidden_dim"] > GRU_MAX_HIDDEN:
        raise ValueError("%s: key 'hidden_dim' is %d; the GRU scan holds at most %d hidden units"
                         % (path, hdr["hidden_dim"], GRU_MAX_HIDDEN))


def load_vae_checkpoint(path: str) -> VaeCheckpoint:
    """torch.load of the dict train_nnet_VAE saves: feature_dim, num_frames, encoder_num_layers, decoder_num_layers,
    hidden_dim, bn_dim and model_state_dict with vae_encoder.layers.{i}.*_l0, vae_encoder.means / vars (Conv1d of
    kernel size 1), vae_decoder.layers.{i}.*_l0 and vae_decoder.means; vae_decoder.vars is ignored.  Every shape is
    checked against the header; the errors name the file and the key."""
    hdr, sd, top = open_checkpoint(path, VAE_KEYS, whole=True)
    if top.get("use_transformer") or any("self_attn" in k for k in sd.keys()):
        raise ValueError("%s: a transformer VAE (key 'use_transformer', or 'self_attn' tensors in model_state_dict) is "
                         "not supported: only the GRU nnetVAE is" % path)
    _check_width(path, hdr)
    K, H, bn = hdr["feature_dim"] * hdr["num_frames"], hdr["hidden_dim"], hdr["bn_dim"]

    def sub(prefix):
        return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}

    def named(prefix, fn):
        try:
            return fn()
        except ValueError as e:   # the shared readers name the key without the prefix they never saw
            msg = str(e)
            for key in ("layers.", "means.", "vars."):
                msg = msg.replace("'" + key, "'" + prefix + key)
            raise ValueError(msg)

    enc, dec = sub("vae_encoder."), sub("vae_decoder.")
    es = named("vae_encoder.", lambda: _gru_stages(path, enc, "layers", hdr["encoder_num_layers"], K, H, hdr))
    mw = named("vae_encoder.", lambda: state_array(path, enc, "means.weight", (bn, H), hdr, conv1d=True))
    mb = named("vae_encoder.", lambda: state_array(path, enc, "means.bias", (bn,), hdr))
    vw = named("vae_encoder.", lambda: state_array(path, enc, "vars.weight", (bn, H), hdr, conv1d=True))
    vb = named("vae_encoder.", lambda: state_array(path, enc, "vars.bias", (bn,), hdr))
    es.append(("linear", np.ascontiguousarray(np.vstack([mw, vw])), np.ascontiguousarray(np.concatenate([mb, vb]))))
    ds = named("vae_decoder.", lambda: _gru_stages(path, dec, "layers", hdr["decoder_num_layers"], bn, H, hdr))
    ds.append(("linear", named("vae_decoder.", lambda: state_array(path, dec, "means.weight", (K, H), hdr, conv1d=True)),
               named("vae_decoder.", lambda: state_array(path, dec, "means.bias", (K,), hdr))))
    return VaeCheckpoint(path, hdr["feature_dim"], hdr["num_frames"], bn, hdr, es, ds)


def load_classifier(path: str):
    """nnetRNN's checkpoint (rnn.load_rnn_checkpoint, --ae_type=noae), its width held to the scan's limit here"""
    _check_width(path, open_checkpoint(path, ("hidden_dim",))[0])   # before the shapes are held to the header
    return load_rnn_checkpoint(path, "noae")


def load_prior64(path: str) -> np.ndarray:
    try:
        with open(path, "rb") as f:
            p = pickle.load(f)
        return np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1))
    except (OSError, IOError):
        raise
    except Exception as e:
        raise ValueError("%s: not a pickled prior vector (%s)" % (path, e))


def split_lists(models_pcx: str, models_px: str, priors: str):
    """the three lists of D entries; their lengths must agree and lie in 1 .. 8"""
    a, b, c = models_pcx.split(","), models_px.split(","), priors.split(",")
    if not (len(a) == len(b) == len(c)):
        raise ValueError("models_pcx names %d models, models_px %d and priors %d: the lists must have one length"
                         % (len(a), len(b), len(c)))
    if not 1 <= len(a) <= MAX_MODELS or not all(a) or not all(c):
        raise ValueError("models_pcx must name 1 .. %d models, got %d" % (MAX_MODELS, len(a)))
    return a, b, c


def one_stream(text: str, what: str) -> str:
    """scp or egs_config: one entry, or one entry repeated; an rspecifier (whose options may hold commas) as it is"""
    if what == "scp" and _split_specifier(text)[0]:
        return text
    t = text.split(",")
    if len(set(t)) != 1:
        raise ValueError("%s names %d different entries (%s): the models share one feature stream, as in the reference"
                         % (what, len(set(t)), text))
    return t[0]


# ---------------------------------------------------------------------------------------------
# runner: RnnRunner's loop around D classifier plans, the VAE plans and the four kernels
# ---------------------------------------------------------------------------------------------
class LifelongRunner(RnnRunner):
    """ckpts: the D classifiers (load_classifier); vaes: the D VaeCheckpoints, or None where task_prior does not need
    them; priors: D float64 log priors [C]; kind, fixed: parse_task_prior's.  noise: {utterance: [D arrays [T, bn_i]]}
    to use instead of drawing (tests); what was used stays in self.noise_used when keep is set, and the per-utterance
    tables in self.mm, self.px and self.weights."""
    BATCH_ROWS, PROG = 32768, "compute-lifelong-likelihood"

    def __init__(self, ckpts, vaes, egs, priors, kind: str, fixed=None, tool: str = "lifelong",
                 stream_selection: bool = False, prior_weight: float = 0.8, device: int = 0,
                 batch_rows: Optional[int] = None, decimals: int = 3, prog: Optional[str] = None, log=None,
                 noise=None, keep: bool = False, say=None, names=None, prior_names=None):
        if tool not in TOOLS:
            raise ValueError("tool must be lifelong or incremental")
        D = len(ckpts)
        names = list(names) if names is not None else ["model %d" % i for i in range(D)]
        prior_names = list(prior_names) if prior_names is not None else ["prior %d" % i for i in range(D)]
        if not 1 <= D <= MAX_MODELS:
            raise ValueError("1 .. %d models, got %d" % (MAX_MODELS, D))
        if len(priors) != D:
            raise ValueError("%d priors for %d models" % (len(priors), D))
        super().__init__(ckpts[0], egs, mode="raw", prior_weight=prior_weight, device=device, batch_rows=batch_rows,
                         decimals=decimals, prog=prog or ("compute-%s-likelihood" % tool), log=log)
        c0 = ckpts[0]
        for name, c in zip(names[1:], ckpts[1:]):
            if c.num_classes != c0.num_classes:
                raise ValueError("%s: key 'num_classes' is %d where %s has %d" % (name, c.num_classes, names[0],
                                                                                 c0.num_classes))
            if (c.feature_dim, c.num_frames) != (c0.feature_dim, c0.num_frames):
                raise ValueError("%s: keys 'feature_dim', 'num_frames' are %d, %d where %s has %d, %d: the models read "
                                 "one feature stream" % (name, c.feature_dim, c.num_frames, names[0], c0.feature_dim,
                                                         c0.num_frames))
        self.ckpts, self.tool, self.kind, self.fixed = list(ckpts), tool, kind, fixed
        self.stream_selection = bool(stream_selection)
        self.D, self.C = D, c0.num_classes
        ps = []
        for name, p in zip(prior_names, priors):
            p = np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1))
            if p.shape[0] != self.C:
                raise ValueError("%s: the prior has %d entries where %s has key 'num_classes' %d"
                                 % (name, p.shape[0], names[0], self.C))
            ps.append(p)
        self.priors_host = np.stack(ps)
        self.need_mm, self.need_px = kind in ("mm", "lowent"), kind in ("dp", "lowent")
        self.vaes = list(vaes) if self.need_px else None
        if self.need_px:
            if vaes is None or len(vaes) != D or any(v is None for v in vaes):
                raise ValueError("task_prior %s needs the %d likelihood models" % (kind, D))
            K = c0.feature_dim * c0.num_frames
            for v in self.vaes:
                if v.feature_dim * v.num_frames != K:
                    raise ValueError("%s: keys 'feature_dim' * 'num_frames' give %d columns where the spliced rows of "
                                     "%s have %d" % (v.path, v.feature_dim * v.num_frames, names[0], K))
        self.noise, self.keep = noise, bool(keep)
        self.noise_used, self.mm, self.px, self.weights = {}, {}, {}, {}
        self.say = say or (lambda line: (sys.stdout.write(line + "\n"), sys.stdout.flush()))
        self.cls_plans, self.enc_plans, self.dec_plans, self.post_plan = [], [], [], None
        self.ms = None     # per-kernel HIP event times when profile() was called

    # -- plans and buffers -----------------------------------------------------------------
    def _close_plans(self):
        for p in self.cls_plans + self.enc_plans + self.dec_plans + ([self.post_plan] if self.post_plan else []):
            p.close()
        self.cls_plans, self.enc_plans, self.dec_plans, self.post_plan, self.plan = [], [], [], None, None

    def _make_plan(self, rows):
        cfg = PostConfig(dim=self.ckpt.feature_dim, left_context=self.egs.left, right_context=self.egs.right)
        self._close_plans()
        mk = dict(max_rows=rows, max_utts=rows, device=self.device)
        self.cls_plans = [RnnPlan(cfg, c.stages, **mk) for c in self.ckpts]
        self.plan = self.cls_plans[0]
        dev = torch.device("cuda", self.device)
        self.cap = rows
        self.P = torch.empty((self.D, rows, self.C), dtype=torch.float32, device=dev)
        if self.need_px:
            self.post_plan = PostPlan(cfg, self.device)
            self.enc_plans = [RnnPlan(cfg, v.enc_stages, **mk) for v in self.vaes]
            self.dec_plans = [RnnPlan(PostConfig(dim=v.bn_dim), v.dec_stages, **mk) for v in self.vaes]
            K = self.post_plan.out_dim
            f32 = dict(dtype=torch.float32, device=dev)
            self.X, self.XH = torch.empty((rows, K), **f32), torch.empty((rows, K), **f32)
            self.ML = [torch.empty((rows, 2 * v.bn_dim), **f32) for v in self.vaes]
            self.Z = [torch.empty((rows, v.bn_dim), **f32) for v in self.vaes]
            self.EPS = [torch.empty((rows, v.bn_dim), **f32) for v in self.vaes]
            self.ELBO = torch.empty((rows,), **f32)

    def _setup(self, dim):
        super()._setup(dim)
        dev = torch.device("cuda", self.device)
        with np.errstate(all="ignore"):
            tab = np.exp(self.priors_host) if self.tool == "lifelong" else self.priors_host
        self.tab = torch.from_numpy(np.ascontiguousarray(tab)).to(dev)

    # -- the noise, drawn as the utterances are read ------------------------------------------
    def _added(self, sl, extra):
        super()._added(sl, extra)
        if not self.need_px:
            return
        utt, T = sl.keys[-1], sl.lens[-1]
        if self.noise is not None:
            eps = [np.ascontiguousarray(e, dtype=np.float32) for e in self.noise[utt]]
            if len(eps) != self.D or any(e.shape != (T, v.bn_dim) for e, v in zip(eps, self.vaes)):
                raise ValueError("noise of utterance %s: need %d arrays [%d, bn_i]" % (utt, self.D, T))
        else:
            eps = [torch.randn(1, T, v.bn_dim)[0].numpy() for v in self.vaes]
        if not hasattr(sl, "eps") or len(sl.keys) == 1:
            sl.eps = []
        sl.eps.append(eps)
        if self.keep:
            self.noise_used[utt] = eps

    # -- one batch ----------------------------------------------------------------------------
    def _timed(self, name, fn):
        if self.ms is None:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self._events.append((name, a, b))
        return r

    def profile(self, on=True):
        """collect HIP event times per kernel family in self.ms (a dict of ms) from the next batch on"""
        self.ms, self._events = ({} if on else None), []

    def collect_times(self):
        torch.cuda.synchronize(self.device)
        for name, a, b in self._events:
            self.ms[name] = self.ms.get(name, 0.0) + a.elapsed_time(b)
        self._events = []
        return self.ms

    def _launch(self, sl):
        n, D = sl.fill, self.D
        d_in = sl.d_in[:n]
        d_in.copy_(sl.h_in[:n], non_blocking=True)
        if self.pre is not None:
            d_in = self.pre.compute(d_in, sl.lens, self.pca, out=sl.d_mid)[:n]
        norm, idx = self._norm_args(sl)
        chain = dict(norm=norm, norm_index=idx, norm_vars=self.NORM_VARS)
        tables = utt_tables(sl.lens, d_in.device)
        U = len(sl.lens)
        for i, plan in enumerate(self.cls_plans):
            self._timed("classifiers", lambda: plan.compute(d_in, sl.lens, mode="softmax", out=self.P[i], **chain))
        both = torch.full((2, U, D), float("nan"), dtype=torch.float64, device=d_in.device)
        if self.need_mm:
            self._timed("mmeasure_kernel", lambda: mmeasure(self.P, tables, out=both[0]))
        if self.need_px:
            self._timed("post_kernel", lambda: self.post_plan.compute(d_in, sl.lens, out=self.X, **chain))
            for i in range(D):
                ml = self._timed("vae_plans", lambda: self.enc_plans[i].compute(d_in, sl.lens, out=self.ML[i], **chain))[:n]
                eps = self.EPS[i][:n]
                eps.copy_(torch.from_numpy(np.concatenate([e[i] for e in sl.eps])), non_blocking=False)
                z = self._timed("vae_sample_kernel", lambda: vae_sample(ml, eps, out=self.Z[i]))[:n]
                xh = self._timed("vae_plans", lambda: self.dec_plans[i].compute(z, sl.lens, out=self.XH))[:n]
                self._timed("vae_elbo_kernel", lambda: vae_elbo(self.X[:n], xh, ml, tables, self.tool,
                                                                 out=both[1, :, i], elbo=self.ELBO[:n]))
        host = both.cpu().numpy() if (self.need_mm or self.need_px) else None   # the one sync of the batch
        w = np.zeros((U, D))
        for u, utt in enumerate(sl.keys):
            mm = host[0, u] if self.need_mm else None
            px = host[1, u] if self.need_px else None
            w[u] = task_weights(self.tool, self.kind, mm, px, self.fixed, self.stream_selection, self.say)
            if self.need_px:
                self.say("".join("p(x) for Task {:d} ={:.6f} with prior ={:.6f} ".format(i, px[i], w[u, i])
                                 for i in range(D)))
            else:
                self.say("".join("Task {:d} prior ={:.6f} ".format(i, w[u, i]) for i in range(D)))
            if self.keep:
                self.mm[utt], self.px[utt], self.weights[utt] = mm, px, w[u].copy()
        wd = torch.from_numpy(w).to(d_in.device)
        self._timed("lifelong_fuse_kernel", lambda: fuse(self.P, tables, max(sl.lens), wd, self.tab, self.prior_weight,
                                                         self.tool, out=sl.d_out))
        sl.h_out[:n].copy_(sl.d_out[:n], non_blocking=True)
        sl.done = torch.cuda.Event()
        sl.done.record()

    def close(self):
        self._close_plans()


# ---------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------
def _parser(prog, tool):
    ap = argparse.ArgumentParser(prog=prog, description="Pseudo log-likelihoods of D GRU classifiers fused with per-utterance "
                                 "task weights (%s recipe), on the MI355X" % tool)
    ap.add_argument("models_pcx", help="the D classifier checkpoints (nnetRNN), comma-separated")
    ap.add_argument("models_px", help="the D likelihood models (nnetVAE), comma-separated; opened for dp / lowent only")
    ap.add_argument("scp", help="feats.scp of the JOB (or an ark: / scp: rspecifier)")
    ap.add_argument("egs_config", help="the egs.config pickle written at data preparation")
    ap.add_argument("priors", help="the D pickled log priors [num_classes], comma-separated")
    ap.add_argument("task_prior", help="mm, dp, lowent, or D comma-separated weights")
    ap.add_argument("save_file", help="output base name: <save_file>.ark and .scp are written (or an ark wspecifier)")
    if tool == "lifelong":
        ap.add_argument("--stream_selection", action="store_true",
                        help="one-hot weights at the best task instead of a fusion (mm and dp)")
    ap.add_argument("--prior_weight", type=float, default=0.8, help="weight of the prior (default 0.8)")
    ap.add_argument("--override_trans", default=None, help="<pca|cmvn|cmvn_utt>,<path> to use instead of egs.config's feat_type")
    ap.add_argument("--seed", type=int, default=None, help="torch.manual_seed(S) before the sampler's noise is drawn "
                    "(default: unseeded, as the reference)")
    ap.add_argument("--ark_precision", type=int, default=3, help="decimals of the written values, like the "
                    "reference's '%%.3f' text ark; negative keeps float32")
    ap.add_argument("--device", type=int, default=int(os.environ.get("FDLP_DEVICE", "0")))
    ap.add_argument("--batch-rows", type=int, default=LifelongRunner.BATCH_ROWS,
                    help="rows per device batch (whole utterances)")
    return ap


def compute_lifelong_likelihood_parser():
    return _parser("compute-lifelong-likelihood", "lifelong")


def compute_incremental_likelihood_parser():
    return _parser("compute-incremental-likelihood", "incremental")


def make_runner(a, tool, prog, **kw):
    """the runner of parsed arguments `a`: every file is read and checked here"""
    pcx, px, pri = split_lists(a.models_pcx, a.models_px, a.priors)
    kind, fixed = parse_task_prior(a.task_prior, len(pcx))
    a.scp = one_stream(a.scp, "scp")
    egs = load_rnn_egs_config(one_stream(a.egs_config, "egs_config"), a.override_trans)
    ckpts = [load_classifier(p) for p in pcx]
    vaes = [load_vae_checkpoint(p) for p in px] if kind in ("dp", "lowent") else None
    priors = [load_prior64(p) for p in pri]
    if a.seed is not None:
        torch.manual_seed(a.seed)
    if kind == "mm":
        print("using mm-measure based task priors")
    elif kind == "dp":
        print("using data based task priors")
    elif kind == "lowent":
        print("Using low-entropy prior")
    return LifelongRunner(ckpts, vaes, egs, priors, kind, fixed, tool=tool,
                          stream_selection=getattr(a, "stream_selection", False), prior_weight=a.prior_weight,
                          device=a.device, batch_rows=a.batch_rows, decimals=a.ark_precision, prog=prog, names=pcx,
                          prior_names=pri, **kw)


def _main(argv, tool):
    prog = "compute-%s-likelihood" % tool
    a = _parser(prog, tool).parse_args(argv)
    return run_model_tool(prog, a, lambda: make_runner(a, tool, prog), "Computed likelihoods")


def main_compute_lifelong_likelihood(argv=None):
    return _main(argv, "lifelong")


def main_compute_incremental_likelihood(argv=None):
    return _main(argv, "incremental")


if __name__ == "__main__":
    sys.exit(main_compute_lifelong_likelihood(sys.argv[1:]))
