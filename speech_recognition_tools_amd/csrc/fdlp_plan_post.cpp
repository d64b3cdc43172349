// fdlp_plan_post.cpp -- the chain plans on float32 feature rows: apply-cmvn | add-deltas | splice-feats
// (post_kernel of fdlp_post.hip), the same chain into transform-feats (xform_kernel), and the CMVN statistics.
#include <stdio.h>
#include <string.h>

#include "fdlp_plan_common.h"

using fdlp::fail;
using namespace fdlp::host;

// ---------------------------------------------------------------------------------------------
// Post-processing plan (apply-cmvn | add-deltas | splice-feats, fdlp_post.hip): fdlp_post_plan, fdlp_plan_common.h
// ---------------------------------------------------------------------------------------------
// extra_lds: bytes a workgroup needs beside the two tiles (the transform's matrix chunk, 0 for the plain chain)
static int post_plan_create(const fdlp_post_config* cfg, fdlp_post_plan** out, size_t extra_lds) {
  *out = nullptr;
  const fdlp_post_config& c = *cfg;
  if (c.dim < 1 || c.truncate < 0 || c.left_context < 0 || c.right_context < 0 || c.delta_order < 0)
    return fail(FDLP_E_INVALID, "invalid post configuration (dim >= 1, truncate, contexts and delta order >= 0)");
  if (c.truncate > c.dim)
    return fail(FDLP_E_INVALID, "Cannot truncate features as dimension " + std::to_string(c.dim) +
                                    " is smaller than truncation dimension " + std::to_string(c.truncate));
  if (c.delta_order > fdlp::kPostMaxOrder) return fail(FDLP_E_INVALID, "delta order above 8 is not supported");
  if (c.delta_order > 0 && (c.delta_window < 1 || c.delta_window >= 1000))
    return fail(FDLP_E_INVALID, "delta window must be in 1 .. 999");
  if (c.left_context > 100000 || c.right_context > 100000) return fail(FDLP_E_INVALID, "context too large");
  PlanPtr<fdlp_post_plan> p(new (std::nothrow) fdlp_post_plan);
  if (!p) return fail(FDLP_E_NOMEM, "out of memory");
  p->cfg = c;
  p->res.device = c.device;
  const int window = c.delta_order > 0 ? c.delta_window : 0;
  p->cfg.delta_window = window;
  p->D = c.truncate > 0 ? c.truncate : c.dim;
  const int64_t Dp = (int64_t)p->D * (c.delta_order + 1);
  const int64_t Dout = Dp * (c.left_context + c.right_context + 1);
  p->tf = Dout < (1 << 24)
      ? fdlp::post_pick_tile(p->D, c.delta_order, window, c.left_context, c.right_context, extra_lds) : 0;
  if (p->tf == 0) {
    const double need = (double)extra_lds + (Dout < (1 << 24)
        ? (double)fdlp::post_lds_bytes(1, p->D, c.delta_order, window, c.left_context, c.right_context) : 4.0 * Dout);
    char msg[320];
    snprintf(msg, sizeof msg, "post plan does not fit the 160 KB LDS at one frame per tile: dim %d, delta order %d "
             "window %d, context -%d..+%d give %lld output columns and need %.0f bytes",
             (int)(c.truncate > 0 ? c.truncate : c.dim), (int)c.delta_order, window, (int)c.left_context,
             (int)c.right_context, (long long)Dout, need);
    return fail(FDLP_E_INVALID, msg);
  }
  p->Dp = (int)Dp;
  p->Dout = (int)Dout;
  p->lds = fdlp::post_lds_bytes(p->tf, p->D, c.delta_order, window, c.left_context, c.right_context);
  post_scale_tables(c.delta_order, window, p->lens, p->scales);
  fdlp::PostConsts& k = p->pc;
  k.Din = c.dim; k.D = p->D; k.order = c.delta_order; k.window = window; k.L = c.left_context; k.R = c.right_context;
  k.tf = p->tf; k.Dp = p->Dp; k.Dout = p->Dout;
  k.a_floats = (int)((p->lds / sizeof(float)) - ((size_t)p->tf + k.L + k.R) * p->Dp);
  k.kstep = 1024 % p->Dout; k.rstep = 1024 / p->Dout;
  int off = 0;
  for (int i = 0; i <= fdlp::kPostMaxOrder; ++i) {
    k.soff[i] = off;
    if (i <= c.delta_order) off += p->lens[(size_t)i];
  }
  if (c.device < 0) {
    *out = p.release();
    return FDLP_OK;
  }
  std::optional<DeviceGuard> dg;
  int rc;
  if ((rc = open_device(c.device, dg)) != FDLP_OK) return rc;
  if ((rc = upload(p->res, &p->d_scales, p->scales.data(), p->scales.size())) != FDLP_OK) return rc;
  if (p->tiles.event(p->res) != hipSuccess) return fail(FDLP_E_NOMEM, "post plan event creation failed");
  k.scales = p->d_scales;
  *out = p.release();
  return FDLP_OK;
}

int fdlp::host::post_compute(fdlp_post_plan* p, const fdlp_post_batch* b, void* stream, const fdlp::XformConsts* xc,
                             const void* mats, const int32_t* mat_index) {
  if (!p || !b || p->cfg.device < 0) return fail(FDLP_E_INVALID, "fdlp_post_compute: bad args or host-only plan");
  if (b->n_utt < 0 || b->n_rows < 0 || (b->n_utt > 0 && (!b->in_dev || !b->out_dev || !b->row_off || !b->utt_len)))
    return fail(FDLP_E_INVALID, "fdlp_post_compute: bad batch");
  if (b->norm_dev && b->n_norm < 1) return fail(FDLP_E_INVALID, "fdlp_post_compute: empty norm table");
  if (((uintptr_t)b->in_dev | (uintptr_t)b->out_dev | (uintptr_t)b->norm_dev) & 3u)
    return fail(FDLP_E_INVALID, "fdlp_post_compute: pointers must be 4-byte aligned");
  size_t nt = 0;
  for (int u = 0; u < b->n_utt; ++u) {
    const int64_t T = b->utt_len[u], r0 = b->row_off[u];
    if (T < 1 || T > INT32_MAX - 2 * 1100000 || r0 < 0 || r0 > b->n_rows - T)
      return fail(FDLP_E_INVALID, "utterance " + std::to_string(u) + " is empty or outside the batch's rows");
    if (b->norm_dev && b->norm_index && (b->norm_index[u] < 0 || b->norm_index[u] >= b->n_norm))
      return fail(FDLP_E_INVALID, "norm_index out of range for utterance " + std::to_string(u));
    if (xc && mat_index && (mat_index[u] < 0 || mat_index[u] >= xc->n_mat))
      return fail(FDLP_E_INVALID, "mat_index out of range for utterance " + std::to_string(u));
    nt += (size_t)((T + p->tf - 1) / p->tf);
  }
  if (nt == 0) return FDLP_OK;
  if (nt > (size_t)INT32_MAX) return fail(FDLP_E_CAPACITY, "too many tiles in one batch");
  DeviceGuard dg(p->cfg.device);
  HIP_TRY(dg.status());
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = p->tiles.wait()) != FDLP_OK) return rc;
  if ((rc = p->tiles.reserve(p->res, nt, "post plan tile table allocation failed")) != FDLP_OK) return rc;
  size_t k = 0;
  for (int u = 0; u < b->n_utt; ++u) {
    const int64_t T = b->utt_len[u];
    for (int64_t t0 = 0; t0 < T; t0 += p->tf) {
      fdlp::PostTile& tl = p->tiles.host[k++];
      tl.row0 = b->row_off[u];
      tl.T = (int32_t)T;
      tl.t0 = (int32_t)t0;
      tl.norm = b->norm_dev && b->norm_index ? b->norm_index[u] : 0;
      tl.mat = xc && mat_index ? mat_index[u] : 0;
    }
  }
  fdlp::PostConsts pc = p->pc;
  pc.vec4 = pc.Din % 4 == 0 && pc.D % 4 == 0 && (((uintptr_t)b->in_dev | (uintptr_t)b->norm_dev) & 15u) == 0;
  if ((rc = p->tiles.publish(nt, s)) != FDLP_OK) return rc;
  if (xc)
    HIP_TRY(fdlp::launch_xform(pc, *xc, p->tiles.dev, (int)nt, (const float*)b->in_dev, b->n_rows,
                               (const float*)b->norm_dev, b->norm_mul, (const float*)mats, (float*)b->out_dev, s));
  else
    HIP_TRY(fdlp::launch_post(pc, p->tiles.dev, (int)nt, (const float*)b->in_dev, b->n_rows,
                              (const float*)b->norm_dev, b->norm_mul, (float*)b->out_dev, s));
  return FDLP_OK;
}

int fdlp_post_plan_create(const fdlp_post_config* cfg, fdlp_post_plan** out) {
  if (!cfg || !out) return fail(FDLP_E_INVALID, "fdlp_post_plan_create: null argument");
  return post_plan_create(cfg, out, 0);
}

int fdlp_post_plan_destroy(fdlp_post_plan* p) { delete p; return FDLP_OK; }

int fdlp_post_plan_info(const fdlp_post_plan* p, int32_t* out_dim, int32_t* tile, int32_t* lds_bytes) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_post_plan_info: null plan");
  if (out_dim) *out_dim = p->Dout;
  if (tile) *tile = p->tf;
  if (lds_bytes) *lds_bytes = (int32_t)p->lds;
  return FDLP_OK;
}

int fdlp_post_plan_scales(const fdlp_post_plan* p, int32_t* lens, float* scales) {
  if (!p) return fail(FDLP_E_INVALID, "fdlp_post_plan_scales: null plan");
  if (lens) memcpy(lens, p->lens.data(), sizeof(int32_t) * p->lens.size());
  if (scales) memcpy(scales, p->scales.data(), sizeof(float) * p->scales.size());
  return FDLP_OK;
}

int fdlp_post_compute(fdlp_post_plan* p, const fdlp_post_batch* b, void* stream) {
  return post_compute(p, b, stream, nullptr, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------
// Transform plan (cmvn | deltas | splice | transform-feats, xform_kernel of fdlp_post.hip): a post plan whose
// tile leaves room for the staged matrix chunk, and the matrix shape (fdlp_xform_plan, fdlp_plan_common.h)
// ---------------------------------------------------------------------------------------------
int fdlp_xform_plan_create(const fdlp_xform_config* cfg, fdlp_xform_plan** out) {
  if (!cfg || !out) return fail(FDLP_E_INVALID, "fdlp_xform_plan_create: null argument");
  *out = nullptr;
  if (cfg->out_dim < 1 || cfg->out_dim > FDLP_XFORM_MAX_OUT_DIM)
    return fail(FDLP_E_INVALID, "transform rows (out_dim) must be in 1 .. " + std::to_string(FDLP_XFORM_MAX_OUT_DIM) +
                                    ", got " + std::to_string(cfg->out_dim));
  PlanPtr<fdlp_xform_plan> x(new (std::nothrow) fdlp_xform_plan);
  if (!x) return fail(FDLP_E_NOMEM, "out of memory");
  fdlp_post_plan* post = nullptr;
  const int rc = post_plan_create(&cfg->post, &post, fdlp::xform_ms_bytes(cfg->out_dim));
  if (rc != FDLP_OK) {
    // the post plan's message names the sizes; add the transform's
    fdlp::last_error_slot() += " (with a transform to " + std::to_string(cfg->out_dim) + " columns, " +
                               std::to_string(fdlp::xform_ms_bytes(cfg->out_dim)) + " of the bytes)";
    return rc;
  }
  x->post.reset(post);
  x->N = cfg->out_dim;
  x->affine = cfg->affine != 0;
  x->C = x->post->Dout + x->affine;
  x->lds = x->post->lds + fdlp::xform_ms_bytes(x->N);
  *out = x.release();
  return FDLP_OK;
}

int fdlp_xform_plan_destroy(fdlp_xform_plan* x) { delete x; return FDLP_OK; }

int fdlp_xform_plan_info(const fdlp_xform_plan* x, int32_t* in_dim, int32_t* out_dim, int32_t* mat_cols,
                         int32_t* tile, int32_t* lds_bytes) {
  if (!x) return fail(FDLP_E_INVALID, "fdlp_xform_plan_info: null plan");
  if (in_dim) *in_dim = x->post->Dout;
  if (out_dim) *out_dim = x->N;
  if (mat_cols) *mat_cols = x->C;
  if (tile) *tile = x->post->tf;
  if (lds_bytes) *lds_bytes = (int32_t)x->lds;
  return FDLP_OK;
}

int fdlp_xform_plan_dispatch(const fdlp_xform_plan* x, int32_t info[8]) {
  if (!x || !info) return fail(FDLP_E_INVALID, "fdlp_xform_plan_dispatch: null argument");
  const fdlp::XformDispatch d = fdlp::xform_dispatch(x->post->pc, x->N);
  info[0] = d.mode; info[1] = d.ncb; info[2] = d.groups; info[3] = d.tile;
  info[4] = d.vec; info[5] = d.full_chunks; info[6] = d.tail; info[7] = d.big_lds;
  return FDLP_OK;
}

int fdlp_xform_compute(fdlp_xform_plan* x, const fdlp_post_batch* b, const void* mat_dev, int32_t n_mat,
                       const int32_t* mat_index, void* stream) {
  if (!x || !b) return fail(FDLP_E_INVALID, "fdlp_xform_compute: null argument");
  if (x->post->cfg.device < 0) return fail(FDLP_E_INVALID, "fdlp_xform_compute: host-only plan");
  if (!mat_dev || n_mat < 1 || ((uintptr_t)mat_dev & 3u))
    return fail(FDLP_E_INVALID, "fdlp_xform_compute: the transform table must be a 4-byte aligned device pointer "
                                "to at least one matrix");
  fdlp::XformConsts xc{};
  xc.N = x->N; xc.C = x->C; xc.affine = x->affine; xc.n_mat = n_mat;
  return post_compute(x->post.get(), b, stream, &xc, mat_dev, mat_index);
}

int fdlp_cmvn_accumulate(const float* feats, int64_t rows, int32_t dim, double* stats, void* stream) {
  if (rows < 0 || dim <= 0 || !stats || (rows > 0 && !feats)) return fail(FDLP_E_INVALID, "fdlp_cmvn_accumulate: bad args");
  hipStream_t s = (hipStream_t)stream;
  const size_t nch = (size_t)fdlp::cmvn_chunks(rows);
  double* part = nullptr;
  // stream-ordered scratch for the per-chunk partial sums [nch, 2, dim]
  HIP_TRY(hipMallocAsync((void**)&part, sizeof(double) * 2 * (size_t)dim * std::max<size_t>(nch, 1), s));
  hipError_t e = fdlp::launch_cmvn(feats, rows, dim, part, stats, s);
  hipError_t e2 = hipFreeAsync(part, s);
  if (e != hipSuccess) return fail(FDLP_E_HIP, std::string("cmvn kernels: ") + hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(FDLP_E_HIP, std::string("hipFreeAsync: ") + hipGetErrorString(e2));
  return FDLP_OK;
}
