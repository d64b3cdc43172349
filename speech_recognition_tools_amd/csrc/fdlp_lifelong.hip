// fdlp_lifelong.hip -- gfx950 kernels of the multi-domain tools (src/nnet/compute_lifelong_likelihood.py and
// compute_incremental_likelihood.py): what those scripts do AFTER the logits of their D (classifier, VAE) pairs
//   mmeasure_kernel       the M-measure of a posterior stream (mmeasure_loss, :32-41), one pass over the posteriors
//   vae_sample_kernel     latentSampler (nnet_models.py:372-382) on noise the host drew
//   vae_elbo_kernel       vae_loss (:20-24) per frame, then its mean (or the mean of its exp) per utterance
//   lifelong_fuse_kernel  the fusion of the D posterior streams into one pseudo-log-likelihood matrix (:192-201;
//                         compute_incremental_likelihood.py:179-187)
// The forward passes are fdlp_nnet.hip's.  Every float64 operation below is rounded as written (no contraction), and
// every sum runs in an order fixed by the utterance's T, the column count and the model count alone: a result does
// not depend on the utterance's place in the batch nor on the batch.  The utterance tables (row_off, utt_len) are
// DEVICE arrays here: the four launches of a batch share one upload.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fdlp_device.h"
#include "fdlp_internal.h"

namespace fdlp {

// -----------------------------------------------------------------------------------------------------------
// mmeasure_kernel.  P [T, C] the float32 posteriors of one (model, utterance); for d in (5, 25, 45, 65), n = max(T - d, 0),
// X = P[d:], Y = P[:-d], lx = log X, ly = log Y (float64 logs of the float32 values), dl = lx - ly:
//     S1_d = sum_{t,c} (X dl - Y dl)            sym_kld's two sums, pair by pair; a zero on either side gives NaN
//     S2_d = sum_{t,c} X (lx - Y)               nn.KLDivLoss()(Y, X) as the script calls it, before its mean
//     M    = (sum_d (S1_d / n + S2_d / (n C))) / 4          d ascending from 0.0; T <= 65 gives 0 / 0 = NaN
// A workgroup owns (column tile of kMmTC columns, utterance, model) and walks t in chunks of kMmRows rows: its 4 waves
// load the chunk (lane = column, kMmRows / 4 rows per wave, the next chunk's loads issued before this chunk's arithmetic),
// take the logs and put (p, log p) into an LDS ring of kMmRing rows; then wave w pairs every new row t with ring
// row t - d_w, t ascending.  So each posterior is read from HBM once and its log taken once.  A lane's two sums
// run over t ascending for its column; lane 0 of the wave then adds the tile's columns ascending, and
// mmeasure_finish_kernel adds the tiles ascending: the order is fixed by (T, C).
// -----------------------------------------------------------------------------------------------------------
constexpr int kMmTC = 64, kMmRows = 8, kMmPer = kMmRows / 4, kMmRing = 76, kMmThreads = 256, kMmLags = 4;
__device__ __constant__ int kMmLag[kMmLags] = {5, 25, 45, 65};
static_assert(kMmRing >= 65 + kMmRows, "a chunk's rows must not overwrite ring rows the chunk still pairs with");

__global__ __launch_bounds__(kMmThreads) void mmeasure_kernel(const float* __restrict__ post, int64_t n_rows, int C,
                                                              const int64_t* __restrict__ row_off,
                                                              const int64_t* __restrict__ utt_len, int n_tiles,
                                                              double* __restrict__ part) {
  __shared__ double lg[kMmRing][kMmTC];
  __shared__ float pv[kMmRing][kMmTC];
  const int tile = blockIdx.x, u = blockIdx.y, m = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = tile * kMmTC + lane;
  const bool act = c < C;
  const int64_t T = utt_len[u], r0 = row_off[u];
  FDLP_CHECK(T >= 0 && r0 >= 0 && r0 + T <= n_rows);
  const float* P = post + ((int64_t)m * n_rows + r0) * C + c;
  const int d = kMmLag[w];
  double s1 = 0.0, s2 = 0.0;
  float nx[kMmPer];  // rows t0 + w + 4 j of the next chunk
#pragma unroll
  for (int j = 0; j < kMmPer; ++j) nx[j] = act && w + 4 * j < T ? P[(int64_t)(w + 4 * j) * C] : 1.f;
  for (int64_t t0 = 0; t0 < T; t0 += kMmRows) {
#pragma unroll
    for (int j = 0; j < kMmPer; ++j) {
      const int64_t t = t0 + w + 4 * j;
      if (t < T) {
        pv[t % kMmRing][lane] = nx[j];
        lg[t % kMmRing][lane] = log((double)nx[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kMmPer; ++j) {
      const int64_t t = t0 + kMmRows + w + 4 * j;
      if (act && t < T) nx[j] = P[t * C];
    }
    __syncthreads();
    const int64_t te = t0 + kMmRows < T ? t0 + kMmRows : T;
    for (int64_t t = t0 > d ? t0 : d; t < te; ++t) {
      const int a = (int)(t % kMmRing), b = (int)((t - d) % kMmRing);
      const double X = (double)pv[a][lane], Y = (double)pv[b][lane], lx = lg[a][lane], ly = lg[b][lane];
      const double dl = __dsub_rn(lx, ly);
      s1 = __dadd_rn(s1, __dsub_rn(__dmul_rn(X, dl), __dmul_rn(Y, dl)));
      s2 = __dadd_rn(s2, __dmul_rn(X, __dsub_rn(lx, Y)));
    }
    __syncthreads();
  }
  // the tile's columns, ascending, by lane 0 of each wave (the ring is free: reuse its first rows)
  lg[2 * w][lane] = s1;
  lg[2 * w + 1][lane] = s2;
  __syncthreads();
  if (lane == 0) {
    const int nc = C - tile * kMmTC < kMmTC ? C - tile * kMmTC : kMmTC;
    double a1 = 0.0, a2 = 0.0;
    for (int j = 0; j < nc; ++j) {
      a1 = __dadd_rn(a1, lg[2 * w][j]);
      a2 = __dadd_rn(a2, lg[2 * w + 1][j]);
    }
    double* o = part + (((int64_t)u * gridDim.z + m) * n_tiles + tile) * (2 * kMmLags);
    o[2 * w] = a1;
    o[2 * w + 1] = a2;
  }
}

// one thread per (utterance, model): the tiles ascending, then the four lags
__global__ void mmeasure_finish_kernel(const double* __restrict__ part, const int64_t* __restrict__ utt_len, int n_utt,
                                       int D, int n_tiles, int C, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_utt * D) return;
  const int64_t T = utt_len[i / D];
  const double* p = part + i * n_tiles * (2 * kMmLags);
  double acc = 0.0;
  for (int k = 0; k < kMmLags; ++k) {
    double a1 = 0.0, a2 = 0.0;
    for (int tl = 0; tl < n_tiles; ++tl) {
      a1 = __dadd_rn(a1, p[tl * 2 * kMmLags + 2 * k]);
      a2 = __dadd_rn(a2, p[tl * 2 * kMmLags + 2 * k + 1]);
    }
    const double n = T > kMmLag[k] ? (double)(T - kMmLag[k]) : 0.0;
    acc = __dadd_rn(acc, __dadd_rn(__ddiv_rn(a1, n), __ddiv_rn(a2, __dmul_rn(n, (double)C))));
  }
  out[i] = __ddiv_rn(acc, (double)kMmLags);
}

int mmeasure_tiles(int C) { return (C + kMmTC - 1) / kMmTC; }

hipError_t launch_mmeasure(const float* post, int D, int64_t n_rows, int C, int n_utt, const int64_t* row_off,
                           const int64_t* utt_len, double* part, double* out, hipStream_t s) {
  if (n_utt <= 0) return hipSuccess;
  if (D < 1 || C < 1 || n_rows < 0 || n_utt > 65535 || D > 65535 || !post || !row_off || !utt_len || !part || !out)
    return hipErrorInvalidValue;
  const int nt = mmeasure_tiles(C);
  hipLaunchKernelGGL(mmeasure_kernel, dim3((unsigned)nt, (unsigned)n_utt, (unsigned)D), dim3(kMmThreads), 0, s, post,
                     n_rows, C, row_off, utt_len, nt, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t n = (int64_t)n_utt * D;
  hipLaunchKernelGGL(mmeasure_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, utt_len, n_utt,
                     D, nt, C, out);
  return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------------------
// vae_sample_kernel: z[r][j] = mu + expf(sigma) eps, float32, the product and the sum each rounded, as torch's
// latent[0] + torch.exp(latent[1]) * noise.  ml [rows, 2 bn] holds mu in columns 0 .. bn - 1 and sigma after it
// (the encoder's `means` stacked on `vars`).
// -----------------------------------------------------------------------------------------------------------
__global__ void vae_sample_kernel(const float* __restrict__ ml, const float* __restrict__ eps, float* __restrict__ z,
                                  int64_t n, int bn) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = i / bn;
  const int j = (int)(i - r * bn);
  const float mu = ml[r * 2 * bn + j], sg = ml[r * 2 * bn + bn + j];
  z[i] = __fadd_rn(mu, __fmul_rn(expf(sg), eps[i]));
}

hipError_t launch_vae_sample(const float* ml, const float* eps, float* z, int64_t rows, int bn, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (bn < 1 || !ml || !eps || !z) return hipErrorInvalidValue;
  const int64_t n = rows * bn, nb = (n + 255) / 256;
  if (nb > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vae_sample_kernel, dim3((unsigned)nb), dim3(256), 0, s, ml, eps, z, n, bn);
  return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------------------
// vae_elbo_kernel: one wave per row r of x, xhat [rows, K] and ml [rows, 2 bn], all float32, every operation float64:
//     a = sum_k (-0.5 (x - xhat)^2 - 0.5 log(2 pi)),   b = sum_j (1 - mu^2 - exp(sigma)^2 + 2 sigma)
//     elbo[r] = float32( a / K + 0.5 (b / bn) )
// a lane adds its k = lane, lane + 64, .. ascending; the 64 lanes are added by the xor butterfly 32, 16, .. 1 (each
// step adds two partners, so every lane holds the same bits).  The order depends on K and bn alone.
// vae_px_kernel: one thread per utterance, t ascending in float64: mean_t elbo (mode 0) or mean_t expf(elbo) (mode 1),
// written at out[u ld]; T = 0 gives 0 / 0.
// -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double life_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(256) void vae_elbo_kernel(const float* __restrict__ x, const float* __restrict__ xh,
                                                       const float* __restrict__ ml, float* __restrict__ elbo,
                                                       int64_t rows, int K, int bn) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const double kHalfLog2Pi = 0.5 * 1.8378770664093453;  // 0.5 * np.log(2 * np.pi * 1)
  double a = 0.0, b = 0.0;
  for (int k = lane; k < K; k += 64) {
    const double e = __dsub_rn((double)x[r * K + k], (double)xh[r * K + k]);
    a = __dadd_rn(a, __dsub_rn(__dmul_rn(-0.5, __dmul_rn(e, e)), kHalfLog2Pi));
  }
  for (int j = lane; j < bn; j += 64) {
    const double mu = (double)ml[r * 2 * bn + j], sg = (double)ml[r * 2 * bn + bn + j], ex = exp(sg);
    b = __dadd_rn(b, __dadd_rn(__dsub_rn(__dsub_rn(1.0, __dmul_rn(mu, mu)), __dmul_rn(ex, ex)), __dmul_rn(2.0, sg)));
  }
  a = life_wave_sum(a);
  b = life_wave_sum(b);
  if (lane == 0)
    elbo[r] = (float)__dadd_rn(__ddiv_rn(a, (double)K), __dmul_rn(0.5, __ddiv_rn(b, (double)bn)));
}

__global__ void vae_px_kernel(const float* __restrict__ elbo, int64_t n_rows, const int64_t* __restrict__ row_off,
                              const int64_t* __restrict__ utt_len, int n_utt, int mode, double* __restrict__ out,
                              int ld) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_utt) return;
  const int64_t T = utt_len[u], r0 = row_off[u];
  FDLP_CHECK(T >= 0 && r0 >= 0 && r0 + T <= n_rows);
  double s = 0.0;
  for (int64_t t = 0; t < T; ++t) {
    const float e = elbo[r0 + t];
    s = __dadd_rn(s, (double)(mode ? expf(e) : e));
  }
  out[(int64_t)u * ld] = __ddiv_rn(s, (double)T);
}

hipError_t launch_vae_elbo(const float* x, const float* xh, const float* ml, float* elbo, int64_t rows, int K, int bn,
                           int n_utt, const int64_t* row_off, const int64_t* utt_len, int mode, double* out, int ld,
                           hipStream_t s) {
  if (K < 1 || bn < 1 || ld < 1 || (mode != 0 && mode != 1)) return hipErrorInvalidValue;
  if (rows > 0) {
    if (!x || !xh || !ml || !elbo) return hipErrorInvalidValue;
    const int64_t nb = (rows + 3) / 4;
    if (nb > (int64_t)INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vae_elbo_kernel, dim3((unsigned)nb), dim3(256), 0, s, x, xh, ml, elbo, rows, K, bn);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (n_utt <= 0) return hipSuccess;
  if (!row_off || !utt_len || !out || !elbo) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vae_px_kernel, dim3((unsigned)((n_utt + 255) / 256)), dim3(256), 0, s, elbo, rows, row_off,
                     utt_len, n_utt, mode, out, ld);
  return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------------------
// lifelong_fuse_kernel.  post [D, n_rows, C] float32, w [n_utt, D] float64, tab [D, C] float64, all arithmetic
// float64, i ascending from 0.0, the result rounded to float32 once; IEEE special values as they fall:
//   mode 0 (lifelong)     out[t][c] = log(sum_i P_i[t][c] w[u][i]) - pw log(sum_i tab_i[c] w[u][i]),  tab = exp(prior)
//   mode 1 (incremental)  out[t][c] = (sum_i (log P_i[t][c] - pw tab_i[c]) w[u][i]) / D,              tab = prior
// A workgroup owns (4 kFuThreads columns, kFuRows rows of one utterance); a thread owns 4 adjacent columns, loads
// them as one float4 per model and row when C % 4 == 0 and the base is 16-byte aligned, and keeps what depends on
// (u, c) alone -- the second logarithm, or pw tab_i[c] -- in registers across its rows.
// -----------------------------------------------------------------------------------------------------------
constexpr int kFuThreads = 256, kFuRows = 64, kFuMaxD = 8;

template <bool VEC, int MODE>
__global__ __launch_bounds__(kFuThreads) void lifelong_fuse_kernel(const float* __restrict__ post, int D, int64_t n_rows,
                                                                   int C, const int64_t* __restrict__ row_off,
                                                                   const int64_t* __restrict__ utt_len,
                                                                   const double* __restrict__ w,
                                                                   const double* __restrict__ tab, double pw,
                                                                   int n_cchunks, float* __restrict__ out) {
  const int u = blockIdx.x / n_cchunks, cc = blockIdx.x - u * n_cchunks;
  const int64_t T = utt_len[u], r0 = row_off[u];
  FDLP_CHECK(T >= 0 && r0 >= 0 && r0 + T <= n_rows);
  const int64_t tb = (int64_t)blockIdx.y * kFuRows;
  if (tb >= T) return;
  const int64_t te = tb + kFuRows < T ? tb + kFuRows : T;
  const int c0 = (cc * kFuThreads + threadIdx.x) * 4;
  if (c0 >= C) return;
  const int nc = C - c0 < 4 ? C - c0 : 4;
  double wi[kFuMaxD];
#pragma unroll
  for (int i = 0; i < kFuMaxD; ++i) wi[i] = i < D ? w[(int64_t)u * D + i] : 0.0;
  double sub[4] = {0.0, 0.0, 0.0, 0.0};  // mode 0: pw log(sum_i E_i[c] w_i)
  double pt[MODE == 1 ? kFuMaxD : 1][4];   // mode 1: pw prior_i[c]
  if (MODE == 1) {
#pragma unroll
    for (int i = 0; i < kFuMaxD; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pt[MODE == 1 ? i : 0][j] = i < D && j < nc ? __dmul_rn(pw, tab[(int64_t)i * C + c0 + j]) : 0.0;
  }
  if (MODE == 0) {
    for (int j = 0; j < nc; ++j) {
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < kFuMaxD; ++i)
        if (i < D) a = __dadd_rn(a, __dmul_rn(tab[(int64_t)i * C + c0 + j], wi[i]));
      sub[j] = __dmul_rn(pw, log(a));
    }
  }
  for (int64_t t = tb; t < te; ++t) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < kFuMaxD; ++i) {
      if (i >= D) break;
      const float* p = post + ((int64_t)i * n_rows + r0 + t) * C + c0;
      float v[4] = {1.f, 1.f, 1.f, 1.f};
      if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        for (int j = 0; j < nc; ++j) v[j] = p[j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (MODE == 0) {
          acc[j] = __dadd_rn(acc[j], __dmul_rn((double)v[j], wi[i]));
        } else {
          acc[j] = __dadd_rn(acc[j], __dmul_rn(__dsub_rn(log((double)v[j]), pt[MODE == 1 ? i : 0][j]), wi[i]));
        }
      }
    }
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      r[j] = MODE == 0 ? (float)__dsub_rn(log(acc[j]), sub[j]) : (float)__ddiv_rn(acc[j], (double)D);
    float* o = out + (r0 + t) * C + c0;
    if (VEC) {
      *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
      for (int j = 0; j < nc; ++j) o[j] = r[j];
    }
  }
}

hipError_t launch_lifelong_fuse(const float* post, int D, int64_t n_rows, int C, int n_utt, int64_t max_len,
                                const int64_t* row_off, const int64_t* utt_len, const double* w, const double* tab,
                                double pw, int mode, float* out, hipStream_t s) {
  if (n_utt <= 0 || max_len <= 0) return hipSuccess;
  if (D < 1 || D > kFuMaxD || C < 1 || n_rows < 0 || (mode != 0 && mode != 1) || !post || !row_off || !utt_len || !w ||
      !tab || !out)
    return hipErrorInvalidValue;
  const int ncc = (C + 4 * kFuThreads - 1) / (4 * kFuThreads);
  const int64_t gx = (int64_t)ncc * n_utt, gy = (max_len + kFuRows - 1) / kFuRows;
  if (gx > (int64_t)INT32_MAX || gy > 65535) return hipErrorInvalidValue;
  const bool vec = C % 4 == 0 && (((uintptr_t)post | (uintptr_t)out) & 15u) == 0;
  const dim3 g((unsigned)gx, (unsigned)gy), b(kFuThreads);
#define FDLP_FUSE_LAUNCH(VEC, MODE)                                                                                 \
  hipLaunchKernelGGL((lifelong_fuse_kernel<VEC, MODE>), g, b, 0, s, post, D, n_rows, C, row_off, utt_len, w, tab, \
                     pw, ncc, out)
  if (mode == 0) {
    if (vec) FDLP_FUSE_LAUNCH(true, 0);
    else FDLP_FUSE_LAUNCH(false, 0);
  } else {
    if (vec) FDLP_FUSE_LAUNCH(true, 1);
    else FDLP_FUSE_LAUNCH(false, 1);
  }
#undef FDLP_FUSE_LAUNCH
  return hipGetLastError();
}

}  // namespace fdlp
