// fdlp_vaeenc.hip -- gfx950 kernels of the VAE-encoded GRU models (src/nnet/compute_vae_encoded_likelihood.py):
//   conv2d_same_kernel  one same-padded nn.Conv2d of VAECNNEncoderNopool over the (feature x time) image of an
//                       utterance, float32, an implicit GEMM on v_mfma_f32_32x32x2_f32
//   utt_norm_kernel     the per-utterance mean / unbiased-variance normaliser of the latent (:128-129)
// Everything else of those models (the GRU encoder, `means`, the GRU classifier, the regression, the output modes)
// is fdlp_nnet.hip's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fdlp_device.h"
#include "fdlp_internal.h"

namespace fdlp {

// -----------------------------------------------------------------------------------------------------------
// conv2d_same_kernel.  Rows are [t][c F + f], channel-major, for the input (Ci channels) and the output (Co):
//     out[t][co F + f] = b[co] + sum_{ci, dh, dw} g(in[t + dw - pw][ci F + f + dh - ph]) W[co][ci][dh][dw]
// ph = (kh - 1) / 2, pw = (kw - 1) / 2, g the identity or max(x, 0) (ReLU on load: a layer stores its
// pre-activation); a tap outside 0 <= f' < F or outside the UTTERANCE's 0 <= t' < T is zero -- the rows of the
// neighbouring utterances of the batch are never read as data.
//
// It is dense_kernel (fdlp_nnet.hip) with another source for the A chunk.  GEMM rows are the positions
// p = t F + f of one utterance, 0 <= p < T F; a workgroup owns the kDenseTM = 128 positions p0 .. p0 + 127 of a
// ConvTile (the host lists the tiles of every utterance, as it does the PostTiles of the splice) and 64 NT output
// channels, and walks K = Ci kh kw in chunks of kDenseKC, k being the flat index of W[co] in torch's layout
// (ci, dh, dw).  So W is dense_kernel's W [Co, K], staged the same way, and the MFMA loop, the lane maps and the
// chain are dense_kernel's: for every output, from acc = +0,
//     for g = 0, 8, 16, .. < ceil(K / 32) 32:   for i = 0 .. 3:   k = g + i,  then  k = g + 4 + i
// acc = fmaf(a_k, W[co][k], acc) with a_k the tap of k (a padded tap is a SELECTED +0, as in dense_kernel on an
// im2col row with zeros there; a k >= K contributes fmaf(+0, +0, acc)), and the bias is one float32 add at the
// end.  An output's bits are those of dense_kernel on the im2col rows, and depend on the layer's shape alone: not
// on the tile, on the utterance's place in the batch, nor on the batch.
//
// The A chunk is gathered from the tile's input patch, which lies in LDS for the whole K loop:
//     patch[j][ci][fp],  j = 0 .. NFR - 1 the frames t_first - pw + j (t_first = p0 / F),  fp = 0 .. F + kh - 2
// holding g(in[t'][ci F + fp - ph]) or zero where t' or fp - ph falls outside (both paddings are in the patch, so
// the gather has no condition but k < K).  NFR = (kDenseTM - 1) / F + kw + 1 frames cover every tile.  The tap of
// (position m, k) is patch[base(m) + koff[k]] with base(m) = (t_m - t_first) Ci FP + f_m and the shape-only table
// koff[k] = dw Ci FP + ci FP + dh, built by the host and copied to LDS.  A thread stages the same 4 x 4 floats of
// the A chunk as in dense_kernel: one 16-byte read of koff, sixteen 4-byte reads of the patch, four 16-byte
// writes; they issue between the two MFMA halves of the previous chunk, like dense_kernel's selects.
// Positions past the utterance gather position T F - 1 and are not stored.
// -----------------------------------------------------------------------------------------------------------
constexpr int kConvThreads = 256;
constexpr int kConvS = kDenseKC + 4;  // floats between rows of a staged chunk
static_assert(kDenseTM == 128 && kDenseKC == 32, "the staging maps of conv2d_same_kernel are dense_kernel's");

typedef float ve_f4 __attribute__((ext_vector_type(4)));
typedef int ve_i4 __attribute__((ext_vector_type(4)));
typedef float ve_f16 __attribute__((ext_vector_type(16)));

int conv_patch_frames(int F, int kw) { return (kDenseTM - 1) / F + kw + 1; }
static int conv_kpad(int K) { return (K + kDenseKC - 1) / kDenseKC * kDenseKC; }
static size_t conv_patch_floats(int F, int Ci, int kh, int kw) {
  return ((size_t)conv_patch_frames(F, kw) * Ci * (F + kh - 1) + 3) / 4 * 4;
}
size_t conv_lds_bytes(int F, int Ci, int Co, int kh, int kw) {
  return sizeof(float) * ((size_t)conv_kpad(Ci * kh * kw) + conv_patch_floats(F, Ci, kh, kw)) + dense_lds_bytes(Co);
}
void conv_koff_table(int F, int Ci, int kh, int kw, int32_t* koff) {
  const int FP = F + kh - 1, K = Ci * kh * kw, KP = conv_kpad(K);
  for (int k = 0; k < KP; ++k) {
    const int ci = k / (kh * kw), dh = k % (kh * kw) / kw, dw = k % kw;
    koff[k] = k < K ? dw * Ci * FP + ci * FP + dh : 0;
  }
}

template <bool VEC>
__device__ __forceinline__ ve_f4 conv_load4(const float* __restrict__ p, int k, int K) {
  if (VEC) return *(const ve_f4*)(p + min(k, K - 4));
  ve_f4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = p[min(k + j, K - 1)];
  return v;
}

template <int NT, bool VEC>
__global__ __launch_bounds__(kConvThreads) void conv2d_same_kernel(const float* __restrict__ in,
                                                                   const float* __restrict__ W,
                                                                   const float* __restrict__ bias,
                                                                   float* __restrict__ out,
                                                                   const ConvTile* __restrict__ tiles,
                                                                   const int32_t* __restrict__ koff_g, int64_t rows,
                                                                   const ConvConsts c, int nct, int relu) {
  constexpr int TN = 64 * NT;
  constexpr int AF = kDenseTM * kConvS, BUF = AF + TN * kConvS;  // floats of the A chunk, of one buffer
  constexpr int NA = kDenseTM * (kDenseKC / 4) / kConvThreads;   // 16-byte pieces of the A chunk per thread: 4
  constexpr int NW = TN * (kDenseKC / 4) / kConvThreads;         // and of the W chunk: 2 NT
  extern __shared__ float4 conv_sh4[];
  const int F = c.F, Ci = c.Ci, Co = c.Co, K = c.K, KP = c.KP;
  const int FP = F + c.kh - 1, CFP = Ci * FP, ph = (c.kh - 1) / 2, pw = (c.kw - 1) / 2;
  int* koff = (int*)conv_sh4;                 // [KP]
  float* patch = (float*)conv_sh4 + KP;       // [NFR][Ci][FP]
  float* sh = patch + c.patch_floats;         // dense_kernel's two chunk buffers
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, h = lane >> 5;
  const ConvTile tl = tiles[blockIdx.x / nct];
  const int n0 = (int)(blockIdx.x % nct) * TN;
  const int T = tl.T, p0 = tl.p0, PT = T * F, t_first = p0 / F;
  FDLP_CHECK(T >= 1 && (int64_t)T * F <= INT32_MAX && p0 >= 0 && p0 < PT && p0 % kDenseTM == 0 && tl.row0 >= 0 &&
             tl.row0 + T <= rows && n0 < Co && K == Ci * c.kh * c.kw && KP % kDenseKC == 0 && KP >= K &&
             c.NFR == (kDenseTM - 1) / F + c.kw + 1 && (!VEC || (K >= 4 && K % 4 == 0)));

  for (int i = tid; i < KP; i += kConvThreads) koff[i] = koff_g[i];
  // the patch: every load is unconditional, from a row and a column clamped into the utterance, and the zeros of
  // both paddings are SELECTED as the value is written
  for (int j = 0; j < c.NFR; ++j) {
    const int tt = t_first - pw + j;
    const bool inu = tt >= 0 && tt < T;
    const int64_t r = tl.row0 + min(max(tt, 0), T - 1);
    FDLP_CHECK(r >= 0 && r < rows);
    const float* src = in + r * ((int64_t)Ci * F);
    for (int idx = tid; idx < CFP; idx += kConvThreads) {
      const int ci = idx / FP, f = idx - ci * FP - ph;
      FDLP_CHECK(ci < Ci && j * CFP + idx < c.patch_floats);
      float v = src[ci * F + min(max(f, 0), F - 1)];
      if (relu) v = fmaxf(v, 0.f);
      patch[j * CFP + idx] = inu && f >= 0 && f < F ? v : 0.f;
    }
  }

  // staging map (dense_kernel's): piece i of this thread is row sr + 32 i of the chunk, floats 4 sq .. 4 sq + 3
  const int sr = tid >> 3, sq = tid & 7;
  int abase[NA];
  const float* wp[NW];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int p = min(p0 + sr + 32 * i, PT - 1), t = p / F;
    abase[i] = (t - t_first) * CFP + (p - t * F);
    FDLP_CHECK(t >= t_first && t - t_first + c.kw - 1 < c.NFR);
  }
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int n = min(n0 + sr + 32 * i, Co - 1);
    FDLP_CHECK(n >= 0 && n < Co);
    wp[i] = W + (size_t)n * K;
  }
  ve_f4 pwr[NW];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) pwr[i] = conv_load4<VEC>(wp[i], k0 + 4 * sq, K);
  };

  ve_f16 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mt][nt][e] = 0.f;

  // a wave none of whose positions or channels exist only helps with the staging
  const bool act = p0 + wr * 64 < PT && n0 + wc * 32 * NT < Co;
  const int arow = (wr * 64 + l31) * kConvS + 4 * h;
  const int wrow = AF + (wc * 32 * NT + l31) * kConvS + 4 * h;

  // the chunk at k0 -> buffer S: the A pieces gathered from the patch, the W pieces from the fetched registers;
  // the zeros at k >= K and n >= Co are selected here
  auto stage = [&](float* S, int k0) {
    const int k = k0 + 4 * sq;
    FDLP_CHECK(k >= 0 && k + 3 < KP);
    const ve_i4 ko = *(const ve_i4*)(koff + k);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int at = (sr + 32 * i) * kConvS + 4 * sq;
      FDLP_CHECK(at >= 0 && at + 3 < AF);
      ve_f4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        FDLP_CHECK(abase[i] + ko[e] >= 0 && abase[i] + ko[e] < c.patch_floats);
        const float x = patch[abase[i] + ko[e]];
        v[e] = k + e < K ? x : 0.f;
      }
      *(ve_f4*)(S + at) = v;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int at = AF + (sr + 32 * i) * kConvS + 4 * sq;
      FDLP_CHECK(at >= AF && at + 3 < BUF);
      ve_f4 v = pwr[i];
      const bool keep = n0 + sr + 32 * i < Co;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = keep && (VEC ? k : k + e) < K ? v[e] : 0.f;
      *(ve_f4*)(S + at) = v;
    }
  };
  auto burst = [&](const float* S, int g0, int g1) {
#pragma unroll
    for (int g = g0; g < g1; ++g) {
      ve_f4 a[2], w[NT];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        FDLP_CHECK(arow + mt * 32 * kConvS + 8 * g + 3 < AF);
        a[mt] = *(const ve_f4*)(S + arow + mt * 32 * kConvS + 8 * g);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        FDLP_CHECK(wrow + nt * 32 * kConvS + 8 * g + 3 < BUF);
        w[nt] = *(const ve_f4*)(S + wrow + nt * 32 * kConvS + 8 * g);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][i], w[nt][i], acc[mt][nt], 0, 0, 0);
    }
  };

  // dense_kernel's loop: chunk c out of buffer c & 1 in two halves, chunk c + 1 staged between them, one barrier
  // per chunk.  The first stage gathers from koff and the patch itself, so a barrier of its own publishes them
  // before it; the one after it publishes chunk 0.
  fetch(0);
  __syncthreads();
  stage(sh, 0);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += kDenseKC, buf ^= 1) {
    const float* S = sh + buf * BUF;
    const bool more = k0 + kDenseKC < K;
    if (more) fetch(k0 + kDenseKC);
    if (act) burst(S, 0, kDenseKC / 16);
    __builtin_amdgcn_sched_barrier(0);
    if (more) stage(sh + (buf ^ 1) * BUF, k0 + kDenseKC);
    __builtin_amdgcn_sched_barrier(0);
    if (act) burst(S, kDenseKC / 16, kDenseKC / 8);
    __syncthreads();
  }
  if (!act) return;
  // results: the lane holds channel l31 of positions (e & 3) + 8 (e >> 2) + 4 h of each 32 x 32 tile
  const int64_t CoF = (int64_t)Co * F;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + (wc * NT + nt) * 32 + l31;
    if (n >= Co) continue;
    const float bn = bias[n];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int p = p0 + wr * 64 + mt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (p >= PT) continue;
        const int t = p / F, f = p - t * F;
        FDLP_CHECK(t >= 0 && t < T && f >= 0 && f < F && tl.row0 + t < rows);
        out[(tl.row0 + t) * CoF + (int64_t)n * F + f] = __fadd_rn(acc[mt][nt][e], bn);
      }
    }
  }
}

hipError_t launch_conv2d_same(const float* in, const float* W, const float* bias, float* out, const ConvTile* tiles,
                              int ntiles, const int32_t* koff, int64_t rows, int F, int Ci, int Co, int kh, int kw,
                              int relu, hipStream_t s) {
  if (ntiles <= 0 || rows <= 0) return hipSuccess;
  if (F < 1 || Ci < 1 || Co < 1 || kh < 1 || kw < 1 || kh % 2 == 0 || kw % 2 == 0) return hipErrorInvalidValue;
  const size_t lds = conv_lds_bytes(F, Ci, Co, kh, kw);
  if (lds > 163840) return hipErrorInvalidValue;
  ConvConsts c{};
  c.F = F; c.Ci = Ci; c.Co = Co; c.kh = kh; c.kw = kw;
  c.K = Ci * kh * kw; c.KP = conv_kpad(c.K); c.NFR = conv_patch_frames(F, kw);
  c.patch_floats = (int)conv_patch_floats(F, Ci, kh, kw);
  const int tn = dense_col_tile(Co);
  const int64_t nct = (Co + tn - 1) / tn;
  if (nct * ntiles > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  const bool vec = c.K % 4 == 0 && ((uintptr_t)W & 15u) == 0;
#define FDLP_CONV_LAUNCH(NT, VEC)                                                                                  \
  do {                                                                                                             \
    if (lds > 65536)                                                                                               \
      (void)hipFuncSetAttribute((const void*)conv2d_same_kernel<NT, VEC>,                                          \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                             \
    hipLaunchKernelGGL((conv2d_same_kernel<NT, VEC>), dim3((unsigned)(nct * ntiles)), dim3(kConvThreads), lds, s,  \
                       in, W, bias, out, tiles, koff, rows, c, (int)nct, relu);                                    \
  } while (0)
  if (tn == 64) {
    if (vec) FDLP_CONV_LAUNCH(1, true);
    else FDLP_CONV_LAUNCH(1, false);
  } else {
    if (vec) FDLP_CONV_LAUNCH(2, true);
    else FDLP_CONV_LAUNCH(2, false);
  }
#undef FDLP_CONV_LAUNCH
  return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------------------
// utt_norm_kernel: compute_vae_encoded_likelihood.py:128-129 on the latent z [rows, D].  One thread owns column d
// of utterance u (a GruSlot: rows row0 .. row0 + T - 1; an empty slot has T = 0) and walks t in ascending order
// three times:
//     m     = float32( (sum_t z_t in float64) / T )
//     d_t   = z_t - m                                     float32
//     v     = float32( (sum_t (d_t - md)^2 in float64) / (T - 1) ),   md = (sum_t d_t in float64) / T
//     out_t = d_t / sqrtf(v)                              sqrt and division correctly rounded
// every float64 operation rounded as written (no contraction).  The order depends on T alone.  T = 1 gives 0 / 0,
// a constant column d / 0: what IEEE gives, as torch does; there is no special case.  in == out is allowed (a
// thread reads z_t before it writes out_t, and no other thread touches the element).
// -----------------------------------------------------------------------------------------------------------
constexpr int kNormThreads = 256;

__global__ __launch_bounds__(kNormThreads) void utt_norm_kernel(const float* in, float* out,
                                                                const GruSlot* __restrict__ slots, int n_slots,
                                                                int64_t rows, int D) {
  const int64_t gid = (int64_t)blockIdx.x * kNormThreads + threadIdx.x;
  const int64_t u = gid / D;
  if (u >= n_slots) return;
  const int d = (int)(gid - u * D);
  const GruSlot sl = slots[u];
  FDLP_CHECK(sl.len >= 0 && sl.row0 >= 0 && sl.row0 + sl.len <= rows);
  const int T = sl.len;
  if (T <= 0) return;
  const float* z = in + sl.row0 * D + d;
  float* o = out + sl.row0 * D + d;
  double s = 0.0;
  for (int t = 0; t < T; ++t) s = __dadd_rn(s, (double)z[(int64_t)t * D]);
  const float m = (float)__ddiv_rn(s, (double)T);
  double sd = 0.0;
  for (int t = 0; t < T; ++t) sd = __dadd_rn(sd, (double)__fsub_rn(z[(int64_t)t * D], m));
  const double md = __ddiv_rn(sd, (double)T);
  double ss = 0.0;
  for (int t = 0; t < T; ++t) {
    const double e = __dsub_rn((double)__fsub_rn(z[(int64_t)t * D], m), md);
    ss = __dadd_rn(ss, __dmul_rn(e, e));
  }
  const float sdv = __fsqrt_rn((float)__ddiv_rn(ss, (double)(T - 1)));
  for (int t = 0; t < T; ++t) {
    FDLP_CHECK(sl.row0 + t < rows);
    o[(int64_t)t * D] = __fdiv_rn(__fsub_rn(z[(int64_t)t * D], m), sdv);
  }
}

hipError_t launch_utt_norm(const float* in, float* out, const GruSlot* slots, int n_slots, int64_t rows, int D,
                           hipStream_t s) {
  if (n_slots <= 0 || rows <= 0) return hipSuccess;
  if (D < 1 || !in || !out || !slots) return hipErrorInvalidValue;
  const int64_t nb = ((int64_t)n_slots * D + kNormThreads - 1) / kNormThreads;
  if (nb > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(utt_norm_kernel, dim3((unsigned)nb), dim3(kNormThreads), 0, s, in, out, slots, n_slots, rows, D);
  return hipGetLastError();
}

hipError_t checks_vaeenc(unsigned int* v, bool reset) { return fdlp_checks_local(v, reset); }

}  // namespace fdlp
