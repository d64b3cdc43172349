// fdlp_nnet.hip -- gfx950 kernels of the feed-forward acoustic model the hybrid recipes run on the spliced rows
// (src/nnet/nnet_models.py nnetFeedforward: nn.Linear layers with ReLU between them; extract_posterior.py):
//   dense_kernel         out[r][n] = sum_k f(A[r][k]) W[n][k] + b[n], f the identity or max(x, 0), float32
//   row_epilogue_kernel  softmax or log-likelihood of a row of logits, in place
// Layer 0 is not here: it is xform_kernel (fdlp_post.hip) with the layer's weights and bias as an affine transform.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fdlp_device.h"
#include "fdlp_internal.h"

namespace fdlp {

// -----------------------------------------------------------------------------------------------------------
// dense_kernel: one workgroup of four waves owns a kDenseTM x TN tile of the output (TN = 64 NT, NT = 1 or 2) and
// walks K in chunks of kDenseKC columns.  A chunk of A (kDenseTM rows) and of W (TN rows) lies in LDS as
// [row][kDenseKC + 4] floats: the 144-byte row stride puts the 16 rows a ds_read_b128 lane group reads on 16
// different 16-byte slots of the bank row.  Two such buffers: the next chunk's global loads are issued before the
// current chunk's MFMAs, land in registers during the first half of them, are written to the other buffer between
// the halves, and one barrier per chunk separates a buffer's writers from its readers (the loop at the bottom).
//
// The waves form a 2 x 2 grid; a wave owns 64 rows x 32 NT columns as 2 x NT tiles of v_mfma_f32_32x32x2_f32
// (exact float32; 16 accumulator registers per tile, so 64 or 32 AGPRs).  Lane l = 32 h + i of that instruction
// supplies A[row i][k_h] and W[col i][k_h] for the two k of the step, and the result is the fmaf chain over k_0 then
// k_1.  A lane half h owns four CONSECUTIVE k of every group of eight (one 16-byte LDS read), so the chain of
// every out[r][n] is, from acc = +0,
//     for g = 0, 8, 16, .. < ceil(K / 32) 32:   for i = 0 .. 3:   k = g + i,  then  k = g + 4 + i
// with acc = fmaf(f(A[r][k]), W[n][k], acc), one rounding per k; a k >= K contributes fmaf(+0, +0, acc) (both
// operands are SELECTED to zero as the chunk is staged; nothing is multiplied by what lies past a row), and the
// bias is one float32 add at the end.  The order is a function of K alone: not of the row, of its tile, of N, of
// NT, nor of what else is in the launch.
//   * rows past the batch read row `rows - 1` and are not stored; columns n >= N are zero in LDS and not stored;
//   * with K a multiple of 4 and 16-byte aligned pointers the chunks are loaded 16 bytes per lane (eight lanes
//     read one row's 128-byte chunk; VEC), otherwise element by element; every load is unconditional, from an
//     address clamped into the row, and the zeros are selected when the registers are written to LDS.
// -----------------------------------------------------------------------------------------------------------
constexpr int kDenseThreads = 256;
constexpr int kDenseS = kDenseKC + 4;  // floats between rows of a staged chunk
static_assert(kDenseTM == 128 && kDenseKC == 32 && kDenseThreads == 256, "the staging maps of dense_kernel");

typedef float nn_f4 __attribute__((ext_vector_type(4)));
typedef float nn_f16 __attribute__((ext_vector_type(16)));

int dense_col_tile(int N) { return N <= 64 ? 64 : kDenseTN; }
size_t dense_lds_bytes(int N) { return sizeof(float) * 2 * (size_t)(kDenseTM + dense_col_tile(N)) * kDenseS; }

// Four floats k .. k + 3 of a row p, loaded UNCONDITIONALLY from clamped addresses (a load behind a per-element branch
// is waited for on the spot, one L2 round trip each); dense_select4 zeroes what lies at k >= K when the chunk is
// written to LDS, after the previous chunk's MFMAs.  VEC: K is a multiple of 4 (so K >= 4) and p is 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ nn_f4 dense_load4(const float* __restrict__ p, int k, int K) {
  if (VEC) return *(const nn_f4*)(p + min(k, K - 4));
  nn_f4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = p[min(k + j, K - 1)];
  return v;
}

template <bool VEC>
__device__ __forceinline__ nn_f4 dense_select4(nn_f4 v, int k, int K, bool keep) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = keep && (VEC ? k : k + j) < K ? v[j] : 0.f;
  return v;
}

template <int NT, bool VEC>
__global__ __launch_bounds__(kDenseThreads) void dense_kernel(const float* __restrict__ A,
                                                              const float* __restrict__ W,
                                                              const float* __restrict__ bias,
                                                              float* __restrict__ out, int64_t rows, int K, int N,
                                                              int nct, int relu) {
  constexpr int TN = 64 * NT;
  constexpr int AF = kDenseTM * kDenseS, BUF = AF + TN * kDenseS;  // floats of the A chunk, of one buffer
  constexpr int NA = kDenseTM * (kDenseKC / 4) / kDenseThreads;    // 16-byte pieces of the A chunk per thread: 4
  constexpr int NW = TN * (kDenseKC / 4) / kDenseThreads;          // and of the W chunk: 2 NT
  extern __shared__ float4 dense_sh4[];
  float* sh = (float*)dense_sh4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, h = lane >> 5;
  const int64_t row0 = (int64_t)(blockIdx.x / nct) * kDenseTM;
  const int n0 = (int)(blockIdx.x % nct) * TN;
  FDLP_CHECK(row0 < rows && n0 < N && K >= 1 && (!VEC || (K >= 4 && K % 4 == 0)));

  // staging map: piece i of this thread is row sr + 32 i of the chunk, floats 4 sq .. 4 sq + 3; rows past the
  // batch read its last row, columns past N read row N - 1 of W
  const int sr = tid >> 3, sq = tid & 7;
  const float* ap[NA];
  const float* wp[NW];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int64_t r = min(row0 + sr + 32 * i, rows - 1);
    FDLP_CHECK(r >= 0 && r < rows);
    ap[i] = A + r * K;
  }
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int n = min(n0 + sr + 32 * i, N - 1);
    FDLP_CHECK(n >= 0 && n < N);
    wp[i] = W + (size_t)n * K;
  }
  nn_f4 pa[NA], pw[NW];
  auto fetch = [&](int k0) {
    const int k = k0 + 4 * sq;
#pragma unroll
    for (int i = 0; i < NA; ++i) pa[i] = dense_load4<VEC>(ap[i], k, K);
#pragma unroll
    for (int i = 0; i < NW; ++i) pw[i] = dense_load4<VEC>(wp[i], k, K);
  };

  nn_f16 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mt][nt][e] = 0.f;

  // a wave none of whose rows or columns exist only helps with the staging
  const bool act = row0 + wr * 64 < rows && n0 + wc * 32 * NT < N;
  const int arow = (wr * 64 + l31) * kDenseS + 4 * h;            // this lane's A row of tile 0, its half's 4 floats
  const int wrow = AF + (wc * 32 * NT + l31) * kDenseS + 4 * h;  // and its W row of tile 0

  // the staged registers of the chunk at k0 -> buffer S: f, and zeros at k >= K and n >= N, are applied here
  auto stage = [&](float* S, int k0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int at = (sr + 32 * i) * kDenseS + 4 * sq;
      FDLP_CHECK(at >= 0 && at + 3 < AF);
      nn_f4 v = dense_select4<VEC>(pa[i], k0 + 4 * sq, K, true);
      if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      *(nn_f4*)(S + at) = v;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int at = AF + (sr + 32 * i) * kDenseS + 4 * sq;
      FDLP_CHECK(at >= AF && at + 3 < BUF);
      *(nn_f4*)(S + at) = dense_select4<VEC>(pw[i], k0 + 4 * sq, K, n0 + sr + 32 * i < N);
    }
  };
  // the MFMAs of the groups of eight k g0 .. g1 - 1 of the chunk in S
  auto burst = [&](const float* S, int g0, int g1) {
#pragma unroll
    for (int g = g0; g < g1; ++g) {
      nn_f4 a[2], w[NT];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        FDLP_CHECK(arow + mt * 32 * kDenseS + 8 * g + 3 < AF);
        a[mt] = *(const nn_f4*)(S + arow + mt * 32 * kDenseS + 8 * g);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        FDLP_CHECK(wrow + nt * 32 * kDenseS + 8 * g + 3 < BUF);
        w[nt] = *(const nn_f4*)(S + wrow + nt * 32 * kDenseS + 8 * g);
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

  // Chunk c is multiplied out of buffer c & 1 in two halves.  The loads of chunk c + 1 are issued before the first
  // half and its registers go to the other buffer between the halves, so that the selects, the ReLU and the LDS
  // writes issue in the shadow of MFMAs instead of in a phase of their own.  That buffer was last read in
  // iteration c - 1, which every wave left through the barrier that ends it; the barrier that ends this iteration
  // publishes the writes and retires this chunk's reads.  One barrier per chunk.
  fetch(0);
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
  // results: the lane holds column l31 of rows (e & 3) + 8 (e >> 2) + 4 h of each 32 x 32 tile
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + (wc * NT + nt) * 32 + l31;
    if (n >= N) continue;
    const float bn = bias[n];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t r = row0 + wr * 64 + mt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (r >= rows) continue;
        FDLP_CHECK(r >= 0 && n >= 0 && n < N);
        out[r * N + n] = __fadd_rn(acc[mt][nt][e], bn);
      }
    }
  }
}

hipError_t launch_dense(const float* A, const float* W, const float* bias, float* out, int64_t rows, int K, int N,
                        int relu, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const int tn = dense_col_tile(N);
  const int64_t nct = (N + tn - 1) / tn, nrt = (rows + kDenseTM - 1) / kDenseTM;
  if (nct * nrt > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  const bool vec = K % 4 == 0 && (((uintptr_t)A | (uintptr_t)W) & 15u) == 0;
  const size_t lds = dense_lds_bytes(N);
#define FDLP_DENSE_LAUNCH(NT, VEC)                                                                                \
  do {                                                                                                            \
    if (lds > 65536)                                                                                              \
      (void)hipFuncSetAttribute((const void*)dense_kernel<NT, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize,   \
                                (int)lds);                                                                        \
    hipLaunchKernelGGL((dense_kernel<NT, VEC>), dim3((unsigned)(nct * nrt)), dim3(kDenseThreads), lds, s, A, W,   \
                       bias, out, rows, K, N, (int)nct, relu);                                                    \
  } while (0)
  if (tn == 64) {
    if (vec) FDLP_DENSE_LAUNCH(1, true);
    else FDLP_DENSE_LAUNCH(1, false);
  } else {
    if (vec) FDLP_DENSE_LAUNCH(2, true);
    else FDLP_DENSE_LAUNCH(2, false);
  }
#undef FDLP_DENSE_LAUNCH
  return hipGetLastError();
}

// -----------------------------------------------------------------------------------------------------------
// row_epilogue_kernel: one wave per row of the [rows, C] logits, in place, any C.  With m = max_j x_j and
// S = sum_j exp(x_j - m) (lane l sums its columns l, l + 64, .. in ascending order, then a butterfly over the 64
// lanes, which leaves the same bits in every lane):
//   MODE 1 (softmax)  p_j = exp(x_j - m) / S
//   MODE 2 (loglike)  y_j = ((x_j - m) - log S) - w prior_j
// exp and log are the device library's float32 functions, the division is the correctly rounded one.  A row's
// result depends on that row alone.
// -----------------------------------------------------------------------------------------------------------
constexpr int kEpiThreads = 256;

template <int MODE>
__global__ __launch_bounds__(kEpiThreads) void row_epilogue_kernel(float* __restrict__ x, int64_t rows, int C,
                                                                   const float* __restrict__ prior, float w) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kEpiThreads / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* p = x + row * C;
  float m = -INFINITY;
  for (int j = lane; j < C; j += 64) m = fmaxf(m, p[j]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f;
  for (int j = lane; j < C; j += 64) s = __fadd_rn(s, expf(__fsub_rn(p[j], m)));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o));
  if (MODE == 1) {
    for (int j = lane; j < C; j += 64) p[j] = __fdiv_rn(expf(__fsub_rn(p[j], m)), s);
  } else {
    const float ls = logf(s);
    for (int j = lane; j < C; j += 64) {
      FDLP_CHECK(prior != nullptr);
      p[j] = __fsub_rn(__fsub_rn(__fsub_rn(p[j], m), ls), __fmul_rn(w, prior[j]));
    }
  }
}

hipError_t launch_row_epilogue(float* x, int64_t rows, int C, int mode, const float* prior, float w, hipStream_t s) {
  if (rows <= 0 || mode == 0) return hipSuccess;
  const int per = kEpiThreads / 64;
  const int64_t nb = (rows + per - 1) / per;
  if (nb > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  if (mode == 1)
    hipLaunchKernelGGL(row_epilogue_kernel<1>, dim3((unsigned)nb), dim3(kEpiThreads), 0, s, x, rows, C, prior, w);
  else
    hipLaunchKernelGGL(row_epilogue_kernel<2>, dim3((unsigned)nb), dim3(kEpiThreads), 0, s, x, rows, C, prior, w);
  return hipGetLastError();
}

hipError_t checks_nnet(unsigned int* v, bool reset) { return fdlp_checks_local(v, reset); }

}  // namespace fdlp
