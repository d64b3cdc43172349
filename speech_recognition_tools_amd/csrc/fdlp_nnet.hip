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

// -----------------------------------------------------------------------------------------------------------
// gru_scan_kernel: the time recurrence of one nn.GRU layer (gate order r, z, n), given the input projection
// G [rows, 3H] = x W_ih^T + b_ih of every row.  For each utterance, h_{-1} = 0 and for t = 0 .. len - 1
//     gh = W_hh h_{t-1} + b_hh,  r = s(G_r[t] + gh_r),  z = s(G_z[t] + gh_z),  n = tanh(G_n[t] + r gh_n),
//     h_t = (1 - z) n + z h_{t-1}            (s the logistic function; h_t is row t of the utterance in out [rows, H])
//
// The M dimension of the MFMA is the UTTERANCES: one workgroup of four waves owns a group of up to kGruGU = 32
// utterances (a GruSlot each; the host sorts by length, fdlp_rnn_plan_groups) and walks t from 0 to the longest
// length of its group.  No workgroup depends on another.
//   * h_{t-1} of the group is the A operand, in LDS as [kGruGU][HS] floats, HS = ceil(H / 16) 16 + 4 (the columns
//     H .. are zero for ever; the row stride is an odd number of 16-byte slots, so a ds_read_b128 lane group falls
//     on 16 different slots).  Two such buffers: h_t goes to the other one, one barrier per step.
//   * a wave owns the SAME 32 hidden units j in all three gates, the r, z and n tiles (v_mfma_f32_32x32x2_f32) of
//     unit block 4 pass + wave, so the gate arithmetic is a register epilogue of its own accumulators.  No other
//     wave reads its 96 rows of W_hh, so it streams them itself from L2 in chunks of kGruKC = 16 columns through
//     two LDS buffers of its own ([96][kGruKC + 4] floats): the next chunk's loads are issued before the current
//     chunk's MFMAs and written to the other buffer after them; LDS operations of one wave complete in order, so
//     no barrier is needed there.
//   * every gh element is one chain acc = fmaf(h[k], W_hh[n][k], acc) from acc = +0 over
//         for g = 0, 8, 16, .. < ceil(H / 16) 16:  for i = 0 .. 3:  k = g + i, then k = g + 4 + i
//     (a k >= H contributes fmaf(+0, +0, acc): both operands are zero in LDS), and the gates are the explicitly
//     rounded float32 operations of gru_gate below.  Order and operations depend on H alone, so an utterance's
//     bits depend on that utterance alone: not on its group, its slot, the other lengths or the batch.
//   * an utterance with len <= t (or an empty slot, len = 0) still takes part in the MFMA with whatever its row of
//     the h buffer holds; it loads G from a clamped row, stores nothing, and no other row reads its row.
//   * STREAMS: one launch runs n_streams <= kGruMaxStreams independent layers of the same H over the same group
//     table (the sub-networks of a multi-stream model): the grid is (groups, streams), and workgroup (g, s) reads
//     G, W_hh, b_hh and the output base of entry s of a table passed BY VALUE in the kernel arguments (no device
//     memory; blockIdx.y is uniform, so these are scalar loads).  Row r of the output is out_s + r ldo: ldo = H for
//     a compact [rows, H] buffer, and out_s = base + s H with ldo = n_streams H writes the streams side by side
//     into one [rows, n_streams H] buffer, the concatenation the next layer reads.  Nothing else depends on the
//     stream: an utterance's bits in stream s are those of a one-stream launch on stream s's arrays.
// -----------------------------------------------------------------------------------------------------------
constexpr int kGruThreads = 256;
constexpr int kGruWS = kGruKC + 4;              // floats between rows of a staged W_hh chunk
constexpr int kGruWBuf = 3 * 32 * kGruWS;       // floats of one wave's chunk buffer: 96 rows
constexpr int kGruHead = kGruGU * 3;            // floats of the slot table in LDS: int64 row0[32], int32 len[32]
static_assert(kGruGU == 32 && kGruKC == 16 && kGruThreads == 256, "the maps of gru_scan_kernel");

static __host__ __device__ int gru_hs(int H) { return (H + kGruKC - 1) / kGruKC * kGruKC + 4; }
size_t gru_lds_bytes(int H) {
  return sizeof(float) * ((size_t)kGruHead + 2 * (size_t)kGruGU * gru_hs(H) + (size_t)(kGruThreads / 64) * 2 * kGruWBuf);
}
int gru_max_hidden() {
  int H = kGruKC;
  while (gru_lds_bytes(H + kGruKC) <= 163840) H += kGruKC;
  return H;
}

// One element of the step, every operation rounded to float32 in this order (include/fdlp.h):
//   a_r = G_r + (acc_r + b_r)     r = 1 / (1 + exp(-a_r))      and z likewise
//   a_n = G_n + r (acc_n + b_n)   n = tanh(a_n)
//   h   = (1 - z) n + z h_prev
__device__ __forceinline__ float gru_sigmoid(float a) { return __fdiv_rn(1.f, __fadd_rn(1.f, expf(-a))); }
__device__ __forceinline__ float gru_gate(float gr, float gz, float gn, float ar, float az, float an, float br,
                                          float bz, float bn, float hprev) {
  const float r = gru_sigmoid(__fadd_rn(gr, __fadd_rn(ar, br)));
  const float z = gru_sigmoid(__fadd_rn(gz, __fadd_rn(az, bz)));
  const float n = tanhf(__fadd_rn(gn, __fmul_rn(r, __fadd_rn(an, bn))));
  return __fadd_rn(__fmul_rn(__fsub_rn(1.f, z), n), __fmul_rn(z, hprev));
}

template <bool VEC>
__global__ __launch_bounds__(kGruThreads) void gru_scan_kernel(const GruStreams streams, int n_streams, int ldo,
                                                               const GruSlot* __restrict__ slots, int64_t rows,
                                                               int H) {
  // this workgroup's layer: blockIdx.y is uniform, so the four pointers are scalar loads from the argument table
  const int sid = blockIdx.y;
  FDLP_CHECK(n_streams >= 1 && n_streams <= kGruMaxStreams && sid < n_streams && ldo >= H);
  const GruStream& my = streams.s[min(sid, kGruMaxStreams - 1)];
  const float* __restrict__ G = my.G;
  const float* __restrict__ Whh = my.Whh;
  const float* __restrict__ bhh = my.bhh;
  float* __restrict__ out = my.out;
  constexpr int NP = 3 * 32 * (kGruKC / 4) / 64;  // 16-byte pieces of a wave's W_hh chunk per lane: 6
  extern __shared__ float4 gru_sh4[];
  const int HS = gru_hs(H), HB = kGruGU * HS;
  int64_t* s_row0 = (int64_t*)gru_sh4;
  int* s_len = (int*)(s_row0 + kGruGU);
  float* hb = (float*)gru_sh4 + kGruHead;                      // [2][kGruGU][HS]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* wS = hb + 2 * HB + wave * 2 * kGruWBuf;               // this wave's two chunk buffers
  const int l31 = lane & 31, hh = lane >> 5;
  FDLP_CHECK(H >= 1 && rows >= 1 && (!VEC || H % 4 == 0));

  if (tid < kGruGU) {
    const GruSlot s = slots[(size_t)blockIdx.x * kGruGU + tid];
    FDLP_CHECK(s.len >= 0 && s.row0 >= 0 && s.row0 + s.len <= rows);
    s_row0[tid] = s.row0;
    s_len[tid] = s.len;
  }
  for (int i = tid; i < 2 * HB; i += kGruThreads) hb[i] = 0.f;  // h_{-1} = 0, and the columns past H for ever
  __syncthreads();
  // the utterances whose results this lane holds: rows (e & 3) + 8 (e >> 2) + 4 hh of every 32 x 32 tile
  int64_t r0[16];
  int ln[16];
  int Tmax = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int u = (e & 3) + 8 * (e >> 2) + 4 * hh;
    r0[e] = s_row0[u];
    ln[e] = s_len[u];
  }
  for (int u = 0; u < kGruGU; ++u) Tmax = max(Tmax, s_len[u]);
  Tmax = __builtin_amdgcn_readfirstlane(Tmax);

  const int nub = (H + 31) / 32;       // blocks of 32 hidden units; pass p gives block 4 p + wave to this wave
  const int kend = HS - 4;
  const int sq = lane & 3;             // this lane's 16-byte piece of a staged row; its rows are (lane >> 2) + 16 q
  const int H3 = 3 * H;
  int cur = 0;
  for (int t = 0; t < Tmax; ++t, cur ^= 1) {
    const float* hp = hb + cur * HB;
    float* hn = hb + (cur ^ 1) * HB;
    for (int ub = wave; ub < nub; ub += kGruThreads / 64) {
      const int j = ub * 32 + l31, jc = min(j, H - 1);
      // this step's G and the biases, from clamped (always valid) addresses: they land during the MFMAs
      float g[3][16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t row = r0[e] + max(min(t, ln[e] - 1), 0);
        FDLP_CHECK(row >= 0 && row < rows);
        const float* gp = G + row * H3 + jc;
        g[0][e] = gp[0];
        g[1][e] = gp[H];
        g[2][e] = gp[2 * H];
      }
      const float br = bhh[jc], bz = bhh[H + jc], bn = bhh[2 * H + jc];
      const float* wp[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const int r = (lane >> 2) + 16 * q;                     // row of the chunk: gate r >> 5, unit r & 31
        const int n = (r >> 5) * H + min(ub * 32 + (r & 31), H - 1);
        FDLP_CHECK(n >= 0 && n < H3);
        wp[q] = Whh + (size_t)n * H;
      }
      nn_f4 pw[NP];
      auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < NP; ++q) pw[q] = dense_load4<VEC>(wp[q], k0 + 4 * sq, H);
      };
      auto stage = [&](float* S, int k0) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          const int at = ((lane >> 2) + 16 * q) * kGruWS + 4 * sq;
          FDLP_CHECK(at >= 0 && at + 3 < kGruWBuf);
          *(nn_f4*)(S + at) = dense_select4<VEC>(pw[q], k0 + 4 * sq, H, true);
        }
      };
      nn_f16 acc[3];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[c][e] = 0.f;

      fetch(0);
      stage(wS, 0);
      wave_lds_sync();
      int buf = 0;
      for (int k0 = 0; k0 < kend; k0 += kGruKC, buf ^= 1) {
        const float* S = wS + buf * kGruWBuf;
        const bool more = k0 + kGruKC < kend;
        if (more) fetch(k0 + kGruKC);
#pragma unroll
        for (int gq = 0; gq < kGruKC / 8; ++gq) {
          const int ka = l31 * HS + k0 + 8 * gq + 4 * hh;
          FDLP_CHECK(ka >= 0 && ka + 3 < HB);
          const nn_f4 a = *(const nn_f4*)(hp + ka);
          nn_f4 w[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int kw = (c * 32 + l31) * kGruWS + 8 * gq + 4 * hh;
            FDLP_CHECK(kw >= 0 && kw + 3 < kGruWBuf);
            w[c] = *(const nn_f4*)(S + kw);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], w[c][i], acc[c], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (more) stage(wS + (buf ^ 1) * kGruWBuf, k0 + kGruKC);
        wave_lds_sync();
      }
      if (j < H) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          if (t >= ln[e]) continue;
          const int u = (e & 3) + 8 * (e >> 2) + 4 * hh;
          const int at = u * HS + j;
          FDLP_CHECK(at >= 0 && at < HB && r0[e] + t < rows && j < ldo && (r0[e] + t) * ldo + j < rows * ldo);
          const float hv = gru_gate(g[0][e], g[1][e], g[2][e], acc[0][e], acc[1][e], acc[2][e], br, bz, bn, hp[at]);
          hn[at] = hv;
          out[(r0[e] + t) * ldo + j] = hv;
        }
      }
    }
    __syncthreads();  // h_t is complete, and every read of h_{t-1} is over
  }
}

hipError_t launch_gru_scan_streams(const GruStreams& st, int n_streams, int ldo, const GruSlot* slots, int n_groups,
                                   int64_t rows, int H, hipStream_t s) {
  if (n_groups <= 0 || rows <= 0) return hipSuccess;
  if (H < 1 || H > gru_max_hidden() || n_streams < 1 || n_streams > kGruMaxStreams || ldo < H)
    return hipErrorInvalidValue;
  // one template for the launch: 16-byte loads only where every stream's W_hh allows them
  bool vec = H % 4 == 0;
  for (int i = 0; i < n_streams; ++i) {
    if (!st.s[i].G || !st.s[i].Whh || !st.s[i].bhh || !st.s[i].out) return hipErrorInvalidValue;
    vec = vec && ((uintptr_t)st.s[i].Whh & 15u) == 0;
  }
  const size_t lds = gru_lds_bytes(H);
#define FDLP_GRU_LAUNCH(VEC)                                                                                     \
  do {                                                                                                           \
    if (lds > 65536)                                                                                             \
      (void)hipFuncSetAttribute((const void*)gru_scan_kernel<VEC>, hipFuncAttributeMaxDynamicSharedMemorySize,   \
                                (int)lds);                                                                       \
    hipLaunchKernelGGL((gru_scan_kernel<VEC>), dim3((unsigned)n_groups, (unsigned)n_streams), dim3(kGruThreads), \
                       lds, s, st, n_streams, ldo, slots, rows, H);                                              \
  } while (0)
  if (vec) FDLP_GRU_LAUNCH(true);
  else FDLP_GRU_LAUNCH(false);
#undef FDLP_GRU_LAUNCH
  return hipGetLastError();
}

// one layer: the one-stream case, rows of out H apart
hipError_t launch_gru_scan(const float* G, const float* Whh, const float* bhh, float* out, const GruSlot* slots,
                           int n_groups, int64_t rows, int H, hipStream_t s) {
  GruStreams st{};
  st.s[0] = {G, Whh, bhh, out};
  return launch_gru_scan_streams(st, 1, H, slots, n_groups, rows, H, s);
}

// this translation unit's counters and fdlp_vaeenc.hip's (the kernels of the same model family)
hipError_t checks_nnet(unsigned int* v, bool reset) {
  unsigned int w[2] = {0u, 0u};
  hipError_t e = fdlp_checks_local(v, reset);
  if (e != hipSuccess) return e;
  if ((e = checks_vaeenc(w, reset)) != hipSuccess) return e;
  v[0] += w[0];
  v[1] = v[1] > w[1] ? v[1] : w[1];
  return hipSuccess;
}

}  // namespace fdlp
