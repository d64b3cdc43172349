// fdlp_post.hip -- gfx950 kernel of the feature post-processing chain every consumer of the reference runs on
// the arks (decode.sh:84-90, get_Tandem_feats.sh:31-35, src/nnet/data_prep_*.py):
//   apply-cmvn   y = fl32(fl32(x * scale[d]) + offset[d])      (two roundings; the multiply only with --norm-vars)
//   add-deltas   block i of frame t = sum_j scales[i][j] * y[clamp(t + j, 0, T-1)]   (float32, ascending j)
//   splice-feats row t = [z[clamp(t-L)] .. z[clamp(t+R)]] of the delta-augmented rows z
// in one launch over a batch of concatenated utterances: every input row is read once per tile it touches,
// every output row is written once, and nothing in between goes through HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdlp_device.h"

namespace fdlp {

// A workgroup owns PostTile: tf consecutive frames t0 .. of one utterance.  LDS:
//   A [tf + L + R + 2H][D]   (only with deltas, H = order * window) the CMVN'd input frames lo .. hi-1,
//                            lo = max(0, t0 - L - H), hi = min(T, t0 + tf + R + H)
//   B [tf + L + R][D']       the delta-augmented rows of the unclamped frames u = t0 - L .. t0 + tf + R - 1
//                            (a row holds the values of frame clamp(u, 0, T-1)), D' = D (order + 1)
// Output row t0 + r is then the contiguous slice B[r D' .. r D' + (L + R + 1) D'), and the tile's output is one
// contiguous global range, streamed out with 16-byte stores between a scalar head and tail.
constexpr int kPostThreads = 256;
constexpr int kPostLdsMax = 160 * 1024;
constexpr int kPostLdsTarget = 64 * 1024;  // two workgroups per CU: one loads while the other stores
constexpr int kPostTileMax = 128;
// Stage ablation for benchmarks/post_throughput.py (a variant library built with -DFDLP_POST_SKIP=n, never the
// default build): bit 0 skips the global loads (frames of zeros), bit 1 the delta filter, bit 2 the stores.
#ifndef FDLP_POST_SKIP
#define FDLP_POST_SKIP 0
#endif

static inline size_t post_a_floats(int tf, int D, int order, int window, int L, int R) {
  if (order == 0) return 0;
  const size_t a = ((size_t)tf + L + R + 2 * (size_t)order * window) * D;
  return (a + 3) / 4 * 4;  // B starts 16-byte aligned
}

size_t post_lds_bytes(int tf, int D, int order, int window, int L, int R) {
  return sizeof(float) * (post_a_floats(tf, D, order, window, L, R) + ((size_t)tf + L + R) * D * (order + 1));
}

int post_pick_tile(int D, int order, int window, int L, int R) {
  for (int tf = kPostTileMax; tf >= 1; tf >>= 1)
    if (post_lds_bytes(tf, D, order, window, L, R) <= (size_t)kPostLdsTarget) return tf;
  return post_lds_bytes(1, D, order, window, L, R) <= (size_t)kPostLdsMax ? 1 : 0;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the two roundings of ApplyCmvn stay separate (no contraction into an FMA)
__device__ __forceinline__ float cmvn1(float v, float s, float o, bool mul) {
  if (mul) v = __fmul_rn(v, s);
  return __fadd_rn(v, o);
}

// MODE -1: no deltas; 0: any order and window (taps read from the table as they are used); 1 .. kPostSpecMax:
// delta order MODE with window 2 (Kaldi's default), the taps in registers and the frame's 4 MODE + 1 input rows
// read from LDS once.  All modes perform the same float32 operations in the same order.
constexpr int kPostSpecMax = 2;  // order 3 would keep 27 taps in SGPRs and spill four of them
constexpr int kPostSpecWindow = 2;

// (r, q) = (e / n, e % n) of a thread's first element and the carry-stepping to its next one, kPostThreads on
struct DivStep {
  int r, q, dr, dq, n;
  __device__ __forceinline__ DivStep(int e, int n_) : n(n_) {
    r = e / n;
    q = e - r * n;
    dr = kPostThreads / n;
    dq = kPostThreads - dr * n;
  }
  __device__ __forceinline__ void next() {
    r += dr;
    q += dq;
    if (q >= n) {
      q -= n;
      ++r;
    }
  }
};

template <int MODE>
__global__ __launch_bounds__(kPostThreads) void post_kernel(PostConsts c, const PostTile* __restrict__ tiles,
                                                            const float* __restrict__ x, int64_t n_rows,
                                                            const float* __restrict__ norm, int norm_mul,
                                                            float* __restrict__ out) {
  extern __shared__ float4 post_sh4[];
  float* sh = (float*)post_sh4;
  const PostTile tl = tiles[blockIdx.x];
  const int tid = threadIdx.x;
  const int T = tl.T, t0 = tl.t0, D = c.D, L = c.L, R = c.R;
  const int tf = min(c.tf, T - t0);
  constexpr bool DELTA = MODE >= 0;
  const int H = DELTA ? c.order * c.window : 0;
  const int lo = max(0, t0 - L - H), hi = min(T, t0 + tf + R + H);
  const int nb = tf + L + R;  // rows of B in use
  float* A = sh;
  float* B = sh + c.a_floats;
  FDLP_CHECK(tf >= 1 && t0 >= 0 && lo < hi && tl.row0 >= 0 && tl.row0 + T <= n_rows);
  FDLP_CHECK(hi - lo <= c.tf + L + R + 2 * H);

  // 1. frames lo .. hi-1 -> LDS, CMVN on the way.  Without deltas they go straight to their rows of B.
  float* dst = DELTA ? A : B + (lo - (t0 - L)) * D;
  const float* sc = norm ? norm + (size_t)tl.norm * 2 * c.Din : nullptr;
  const float* of = norm ? sc + c.Din : nullptr;
  const float* src = x + (tl.row0 + lo) * c.Din;
  const bool mul = norm_mul != 0;
  if (c.vec4) {
    const int D4 = D >> 2;
    const int n4 = (hi - lo) * D4;
    DivStep ds(tid, D4);
    for (int e = tid; e < n4; e += kPostThreads, ds.next()) {
      const int r = ds.r, q = ds.q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!(FDLP_POST_SKIP & 1)) v = ((const float4*)(src + (int64_t)r * c.Din))[q];
      if (norm) {
        const float4 s4 = ((const float4*)sc)[q], o4 = ((const float4*)of)[q];
        v.x = cmvn1(v.x, s4.x, o4.x, mul);
        v.y = cmvn1(v.y, s4.y, o4.y, mul);
        v.z = cmvn1(v.z, s4.z, o4.z, mul);
        v.w = cmvn1(v.w, s4.w, o4.w, mul);
      }
      ((float4*)(dst + r * D))[q] = v;
    }
  } else {
    const int n1 = (hi - lo) * D;
    DivStep ds(tid, D);
    for (int e = tid; e < n1; e += kPostThreads, ds.next()) {
      const int r = ds.r, d = ds.q;
      float v = 0.f;
      if (!(FDLP_POST_SKIP & 1)) v = src[(int64_t)r * c.Din + d];
      if (norm) v = cmvn1(v, sc[d], of[d], mul);
      dst[e] = v;
    }
  }
  __syncthreads();

  if constexpr (MODE > 0) {
    // 2. delta-augmented rows of the unclamped frames u = t0 - L + m: the filter runs on the edge-clamped
    //    input (DeltaFeatures::Process), block 0 is the frame itself, zero taps are skipped as Kaldi does
    constexpr int W = kPostSpecWindow, HW = MODE * W, NT = MODE + W * MODE * (MODE + 1);
    float taps[NT];  // scales[1] .. scales[MODE], uniform
#pragma unroll
    for (int k = 0; k < NT; ++k) taps[k] = c.scales[1 + k];
    const int n2 = nb * D;
    DivStep ds(tid, D);
    for (int e = tid; e < n2; e += kPostThreads, ds.next()) {
      const int m = ds.r, d = ds.q;
      const int cc = clampi(t0 - L + m, 0, T - 1);
      float w[2 * HW + 1];
#pragma unroll
      for (int j = -HW; j <= HW; ++j) {
        const int f = clampi(cc + j, 0, T - 1);
        FDLP_CHECK(f >= lo && f < hi);
        w[j + HW] = A[(f - lo) * D + d];
      }
      float* brow = B + m * c.Dp + d;
      brow[0] = w[HW];
      int tp = 0;
#pragma unroll
      for (int i = 1; i <= MODE; ++i) {
        const int hw = i * W;
        float acc = 0.f;
        if (!(FDLP_POST_SKIP & 2)) {
#pragma unroll
          for (int j = -hw; j <= hw; ++j) {
            const float sj = taps[tp + j + hw];
            if (sj != 0.f) acc = __fmaf_rn(sj, w[HW + j], acc);
          }
        }
        tp += 2 * hw + 1;
        brow[i * D] = acc;
      }
    }
  } else if constexpr (MODE == 0) {
    const int n2 = nb * D;
    DivStep ds(tid, D);
    for (int e = tid; e < n2; e += kPostThreads, ds.next()) {
      const int m = ds.r, d = ds.q;
      const int cc = clampi(t0 - L + m, 0, T - 1);
      float* brow = B + m * c.Dp + d;
      FDLP_CHECK(cc >= lo && cc < hi);
      brow[0] = A[(cc - lo) * D + d];
      for (int i = 1; i <= c.order; ++i) {
        const int hw = i * c.window;
        const float* s = c.scales + c.soff[i] + hw;
        float acc = 0.f;
        if (!(FDLP_POST_SKIP & 2)) {
          for (int j = -hw; j <= hw; ++j) {
            const float sj = s[j];
            const int f = clampi(cc + j, 0, T - 1);
            FDLP_CHECK(f >= lo && f < hi);
            if (sj != 0.f) acc = __fmaf_rn(sj, A[(f - lo) * D + d], acc);
          }
        }
        brow[i * D] = acc;
      }
    }
  } else {
    // 2'. no deltas: only the replicated edge rows of B are missing (u < 0 or u >= T)
    const int n2 = L + R > 0 ? nb * D : 0;
    DivStep ds(tid, D);
    for (int e = tid; e < n2; e += kPostThreads, ds.next()) {
      const int m = ds.r, d = ds.q;
      const int u = t0 - L + m;
      if (u < lo || u >= hi) {
        const int cc = clampi(u, 0, T - 1);
        FDLP_CHECK(cc >= lo && cc < hi && (u < 0 || u >= T));
        B[e] = B[(cc - (t0 - L)) * D + d];
      }
    }
    FDLP_CHECK(L + R > 0 || (lo == t0 && hi == t0 + tf));
  }
  __syncthreads();

  // 3. the tile's output range [(row0 + t0) Dout, (row0 + t0 + tf) Dout): element g is row r = g / Dout,
  //    column k = g % Dout, and lives at B[r D' + k]
  if (FDLP_POST_SKIP & 4) return;
  const int Dout = c.Dout, Dp = c.Dp;
  float* o = out + (tl.row0 + t0) * (int64_t)Dout;
  const int n = tf * Dout;
  const int blds = nb * Dp;
  (void)blds;  // read by the range checks only
  int head = 0, nvec = 0;
  if (Dout >= 4) {  // k + 3 wraps into the next row at most once
    head = min(n, (int)(((16u - (unsigned)((uintptr_t)o & 15u)) & 15u) >> 2));
    nvec = (n - head) >> 2;
  }
  if (nvec > 0) {
    const int wrap = Dout - Dp;  // a column past Dout is column k - Dout of the next row: LDS index - (L + R) D'
    int g = head + 4 * tid;
    int r = g / Dout, k = g - r * Dout;
    for (int v = tid; v < nvec; v += kPostThreads) {
      const int li = r * Dp + k;
      const int i0 = li, i1 = li + 1 - (k + 1 >= Dout ? wrap : 0), i2 = li + 2 - (k + 2 >= Dout ? wrap : 0),
                i3 = li + 3 - (k + 3 >= Dout ? wrap : 0);
      FDLP_CHECK(i0 >= 0 && i0 < blds && i1 >= 0 && i1 < blds && i2 >= 0 && i2 < blds && i3 >= 0 && i3 < blds);
      FDLP_CHECK(head + 4 * v + 3 < n && (((uintptr_t)(o + head + 4 * v)) & 15u) == 0);
      *(float4*)(o + head + 4 * v) = make_float4(B[i0], B[i1], B[i2], B[i3]);
      k += c.kstep;
      r += c.rstep;
      if (k >= Dout) {
        k -= Dout;
        ++r;
      }
    }
  }
  // scalar head and tail (everything when Dout < 4)
  const int ntail = n - head - 4 * nvec;
  for (int e = tid; e < head + ntail; e += kPostThreads) {
    const int g = e < head ? e : e + 4 * nvec;
    const int r = g / Dout, k = g - r * Dout;
    FDLP_CHECK(g >= 0 && g < n && r * Dp + k < blds);
    o[g] = B[r * Dp + k];
  }
}

hipError_t launch_post(const PostConsts& c, const PostTile* tiles, int ntiles, const float* x, int64_t n_rows,
                       const float* norm, int norm_mul, float* out, hipStream_t s) {
  if (ntiles <= 0) return hipSuccess;
  const size_t lds = post_lds_bytes(c.tf, c.D, c.order, c.window, c.L, c.R);
  const int mode = c.order == 0 ? -1 : (c.window == kPostSpecWindow && c.order <= kPostSpecMax ? c.order : 0);
#define FDLP_POST_LAUNCH(M)                                                                                        \
  do {                                                                                                             \
    if (lds > 65536)                                                                                               \
      (void)hipFuncSetAttribute((const void*)post_kernel<M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL(post_kernel<M>, dim3(ntiles), dim3(kPostThreads), lds, s, c, tiles, x, n_rows, norm,        \
                       norm_mul, out);                                                                             \
  } while (0)
  switch (mode) {
    case -1: FDLP_POST_LAUNCH(-1); break;
    case 1: FDLP_POST_LAUNCH(1); break;
    case 2: FDLP_POST_LAUNCH(2); break;
    default: FDLP_POST_LAUNCH(0); break;
  }
#undef FDLP_POST_LAUNCH
  return hipGetLastError();
}

hipError_t checks_post(unsigned int* v, bool reset) { return fdlp_checks_local(v, reset); }

}  // namespace fdlp
