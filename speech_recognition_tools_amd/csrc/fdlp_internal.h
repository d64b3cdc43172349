// fdlp_internal.h -- structures shared by the host runtime (fdlp_plan*.cpp) and the gfx950
// kernels (fdlp_*.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace fdlp {

constexpr int kMaxRadices = 16;
constexpr int kXcds = 8;  // XCDs of an MI355X; workgroup b is dispatched to XCD b mod 8

// A length-n complex DFT factored into radices (Stockham autosort, one LDS-resident pass).
struct DftPlan {
  int n;
  int nrad;
  int rad[kMaxRadices];
};

// One analysis frame of the batch (getFrames, features.py:118-154).
struct FrameDesc {
  int64_t pcm_off;     // first sample of the utterance in the batch PCM buffer
  int64_t noise_off;   // noise mixing offset (features.py:25), -1 = none
  double alpha;        // noise mixing gain (features.py:29)
  int32_t T;           // utterance length in samples
  int32_t k;           // frame index inside the utterance
  int32_t dst, src, cnt;  // OLA slice (computeFDLPSpectrogram.py:207-218)
  int32_t utt;         // utterance index in the batch
};

// One utterance of the batch (output side).
struct UttDesc {
  int64_t out_row;     // first output row
  int32_t L;           // output frames
  int32_t frame0;      // first analysis frame (global index in the batch)
  int32_t F;           // analysis frames
  int32_t pad;
};

// One snapshot of a skirt sweep: after the positions >= S are consumed, band `band` receives
// K times the truncated autocorrelation (structured autocorrelation, fdlp_autocorr.hip 3s).
struct SkSnap {
  int32_t S;
  int32_t band;
  double K;
};

constexpr int kMaxFlatParts = 4;
constexpr int kMaxChains = 8;
// doubles every autocorrelation row buffer (r, r_up, r_flat, r_wrap, r_flat_part) carries past its last row:
// ac_band_kernel reads its combine rows in whole 32-lag blocks (lags up to 32 ceil(nlags / 32) - 1)
constexpr int kRowSlack = 64;

// One event of the flat-top sweep (ac_vsweep_kernel): at sweep position S (after the positions >= S
// are consumed) restart (type 0) or emit (type 1) chain `chain`, which serves band `band`.
struct FlatEv {
  int32_t S, band, type, chain;
};

// ac_vsweep_kernel's sweep geometry and block schedule, shared with the host's replay of it
// (fdlp_plan_sweep_schedule): ring positions per unit, positions staged per chunk, and the rule for the
// runs of whole blocks that the kernel takes without a test.
constexpr int kVsRingPositions = 512;
constexpr int vs_chunk_positions(int A, bool flat) { return (!flat && 18 * A < kVsRingPositions - 256) ? 256 : 128; }
// The lowest block (index = base / A) that is still "plain" when the next event is at evS (-1: none), the
// staged positions start at lo_loaded and the sweep's last block is b_bot: its base lies above the event, the
// block below it is staged, and it is not the last block.  Blocks from there up to the current one (if that
// ends at or below the sweep's top) hold no event, no sweep end and need no chunk: one unmasked pass each.
__host__ __device__ inline int vs_plain_low(int evS, int lo_loaded, int b_bot, int A) {
  const int be = (evS + A) / A, bs = (lo_loaded + A - 1) / A + 1, bb = b_bot + 1;
  const int m = be > bs ? be : bs;
  return m > bb ? m : bb;
}
// The highest block that ends at or below the sweep's top nhi (the top block itself may be cut by nhi).
__host__ __device__ inline int vs_whole_top(int nhi, int A) { return nhi / A - 1; }
// Number of (X, Y) pairs of plain blocks to run from block b down before the next general block; 0 when b is
// above b_whole or fewer than two plain blocks are left (b - low + 1 is then below 2, possibly negative).
__host__ __device__ inline int vs_run_pairs(int b, int b_whole, int evS, int lo_loaded, int b_bot, int A) {
  if (b > b_whole) return 0;
  const int n = b - vs_plain_low(evS, lo_loaded, b_bot, A) + 1;
  return n > 0 ? n >> 1 : 0;
}
// One step of a sweep's schedule as the host lists it: `run` plain blocks (always even: (X, Y) bank
// pairs), then the action -- commit the chunk that starts at pos, run the general block at base pos
// (aux = events it handles), or end the sweep (aux = events handled after the last block).
enum VsAction { kVsCommit = 0, kVsGeneral = 1, kVsEnd = 2 };
struct VsRec {
  int32_t run, action, pos, aux;
};

// Device-resident constants of a plan.
struct DevConsts {
  int B, N, hop, ext, p, nlags, M, Me, kk, env_nfft;
  const double* fbank;     // [B, N] dense taps (column N of the reference's nfft/2+1 dropped, :190)
  const int* lo;           // [B] first tap >= eps
  const int* hi;           // [B] one past the last tap >= eps
  const double* hamming;   // [N]   np.hamming(N)
  const double* weights;   // [3, M] mask (:94-103), lifter (:195-196), gamma (:197-198); 1.0 if absent
  const double* env_cos;   // [env_nfft] cos(2*pi*q/env_nfft)
  const double* env_win;   // [kk, 2] (hanning(kk)[t] / hamming(kk)[t], 1.0) interleaved (:205)
  const double* tw1;       // [N1 * N2] four-step twiddles exp(-2*pi*i*n2*k1/(N1*N2)) (complex)
  const double* post;      // [N] complex exp(-i*pi*k/(2N)) (Makhoul post-twiddle)
  const double* rtw;       // [N/2] complex exp(-2*pi*i*k/N) (real-FFT unpacking; real_fft only)
  int real_fft;            // N even: the DCT runs a length-N/2 complex FFT of the packed real sequence
  // structured autocorrelation (cochlear filterbank, fixed skirt slope); null when not used
  const double* sk_e;      // [2, N] E = 10^(a (fw - c0)) (lower skirt), E' = 10^(-b (fw - c0)) (upper)
  const SkSnap* sk_snap;   // [2, B] sorted by S descending: S = N - m1_j (lower) / m2_j (upper) with
                           // K_j = 10^(a (w - 2 fc_j + 2 c0)) / K'_j = 10^(b (2 fc_j + w - 2 c0))
  const int2* sk_reg;      // [B] (m1_j, m2_j): lower skirt [0,m1), flat top [m1,m2), upper skirt [m2,N)
  int sk_min[2];           // smallest threshold per skirt
  // lag-parallel VALU sweeps (ac_vsweep_kernel); fl_ev null when not used
  const FlatEv* fl_ev = nullptr;  // [fl_nev] flat-top events sorted by S descending
  int fl_nev = 0, fl_C = 0;       // event count, chains needed (bands j and j - C never overlap)
  int fl_lo = 0, fl_hi = 0;       // min m1, max m2
  // the flat sweep is split into fl_H position parts [fl_part_lo[h], fl_part_hi[h]) run by different
  // waves; part h takes the events fl_ev[fl_part_ev[h] .. fl_part_ev[h+1]) and, for h < fl_H - 1, leaves
  // every chain in rflat_part[f][h][chain] for the bands that continue below it
  int fl_H = 1;
  int fl_part_lo[kMaxFlatParts] = {0}, fl_part_hi[kMaxFlatParts] = {0}, fl_part_ev[kMaxFlatParts + 1] = {0};
  const int2* fl_band = nullptr;  // [B] (chain, bitmask of the parts h < fl_H - 1 it needs a partial from)
  int fl_stage = 0;               // fdlp_set_flat_staging: 0 LDS-DMA where it applies (default), 1 the register form
  // wrap straddle shared by the bands whose first / last nlags - 1 taps lie on their skirts: [B]
  // sqrt(K_j K'_j), 0 for the bands whose wrap straddle ac_band_kernel computes from the taps; null: none
  const double* sk_wrap = nullptr;
  // persistent LPC kernel: resident blocks on the plan's device (prepare_lpc_env, at plan creation)
  int lpc_blocks = 0;
  int lpc_mode = 0;        // fdlp_set_lpc_path: 0 lattice kernels (default), 1 the LDS Durbin (cross-check)
  int lpc_split = 0;       // the Durbin as durbin8_kernel (8 lanes per item), then the cepstrum/envelope
                           // kernel (set by prepare_lpc_env when p fits durbin8_kernel)
  int natural = 0;         // complex modulation: frames in sample order, dft2 writes X = conj(DFT_N)/N
                           // (scipy.fftpack.ifft of the real frame), bins [0, N/2), as double2 rows of N doubles
  int lpc_astride = 0;     // split Durbin: row stride of a_pad (the cepstrum kernel's a-area length,
                           // zero past p), so a row is one contiguous LDS-DMA copy
  const double2* dct1_tw = nullptr;  // dct_frame_kernel tables (N = 24000 only; see dct_frame_tables)
};

// Per-kernel HIP-event marks (fdlp_set_profiling(plan, 2), fdlp_kernel_times): while a profiled fdlp_compute
// issues its kernels, each launch site calls kmark(id, stream) after its launch, which records an event on
// that stream when marks are being collected on this thread (g_kmarks), and does nothing otherwise.
enum KernelId {
  kKDctFrame = 0, kKFramesDft1, kKDft2Dct, kKVsweepSkirt, kKVsweepFlat, kKAcWrap, kKAcBand, kKAcSweep,
  kKAutocorr, kKDurbin4, kKDurbin8, kKLattice, kKLpcLds, kKOlaLog, kKOther, kKCount
};
struct KMark {
  int id;
  hipEvent_t ev;
};
extern thread_local std::vector<KMark>* g_kmarks;
hipError_t kmark(int id, hipStream_t s);

}  // namespace fdlp

// Launch wrappers implemented in fdlp_{dct,autocorr,lpc,misc}.hip (host-callable).
namespace fdlp {
struct Workspace {
  double2* z;      // [F, N1, N2] complex (four-step intermediate)
  double* dct;     // [F, N]
  double* r;       // [F*B, nlags]
  double* a;       // [F*B, p+1]
  double* a_pad;   // [F*B, lpc_astride] (split Durbin only)
  double* gg;      // [F*B]
  double* cep;     // [F*B, M]
  double* env;     // [F*B, kk]
};

hipError_t launch_frames_dft1(const DevConsts& c, const DftPlan& d1, int N2, const void* pcm,
                              int pcm_kind, const int16_t* noise, const FrameDesc* frames,
                              const double* dense_rows, int nframes, double2* z,
                              const double2* om1, hipStream_t s);
hipError_t launch_dft2_dct(const DevConsts& c, const DftPlan& d2, int N1, const double2* z,
                           int nframes, double* dct, const double2* om2, hipStream_t s);
// the recipes' DCT (N = 24000, real FFT) as one kernel per frame; hipErrorInvalidValue otherwise
hipError_t launch_dct_frame(const DevConsts& c, const void* pcm, int pcm_kind, const int16_t* noise,
                            const FrameDesc* frames, const double* dense_rows, int nframes, double* dct,
                            hipStream_t s);
std::vector<double2> dct_frame_tables(int N, const std::vector<double>& window);
// FDLP_DEVICE_CHECKS builds: each kernel translation unit's violation counter and last failing line
hipError_t checks_dct(unsigned int* v, bool reset);
hipError_t checks_autocorr(unsigned int* v, bool reset);
hipError_t checks_lpc(unsigned int* v, bool reset);
hipError_t checks_misc(unsigned int* v, bool reset);
hipError_t launch_autocorr(const DevConsts& c, const double* dct, const double* dense_rows,
                           int nframes_or_items, double* r, hipStream_t s);
hipError_t launch_autocorr_structured(const DevConsts& c, const double* dct, int nframes, double* r,
                                      double* rup, double* rflat, double* rflat_part, double* rwrap, hipStream_t s);
int vsweep_lanes_lags(int nlags);   // lags per lane of ac_vsweep_kernel, 0 = unsupported
int vsweep_chains(int C);           // chain count instantiated for C needed chains, 0 = unsupported
bool vsweep_fast22(int A, int C);   // vs_fast22<A, C>(): the sweep's plain runs in the 2x2 fast-correlation form (C = 0: skirts)
// the flat sweep <A, C> stages its chunks by LDS-DMA (else through registers): the instantiation has that form,
// fl_stage (DevConsts) does not force the register form, N is even and the D rows' base is 16-byte aligned
bool vsweep_flat_dma(int A, int C, int N, int fl_stage, const void* dct);
// What the autocorrelation stage launches on the resolved path (1 direct, 2 structured, 3 structured_mfma), from
// the launchers' own dispatch functions (no device needed): out as fdlp_plan_autocorr_dispatch documents it.
// reg [B] (m1, m2); wrap_kw [B] the shared-wrap factors, null when the plan has none.
void autocorr_dispatch_info(int path, int N, int nlags, int B, int fl_C, int fl_H, const int2* reg,
                            const double* wrap_kw, int32_t out[10]);
hipError_t launch_levinson(const DevConsts& c, const double* r, int items, double* a,
                           double* gg, hipStream_t s);
hipError_t launch_cepstrum(int p, int M, const double* a, const double* gg, int items,
                           double* cep, hipStream_t s);
// a_ws / gg_ws: [items, c.lpc_astride] / [items] workspace of the split Durbin (durbin8_kernel,
// c.lpc_split); a_out / gg_out (debug, [items, p+1] / [items]) get copies
hipError_t launch_lpc_env(const DevConsts& c, int odd_zero, const double* r, int items, double* env,
                          double* a_out, double* gg_out, double* cep_out, double* a_ws, double* gg_ws,
                          hipStream_t s);
int lpc_env_region(int p, int M);
// Per-plan launch setup of launch_lpc_env for the current device: sets the kernel's large-LDS
// attribute and stores the resident block count in c.lpc_blocks.
hipError_t prepare_lpc_env(DevConsts& c);
// The kernels launch_lpc_env picks for c, from the launcher's own dispatch functions (no device needed):
// out = SL, CB, DM, Durbin kernel, TS, lpc_blocks as fdlp_plan_lpc_dispatch documents them.
void lpc_dispatch_info(const DevConsts& c, int32_t out[6]);
int autocorr_tiles(int nlags);
constexpr int kDftMaxSub = 512;  // longest LDS-resident sub-DFT of the four-step DCT
// Complex modulation spectrum (computeModulationSpectrum.py --complex_modulation): per (frame, band) the
// complex circular autocorrelation of W_j X (lags 0..p+1), then Hermitian Levinson, complex gain and
// cepstrum, and the feature slice (real/imag or abs, keep_even, 1/f compensation) into the output rows.
hipError_t launch_cplx_modspec(const DevConsts& c, int L, const double* X, int nframes, double* ycplx,
                               const FrameDesc* frames, const UttDesc* utts, int c0, int coeff_n, int feat_len,
                               int step, int first, const double* faxis, int absval, float* out, double* out64,
                               int decimals, hipStream_t s);
hipError_t launch_ola_log(const DevConsts& c, const double* env, const FrameDesc* frames,
                          const UttDesc* utts, int n_utt, int maxL, float* out,
                          double* out_f64, int16_t* out_q, uint32_t* q_flag, int decimals, hipStream_t s);
// ola_log_tiled_kernel's tile shape and LDS need at B bands (no device needed; fdlp_ola_info): output rows per
// tile, the most frames on a tile / bands its register path sums, the dynamic LDS bytes, whether those need the
// large-LDS attribute, and whether a tile fits a CU at all.  launch_ola_log launches by the same numbers.
struct OlaLaunch {
  int rows, reg_frames, reg_bands;
  size_t dyn_lds;
  bool needs_attr, fits;
};
OlaLaunch ola_launch_info(int B);
// Mel spectrum (computeMelSpectrum.py): one analysis frame and the plan constants.
struct MelFrame {
  int64_t pcm_off, noise_off;  // noise_off < 0: no mixing
  double alpha;
  int64_t out_row;
  int32_t T, k;
};
struct MelConsts {
  int L, hop, ext, nfft, nh, nbins, nfilters, power;
  const double* window;  // [L]  np.hamming(L)
  const double* fbank;   // [nfilters, nbins]
  const int* lo;         // [nfilters] first non-zero tap
  const int* hi;         // [nfilters] one past the last non-zero tap
  const double2* om;     // [nh] exp(-2 pi i q / nh)
  const double2* rtw;    // [nh + 1] exp(-2 pi i k / nfft)
  DftPlan dp;            // length nh
};
hipError_t launch_mel(const MelConsts& c, const MelFrame* frames, int nframes, const void* pcm, int pcm_kind,
                      const int16_t* noise, float* out, double* out64, int decimals, hipStream_t s);
size_t mel_lds_bytes(int nh);

// MFCC (computeMfccFeatures.py): one analysis frame and the plan constants (fdlp_mfcc.hip).
struct MfccFrame {
  int64_t pcm_off, noise_off;  // noise_off < 0: no mixing
  double alpha;
  int64_t out_row;
  int32_t T, k, F, pad_;       // utterance samples, frame index in the utterance, its frame count
};
struct MfccConsts {
  int L, hop, ext, n, nb, K, Kpad, nbpad, nfilters, ncep, context, rt;
  const double* window;  // [L]  np.hamming(L)
  const double* tw;      // [Kpad, 2 nbpad]  cos | -sin of 2 pi ((i k) mod n) / n, zero padded
  const double* fold;    // [nfilters, nb]   filterbank with the mirrored bins folded in
  const int* lo;         // [nfilters] first non-zero tap of fold
  const int* hi;         // [nfilters] one past the last
  const double* dct;     // [nfilters, ncep] 2 cos(pi q (2m+1) / (2 nfilters))
};
// cep: [nframes, ncep] fp64 scratch, used when c.context > 0
hipError_t launch_mfcc(const MfccConsts& c, const MfccFrame* frames, int nframes, const void* pcm, int pcm_kind,
                       const int16_t* noise, double* cep, float* out, double* out64, int decimals, hipStream_t s);
size_t mfcc_lds_bytes(int rt, int Kpad, int nbpad, int nfilters);
int mfcc_row_tiles(int Kpad, int nbpad, int nfilters);  // 16-frame row tiles per workgroup (2, 1; 0 = too large)
hipError_t checks_mfcc(unsigned int* v, bool reset);

// Post-processing chain (apply-cmvn | add-deltas | splice-feats, fdlp_post.hip): one tile of consecutive
// frames of one utterance and the plan constants.
constexpr int kPostMaxOrder = 8;
struct PostTile {
  int64_t row0;            // batch row of the utterance's frame 0 (input and output rows coincide)
  int32_t T, t0, norm, mat;   // utterance frames, first frame of the tile, index into the norm table, and into
};                            // the transform table (xform_kernel only)
struct PostConsts {
  int Din, D, order, window, L, R, tf;  // input columns, columns kept (--truncate), ..., frames per tile
  int Dp, Dout;                         // D (order + 1), (L + R + 1) Dp
  int a_floats;                         // floats of the LDS input tile (0 without deltas)
  int kstep, rstep;                     // 1024 = rstep Dout + kstep (the store loop's stride)
  int vec4;                             // 16-byte loads: Din, D multiples of 4 and aligned pointers
  int soff[kPostMaxOrder + 1];          // scales[i] starts at scales + soff[i], 2 i window + 1 taps
  const float* scales;
};
hipError_t launch_post(const PostConsts& c, const PostTile* tiles, int ntiles, const float* x, int64_t n_rows,
                       const float* norm, int norm_mul, float* out, hipStream_t s);
size_t post_lds_bytes(int tf, int D, int order, int window, int L, int R);
// frames per tile, 0 = does not fit the LDS; extra: bytes needed beside the two tiles
int post_pick_tile(int D, int order, int window, int L, int R, size_t extra = 0);
// transform-feats fused after the splice (xform_kernel, fdlp_post.hip): out [n_rows, N] = rows x M[:, :K]^T
// (+ M[:, K]) with the device table mats [n_mat, N, C], C = K + affine, PostTile::mat picking the matrix.
struct XformConsts {
  int N, C, affine, n_mat;
  int ms_off;  // floats from the start of the LDS to the staged matrix chunk (set by launch_xform)
};
hipError_t launch_xform(const PostConsts& c, XformConsts xc, const PostTile* tiles, int ntiles, const float* x,
                        int64_t n_rows, const float* norm, int norm_mul, const float* mats, float* out,
                        hipStream_t s);
size_t xform_ms_bytes(int N);  // LDS bytes of the staged matrix chunk
int post_mode(int order, int window);  // MODE of post_kernel / xform_kernel: -1 no deltas, 0 general, 1, 2 at window 2
// The launch launch_xform makes for a plan (it reads this struct itself) and the branches xform_stage then takes.
struct XformDispatch {
  int mode, ncb;          // xform_kernel<mode, ncb>
  int groups;             // column groups of 16 ncb the kernel loops over
  int tile;               // frames per workgroup
  int vec;                // 16-byte LDS loads of the rows (D' a multiple of 4)
  int full_chunks, tail;  // K = 32 full_chunks + tail
  int big_lds;            // the launch raises the kernel's dynamic LDS limit first
  size_t post_lds, lds;   // bytes of the two tiles, and with the staged matrix chunk
};
XformDispatch xform_dispatch(const PostConsts& c, int N);
size_t xform_lds_bytes(int tf, int D, int order, int window, int L, int R, int N);
hipError_t checks_post(unsigned int* v, bool reset);

// Feed-forward network after the chain (fdlp_nnet.hip).  dense_kernel: out [rows, N] = f(A [rows, K]) W[N, K]^T + b,
// f = max(x, 0) with relu, a kDenseTM x dense_col_tile(N) output tile per workgroup, K in chunks of kDenseKC.
constexpr int kDenseTM = 128, kDenseTN = 128, kDenseKC = 32;
int dense_col_tile(int N);       // kDenseTN, or 64 for N <= 64
size_t dense_lds_bytes(int N);   // LDS bytes of a workgroup
hipError_t launch_dense(const float* A, const float* W, const float* bias, float* out, int64_t rows, int K, int N,
                        int relu, hipStream_t s);
// mode 1: softmax, 2: log_softmax - w prior, in place on x [rows, C]; 0: nothing
hipError_t launch_row_epilogue(float* x, int64_t rows, int C, int mode, const float* prior, float w, hipStream_t s);
// The time scan of a GRU layer (gru_scan_kernel, fdlp_nnet.hip): one workgroup per group of up to kGruGU
// utterances (the M dimension of v_mfma_f32_32x32x2_f32), W_hh streamed in chunks of kGruKC columns.  Slot i of
// group g is slots[g kGruGU + i]: rows row0 .. row0 + len - 1 of G [rows, 3H] and out [rows, H]; len 0 = empty.
constexpr int kGruGU = 32, kGruKC = 16;
struct GruSlot {
  int64_t row0;
  int32_t len, pad;
};
size_t gru_lds_bytes(int H);     // LDS bytes of a workgroup
int gru_max_hidden();            // the largest H whose workgroup fits the 160 KB LDS
hipError_t launch_gru_scan(const float* G, const float* Whh, const float* bhh, float* out, const GruSlot* slots,
                           int n_groups, int64_t rows, int H, hipStream_t s);
// The same scan for n_streams independent layers of one width H in one launch, grid (n_groups, n_streams): stream i
// reads G [rows, 3H], Whh, bhh of entry i and writes row r at out + r ldo (ldo >= H; out = base + i H with
// ldo = n_streams H puts the streams side by side in one [rows, n_streams H] buffer).  The table travels by value in
// the kernel arguments.  launch_gru_scan is the case n_streams = 1, ldo = H.
constexpr int kGruMaxStreams = 8;  // FDLP_MMOD_MAX_STREAMS
struct GruStream {
  const float *G, *Whh, *bhh;
  float* out;
};
struct GruStreams {
  GruStream s[kGruMaxStreams];
};
hipError_t launch_gru_scan_streams(const GruStreams& st, int n_streams, int ldo, const GruSlot* slots, int n_groups,
                                   int64_t rows, int H, hipStream_t s);
hipError_t checks_nnet(unsigned int* v, bool reset);

// The VAE-encoded models (fdlp_vaeenc.hip).  conv2d_same_kernel: one same-padded Conv2d over rows [t][c F + f]; GEMM
// rows are the positions p = t F + f of ONE utterance, a ConvTile the kDenseTM positions from p0, and the chain of
// every output is dense_kernel's at K = Ci kh kw (k the flat index of W[co] in (ci, dh, dw)).  koff: the device copy
// of conv_koff_table's ceil(K / kDenseKC) kDenseKC offsets into the staged input patch.
struct ConvTile {
  int64_t row0;        // batch row of the utterance's frame 0 (input and output rows coincide)
  int32_t T, p0;       // utterance frames; first position of the tile, a multiple of kDenseTM below T F
};
struct ConvConsts {
  int F, Ci, Co, kh, kw;
  int K, KP, NFR, patch_floats;  // Ci kh kw, K rounded up to kDenseKC, frames and floats of the staged patch
};
int conv_patch_frames(int F, int kw);
size_t conv_lds_bytes(int F, int Ci, int Co, int kh, int kw);  // LDS bytes of a workgroup
void conv_koff_table(int F, int Ci, int kh, int kw, int32_t* koff);
hipError_t launch_conv2d_same(const float* in, const float* W, const float* bias, float* out, const ConvTile* tiles,
                              int ntiles, const int32_t* koff, int64_t rows, int F, int Ci, int Co, int kh, int kw,
                              int relu, hipStream_t s);
// utt_norm_kernel: out = (z - mean_t z) / sqrt(var_t), unbiased, per utterance (a GruSlot; len 0 = empty) and column
// of z [rows, D]; in == out is allowed
hipError_t launch_utt_norm(const float* in, float* out, const GruSlot* slots, int n_slots, int64_t rows, int D,
                           hipStream_t s);
hipError_t checks_vaeenc(unsigned int* v, bool reset);  // summed into checks_nnet

// The multi-domain tools (fdlp_lifelong.hip; include/fdlp.h states the arithmetic).  row_off and utt_len are DEVICE
// int64 [n_utt]; post is [D, n_rows, C] float32.  part: mmeasure_kernel's tile partials, 8 n_utt D mmeasure_tiles(C)
// doubles; out [n_utt, D].
int mmeasure_tiles(int C);
hipError_t launch_mmeasure(const float* post, int D, int64_t n_rows, int C, int n_utt, const int64_t* row_off,
                           const int64_t* utt_len, double* part, double* out, hipStream_t s);
hipError_t launch_vae_sample(const float* ml, const float* eps, float* z, int64_t rows, int bn, hipStream_t s);
// elbo [rows] float32 is written, then reduced per utterance into out[u ld] (mode 0: mean, 1: mean of expf)
hipError_t launch_vae_elbo(const float* x, const float* xh, const float* ml, float* elbo, int64_t rows, int K, int bn,
                           int n_utt, const int64_t* row_off, const int64_t* utt_len, int mode, double* out, int ld,
                           hipStream_t s);
// mode 0: lifelong (tab = exp(prior)), 1: incremental (tab = prior); max_len: the longest utterance of the batch
hipError_t launch_lifelong_fuse(const float* post, int D, int64_t n_rows, int C, int n_utt, int64_t max_len,
                                const int64_t* row_off, const int64_t* utt_len, const double* w, const double* tab,
                                double pw, int mode, float* out, hipStream_t s);

// One utterance of a reverb batch (fdlp_reverb): samples at pcm[off, off+T), y at [yoff, yoff+T+R-1).
struct RevUtt {
  int64_t off, T, yoff, noff;  // noff < 0: no noise mixing
  double alpha;
};
hipError_t launch_reverb(const RevUtt* U, int n_utt, int64_t maxT, const void* pcm, int kind, int pre,
                         const int16_t* noise, const double* rir, int R, double* x, double* y, double* xs,
                         double* out, int64_t* out_len, hipStream_t s);
hipError_t launch_modspec_out(const double* cep, const FrameDesc* frames, const UttDesc* utts, int nframes, int B,
                              int M, int c0, int feat_len, int step, int first, const double* faxis, int absval,
                              float* out, double* out64, int decimals, hipStream_t s);
int cmvn_chunks(int64_t rows);
hipError_t launch_cmvn(const float* x, int64_t rows, int D, double* part, double* stats, hipStream_t s);
hipError_t launch_device_fn(int fn, const double* x, double* y, int64_t n, hipStream_t s);
}  // namespace fdlp
