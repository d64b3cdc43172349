/*
 * fdlp.h -- C ABI of libfdlp_hip.so, the MI355X (gfx950) FDLP-spectrogram extractor.
 *
 * Drop-in boundary for the reference hot path
 *   sadhusamik/speech_recognition_tools  src/featgen/computeFDLPSpectrogram.py  getFeats :29-237
 *   (+ the helpers it imports from src/featgen/features.py).
 * The reference has no FFI of its own (it is pure Python calling numpy/scipy); the entry points
 * below are what a ctypes binding of that path needs (INTEGRATION.md shows the binding).
 * Each function names the reference interface it replaces.
 *
 * Conventions: plain C types, caller-owned buffers, no C++ exceptions across the boundary.
 * Every function returns 0 on success or a negative FDLP_E* code; fdlp_last_error() returns a
 * thread-local message for the last failure.  "dev" pointers are device (HBM) pointers,
 * everything else is host memory.  `stream` is a hipStream_t passed as void* (NULL = default).
 */
#ifndef FDLP_H
#define FDLP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDLP_ABI_VERSION 13

enum {
  FDLP_OK = 0,
  FDLP_E_INVALID = -1,   /* bad argument / configuration the reference would reject      */
  FDLP_E_HIP = -2,       /* HIP runtime failure                                            */
  FDLP_E_NOMEM = -3,     /* allocation failure                                             */
  FDLP_E_CAPACITY = -4,  /* batch larger than the plan's max_frames                        */
  FDLP_E_IO = -5,        /* file read/write failure                                        */
  FDLP_E_BROADCAST = -6  /* the reference's numpy OLA slicing would raise ValueError here  */
};

enum { FDLP_FBANK_MEL = 0, FDLP_FBANK_COCHLEAR = 1 };
enum { FDLP_PCM_I16 = 0, FDLP_PCM_F64 = 1 };
enum { FDLP_PRE_NONE = 0, FDLP_PRE_DIFF = 1 };  /* --add_noise diff (computeFDLPSpectrogram.py:162-164) */

/* Frozen feature configuration.  Mirrors the argparse surface of
 * computeFDLPSpectrogram.py:240-262 after the parsing getFeats does (:43-118). */
typedef struct fdlp_config {
  int32_t nfilters;          /* --nfilters                                   (:245) */
  int32_t coeff_num;         /* --coeff_num  (M)                             (:246) */
  int32_t coeff_lp;          /* --coeff_range "lp,hp" -> mask lp<=i<=hp      (:94-103) */
  int32_t coeff_hp;
  int32_t order;             /* --order (p)                                  (:248) */
  int32_t frate;             /* --frate                                      (:250) */
  int32_t srate;             /* 16000 (getFeats default, :29)                       */
  int32_t fbank_kind;        /* FDLP_FBANK_MEL | FDLP_FBANK_COCHLEAR          (:49-63) */
  double fduration;          /* --fduration                                  (:249) */
  double overlap_fraction;   /* --overlap_fraction (before the 1-x at :104)  (:251) */
  double warp_fact;          /* mel "mel,wf" / cochlear 6th field                    */
  double om_w, alp, bet;     /* cochlear "cochlear,om_w,alp,fixed,bet,wf"    (:59-61) */
  int32_t fixed;
  int32_t odd_mod_zero;      /* --odd_mod_zero                               (:199-200) */
  int32_t gamma_enabled;     /* --gamma_weight "scale,shape,pk" (!= "None")  (:107-118) */
  double gamma_scale, gamma_shape, gamma_pk;
  const double* lifter;      /* nullable; coeff_num values (--lifter_config first line, :43-46) */
  int32_t lifter_len;
  double support_eps;        /* filter taps < eps*peak are skipped in the autocorrelation
                                (0 = every non-zero tap; DESIGN.md "support")            */
  int32_t max_frames;        /* workspace capacity: analysis frames per fdlp_compute call  */
  /* ---- sibling feature: FDLP modulation spectrum (src/featgen/computeModulationSpectrum.py) ---- */
  int32_t mode;              /* FDLP_MODE_SPECTROGRAM | FDLP_MODE_MODSPEC | FDLP_MODE_MODSPEC_COMPLEX */
  int32_t window;            /* analysis window: FDLP_WIN_HAMMING (spectrogram, :29) |
                                FDLP_WIN_HANNING (modspec default, :30) | FDLP_WIN_RECT (--no_window) */
  int32_t coeff_0;           /* modspec --coeff_0 (1-based first kept coefficient); --coeff_n = coeff_num */
  int32_t keep_even;         /* modspec --keep_even (:66-72, :191-195)                              */
  int32_t compensate_noise;  /* modspec --compensate_noise: x linspace(0, n/(2 fduration), coeff_n) (:82-88) */
  int32_t absolute_value;    /* modspec --absolute_value (:186-187)                                 */
} fdlp_config;
enum { FDLP_MODE_SPECTROGRAM = 0, FDLP_MODE_MODSPEC = 1,
       FDLP_MODE_MODSPEC_COMPLEX = 2 /* modspec --complex_modulation (computeModulationSpectrum.py:45-47,
                                        :74-88, :153-180): ifft frames, complex LPC and cepstrum */ };
enum { FDLP_WIN_HAMMING = 0, FDLP_WIN_HANNING = 1, FDLP_WIN_RECT = 2 };

typedef struct fdlp_plan fdlp_plan;

/* Per-call batch of utterances.  Replaces the per-utterance body of getFeats
 * (computeFDLPSpectrogram.py:159-229): signal -> frames -> DCT -> per-band LPC -> cepstrum ->
 * envelope -> OLA -> log.  Samples of all utterances are concatenated in one device buffer. */
typedef struct fdlp_batch {
  int32_t n_utt;
  int32_t pcm_kind;              /* FDLP_PCM_I16 (scipy wavfile int16, :139) | FDLP_PCM_F64    */
  const void* pcm_dev;           /* device: samples                                              */
  const int64_t* pcm_off;        /* host [n_utt]: first sample of each utterance                 */
  const int64_t* utt_len;        /* host [n_utt]: T (samples) of each utterance                  */
  const uint8_t* jitter;         /* host: concatenated randrange(2) draws, F_u-1 per utterance,
                                    in utterance order (:225); see fdlp_pyrandom_*               */
  /* optional on-device noise mixing  x = s + alpha*noise[off:off+T]  (features.py:24-31) */
  const int16_t* noise_dev;      /* nullable device noise samples                                */
  const int64_t* noise_off;      /* host [n_utt]                                                 */
  const double* noise_alpha;     /* host [n_utt]                                                 */
  float* out_dev;                /* device: [sum_u L_u, nfilters] float32, row-major (ark layout) */
  const int64_t* out_row;        /* host [n_utt]: first output row of each utterance             */
  double* out_f64_dev;           /* nullable device: same layout, fp64 log features (parity)     */
  int32_t ark_decimals;          /* >=0: round out_dev like '%.<d>f' text ark (dict2Ark
                                    features.py:66 uses 3); <0: keep full float32               */
  int32_t preprocess;            /* FDLP_PRE_DIFF: x = convolve(int16 s, [1,2,3,2,0,-2,-5,-2,0,2,3,
                                    2,1], 'same') on the device (int16 PCM only)                 */
  /* ABI 7: compact ark codes, half the bytes of out_dev for the device-to-host leg.  With
     ark_decimals = d >= 0 the ark value of a feature is the float32 (float)(k / 10^d) with
     k = nearbyint(v * 10^d) (dict2Ark's '%.3f' text read back by copy-feats, features.py:66).
     out_q_dev receives k as int16 (-32768 = -0.0), same layout as out_dev; fdlp_q_widen turns the
     codes into exactly the float32 values out_dev would hold.  A value without a code (|k| > 32767
     or NaN; log features of 16-bit audio stay within [-32.24, +19]) stores -32768 and writes 1 to
     *out_q_flag_dev, which the caller zeroes before the call: that batch's float32 rows (out_dev,
     when also given) are then the ones to use.  Spectrogram plans only.                          */
  int16_t* out_q_dev;            /* nullable device [sum_u L_u, nfilters] int16 codes               */
  uint32_t* out_q_flag_dev;      /* device word, required with out_q_dev                            */
} fdlp_batch;

/* ---- plan ------------------------------------------------------------------------------- */
/* Replaces getFeats setup (:43-118): filterbank (features.py:172-219), mask/lifter/gamma
 * weights, windows, DFT plans; uploads them to `device` and allocates the workspace.
 * device < 0 creates a host-only plan (geometry, filterbank, weights, OLA tables; no compute). */
int fdlp_plan_create(const fdlp_config* cfg, int device, fdlp_plan** out);
int fdlp_plan_destroy(fdlp_plan* plan);
const char* fdlp_last_error(void);
int fdlp_abi_version(void);
/* Device address of pinned host memory (hipHostMalloc / hipHostRegister): fdlp_batch.out_dev may point
 * there, the OLA kernel then stores the features straight into host memory (no D2H copy; ABI 4). */
int fdlp_mapped_ptr(void* host, void** dev);

/* Frame geometry of one utterance of T samples: F analysis frames (getFrames,
 * features.py:151) and L output frames (int(ceil(T*frate/srate)), :182; L = F for the modspec
 * mode, one feature row per analysis frame, computeModulationSpectrum.py:161). */
int fdlp_geometry(const fdlp_plan* plan, int64_t T, int32_t* F, int32_t* L);
/* Output feature dimension per row: nfilters (spectrogram) or nfilters * feat_len (modspec). */
int fdlp_plan_out_dim(const fdlp_plan* plan, int32_t* dim);
/* Plan constants: N (DCT length), nfft, hop, nlags (=order+2), kk (envelope length). */
int fdlp_plan_info(const fdlp_plan* plan, int32_t* N, int32_t* hop, int32_t* nlags, int32_t* kk,
                   int32_t* ola_hop);
/* Host copy of the filterbank [nfilters, nfft/2+1] fp64 (createFbank / createFbankCochlear,
 * features.py:172-219) and of the per-band tap support [lo, hi). */
int fdlp_plan_fbank(const fdlp_plan* plan, double* fbank_out, int32_t* lo, int32_t* hi);
/* createFbank / createFbankCochlear (features.py:172-219) for an arbitrary nfft, using the
 * fbank_kind / warp_fact / om_w / alp / fixed / bet / nfilters / srate fields of cfg.
 * out: [nfilters, floor(nfft/2+1)]; *ncol receives the column count. */
int fdlp_make_fbank(const fdlp_config* cfg, int32_t nfft, double* out, int32_t* ncol);
/* Host copy of the folded modulation weights w[coeff_num] (:94-118, :194-200). */
int fdlp_plan_weights(const fdlp_plan* plan, double* w_out);

/* OLA table of one utterance (computeFDLPSpectrogram.py:207-225): per frame (dst, src, cnt).
 * Returns FDLP_E_BROADCAST where the reference's numpy slicing raises. */
int fdlp_ola_table(const fdlp_plan* plan, int64_t T, const uint8_t* jitter, int32_t* dst,
                   int32_t* src, int32_t* cnt);

/* ---- compute ---------------------------------------------------------------------------- */
/* Whole pipeline for a batch (getFeats :159-229).  Enqueued on `stream`; host arrays are
 * consumed before return. */
int fdlp_compute(fdlp_plan* plan, const fdlp_batch* batch, void* stream);
/* Host: the float32 ark values of n compact codes (fdlp_batch.out_q_dev) with the batch's ark_decimals,
 * bit-identical to the float32 out_dev rows; `threads` > 1 splits the work (ABI 7). */
int fdlp_q_widen(const int16_t* q, int64_t n, int32_t decimals, float* out, int32_t threads);
/* Keep the fused LPC kernel's a/gg/cep in the workspace (off by default; needed by
 * fdlp_debug_fetch for those three arrays). */
int fdlp_set_debug(fdlp_plan* plan, int32_t keep_intermediates);
/* Device range checks (ABI 6): *enabled = 1 in a library built with -DFDLP_DEVICE_CHECKS=1, whose
 * index-heavy kernels count violated range assertions (descriptors, sample / LDS / exchange indices,
 * straddle windows, OLA slices) on the device instead of trapping; *violations and *last_line (the
 * largest failing source line of csrc/) since the last reset; reset != 0 zeroes them.  Synchronises the
 * current device.  The default build reports enabled = 0 and zeros. */
int fdlp_device_checks(int32_t* enabled, uint32_t* violations, uint32_t* last_line, int32_t reset);
/* Autocorrelation algorithm (stage 2).  FDLP_AC_DIRECT: per band, over the taps >= support_eps *
 * peak.  FDLP_AC_STRUCTURED: exact (no tap truncation) skirt-factorised algorithm for the cochlear
 * filterbank with a fixed slope (fbank_type cochlear,..,fixed=1,..; DESIGN.md "Structured
 * autocorrelation"), its three sweeps (lower skirt, flat tops, upper skirt) lag-parallel on the fp64
 * VALU; FDLP_AC_STRUCTURED_MFMA: the same algorithm with MFMA lag-tile skirt sweeps and per-band
 * flat tops (also used when the VALU sweeps do not fit: more than 160 lags or 8 overlapping flat
 * tops).  FDLP_AC_AUTO (plan default) picks the first available of STRUCTURED, STRUCTURED_MFMA,
 * DIRECT.  fdlp_set_autocorr_path returns FDLP_E_INVALID when the structured paths are not
 * available; fdlp_autocorr_path returns the path in use or a negative error code. */
#define FDLP_AC_AUTO 0
#define FDLP_AC_DIRECT 1
#define FDLP_AC_STRUCTURED 2
#define FDLP_AC_STRUCTURED_MFMA 3
int fdlp_set_autocorr_path(fdlp_plan* plan, int32_t path);
int fdlp_autocorr_path(const fdlp_plan* plan);
/* What the autocorrelation stage launches for a requested path (ABI 12): FDLP_AC_AUTO or one of the explicit
 * paths, resolved as fdlp_set_autocorr_path resolves it (FDLP_E_INVALID likewise) without changing the plan's
 * path.  Answered by the functions the launchers themselves dispatch by; works on a host-only plan.
 *   out[0] the path launched: FDLP_AC_DIRECT, FDLP_AC_STRUCTURED or FDLP_AC_STRUCTURED_MFMA
 *   out[1] lag tiles NT of autocorr_kernel / ac_sweep_kernel / ac_band_kernel<NT>
 * and, on FDLP_AC_STRUCTURED (0 on the other two paths, which launch none of these):
 *   out[2] lags per lane A of ac_vsweep_kernel<A, C> (4, 8 or 10)
 *   out[3] chains the flat tops need, out[4] the chain slots C instantiated for them (4, 5, 6 or 8)
 *   out[5] position parts of the flat sweep (1 or 2)
 *   out[6], out[7] 1 when the skirt sweeps <A, 0> / the flat sweep <A, C> take their plain runs in the 2x2
 *          fast-correlation form
 *   out[8] 1 when ac_wrap_kernel runs (bands whose outermost lags - 1 taps are skirt taps share one wrap straddle)
 *   out[9] bands whose straddles ac_band_kernel stages in its compact `fast` form (the others: the general form) */
int fdlp_plan_autocorr_dispatch(const fdlp_plan* plan, int32_t path, int32_t out[10]);
/* LPC stage (Levinson-Durbin + cepstrum + envelope).  FDLP_LPC_AUTO (plan default): the register-resident
 * lattice kernels (durbin4_kernel, 4 lanes per item, for 128 <= p <= 150; durbin8_kernel, 8 lanes per item,
 * for 150 < p <= 183; then the cepstrum / envelope kernel); FDLP_LPC_LATTICE8 (ABI 6): the same with
 * durbin8_kernel for every 128 <= p <= 183 (cross-check of durbin4_kernel); FDLP_LPC_LDS:
 * the LDS Durbin kernel for every p (the fallback for p > 255 and an independent cross-check; its
 * order-k dot products are summed in another order).  The only switches between kernel variants are
 * these explicit calls: nothing is read from the environment (ABI 4). */
#define FDLP_LPC_AUTO 0
#define FDLP_LPC_LDS 1
#define FDLP_LPC_LATTICE8 2
int fdlp_set_lpc_path(fdlp_plan* plan, int32_t path);
/* The kernels the LPC stage launches for the plan's current LPC path (ABI 10), answered by the launcher's
 * own dispatch functions; works on a host-only plan, where fdlp_set_lpc_path only records the path.
 *   out[0] SL  lanes' coefficients of lpc_env_lattice_kernel<SL, CB, DM>, ceil((p+1)/16); 0 on the LDS path
 *   out[1] CB  7 the register cepstrum, -1 the sliding-window cepstrum, 0 the LDS cepstrum
 *   out[2] DM  1 the Durbin inside the lattice kernel, 2 an external Durbin kernel; 0 on the LDS path
 *   out[3] the Durbin kernel: FDLP_LPC_DURBIN_INREG, FDLP_LPC_DURBIN_4 (durbin4_kernel), 17 / 19 / 21 / 23
 *          (durbin8_kernel<SL8>), FDLP_LPC_DURBIN_LDS (lpc_env_kernel<TS>) or FDLP_LPC_DURBIN_CPLX
 *          (complex-modulation plans: cplx_lpc_out_kernel, every other field 0)
 *   out[4] TS  envelope slots per lane of lpc_env_kernel<TS>; 0 on the lattice path
 *   out[5] resident blocks of the persistent lattice kernel on the plan's device; 0 on a host-only plan
 *          and on the LDS path */
#define FDLP_LPC_DURBIN_INREG 0
#define FDLP_LPC_DURBIN_4 4
#define FDLP_LPC_DURBIN_LDS (-1)
#define FDLP_LPC_DURBIN_CPLX (-2)
int fdlp_plan_lpc_dispatch(const fdlp_plan* plan, int32_t out[6]);
/* How the flat sweep of FDLP_AC_STRUCTURED stages D into its LDS ring.  FDLP_FLAT_AUTO (plan default): by LDS-DMA
 * (global_load_lds_dwordx4, no staging registers) when every D row is 16-byte aligned, i.e. N is even and the
 * plan's dct rows start aligned; otherwise through registers.  FDLP_FLAT_REGISTER forces the register form: a
 * test switch, so that one build can compare the two (they give the same r bit for bit).  fdlp_flat_staging
 * returns the form in use, FDLP_FLAT_REGISTER or FDLP_FLAT_DMA (host-only plans too), 0 when the plan has no
 * VALU sweeps, or a negative error code. */
#define FDLP_FLAT_AUTO 0
#define FDLP_FLAT_REGISTER 1
#define FDLP_FLAT_DMA 2
int fdlp_set_flat_staging(fdlp_plan* plan, int32_t staging);
int fdlp_flat_staging(const fdlp_plan* plan);
/* DCT stage (ABI 5).  FDLP_DCT_AUTO (plan default): for the recipes' frame length N = 24000 one kernel per
 * frame (dct_frame_kernel: the packed 12000-point FFT as three in-register passes with LDS exchanges,
 * D written once); other N, and FDLP_DCT_FOUR_STEP, the two four-step kernels through the Z workspace
 * (allocated when first needed).  fdlp_dct_path returns FDLP_DCT_FRAME or FDLP_DCT_FOUR_STEP. */
#define FDLP_DCT_AUTO 0
#define FDLP_DCT_FOUR_STEP 1
#define FDLP_DCT_FRAME 2
int fdlp_set_dct_path(fdlp_plan* plan, int32_t path);
int fdlp_dct_path(const fdlp_plan* plan);
/* Lower-skirt / flat-top / upper-skirt split of every band, [0,m1) [m1,m2) [m2,N), used by the
 * STRUCTURED path; FDLP_E_INVALID when the filterbank does not have it. */
int fdlp_plan_regions(const fdlp_plan* plan, int32_t* m1, int32_t* m2);
/* The flat-top sweep of FDLP_AC_STRUCTURED (DESIGN.md "Lag-parallel VALU sweeps"): number of chains
 * (0 when the VALU sweeps are not available), position parts, and for up to cap events (S, band, type
 * 0 restart / 1 emit, chain) in sweep order; *nev receives the event count. */
int fdlp_plan_flat_events(const fdlp_plan* plan, int32_t* chains, int32_t* parts, int32_t* nev, int32_t* events,
                          int32_t cap);
/* The walk of one lag-parallel VALU sweep over its positions, as ac_vsweep_kernel takes it (DESIGN.md
 * "Lag-parallel VALU sweeps"): kind 0 lower skirt, 1 upper skirt, 2 flat tops (part < parts of
 * fdlp_plan_flat_events).  Up to cap records (run, action, pos, aux) in sweep order, top-down: `run` whole
 * blocks taken without a test (always even), then action 0 = commit the staged chunk that starts at pos,
 * 1 = one general block at base pos handling aux events, 2 = end of the sweep with aux events left.
 * info[4] = lags per lane A (the block length), positions per chunk, sweep limits nlo, nhi.  Computed on the
 * host from the plan alone (host-only plans too); *nrec = 0 when the plan has no VALU sweeps. */
int fdlp_plan_sweep_schedule(const fdlp_plan* plan, int32_t kind, int32_t part, int32_t* info, int32_t* nrec,
                             int32_t* recs, int32_t cap);
/* fdlp_compute splits a batch of F frames into min(n_sub, F/256) sub-batches that alternate
 * between the caller's stream and a second stream of the plan, so the MFMA-bound autocorrelation
 * of one sub-batch can overlap the VALU-bound kernels of the other (default 1 = serial: on MI355X
 * the fp64 MFMA and fp64 VALU work measured no net overlap). */
int fdlp_set_pipeline(fdlp_plan* plan, int32_t n_sub);
/* Reads back the intermediates of the most recent fdlp_compute (parity/debug; synchronous):
 * any pointer may be NULL.  Layouts: dct [F,N]; r [F,B,nlags]; a [F,B,order+1]; gg [F,B];
 * cep [F,B,coeff_num]; env [F,B,kk] (spectrogram plans).  ABI 9 removed the fused OLA stage
 * (fdlp_set_ola_path / fdlp_ola_path, measured slower than the separate OLA kernel). */
int fdlp_debug_fetch(fdlp_plan* plan, int32_t n_frames, double* dct, double* r, double* a,
                     double* gg, double* cep, double* env);
/* Same for the frames [first_frame, first_frame + n_frames) of the most recent batch (ABI 3).
 * a and cep need fdlp_set_debug(plan, 1) before that compute (their workspaces are allocated by it;
 * FDLP_E_INVALID otherwise); dct, r, gg and (spectrogram plans) env are always available. */
int fdlp_debug_fetch_range(fdlp_plan* plan, int32_t first_frame, int32_t n_frames, double* dct, double* r,
                           double* a, double* gg, double* cep, double* env);

/* Per-stage device time (HIP events on the stream each stage runs on) of every fdlp_compute since
 * profiling was (re)enabled.  Stages: 0 frames+column DFT, 1 row DFT+DCT, 2 autocorrelation,
 * 3 fused Levinson+cepstrum+envelope, 4 OLA+log.  With sub-batch pipelining the stage times are
 * summed over the sub-batches and overlap each other in wall time.  fdlp_stage_times
 * synchronises on the events. */
#define FDLP_NUM_STAGES 5
int fdlp_set_profiling(fdlp_plan* plan, int32_t enable);
int fdlp_stage_times(fdlp_plan* plan, double* ms_sum /* [FDLP_NUM_STAGES] */, int32_t* n_calls);
/* Per-kernel device time (ABI 9): with fdlp_set_profiling(plan, 2) every kernel launch of an fdlp_compute
 * (one sub-batch) is followed by a HIP event on the stream it runs on, and the time between consecutive
 * events -- one kernel each, the stage's launch gaps included -- is summed per kernel id.  fdlp_kernel_name
 * gives the id's kernel (the rocprofv3 name prefix, e.g. "fdlp::ac_band_kernel"); launches counts them. */
#define FDLP_NUM_KERNELS 16
int fdlp_kernel_times(fdlp_plan* plan, double* ms_sum /* [FDLP_NUM_KERNELS] */, int64_t* launches);
const char* fdlp_kernel_name(int32_t id);
/* Seconds fdlp_plan_create spent in: [0] host tables (filterbank, structured-autocorrelation tables,
 * weights), [1] device open + table uploads, [2] LPC kernel launch setup, [3] workspace allocation,
 * [4] total (a cold JOB's fixed cost, benchmarks/cold_start_probe.py; ABI 4). */
int fdlp_plan_setup_times(const fdlp_plan* plan, double* sec /* [5] */);

/* ---- stage entry points (the features.py helpers, batched on the device) --------------- */
/* scipy.fftpack.dct(x)/sqrt(2N) of n_rows windowed frames [n_rows, N] (computeFDLPSpectrogram
 * .py:178).  N is the plan's frame length. */
int fdlp_dct_rows(fdlp_plan* plan, const double* x_dev, int32_t n_rows, double* y_dev,
                  void* stream);
/* computeLpcFast (features.py:222-230) for n_items dense band signals [n_items, N]:
 * a [n_items, order+1] (a0=1), gg [n_items], and the lags r [n_items, order+2]. */
int fdlp_lpc_rows(fdlp_plan* plan, const double* band_dev, int32_t n_items, double* r_dev,
                  double* a_dev, double* gg_dev, void* stream);
/* computeModSpecFromLpc (features.py:233-246): cep [n_items, lim] from a [n_items, p+1], gg. */
int fdlp_cepstrum_rows(fdlp_plan* plan, const double* a_dev, const double* gg_dev,
                       int32_t n_items, int32_t p, int32_t lim, double* cep_dev, void* stream);
/* The output stage (computeFDLPSpectrogram.py:207-229; ABI 11) on the caller's envelopes: env_dev
 * [sum_u F_u, nfilters, kk] fp64, laid out as fdlp_debug_fetch's env, utterance after utterance.  The frame
 * and utterance tables are filled by the code fdlp_compute fills them with (utt_len, jitter and out_row as
 * in fdlp_batch) and ola_log_tiled_kernel is launched on them; out_dev / out_f64_dev / out_q_dev /
 * out_q_flag_dev / ark_decimals as in fdlp_batch, any of the three outputs may be NULL but not all.
 * The refusals are fdlp_compute's: an utterance without an analysis frame, more frames than max_frames,
 * FDLP_E_BROADCAST where the reference's OLA slicing raises, codes without ark_decimals >= 0 or a flag,
 * a host-only or modulation-spectrum plan, more bands than an LDS tile holds (fdlp_ola_info). */
int fdlp_ola_rows(fdlp_plan* plan, const double* env_dev, const int64_t* utt_len, int32_t n_utt,
                  const uint8_t* jitter, const int64_t* out_row, float* out_dev, double* out_f64_dev,
                  int16_t* out_q_dev, uint32_t* out_q_flag_dev, int32_t ark_decimals, void* stream);
/* Launch shape of the output stage for the plan's nfilters (ABI 11; host-only plans too), from the helper
 * the launcher itself uses:
 *   info[0] output rows per tile (one workgroup)
 *   info[1] the most frames overlapping a tile that the register path sums; more take the LDS loop
 *   info[2] the most bands the register path sums; more take the LDS loop
 *   info[3] dynamic LDS bytes of the launch
 *   info[4] 1 when the launch needs the large-LDS function attribute (static + dynamic LDS above 64 KB)
 *   info[5] 1 when the launcher accepts nfilters, 0 when no tile fits a CU's LDS (the launch is refused) */
int fdlp_ola_info(const fdlp_plan* plan, int32_t info[6]);

/* ---- sibling feature: mel spectrum (src/featgen/computeMelSpectrum.py, run_melspec) ----- */
/* Replaces compute_mel_spectrum (computeMelSpectrum.py:40-170): getFrames with np.hamming(L),
 * |scipy.fftpack.fft(frame, nfft)[:nfft/2+1]| @ fbank.T, log10 ('log') or squared ('power'). */
typedef struct fdlp_mel_config {
  int32_t nfilters;          /* --nfilters (23)                                        (:26)   */
  int32_t nfft;              /* --nfft (1024); even, nfft/2 a 2/3/5/7-smooth size <= 2048 (:29) */
  int32_t frate;             /* --frate (100)                                          (:28)   */
  int32_t srate;             /* 16000                                                  (:40)   */
  int32_t fbank_kind;        /* --fbank_type "mel,wf" | "cochlear,om_w,alp,fixed,bet,wf" (:53-67) */
  int32_t fixed;
  int32_t power;             /* --spectrum_type: 0 log (log10), 1 power (squared)      (:150-158) */
  double fduration;          /* --fduration (0.02)                                     (:27)   */
  double warp_fact, om_w, alp, bet;
  int32_t max_frames;        /* frames per fdlp_mel_compute call                             */
} fdlp_mel_config;
typedef struct fdlp_mel_plan fdlp_mel_plan;
int fdlp_mel_plan_create(const fdlp_mel_config* cfg, int device, fdlp_mel_plan** out);
int fdlp_mel_plan_destroy(fdlp_mel_plan* plan);
/* F frames of an utterance of T samples (getFrames, features.py:151). */
int fdlp_mel_geometry(const fdlp_mel_plan* plan, int64_t T, int32_t* F);
/* A batch (fdlp_batch: pcm, offsets, lengths, noise / diff preprocessing, out [sum F, nfilters] at
 * out_row, optional fp64 copy, ark_decimals; `jitter` is unused). */
int fdlp_mel_compute(fdlp_mel_plan* plan, const fdlp_batch* batch, void* stream);

/* ---- sibling feature: MFCC (src/featgen/computeMfccFeatures.py, make_mfcc_feats.sh) ------- */
/* Replaces extractMelEnergyFeats (computeMfccFeatures.py:58-135): signal / 2^15, getFrames with np.hamming(L),
 * |scipy.fftpack.fft(frame, n)| with n = nfft/2 + 1 (a DFT of arbitrary length: 513 at the defaults; a longer
 * frame is truncated to n samples), all n bins @ createFbank(nfilters, nfft, srate).T, log10,
 * scipy.fftpack.dct (type 2, unnormalised)[:, :13], then spliceFeats(context) whose last `context` rows of
 * an utterance stay zero.  The DFT is a dense GEMM on the fp64 MFMA; the work tile lives in the 160 KB LDS,
 * which bounds the sizes: max(min(L, n), nfilters) + n/2 <= ~1230 (L = srate * fduration), e.g. nfft <= 2048
 * with 20 ms frames; larger configurations are FDLP_E_INVALID. */
typedef struct fdlp_mfcc_config {
  int32_t nfilters;          /* --nfilters (30); >= 1                                   (:142)  */
  int32_t nfft;              /* --nfft (1024); even, no smoothness condition            (:146)  */
  int32_t frate;             /* --frate (100)                                           (:144)  */
  int32_t srate;             /* 16000                                                   (:58)   */
  double fduration;          /* --fduration (0.02)                                      (:143)  */
  int32_t context;           /* --context (0 = no splicing)                             (:145)  */
  int32_t max_frames;        /* frames per fdlp_mfcc_compute call                               */
} fdlp_mfcc_config;
typedef struct fdlp_mfcc_plan fdlp_mfcc_plan;
int fdlp_mfcc_plan_create(const fdlp_mfcc_config* cfg, int device, fdlp_mfcc_plan** out);
int fdlp_mfcc_plan_destroy(fdlp_mfcc_plan* plan);
/* F frames of an utterance of T samples (getFrames, features.py:151) and the output width
 * min(13, nfilters) * (2 context + 1) (width may be NULL). */
int fdlp_mfcc_geometry(const fdlp_mfcc_plan* plan, int64_t T, int32_t* F, int32_t* width);
/* A batch (fdlp_batch as for fdlp_mel_compute: pcm int16 or float64 in the WAV's own scale, offsets, lengths,
 * optional int16 noise mixing, out [sum F, width] at out_row, optional fp64 copy, ark_decimals).  `preprocess`
 * must be FDLP_PRE_NONE; `jitter` and the compact-code fields are unused.  FDLP_E_CAPACITY past max_frames. */
int fdlp_mfcc_compute(fdlp_mfcc_plan* plan, const fdlp_batch* batch, void* stream);
/* Host-only view of the plan's tables (works on a device = -1 plan).  dims[8] = {n, nb, K, Kpad, nbpad, ncep,
 * nfilters, frames per workgroup tile}; fold [nfilters, nb] (fb[m,k] + fb[m,n-k]), tw [Kpad, 2 nbpad]
 * (cos | -sin of 2 pi ((i k) mod n) / n, zero padded), dct [nfilters, ncep].  Any of the three may be NULL. */
int fdlp_mfcc_plan_tables(const fdlp_mfcc_plan* plan, int32_t* dims, double* fold, double* tw, double* dct);

/* ---- feature post-processing: apply-cmvn | add-deltas | splice-feats ------------------------ */
/* The chain every consumer of the reference pipes the arks through (recipes/timit/local_pyspeech/decode.sh:84-90,
 * get_Tandem_feats.sh:31-35, make_mfcc_feats.sh:108-118, src/nnet/data_prep_*.py), restated from Kaldi's
 * documented behaviour (transform/cmvn.cc ApplyCmvn, feat/feature-functions.cc DeltaFeatures, SpliceFrames) and
 * run as ONE kernel (fdlp_post.hip): each input row is read once per tile, each output row written once.
 *   cmvn    y = fl32(fl32(x * scale[d]) + offset[d]); the multiply only when the batch sets norm_mul
 *   deltas  block i of frame t = sum_j scales[i][j] * y[clamp(t + j, 0, T-1)], float32, ascending j, taps equal
 *           to zero skipped; block 0 is y itself; columns [y | d | dd | ..] over the first `truncate` columns
 *   splice  row t = rows clamp(t - L, 0, T-1) .. clamp(t + R, 0, T-1) of the above, concatenated
 * A stage that is off (no norm table, delta_order 0, no context) is not executed. */
typedef struct fdlp_post_config {
  int32_t dim;            /* columns of the input rows                                        */
  int32_t truncate;       /* add-deltas --truncate: keep the first n columns (0 = all)        */
  int32_t delta_order;    /* add-deltas --delta-order (0 = no deltas; at most 8)              */
  int32_t delta_window;   /* add-deltas --delta-window (1 .. 999)                             */
  int32_t left_context;   /* splice-feats --left-context                                      */
  int32_t right_context;  /* splice-feats --right-context                                     */
  int32_t device;         /* HIP device; -1 = host-only plan (info and scales only)           */
} fdlp_post_config;
/* A batch of concatenated utterances: utterance u is rows row_off[u] .. row_off[u] + utt_len[u] - 1 of both
 * in_dev [n_rows, dim] and out_dev [n_rows, out_dim] (float32, device).  norm_dev is a device table
 * [n_norm, 2, dim] of float32 (scale row, offset row: fdlp_cmvn_norm) or NULL for no CMVN; norm_index[u]
 * picks utterance u's pair (NULL = pair 0), so per-speaker CMVN shares the launch. */
typedef struct fdlp_post_batch {
  int32_t n_utt;
  int32_t norm_mul;            /* 1: multiply by the scale row (--norm-vars or --reverse with it)   */
  const void* in_dev;
  int64_t n_rows;
  const int64_t* row_off;      /* host [n_utt] */
  const int64_t* utt_len;      /* host [n_utt], every length >= 1 */
  const void* norm_dev;
  int32_t n_norm;
  const int32_t* norm_index;   /* host [n_utt] or NULL */
  void* out_dev;
} fdlp_post_batch;
typedef struct fdlp_post_plan fdlp_post_plan;
/* FDLP_E_INVALID (the message names the sizes) when one frame per tile does not fit the 160 KB LDS. */
int fdlp_post_plan_create(const fdlp_post_config* cfg, fdlp_post_plan** out);
int fdlp_post_plan_destroy(fdlp_post_plan* plan);
/* out_dim = (L + R + 1) * D * (order + 1) with D = truncate or dim; frames per workgroup tile; LDS bytes of a
 * workgroup.  Any pointer may be NULL. */
int fdlp_post_plan_info(const fdlp_post_plan* plan, int32_t* out_dim, int32_t* tile, int32_t* lds_bytes);
/* The delta filters: lens[order + 1] (2 i window + 1) and the tables concatenated in `scales`
 * (sum of lens floats).  scales[0] = [1]; scales[i] is scales[i-1] convolved with j = -window .. window over
 * sum j^2, kept as exact integer numerators over (sum j^2)^i and rounded to float32 once.  Either may be NULL. */
int fdlp_post_plan_scales(const fdlp_post_plan* plan, int32_t* lens, float* scales);
int fdlp_post_compute(fdlp_post_plan* plan, const fdlp_post_batch* batch, void* stream);

/* ---- transform-feats: LDA / fMLLR as the last stage of the chain ---------------------------- */
/* Kaldi's featbin/transform-feats (decode.sh:90 and :116-119, get_Tandem_feats.sh:33-36, the transform-feats
 * strings of src/nnet/data_prep_*.py), restated from its documented behaviour and fused after the splice in the
 * same kernel launch (xform_kernel, fdlp_post.hip): the spliced rows stay in LDS and are the A operand of a
 * float32 MFMA GEMM (v_mfma_f32_16x16x4_f32, exact float32).  With K = fdlp_post_plan_info's out_dim of `post`:
 *   linear  (affine 0, M [out_dim, K])      out = row M^T
 *   affine  (affine 1, M [out_dim, K + 1])  out = row M[:, :K]^T + M[:, K]
 * Every result is one chain acc = fmaf(row[k], M[n][k], acc) from acc = 0 that visits k in the fixed order
 * "for g = 0, 16, ..: for s = 0 .. 3: for q = 0 .. 3: k = g + 4 q + s" (k >= K skipped), then (affine) one float32
 * add of M[n][K]: a function of K alone, so a row's result does not depend on the batch, on the tile or on where
 * its utterance lies.  Kaldi leaves the summation order to its BLAS; the average-logdet log line is not
 * reproduced.  With every stage of `post` off this is the stand-alone transform-feats. */
#define FDLP_XFORM_MAX_OUT_DIM 65536
typedef struct fdlp_xform_config {
  fdlp_post_config post;  /* the stages before the transform (post.device is the plan's device) */
  int32_t out_dim;        /* N, rows of the transform matrix: 1 .. FDLP_XFORM_MAX_OUT_DIM          */
  int32_t affine;         /* 1: the matrices have K + 1 columns, the last one the offset          */
} fdlp_xform_config;
typedef struct fdlp_xform_plan fdlp_xform_plan;
/* FDLP_E_INVALID (the message names the sizes) when out_dim is out of range or one frame per tile, with the
 * staged matrix chunk beside it, does not fit the 160 KB LDS. */
int fdlp_xform_plan_create(const fdlp_xform_config* cfg, fdlp_xform_plan** out);
int fdlp_xform_plan_destroy(fdlp_xform_plan* plan);
/* in_dim = K, the row width entering the transform; out_dim = N; mat_cols = K + affine; frames per workgroup
 * tile; LDS bytes of a workgroup.  Works on a host-only plan (post.device = -1).  Any pointer may be NULL. */
int fdlp_xform_plan_info(const fdlp_xform_plan* plan, int32_t* in_dim, int32_t* out_dim, int32_t* mat_cols,
                         int32_t* tile, int32_t* lds_bytes);
/* What a compute call of this plan launches, from the function the launcher itself selects by:
 *   info[0] mode     delta stage of the code object: -1 none, 0 any order and window, 1 and 2 = that order at window 2
 *   info[1] ncb      16-column blocks of the result a wave accumulates at once: min(ceil(out_dim / 16), 4)
 *   info[2] groups   column groups of 16 ncb the kernel loops over
 *   info[3] tile     frames per workgroup
 *   info[4] vec      1: the rows are read from LDS 16 bytes at a time (D (order + 1) a multiple of 4)
 *   info[5], [6]     K = 32 info[5] + info[6]: full chunks of the staged matrix, and the length of the tail chunk
 *   info[7]          1: the launch asks for more than 64 KB of dynamic LDS and raises the kernel's limit first
 * xform_kernel<mode, ncb> is one of 16 code objects.  Works on a host-only plan. */
int fdlp_xform_plan_dispatch(const fdlp_xform_plan* plan, int32_t info[8]);
/* `batch` as for fdlp_post_compute, except that out_dev is [n_rows, out_dim].  mat_dev: device table
 * [n_mat, out_dim, mat_cols] of float32; mat_index[u] (host, or NULL = matrix 0) picks utterance u's matrix, so
 * per-speaker fMLLR shares the launch. */
int fdlp_xform_compute(fdlp_xform_plan* plan, const fdlp_post_batch* batch, const void* mat_dev, int32_t n_mat,
                       const int32_t* mat_index, void* stream);

/* ---- extract-posterior: the feed-forward acoustic model after the chain --------------------- */
/* nnetFeedforward of the reference (src/nnet/nnet_models.py:9-31; extract_posterior.py, compute_per_utt_fer.py):
 * n_linear nn.Linear layers with ReLU between them, on the rows the stages of `post` give.  With x_0 the row
 * (width dims[0]) and W_l [dims[l+1], dims[l]], b_l [dims[l+1]] in nn.Linear's layout:
 *     y_l = f_l(x_l) W_l^T + b_l,   f_0 the identity, f_l = max(x, 0) for l > 0,   x_{l+1} = y_l
 * so every layer stores its PRE-activation, which is what the reference taps (embeds.append before the ReLU).
 * Layer 0 runs in the chain's own kernel launch as an affine transform ([W_0 | b_0], xform_kernel: the spliced
 * rows never reach HBM); the others in dense_kernel (fdlp_nnet.hip) on v_mfma_f32_32x32x2_f32, exact float32.
 * Each y_l[n] of a dense layer is one chain acc = fmaf(f(x[k]), W[n][k], acc) from acc = +0 over
 *     for g = 0, 8, 16, .. < ceil(K / 32) 32:  for i = 0 .. 3:  k = g + i, then k = g + 4 + i
 * (a k >= K contributes fmaf(+0, +0, acc)), then one float32 add of b[n]; layer 0 follows the order documented
 * for fdlp_xform_config.  Both are functions of K alone: a row's bits do not depend on the batch, on the row's
 * position or on the rows beside it.
 * The row epilogue, on the last layer's logits x [C] with m = max_j x_j and S = sum_j exp(x_j - m):
 *     FDLP_NNET_SOFTMAX  p_j = exp(x_j - m) / S   (extract_posterior.py --add_softmax; the reference's
 *                        np.exp(X) / sum has no max subtraction and gives NaN above 88: that is not reproduced)
 *     FDLP_NNET_LOGLIKE  ((x_j - m) - log S) - prior_weight * prior[j]   (log_softmax - prior_weight * prior of
 *                        dump_genclassifier_outputs.py:110, what latgen-faster-mapped consumes)
 * A feed-forward net is the linear-only stage plan: fdlp_nnet_* is a front over fdlp_rnn_* (below) with the stages
 * FDLP_RNN_LINEAR_RELU x (n_linear - 1), FDLP_RNN_LINEAR, no group table and no limit on the utterances of a batch.
 * The launches, the evaluation order and the checks are that plan's. */
#define FDLP_NNET_MAX_LINEAR 32   /* <= FDLP_RNN_MAX_STAGES */
enum { FDLP_NNET_RAW = 0, FDLP_NNET_SOFTMAX = 1, FDLP_NNET_LOGLIKE = 2 };
typedef struct fdlp_nnet_config {
  fdlp_post_config post;                    /* the stages before the network (post.device is the plan's device) */
  int32_t n_linear;                         /* linear layers: 1 .. FDLP_NNET_MAX_LINEAR                          */
  int32_t dims[FDLP_NNET_MAX_LINEAR + 1];   /* dims[0] = the stages' out_dim, dims[l+1] = outputs of layer l     */
} fdlp_nnet_config;
typedef struct fdlp_nnet_plan fdlp_nnet_plan;
/* weights[l] / biases[l]: host float32 [dims[l+1], dims[l]] / [dims[l+1]], copied to the device (the plan owns the
 * copies; both may be NULL for a host-only plan).  The plan allocates two [max_rows, max hidden width] float32
 * workspaces the layers ping-pong between (none with one layer).  FDLP_E_INVALID with the sizes in the message for
 * n_linear outside its range, a dimension < 1, dims[0] different from the stages' out_dim, max_rows < 1, or a
 * layer 0 that does not fit the LDS beside the chain's tile. */
int fdlp_nnet_plan_create(const fdlp_nnet_config* cfg, const float* const* weights, const float* const* biases,
                          int64_t max_rows, fdlp_nnet_plan** out);
int fdlp_nnet_plan_destroy(fdlp_nnet_plan* plan);
/* in_dim = dims[0]; n_linear; out_dims[n_linear] = dims[1 ..]; bytes of the two workspaces together; tile[3] = row
 * tile, column tile and k chunk of dense_kernel; its LDS bytes at the full column tile.  Works on a host-only plan.
 * Any pointer may be NULL. */
int fdlp_nnet_plan_info(const fdlp_nnet_plan* plan, int32_t* in_dim, int32_t* n_linear, int32_t* out_dims,
                        int64_t* workspace_bytes, int32_t* tile, int32_t* lds_bytes);
/* `batch` as for fdlp_post_compute (n_rows <= max_rows, else FDLP_E_CAPACITY).  tap 0: the last layer's output;
 * tap l in 1 .. n_linear - 1: the pre-activation of hidden layer n_linear - l (counted from 1), the reference's
 * embeds[-l].  out_dev is [n_rows, width of the tapped layer]; layers after the tap are not computed.  mode: raw,
 * or with tap 0 softmax / loglike; loglike needs prior_dev (device float32 [C]).  Rows of the batch that belong to
 * no utterance are left alone when layer 0 is tapped and hold unspecified values otherwise. */
int fdlp_nnet_compute(fdlp_nnet_plan* plan, const fdlp_post_batch* batch, int32_t tap, int32_t mode,
                      const void* prior_dev, float prior_weight, void* stream);

/* ---- dump-genclassifier-outputs: GRU acoustic models after the chain -------------------------- */
/* The recurrent models of the reference's hybrid recipes (src/nnet/nnet_models.py nnetRNN and the classifier
 * branch of nnetAEClassifierMultitask; dump_genclassifier_outputs.py) as a list of stages on the rows the stages
 * of `post` give.  Stage s maps rows of width dims[s] to rows of width dims[s+1]:
 *   FDLP_RNN_GRU          nn.GRU (one layer, gate order r, z, n): W_ih [3H, K], W_hh [3H, H], b_ih, b_hh [3H]
 *   FDLP_RNN_LINEAR       y = x W^T + b, W [N, K] (a Conv1d of kernel size 1, squeezed)
 *   FDLP_RNN_LINEAR_RELU  the same; the ReLU is applied when the NEXT stage loads the output, so a tap gives the
 *                         pre-activation (the encoder's bottleneck)
 * A GRU stage is two launches: the input projection G = x W_ih^T + b_ih of all rows at once (stage 0: inside the
 * chain's launch as the affine transform [W_ih | b_ih], so the spliced rows never reach HBM; later stages:
 * dense_kernel, its chain order above), then gru_scan_kernel (fdlp_nnet.hip), one workgroup per group of up to
 * group_utts = 32 utterances, which are the M dimension of v_mfma_f32_32x32x2_f32.  Per utterance, h_{-1} = 0 and
 *     acc_c[j] = the chain fmaf(h_{t-1}[k], W_hh[c H + j][k], acc) from acc = +0 over
 *                for g = 0, 8, 16, .. < ceil(H / 16) 16:  for i = 0 .. 3:  k = g + i, then k = g + 4 + i
 *                (a k >= H contributes fmaf(+0, +0, acc)),  c = r, z, n
 *     a_r = G_r[t][j] + (acc_r[j] + b_hr[j])          r = 1 / (1 + exp(-a_r))        and z likewise
 *     a_n = G_n[t][j] + r (acc_n[j] + b_hn[j])        n = tanh(a_n)
 *     h_t[j] = (1 - z) n + z h_{t-1}[j]
 * every operation rounded to float32 as written, exp and tanh the device library's float32 functions, the division
 * correctly rounded.  Order and operations depend on H alone, so an utterance's bits do not depend on its group,
 * its slot, the other utterances' lengths or the batch.  Utterances are sorted by length (descending, stable) and
 * cut into groups of group_utts; a workgroup walks t up to the longest length of its group and depends on no other
 * workgroup.  Sizing: a step of a full group is 2 x 32 x 3H x H flop of float32 MFMA and re-reads the 12 H^2 bytes
 * of W_hh from L2; a batch of n utterances keeps ceil(n / 32) CUs busy; H is limited by the 160 KB LDS (two
 * [32, H] state buffers beside the W_hh chunks) to 384. */
#define FDLP_RNN_MAX_STAGES 32
enum { FDLP_RNN_GRU = 0, FDLP_RNN_LINEAR = 1, FDLP_RNN_LINEAR_RELU = 2 };
typedef struct fdlp_rnn_config {
  fdlp_post_config post;                    /* the stages before the model (post.device is the plan's device)   */
  int32_t n_stages;                         /* 1 .. FDLP_RNN_MAX_STAGES                                          */
  int32_t kind[FDLP_RNN_MAX_STAGES];
  int32_t dims[FDLP_RNN_MAX_STAGES + 1];    /* dims[0] = the post stages' out_dim, dims[s+1] = outputs of stage s */
} fdlp_rnn_config;
typedef struct fdlp_rnn_plan fdlp_rnn_plan;
/* params: 4 host float32 pointers per stage, {w_ih, w_hh, b_ih, b_hh} for a GRU and {w, NULL, b, NULL} otherwise,
 * copied to the device (may be NULL for a host-only plan).  The plan allocates one [max_rows, 3 max H] buffer for G
 * (max H over the GRU stages), two [max_rows, widest of dims[1 .. n_stages - 1]] buffers the stages ping-pong
 * between, and the group table of ceil(max_utts / 32) groups of 32 slots of 16 bytes.  FDLP_E_INVALID with the
 * numbers in the message for n_stages outside its range, an unknown kind, a dimension < 1, dims[0] different from
 * the post stages' out_dim, max_rows < 1, max_utts < 1, or a GRU too wide for the LDS. */
int fdlp_rnn_plan_create(const fdlp_rnn_config* cfg, const float* const* params, int64_t max_rows, int32_t max_utts,
                         fdlp_rnn_plan** out);
int fdlp_rnn_plan_destroy(fdlp_rnn_plan* plan);
/* in_dim = dims[0]; n_stages; out_dims[n_stages] = dims[1 ..]; the bytes of the workspaces above together;
 * group_utts = 32; the LDS bytes of gru_scan_kernel at the plan's widest GRU (0 without one).  Works on a host-only
 * plan.  Any pointer may be NULL. */
int fdlp_rnn_plan_info(const fdlp_rnn_plan* plan, int32_t* in_dim, int32_t* n_stages, int32_t* out_dims,
                       int64_t* workspace_bytes, int32_t* group_utts, int32_t* lds_bytes);
/* The group table of a batch with these lengths (each >= 1): utterance u is slot slot_of[u] of group group_of[u],
 * *n_groups = ceil(n_utts / 32).  Host only. */
int fdlp_rnn_plan_groups(const fdlp_rnn_plan* plan, const int32_t* lengths, int32_t n_utts, int32_t* group_of,
                         int32_t* slot_of, int32_t* n_groups);
/* `batch` as for fdlp_post_compute, with n_utt <= max_utts (FDLP_E_INVALID), n_rows <= max_rows (FDLP_E_CAPACITY)
 * and utterances that do not overlap.  tap s: the output of stage n_stages - 1 - s, [n_rows, its width] in out_dev;
 * later stages are not computed.  mode as for fdlp_nnet_compute (FDLP_NNET_RAW, or with tap 0 SOFTMAX / LOGLIKE).
 * Rows that belong to no utterance hold unspecified values or are left alone. */
int fdlp_rnn_compute(fdlp_rnn_plan* plan, const fdlp_post_batch* batch, int32_t tap, int32_t mode,
                     const void* prior_dev, float prior_weight, void* stream);
/* Per-kernel times of the plan's computes since the last call, from HIP events recorded around every launch while
 * `on` (fdlp_rnn_set_profiling): ms[0] the input projections and linear stages, ms[1] the scans.  fdlp_rnn_times
 * waits for the recorded work. */
int fdlp_rnn_set_profiling(fdlp_rnn_plan* plan, int32_t on);
int fdlp_rnn_times(fdlp_rnn_plan* plan, double* ms);

/* ---- dump-multimod-outputs: multi-stream GRU models after n_streams chains -------------------- */
/* nnetRNNMultimod of the reference (src/nnet/nnet_models.py:92-161; dump_multimod_outputs.py): stream s, the rows
 * of its own chain post[s] (its own cmvn and splice; every stream gives in_dim columns), runs through sub-network s,
 * n_sub_layers nn.GRU of hidden_sub = Hs units; the M = n_streams outputs side by side, [rows, M Hs], run through
 * n_trunk_layers nn.GRU of M Hs units and the regression [n_classes, M Hs].  Every GRU is the stage of fdlp_rnn_*
 * above, bit for bit: layer 0's projection inside its stream's chain launch, later projections in dense_kernel, the
 * scan in gru_scan_kernel.  The M scans of a sub-network layer are ONE launch on the grid (groups, streams), so a
 * batch of n utterances keeps M ceil(n / 32) CUs busy there; the last sub-network layer writes stream s at column
 * s Hs of the concatenated buffer (row stride M Hs), which is never assembled by a copy.  The streams' pointers
 * travel in the kernel arguments, at most FDLP_MMOD_MAX_STREAMS of them.  An utterance's bits in stream s depend on
 * Hs and that utterance's rows of stream s alone.  The trunk's width is limited like any GRU's: M Hs <= 384. */
#define FDLP_MMOD_MAX_STREAMS 8
typedef struct fdlp_mmod_config {
  int32_t n_streams;                              /* 1 .. FDLP_MMOD_MAX_STREAMS                                   */
  fdlp_post_config post[FDLP_MMOD_MAX_STREAMS];   /* per stream; post[0].device is the plan's device              */
  int32_t in_dim;                                 /* the width every stream's chain must give                      */
  int32_t n_sub_layers, hidden_sub;               /* >= 1 (at most FDLP_RNN_MAX_STAGES layers)                      */
  int32_t n_trunk_layers;                         /* 0 .. FDLP_RNN_MAX_STAGES                                      */
  int32_t n_classes;
} fdlp_mmod_config;
typedef struct fdlp_mmod_plan fdlp_mmod_plan;
/* params: host float32 pointers in nn.GRU's layout, copied to the device (may be NULL for a host-only plan):
 * {w_ih, w_hh, b_ih, b_hh} of sub-network 0's layers, then sub-network 1's, ..; then of the trunk's layers; then the
 * regression's {w [n_classes, M Hs], b}: 4 (M n_sub_layers + n_trunk_layers) + 2 pointers.  The plan allocates five
 * [max_rows, M Hs] float32 buffers (three hold the projections, two the layers' outputs) and the group table of
 * ceil(max_utts / 32) groups.  FDLP_E_INVALID with the numbers in the message for n_streams outside its range, a
 * stream whose chain gives another width than in_dim (the message names the stream), Hs or M Hs above the widest GRU
 * the LDS holds (the message names M Hs and that limit), a dimension < 1, max_rows < 1 or max_utts < 1. */
int fdlp_mmod_plan_create(const fdlp_mmod_config* cfg, const float* const* params, int64_t max_rows,
                          int32_t max_utts, fdlp_mmod_plan** out);
int fdlp_mmod_plan_destroy(fdlp_mmod_plan* plan);
/* in_dim; n_taps = n_trunk_layers + 2; tap_dims[n_taps]; the bytes of the workspaces above together; group_utts =
 * 32; the LDS bytes of gru_scan_kernel at the widest GRU.  Works on a host-only plan.  Any pointer may be NULL. */
int fdlp_mmod_plan_info(const fdlp_mmod_plan* plan, int32_t* in_dim, int32_t* n_taps, int32_t* tap_dims,
                        int64_t* workspace_bytes, int32_t* group_utts, int32_t* lds_bytes);
/* As fdlp_rnn_plan_groups: the one group table all streams share.  Host only. */
int fdlp_mmod_plan_groups(const fdlp_mmod_plan* plan, const int32_t* lengths, int32_t n_utts, int32_t* group_of,
                          int32_t* slot_of, int32_t* n_groups);
/* batches[n_streams], each as for fdlp_rnn_compute; all must hold the same n_utt, n_rows, utt_len and row_off
 * (FDLP_E_INVALID names the first utterance that differs), each its own in_dev and norm table.  The output goes to
 * batches[0].out_dev.  tap 0: the logits [n_rows, n_classes] (mode as for fdlp_nnet_compute); tap t in
 * 1 .. n_trunk_layers: trunk GRU n_trunk_layers - t, counted from the end like the other plans' taps; tap
 * n_trunk_layers + 1: the concatenated sub-network outputs; both [n_rows, M Hs], raw. */
int fdlp_mmod_compute(fdlp_mmod_plan* plan, const fdlp_post_batch* batches, int32_t tap, int32_t mode,
                      const void* prior_dev, float prior_weight, void* stream);
/* As fdlp_rnn_set_profiling / fdlp_rnn_times: ms[0] the projections and the regression, ms[1] the scans. */
int fdlp_mmod_set_profiling(fdlp_mmod_plan* plan, int32_t on);
int fdlp_mmod_times(fdlp_mmod_plan* plan, double* ms);

/* ---- compute-vae-encoded-likelihood: VAE-encoded GRU models after the chain -------------------- */
/* src/nnet/compute_vae_encoded_likelihood.py of the reference: a VAE encoder, of which only `means` is kept (the
 * script is deterministic: the sampled decoder output is thrown away), the latent normalised per utterance over time,
 * and nnetRNN on it.  It is the stage plan of fdlp_rnn_* with the stages
 *     encoder | means (FDLP_RNN_LINEAR) | norm | n_cls_layers x FDLP_RNN_GRU | regression (FDLP_RNN_LINEAR)
 * encoder, FDLP_VENC_RNN (VAEEncoder): n_enc_layers x FDLP_RNN_GRU of enc_hidden units on the in_dim columns the
 *   stages of `post` give; stage 0's projection runs inside the chain's launch, as in fdlp_rnn_*.
 * encoder, FDLP_VENC_CNN (VAECNNEncoderNopool): n_conv same-padded nn.Conv2d + ReLU, channels[l] -> channels[l+1],
 *   kernel (kh, kw), both odd, over the (feat_h x time) image of the utterance; channels[0] = 1 and the chain must give
 *   feat_h columns.  Rows are [t][c feat_h + f], channel-major, so the last layer's rows are the reference's
 *   view(B, -1, T) flattening and `means` is a plain linear stage of K = channels[n_conv] feat_h.  A layer is one
 *   launch of conv2d_same_kernel (fdlp_vaeenc.hip), an implicit GEMM on v_mfma_f32_32x32x2_f32:
 *       out[t][co F + f] = b[co] + sum_{ci,dh,dw} g(in[t + dw - pw][ci F + f + dh - ph]) W[co][ci][dh][dw]
 *   ph = (kh-1)/2, pw = (kw-1)/2, g the identity for the first layer and max(x, 0) for the others (ReLU on load: a tap
 *   gives the pre-activation); taps outside 0 <= f' < F or outside the utterance's own 0 <= t' < T are zero.  Every
 *   output is dense_kernel's fmaf chain (above) at K = Ci kh kw, k the flat index of W[co] in torch's (ci, dh, dw)
 *   layout, a padded tap a zero operand, the bias one add at the end: the bits of dense_kernel on the im2col rows.
 *   They depend on the layer's shape alone, not on the tile, the utterance's place in the batch, or the batch.
 * norm (utt_norm_kernel), per utterance and column of the latent, t ascending:
 *       m = float32((sum_t z_t in float64) / T),  d_t = z_t - m (float32),  md = (sum_t d_t in float64) / T,
 *       v = float32((sum_t (d_t - md)^2 in float64) / (T - 1)),  out_t = d_t / sqrtf(v)
 *   sqrt and division correctly rounded; the order depends on T alone.  T = 1 or a constant column gives what IEEE
 *   gives (NaN), as the reference does.
 * The GRU scan's limit (384 hidden units) holds for enc_hidden and cls_hidden. */
#define FDLP_VENC_MAX_CONV 8
enum { FDLP_VENC_RNN = 0, FDLP_VENC_CNN = 1 };
typedef struct fdlp_venc_config {
  fdlp_post_config post;                        /* the stages before the model (post.device is the plan's device) */
  int32_t arch;                                 /* FDLP_VENC_RNN or FDLP_VENC_CNN                                  */
  int32_t in_dim, n_enc_layers, enc_hidden;     /* RNN encoder: the first GRU's input width, layers, units         */
  int32_t n_conv;                               /* CNN encoder: 1 .. FDLP_VENC_MAX_CONV layers                     */
  int32_t channels[FDLP_VENC_MAX_CONV + 1];     /*   channels[0] = 1, channels[l + 1] = outputs of layer l         */
  int32_t kh, kw, feat_h;                       /*   kernel (feature, time), both odd; image height                */
  int32_t latent_dim;                           /* outputs of `means`                                              */
  int32_t n_cls_layers, cls_hidden, n_classes;  /* nnetRNN                                                         */
} fdlp_venc_config;
typedef struct fdlp_venc_plan fdlp_venc_plan;
/* params: 4 host float32 pointers per stage in stage order, as for fdlp_rnn_plan_create; a convolution is
 * {w [Co, Ci, kh, kw], NULL, b [Co], NULL}, the norm stage four NULLs.  The plan allocates the G buffer and the group
 * table of fdlp_rnn_plan_create and two [max_rows, widest stage input] buffers the stages ping-pong between, which
 * for the CNN encoder is max_l channels[l] feat_h.  FDLP_E_INVALID with the numbers in the message for an even kh or
 * kw, channels[0] != 1, a chain whose out_dim differs from feat_h (CNN) or in_dim (RNN), a GRU wider than the scan's
 * limit, a convolution whose staged patch and chunks exceed the 160 KB LDS, and what fdlp_rnn_plan_create refuses.
 * The name is an exception to the <family>_plan_create pattern of the other fronts, on purpose: the table of
 * create-time refusals in tests/test_plan_errors.py claims a row of its own for every exported *_plan_create, and
 * this front's rows live with its other tests (tests/test_vaeenc.py, CREATE_CASES).  Renaming it to
 * fdlp_venc_plan_create means moving those rows into that table in the same change. */
int fdlp_venc_create(const fdlp_venc_config* cfg, const float* const* params, int64_t max_rows,
                          int32_t max_utts, fdlp_venc_plan** out);
int fdlp_venc_plan_destroy(fdlp_venc_plan* plan);
/* As fdlp_rnn_plan_info, with lds_bytes[2]: gru_scan_kernel at the widest GRU, conv2d_same_kernel at its largest
 * layer (0 for the RNN encoder).  Works on a host-only plan.  Any pointer may be NULL. */
int fdlp_venc_plan_info(const fdlp_venc_plan* plan, int32_t* in_dim, int32_t* n_stages, int32_t* out_dims,
                        int64_t* workspace_bytes, int32_t* group_utts, int32_t* lds_bytes);
/* As fdlp_rnn_plan_groups.  Host only. */
int fdlp_venc_plan_groups(const fdlp_venc_plan* plan, const int32_t* lengths, int32_t n_utts, int32_t* group_of,
                          int32_t* slot_of, int32_t* n_groups);
/* As fdlp_rnn_compute: tap s is the output of stage n_stages - 1 - s, mode applies to tap 0. */
int fdlp_venc_compute(fdlp_venc_plan* plan, const fdlp_post_batch* batch, int32_t tap, int32_t mode,
                      const void* prior_dev, float prior_weight, void* stream);
/* As fdlp_rnn_set_profiling / fdlp_rnn_times with ms[3]: ms[0] the projections, linear stages and the normaliser,
 * ms[1] the scans, ms[2] the convolutions. */
int fdlp_venc_set_profiling(fdlp_venc_plan* plan, int32_t on);
int fdlp_venc_times(fdlp_venc_plan* plan, double* ms);

/* ---- compute-lifelong-likelihood, compute-incremental-likelihood: after the logits of D model pairs ---------- */
/* src/nnet/compute_lifelong_likelihood.py and compute_incremental_likelihood.py of the reference run D (nnetRNN,
 * nnetVAE) pairs on one feature stream and fuse the D posterior streams with per-utterance task weights.  The forward
 * passes are fdlp_rnn_* plans (the classifiers in mode FDLP_NNET_SOFTMAX); these four stateless calls are everything
 * after them (kernels of fdlp_lifelong.hip).  They work on the CURRENT device, on `stream`, and return at once.
 * post is [n_models, n_rows, n_classes] float32; row_off and utt_len are DEVICE int64 [n_utt] tables (utterance u is
 * rows row_off[u] .. row_off[u] + utt_len[u] - 1; the caller uploads them once for the calls of a batch).  Every
 * float64 operation is rounded as written, and every sum runs in an order fixed by the utterance's length T,
 * n_classes = C and n_models = D alone: no result depends on the utterance's place in the batch or on the batch.
 *
 * fdlp_life_mmeasure (mmeasure_kernel), mmeasure_loss of the scripts, per (utterance, model) into out [n_utt, D]
 * float64.  P [T, C] the posteriors; for d in (5, 25, 45, 65): X = P[d:], Y = P[:-d], n = max(T - d, 0), lx = log X
 * and ly = log Y the float64 logarithms of the float32 values, dl = lx - ly:
 *     S1_d = sum (X dl - Y dl)       sym_kld's two sums pair by pair: (X - Y)(lx - ly), with a NaN for a zero on either side
 *     S2_d = sum X (lx - Y)          nn.KLDivLoss()(P[:-d], P[d:]) as written there: the input NOT in log space
 *     M = (sum_d (S1_d / n + S2_d / (n C))) / 4,   d ascending from 0.0
 * T <= 65 gives 0 / 0 = NaN and a posterior that underflowed to 0 gives NaN, as the reference does.  Order of a sum:
 * t ascending per column; the columns of a tile of 64 ascending; the tiles ascending.  Every posterior is read once
 * (an LDS ring of the last rows of a 64-column tile, p and log p).  At most 65535 utterances per call.
 *
 * fdlp_life_vae_sample (vae_sample_kernel), latentSampler: z [n_rows, bn] = mu + expf(sigma) eps in float32, the
 * product and the sum each rounded; ml [n_rows, 2 bn] holds mu, then sigma; eps [n_rows, bn] is the caller's noise.
 *
 * fdlp_life_vae_elbo (vae_elbo_kernel), vae_loss per row of x, xhat [n_rows, in_dim] and ml, all sums float64:
 *     elbo[r] = float32( (sum_k (-0.5 (x - xhat)^2 - 0.5 log(2 pi))) / in_dim
 *                        + 0.5 ((sum_j (1 - mu^2 - exp(sigma)^2 + 2 sigma)) / bn) )
 * (a lane of the row's wave adds k = lane, lane + 64, ..; the lanes are added by the xor butterfly 32, 16, .., 1), then
 * per utterance, t ascending in float64, out[u ld_out] = mean_t elbo (FDLP_LIFE_LIFELONG) or mean_t expf(elbo)
 * (FDLP_LIFE_INCREMENTAL).  elbo [n_rows] float32 is an output too.
 *
 * fdlp_life_fuse (lifelong_fuse_kernel): out [n_rows, C] float32 from post, w [n_utt, D] float64 and tab [D, C]
 * float64, all arithmetic float64, i ascending from 0.0, rounded to float32 once, IEEE special values as they fall:
 *     FDLP_LIFE_LIFELONG     out[t][c] = log(sum_i P_i[t][c] w[u][i]) - prior_weight log(sum_i tab_i[c] w[u][i]),
 *                            tab = exp(prior)
 *     FDLP_LIFE_INCREMENTAL  out[t][c] = (sum_i (log P_i[t][c] - prior_weight tab_i[c]) w[u][i]) / D,  tab = prior
 * max_len: the longest utterance of the batch (it sizes the grid).  Rows of no utterance are left alone.
 * FDLP_E_INVALID for a count outside its range or a null pointer. */
#define FDLP_LIFE_MAX_MODELS 8
enum { FDLP_LIFE_LIFELONG = 0, FDLP_LIFE_INCREMENTAL = 1 };
int fdlp_life_mmeasure(const float* post_dev, int32_t n_models, int64_t n_rows, int32_t n_classes, int32_t n_utt,
                       const int64_t* row_off_dev, const int64_t* utt_len_dev, double* out_dev, void* stream);
int fdlp_life_vae_sample(const float* ml_dev, const float* eps_dev, float* z_dev, int64_t n_rows, int32_t bn,
                         void* stream);
int fdlp_life_vae_elbo(const float* x_dev, const float* xhat_dev, const float* ml_dev, int64_t n_rows, int32_t in_dim,
                       int32_t bn, int32_t n_utt, const int64_t* row_off_dev, const int64_t* utt_len_dev, int32_t mode,
                       float* elbo_dev, double* out_dev, int32_t ld_out, void* stream);
int fdlp_life_fuse(const float* post_dev, int32_t n_models, int64_t n_rows, int32_t n_classes, int32_t n_utt,
                   int64_t max_len, const int64_t* row_off_dev, const int64_t* utt_len_dev, const double* w_dev,
                   const double* tab_dev, double prior_weight, int32_t mode, float* out_dev, void* stream);

/* ApplyCmvn / ApplyCmvnReverse as two float32 vectors: out[0 .. dim) = scale, out[dim .. 2 dim) = offset, from the
 * [2, dim + 1] double stats compute-cmvn-stats writes (count = stats[dim]; count < 1 is FDLP_E_INVALID).
 * mean = s0/count; norm_vars: var = s1/count - mean^2 floored at 1e-20 (a warning on stderr), scale = 1/sqrt(var),
 * offset = -mean * scale (a non-finite scale is FDLP_E_INVALID); reverse: scale = sqrt(var) (or 1), offset = mean;
 * skip_dims columns get scale 1, offset 0; norm_vars without norm_means is FDLP_E_INVALID; neither gives the
 * identity.  Host only. */
int fdlp_cmvn_norm(const double* stats, int32_t dim, int32_t norm_means, int32_t norm_vars, int32_t reverse,
                   const int32_t* skip_dims, int32_t n_skip, float* out);

/* ---- augmentation: addReverb (features.py:110-115) -------------------------------------- */
/* --add_reverb small_room|medium_room|large_room (computeFDLPSpectrogram.py:75-91, :168-170): after the
 * optional diff / noise preprocessing, every utterance is convolved with the RIR (channel 1 of
 * ./RIR/<room>.wav / 2^15) and re-aligned on the argmax of np.correlate(x, y, 'valid').  Writes the
 * fp64 signals to out_dev at the same offsets as the input (feed them to fdlp_compute as
 * FDLP_PCM_F64 with preprocess NONE and no noise) and their lengths to out_len (T, or T-1 in the
 * reference's edge case of a best shift of R-1).  Synchronous: waits for `stream` to return the
 * lengths. */
typedef struct fdlp_reverb_batch {
  int32_t n_utt;
  int32_t pcm_kind;              /* FDLP_PCM_I16 | FDLP_PCM_F64 (f64: no preprocessing)            */
  const void* pcm_dev;
  const int64_t* pcm_off;        /* host [n_utt] */
  const int64_t* utt_len;        /* host [n_utt] */
  int32_t preprocess;            /* FDLP_PRE_DIFF or FDLP_PRE_NONE (int16 input only)              */
  const int16_t* noise_dev;      /* nullable: x = s + alpha * noise[off:off+T] before the reverb    */
  const int64_t* noise_off;      /* host [n_utt] */
  const double* noise_alpha;     /* host [n_utt] */
  const double* rir_dev;         /* device [rir_len] */
  int32_t rir_len;
  double* out_dev;               /* device f64, indexed like pcm_dev                              */
  int64_t* out_len;              /* host [n_utt] */
} fdlp_reverb_batch;
int fdlp_reverb(const fdlp_reverb_batch* batch, void* stream);

/* ---- global CMVN statistics (the step after feature extraction) ------------------------- */
/* Kaldi `compute-cmvn-stats scp:feats.scp cmvn.ark` (e2e/wsj/run_fdlp_e1.sh:280; reverb :224,
 * chime4 :193): AccCmvnStats (Kaldi transform/cmvn.cc) over `rows` feature rows [rows, dim] float32
 * on the device, ADDED into stats_dev [2, dim+1] fp64 (row 0: sum x_d, then the frame count;
 * row 1: sum of the float32 products x_d*x_d, then 0).  Deterministic (fixed-order reduction). */
int fdlp_cmvn_accumulate(const float* feats_dev, int64_t rows, int32_t dim, double* stats_dev,
                         void* stream);

/* ---- the path's device transcendental functions (for accuracy tests) ------------------------ */
/* y_dev[i] = fn(x_dev[i]) for n fp64 values on the device, with the function the path itself uses:
 * FDLP_FN_LOG the OLA stage's log of its clipped sums (computeFDLPSpectrogram.py:227 np.log; x > 0, NaN /
 * +inf pass through; a table + polynomial form within ~0.5 ulp, fdlp_device.h ola_log), FDLP_FN_EXP the
 * envelope's exp (:204-205 np.exp; the device library's exp).  ABI 8. */
enum { FDLP_FN_LOG = 0, FDLP_FN_EXP = 1 };
int fdlp_device_fn(int32_t fn, const double* x_dev, double* y_dev, int64_t n, void* stream);

/* ---- host-side RNG replicas (no device work) --------------------------------------------- */
/* CPython `random` (MT19937, init_by_array seeding, randrange(2) = getrandbits(2) with
 * rejection) -- the jitter source of computeFDLPSpectrogram.py:21,225. */
typedef struct fdlp_pyrandom fdlp_pyrandom;
int fdlp_pyrandom_create(const uint32_t* key, int32_t key_len, fdlp_pyrandom** out);
int fdlp_pyrandom_randbits2(fdlp_pyrandom* rng, int64_t n, uint8_t* out);
int fdlp_pyrandom_destroy(fdlp_pyrandom* rng);
/* numpy legacy RandomState: seed(int) = init_genrand; rand() = 53-bit double
 * (features.py:25 noise offset). */
typedef struct fdlp_nprandom fdlp_nprandom;
int fdlp_nprandom_create(uint32_t seed, fdlp_nprandom** out);
int fdlp_nprandom_rand(fdlp_nprandom* rng, int64_t n, double* out);
int fdlp_nprandom_destroy(fdlp_nprandom* rng);
/* (offset, alpha) of add_noise_to_wav (features.py:24-31) given the uniform draw u:
 * energies from int16-wrapped squares exactly like the reference. */
int fdlp_noise_params(const int16_t* sig, int64_t T, const int16_t* noise, int64_t noise_len,
                      double snr, double u, int64_t* off, double* alpha);
/* scipy.io.wavfile.read's dtype of a WAV's samples (ABI 9; fdlp_wav_kind): 8-bit PCM -> uint8, 16 -> int16,
 * 24/32 -> int32 (24-bit left-justified), 40..64 -> int64, IEEE float 32 / 64. */
enum { FDLP_SIG_U8 = 1, FDLP_SIG_I16 = 2, FDLP_SIG_I32 = 3, FDLP_SIG_I64 = 4, FDLP_SIG_F32 = 5, FDLP_SIG_F64 = 6 };
/* The same for a signal of any of those dtypes, given as the double values of scipy's array (ABI 9): the
 * reference squares the signal in its own dtype (integer squares wrap, float32 squares round to float32) and
 * np.mean sums them like numpy (8192-element chunks, pairwise inside a chunk; float32 accumulated in float32),
 * features.py:27.  The noise is int16 (noises/<name>.wav of the recipes). */
int fdlp_noise_params_any(const double* sig, int64_t T, int32_t sig_kind, const int16_t* noise,
                          int64_t noise_len, double snr, double u, int64_t* off, double* alpha);

/* computeMfccFeatures.py's own add_noise_to_wav (:48-55): signal and noise are divided by 2^15 into float64
 * before the energies are taken, so no square wraps (unlike the two functions above).  `sig` holds the WAV's
 * unscaled sample values; the exact 2^-15 scaling cancels in alpha. */
int fdlp_noise_params_f64(const double* sig, int64_t T, const int16_t* noise, int64_t noise_len,
                          double snr, double u, int64_t* off, double* alpha);

/* ---- native I/O (replaces scipy.io.wavfile.read :139 and dict2Ark + copy-feats :231) ---- */
/* Parse a RIFF/WAVE PCM16 mono buffer.  *samples points into `buf`. */
int fdlp_wav_parse(const uint8_t* buf, int64_t len, int32_t* srate, int32_t* channels,
                   const int16_t** samples, int64_t* n_samples);
/* Any RIFF/RIFX WAVE buffer scipy.io.wavfile.read accepts (PCM 1-64 bit, <= 8 bit unsigned, 3/5/6/7-byte
 * containers left-justified; IEEE float 32/64; WAVE_FORMAT_EXTENSIBLE): sample rate, channels, frames, and
 * *is_int16 = 1 when scipy would return little-endian int16 (the samples can be used in place, fdlp_wav_parse),
 * 2 for big-endian (RIFX) int16 (decode; the values are int16), 0 otherwise.  With out != NULL the interleaved samples are written as
 * the double values of scipy's array (ABI 3). */
int fdlp_wav_decode(const uint8_t* buf, int64_t len, int32_t* srate, int32_t* channels, int32_t* is_int16,
                    int64_t* n_samples, double* out);
/* FDLP_SIG_* kind of the samples scipy.io.wavfile.read returns for this buffer (ABI 9). */
int fdlp_wav_kind(const uint8_t* buf, int64_t len, int32_t* kind);
typedef struct fdlp_ark_writer fdlp_ark_writer;
/* Kaldi binary ark + scp ("<utt> <abs ark path>:<offset>") like `copy-feats ark,t:- ark,scp:`.  Written to
 * <path>.tmp and renamed to <path> by fdlp_ark_close (removed instead after a failed write). */
int fdlp_ark_open(const char* ark_path, const char* scp_path, fdlp_ark_writer** out);
int fdlp_ark_write(fdlp_ark_writer* w, const char* utt, const float* mat, int32_t rows,
                   int32_t cols);
int fdlp_ark_close(fdlp_ark_writer* w);
/* Closes the writer and deletes <path>.tmp without publishing: the failure path of a JOB, so its outputs
 * appear complete or not at all (ABI 4). */
int fdlp_ark_abort(fdlp_ark_writer* w);
/* Kaldi matrix reader for `compute-cmvn-stats`-style rspecifiers: "scp:<feats.scp>" (lines
 * "<utt> <ark path>:<offset>") or "ark:<file>" (binary ark, "-" = stdin).  Float ("FM") and double
 * ("DM") binary matrices; data is returned as float32 (double matrices are narrowed, as Kaldi's
 * Matrix<BaseFloat> reader does).  fdlp_mat_reader_next returns 1 with a matrix, 0 at the end,
 * <0 on error; *key and *data stay valid until the next call. */
typedef struct fdlp_mat_reader fdlp_mat_reader;
int fdlp_mat_reader_open(const char* rspecifier, fdlp_mat_reader** out);
int fdlp_mat_reader_next(fdlp_mat_reader* r, const char** key, int32_t* rows, int32_t* cols,
                         const float** data);
int fdlp_mat_reader_close(fdlp_mat_reader* r);
/* Write a double matrix as a Kaldi object file (WriteKaldiObject): binary = "\0B" + "DM " + sizes
 * + row-major fp64, or Kaldi text " [\n  v v ... \n  v v ... ]\n" (%g, the ostream default). */
int fdlp_kaldi_write_dmatrix(const char* path, const double* m, int32_t rows, int32_t cols,
                             int32_t binary);

/* ---- native JOB runner (getFeats' utterance loop, computeFDLPSpectrogram.py:119-237) --------- */
/* One scp shard end to end: reader threads (files, `<cmd> |` pipes, `<ark>:<offset>` wave entries,
 * scipy's WAV formats), the reference's skip / sample-rate semantics, noise offsets and hop jitter from
 * the RNG replicas, device batches of <= batch_frames frames through fdlp_compute (copies and kernels of
 * consecutive batches overlapped), and a writer thread for <outfile>.ark/.scp (and .len), each written
 * to <name>.tmp and renamed when complete.  Progress lines go to stdout like the reference's (:185). */
typedef struct fdlp_job_opts {
  int32_t scp_type;            /* 0 wav, 1 segment (both read natively; no wav-copy needed)           */
  int32_t write_len;           /* --write_utt2num_frames                                               */
  int32_t ark_decimals;        /* '%.3f' text-ark rounding of the reference (3); <0 keeps float32      */
  int32_t batch_frames;        /* analysis frames per device batch (a longer utterance grows the plan) */
  int32_t io_threads;          /* reader threads                                                       */
  int32_t preprocess;          /* FDLP_PRE_NONE | FDLP_PRE_DIFF (--add_noise diff)                     */
  const int16_t* noise;        /* nullable host noise samples (--add_noise <type>,<snr>)              */
  int64_t noise_len;
  double snr;
  uint32_t noise_seed;         /* numpy legacy seed of the noise offsets (np.random.rand, features.py:25) */
  const uint32_t* jitter_key;  /* CPython random.seed key words of the hop jitter (:225)              */
  int32_t jitter_key_len;
  int32_t srate;               /* the sample rate the reference asserts (16000, :144)                 */
  const char* progress_name;   /* non-NULL: "<name>: Computing Features for file: <utt>" per utterance */
  const char* cmvn_path;       /* non-NULL: global CMVN stats (Kaldi binary DM) of the written features */
  int32_t out_mapped;          /* 1: the OLA kernel stores the features straight into the pinned host
                                  slots (no D2H copy); 0 (default): device buffer + D2H copy (ABI 4)   */
  /* ---- ABI 8 ---- */
  int32_t out_codes;           /* D2H leg as int16 ark codes (fdlp_batch.out_q_dev), widened to the
                                  float32 ark values on the host by a thread pool: -1 auto (codes when
                                  0 <= ark_decimals <= 3 and not out_mapped), 0 float32, 1 codes.  A
                                  batch whose codes overflow is copied again as float32 (same arks)  */
  int32_t chunk_rows;          /* feature rows per D2H piece (0: 65536); the writer starts on a batch's
                                  first piece while the rest are still in flight                     */
  int32_t keep_warm;           /* 1: keep the plan, streams and pinned slots of this call for the next
                                  call in the process with the same config (fdlp_job_release frees
                                  them); 0: release them on return                                    */
  const char* trace_path;      /* non-NULL: JSON lines of the JOB's pipeline events (seconds since the
                                  call started; benchmarks/job_timeline.py summarises them)           */
} fdlp_job_opts;
typedef struct fdlp_job_stats {
  int64_t n_lines;             /* scp entries                                  */
  int64_t n_done;              /* utterances featurised                        */
  int64_t n_skipped;           /* unreadable entries skipped (:135-142)         */
  int64_t n_frames_out;        /* feature rows written                         */
  int64_t n_samples;           /* samples featurised                           */
  double seconds;              /* wall time of the call                        */
  double setup_seconds;        /* plan creation, buffers, output files          */
  double read_wait_seconds;    /* consumer waiting for the reader threads       */
  double write_seconds;        /* writer thread busy (ark/scp/len)              */
  double slot_wait_seconds;    /* consumer waiting for a free batch slot        */
  double plan_seconds;         /* fdlp_plan_create (part of setup)              */
  double pinned_seconds;       /* pinned host buffers of the first slot (setup); the
                                  other slots are pinned by a helper thread      */
  /* ---- ABI 8 ---- */
  double d2h_wait_seconds;     /* widening stage waiting for D2H pieces to land  */
  double widen_seconds;        /* widening stage busy (codes -> float32)        */
  int64_t n_batches;           /* device batches                               */
  int64_t n_code_fallbacks;    /* batches copied again as float32 (code overflow) */
  int32_t codes;               /* 1: the D2H leg carried int16 codes            */
  int32_t warm;                /* 1: plan and slots came from the previous call */
} fdlp_job_stats;
int fdlp_job_run(const fdlp_config* cfg, int device, const char* scp_path, const char* outfile,
                 const fdlp_job_opts* opts, fdlp_job_stats* stats);
/* Frees what a keep_warm call parked (plan, streams, pinned and device slots); a no-op when nothing
 * is parked.  Call before destroying the HIP context of the process. */
int fdlp_job_release(void);

#ifdef __cplusplus
}
#endif
#endif /* FDLP_H */
