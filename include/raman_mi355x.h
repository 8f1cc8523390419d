/*
 * raman_mi355x — C ABI of the MI355X (gfx950) Raman-denoising inference engine.
 *
 * Plain pointers and sizes only: no PyTorch or HIP types cross this boundary (a HIP stream is
 * passed as `void*`).  Every entry point returns RDN_OK (0) or a negative RDN_E* code and leaves
 * a message for rdn_last_error() (thread-local).  No exception crosses the ABI.  All device
 * buffers are owned by the caller (e.g. the PyTorch caching allocator); the library keeps no
 * device state of its own, enqueues on the caller's stream and never synchronises it.
 * Every kernel and memset of a call goes to the stream it was given, on the device that owns that
 * stream (which need not be the current device), and the call returns without waiting for them.  The
 * two exceptions read status words back and so wait for the stream: rdn_forward_status and
 * rdn_forward_status_ex.  Rows of every admitted length (L < 2^31) get a tile count computed in 64
 * bits, and no launcher walks a batch in chunks below one spectrum.
 *
 * Reference interfaces these entry points replace (paths relative to the reference repo):
 *   rdn_param_names / rdn_packed_size / rdn_pack
 *       -> Model().load_state_dict(torch.load(path))            <model>/evaulate.py:65-66
 *          (the reference keeps nn.Module parameters; the engine folds eval-mode BatchNorm and
 *           re-lays the weights out as MFMA operand fragments once, at load time)
 *   rdn_forward
 *       -> Model.forward(x), x float32 (N, 1, L)                   <model>/evaulate.py:30-32, :84-85
 *          DenoiseCNN 1DCNN/train.py:71-82 · RRCDNet RRCDNet/train.py:72-98 · DSDN DSDN/train.py:101-126
 *          ADSDN ADSDN/train.py:150-167 · PIDN PIDN/train.py:72-106 · APIDN APIDN/train.py:119-159
 *   rdn_generate
 *       -> generate_signals(num_samples, signal_length, snr_range, extreme_noise_prob, max_repeat)
 *                                                                  数据集产生.py:5-64
 *   rdn_metrics / rdn_metrics_ex / rdn_acc_value
 *       -> compute_mse / compute_smoothness / compute_peak_to_peak + skimage SSIM, averaged
 *                                                                  <model>/evaulate.py:14-39
 *   rdn_forward_metrics
 *       -> the body of evaluate(): model(input) then the four metrics of each spectrum, averaged
 *                                                                  <model>/evaulate.py:25-39
 */
#ifndef RAMAN_MI355X_H
#define RAMAN_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDN_ABI_VERSION 6

typedef enum {
  RDN_DENOISECNN = 0, /* 1DCNN/train.py   class DenoiseCNN */
  RDN_RRCDNET = 1,    /* RRCDNet/train.py class RRCDNet    */
  RDN_DSDN = 2,       /* DSDN/train.py    class DSDN       */
  RDN_ADSDN = 3,      /* ADSDN/train.py   class ADSDN      */
  RDN_PIDN = 4,       /* PIDN/train.py    class PIDN       */
  RDN_APIDN = 5       /* APIDN/train.py   class APIDN      */
} rdn_arch;

/* Arithmetic of the 64->64 convolutions (stems, activations math: fp32; heads: fp32 operands,
 * fp64 accumulation, one final rounding).
 *   RDN_F32    exact-fp32 MFMA, fp32 activations, compensated (chunked TwoSum) accumulation
 *                                                               (1e-5 parity mode)
 *   RDN_BF16   one bf16 MFMA per product, bf16 activations: NO tolerance guarantee (misses the
 *              2e-2 bf16 bar on trained RRCDNet: 0.24); the Python layer names it 'bf16-unsafe' 
 *   RDN_BF16X3 split bf16: operands as bf16 hi+lo pairs, three bf16 MFMAs per product
 *              (hi*hi + hi*lo + lo*hi), ~16-bit operands        (bf16 MFMA at 2e-2-safe accuracy)
 *   RDN_F16F8  f16 main product (v = hi + lo, hi = f16(v)) plus both correction products
 *              W_lo*X_hi + W_hi*X_lo as ONE block-scaled e4m3 MFMA at twice the 16-bit rate; f16 hi
 *              + e4m3 lo activations (~15 significant bits).  2e-2-safe at 2/3 of the MFMA cycles
 *              of RDN_BF16X3.  Range: the e4m3 planes hold |activation| <= 1792 (hi / 4 in e4m3); a
 *              tile whose activations exceed it writes NaN outputs and raises the workspace's range
 *              word (rdn_forward_status: RDN_ERANGE) -- never a silently clamped value.  Inputs of
 *              normalised intensity stay far inside it (trained networks: max |activation| 9-28);
 *              ~100x larger inputs need RDN_F32 or RDN_BF16X3.
 *   RDN_F16    one f16 MFMA per product (v_mfma_f32_16x16x32_f16, the bf16 rate), f16 weights and
 *              activations (11 significant bits), fp32 accumulation: the fastest mode within the 2e-2
 *              bf16 bar on the golden fixtures of 1DCNN, DSDN, ADSDN, PIDN and APIDN (worst 6.9e-3,
 *              trained DSDN) -- NOT on trained RRCDNet (3.6e-2): use RDN_F16MIX there.  Activations
 *              must stay below the f16 range (65504); a larger one becomes inf, never a silent wrong
 *              value.
 *   RDN_F16MIX RRCDNet only: RDN_F16 arithmetic with the RDN_F16F8 correction kept on the last five
 *              layers of the right branch (the ones the head's cancellation x - (r + l)/2 amplifies),
 *              and every layer corrected on a tile whose input window leaves [-0.3, 1.3] (a spike):
 *              within 2e-2 (1.19e-2 on the trained fixture, 1.54e-2 worst over config 1's 1000
 *              spectra).  The corrected layers have RDN_F16F8's range and range guard (RDN_ERANGE);
 *              on the walk geometry a saturated tile NaNs the rest of its spectrum (its clamped values
 *              travel on in the carried rows), on the tile geometries the tile alone.
 *              One hybrid kernel: the plain layers, the whole left branch and its head
 *              on the RDN_F16 ping-pong engine, the corrected tail and the right head on the in-place
 *              tile.  The corrected layers are compiled in; rdn_get_correction_mask reads them back
 *              from a packed blob.
 * RDN_F16 / RDN_F16MIX launches that would occupy at most half the CUs with 640-row tiles (e.g. one
 * spectrum per call, evaulate.py:29-32) run on 256-row tiles (same arithmetic and, for RDN_F16MIX, the
 * same hybrid composition); the environment variable RDN_SHORT_TILES=0/1 forces either.  Launches large
 * enough to give every CU several spectra run RDN_F16 (DenoiseCNN, RRCDNet, DSDN, PIDN) and RDN_F16MIX
 * on the walk geometry instead: one workgroup walks a whole spectrum with time-skewed layers and no
 * halo recompute (same per-output arithmetic; RDN_WALK=0/1 forces either). */
typedef enum { RDN_F32 = 0, RDN_BF16 = 1, RDN_BF16X3 = 2, RDN_F16F8 = 3, RDN_F16 = 4, RDN_F16MIX = 5 } rdn_dtype;

enum {
  RDN_OK = 0,
  RDN_EINVAL = -1,       /* bad argument (null pointer, unknown arch/dtype, n or L < 1)      */
  RDN_EUNSUPPORTED = -2, /* combination not built                                            */
  RDN_ESHAPE = -3,       /* a tensor handed to rdn_pack has the wrong number of elements      */
  RDN_ESIZE = -4,        /* destination / workspace buffer too small                          */
  RDN_EHIP = -5,         /* a HIP runtime call failed (message carries hipGetErrorString)     */
  RDN_ERANGE = -6        /* rdn_forward_status: an RDN_F16F8 / RDN_F16MIX activation left the
                            e4m3 planes' range; the affected tiles' outputs are NaN          */
};

/* ABI version (RDN_ABI_VERSION) of the loaded library. */
int rdn_version(void);

/* Build stamp: sha256 prefix of the sources this library was compiled from (csrc/Makefile). */
const char* rdn_build_id(void);

/* Message of the last failing call on this thread ("" if none). */
const char* rdn_last_error(void);

/* The reference state_dict keys rdn_pack consumes, in order, '\n'-separated, NUL-terminated.
 * Writes at most `cap` bytes to `buf` (may be NULL with cap 0); `*needed` receives the size. */
int rdn_param_names(int arch, char* buf, size_t cap, size_t* needed);

/* Bytes of the packed weight blob for (arch, dtype). */
int rdn_packed_size(int arch, int dtype, size_t* bytes);

/* Fold eval-mode BatchNorm (eps 1e-5) into the preceding Conv1d (in fp64) and lay every layer out
 * as MFMA operand fragments.  `tensors[i]` is a HOST fp32 pointer to the tensor named by line i
 * of rdn_param_names (row-major, torch layout), `numels[i]` its element count.  Writes the blob
 * into host memory `dst` (cap bytes); the caller copies it to the device. */
int rdn_pack(int arch, int dtype, const float* const* tensors, const int64_t* numels, int n_tensors,
             void* dst, size_t cap);

/* Blob layout tag: rdn_pack writes RDN_BLOB_MAGIC | arch << 8 | dtype into a word of the small
 * section, and rdn_check_blob verifies that a host blob was packed for (arch, dtype) and is at
 * least rdn_packed_size bytes.  The blob layouts differ per dtype (e.g. an RDN_F16MIX blob holds one
 * more record than an RDN_F16F8 one): rdn_forward needs a blob packed for the same (arch, dtype).
 * The RDN_F16MIX kernels also check the tag on the device and write NaN outputs on a mismatch. */
#define RDN_BLOB_MAGIC 0x52440000u
int rdn_check_blob(int arch, int dtype, const void* host_blob, size_t bytes);

/* Per-layer correction mask (bit i = big layer i, execution order of rdn_param_names' convs, runs
 * the e4m3 correction).  default: the RDN_F16MIX pattern of `arch` (0 = plain RDN_F16 already meets
 * 2e-2 there, and RDN_F16MIX is not built); get: read back from a packed RDN_F16F8 (all ones) or
 * RDN_F16MIX host blob. */
int rdn_default_correction_mask(int arch, uint64_t* mask);
int rdn_get_correction_mask(int arch, int dtype, const void* host_blob, size_t bytes, uint64_t* mask);

/* Device scratch rdn_forward takes for a batch on the device of `stream`: the CBAM networks' team
 * geometry (depends on the device's CU count and occupancy; required); every 16-bit dtype on the fused
 * networks 256 bytes whose first 4 bytes are the status word (optional; ABI v5), 0 otherwise (RDN_F32).
 * Status word bits, sticky until read: RDN_STATUS_RANGE an RDN_F16F8 / RDN_F16MIX activation left the
 * e4m3 planes' range (the tile's outputs are NaN; rdn_forward_status returns RDN_ERANGE);
 * RDN_STATUS_GATE an input value left [-4, 4], the 16-bit modes' domain (normalised intensity: every
 * simulated spectrum lies in [-1, 2]) -- set by the kernels' stems, which read every input anyway;
 * informational (rdn_forward_status does not fail on it; rdn_forward_status_ex reports it): the Python
 * module reads the word once per call and re-runs such a batch in RDN_F32.  Without the workspace a
 * saturated tile still writes NaN, but neither bit is reported.  The CBAM networks' workspaces hold the
 * same information in words of their own (the team kernels' and segment kernels' stems raise the gate
 * there too, ABI v6); read it with rdn_forward_status_ex. */
#define RDN_STATUS_RANGE 1u
#define RDN_STATUS_GATE 2u
#define RDN_STATUS_TIMEOUT 4u   /* rdn_forward_status_ex only: a CBAM team hand-off timed out */
int rdn_workspace_size(int arch, int dtype, int64_t n, int64_t L, size_t* bytes, void* stream);

/* Prepare a newly allocated workspace for rdn_forward on `stream`: clears its status words -- the
 * CBAM hand-off error word and the range word (both sticky across forwards until rdn_forward_status
 * reads and clears them, so one status call after many forwards that share a workspace covers all
 * of them). */
int rdn_workspace_init(int arch, int dtype, int64_t n, int64_t L, void* workspace, size_t workspace_bytes,
                       void* stream);

/* y[n][L] = Model(x[n][L]) on the device.  x, y: fp32 device pointers (the (N,1,L) tensor is
 * (N,L) contiguous) that must not overlap (RDN_EINVAL: tiles re-read input halos while outputs are
 * written); packed: device copy of the rdn_pack blob; stream: hipStream_t or NULL.  n = 0 launches
 * nothing and returns RDN_OK; x and y may then be NULL (every entry point below that takes a batch
 * accepts NULL data pointers for n = 0 the same way). */
int rdn_forward(int arch, int dtype, const void* packed, const float* x, float* y, int64_t n, int64_t L,
                void* workspace, size_t workspace_bytes, void* stream);

/* Completion status of every rdn_forward enqueued on `stream` with this workspace since the last
 * status call (or rdn_workspace_init): waits for the stream (hipStreamSynchronize), then reads and
 * clears the workspace's sticky status words (the fused networks' word: cleared on `stream`).  RDN_EHIP if a CBAM team wait timed out (co-residency
 * broken by a concurrent kernel; the affected spectra's outputs are NaN) or the stream reported an
 * error; RDN_ERANGE if an RDN_F16F8 / RDN_F16MIX activation left the e4m3 planes' range (NaN tiles;
 * for the CBAM networks the CBAM statistics of the saturated tile also reached the rest of its
 * spectrum, so the status word, not the NaN, is the authoritative signal); RDN_ESIZE if the workspace
 * is smaller than this device's team geometry needs; RDN_OK otherwise.  Replaces nothing in the
 * reference (its forward is synchronous PyTorch): the Python module calls it after each
 * range-checked or CBAM forward (and re-runs a saturated batch in RDN_F32), the batched evaluate
 * drivers once at the end. */
int rdn_forward_status(int arch, int dtype, int64_t n, int64_t L, void* workspace, size_t workspace_bytes,
                       void* stream);
/* rdn_forward_status that also reports WHICH status words were set (ABI v6): *flags (may be NULL)
 * receives RDN_STATUS_RANGE | RDN_STATUS_GATE | RDN_STATUS_TIMEOUT as read before the words were
 * cleared, so a caller learns of the input gate (informational: no error code) without reading the
 * workspace itself.  rdn_forward_status clears the same words and drops the gate bit: a C caller that
 * needs it calls this form.  Every network keeps the gate: the fused networks' status word, and the
 * CBAM networks' team / segment workspaces (their stems raise it, ABI v6). */
int rdn_forward_status_ex(int arch, int dtype, int64_t n, int64_t L, void* workspace, size_t workspace_bytes,
                          void* stream, unsigned* flags);

/* rdn_forward followed by rdn_metrics_ex(y, clean, ...) on the same stream (ABI v6): y = Model(x), then
 * each spectrum's MSE, SSIM, Smoothness and Peak2Peak against clean (fp32 or fp64 [n][L], device) into
 * per_spectrum / sums / acc (each may be NULL; sums and acc ACCUMULATED, as rdn_metrics_ex).  Where the
 * forward runs on the walk geometry (RDN_F16 on DenoiseCNN / RRCDNet / DSDN / PIDN, RDN_F16MIX on
 * RRCDNet, large batches) the forward kernel computes them itself -- each spectrum's workgroup right
 * after its walk, from the y rows it just wrote (read back from L2) -- so the separate metrics pass over
 * y is gone; *fused (may be NULL) is then 1.  Otherwise the metrics kernel follows the forward (*fused
 * = 0).  Both paths give every spectrum the same bits (one shared fp64 routine).  L must be >= 7. */
int rdn_forward_metrics(int arch, int dtype, const void* packed, const float* x, float* y, int64_t n, int64_t L,
                        const void* clean, int clean_is_f64, double* per_spectrum, double* sums, int64_t* acc,
                        void* workspace, size_t workspace_bytes, void* stream, int* fused);
/* Simulator parameters; defaults of 数据集产生.py:5-7 are {10000, 20, 37, 0.05, 40}. */
typedef struct {
  int64_t signal_length;
  float snr_lo;
  float snr_hi;
  float extreme_noise_prob;
  int32_t max_repeat;
} rdn_gen_params;

/* Generate spectra first_index .. first_index+n-1 of the stream `seed` (counter-based Philox,
 * so any index range is reproducible on any device).  clean/noisy: fp32 [n][L] device;
 * snr_db / noise_std: fp32 [n] device (either may be NULL).
 * Parameters (RDN_EINVAL otherwise, checked before any device call, also for n = 0):
 *   1 <= signal_length <= INT32_MAX and max_repeat >= 1 with
 *   signal_length + 256 * max_repeat <= INT32_MAX (the kernel sums 256 segment lengths per pass in
 *   32 bits; at signal_length = 1000 the largest max_repeat is 8388604);
 *   snr_lo and snr_hi finite with snr_lo <= snr_hi; extreme_noise_prob not NaN (values <= 0 never
 *   spike, values >= 1 always do).
 * The spectrum index is first_index + i in 64 bits: a caller keeps first_index + n <= 2^64, past
 * which the index would wrap onto spectrum 0. */
int rdn_generate(uint64_t seed, uint64_t first_index, int64_t n, const rdn_gen_params* params,
                 float* clean, float* noisy, float* snr_db, float* noise_std, void* stream);

/* Per-spectrum MSE, SSIM, Smoothness, Peak2Peak of denoised y against clean (both fp32 [n][L],
 * device), computed in fp64.  per_spectrum: fp64 [n][4] device (may be NULL).  sums: fp64 [5]
 * device, ACCUMULATED (+=) as {ΣMSE, ΣSSIM, ΣSmoothness, ΣPeak2Peak, count} (may be NULL).
 * L must be >= 7 (SSIM window).
 * Non-finite values: every metric is the IEEE / numpy value of its definition.  Peak2Peak (np.max(y) -
 * np.min(y)) and SSIM's data range (max - min of clean) are NaN if any contributing value is NaN, and
 * +-inf or NaN as max - min gives otherwise; MSE, Smoothness and SSIM are the IEEE sums (NaN for a NaN
 * or an inf - inf among the terms, else +inf for an infinite term; a 0/0 SSIM window -- all-zero rows --
 * gives NaN).  A non-finite metric is written as it is to per_spectrum and sums and counted in the
 * out-of-range word of that metric in acc: never clamped, never skipped.  The metric epilogue of
 * rdn_forward_metrics follows the same contract (a saturated spectrum's NaN outputs give four NaN metrics).
 * fp32 subnormals in y and clean are read as their values, not flushed to zero. */
int rdn_metrics(const float* y, const float* clean, int64_t n, int64_t L, double* per_spectrum,
                double* sums, void* stream);

/* Exact metric accumulator: RDN_ACC_WORDS int64 on the device.  Metric k (MSE, SSIM, Smoothness,
 * Peak2Peak) owns words [k * RDN_ACC_STRIDE, ...): RDN_ACC_LIMBS limbs, limb j holding the sum of the
 * spectra's 32-bit chunks of weight 2^(32 j - RDN_ACC_FRAC_BITS) (values truncated toward zero below
 * 2^-128), then a count of values that were non-finite or >= 2^64 in magnitude; word RDN_ACC_COUNT
 * counts spectra.  Integer addition is associative, so the accumulated bits do not depend on the
 * batch split, the atomics' order or the number of ranks whose accumulators are summed (all-reduce
 * SUM over int64), for up to 2^31 spectra per accumulator. */
#define RDN_ACC_LIMBS 6
#define RDN_ACC_FRAC_BITS 128
#define RDN_ACC_STRIDE (RDN_ACC_LIMBS + 1)
#define RDN_ACC_COUNT (4 * RDN_ACC_STRIDE)
#define RDN_ACC_WORDS (RDN_ACC_COUNT + 1)

/* rdn_metrics with the clean reference in fp32 (clean_is_f64 = 0) or fp64 (1, e.g. a test.npz as
 * the reference loads it), and an optional exact accumulator `acc` (device, RDN_ACC_WORDS int64,
 * ACCUMULATED).  per_spectrum, sums and acc may each be NULL. */
int rdn_metrics_ex(const float* y, const void* clean, int clean_is_f64, int64_t n, int64_t L, double* per_spectrum,
                   double* sums, int64_t* acc, void* stream);

/* Host: {ΣMSE, ΣSSIM, ΣSmoothness, ΣPeak2Peak, count} from a HOST copy of an exact accumulator, each
 * sum the exact accumulated value rounded once to the nearest double (NaN for a metric with an
 * out-of-range value). */
int rdn_acc_value(const int64_t* acc, double* sums);

/* ---- SNR report (entry points added to ABI v6 without a version bump: detect them by symbol) -------
 *
 * Per spectrum, in fp64, from the noisy input x (fp32), the denoised y (fp32) and clean (fp32 / fp64):
 *   P  = mean(clean^2)              the simulator's own signal power, 数据集产生.py:43
 *   Ni = mean((x - clean)^2)        No = mean((y - clean)^2)
 *   SNR_in = 10 log10(P / Ni)       SNR_out = 10 log10(P / No)       SNR_gain = SNR_out - SNR_in   [dB]
 * A zero denominator or a zero P gives the IEEE result (+-inf or NaN), written as it is to the
 * per-spectrum output and counted in the out-of-range word of that quantity in a report: never clamped.
 *
 * Report: RDN_REPORT_WORDS(nbins) int64 on the device, RDN_REPORT_ROWS(nbins) = nbins + 2 rows of
 * RDN_REPORT_ROW_WORDS words.  Row 0 is the underflow bin (key < lo), rows 1 .. nbins the uniform bins
 * of [lo, hi), row nbins + 1 the overflow bin (key >= hi, or a NaN key).  A row holds
 * RDN_REPORT_QUANTITIES exact accumulators of RDN_ACC_STRIDE words each, in the order {MSE, SSIM,
 * Smoothness, Peak2Peak, SNR_in, SNR_out, SNR_gain} and in the format of rdn_metrics_ex's accumulator
 * (RDN_ACC_LIMBS limbs, then the count of values that were non-finite or >= 2^64 in magnitude), then word
 * RDN_REPORT_COUNT, the number of spectra in the bin, and word RDN_REPORT_COUNT4, the number of those
 * whose four metrics were supplied (per4): without per4 the first four accumulators and this count stay 0.
 * Integer sums: a report's bits do not depend on the batch split, the atomics' order or the number of
 * ranks whose reports are summed (all-reduce SUM over int64), for up to 2^31 spectra per report.
 * Whole-set totals need no accumulator of their own: they are the word-wise sum of a report's rows
 * (rdn_report_value's last row), so a caller who wants only totals passes nbins = 1 and any finite lo < hi.
 *
 * Bin of a key, evaluated in IEEE fp32 (every operation rounded to fp32, no fused multiply-add):
 *   scale = (float)nbins / (hi - lo)
 *   key is NaN  -> row nbins + 1;   key < lo -> row 0;   key >= hi -> row nbins + 1;   otherwise
 *   i = (int)((key - lo) * scale)   truncated toward zero;   row = 1 + min(i, nbins - 1)
 * (numpy: np.float32 scalars / arrays throughout, .astype(np.int32) for the truncation).
 * rdn_report_bin evaluates it on the host. */
#define RDN_REPORT_QUANTITIES 7
#define RDN_REPORT_MAX_BINS 64
#define RDN_REPORT_COUNT (RDN_REPORT_QUANTITIES * RDN_ACC_STRIDE)
#define RDN_REPORT_COUNT4 (RDN_REPORT_COUNT + 1)
#define RDN_REPORT_ROW_WORDS (RDN_REPORT_COUNT4 + 1)
#define RDN_REPORT_ROWS(nbins) ((nbins) + 2)
#define RDN_REPORT_WORDS(nbins) (RDN_REPORT_ROWS(nbins) * RDN_REPORT_ROW_WORDS)
/* doubles per row of rdn_report_value: {count, sum MSE, SSIM, Smoothness, Peak2Peak, SNR_in, SNR_out,
 * SNR_gain, count4} */
#define RDN_REPORT_VALUES (RDN_REPORT_QUANTITIES + 2)

/* One pass over x, y and clean ([n][L] device; clean fp32 or fp64 as rdn_metrics_ex takes it), L >= 1
 * (L < 2^31: rows are addressed with 64-bit offsets, no 2^29 limit).  per_spectrum3: fp64 [n][3] device
 * {SNR_in, SNR_out, SNR_gain} (may be NULL).  report: device, RDN_REPORT_WORDS(nbins) int64,
 * ACCUMULATED (may be NULL; key, lo, hi, nbins and per4 are then not used and key / per4 must be NULL).
 * With a report: 1 <= nbins <= RDN_REPORT_MAX_BINS, lo < hi both finite; key: fp32 [n] device, the value
 * each spectrum is binned by (the nominal SNR of rdn_generate's snr_db or of a dataset), or NULL: the
 * measured SNR_in rounded to fp32; per4: fp64 [n][4] device, the per-spectrum output of rdn_metrics_ex /
 * rdn_forward_metrics for the same spectra, or NULL.  At least one of per_spectrum3 / report is needed. */
int rdn_snr(const float* x, const float* y, const void* clean, int clean_is_f64, int64_t n, int64_t L,
            double* per_spectrum3, const float* key, float lo, float hi, int nbins, const double* per4,
            int64_t* report, void* stream);

/* Host: the report row (0 .. nbins + 1) of `key` by the formula above. */
int rdn_report_bin(float key, float lo, float hi, int nbins, int* row);

/* Host: doubles of a HOST copy of a report.  out: (RDN_REPORT_ROWS(nbins) + 1) rows of RDN_REPORT_VALUES
 * doubles: the report's rows in order, then the totals over all rows (their limbs added as integers).
 * Each sum is the exact accumulated value rounded once to the nearest double, NaN for a quantity with an
 * out-of-range value in that row (the contract of rdn_acc_value). */
int rdn_report_value(const int64_t* report, int nbins, double* out);

/* ---- PhysicsAwareLoss report (added to ABI v6 without a version bump: detect the entry points by symbol)
 *
 * The forward value of the loss PIDN and APIDN are trained against (PIDN/train.py:109-146), per spectrum.
 * With p the denoised output (fp32), c clean (fp32 / fp64) and x the noisy input (fp32), i = 0 .. L-1, all
 * arithmetic in fp64 on the stored values except the mask:
 *   MSE    = sum_i (p_i - c_i)^2 / L
 *   Smooth = sum_{i < L-1} |(p_{i+1} - p_i) - (c_{i+1} - c_i)| / (L - 1)
 *   m_i    = 1 if (c_{i+1} - c_i) < (c_i - c_{i-1}) else 0,  i = 1 .. L-2; both differences are formed and
 *            compared in clean's own storage type (fp32 arithmetic for fp32 clean, fp64 for fp64 clean):
 *            torch.diff(clean, n=2) < 0.  NaN compares false.
 *   PeakCount = sum_i m_i
 *   Peak   = sum_{i=1}^{L-2} (m_i p_i - m_i c_i)^2 / (L - 2)     the mean over ALL L - 2 positions; m_i is a
 *            factor, not a select: a non-finite p at an unmasked position gives NaN, as the reference does
 *   d_i = x_i - c_i;  mu = sum_i d_i / L;  v = sum_i (d_i - mu)^2 / (L - 1)   (unbiased, centred two-pass)
 *   Noise  = sum_i (d_i^2 - v)^2 / L
 *   Total  = ((MSE + alpha Smooth) + beta Peak) + gamma Noise      reference defaults 0.1, 0.05, 0.01
 * All spectra of a call share one L, so the reference's loss over a batch is the mean of Total over its
 * spectra (and each of its terms the mean of the per-spectrum term).  Non-finite values are written as
 * they are to the per-spectrum output and counted in the quantity's out-of-range word in a report: never
 * clamped.
 *
 * Report: RDN_PHYS_WORDS(nbins) int64 on the device, RDN_REPORT_ROWS(nbins) rows of RDN_PHYS_ROW_WORDS
 * words with the row structure and bin formula of the SNR report above (row 0 underflow, rows 1 .. nbins
 * the uniform bins of [lo, hi), row nbins + 1 overflow / NaN key).  A row holds RDN_PHYS_QUANTITIES exact
 * accumulators of RDN_ACC_STRIDE words in the order {MSE, Smooth, Peak, Noise, Total, PeakCount}, in
 * rdn_metrics_ex's limb format, then word RDN_PHYS_COUNT, the number of spectra in the row.  Integer
 * sums: the same bits for any batch split, atomics order or number of ranks. */
#define RDN_PHYS_QUANTITIES 6
#define RDN_PHYS_COUNT (RDN_PHYS_QUANTITIES * RDN_ACC_STRIDE)
#define RDN_PHYS_ROW_WORDS (RDN_PHYS_COUNT + 1)
#define RDN_PHYS_WORDS(nbins) (RDN_REPORT_ROWS(nbins) * RDN_PHYS_ROW_WORDS)
/* doubles per row of rdn_physics_value: {count, sum MSE, Smooth, Peak, Noise, Total, PeakCount} */
#define RDN_PHYS_VALUES (RDN_PHYS_QUANTITIES + 1)

/* x, y, clean: [n][L] device (clean fp32 or fp64 as rdn_metrics_ex takes it), 3 <= L < 2^31 (rows are
 * addressed with 64-bit offsets).  alpha, beta, gamma: the weights of Total, finite.  per_spectrum6: fp64
 * [n][6] device, the six quantities in the order above (may be NULL).  report: device,
 * RDN_PHYS_WORDS(nbins) int64, ACCUMULATED (may be NULL; key, lo, hi and nbins are then not used and key
 * must be NULL).  With a report: 1 <= nbins <= RDN_REPORT_MAX_BINS, lo < hi both finite; key: fp32 [n]
 * device, the value each spectrum is binned by, or NULL: every spectrum goes into row 1 (an unbinned
 * report: nbins = 1 and any finite lo < hi).  At least one of per_spectrum6 / report is needed.  n = 0
 * launches nothing and accepts NULL data pointers. */
int rdn_physics(const float* x, const float* y, const void* clean, int clean_is_f64, int64_t n, int64_t L,
                double alpha, double beta, double gamma, double* per_spectrum6, const float* key, float lo,
                float hi, int nbins, int64_t* report, void* stream);

/* ---- PhysicsAwareLoss gradient (added to ABI v6 without a version bump: detect the entry point by symbol)
 *
 * Value and gradient of the loss from one launch: what a training step needs (criterion(output, clean,
 * noisy), then loss.backward()).  Per spectrum, on the stored values and in fp64 except the mask, with p,
 * c and m_i as above (m_i exactly rdn_physics's, formed in clean's own storage type), i = 0 .. L-1:
 *   r_i = p_i - c_i
 *   e_i = (p_{i+1} - p_i) - (c_{i+1} - c_i)          i = 0 .. L-2
 *   s_i = (e_i > 0) - (e_i < 0)                      0 for e_i = 0 and for NaN: torch's abs backward
 *   g_i = scale * [ 2 r_i / L
 *                 + alpha * (s_{i-1} [i >= 1] - s_i [i <= L-2]) / (L - 1)
 *                 + beta * 2 m_i (m_i p_i - m_i c_i) / (L - 2)   [1 <= i <= L-2] ]
 * rounded once to fp32.  Terms that do not exist at the row's ends are selected away, not multiplied by
 * zero; m_i is a factor, as in the value: a non-finite p at an unmasked centre position gives NaN there,
 * as the reference does.  A NaN at p_i gives NaN at i only (its neighbours' smoothness terms see
 * sign(NaN) = 0); +-inf at a row's end gives +-inf there only.  gamma takes no part: the Noise term is a
 * function of x - c alone.  With scale = 1 / n, g is d(mean over the batch of Total) / d p: the reference's
 * loss.backward() for (N, 1, L) inputs.
 *
 * grad: fp32 [n][L] device, required, WRITTEN (not accumulated); it must not overlap x, y or clean (each
 * position reads its neighbours): RDN_EINVAL.  per_spectrum6: fp64 [n][6] device or NULL, the six
 * quantities of rdn_physics with the same bits for every spectrum (one shared device routine).  x may be
 * NULL when per_spectrum6 is NULL: a gradient-only call reads no x and runs no reduction and no noise
 * pass.  3 <= L < 2^31 (64-bit row offsets); alpha, beta, gamma and scale finite; scale is applied per
 * call, whatever the number of launches a huge n is split into, so the gradient of rows [0, k) and [k, n)
 * from two calls with one scale is the rows of one call.  n = 0 launches nothing and accepts NULL data
 * pointers; it still checks L, the weights and scale. */
int rdn_physics_grad(const float* x, const float* y, const void* clean, int clean_is_f64, int64_t n, int64_t L,
                     double alpha, double beta, double gamma, double scale, double* per_spectrum6, float* grad,
                     void* stream);

/* Host: doubles of a HOST copy of a report of rdn_physics.  out: (RDN_REPORT_ROWS(nbins) + 1) rows of
 * RDN_PHYS_VALUES doubles: the report's rows in order, then the totals over all rows (their limbs added as
 * integers).  Each sum is the exact accumulated value rounded once to the nearest double, NaN for a
 * quantity with an out-of-range value in that row (the contract of rdn_acc_value). */
int rdn_physics_value(const int64_t* report, int nbins, double* out);

/* ---- classical baseline filters (added to ABI v6 without a version bump: detect by symbol) ----
 *
 * The filters a denoising result is compared with -- moving average, Gaussian, Savitzky-Golay (rdn_fir) and
 * the running median (rdn_median) -- on device-resident spectra, so that their columns of a comparison come
 * from the same meters as a network's.  x, y: fp32 [n][L] device, y WRITTEN; w: the odd window,
 * 1 <= w <= RDN_FILTER_MAX_WINDOW, h = (w - 1) / 2.  A spectrum's output bits depend on its own samples
 * only: not on n, its row index or the launches a huge n is split into.
 *
 * Mirror indexing (scipy's mode='mirror', no repeated edge sample): idx(j) = -j for j < 0,
 * 2 (L - 1) - j for j > L - 1, j otherwise.
 *
 * rdn_fir, taps: fp64 [w] DEVICE.  In fp64, products and sums each rounded on their own, in this order,
 * never fused:
 *   acc = 0.0;  for k = 0 .. w-1:  acc = acc + taps[k] * (double)x[idx(i - h + k)];   y[i] = (float)acc
 * (one final rounding to fp32; fp32 subnormals are read as their values).  edge_taps: NULL, or fp64
 * [w - 1][w] DEVICE: the first and last h outputs then run the same recurrence over a fixed window,
 *   y[j]         = sum_k edge_taps[j][k]     * x[k]           j < h
 *   y[L - h + j] = sum_k edge_taps[h + j][k] * x[L - w + k]   j < h
 * which is how scipy's savgol_filter(mode='interp') is expressed.  Non-finite inputs or taps give the
 * IEEE result of the recurrence.
 *
 * rdn_median: samples are ordered by the monotone unsigned key of their fp32 bits (bits ^ 0x80000000 for a
 * clear sign bit, ~bits for a set one: -0 < +0, and -inf and +inf are ordinary values).  y[i] is the sample
 * of rank h among x[idx(i - h)] .. x[idx(i + h)], bit for bit one of the inputs; a window that holds a NaN
 * gives the quiet NaN 0x7fc00000.
 *
 * RDN_EINVAL, checked before any device call and also for n = 0: a NULL taps; n < 0; w even, w < 1 or
 * w > RDN_FILTER_MAX_WINDOW; L < w or L >= 2^31; for n > 0 a NULL x or y, or x and y overlapping.  n = 0
 * launches nothing and accepts NULL data pointers.  taps and edge_taps stay the caller's: the library keeps
 * no device state and never synchronises; the call is asynchronous on `stream`. */
#define RDN_FILTER_MAX_WINDOW 255
#define RDN_FILTER_TILE 2048         /* outputs per workgroup (tests probe the sizes around it) */
int rdn_fir(const float* x, float* y, int64_t n, int64_t L, const double* taps, int w,
            const double* edge_taps /* device [w-1][w] or NULL = mirror */, void* stream);
int rdn_median(const float* x, float* y, int64_t n, int64_t L, int w, void* stream);

/* ---- translation-invariant Haar shrinkage (added to ABI v6 without a version bump: detect by symbol) ----
 *
 * The classical denoiser of a piecewise-constant signal under white noise: the undecimated (a trous) Haar
 * transform of each spectrum, its detail planes thresholded in units of the spectrum's own noise estimate,
 * and the inverse transform (Coifman & Donoho's cycle spinning).  x, y: fp32 [n][L] device, y WRITTEN;
 * J = levels, 1 <= J <= RDN_HAAR_MAX_LEVELS, 2^J <= L < 2^31; k: fp64 [J] HOST, each finite and >= 0.
 * Indexing is periodic: idx(j) = j mod L, taken non-negative.  All arithmetic is fp64, each operation rounded
 * on its own, none fused:
 *   a_0[i] = (double)x[i]
 *   for j = 1..J, s = 2^(j-1):   p = a_{j-1}[i],  q = a_{j-1}[idx(i - s)]
 *       a_j[i] = 0.5 * (p + q)        d_j[i] = 0.5 * (p - q)
 *   m = median over i in [0, L) of |d_1[i]|   (numpy's: rank (L-1)/2 for odd L; 0.5 * (lo + hi) of ranks
 *                                              L/2-1, L/2 for even L)
 *   t_j = k[j-1] * m                                  (one product)
 *   RDN_HAAR_SOFT:  e_j = d_j - t_j if d_j > t_j;  d_j + t_j if d_j < -t_j;  else +0.0
 *   RDN_HAAR_HARD:  e_j = d_j if |d_j| > t_j;  else +0.0
 *   b_J = a_J;  for j = J..1, s = 2^(j-1):
 *       b_{j-1}[i] = 0.5 * ((b_j[i] + e_j[i]) + (b_j[idx(i + s)] - e_j[idx(i + s)]))
 *   y[i] = (float)b_0[i]                              (one rounding to fp32)
 * med: fp64 [n] device, WRITTEN: m of each spectrum.  A spectrum that holds a NaN or an infinity gives the
 * quiet NaN 0x7fc00000 at every output and NaN in med.  fp32 subnormals are read as their values.  A
 * spectrum's output bits depend on its own samples only: not on n, its row index, the tiling or the launches
 * a huge n is split into.
 *
 * With every k = 0 this is a perfect-reconstruction transform.  With
 * k[j-1] = lambda * 2^((1-j)/2) / 0.6744897501960817 it is cycle spinning over all 2^J shifts of the
 * orthonormal decimated Haar transform with threshold lambda * sigma, where
 * sigma = m * sqrt(2) / 0.6744897501960817 is the MAD estimate of the noise.
 *
 * RDN_EINVAL, checked before any device call and also for n = 0: a NULL k; a k entry that is negative or not
 * finite; levels outside [1, RDN_HAAR_MAX_LEVELS]; an unknown mode; L < 2^levels or L >= 2^31; n < 0; for
 * n > 0 a NULL x, y or med, x and y overlapping, or med overlapping x or y.  n = 0 launches nothing.  The library keeps no device
 * state and never synchronises; med is the caller's buffer; the call is asynchronous on `stream`. */
#define RDN_HAAR_MAX_LEVELS 7
#define RDN_HAAR_TILE 512            /* outputs per workgroup (tests probe the sizes around it) */
#define RDN_HAAR_SELECT_LDS_L 12288  /* longer spectra are re-read through L2 by the median's select passes */
enum { RDN_HAAR_SOFT = 0, RDN_HAAR_HARD = 1 };
int rdn_haar_shrink(const float* x, float* y, double* med, int64_t n, int64_t L, int levels,
                    const double* k /* HOST [levels] */, int mode, void* stream);

/* m of rdn_haar_shrink's contract alone (median over i of |0.5 * (x[i] - x[idx(i - 1)])|, periodic, numpy's
 * median): the same select kernel, the same bits; NaN for a spectrum with a NaN or an infinity.  x: fp32 [n][L]
 * device; med: fp64 [n] device, WRITTEN; 1 <= L < 2^31 (m = 0 for L = 1).  RDN_EINVAL, checked before any
 * device call and also for n = 0: n < 0; L < 1 or L >= 2^31; for n > 0 a NULL x or med, or med overlapping x.
 * n = 0 launches nothing.  No device state, no synchronisation; asynchronous on `stream`.
 * (Added to ABI v6 without a version bump: detect by symbol.) */
int rdn_noise_mad(const float* x, double* med, int64_t n, int64_t L, void* stream);

/* ---- exact piecewise-constant (Potts) fit (added to ABI v6 without a version bump: detect by symbol) ----
 *
 * The jump-penalised least-squares fit of each spectrum: the segmentation into runs of at most K = max_len
 * samples and the per-run means that minimise  sum (x - fit)^2 + g * #runs  exactly, by dynamic programming
 * (the Potts functional; for a piecewise-constant signal under white noise of variance sigma^2, g is a small
 * multiple of sigma^2).  x, y: fp32 [n][L] device, y WRITTEN; gamma: fp64 [n] DEVICE, g of each spectrum;
 * nseg: int32 [n] device or NULL, WRITTEN: the number of runs; 1 <= K <= RDN_POTTS_MAX_LEN, 1 <= L < 2^31.
 * All arithmetic is fp64, each operation rounded on its own, none fused:
 *   S1[0] = S2[0] = 0.0;  for i = 1..L:  v = (double)x[i-1];  S1[i] = S1[i-1] + v;  S2[i] = S2[i-1] + v * v
 *   B[0] = 0.0
 *   for r = 1..L:  for len = 1..min(K, r), l = r - len:
 *        d1 = S1[r] - S1[l];   d2 = S2[r] - S2[l];   sse = d2 - (d1 * d1) / (double)len     (not clamped at 0)
 *        c(len) = (B[l] + g) + sse
 *      B[r] = min over len of c(len);   A[r] = the SMALLEST len that attains it
 *   r = L;  while r > 0:  len = A[r];  mean = (S1[r] - S1[r-len]) / (double)len
 *        y[r-len .. r-1] = (float)mean  (one rounding);  nseg += 1;  r -= len
 * A spectrum that holds a NaN or an infinity, or whose g is negative, NaN or infinite, gets the quiet NaN
 * 0x7fc00000 at every output and nseg = 0.  A finite spectrum never produces a non-finite intermediate
 * (fp32^2 * 2^31 fits fp64).  fp32 subnormals are read as their values.  A spectrum's output bits depend on
 * its own samples and its own g only: not on n, its row index or the launches a huge n is split into.
 *
 * work: caller-owned device scratch of work_bytes >= n * L bytes, contents unspecified afterwards (the
 * back-pointers A, one byte per position).
 *
 * RDN_EINVAL, checked before any device call and also for n = 0: a NULL gamma; n < 0; max_len outside
 * [1, RDN_POTTS_MAX_LEN]; L < 1 or L >= 2^31; for n > 0 a NULL x, y or work, work_bytes < n * L, x and y
 * overlapping, work overlapping x or y, nseg overlapping x, y or work.  n = 0 launches nothing and accepts
 * NULL data pointers.  The library keeps no device state and never synchronises; the call is asynchronous on
 * `stream`. */
#define RDN_POTTS_MAX_LEN 64
int rdn_potts(const float* x, float* y, int32_t* nseg /* may be NULL */, const double* gamma /* DEVICE [n] */,
              int64_t n, int64_t L, int max_len, uint8_t* work, size_t work_bytes, void* stream);

/* ---- Bayesian change-point smoother (added to ABI v6 without a version bump: detect by symbol) ----
 *
 * The posterior mean of each spectrum under the simulator's own signal model -- runs of 1 .. K = max_len equal
 * samples (the run length uniform), the levels uniform on a range of width W = level_range, white Gaussian
 * noise of standard deviation sigma -- by an exact forward-backward recursion over the run boundaries; with
 * it the posterior probability that a run starts at each sample, and the log evidence of the spectrum.
 * x, y: fp32 [n][L] device, y WRITTEN; jump: fp32 [n][L] device or NULL, WRITTEN; logz: fp64 [n] device or
 * NULL, WRITTEN; sigma: fp64 [n] DEVICE, one per spectrum; 1 <= K <= RDN_BAYES_MAX_LEN, 1 <= L < 2^31.
 * Per spectrum, with boundaries 0 .. L (a run [s, t) holds the samples s .. t - 1, n = t - s of them):
 *   c0 = log((sqrt(2 pi) * sigma) / (W * (double)K));   h = 1.0 / ((2.0 * sigma) * sigma)
 *   log w(s, t) = (c0 - 0.5 * log((double)n)) - M2(s, t) * h       M2 = sum (x - m)^2 about the run mean m
 *   G[L] = 0;   G[s] = LSE over n = 1..min(K, L - s) of (G[s + n] + log w(s, s + n)),   s = L - 1 .. 0
 *   F[0] = 0;   F[t] = LSE over n = 1..min(K, t) of (F[t - n] + log w(t - n, t)),       t = 1 .. L
 *   logZ = G[0]
 *   P(s, t) = exp(F[s] + log w(s, t) + G[t] - logZ)              the posterior probability of the run [s, t)
 *   y[i] = (float)(sum over s <= i < t of P(s, t) * m(s, t))      (one rounding)
 *   jump[i] = (float)exp(F[i] + G[i] - logZ), i = 1 .. L - 1;     jump[0] = 1.0f exactly
 * This is the evidence of n samples that share one level under a flat prior of width W, times the run-length
 * prior 1 / K; the factor common to every segmentation is dropped and every run, the last included, has the
 * same weight.  All arithmetic is fp64, no operation fused.  m and M2 of a candidate run are Welford sums
 * started at the run's first sample in the sweep's direction (the right end for G, the left end for F and y):
 *   d = v - m;  m = m + d * (1.0 / (double)n);  M2 = M2 + d * (v - m)        n the count that includes v
 * never differences of whole-row prefix sums.  Every LSE is  M + log(sum exp(a - M))  with M the maximum of
 * its terms.  P(s, t) is formed from the LSE's own terms: exp(a - M) * exp(M + G[t] - logZ), and jump[t] as
 * (sum exp(a - M)) * exp(M + G[t] - logZ).  The order of each sum is fixed by the code (the 64 candidates of
 * a step sit in the lanes their boundaries have modulo 64), so a spectrum's output bits depend on its own
 * samples, its own sigma, K and W only: not on n, its row index or the launches a huge n is split into.
 * A spectrum that holds a NaN or an infinity, or whose sigma is NaN, infinite or <= 0 (or so small that h is
 * infinite), gets the quiet NaN 0x7fc00000 at every y and jump and logz = NaN.  fp32 subnormals are read as
 * their values.
 *
 * work: caller-owned device scratch of work_bytes >= n * (L + 1) * 8 bytes, 8-byte aligned, contents
 * unspecified afterwards (G of every boundary).
 *
 * RDN_EINVAL, checked before any device call and also for n = 0: a NULL sigma; n < 0; max_len outside
 * [1, RDN_BAYES_MAX_LEN]; level_range not finite or <= 0; L < 1 or L >= 2^31; for n > 0 a NULL x, y or work,
 * a work that is not 8-byte aligned, work_bytes < n * (L + 1) * 8, x and y overlapping, work overlapping x or
 * y, jump or logz overlapping x, y, work or each other, sigma overlapping anything written.  n = 0 launches nothing and accepts NULL data
 * pointers.  The library keeps no device state and never synchronises; the call is asynchronous on `stream`. */
#define RDN_BAYES_MAX_LEN 64
int rdn_bayes_steps(const float* x, float* y, float* jump /* may be NULL */, double* logz /* may be NULL */,
                    const double* sigma /* DEVICE [n] */, int64_t n, int64_t L, int max_len, double level_range,
                    double* work, size_t work_bytes, void* stream);

/* ---- blind residual report (added to ABI v6 without a version bump: detect the entry points by symbol) ----
 *
 * What can be said about a denoised spectrum without its clean twin (a measured trace has none): if y is the
 * signal, r = x - y is the noise -- its RMS is the noise level, its mean is zero and it is white.  A denoiser
 * that removes signal leaves autocorrelation in r and a Ljung-Box Q far above its K degrees of freedom; one
 * that under-smooths leaves an RMS below the noise estimate.  x: the noisy input, y: the denoised output,
 * fp32 [n][L] device; sigma: fp64 [n] DEVICE, each spectrum's noise level (e.g. rdn_noise_mad's m times
 * sqrt(2) / 0.6744897501960817); K = lags, 1 <= K <= RDN_BLIND_MAX_LAGS, K < L < 2^31.  Per spectrum, all
 * arithmetic is fp64 on the stored fp32 values, each operation rounded on its own, none fused:
 *   a_i = (double)x_i;  b_i = (double)y_i;  r_i = a_i - b_i
 *   Mean = (sum_i r_i) / L          RMS = sqrt((sum_i r_i^2) / L)          Ratio = RMS / sigma
 *   d_i = r_i - Mean                D = sum_i d_i^2                         (two passes: centred after the mean)
 *   rho_k = (sum_{i < L-k} d_i * d_{i+k}) / D,   k = 1..K                   Rho1 = rho_1
 *   RhoMax = NaN if any rho_k is NaN, else max_k |rho_k|
 *   Q = ((double)L * (double)(L+2)) * sum_{k=1..K, ascending} (rho_k * rho_k) / (double)(L - k)    (Ljung-Box)
 *   S = (sum_i a_i^2) / L;  s2 = sigma * sigma;  SNR_est = 10 * log10((S - s2) / s2)                [dB]
 *   flagged = Q > q_crit            (false for a NaN Q)
 * The sums over i are taken in an order the code fixes (no floating-point atomics).  A spectrum's seven values
 * and its rho row depend on its own samples, its own sigma and K only: not on n, its row index or the launches
 * a huge n is split into.  Zero denominators, NaN or infinite samples and a NaN, zero or negative sigma give
 * the IEEE result, written as it is and counted in the out-of-range word of that quantity in a report: nothing
 * is clamped or skipped (the contract of rdn_snr).
 *
 * per_spectrum7: fp64 [n][7] device {Mean, RMS, Ratio, Rho1, RhoMax, Q, SNR_est}, or NULL.  rho: fp64
 * [n][lags] device {rho_1 .. rho_K}, or NULL.  report: device, RDN_BLIND_WORDS(nbins) int64, ACCUMULATED (integer
 * atomics only), or NULL: RDN_REPORT_ROWS(nbins) = nbins + 2 rows of RDN_BLIND_ROW_WORDS words with the row
 * structure of the SNR report (row 0 underflow, rows 1 .. nbins the uniform bins of [lo, hi), row nbins + 1
 * overflow / NaN key).  A row holds RDN_BLIND_QUANTITIES exact accumulators of RDN_ACC_STRIDE words in the
 * order above, in rdn_metrics_ex's limb format, then word RDN_BLIND_COUNT, the number of spectra in the row,
 * then word RDN_BLIND_FLAGGED, the number of those that were flagged.  The bin of a spectrum is that of
 * key[n], or of (float)SNR_est when key is NULL, by the SAME bin formula as rdn_snr (above; rdn_report_bin
 * evaluates it on the host).  Integer sums: the same bits for any batch split, atomics order or number of ranks.
 *
 * RDN_EINVAL, checked before any device call and also for n = 0: a NULL sigma; lags outside
 * [1, RDN_BLIND_MAX_LAGS]; L <= lags or L >= 2^31; n < 0; a NaN or negative q_crit (+inf is allowed and flags
 * nothing); none of per_spectrum7, rho and report given; with a report, nbins outside
 * [1, RDN_REPORT_MAX_BINS] or lo / hi not finite with lo < hi; without a report, a non-NULL key; for n > 0 a
 * NULL x or y, or any output overlapping an input or another output.  n = 0 launches nothing.  The library
 * keeps no device state and never synchronises; the call is asynchronous on `stream`. */
#define RDN_BLIND_MAX_LAGS 32
#define RDN_BLIND_QUANTITIES 7
#define RDN_BLIND_COUNT (RDN_BLIND_QUANTITIES * RDN_ACC_STRIDE)
#define RDN_BLIND_FLAGGED (RDN_BLIND_COUNT + 1)
#define RDN_BLIND_ROW_WORDS (RDN_BLIND_FLAGGED + 1)
#define RDN_BLIND_WORDS(nbins) (RDN_REPORT_ROWS(nbins) * RDN_BLIND_ROW_WORDS)
/* doubles per row of rdn_blind_value: {count, sum Mean, RMS, Ratio, Rho1, RhoMax, Q, SNR_est, flagged} */
#define RDN_BLIND_VALUES (RDN_BLIND_QUANTITIES + 2)
#define RDN_BLIND_LDS_L 20000        /* the longest spectrum whose residual is staged in LDS; longer ones are
                                        recomputed from x and y through L2 (tests probe the sizes around it) */
int rdn_blind(const float* x, const float* y, const double* sigma /* DEVICE [n] */, int64_t n, int64_t L,
              int lags, double q_crit, double* per_spectrum7 /* [n][7] or NULL */, double* rho /* [n][lags] or NULL */,
              const float* key /* [n] or NULL */, float lo, float hi, int nbins, int64_t* report /* or NULL */,
              void* stream);

/* Host: doubles of a HOST copy of a report of rdn_blind.  out: (RDN_REPORT_ROWS(nbins) + 1) rows of
 * RDN_BLIND_VALUES doubles: the report's rows in order, then the totals over all rows (their limbs added as
 * integers).  Each sum is the exact accumulated value rounded once to the nearest double, NaN for a
 * quantity with an out-of-range value in that row (the contract of rdn_acc_value). */
int rdn_blind_value(const int64_t* report, int nbins, double* out);

#ifdef __cplusplus
}
#endif

#endif /* RAMAN_MI355X_H */
