/*
 * sepvad.h — C ABI of libsepvad.so, the MI355X (gfx950) Sep-TFAnet^VAD forward path.
 *
 * The reference has no native interface: its hot path is the PyTorch module
 * `SeparationModel` (reference model/model.py:360-461) called as
 *     model = SeparationModel(**config["arch"]["args"])      (parse_config.py:99-103)
 *     model.load_state_dict(ckpt["state_dict"], strict=True)  (only_inference.py:57-61)
 *     sep, vad, est = model(x, inference_kw)                  (only_inference.py:90-91,
 *                                                               model/online_class_unknown_targets.py:84)
 * Each entry point below replaces one of those steps; the Python host
 * (sep-tfanet-vad_amd/model.py, native.py) binds them with ctypes. Plain pointers and sizes
 * only; no torch types cross this boundary. All device pointers are HIP device memory on
 * the handle's device; calls are ordered on the caller's hipStream_t.
 *
 * Errors: functions return SEPVAD_OK (0) or a negative status; sepvad_last_error() gives a
 * thread-local message. The Python host turns a non-zero status into RuntimeError.
 */
#ifndef SEPVAD_H
#define SEPVAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEPVAD_ABI_VERSION 2

enum {
  SEPVAD_OK = 0,
  SEPVAD_E_ARG = -1,      /* invalid argument / unsupported configuration */
  SEPVAD_E_WEIGHTS = -2,  /* missing or mis-shaped state_dict entry */
  SEPVAD_E_HIP = -3,      /* a HIP runtime call failed */
  SEPVAD_E_SHAPE = -4     /* B/N outside what the handle supports */
};

/* TCN residual mode (model/model.py:347-352). */
enum { SEPVAD_LN_PLAIN = 0, SEPVAD_LN_RECURSIVE = 1, SEPVAD_LN_RESIDUAL = 2 };

/* Arithmetic of the pointwise (1x1) GEMMs (reference model/model.py:104,114,324). FP32 and F16X3 meet the
 * fp32 parity gates (max-abs <= 1e-4):
 *   FP32:  v_mfma_f32_32x32x2_f32 (exact fp32 fma chain);
 *   F16X3: fp32-equivalent split: x = hi + lo (fp16 each), acc += hi*hi + hi*lo + lo*hi on
 *          v_mfma_f32_32x32x16_f16 with fp32 accumulation (default; 16x the fp32 MFMA rate per pass).
 * F16 and BF16 are the reduced-precision arms (BASELINE cfg 2 "bf16", cfg 5 "fp16 vs fp32"): operands
 * rounded to fp16 / bf16, one v_mfma_f32_32x32x16_{f16,bf16} product, fp32 accumulation; everything outside
 * the GEMMs stays fp32. Their tolerance vs fp32 is measured, not gated.
 * Weight condition of F16X3 (DESIGN.md §4b "Weight statistics", tests/test_gpu_profiles.py): with the fp16 lo plane
 * (SEPVAD_WLO_F16, the multi-kernel schedule) the parity gates -- waveforms 1e-4, VAD labels, masks_b 2e-4 -- hold
 * under signed gains and PReLU slopes in {-0.25, 0, 1, 1.5}, GroupNorm beta and conv biases offset by 2 and 3, zero
 * rows / zero gammas, and gammas, gains and input columns spread over 2^-3..2^3. The default int8 lo plane keeps the
 * waveform and VAD gates under all of these; its steps are absolute (2^-19 of a row's largest weight), so where a few
 * input columns dominate every row (the `spread` profile: columns x 2^-U[0,3]) the pre-sigmoid masks_b, not the
 * waveforms, leave the 2e-4 gate: 2.2e-4 measured against 6.6e-5 with the fp16 lo plane and 5.6e-5 in FP32. */
enum { SEPVAD_PREC_FP32 = 0, SEPVAD_PREC_F16X3 = 1, SEPVAD_PREC_F16 = 2, SEPVAD_PREC_BF16 = 3 };
/* Storage of the weight lo plane of F16X3 in the fused TCN (the 1x1 convs of model/model.py:104,114); the row-scaled
 * weight w*2^-e = hi + lo with hi fp16 and |lo| <= 2^-12:
 *   I8 (default): lo as int8 steps of 2^-19 (biased by 128), widened exactly to fp16 in registers by v_perm_b32 + one
 *          packed fp16 fma: 3 bytes per weight streamed instead of 4, absolute lo error <= 2^-20 of the row's largest
 *          weight. k_tcn -1.8 % shader cycles at cfg 2; every parity gate at its fp16-lo bound.
 *   F16:   lo as fp16 (rounds 1-2; 4 bytes per weight).
 *   E4M3:  lo as OCP e4m3 (scaled by 2^19), widened by v_cvt_scalef32_pk_f16_fp8: 3 bytes per weight, the cheapest
 *          widening (k_tcn -4.0 %), but 4 significant bits of lo move masks / est by up to 1.4e-5 of their range
 *          (others: below 1e-5), so it is opt-in. tools/lo_plane_precision.py emulates the formats on the CPU.
 * Waveforms stay within 3.1e-6 of the oracle with 0 VAD label flips in all three (tests/test_gpu_precision.py).
 * The multi-kernel schedule and the head always use F16. Environment override at create time: SEPVAD_WLO=f16|e4m3|i8. */
enum { SEPVAD_WLO_E4M3 = 0, SEPVAD_WLO_F16 = 1, SEPVAD_WLO_I8 = 2 };

/* SeparationModel kwargs that change the computation (model/model.py:362-366). */
typedef struct SepVadConfig {
  int32_t n_fft;                      /* n_fftBins; 512 */
  int32_t bn_dim;                     /* BN_dim; must be n_fft/2 */
  int32_t h_dim;                      /* H_dim; must be 2*bn_dim */
  int32_t layer;                      /* blocks per stack */
  int32_t stack;                      /* stacks; blocks = layer*stack */
  int32_t num_spk;                    /* 2 */
  int32_t tf_attention;               /* TF_Attention after every block */
  int32_t ln_mode;                    /* SEPVAD_LN_* */
  int32_t final_vad;                  /* VAD head present */
  int32_t final_vad_masked_speakers;  /* VAD on masked magnitudes instead of pre-sigmoid masks */
  int32_t noisy_phase;                /* est = (|X| m) e^{j angle X} instead of X m */
  int32_t activity_input;             /* 3x3 activity gate on the dB spectrum */
  int32_t precision;                  /* SEPVAD_PREC_* */
} SepVadConfig;

/* forward()'s inference_kw (only_inference.py:102-108; model/model.py:444-457). */
typedef struct SepVadInferKw {
  int32_t enabled;                    /* 0 == empty dict: the branch is skipped */
  int32_t filter_signals_by_smo_vad;
  int32_t filter_signals_by_unsmo_vad;
  int32_t length_smoothing_filter;    /* accepted, no effect on the math (reference overrides the taps) */
  float threshold_activated_vad;
  int32_t return_smoothed_vad;
} SepVadInferKw;

/* Caller-owned outputs of one forward (device pointers). T = 1 + N / (n_fft/2). */
typedef struct SepVadOutputs {
  float* sep;       /* [B, num_spk, N] f32, required                                        */
  float* vad;       /* [B, num_spk, T] f32 (probabilities, or {0,1} when smoothed); NULL if !final_vad */
  void* est;        /* [B, num_spk, n_fft/2+1, T] complex64 (re,im interleaved); nullable  */
  float* spectrum;  /* [B, n_fft/2+1, T] gated dB spectrum (self.spectrum); nullable         */
  float* masks_b;   /* [B, num_spk*(n_fft/2+1), T] pre-sigmoid masks (self.masks_b); nullable */
  float* mask;      /* [B, num_spk, n_fft/2+1, T] post-sigmoid (self.mask_per_speaker); nullable */
} SepVadOutputs;

typedef struct sepvad_model* sepvad_handle;

/* Replaces SeparationModel(**args) + load_state_dict(strict=True) (model/model.py:361-400,
 * only_inference.py:57-61). `tensors[i]` is a HOST float32 array of `numels[i]` elements named
 * `names[i]` (reference state_dict keys). Folds weight-norm (w = v * (g/||v||)) once, packs the
 * weights for the kernels and uploads them to `device`. Returns NULL on error. */
sepvad_handle sepvad_create(const SepVadConfig* cfg, const float* const* tensors,
                            const char* const* names, const int64_t* numels, int32_t n,
                            int32_t device);

/* Pre-size the workspace for up to B utterances of N samples (so forward never allocates). */
int32_t sepvad_reserve(sepvad_handle h, int32_t B, int32_t N);

/* Switch the GEMM arithmetic of later forwards (SEPVAD_PREC_*); weights for both are resident. */
int32_t sepvad_set_precision(sepvad_handle h, int32_t precision);

/* Weight lo-plane format of the fused TCN for later F16X3 forwards (SEPVAD_WLO_*); all three are resident. */
int32_t sepvad_set_weight_lo(sepvad_handle h, int32_t mode);

/* HOST function: the packer's float -> OCP e4m3fn encoder (round to nearest even, saturating at 448), as used
 * for the weight lo plane; out[i] = e4m3(in[i]). Lets the host-side quantisation be checked without a GPU. */
int32_t sepvad_e4m3_encode(const float* in, uint8_t* out, int64_t n);

/* Replaces SeparationModel.forward(x, inference_kw) (model/model.py:402-461).
 * x: device [B, N] f32. kw may be NULL (== empty dict). Stream-ordered on `stream`
 * (a hipStream_t; NULL = default stream). */
int32_t sepvad_forward(sepvad_handle h, const float* x, int32_t B, int32_t N,
                       const SepVadOutputs* out, const SepVadInferKw* kw, void* stream);

/* Same as sepvad_forward with a row stride: utterance b starts at x + b * ldx (ldx >= N).
 * The streaming wrapper passes its overlapping windows this way (window k of stream b is
 * x + b * N_total + k * hop, model/online_class_unknown_targets.py:39-41) without a gather copy. */
int32_t sepvad_forward_strided(sepvad_handle h, const float* x, int64_t ldx, int32_t B, int32_t N,
                               const SepVadOutputs* out, const SepVadInferKw* kw, void* stream);

/* Replaces the window loop of OnlineSaving.calc_online (model/online_class_unknown_targets.py:80-97) as ONE
 * forward: n_win windows of N samples for each of n_streams signals, window k of stream b starting at
 * x + b * ld_stream + k * hop (no gather copy); utterance u = k * n_streams + b of the outputs (so window k of
 * every stream is a contiguous [n_streams, ...] block). Requires (n_win - 1) * hop + N <= ld_stream. */
int32_t sepvad_forward_windows(sepvad_handle h, const float* x, int64_t ld_stream, int32_t n_streams, int32_t n_win,
                               int64_t hop, int32_t N, const SepVadOutputs* out, const SepVadInferKw* kw,
                               void* stream);

/* Split each forward's batch into n (1..4) utterance chunks that run concurrently on internal
 * streams forked from / joined to the caller's stream (results are bitwise identical for any n:
 * every reduction is per utterance). Default 1, or the SEPVAD_SPLIT environment variable. */
int32_t sepvad_set_split(sepvad_handle h, int32_t nsplit);

/* Select the TCN schedule of later forwards: 1 (default, or env SEPVAD_FUSED) = the whole separator stack
 * as one persistent launch when the GEMMs are F16X3 / F16 / BF16 and T <= 8192 (groups of ceil(T/32) <= 256 workgroups per
 * utterance); 0 = one launch per stage (4 per block). Both meet the same parity gates.
 * Every other environment variable a forward reads is a test or diagnostics knob: one table, KNOBS in csrc/forward.hip. */
int32_t sepvad_set_fused(sepvad_handle h, int32_t on);
/* Synchronises the device and reports the schedule of the last forward and the persistent launch's
 * health: *used = 0 if it ran one launch per stage, else the 32-frame slices per workgroup of its persistent launch
 * (1, or 2 when the batch needs more than one round of one-slice workgroups; both give the same bits); returns
 * SEPVAD_OK, or SEPVAD_E_HIP if a group hand-off gave up (a bounded wait timed out; outputs of that forward are
 * invalid). */
int32_t sepvad_fused_status(sepvad_handle h, int32_t* used);

/* The side attributes of the LAST forward on `stream` (self.spectrum, self.masks_b, self.mask_per_speaker,
 * reference model/model.py:412-429), materialised from that stream's workspace: `out->spectrum`, `out->masks_b`
 * and `out->mask` (each nullable; the other members are ignored) receive exactly the values the forward would
 * have written to them. Valid until the next forward on the same stream. The Python host calls this when
 * one of the attributes is first read, so a forward whose side attributes nobody reads does not pay for
 * their bin-major copies. SEPVAD_E_ARG if no forward ran on `stream`. */
int32_t sepvad_side_outputs(sepvad_handle h, const SepVadOutputs* out, void* stream);

/* The forward that sepvad_side_outputs would read: *seq = forwards enqueued so far on `stream` (a per-stream
 * sequence id), *B / *N = its shape. SEPVAD_E_ARG if no forward ran on `stream`. */
int32_t sepvad_last_forward(sepvad_handle h, void* stream, int64_t* seq, int32_t* B, int32_t* N);

/* sepvad_side_outputs of ONE forward: fails with SEPVAD_E_ARG (no write) unless forward `seq` of shape (B, N)
 * (from sepvad_last_forward right after it) is still the last forward on `stream`, so a later forward of another
 * shape can never be copied into buffers sized for this one (the reference's attributes belong to the forward that
 * set them, model/model.py:412-429). */
int32_t sepvad_side_outputs_of(sepvad_handle h, const SepVadOutputs* out, void* stream, int64_t seq, int32_t B,
                               int32_t N);

/* Diagnostics: with SEPVAD_TCN_CLOCK=1 in the environment every k_tcn launch records {~(min start), max end (100 MHz
 * wall clock over all workgroups), workgroup 0: start / end wall clock, start / end shader clock (s_memtime), 0, 0}.
 * Synchronises the device and copies the last min(max_records, recorded) records, oldest first, as 8 uint64 each;
 * *n = records available (at most 4096). */
int32_t sepvad_tcn_clock(sepvad_handle h, uint64_t* out, int32_t max_records, int32_t* n);

/* Synchronises `stream` and frees the per-stream context (workspace, hand-off words, pinned give-up word) the handle
 * holds for it. Contexts are otherwise kept (at most SEPVAD_MAX_STREAM_CTX = 32 per handle by default, the least
 * recently used evicted after a device-wide sync -- the host waits until every stream on the device is idle, other
 * handles' and the application's work included -- because its stream may already be destroyed with work pending). */
int32_t sepvad_release_stream(sepvad_handle h, void* stream);

/* Kernel-level test entries of the forward's own front and back end (the fused schedule's k_stft_gate and
 * k_istft_pair), in the frame-major layouts the forward's workspace holds (Tp = roundup(T, 64), T = 1 + N / 256):
 * sepvad_stft_gate_test: X_fm [B][Tp][257] complex (DC zeroed) and db_fm [B][Tp][260] = 10 log10(clamp(|X|^2, 1e-10))
 * of x [B][N] (model/model.py:16-25,408-412; the activity gate's outputs go to the stream's workspace).
 * sepvad_istft_pair_test: est[b][s] = X_fm[b] * sigmoid(masks_fm[b][:, 257 s + k]) and y[b][s] = torch.istft(est,
 * center=True, length=N) (model/model.py:429-460, no VAD gain), y [B][2][N], est (nullable) [B][2][257][T] complex,
 * masks_fm [B][Tp][576]. Tests only. */
int32_t sepvad_stft_gate_test(sepvad_handle h, const float* x, int32_t B, int32_t N, void* X_fm, float* db_fm,
                              void* stream);
int32_t sepvad_istft_pair_test(sepvad_handle h, const void* X_fm, const float* masks_fm, int32_t B, int32_t N, float* y,
                               void* est, void* stream);

/* Block-level parity probe of the fused TCN: while `dump` (device, >= 3 * B * roundup(T, 64) * 256 floats) is
 * set, forwards that run the fused TCN in one launch write dump[0] = TCN.LN output x'_0 (model/model.py:333),
 * dump[1] = block 0's DepthConv1d output (:144) and dump[2] = block 0's TF_Attention output (:207), each
 * [B][roundup(T, 64)][256] channel-last. NULL disables. F16X3 arithmetic only (a separate instantiation of the
 * kernel); tests only (the reference golden's tcn_in, blk0_res, blk0_att). */
int32_t sepvad_set_tcn_dump(sepvad_handle h, float* dump);

/* ---- streaming wrapper (model/online_class_unknown_targets.py:72-105) -------------------------
 * Signals are [B, 2, ld] f32 device arrays (speaker rows of stride ld).
 *
 * Replaces PITLossWrapper(nn.L1Loss(), pit_from="pw_pt")(est, ref, return_incides=True)
 * (model/pit_wrapper.py:77-140,149-177,261-312) on est[..., 0:L] vs ref[..., 0:L]: pairwise L1
 * means over batch and samples (nn.L1Loss reduces the batch too, so the permutation is shared by
 * the whole batch), loss set over the 2 permutations, first minimum. Writes perm_out [B, 2] int64
 * (batch_indices), loss_out (min loss) and pw_out [2, 2] (pairwise losses), each nullable.
 * scratch: device buffer of at least SEPVAD_PIT_SCRATCH_BYTES. Deterministic. */
#define SEPVAD_PIT_SCRATCH_BYTES 16448
int32_t sepvad_pit_l1(const float* est, int64_t est_ld, const float* ref, int64_t ref_ld, int32_t B, int64_t L,
                      void* scratch, int64_t* perm_out, float* loss_out, float* pw_out, void* stream);
/* The same in two steps, for a stream batch sharded over ranks (nn.L1Loss means over the WHOLE batch,
 * model/pit_wrapper.py:172-177): sepvad_pit_l1_sums writes this device's 4 pairwise L1 sums (double,
 * fixed order) to sums[4] (device); the caller all-reduces them over the ranks (RCCL, 32 bytes); then
 * sepvad_pit_l1_choose turns sums / count (count = total rows x L over all ranks) into the permutation
 * for this device's B rows, the loss and the pairwise means, exactly as sepvad_pit_l1 does. */
int32_t sepvad_pit_l1_sums(const float* est, int64_t est_ld, const float* ref, int64_t ref_ld, int32_t B, int64_t L,
                           void* scratch, double* sums, void* stream);
int32_t sepvad_pit_l1_choose(const double* sums, double count, int32_t B, int64_t* perm_out, float* loss_out,
                             float* pw_out, void* stream);

/* Replaces reorder_source_mse(preds, batch_indices) (model/combined_loss.py:63-78) fused with
 * OnlineSaving.update_online_signal (online_class_unknown_targets.py:28-37):
 * dst[b, i, d0 + n] = src[b, perm[b, i], s0 + n] for n < H (perm NULL = identity). */
int32_t sepvad_stream_append(const float* src, int64_t src_ld, int64_t s0, int32_t B, int64_t H,
                             const int64_t* perm, float* dst, int64_t dst_ld, int64_t d0, void* stream);

/* ---- live sessions: the same wrapper fed a chunk at a time ------------------------------------
 * Stateless like the entries above: the caller owns the rings and the counters (live.py does).
 *
 * Extends get_truncated_signal (model/online_class_unknown_targets.py:39-41) to input that arrives in
 * chunks. ring is [rows][2R] f32, a mirrored ring: sample j of chunk row r ([rows][chunk_ld], n samples) is
 * stored at ring[r][(pos + j) % R] and again at that index + R, so after any push every span of up to R most
 * recent samples is contiguous in memory and a window (or several, hop apart) goes to sepvad_forward_strided /
 * sepvad_forward_windows with a row stride of 2R and no gather copy. The caller advances pos by n modulo R.
 * SEPVAD_E_ARG (nothing launched) for a null pointer, n < 1, n > R, pos outside [0, R) or chunk_ld < n. */
int32_t sepvad_ring_push(const float* chunk, int64_t chunk_ld, int32_t rows, int64_t n, float* ring, int64_t R,
                         int64_t pos, void* stream);

/* The PIT-L1 of sepvad_pit_l1 (model/pit_wrapper.py:149-177,261-312) applied to each row on its own: what the
 * window loop (model/online_class_unknown_targets.py:72-97) computes for a batch of one stream, for B
 * independent streams in one call. Row b's perm_out[b][2], loss_out[b] and pw_out[b][4] (each nullable) have
 * the bits of sepvad_pit_l1 called on that row alone with B = 1: the same blocks per row, accumulation and
 * reduction order. Ties keep the identity permutation. scratch: device buffer of scratch_bytes >=
 * sepvad_pit_l1_rows_scratch_bytes (host query; negative for B < 1, B > 65535 or L < 1). */
int64_t sepvad_pit_l1_rows_scratch_bytes(int32_t B, int64_t L);
int32_t sepvad_pit_l1_rows(const float* est, int64_t est_ld, const float* ref, int64_t ref_ld, int32_t B, int64_t L,
                           void* scratch, int64_t scratch_bytes, int64_t* perm_out, float* loss_out, float* pw_out,
                           void* stream);

/* One emitted window: reorder_source_mse (model/combined_loss.py:63-78) + update_online_signal
 * (model/online_class_unknown_targets.py:28-37) on the window's last hop, kept as a chunk and a tail instead of
 * a growing signal. win is one window's separation [B][2][win_ld] of N samples. For row b, output speaker i and
 * p = perm[b][i] (perm NULL = identity), n < H:
 *   out[b][i][d0 + n] = win[b][p][N - H + n]                       (out [B][2][out_ld], the caller's chunk)
 *   tail[b][i][(tpos + n) % Rt] and the same index + Rt            (mirrored ring [B][2][2Rt]: the stitched
 *                        signal's last Rt samples stay contiguous for the next window's PIT, :87-91)
 *   vad_out[b][i][v0 + j] = vad[b][p][T - nf + j], j < nf           (vad nullable: [B][2][T] of the window)
 * SEPVAD_E_ARG (nothing launched) for a null pointer, H > Rt, H > N, nf > T, tpos outside [0, Rt) or offsets
 * that leave their rows. */
int32_t sepvad_live_stitch(const float* win, int64_t win_ld, int64_t N, int32_t B, int64_t H, const int64_t* perm,
                           float* out, int64_t out_ld, int64_t d0, float* tail, int64_t Rt, int64_t tpos,
                           const float* vad, int32_t T, int32_t nf, float* vad_out, int64_t vad_ld, int64_t v0,
                           void* stream);

/* ---- quality metrics (model/combined_loss.py:16-56 calc_sisdr == model/metric.py:61-101
 * scale_invariant_signal_distortion_ratio; PIT over it: metric.py:258 pit_si_sdr) --------------------
 * out[r] = SI-SDR(P[pidx[r]], Tg[tidx[r]]) in dB for r < R: rows of N samples with row strides p_ld / t_ld,
 * pidx / tidx nullable (identity). eps = float32 epsilon; zero_mean as the reference's flag. Moments in
 * double, fixed-order reductions (bitwise reproducible). Device pointers, stream-ordered. */
int32_t sepvad_si_sdr(const float* P, int64_t p_ld, const float* Tg, int64_t t_ld, int64_t N, int32_t R,
                      const int32_t* pidx, const int32_t* tidx, int32_t zero_mean, float* out, void* stream);

/* Replaces signal_noise_ratio (model/metric.py:104-143; PIT over it: metric.py:255-256 pit_snr) with the argument
 * list of the SI-SDR entry above: out[r] = 10 log10((<t,t> + eps) / (<t - p, t - p> + eps)) in dB, p = P[pidx[r]],
 * t = Tg[tidx[r]], optional zero mean, eps = float32 epsilon. The same five double moments, fixed order. */
int32_t sepvad_snr(const float* P, int64_t p_ld, const float* Tg, int64_t t_ld, int64_t N, int32_t R,
                   const int32_t* pidx, const int32_t* tidx, int32_t zero_mean, float* out, void* stream);

/* ---- STOI (model/stoi_metric.py:207-301 stoi, extended=False; model/metric.py:207-223 Stoi; the extended
 * form follows below) ----------
 * HOST function, no GPU needed: the design the device path uses for signals sampled at fs_sig (8000, 10000 or
 * 16000 Hz). taps (capacity `cap` floats) receive the resampling window h / sum(h) of _resample_window_oct and
 * resample_oct (stoi_metric.py:11-52), computed in double and rounded to float: 581 taps at 16 kHz (5/8), 365 at
 * 8 kHz (5/4), none at 10 kHz. info[SEPVAD_STOI_INFO_LEN] receives {up, down, ntaps, 15} followed by the 15
 * third-octave bands of thirdoct / OBM (stoi_metric.py:55-85,201) as {first bin, one past the last bin} pairs of the
 * 512-point spectrum at 10 kHz. taps NULL = size query. SEPVAD_E_ARG on a short buffer or another rate. */
#define SEPVAD_STOI_INFO_LEN 34
int32_t sepvad_stoi_filter(int32_t fs_sig, float* taps, int32_t cap, int32_t* info);

/* HOST function: bytes of device scratch the STOI entry below needs for R pairs of N samples at fs_sig (the
 * resampled signals, frame energies, kept-frame lists and band magnitudes, sized for every frame kept). Negative
 * status if the rate is unsupported, R is outside 1..65535 or N gives no frame (256 samples or fewer at 10 kHz). */
int64_t sepvad_stoi_scratch_bytes(int32_t R, int64_t N, int32_t fs_sig);

/* Replaces stoi(x, y, fs_sig) (model/stoi_metric.py:207-301, extended=False) for R signal pairs in one call:
 * out[r] = STOI of clean X[xidx[r]] against estimate Y[yidx[r]] (rows of N samples with row strides x_ld / y_ld,
 * index arrays nullable = identity, so PIT pairings need no gather). Resampling to 10 kHz, silent-frame removal
 * (40 dB below the loudest clean frame), 512-point STFT, 15 third-octave bands and the clipped, normalised
 * correlation over windows of 30 frames all run on the device without a host synchronisation; the arithmetic is
 * double apart from the float store of the resampled signals. frames (nullable) receives M, the number of spectra
 * left after silence removal; out[r] is exactly 1e-5 when M < 30 (stoi_metric.py:251-256, without its warning).
 * scratch: 256-byte aligned device memory of scratch_bytes >= the size query above. Fixed-order reductions per
 * pair: bitwise reproducible, independent of R and of the other pairs. Device pointers, stream-ordered (the first
 * call per device and rate uploads the design tables synchronously). */
int32_t sepvad_stoi(const float* X, int64_t x_ld, const float* Y, int64_t y_ld, int64_t N, int32_t R,
                    const int32_t* xidx, const int32_t* yidx, int32_t fs_sig, void* scratch, int64_t scratch_bytes,
                    double* out, int32_t* frames, void* stream);

/* ---- Extended STOI (ESTOI; stoi(x, y, fs_sig, extended=True), stoi_metric.py:177-193,268-271) ----------
 * modes of the two entries below: a bit mask of the results asked for. */
#define SEPVAD_STOI_CLASSIC 1
#define SEPVAD_STOI_EXTENDED 2

/* HOST function: bytes of device scratch sepvad_stoi_ex needs: with SEPVAD_STOI_CLASSIC alone the size of the
 * classic query above, with SEPVAD_STOI_EXTENDED that plus one double per pair and chunk of 64 segments. Negative
 * status as above, and if modes is outside 1..3. */
int64_t sepvad_stoi_ex_scratch_bytes(int32_t R, int64_t N, int32_t fs_sig, int32_t modes);

/* sepvad_stoi's arguments plus modes: the front end (resampling, silence removal, spectra, band magnitudes) runs once,
 * then the correlation stage of every mode asked for. out_stoi[r] (SEPVAD_STOI_CLASSIC) has the bits sepvad_stoi
 * gives: it is the same launches. out_estoi[r] (SEPVAD_STOI_EXTENDED) is extended STOI: for every window j of 30
 * spectra and each signal, the 15 x 30 block of band magnitudes has the mean over its 30 frames subtracted from every
 * band row and the row divided by its norm, then the mean over its 15 bands subtracted from every frame column and
 * the column divided by its norm; out_estoi[r] = sum over windows, bands and frames of the product of the two
 * signals' blocks / (30 J), J = M - 29 windows. The reference adds 2.2e-16 * randn noise before each centring; that
 * term is left out (it moves the reference's value by 1e-15 where the value does not depend on the draw).
 * Degenerate rule: a row or column whose norm is zero becomes a row or column of zeros (the reference normalises
 * its noise there, so its value is a random draw), and an all-zero estimate scores exactly 0.0, as with classic STOI.
 * Zero includes the rounding remainder of an exact zero: a row norm up to 2^-40 sqrt(30) times the row's mean (30
 * equal magnitudes) and a column norm up to 2^-40 (15 unit-norm rows that agree in that frame); dividing by such a
 * norm would turn rounding into a unit vector. M < 30 stores exactly 1e-5. All in double; every sum has a fixed order that depends on the pair
 * alone (no atomics): the result is bitwise independent of R, of the other pairs and of repeated runs.
 * An output pointer that is missing for a requested mode is SEPVAD_E_ARG; one for a mode not requested is ignored.
 * frames nullable. Every refusal (null pointers, x_ld / y_ld < N, rate, shape, modes, scratch size or alignment)
 * is made on the host before any device call. */
int32_t sepvad_stoi_ex(const float* X, int64_t x_ld, const float* Y, int64_t y_ld, int64_t N, int32_t R,
                       const int32_t* xidx, const int32_t* yidx, int32_t fs_sig, void* scratch, int64_t scratch_bytes,
                       int32_t modes, double* out_stoi, double* out_estoi, int32_t* frames, void* stream);

/* Replaces Accuracy_Vad()(preds, targets, _) (model/metric.py:163-177): labels = preds > 0.5 (NaN kept),
 * written back into preds when in_place (the reference masks its argument in place); out[0] = fraction of
 * labels equal to targets over [B, S, T], out[1 + s] = the same for speaker s (S <= 8). Device pointers,
 * contiguous [B][S][T] f32, stream-ordered; integer counts (exact). */
int32_t sepvad_vad_accuracy(float* preds, const float* targets, int32_t B, int32_t S, int32_t T, int32_t in_place,
                            float* out, void* stream);

/* ---- the evaluation criterion of test.py (test.py:49-64 builds it, :129-172 uses it) ----------------
 * One pass over the five rows of every utterance (two estimates, two targets, the mixture) gives 16 double
 * moments; every separation number of a test.py step is a closed form of them (csrc/eval.hip). */
enum { SEPVAD_SDR_SISDR = 0, SEPVAD_SDR_SDSDR = 1, SEPVAD_SDR_SNR = 2 };  /* PairwiseNegSDR's sdr_type */
/* Columns of the per-utterance score sheet (dB, float32, zero-mean, eps = float32 epsilon as sepvad_si_sdr). */
enum {
  SEPVAD_EV_SISDR0 = 0,      /* calc_sisdr(est reordered by perm, tgt)[b, 0]  (test.py:131-134) */
  SEPVAD_EV_SISDR1,          /* ... [b, 1] */
  SEPVAD_EV_SISDR_MIX0,      /* calc_sisdr(mix, tgt)[b, 0]  (test.py:139-142) */
  SEPVAD_EV_SISDR_MIX1,
  SEPVAD_EV_PIT_SISDR,       /* pit_si_sdr of utterance b: best permutation by mean SI-SDR (metric.py:258; test.py:151) */
  SEPVAD_EV_PIT_SNR,         /* pit_snr of utterance b (metric.py:255-256) */
  SEPVAD_EV_PIT_SISDR_MIX,   /* the same two with the mixture as both estimates (test.py:152) */
  SEPVAD_EV_PIT_SNR_MIX,
  SEPVAD_EV_COLS
};
/* means[4] of sepvad_eval_separation */
enum { SEPVAD_EV_MEAN_LOSS = 0, SEPVAD_EV_MEAN_PIT_SISDR, SEPVAD_EV_MEAN_PIT_SNR, SEPVAD_EV_MEAN_SI_SDRI };

/* HOST query: bytes of device scratch sepvad_eval_separation needs for B utterances of N samples (SEPVAD_E_ARG
 * for B < 1, B > 65535, N < 1 or N > 2^40). Monotone in B and in N. */
int64_t sepvad_eval_scratch_bytes(int32_t B, int64_t N);

/* Replaces PITLossWrapper(PairwiseNegSDR(sdr_type, zero_mean, take_log, EPS), pit_from="pw_mtx") (model/sdr.py:48-86,
 * model/pit_wrapper.py:100-145,287-312; built by test.py:49-56, called through CombinedLoss at test.py:129-130) and
 * the separation metrics of the same step: calc_sisdr of the reordered estimates and of the mixture (test.py:134,142),
 * pit_si_sdr / pit_snr of both (test.py:149-152, model/metric.py:255-258) and si_sdri (test.py:179-181,
 * model/metric.py:145-160). est, tgt: [B][2][ld] rows of N samples with unit sample stride (speaker stride ld, batch
 * stride 2 ld, as sepvad_pit_l1_rows); mix: [B][mix_ld], nullable (its moments are then 0 and the mixture columns
 * are those of a silent mixture). Outputs (device): pw[b][i][j] = loss of estimate i against target j;
 * perm[b][j] = the estimate assigned to target j, (0,1) or (1,0), the identity on a tie; min_loss[b] = the chosen
 * permutation's mean loss; sheet[b][SEPVAD_EV_COLS] (nullable); means = {mean min_loss, pit_si_sdr, pit_snr, si_sdri}.
 * Sums in double in a fixed order, float32 on store: bitwise reproducible, and utterance b's outputs do not depend
 * on B or on the rows' alignment. scratch: 8-byte aligned device memory of scratch_bytes >= the query above.
 * SEPVAD_E_ARG (nothing launched) for a null pointer (mix and sheet excepted), B < 1, B > 65535, N < 1, N > 2^40, a
 * row stride below N (mix_ld only with mix), an unknown sdr_type, a short scratch or a scratch pointer that is not
 * 8-byte aligned. */
int32_t sepvad_eval_separation(const float* est, int64_t est_ld, const float* tgt, int64_t tgt_ld, const float* mix,
                               int64_t mix_ld, int32_t B, int64_t N, int32_t sdr_type, int32_t zero_mean,
                               int32_t take_log, double eps, void* scratch, int64_t scratch_bytes, float* pw,
                               float* min_loss, int64_t* perm, float* sheet, float* means, void* stream);

/* Replaces BinaryCrossEntropyLoss_Mean (model/combined_loss.py:120-138) on the VAD track reordered by perm
 * (combined_loss.py:109-110), the pairwise table behind pit_CE_vad (model/metric.py:264; model/pit_wrapper.py:172-177
 * get_pw_losses), the per-speaker confusion_matrix(labels=[0., 1.]) of test.py:164,172 and calc_vad
 * (Our_utils/utils_test.py:67-73) on the masks reordered by perm (test.py:148,170). vad, labels: contiguous
 * [B][2][T] float32; labels equal to 2 count as 1 and, when fix_labels, are written back as 1 (the reference mutates
 * its argument). perm: [B][2] int64 on the device, nullable (identity); pred[b][s] = vad[b][perm[b][s]].
 *   bce_rows[b] = sum over s, t of w (-(y log p + (1 - y) log(1 - p))), w = 0.36 y + 0.64 (1 - y), logs clamped at
 *                 -100; bce_mean = their mean over the batch;
 *   pw_ce[i][j] = the same sum over the whole batch and all frames of vad[:, i] against labels[:, j];
 *   conf[b][s]  = (tn, fp, fn, tp) of pred > 0.5 against the labels, pairs with a label other than 0 / 1 left out
 *                 (a NaN pred is not > 0.5 and counts as prediction 0);
 *   simple[b][s][t] (int64, with masks [B][2][257][T] post-sigmoid) = at least 65 of the 257 bins of
 *                 masks[b][perm[b][s]][:, t] are >= 0.5; conf_simple (nullable) = its confusion counts.
 * masks NULL: simple and conf_simple are not touched. vad and labels both NULL with masks and simple given: only
 * simple is written. SEPVAD_E_ARG (nothing launched) for any other null pointer (perm, masks, simple without masks
 * and conf_simple excepted), masks without simple, B < 1, B > 65535 or T < 1. */
int32_t sepvad_eval_vad(const float* vad, float* labels, int32_t fix_labels, const int64_t* perm, const float* masks,
                        int32_t B, int32_t T, float* bce_rows, float* bce_mean, float* pw_ce, int32_t* conf,
                        int64_t* simple, int32_t* conf_simple, void* stream);

/* ---- the training criterion's backward (trainer/trainer.py:57-63: criterion(...) then loss.backward()) ----------
 * The gradients of CombinedLoss (model/combined_loss.py:93-138) over PITLossWrapper(PairwiseNegSDR(...), "pw_mtx")
 * (model/sdr.py:48-86) and the weighted BCE with respect to the separated signals and the VAD track. The forward is
 * sepvad_eval_separation and sepvad_eval_vad as they are; the gradient of an estimate row is a combination of that row
 * and of its paired target row, both centred when zero_mean, whose coefficients follow from the forward's moments
 * (csrc/criterion.hip). */
enum { SEPVAD_CRIT_COEF = 6 };  /* doubles per estimate row in coef: c_t, c_n, a, mean of the estimate row, mean of the
                                   paired target row (both 0 without zero_mean), index of the paired target */

/* After sepvad_eval_separation(est, tgt, ..., B, N, sdr_type, zero_mean, take_log, eps, scratch, ..., perm, ...) on
 * the same stream, with the same arguments and before anything else writes scratch: coef[b][i][SEPVAD_CRIT_COEF]
 * (device, doubles) such that, for estimate row i of utterance b paired with target j (perm[b][j] = i),
 *   d pw[b][i][j] / d est[b][i][n] = c_t t'[n] + c_n (e'[n] - a t'[n]),  e' = est[b][i] - mean e, t' = tgt[b][j] - mean t:
 * the exact derivative of model/sdr.py:54-86 with its EPS placement (finite zeros on silence). coef is all a backward
 * needs beside the rows: scratch may be overwritten afterwards. SEPVAD_E_ARG (nothing launched) for a null pointer,
 * B < 1, B > 65535, N < 1, N > 2^40, a row stride below N, an unknown sdr_type, a short or misaligned scratch. */
int32_t sepvad_criterion_coef(const float* est, int64_t est_ld, const float* tgt, int64_t tgt_ld, int32_t B, int64_t N,
                              int32_t sdr_type, int32_t zero_mean, int32_t take_log, double eps, const void* scratch,
                              int64_t scratch_bytes, const int64_t* perm, double* coef, void* stream);

/* Replaces loss.backward() through the reference criterion (trainer/trainer.py:57-63; model/sdr.py:48-86 and
 * model/combined_loss.py:93-138 under autograd). Two independent parts, either may be left out:
 *   est != NULL: grad_est[b][i][n] = g_sep / (2 B) (c_t t'[n] + c_n (e'[n] - a t'[n])) from coef (above), for
 *     est, tgt [B][2][ld] rows of N samples as sepvad_eval_separation takes them and grad_est [B][2][grad_ld];
 *     evaluated in double from the float32 samples, rounded once;
 *   vad != NULL: grad_vad[b][perm[b][s]][t] = g_vad / B  w (p - y) / max(p (1 - p), 1e-12f), p = vad[b][perm[b][s]][t],
 *     y = labels[b][s][t] (2 counts as 1), w = 0.36 y + 0.64 (1 - y); contiguous [B][2][T]; perm nullable (identity).
 * g_sep, g_vad: the upstream gradients of the two mean losses, one float32 each ON THE DEVICE (no host read). No
 * atomics: bitwise reproducible, independent of the rows' alignment and strides, and B times the gradient of
 * utterance b depends on its own rows only. SEPVAD_E_ARG (nothing launched) for B < 1, B > 65535, both parts left out,
 * a part with a null pointer (perm excepted), N < 1, N > 2^40, a row stride below N or T < 1. */
int32_t sepvad_criterion_backward(int32_t B, const float* est, int64_t est_ld, const float* tgt, int64_t tgt_ld,
                                  int64_t N, const double* coef, const float* g_sep, float* grad_est, int64_t grad_ld,
                                  const float* vad, const float* labels, const int64_t* perm, int32_t T,
                                  const float* g_vad, float* grad_vad, void* stream);

/* ---- backward of the back end and the VAD head (model/model.py:421-461) -----------------------------
 * loss.backward() through the forward's tail: torch.istft (model/model.py:438-441), the mask product
 * est = X sigmoid(masks) (:429-437; the noisy-phase form has the same gradient), the sigmoid, and the VAD head
 * (:153-179, called at :424-427) on the pre-sigmoid masks. The result is the gradient at masks_b [B][514][T], the trunk's
 * output, and the gradients of the VAD head's folded parameters (csrc/tail_grad.hip). There is no gradient
 * with respect to x or est, none through the inference-only branch (:444-457), and final_vad_masked_speakers is refused. */
enum { SEPVAD_TAIL_NPAR = 5166 };  /* vadw and gpar: conv1_1 weight [4][257][5] (folded: v g / |v|) | output_layer_vad weight
                                      [4][3] (folded) | its bias | BN_1 weight [4] | BN_1 bias [4] | relu_1 weight | conv1_1
                                      bias [4] */

/* Device bytes of scratch (256-byte aligned) that sepvad_tail_forward and sepvad_tail_backward need for B utterances of
 * N samples; negative status for B < 1, B > 32767, N <= 256 or N >= 2^29. */
int64_t sepvad_tail_scratch_bytes(int32_t B, int32_t N);

/* model/model.py:421-441 on given masks, through launches the forward has: the front end (X = STFT of x, rows of stride
 * ldx), the multi-kernel schedule's VAD conv1_1 and the forward's back end. masks_fm: pre-sigmoid masks frame-major
 * [B][Tp][576], Tp = T rounded up to 64, speaker q's bins at [257 q, 257 q + 257), the rest zero. sep [B][2][N]; vad
 * [B][2][T], ignored without final_vad. Nothing of a handle's forward is touched: every intermediate lives in scratch.
 * SEPVAD_E_ARG (nothing launched) for a null pointer, a bad shape, final_vad_masked_speakers, a short or misaligned
 * scratch. */
int32_t sepvad_tail_forward(sepvad_handle h, const float* x, int64_t ldx, const float* masks_fm, int32_t B, int32_t N,
                            void* scratch, int64_t scratch_bytes, float* sep, float* vad, void* stream);

/* The backward of model/model.py:421-441 at masks_b [B][2][257][T] (pre-sigmoid, bin-major, as the side attribute) for
 * the mixtures x the forward ran on. g_sep: upstream gradient of sep [B][2][N] with element strides gs_b, gs_s, gs_n
 * (>= 0: an expanded scalar has stride 0), NULL for zero; g_vad likewise for vad [B][2][T]. vadw [SEPVAD_TAIL_NPAR] device
 * doubles: the VAD head's parameters with the two weight-norm folds applied in double (needed with g_vad: the head's
 * backward runs in double, so the parameter gradients carry one float32 rounding, the caller's). g_masks [B][2][257][T]
 * (NULL: not wanted) receives d loss / d masks_b, every element written once; gpar [SEPVAD_TAIL_NPAR] doubles (NULL: not
 * wanted; written only with g_vad) the gradients of the VAD head's folded parameters added over the batch in a fixed order.
 * X is recomputed from x and the VAD head's forward from the masks (in double), so the call needs nothing a forward left
 * behind. No atomics: bitwise reproducible, independent of the gradients' strides, and utterance b's masks gradient
 * depends on its own rows only. SEPVAD_E_ARG (nothing launched) for a null x or masks_b, a bad shape, both gradients
 * NULL, nothing to compute, g_vad without a VAD head or without vadw, a negative stride, a short or misaligned scratch. */
int32_t sepvad_tail_backward(sepvad_handle h, const float* x, int64_t ldx, const float* masks_b, int32_t B, int32_t N,
                             const float* g_sep, int64_t gs_b, int64_t gs_s, int64_t gs_n, const float* g_vad,
                             int64_t gv_b, int64_t gv_s, int64_t gv_t, const double* vadw, void* scratch,
                             int64_t scratch_bytes, float* g_masks, double* gpar, void* stream);

/* ---- the output head with a backward (model/model.py:322-325,357) --------------------------------------
 * TCN.output = PReLU -> GroupNorm(1, 256, eps 1e-5) -> weight-normed Conv1d(256 -> 514, 1): from the trunk output y
 * [B][256][T] to masks_b [B][514][T] (both bin-major, as torch holds them), and loss.backward() through it: the stage
 * behind sepvad_tail_backward's g_masks (csrc/head_grad.hip). The entries take plain device pointers: no
 * handle, no allocation, no host synchronisation, nothing a forward left behind. hpar and gpar are
 * SEPVAD_HEAD_NPAR device doubles: the folded conv weight v g / |v| [514][256] | its bias [514] | GroupNorm weight [256] |
 * GroupNorm bias [256] | the PReLU slope. The fold and the weight-norm Jacobian are the caller's, in double. */
enum { SEPVAD_HEAD_NPAR = 132611 };

/* Device bytes of scratch (256-byte aligned) that sepvad_head_forward and sepvad_head_backward need for B utterances of
 * T frames; negative status for B < 1, B > 32767, T < 2 or T > 2^20. */
int64_t sepvad_head_scratch_bytes(int32_t B, int32_t T);

/* masks_b [B][514][T] = W z + bias with z = GroupNorm(PReLU(y)). The product runs on fp32 MFMA in fp32 chains of 16 terms
 * that are combined in double; the statistics and z are double arithmetic on the float32 y. SEPVAD_E_ARG (nothing
 * launched) for a null pointer, a bad shape, a short or misaligned scratch. */
int32_t sepvad_head_forward(const float* y, int32_t B, int32_t T, const double* hpar, void* scratch,
                            int64_t scratch_bytes, float* masks_b, void* stream);

/* The backward at y for G = d loss / d masks_b [B][514][T] with element strides g_b, g_m, g_t (>= 0: an expanded scalar
 * has stride 0). g_y [B][256][T] (NULL: not wanted) receives d loss / d y, every element written once; gpar
 * [SEPVAD_HEAD_NPAR] doubles (NULL: not wanted) the gradients of the folded parameters, added over time and the batch
 * in a fixed order. The forward's intermediates are recomputed from y. No atomics: bitwise reproducible, independent of
 * G's strides, and utterance b's g_y depends on its own rows only. SEPVAD_E_ARG (nothing launched) for a null y, G, hpar
 * or scratch, a bad shape, a negative stride, g_y and gpar both NULL, a short or misaligned scratch. */
int32_t sepvad_head_backward(const float* y, const float* G, int64_t g_b, int64_t g_m, int64_t g_t, int32_t B, int32_t T,
                             const double* hpar, void* scratch, int64_t scratch_bytes, float* g_y, double* gpar,
                             void* stream);

/* ---- streaming evaluation with known targets (model/online_class_known_targets.py:85-154) --------
 * The window loop of calc_online (:101-123) for the windows of one sepvad_forward_windows chunk in a fixed number of
 * launches (csrc/stream_eval.hip): each window's PIT against its target window
 * (criterion_separation, :106: PITLossWrapper(PairwiseNegSDR(sdr_type, zero_mean, take_log, eps), "pw_mtx"), with the
 * bits of sepvad_eval_separation on that window and target slice), the similarity PIT of the window's overlap against
 * the signal stitched so far (:108-117), reorder_source_mse and update_online_signal (:118-119, :29-38).
 * mode selects the similarity criterion (test.py:96-106). */
enum {
  SEPVAD_SE_NONE = 0,   /* criterion_similarity None: every window is appended under its target permutation */
  SEPVAD_SE_L1 = 1,     /* PITLossWrapper(nn.L1Loss(), "pw_pt"): one scalar per pair over batch and samples, so the
                           permutation is shared by the batch (as sepvad_pit_l1) */
  SEPVAD_SE_SISDR = 2   /* PITLossWrapper(calc_sisdr_loss, "pw_pt") (model/combined_loss.py:16-60): per-row losses, a
                           permutation per row */
};

/* HOST query: bytes of device scratch one sepvad_stream_eval call needs for n windows of B streams. SEPVAD_E_ARG for B
 * outside 1..65535, n < 1, H < 1, H > W, an unknown mode, 2 H > W or more than 4096 hops per window in a similarity
 * mode, or a chunk above 2^31 - 1 workgroups. Monotone in n. */
int64_t sepvad_stream_eval_scratch_bytes(int32_t B, int32_t n, int64_t W, int64_t H, int32_t mode);

/* sep: the separations of windows k0 .. k0 + n - 1 of K, window-major [n][B][2][sep_ld] with W samples per row
 * (sepvad_forward_windows' layout); window k starts at sample k H of its stream. tgt: [B][2][tgt_ld], the padded
 * targets, read in place at + k H (tgt_ld >= (K - 1) H + W). The caller owns every buffer and keeps the persistent
 * ones between the chunks of one signal (the entry is stateless, like the streaming entries above):
 *   raw    [B][2][raw_ld]     every window's own last hop at k H, un-permuted (raw_ld >= K H); window k is compared
 *                             with raw[k H - L_k, k H), L_k = min(k H, W - H), each hop under the permutation of the
 *                             window it came from; window 0 with its own last hop (the reference's seed, :109-111)
 *   perm   [K][B][2] int64    the permutation each window is appended under (perm[k][b][t] = the estimate that
 *                             becomes speaker t): the target permutation with SEPVAD_SE_NONE, else the similarity one
 *   online [B][2][online_ld]  the stitched signal, online[b][t][k H + i] = sep[k][b][perm[k][b][t]][W - H + i]
 * and the per-window outputs pw_tgt [K][B][2][2], loss_tgt [K][B], perm_tgt [K][B][2] int64 (pw, min_loss and perm of
 * sepvad_eval_separation; perm_tgt is nullable with SEPVAD_SE_NONE, where perm receives it) and pw_sim [K][G][2][2]
 * (the similarity PIT's pairwise table, estimate i against stitched speaker j; G = B with SEPVAD_SE_SISDR, 1 with
 * SEPVAD_SE_L1; nullable, unused with SEPVAD_SE_NONE). Chunks must arrive in window order; any split into chunks
 * gives the bits of one call. Ties keep the identity. Sums in double in a fixed order: bitwise reproducible.
 * scratch: 8-byte aligned device memory of scratch_bytes >= the query above.
 * SEPVAD_E_ARG (nothing launched) for a null pointer (the nullable ones excepted), what the query refuses, k0 < 0,
 * k0 + n > K, a row stride below its row's length, an unknown sdr_type, a short or misaligned scratch. */
int32_t sepvad_stream_eval(const float* sep, int64_t sep_ld, int32_t n, int32_t k0, int32_t K, int32_t B, int64_t W,
                           int64_t H, const float* tgt, int64_t tgt_ld, int32_t mode, int32_t sdr_type,
                           int32_t zero_mean, int32_t take_log, double eps, float* raw, int64_t raw_ld, float* online,
                           int64_t online_ld, int64_t* perm, int64_t* perm_tgt, float* pw_tgt, float* loss_tgt,
                           float* pw_sim, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- synthetic reverberant mixtures (BASELINE cfg 4): image-method room impulse responses --------
 * Replaces pyrirgen.generateRir / gen_rir (create_data/rirgen.cpp:115-351, create_data/pyrirgen.pyx)
 * as create_data/create_simulation_data.py:284-289 calls it. HOST function, double precision:
 * c sound speed (m/s), fs (Hz), mics [n_mics][3] and src [3] positions (m), room [3] dimensions (m),
 * beta: n_beta = 1 -> T60 (s; 0 = anechoic) or n_beta = 6 -> reflection coefficients, orientation [2]
 * (azimuth, elevation; nullable = 0), high_pass 1/0, n_dim 2/3, order (-1 = all), n_samples (-1 = T60 fs),
 * mic_type 'o','s','c','h','b'. Writes out [n_mics][n_samples] (cap doubles) and returns n_samples;
 * out NULL = size query. Negative status on bad arguments. */
int32_t sepvad_rir_generate(double c, double fs, const double* mics, int32_t n_mics, const double* src,
                            const double* room, const double* beta, int32_t n_beta, const double* orientation,
                            int32_t high_pass, int32_t n_dim, int32_t order, int32_t n_samples, char mic_type,
                            double* out, int64_t cap);

/* ---- reverberant scene simulation on the device (create_data/create_simulation_data.py) --------
 * The entries below follow the metric entries: plain device pointers, row strides and optional index arrays,
 * stream-ordered on the caller's hipStream_t, no allocation and no host synchronisation inside, ordinary kernel
 * launches only. Every reduction has a fixed order: results are bitwise reproducible and a row's (job's, scene's)
 * result does not depend on the batch around it.
 *
 * One microphone's response as the arguments of the host generator above (create_data/rirgen.cpp:115-131,
 * create_simulation_data.py:258-291): beta holds n_beta = 1 (T60) or 6 values. */
typedef struct SepVadRirDesc {
  double c, fs;
  double mic[3], src[3], room[3];
  double beta[6];
  double orientation[2];
  int32_t n_beta, high_pass, n_dim, order, n_samples, mic_type; /* mic_type: the character code, e.g. 'o' */
} SepVadRirDesc;

/* The same job resolved (create_data/rirgen.cpp:133-199): the six reflection coefficients, the positions and the
 * room in units of c/fs, the lattice bounds n_i = ceil(n_samples / (2 L_i)), the width Tw of the windowed sinc and
 * the high-pass constants hp = {B1, B2, A1, R1}. */
typedef struct SepVadRirJob {
  double beta[6];
  double s[3], r[3], L[3];
  double cTs;
  double angle[2];
  double hp[4];
  int32_t n_samples, n1, n2, n3, Tw, order, high_pass, mic_type;
} SepVadRirJob;

/* Largest lattice of one device job, counted in mirror images: 8 (2 n1 + 1)(2 n2 + 1)(2 n3 + 1). The value is that
 * of a T60 = 1 s response (16 000 samples) of a 3 x 3 x 2.2 m room at 16 kHz, c = 340 m/s: n = (57, 57, 78). Every
 * workgroup of the device generator walks its job's lattice once, so the cap bounds the longest kernel. Tw is
 * capped at SEPVAD_RIR_MAX_TW (fs <= 64 kHz). */
#define SEPVAD_RIR_MAX_IMAGES 16610600
#define SEPVAD_RIR_MAX_TW 512

/* HOST function: resolves n_jobs descriptions into jobs[n_jobs] in host double, with the code the host generator
 * runs for its own prologue (csrc/rir_setup.h). Returns the largest n_samples of the table (>= 0), or SEPVAD_E_ARG
 * (nothing usable written) under the host generator's conditions (c <= 0, fs <= 0, n_beta not 1 or 6, a negative
 * length), for a lattice above SEPVAD_RIR_MAX_IMAGES or Tw above SEPVAD_RIR_MAX_TW, and for n_jobs outside
 * 1..65535. */
int32_t sepvad_rir_jobs_prepare(const SepVadRirDesc* desc, int32_t n_jobs, SepVadRirJob* jobs);

/* HOST function: bytes of device scratch sepvad_rir_generate_device needs for n_jobs rows of ld doubles; negative
 * for n_jobs < 1 or ld < 1. The generator keeps its image lists in LDS, so the answer is currently 0 and a null
 * scratch is accepted; the pair stays in the signature as with the other entries. */
int64_t sepvad_rir_scratch_bytes(int32_t n_jobs, int64_t ld);

/* Replaces the generateRir calls of create_simulation_data.py:258-291 (create_data/rirgen.cpp:200-351) for a batch:
 * jobs [n_jobs] (DEVICE copy of a prepared table), h [n_jobs][ld] double. Job j writes h[j][0 : n_samples_j] and
 * zeroes the rest of its row (a job longer than ld is cut at ld). One workgroup per (job, 256 output samples) walks
 * the lattice in the reference's loop order, keeps the images that touch its samples in that order, and one thread
 * per sample sums their contributions in list order: the reference's summation order, no atomics. What decides a
 * branch (the distance, its floor, the length, order and clipping tests) is computed in the host's operation order
 * without FMA contraction and has the host's bits; gains, window and sinc use the device's pow / sin / cos
 * (measured against the reference's goldens: DESIGN.md). The optional high-pass is the reference's two-pole
 * recursion in its operation order, one lane per job. A table entry outside the caps above yields a zero row. */
int32_t sepvad_rir_generate_device(const SepVadRirJob* jobs, int32_t n_jobs, double* h, int64_t ld, void* scratch,
                                   int64_t scratch_bytes, void* stream);

/* Replaces np.convolve(wave, h)[:cut_length] (create_simulation_data.py:482-500) for R rows:
 *   y[r][n] = sum_{k=0}^{min(n, K_r - 1)} h[hidx[r]][k] * x[xidx[r]][n - k],  n < L,
 * x float32 [.][x_ld] read as zero at and beyond Nx (widened to double exactly), h double [.][h_ld] with
 * K_r = klen[hidx[r]] (device int32, clamped to 0..K; null: K for every row), y double [R][y_ld]; xidx / hidx
 * nullable (identity). Each output is one fused-multiply-add chain over k ascending in double, whatever the tiling:
 * bitwise reproducible, independent of R and of the other rows. */
int32_t sepvad_fir_convolve(const float* x, int64_t x_ld, int64_t Nx, const double* h, int64_t h_ld, int32_t K,
                            const int32_t* klen, const int32_t* xidx, const int32_t* hidx, int32_t R, int64_t L,
                            double* y, int64_t y_ld, void* stream);

/* Replaces the mixing and normalisation of create_simulation_data.py:558-588 with Noise.get_mixed (:707-713):
 * mixed = sum_s rev[b][s] over rev [B][S][L] double (S <= 8, s ascending); with noise [B][L] float32 and snr_db [B]
 * (both null, or both given; a NaN snr_db[b] leaves scene b without noise)
 *   power_mode 0: gain = sqrt(10^(-snr/10) * std(mixed)^2 / std(noise)^2), numpy's population std (the reference);
 *   power_mode 1: gain = sqrt(mean(mixed^2) / (mean(noise^2) * 10^(snr/10))) (synth.make_reverb_mixture);
 * x = mixed + gain * noise, mix = a * (x - min) / (max - min) - b in that operation order, stored as float32 [B][L].
 * (a, b) = (2, 1) in the reference, (1.8, 0.9) in only_inference.py:81. stats [B][4] double (nullable) receives
 * {gain (0 without noise), min, max, a / (max - min)}. One workgroup per scene, double throughout. */
int32_t sepvad_scene_mix(const double* rev, int32_t B, int32_t S, int64_t L, const float* noise,
                         const double* snr_db, int32_t power_mode, double a, double b, float* mix, double* stats,
                         void* stream);

/* Targets of the same scenes from dry [B][S][L] double, out float32 [B][S][L]. mode 0: each row's own min-max with
 * (a, b) (create_simulation_data.py:605-620); mode 1: stats[b][3] * dry, the mixture's scale without offset
 * (synth.make_reverb_mixture: the targets stay SI-SDR-comparable with the mixture; stats from the entry above). */
int32_t sepvad_scene_targets(const double* dry, int32_t B, int32_t S, int64_t L, int32_t mode, double a, double b,
                             const double* stats, float* out, void* stream);

/* Replaces convert_samples2frames_vad and the edge frames around it (create_data/vad_labels2stft_labels.py:14-23,
 * 47-66): act [R][act_ld] uint8 sample-level activity with values 0..8 (larger values are not counted), L a multiple
 * of 512; out [R][T] float32, T = 2 L / 512 + 1 (the model's 1 + N / 256, so the result feeds the VAD accuracy
 * entry). Frame j = 1..T-2 is the most frequent value of act[256 (j-1) : 256 (j-1) + 512], the lowest value
 * winning ties (argmax of bincount). Edge frames 0 and T-1 look at the first / last 256 samples: edge_mode 0 counts
 * 256 zeros with them (the per-speaker rule, :52-56), edge_mode 1 the samples alone (the sum-track rule, :62-66). */
int32_t sepvad_vad_frame_labels(const uint8_t* act, int64_t act_ld, int32_t R, int64_t L, int32_t edge_mode,
                                float* out, void* stream);

/* ---- input preprocessing of the reference CLI (only_inference.py:68-83) ---------------------
 * Windowed-sinc resampling filter of torchaudio.transforms.Resample(orig_freq, new_freq) with its
 * defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), host-side, double precision
 * rounded to float: taps [phases][ntaps] into `taps` (capacity `cap` floats); info receives
 * {phases, ntaps, stride, width}. Returns SEPVAD_E_ARG if cap is too small. */
int32_t sepvad_resample_filter(int32_t orig_freq, int32_t new_freq, float* taps, int32_t cap, int32_t* info);

/* Polyphase FIR on the device: y [ylen] = resample(x [n]) with ylen = ceil(new * n / orig) (reduced
 * by the gcd) and taps (device) from sepvad_resample_filter. */
int32_t sepvad_resample(const float* x, int64_t n, const float* taps, const int32_t* info, float* y, int64_t ylen,
                        void* stream);

/* y = 1.8 * (x - min x) / (max x - min x) - 0.9 over n samples (only_inference.py:81), fp32 in the
 * reference's numpy operation order (bit-exact). scratch: SEPVAD_NORM_SCRATCH_BYTES device bytes. */
#define SEPVAD_NORM_SCRATCH_BYTES 8192
int32_t sepvad_normalize(const float* x, int64_t n, float* y, void* scratch, void* stream);

/* Seconds of the last forward's dominant-kernel launches measured with HIP events
 * (enabled by sepvad_set_timing(h, 1)); see bench.py. */
int32_t sepvad_set_timing(sepvad_handle h, int32_t on);
int32_t sepvad_timing(sepvad_handle h, double* gemm_ms, int32_t* gemm_launches, double* total_ms);

void sepvad_destroy(sepvad_handle h);
const char* sepvad_last_error(void);
int32_t sepvad_abi_version(void);
/* Source hash of this build: the first 16 hex digits of sha256 over include/sepvad.h and the library's sources
 * (sep-tfanet-vad_amd/buildid.py, computed at build time). A static string; tests compare it with the hash of the
 * tree they run in. No reference equivalent (build provenance). */
const char* sepvad_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* SEPVAD_H */
