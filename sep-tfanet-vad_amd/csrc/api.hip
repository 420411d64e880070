// C ABI of libsepvad.so (include/sepvad.h): argument validation, then a call into pack.h (weight folding and
// packing at create time), context.hip (handle lifetime, per-stream contexts), forward.hip (the launch sequence of one
// SeparationModel.forward) or a kernel's launcher (the stateless entries).
#include "build/build_id.h"  // SEPVAD_BUILD_ID (Makefile: buildid.py)

#include <numeric>

#include "handle.h"
#include "stoi_design.h"

using namespace sepvad;

namespace {
thread_local std::string g_err;

PitArgs pit_args(const float* est, int64_t est_ld, const float* ref, int64_t ref_ld, int32_t B, int64_t L, int nblk,
                 void* scratch, int64_t* perm_out, float* loss_out, float* pw_out) {
  PitArgs a{};
  a.B = B; a.L = L; a.est = est; a.est_ld = est_ld; a.ref = ref; a.ref_ld = ref_ld;
  a.nblk = nblk;
  a.partial = (double*)scratch;
  a.perm_out = (long long*)perm_out; a.loss_out = loss_out; a.pw_out = pw_out;
  return a;
}
int pit_batch_blocks(int32_t B, int64_t L) {  // the blocks of a PIT-L1 over the whole batch
  return (int)std::min<long long>(PIT_MAX_BLOCKS, std::max<long long>(1, ((long long)B * L + 8191) / 8192));
}

SiSdrArgs sisdr_args(const float* P, int64_t p_ld, const float* Tg, int64_t t_ld, int64_t N, int32_t R,
                     const int32_t* pidx, const int32_t* tidx, int32_t zero_mean, float* out) {
  SiSdrArgs a{};
  a.P = P; a.p_ld = p_ld; a.Tg = Tg; a.t_ld = t_ld; a.N = N; a.R = R; a.pidx = pidx; a.tidx = tidx;
  a.zero_mean = zero_mean; a.out = out;
  return a;
}
// sepvad_si_sdr and sepvad_snr: one argument list and one check, `launch` the entry's kernel launcher
int32_t pair_metric(const char* entry, hipError_t (*launch)(const SiSdrArgs&, hipStream_t), const float* P, int64_t p_ld,
                    const float* Tg, int64_t t_ld, int64_t N, int32_t R, const int32_t* pidx, const int32_t* tidx,
                    int32_t zero_mean, float* out, void* stream) {
  if (!P || !Tg || !out || N < 1 || R < 1 || p_ld < N || t_ld < N)
    return fail(SEPVAD_E_ARG, std::string(entry) + ": bad arguments");
  HIPRET(launch(sisdr_args(P, p_ld, Tg, t_ld, N, R, pidx, tidx, zero_mean, out), (hipStream_t)stream));
}

// The scratch refusals of every entry that takes scratch, in their order: `e` starts the message ("<entry>: "), `need`
// is the answer of the size query `query` for the call's shapes, `align` what the entry asks for (1: nothing).
int32_t scratch_check(const std::string& e, const void* scratch, int64_t have, int64_t need, int align, const char* query) {
  if (!scratch || have < need) return fail(SEPVAD_E_ARG, e + "scratch too small (" + query + ")");
  if ((reinterpret_cast<uintptr_t>(scratch) & (uintptr_t)(align - 1)) != 0)
    return fail(SEPVAD_E_ARG, e + "scratch must be " + std::to_string(align) + "-byte aligned");
  return SEPVAD_OK;
}
// ... for the arrays `list` names (scratch_plan.h), which it then binds in `scratch`
template <class L>
int32_t scratch_bind(const std::string& e, void* scratch, int64_t have, int align, const char* query, L&& list) {
  if (const int32_t rc = scratch_check(e, scratch, have, plan_bytes(list, align), align, query)) return rc;
  ScratchPlan p(scratch, align);
  list(p);
  return SEPVAD_OK;
}

// The eval family: sepvad_eval_separation, sepvad_criterion_coef and, for what it shares, sepvad_stream_eval. Their
// scratch is plain doubles, one array behind the other: plans with alignment 8.
constexpr size_t EV_ALIGN = sizeof(double);
// The criterion fields of EvalSepArgs / CritCoefArgs
template <typename Args>
void set_criterion(Args& a, int32_t B, int64_t N, int32_t sdr_type, int32_t zero_mean, int32_t take_log, double eps) {
  a.B = B; a.N = N; a.nchunk = (int)((N + EV_CHUNK - 1) / EV_CHUNK);
  a.sdr_type = sdr_type; a.zero_mean = zero_mean != 0; a.take_log = take_log != 0; a.eps = eps;
}
// The evaluation's scratch, each array once (a.B and a.nchunk are set)
void eval_scratch(EvalSepArgs& a, ScratchPlan& p) {
  p.take(a.partial, (size_t)a.B * a.nchunk * EV_MOM); p.take(a.rowvals, (size_t)a.B * EV_ROWVALS);
}
// The checks sepvad_eval_separation and sepvad_criterion_coef share, in their order (min_ld: the smallest row stride)
int32_t eval_check(const char* entry, int32_t B, int64_t N, int64_t min_ld, int32_t sdr_type, const void* scratch,
                   int64_t scratch_bytes) {
  const std::string e = std::string(entry) + ": ";
  if (B < 1 || B > 65535 || N < 1 || N > (1LL << 40)) return fail(SEPVAD_E_ARG, e + "need 1 <= B <= 65535, 1 <= N <= 2^40");
  if (min_ld < N) return fail(SEPVAD_E_ARG, e + "row strides must be >= N");
  if (sdr_type < SEPVAD_SDR_SISDR || sdr_type > SEPVAD_SDR_SNR) return fail(SEPVAD_E_ARG, e + "unknown sdr_type");
  return scratch_check(e, scratch, scratch_bytes, sepvad_eval_scratch_bytes(B, N), EV_ALIGN, "sepvad_eval_scratch_bytes");
}
}  // namespace

void sepvad::set_error(const std::string& msg) { g_err = msg; }
int sepvad::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" {
const char* sepvad_last_error(void) { return g_err.c_str(); }
int32_t sepvad_abi_version(void) { return SEPVAD_ABI_VERSION; }
const char* sepvad_build_id(void) { return SEPVAD_BUILD_ID; }

sepvad_handle sepvad_create(const SepVadConfig* cfg, const float* const* tensors, const char* const* names,
                            const int64_t* numels, int32_t n, int32_t device) {
  if (!cfg || !tensors || !names || !numels) { g_err = "null argument"; return nullptr; }
  const SepVadConfig& c = *cfg;
  if (c.n_fft != NFFT || c.bn_dim != CH || c.h_dim != HID || c.num_spk != 2 || c.layer < 1 || c.stack < 1 ||
      c.precision < SEPVAD_PREC_FP32 || c.precision > SEPVAD_PREC_BF16) {
    g_err = "unsupported configuration (native path: n_fft=512, BN_dim=256, H_dim=512, num_spk=2)";
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { g_err = "invalid device"; return nullptr; }
  DeviceGuard dg(device);
  TensorMap tm;
  for (int i = 0; i < n; ++i) tm.m[names[i]] = {tensors[i], numels[i]};
  Packed pm;
  if (!pack_model(c, tm, pm, g_err)) return nullptr;
  return model_create(c, pm, device);
}

void sepvad_destroy(sepvad_handle h) { model_destroy(h); }

int32_t sepvad_reserve(sepvad_handle h, int32_t B, int32_t N) {
  if (!h || B < 1 || N <= HOP) return fail(SEPVAD_E_ARG, "sepvad_reserve: bad arguments");
  DeviceGuard dg(h->device);
  std::lock_guard<std::mutex> lk(h->mu);
  h->res_B = std::max(h->res_B, (int)B);
  h->res_N = std::max(h->res_N, (int)N);
  StreamCtx* c0 = nullptr;
  int rc = get_ctx(h, nullptr, &c0);  // the default stream's context exists from here on
  for (size_t i = 0; rc == SEPVAD_OK && i < h->ctx.size(); ++i) rc = ws_reserve(h->ctx[i].get(), h->res_B, h->res_N);
  return rc;
}

int32_t sepvad_set_precision(sepvad_handle h, int32_t precision) {
  if (!h) return fail(SEPVAD_E_ARG, "null handle");
  if (precision < SEPVAD_PREC_FP32 || precision > SEPVAD_PREC_BF16) return fail(SEPVAD_E_ARG, "unknown precision");
  h->prec = precision;
  return SEPVAD_OK;
}

int32_t sepvad_set_weight_lo(sepvad_handle h, int32_t mode) {
  if (!h) return fail(SEPVAD_E_ARG, "null handle");
  if (mode != SEPVAD_WLO_E4M3 && mode != SEPVAD_WLO_F16 && mode != SEPVAD_WLO_I8)
    return fail(SEPVAD_E_ARG, "unknown weight lo-plane format");
  h->lo8 = mode == SEPVAD_WLO_E4M3 ? 1 : (mode == SEPVAD_WLO_I8 ? 2 : 0);
  return SEPVAD_OK;
}

int32_t sepvad_e4m3_encode(const float* in, uint8_t* out, int64_t n) {
  if ((!in || !out) && n > 0) return fail(SEPVAD_E_ARG, "sepvad_e4m3_encode: null buffer");
  for (int64_t i = 0; i < n; ++i) out[i] = e4m3_rn(in[i]);
  return SEPVAD_OK;
}

int32_t sepvad_set_timing(sepvad_handle h, int32_t on) {
  if (!h) return fail(SEPVAD_E_ARG, "null handle");
  h->timing = on != 0;
  return SEPVAD_OK;
}

int32_t sepvad_timing(sepvad_handle h, double* gemm_ms, int32_t* gemm_launches, double* total_ms) {
  if (!h) return fail(SEPVAD_E_ARG, "null handle");
  if (gemm_ms) { gemm_ms[0] = h->gemm_ms; gemm_ms[1] = h->g2_ms; }
  if (gemm_launches) { gemm_launches[0] = h->gemm_launches; gemm_launches[1] = h->g2_launches; }
  if (total_ms) *total_ms = h->total_ms;
  return SEPVAD_OK;
}

int32_t sepvad_forward(sepvad_handle h, const float* x, int32_t B, int32_t N, const SepVadOutputs* out,
                       const SepVadInferKw* kw, void* stream) {
  return sepvad_forward_strided(h, x, N, B, N, out, kw, stream);
}

int32_t sepvad_forward_strided(sepvad_handle h, const float* x, int64_t ldx, int32_t B, int32_t N,
                               const SepVadOutputs* out, const SepVadInferKw* kw, void* stream) {
  if (!h || !x || !out || !out->sep) return fail(SEPVAD_E_ARG, "sepvad_forward: null argument");
  if (B < 1) return fail(SEPVAD_E_SHAPE, "sepvad_forward: B must be >= 1");
  if (N <= HOP) return fail(SEPVAD_E_SHAPE, "sepvad_forward: N must exceed 256 (reflect padding of the STFT)");
  if (ldx < N || ldx > INT32_MAX) return fail(SEPVAD_E_SHAPE, "sepvad_forward: row stride must be >= N");
  TraceRange trace("sepvad_forward");
  DeviceGuard dg(h->device);
  std::lock_guard<std::mutex> lk(h->mu);
  return forward_impl(h, x, (int)ldx, B, N, out, kw, (hipStream_t)stream);
}

int32_t sepvad_forward_windows(sepvad_handle h, const float* x, int64_t ld_stream, int32_t n_streams, int32_t n_win,
                               int64_t hop, int32_t N, const SepVadOutputs* out, const SepVadInferKw* kw,
                               void* stream) {
  if (!h || !x || !out || !out->sep) return fail(SEPVAD_E_ARG, "sepvad_forward_windows: null argument");
  if (n_streams < 1 || n_win < 1 || hop < 0 || (long long)n_streams * n_win > INT32_MAX)
    return fail(SEPVAD_E_SHAPE, "sepvad_forward_windows: bad window counts");
  if (N <= HOP) return fail(SEPVAD_E_SHAPE, "sepvad_forward_windows: N must exceed 256");
  if ((long long)(n_win - 1) * hop + N > ld_stream || ld_stream > INT32_MAX)
    return fail(SEPVAD_E_SHAPE, "sepvad_forward_windows: windows exceed the stream rows");
  DeviceGuard dg(h->device);
  std::lock_guard<std::mutex> lk(h->mu);
  return forward_impl(h, x, (int)ld_stream, n_streams * n_win, N, out, kw, (hipStream_t)stream, n_streams, hop);
}

int32_t sepvad_set_split(sepvad_handle h, int32_t nsplit) {
  if (!h || nsplit < 1 || nsplit > MAX_SPLIT) return fail(SEPVAD_E_ARG, "sepvad_set_split: 1 <= n <= 4");
  h->split = nsplit;
  return SEPVAD_OK;
}
int32_t sepvad_set_fused(sepvad_handle h, int32_t on) {
  if (!h) return fail(SEPVAD_E_ARG, "null handle");
  h->fused = on != 0;
  return SEPVAD_OK;
}

int32_t sepvad_set_tcn_dump(sepvad_handle h, float* dump) {
  if (!h) return fail(SEPVAD_E_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  h->tdump = dump;
  return SEPVAD_OK;
}

int32_t sepvad_fused_status(sepvad_handle h, int32_t* used) {
  if (!h) return fail(SEPVAD_E_ARG, "null handle");
  DeviceGuard dg(h->device);
  std::lock_guard<std::mutex> lk(h->mu);
  if (used) *used = h->last_fused ? h->last_nsl : 0;
  HIPCHK(hipDeviceSynchronize());
  const Knobs kn = read_knobs();
  int rc = SEPVAD_OK;
  for (auto& c : h->ctx) {
    const int r = check_giveup(c.get(), kn);
    if (r && rc == SEPVAD_OK) rc = r;
  }
  return rc;
}

int32_t sepvad_tcn_clock(sepvad_handle h, uint64_t* out, int32_t max_records, int32_t* n) {
  if (!h || !n || (max_records > 0 && !out)) return fail(SEPVAD_E_ARG, "sepvad_tcn_clock: null argument");
  DeviceGuard dg(h->device);
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipDeviceSynchronize());
  const long long have = std::min<long long>(h->tclk_n, TCLK_RECS);
  const int k = (int)std::min<long long>(have, std::max(0, max_records));
  *n = (int)have;
  if (k > 0) {  // the last k records, oldest first
    std::vector<unsigned long long> all((size_t)TCLK_RECS * 8);
    HIPCHK(hipMemcpy(all.data(), h->tclk, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < k; ++i) {
      const long long r = (h->tclk_n - k + i) % TCLK_RECS;
      for (int j = 0; j < 8; ++j) out[(size_t)i * 8 + j] = all[(size_t)r * 8 + j];
    }
  }
  return SEPVAD_OK;
}

int32_t sepvad_last_forward(sepvad_handle h, void* stream, int64_t* seq, int32_t* B, int32_t* N) {
  if (!h || !seq || !B || !N) return fail(SEPVAD_E_ARG, "sepvad_last_forward: null argument");
  std::lock_guard<std::mutex> lk(h->mu);
  const StreamCtx* c = find_ctx(h, stream);
  if (!c) return fail(SEPVAD_E_ARG, "sepvad_last_forward: no forward has run on this stream");
  *seq = c->seq; *B = c->last_B; *N = c->last_N;
  return SEPVAD_OK;
}

int32_t sepvad_release_stream(sepvad_handle h, void* stream) {
  if (!h) return fail(SEPVAD_E_ARG, "sepvad_release_stream: null handle");
  DeviceGuard dg(h->device);
  std::lock_guard<std::mutex> lk(h->mu);
  return release_ctx(h, stream);
}

int32_t sepvad_side_outputs_of(sepvad_handle h, const SepVadOutputs* out, void* stream, int64_t seq, int32_t Bx,
                               int32_t Nx) {
  if (!h || !out) return fail(SEPVAD_E_ARG, "sepvad_side_outputs_of: null argument");
  DeviceGuard dg(h->device);
  std::lock_guard<std::mutex> lk(h->mu);
  const StreamCtx* cx = find_ctx(h, stream);
  // seq is handle-wide (never reused by a context that was evicted and recreated)
  if (!cx || cx->seq != seq || cx->last_B != Bx || cx->last_N != Nx)
    return fail(SEPVAD_E_ARG, "side outputs: a later forward on the same stream has replaced the workspace of the "
                              "forward that produced them (read them before the next forward on that stream)");
  return side_outputs_locked(h, out, stream);
}

int32_t sepvad_side_outputs(sepvad_handle h, const SepVadOutputs* out, void* stream) {
  if (!h || !out) return fail(SEPVAD_E_ARG, "sepvad_side_outputs: null argument");
  DeviceGuard dg(h->device);
  std::lock_guard<std::mutex> lk(h->mu);
  return side_outputs_locked(h, out, stream);
}

int32_t sepvad_stft_gate_test(sepvad_handle h, const float* x, int32_t B, int32_t N, void* X_fm, float* db_fm,
                              void* stream) {
  if (!h || !x || !X_fm || !db_fm || B < 1 || N <= HOP) return fail(SEPVAD_E_ARG, "sepvad_stft_gate_test: bad arguments");
  DeviceGuard dg(h->device);
  std::lock_guard<std::mutex> lk(h->mu);
  StreamCtx* cx = nullptr;
  int rc = get_ctx(h, stream, &cx);
  if (!rc) rc = ws_reserve(cx, B, N);  // S0 and the TCN.LN records land in this stream's workspace
  if (rc) return rc;
  StftArgs sa = stft_gate_args(h, ws_view(cx->ws, 0, round_up(1 + N / HOP, TILE)), x, N, B, N);
  sa.X = (float2*)X_fm; sa.specdb = db_fm; sa.db_out = 1;
  HIPRET(launch_stft_gate(sa, (hipStream_t)stream));
}

int32_t sepvad_istft_pair_test(sepvad_handle h, const void* X_fm, const float* masks_fm, int32_t B, int32_t N, float* y,
                               void* est, void* stream) {
  if (!h || !X_fm || !masks_fm || !y || B < 1 || N <= HOP) return fail(SEPVAD_E_ARG, "sepvad_istft_pair_test: bad arguments");
  DeviceGuard dg(h->device);
  IstftArgs is = istft_pair_args(h, (const float2*)X_fm, masks_fm, B, N);
  is.est_out = (float2*)est; is.y = y;
  HIPRET(launch_istft_pair(is, (hipStream_t)stream));
}

int32_t sepvad_pit_l1(const float* est, int64_t est_ld, const float* ref, int64_t ref_ld, int32_t B, int64_t L,
                      void* scratch, int64_t* perm_out, float* loss_out, float* pw_out, void* stream) {
  if (!est || !ref || !scratch || B < 1 || L < 1 || est_ld < L || ref_ld < L)
    return fail(SEPVAD_E_ARG, "sepvad_pit_l1: bad arguments");
  static_assert((PIT_MAX_BLOCKS + 1) * 4 * sizeof(double) <= SEPVAD_PIT_SCRATCH_BYTES, "scratch size");
  HIPRET(launch_pit_l1(pit_args(est, est_ld, ref, ref_ld, B, L, pit_batch_blocks(B, L), scratch, perm_out, loss_out, pw_out),
                       (hipStream_t)stream));
}

int32_t sepvad_pit_l1_sums(const float* est, int64_t est_ld, const float* ref, int64_t ref_ld, int32_t B, int64_t L,
                           void* scratch, double* sums, void* stream) {
  if (!est || !ref || !scratch || !sums || B < 1 || L < 1 || est_ld < L || ref_ld < L)
    return fail(SEPVAD_E_ARG, "sepvad_pit_l1_sums: bad arguments");
  HIPRET(launch_pit_l1_sums(pit_args(est, est_ld, ref, ref_ld, B, L, pit_batch_blocks(B, L), scratch, nullptr, nullptr, nullptr),
                            sums, (hipStream_t)stream));
}

int32_t sepvad_pit_l1_choose(const double* sums, double count, int32_t B, int64_t* perm_out, float* loss_out,
                             float* pw_out, void* stream) {
  if (!sums || B < 1 || !(count > 0.0)) return fail(SEPVAD_E_ARG, "sepvad_pit_l1_choose: bad arguments");
  HIPRET(launch_pit_l1_choose(pit_args(nullptr, 0, nullptr, 0, B, 0, 0, nullptr, perm_out, loss_out, pw_out), sums, count,
                              (hipStream_t)stream));
}

int32_t sepvad_stream_append(const float* src, int64_t src_ld, int64_t s0, int32_t B, int64_t H,
                             const int64_t* perm, float* dst, int64_t dst_ld, int64_t d0, void* stream) {
  if (!src || !dst || B < 1 || H < 1 || s0 < 0 || d0 < 0 || s0 + H > src_ld || d0 + H > dst_ld)
    return fail(SEPVAD_E_ARG, "sepvad_stream_append: bad arguments");
  AppendArgs a{};
  a.B = B; a.H = H; a.src = src; a.src_ld = src_ld; a.s0 = s0; a.perm = (const long long*)perm;
  a.dst = dst; a.dst_ld = dst_ld; a.d0 = d0;
  HIPRET(launch_stream_append(a, (hipStream_t)stream));
}

int32_t sepvad_ring_push(const float* chunk, int64_t chunk_ld, int32_t rows, int64_t n, float* ring, int64_t R,
                         int64_t pos, void* stream) {
  if (!chunk || !ring) return fail(SEPVAD_E_ARG, "sepvad_ring_push: null pointer");
  if (rows < 1 || R < 1) return fail(SEPVAD_E_ARG, "sepvad_ring_push: rows and R must be >= 1");
  if (n < 1 || n > R) return fail(SEPVAD_E_ARG, "sepvad_ring_push: need 1 <= n <= R");
  if (pos < 0 || pos >= R) return fail(SEPVAD_E_ARG, "sepvad_ring_push: pos must be in [0, R)");
  if (chunk_ld < n) return fail(SEPVAD_E_ARG, "sepvad_ring_push: chunk_ld must be >= n");
  RingPushArgs a{};
  a.rows = rows; a.n = n; a.R = R; a.pos = pos; a.chunk = chunk; a.chunk_ld = chunk_ld; a.ring = ring;
  HIPRET(launch_ring_push(a, (hipStream_t)stream));
}

int64_t sepvad_pit_l1_rows_scratch_bytes(int32_t B, int64_t L) {
  if (B < 1 || B > 65535 || L < 1) return fail(SEPVAD_E_ARG, "sepvad_pit_l1_rows_scratch_bytes: need 1 <= B <= 65535, L >= 1");
  return (int64_t)B * pit_row_blocks(L) * 4 * (int64_t)sizeof(double);
}

int32_t sepvad_pit_l1_rows(const float* est, int64_t est_ld, const float* ref, int64_t ref_ld, int32_t B, int64_t L,
                           void* scratch, int64_t scratch_bytes, int64_t* perm_out, float* loss_out, float* pw_out,
                           void* stream) {
  if (!est || !ref || !scratch) return fail(SEPVAD_E_ARG, "sepvad_pit_l1_rows: null pointer");
  if (B < 1 || B > 65535 || L < 1 || est_ld < L || ref_ld < L)
    return fail(SEPVAD_E_ARG, "sepvad_pit_l1_rows: need 1 <= B <= 65535, L >= 1 and row strides >= L");
  if (const int32_t rc = scratch_check("sepvad_pit_l1_rows: ", scratch, scratch_bytes, sepvad_pit_l1_rows_scratch_bytes(B, L), 1,
                                       "sepvad_pit_l1_rows_scratch_bytes")) return rc;
  HIPRET(launch_pit_l1_rows(pit_args(est, est_ld, ref, ref_ld, B, L, pit_row_blocks(L), scratch, perm_out, loss_out, pw_out),
                            (hipStream_t)stream));
}

int32_t sepvad_live_stitch(const float* win, int64_t win_ld, int64_t N, int32_t B, int64_t H, const int64_t* perm,
                           float* out, int64_t out_ld, int64_t d0, float* tail, int64_t Rt, int64_t tpos,
                           const float* vad, int32_t T, int32_t nf, float* vad_out, int64_t vad_ld, int64_t v0,
                           void* stream) {
  if (!win || !out || !tail) return fail(SEPVAD_E_ARG, "sepvad_live_stitch: null pointer");
  if (B < 1 || B > INT32_MAX / 2 || H < 1 || H > N || N > win_ld)
    return fail(SEPVAD_E_ARG, "sepvad_live_stitch: need B >= 1 and 1 <= H <= N <= win_ld");
  if (H > Rt) return fail(SEPVAD_E_ARG, "sepvad_live_stitch: H must be <= Rt");
  if (tpos < 0 || tpos >= Rt) return fail(SEPVAD_E_ARG, "sepvad_live_stitch: tpos must be in [0, Rt)");
  if (d0 < 0 || d0 + H > out_ld) return fail(SEPVAD_E_ARG, "sepvad_live_stitch: d0 + H exceeds the output row");
  if (vad) {
    if (!vad_out) return fail(SEPVAD_E_ARG, "sepvad_live_stitch: vad without vad_out");
    if (nf < 0 || nf > T) return fail(SEPVAD_E_ARG, "sepvad_live_stitch: nf must be in [0, T]");
    if (v0 < 0 || v0 + nf > vad_ld) return fail(SEPVAD_E_ARG, "sepvad_live_stitch: v0 + nf exceeds the VAD row");
  }
  LiveStitchArgs a{};
  a.B = B; a.H = H; a.win = win; a.win_ld = win_ld; a.s0 = N - H; a.perm = (const long long*)perm;
  a.out = out; a.out_ld = out_ld; a.d0 = d0; a.tail = tail; a.Rt = Rt; a.tpos = tpos;
  if (vad && nf > 0) {
    a.vad = vad; a.vad_in_ld = T; a.f0 = T - nf; a.nf = nf; a.vad_out = vad_out; a.vad_ld = vad_ld; a.v0 = v0;
  }
  HIPRET(launch_live_stitch(a, (hipStream_t)stream));
}

int32_t sepvad_resample_filter(int32_t orig_freq, int32_t new_freq, float* taps, int32_t cap, int32_t* info) {
  if (orig_freq < 1 || new_freq < 1 || !info) return fail(SEPVAD_E_ARG, "sepvad_resample_filter: bad arguments");
  // torchaudio.functional.functional._get_sinc_resample_kernel, sinc_interp_hann, width 6, rolloff 0.99
  const int g = std::gcd(orig_freq, new_freq);
  const int o = orig_freq / g, nw = new_freq / g;
  const double lpw = 6.0, base = std::min(o, nw) * 0.99;
  const int width = (int)std::ceil(lpw * o / base);
  const int ntaps = 2 * width + o;
  info[0] = nw; info[1] = ntaps; info[2] = o; info[3] = width;
  if ((long long)nw * ntaps > (1 << 22)) return fail(SEPVAD_E_ARG, "sepvad_resample_filter: ratio too large");
  if (!taps) return SEPVAD_OK;  // size query
  if (cap < nw * ntaps) return fail(SEPVAD_E_ARG, "sepvad_resample_filter: taps capacity too small");
  for (int j = 0; j < nw; ++j) {
    for (int i = 0; i < ntaps; ++i) {
      double t = -(double)j / nw + (double)(i - width) / o;
      t *= base;
      t = std::min(lpw, std::max(-lpw, t));
      const double c = std::cos(t * M_PI / lpw / 2.0);
      const double win = c * c;
      t *= M_PI;
      const double k = (t == 0.0) ? 1.0 : std::sin(t) / t;
      taps[j * ntaps + i] = (float)(k * win * (base / o));
    }
  }
  return SEPVAD_OK;
}

int32_t sepvad_resample(const float* x, int64_t n, const float* taps, const int32_t* info, float* y, int64_t ylen,
                        void* stream) {
  if (!x || !taps || !info || !y || n < 1 || ylen < 1) return fail(SEPVAD_E_ARG, "sepvad_resample: bad arguments");
  ResampleArgs a{};
  a.x = x; a.n = n; a.taps = taps; a.phases = info[0]; a.ntaps = info[1]; a.stride = info[2]; a.width = info[3];
  a.y = y; a.ylen = ylen;
  const long long full = (long long)std::ceil((double)a.phases * (double)n / (double)a.stride);
  if (ylen > full) return fail(SEPVAD_E_ARG, "sepvad_resample: ylen exceeds ceil(new * n / orig)");
  HIPRET(launch_resample(a, (hipStream_t)stream));
}

int32_t sepvad_si_sdr(const float* P, int64_t p_ld, const float* Tg, int64_t t_ld, int64_t N, int32_t R,
                      const int32_t* pidx, const int32_t* tidx, int32_t zero_mean, float* out, void* stream) {
  return pair_metric("sepvad_si_sdr", launch_si_sdr, P, p_ld, Tg, t_ld, N, R, pidx, tidx, zero_mean, out, stream);
}

int32_t sepvad_snr(const float* P, int64_t p_ld, const float* Tg, int64_t t_ld, int64_t N, int32_t R,
                   const int32_t* pidx, const int32_t* tidx, int32_t zero_mean, float* out, void* stream) {
  return pair_metric("sepvad_snr", launch_snr, P, p_ld, Tg, t_ld, N, R, pidx, tidx, zero_mean, out, stream);
}

int32_t sepvad_stoi_filter(int32_t fs_sig, float* taps, int32_t cap, int32_t* info) {
  StoiDesign d;
  if (!info || !stoi_design(fs_sig, d)) return fail(SEPVAD_E_ARG, "sepvad_stoi_filter: fs_sig must be 8000, 10000 or 16000");
  const int ntaps = (int)d.w.size();
  info[0] = d.up; info[1] = d.down; info[2] = ntaps; info[3] = STOI_BANDS;
  for (int b = 0; b < STOI_BANDS; ++b) {
    info[4 + 2 * b] = d.lo[b];
    info[5 + 2 * b] = d.hi[b];
  }
  if (!taps) return SEPVAD_OK;  // size query
  if (cap < ntaps) return fail(SEPVAD_E_ARG, "sepvad_stoi_filter: taps capacity too small");
  for (int i = 0; i < ntaps; ++i) taps[i] = (float)d.w[i];
  return SEPVAD_OK;
}

// (R, N, fs_sig) that sepvad_stoi accepts: at least one frame after resampling, grid and index ranges
static bool stoi_shape_ok(int32_t R, int64_t N, int up, int down) {
  if (R < 1 || R > 65535 || N < 1 || N > (1LL << 31)) return false;
  const long long nF = stoi_num_frames(stoi_resampled_len(N, up, down));
  return nF >= 1 && (long long)R * 2 * STOI_BANDS * nF < (1LL << 40);
}

static_assert(STOI_MODE_CLASSIC == SEPVAD_STOI_CLASSIC && STOI_MODE_EXTENDED == SEPVAD_STOI_EXTENDED, "sepvad.h");
static bool stoi_modes_ok(int32_t modes) { return modes >= 1 && modes <= (SEPVAD_STOI_CLASSIC | SEPVAD_STOI_EXTENDED); }

// The shape refusals of the STOI entries and size queries (`e`: whose), from the host design alone; a's shapes
static int32_t stoi_shape(const std::string& e, int32_t R, int64_t N, int32_t fs_sig, int32_t modes, StoiArgs& a) {
  StoiDesign d;
  if (!stoi_design(fs_sig, d)) return fail(SEPVAD_E_ARG, e + "fs_sig must be 8000, 10000 or 16000");
  if (!stoi_modes_ok(modes)) return fail(SEPVAD_E_ARG, e + "modes must be 1, 2 or 3");
  if (!stoi_shape_ok(R, N, d.up, d.down))
    return fail(SEPVAD_E_ARG, e + "need 1 <= R <= 65535 and more than 256 samples at 10 kHz");
  a.N = N; a.R = R; a.up = d.up; a.down = d.down;
  return SEPVAD_OK;
}

static int64_t stoi_bytes(const std::string& e, int32_t R, int64_t N, int32_t fs_sig, int32_t modes) {
  StoiArgs a{};
  if (const int32_t rc = stoi_shape(e, R, N, fs_sig, modes, a)) return rc;
  return plan_bytes([&](ScratchPlan& p) { stoi_scratch(a, modes, p); });
}
int64_t sepvad_stoi_scratch_bytes(int32_t R, int64_t N, int32_t fs_sig) {
  return stoi_bytes("sepvad_stoi_scratch_bytes: ", R, N, fs_sig, SEPVAD_STOI_CLASSIC);
}
int64_t sepvad_stoi_ex_scratch_bytes(int32_t R, int64_t N, int32_t fs_sig, int32_t modes) {
  return stoi_bytes("sepvad_stoi_ex_scratch_bytes: ", R, N, fs_sig, modes);
}

// sepvad_stoi_ex, and sepvad_stoi as its classic mode; `entry` names the caller in the messages. Every refusal comes
// before the first HIP call (stoi_tables uploads the design): the host design gives up / down.
static int32_t stoi_entry(const std::string& entry, const float* X, int64_t x_ld, const float* Y, int64_t y_ld, int64_t N,
                          int32_t R, const int32_t* xidx, const int32_t* yidx, int32_t fs_sig, void* scratch,
                          int64_t scratch_bytes, int32_t modes, double* out_stoi, double* out_estoi, int32_t* frames,
                          void* stream) {
  const std::string e = entry + ": ";
  if (!X || !Y || !scratch || N < 1 || x_ld < N || y_ld < N) return fail(SEPVAD_E_ARG, e + "bad arguments");
  if (!stoi_modes_ok(modes)) return fail(SEPVAD_E_ARG, e + "modes must be 1, 2 or 3");
  if (((modes & SEPVAD_STOI_CLASSIC) && !out_stoi) || ((modes & SEPVAD_STOI_EXTENDED) && !out_estoi))
    return fail(SEPVAD_E_ARG, e + "a requested mode has no output pointer");
  StoiArgs a{};
  if (const int32_t rc = stoi_shape(e, R, N, fs_sig, modes, a)) return rc;
  if (const int32_t rc = scratch_bind(e, scratch, scratch_bytes, 256, (entry + "_scratch_bytes").c_str(),
                                      [&](ScratchPlan& p) { stoi_scratch(a, modes, p); })) return rc;
  HIPCHK(stoi_tables(fs_sig, a));
  a.X = X; a.x_ld = x_ld; a.Y = Y; a.y_ld = y_ld; a.xidx = xidx; a.yidx = yidx;
  a.out = (modes & SEPVAD_STOI_CLASSIC) ? out_stoi : nullptr;
  a.out_ex = (modes & SEPVAD_STOI_EXTENDED) ? out_estoi : nullptr;
  a.frames = frames;
  HIPRET(launch_stoi_ex(a, modes, (hipStream_t)stream));
}

int32_t sepvad_stoi(const float* X, int64_t x_ld, const float* Y, int64_t y_ld, int64_t N, int32_t R,
                    const int32_t* xidx, const int32_t* yidx, int32_t fs_sig, void* scratch, int64_t scratch_bytes,
                    double* out, int32_t* frames, void* stream) {
  if (!out) return fail(SEPVAD_E_ARG, "sepvad_stoi: bad arguments");  // (its word for a missing output)
  return stoi_entry("sepvad_stoi", X, x_ld, Y, y_ld, N, R, xidx, yidx, fs_sig, scratch, scratch_bytes, SEPVAD_STOI_CLASSIC,
                    out, nullptr, frames, stream);
}

int32_t sepvad_stoi_ex(const float* X, int64_t x_ld, const float* Y, int64_t y_ld, int64_t N, int32_t R,
                       const int32_t* xidx, const int32_t* yidx, int32_t fs_sig, void* scratch, int64_t scratch_bytes,
                       int32_t modes, double* out_stoi, double* out_estoi, int32_t* frames, void* stream) {
  return stoi_entry("sepvad_stoi_ex", X, x_ld, Y, y_ld, N, R, xidx, yidx, fs_sig, scratch, scratch_bytes, modes, out_stoi,
                    out_estoi, frames, stream);
}

int32_t sepvad_vad_accuracy(float* preds, const float* targets, int32_t B, int32_t S, int32_t T, int32_t in_place,
                            float* out, void* stream) {
  if (!preds || !targets || !out || B < 1 || S < 1 || S > VACC_MAX_S || T < 1)
    return fail(SEPVAD_E_ARG, "sepvad_vad_accuracy: bad arguments");
  VadAccArgs a{};
  a.preds = preds; a.targets = targets; a.B = B; a.S = S; a.T = T; a.in_place = in_place; a.out = out;
  HIPRET(launch_vad_acc(a, (hipStream_t)stream));
}

int64_t sepvad_eval_scratch_bytes(int32_t B, int64_t N) {
  if (B < 1 || B > 65535 || N < 1 || N > (1LL << 40))
    return fail(SEPVAD_E_ARG, "sepvad_eval_scratch_bytes: need 1 <= B <= 65535, 1 <= N <= 2^40");
  EvalSepArgs a{};
  set_criterion(a, B, N, 0, 0, 0, 0.0);
  return plan_bytes([&](ScratchPlan& p) { eval_scratch(a, p); }, EV_ALIGN);
}

// PITLossWrapper(PairwiseNegSDR(...), "pw_mtx") (model/sdr.py:48-86, model/pit_wrapper.py:100-145,287-312) and the
// separation scores of the same test.py step (test.py:129-152,179-181): csrc/eval.hip
int32_t sepvad_eval_separation(const float* est, int64_t est_ld, const float* tgt, int64_t tgt_ld, const float* mix,
                               int64_t mix_ld, int32_t B, int64_t N, int32_t sdr_type, int32_t zero_mean,
                               int32_t take_log, double eps, void* scratch, int64_t scratch_bytes, float* pw,
                               float* min_loss, int64_t* perm, float* sheet, float* means, void* stream) {
  if (!est || !tgt || !scratch || !pw || !min_loss || !perm || !means)
    return fail(SEPVAD_E_ARG, "sepvad_eval_separation: null pointer");
  if (const int32_t rc = eval_check("sepvad_eval_separation", B, N, std::min({est_ld, tgt_ld, mix ? mix_ld : N}), sdr_type,
                                    scratch, scratch_bytes))
    return rc;
  EvalSepArgs a{};
  a.est = est; a.est_ld = est_ld; a.tgt = tgt; a.tgt_ld = tgt_ld; a.mix = mix; a.mix_ld = mix_ld;
  set_criterion(a, B, N, sdr_type, zero_mean, take_log, eps);
  ScratchPlan p(scratch, EV_ALIGN);
  eval_scratch(a, p);
  a.pw = pw; a.min_loss = min_loss; a.perm = (long long*)perm; a.sheet = sheet; a.means = means;
  HIPRET(launch_eval_separation(a, (hipStream_t)stream));
}

// calc_online's window loop with known targets (model/online_class_known_targets.py:101-123): csrc/stream_eval.hip.
namespace {
// The shape refusals of sepvad_stream_eval and its size query (null: none); fills a's shapes, S, ev.B and ev.nchunk
const char* se_shape(StreamEvalArgs& a, int32_t B, int32_t n, int64_t W, int64_t H, int32_t mode) {
  a.B = B; a.n = n; a.W = W; a.H = H; a.mode = mode;
  if (a.B < 1 || a.B > 65535 || a.n < 1) return "need 1 <= B <= 65535 and n >= 1";
  if (a.H < 1 || a.H > a.W || a.W > INT32_MAX) return "need 1 <= H <= W < 2^31";
  if (a.mode < SEPVAD_SE_NONE || a.mode > SEPVAD_SE_SISDR) return "unknown mode";
  const bool sim = a.mode != SEPVAD_SE_NONE;
  if (sim && 2 * a.H > a.W) return "a similarity mode needs 2 H <= W (the reference's slices stop matching beyond)";
  a.S = sim ? se_segments(a.W, a.H) : 0;
  if (a.S > SE_MAX_SEG) return "a similarity mode takes at most 4096 hops per window";
  a.ev.nchunk = (int)((a.W + EV_CHUNK - 1) / EV_CHUNK);
  const int64_t nu = (int64_t)a.n * a.B;
  if (nu * ((int64_t)a.S + a.ev.nchunk) > INT32_MAX) return "the chunk exceeds 2^31 - 1 workgroups (fewer windows per call)";
  a.ev.B = (int)nu;
  return nullptr;
}
// Its scratch, each array once: with SEPVAD_SE_L1 also the batch sums and launch_pit_l1's scratch; last the evaluation's
void se_scratch(StreamEvalArgs& a, double*& pit0, ScratchPlan& p) {
  const bool l1 = a.mode == SEPVAD_SE_L1;
  p.take(a.seg, (size_t)a.ev.B * a.S * SE_NV); p.take(a.bsum, l1 ? (size_t)a.n * a.S * 4 : 0);
  p.take(pit0, l1 ? SEPVAD_PIT_SCRATCH_BYTES / sizeof(double) : 0);
  eval_scratch(a.ev, p);
}
}  // namespace

int64_t sepvad_stream_eval_scratch_bytes(int32_t B, int32_t n, int64_t W, int64_t H, int32_t mode) {
  StreamEvalArgs a{};
  if (const char* why = se_shape(a, B, n, W, H, mode)) return fail(SEPVAD_E_ARG, std::string("sepvad_stream_eval_scratch_bytes: ") + why);
  double* pit0 = nullptr;
  return plan_bytes([&](ScratchPlan& p) { se_scratch(a, pit0, p); }, EV_ALIGN);
}

int32_t sepvad_stream_eval(const float* sep, int64_t sep_ld, int32_t n, int32_t k0, int32_t K, int32_t B, int64_t W,
                           int64_t H, const float* tgt, int64_t tgt_ld, int32_t mode, int32_t sdr_type,
                           int32_t zero_mean, int32_t take_log, double eps, float* raw, int64_t raw_ld, float* online,
                           int64_t online_ld, int64_t* perm, int64_t* perm_tgt, float* pw_tgt, float* loss_tgt,
                           float* pw_sim, void* scratch, int64_t scratch_bytes, void* stream) {
  const std::string er = "sepvad_stream_eval: ";
  StreamEvalArgs a{};
  if (const char* why = se_shape(a, B, n, W, H, mode)) return fail(SEPVAD_E_ARG, er + why);
  if (!sep || !tgt || !raw || !online || !perm || !pw_tgt || !loss_tgt || !scratch || (mode != SEPVAD_SE_NONE && !perm_tgt))
    return fail(SEPVAD_E_ARG, er + "null pointer");
  if (k0 < 0 || K < 1 || (int64_t)k0 + n > K) return fail(SEPVAD_E_ARG, er + "need 0 <= k0 and k0 + n <= K");
  if (sep_ld < W || tgt_ld < (int64_t)(K - 1) * H + W || raw_ld < (int64_t)K * H || online_ld < (int64_t)K * H)
    return fail(SEPVAD_E_ARG, er + "row strides must cover W (sep), (K - 1) H + W (tgt) and K H (raw, online)");
  if (sdr_type < SEPVAD_SDR_SISDR || sdr_type > SEPVAD_SDR_SNR) return fail(SEPVAD_E_ARG, er + "unknown sdr_type");
  double* pit0 = nullptr;
  if (const int32_t rc = scratch_bind(er, scratch, scratch_bytes, EV_ALIGN, "sepvad_stream_eval_scratch_bytes",
                                      [&](ScratchPlan& p) { se_scratch(a, pit0, p); })) return rc;
  a.k0 = k0; a.K = K; a.sep = sep; a.sep_ld = sep_ld; a.raw = raw; a.raw_ld = raw_ld; a.online = online; a.on_ld = online_ld;
  a.perm = (long long*)perm; a.pw_sim = pw_sim;
  EvalSepArgs& e = a.ev;
  set_criterion(e, n * B, W, sdr_type, zero_mean, take_log, eps);  // (B and nchunk as se_shape left them)
  if (mode == SEPVAD_SE_L1 && k0 == 0)  // window 0's seed comparison: its second-last hop against its own last hop
    a.pit0 = pit_args(sep + (W - 2 * H), sep_ld, raw, raw_ld, B, H, pit_batch_blocks(B, H), pit0, perm, nullptr, pw_sim);
  const int64_t w0 = (int64_t)k0 * B;  // the per-window outputs of this chunk start at window k0
  e.est = sep; e.est_ld = sep_ld; e.tgt = tgt + (int64_t)k0 * H; e.tgt_ld = tgt_ld;
  e.pw = pw_tgt + w0 * 4; e.min_loss = loss_tgt + w0;
  e.perm = (long long*)(mode == SEPVAD_SE_NONE ? perm : perm_tgt) + w0 * 2;
  HIPRET(launch_stream_eval(a, (hipStream_t)stream));
}

// BinaryCrossEntropyLoss_Mean (model/combined_loss.py:120-138), pit_CE_vad's pairwise table (model/metric.py:264),
// the confusion counts of test.py:164,172 and calc_vad (Our_utils/utils_test.py:67-73): csrc/eval.hip
int32_t sepvad_eval_vad(const float* vad, float* labels, int32_t fix_labels, const int64_t* perm, const float* masks,
                        int32_t B, int32_t T, float* bce_rows, float* bce_mean, float* pw_ce, int32_t* conf,
                        int64_t* simple, int32_t* conf_simple, void* stream) {
  if (B < 1 || B > 65535 || T < 1) return fail(SEPVAD_E_ARG, "sepvad_eval_vad: need 1 <= B <= 65535, T >= 1");
  const bool masks_only = !vad && !labels && masks && simple;
  if (!masks_only && (!vad || !labels || !bce_rows || !bce_mean || !pw_ce || !conf))
    return fail(SEPVAD_E_ARG, "sepvad_eval_vad: null pointer");
  if (masks && !simple) return fail(SEPVAD_E_ARG, "sepvad_eval_vad: masks without simple");
  EvalVadArgs a{};
  a.vad = vad; a.labels = labels; a.fix_labels = fix_labels != 0; a.perm = (const long long*)perm; a.masks = masks;
  a.B = B; a.T = T; a.bce_rows = bce_rows; a.bce_mean = bce_mean; a.pw_ce = pw_ce; a.conf = conf;
  a.simple = masks ? (long long*)simple : nullptr;
  a.conf_simple = masks && !masks_only ? conf_simple : nullptr;
  HIPRET(launch_eval_vad(a, (hipStream_t)stream));
}

// the backward of the training criterion (trainer/trainer.py:57-63 over model/sdr.py:48-86 and
// model/combined_loss.py:93-138): csrc/criterion.hip
int32_t sepvad_criterion_coef(const float* est, int64_t est_ld, const float* tgt, int64_t tgt_ld, int32_t B, int64_t N,
                              int32_t sdr_type, int32_t zero_mean, int32_t take_log, double eps, const void* scratch,
                              int64_t scratch_bytes, const int64_t* perm, double* coef, void* stream) {
  if (!est || !tgt || !scratch || !perm || !coef) return fail(SEPVAD_E_ARG, "sepvad_criterion_coef: null pointer");
  if (const int32_t rc = eval_check("sepvad_criterion_coef", B, N, std::min(est_ld, tgt_ld), sdr_type, scratch, scratch_bytes))
    return rc;
  CritCoefArgs a{};
  a.est = est; a.est_ld = est_ld; a.tgt = tgt; a.tgt_ld = tgt_ld;
  set_criterion(a, B, N, sdr_type, zero_mean, take_log, eps);
  a.partial = (const double*)scratch;  // the first array of eval_scratch, as sepvad_eval_separation left it
  a.perm = (const long long*)perm; a.coef = coef;
  HIPRET(launch_crit_coef(a, (hipStream_t)stream));
}

int32_t sepvad_criterion_backward(int32_t B, const float* est, int64_t est_ld, const float* tgt, int64_t tgt_ld,
                                  int64_t N, const double* coef, const float* g_sep, float* grad_est, int64_t grad_ld,
                                  const float* vad, const float* labels, const int64_t* perm, int32_t T,
                                  const float* g_vad, float* grad_vad, void* stream) {
  if (B < 1 || B > 65535) return fail(SEPVAD_E_ARG, "sepvad_criterion_backward: need 1 <= B <= 65535");
  if (!est && !vad) return fail(SEPVAD_E_ARG, "sepvad_criterion_backward: neither a separation nor a VAD part");
  CritGradArgs a{};
  a.B = B;
  if (est) {
    if (!tgt || !coef || !g_sep || !grad_est) return fail(SEPVAD_E_ARG, "sepvad_criterion_backward: null pointer (separation part)");
    if (N < 1 || N > (1LL << 40)) return fail(SEPVAD_E_ARG, "sepvad_criterion_backward: need 1 <= N <= 2^40");
    if (est_ld < N || tgt_ld < N || grad_ld < N) return fail(SEPVAD_E_ARG, "sepvad_criterion_backward: row strides must be >= N");
    const int64_t nchunk = (N + CG_CHUNK - 1) / CG_CHUNK;
    if (B * nchunk > INT32_MAX) return fail(SEPVAD_E_ARG, "sepvad_criterion_backward: more than 2^31 - 1 workgroups (fewer utterances per call)");
    a.est = est; a.est_ld = est_ld; a.tgt = tgt; a.tgt_ld = tgt_ld; a.N = N; a.nchunk = (int)nchunk;
    a.coef = coef; a.g_sep = g_sep; a.grad_est = grad_est; a.grad_ld = grad_ld;
  }
  if (vad) {
    if (!labels || !g_vad || !grad_vad) return fail(SEPVAD_E_ARG, "sepvad_criterion_backward: null pointer (VAD part)");
    if (T < 1) return fail(SEPVAD_E_ARG, "sepvad_criterion_backward: need T >= 1");
    a.vad = vad; a.labels = labels; a.perm = (const long long*)perm; a.T = T; a.g_vad = g_vad; a.grad_vad = grad_vad;
  }
  HIPRET(launch_crit_grad(a, (hipStream_t)stream));
}

// The tail with a backward (model/model.py:421-461; csrc/tail_grad.hip).
namespace {
static_assert(TG_NPAR == SEPVAD_TAIL_NPAR, "gpar layout (include/sepvad.h)");
const char* tail_shape(int32_t B, int32_t N) {
  if (B < 1 || B > 32767) return "need 1 <= B <= 32767";
  return N <= HOP || N >= (1 << 29) ? "need 256 < N < 2^29 (reflect padding of the STFT)" : nullptr;
}
// Its scratch, each array once: the forward's frame-major buffers as the workspace has them (handle.h ws_each; the
// record arrays without its slack), then over the same bytes the backward's arrays (sepvad_internal.h TailGradArgs)
void tail_scratch(Workspace& w, TailGradArgs& g, int32_t B, int32_t N, ScratchPlan& p) {
  const int T = 1 + N / HOP;
  const size_t rows = (size_t)B * round_up(T, TILE), bst = (size_t)B * 2 * T;
  p.take(w.X, rows * NBIN); p.take(w.specdb, rows * SPEC_LD); p.take(w.S0, rows * CH);
  p.take(w.rec_gate, rows / GATE_ROWS * 2); p.take(w.vy, rows * 2 * 4); p.take(w.rec_vad, rows / VAD_ROWS * 2 * 2);
  p.rewind();
  p.take(g.feat, bst * 4); p.take(g.gz, bst); p.take(g.gyd, bst * 4); p.take(g.gy, bst * 4);
  p.take(g.part_small, (size_t)B * 2 * TG_NSMALL); p.take(g.part_w1, (size_t)B * 2 * tg_w1_chunks(T) * TG_NW1);
}
// The refusals both directions share, then the arrays of w and g in the caller's scratch
int32_t tail_check(const std::string& e, sepvad_handle h, int32_t B, int32_t N, int64_t ldx, void* scratch,
                   int64_t scratch_bytes, Workspace& w, TailGradArgs& g) {
  if (!h) return fail(SEPVAD_E_ARG, e + "null handle");
  if (const char* why = tail_shape(B, N)) return fail(SEPVAD_E_ARG, e + why);
  if (ldx < N || ldx > INT32_MAX) return fail(SEPVAD_E_ARG, e + "row stride must be >= N");
  if (h->cfg.final_vad && h->cfg.final_vad_masked_speakers)
    return fail(SEPVAD_E_ARG, e + "final_vad_masked_speakers has no backward");
  return scratch_bind(e, scratch, scratch_bytes, 256, "sepvad_tail_scratch_bytes",
                      [&](ScratchPlan& p) { tail_scratch(w, g, B, N, p); });
}
}  // namespace

int64_t sepvad_tail_scratch_bytes(int32_t B, int32_t N) {
  if (const char* why = tail_shape(B, N)) return fail(SEPVAD_E_ARG, std::string("sepvad_tail_scratch_bytes: ") + why);
  Workspace w{}; TailGradArgs g{};
  return plan_bytes([&](ScratchPlan& p) { tail_scratch(w, g, B, N, p); });
}

int32_t sepvad_tail_forward(sepvad_handle h, const float* x, int64_t ldx, const float* masks_fm, int32_t B, int32_t N,
                            void* scratch, int64_t scratch_bytes, float* sep, float* vad, void* stream) {
  Workspace w{}; TailGradArgs unused{};
  if (const int32_t rc = tail_check("sepvad_tail_forward: ", h, B, N, ldx, scratch, scratch_bytes, w, unused)) return rc;
  if (!x || !masks_fm || !sep || (h->cfg.final_vad && !vad)) return fail(SEPVAD_E_ARG, "sepvad_tail_forward: null pointer");
  DeviceGuard dg(h->device);
  w.masks = const_cast<float*>(masks_fm);  // (read only by the stages that run)
  return tail_stages(h, w, x, (int)ldx, B, N, sep, vad, (hipStream_t)stream);
}

int32_t sepvad_tail_backward(sepvad_handle h, const float* x, int64_t ldx, const float* masks_b, int32_t B, int32_t N,
                             const float* g_sep, int64_t gs_b, int64_t gs_s, int64_t gs_n, const float* g_vad,
                             int64_t gv_b, int64_t gv_s, int64_t gv_t, const double* vadw, void* scratch,
                             int64_t scratch_bytes, float* g_masks, double* gpar, void* stream) {
  Workspace unused{}; TailGradArgs a{}, no_vad{};  // (the scratch arrays are bound only with a VAD gradient)
  if (const int32_t rc = tail_check("sepvad_tail_backward: ", h, B, N, ldx, scratch, scratch_bytes, unused, g_vad ? a : no_vad))
    return rc;
  if (!x || !masks_b) return fail(SEPVAD_E_ARG, "sepvad_tail_backward: null pointer");
  if (!g_sep && !g_vad) return fail(SEPVAD_E_ARG, "sepvad_tail_backward: neither upstream gradient");
  if (!g_masks && !(g_vad && gpar)) return fail(SEPVAD_E_ARG, "sepvad_tail_backward: nothing to compute");
  if (g_vad && !h->cfg.final_vad) return fail(SEPVAD_E_ARG, "sepvad_tail_backward: g_vad without a VAD head");
  if (g_vad && !vadw) return fail(SEPVAD_E_ARG, "sepvad_tail_backward: g_vad without the VAD head's parameters");
  if (gs_b < 0 || gs_s < 0 || gs_n < 0 || gv_b < 0 || gv_s < 0 || gv_t < 0)
    return fail(SEPVAD_E_ARG, "sepvad_tail_backward: negative stride");
  DeviceGuard dg(h->device);
  a.B = B; a.N = N; a.T = 1 + N / HOP; a.x = x; a.ldx = ldx; a.masks = masks_b;
  a.g_sep = g_sep; a.gs_b = gs_b; a.gs_s = gs_s; a.gs_n = gs_n;
  a.g_vad = g_vad; a.gv_b = gv_b; a.gv_s = gv_s; a.gv_t = gv_t;
  a.win_x = h->P(h->win_out); a.win_inv = h->P(h->win_inv); a.tw = (const float2*)h->P(h->tw);
  if (g_vad) { a.vw = vadw; a.eps = 1e-8f; a.gpar = gpar; }
  a.g_masks = g_masks;
  HIPRET(launch_tail_grad(a, (hipStream_t)stream));
}

// The output head with a backward (model/model.py:322-325,357; csrc/head_grad.hip).
namespace {
static_assert(HG_NPAR == SEPVAD_HEAD_NPAR, "hpar and gpar layout (include/sepvad.h)");
const char* head_shape(int32_t B, int32_t T) {
  if (B < 1 || B > 32767) return "need 1 <= B <= 32767";
  return T < 2 || T > (1 << 20) ? "need 2 <= T <= 2^20" : nullptr;
}
// The refusals both directions share, then a's shapes, inputs and scratch arrays (sepvad_internal.h head_scratch)
int32_t head_check(const std::string& e, const float* y, int32_t B, int32_t T, const double* hpar, void* scratch,
                   int64_t scratch_bytes, HeadArgs& a) {
  if (const char* why = head_shape(B, T)) return fail(SEPVAD_E_ARG, e + why);
  if (!y || !hpar) return fail(SEPVAD_E_ARG, e + "null pointer");
  a.B = B; a.T = T; a.y = y; a.hp = hpar;
  return scratch_bind(e, scratch, scratch_bytes, 256, "sepvad_head_scratch_bytes", [&](ScratchPlan& p) { head_scratch(a, p); });
}
}  // namespace

int64_t sepvad_head_scratch_bytes(int32_t B, int32_t T) {
  if (const char* why = head_shape(B, T)) return fail(SEPVAD_E_ARG, std::string("sepvad_head_scratch_bytes: ") + why);
  HeadArgs a{};
  a.B = B; a.T = T;
  return plan_bytes([&](ScratchPlan& p) { head_scratch(a, p); });
}

int32_t sepvad_head_forward(const float* y, int32_t B, int32_t T, const double* hpar, void* scratch,
                            int64_t scratch_bytes, float* masks_b, void* stream) {
  HeadArgs a{};
  if (const int32_t rc = head_check("sepvad_head_forward: ", y, B, T, hpar, scratch, scratch_bytes, a)) return rc;
  if (!masks_b) return fail(SEPVAD_E_ARG, "sepvad_head_forward: null pointer");
  a.masks = masks_b;
  HIPRET(launch_head_forward(a, (hipStream_t)stream));
}

int32_t sepvad_head_backward(const float* y, const float* G, int64_t g_b, int64_t g_m, int64_t g_t, int32_t B, int32_t T,
                             const double* hpar, void* scratch, int64_t scratch_bytes, float* g_y, double* gpar,
                             void* stream) {
  HeadArgs a{};
  if (const int32_t rc = head_check("sepvad_head_backward: ", y, B, T, hpar, scratch, scratch_bytes, a)) return rc;
  if (!G) return fail(SEPVAD_E_ARG, "sepvad_head_backward: null pointer");
  if (g_b < 0 || g_m < 0 || g_t < 0) return fail(SEPVAD_E_ARG, "sepvad_head_backward: negative stride");
  if (!g_y && !gpar) return fail(SEPVAD_E_ARG, "sepvad_head_backward: nothing to compute");
  a.G = G; a.g_b = g_b; a.g_m = g_m; a.g_t = g_t; a.g_y = g_y; a.gpar = gpar;
  HIPRET(launch_head_backward(a, (hipStream_t)stream));
}

int32_t sepvad_normalize(const float* x, int64_t n, float* y, void* scratch, void* stream) {
  if (!x || !y || !scratch || n < 1) return fail(SEPVAD_E_ARG, "sepvad_normalize: bad arguments");
  static_assert(NORM_MAX_BLOCKS * 2 * sizeof(float) <= SEPVAD_NORM_SCRATCH_BYTES, "scratch size");
  NormArgs a{};
  a.x = x; a.n = n; a.y = y; a.part = (float*)scratch;
  HIPRET(launch_normalize(a, (hipStream_t)stream));
}
}  // extern "C"
