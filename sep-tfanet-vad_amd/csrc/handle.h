// The handle behind include/sepvad.h and what its three translation units share: api.hip (the extern "C" surface),
// context.hip (handle lifetime, per-stream contexts, workspace, hand-off salts and give-up words) and forward.hip
// (knobs, schedule choice, the launch sequence and its diagnostics).
#pragma once
#include <climits>
#include <memory>
#include <mutex>

#include <rocprofiler-sdk-roctx/roctx.h>

#include "../../include/sepvad.h"
#include "pack.h"
#include "scratch_plan.h"

namespace sepvad {
// The calling thread's sepvad_last_error text (api.hip); fail returns `code`.
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return fail(SEPVAD_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
  } while (0)
// ... as a function's last statement: the check and `return SEPVAD_OK`
#define HIPRET(expr) do { HIPCHK(expr); return SEPVAD_OK; } while (0)

struct Workspace {
  int Bmax = 0, Tpmax = 0;
  char* base = nullptr;
  size_t bytes = 0;
  float2* X; float* specdb; float* S0; float* O[2]; float* A; float* R;
  float* masks; float* colsum; float* rowsum; float* at; float* af; float* vy; float* vad;
  float* vP;  // [B][2][Tp][HEAD_VAD_N] VAD conv1_1 tap products from k_tcn's output head (fused schedule)
  __half* Dhi; __half* Dlo; float* D32;  // res_out operand d (fp16 split planes, or fp32, same bytes)
  // partial records of the statistics producers (deterministic per-workgroup sums)
  double* rec_gate; double* rec_g1; double* rec_dw; double* rec_mom; double* rec_hs; double* rec_vad;
};

// The workspace layout, one line per array in allocation order: n elements per unit, a unit being `rows` frames of
// one utterance (1: per frame; 0: per utterance; a record producer's rows per workgroup), `slack` bytes after the
// array. Every array is utterance-major and starts on a 256-byte boundary. D32 overlays the Dhi and Dlo planes.
struct WsDim {
  // slack: the record arrays carry the 16 bytes their first hand-written layout gave them. Nothing reads or writes
  // them: a producer (k_stft_gate, k_vad1, the statistics kernels) stores exactly its own record through
  // block_reduce_store, and reduce_records and its staged variants (k_tcn, the res_out GEMM) load records r < n
  // only, value by value. A caller-owned copy of such an array (the tail's scratch) needs none.
  int n, rows = 1, slack = 0;
  bool overlay = false;  // shares the bytes of the arrays that follow
  size_t elems(int B, int Tp) const { return (size_t)B * (rows ? Tp / rows : 1) * n; }
};
template <class W, class F>
void ws_each(W& w, F&& f) {
  f(w.X, WsDim{NBIN}); f(w.specdb, WsDim{SPEC_LD}); f(w.S0, WsDim{CH});
  f(w.O[0], WsDim{CH}); f(w.O[1], WsDim{CH}); f(w.A, WsDim{CH}); f(w.R, WsDim{CH});
  f(w.masks, WsDim{MOUT_PAD});
  f(w.D32, WsDim{HID, 1, 0, true}); f(w.Dhi, WsDim{HID}); f(w.Dlo, WsDim{HID});
  f(w.colsum, WsDim{CH / TILE}); f(w.rowsum, WsDim{CH, TILE});
  f(w.at, WsDim{1}); f(w.af, WsDim{CH, 0}); f(w.vy, WsDim{2 * 4}); f(w.vad, WsDim{2});
  f(w.rec_gate, WsDim{2, GATE_ROWS, 16}); f(w.rec_g1, WsDim{CH / TILE * 2, TILE});
  f(w.rec_dw, WsDim{2, STAT_ROWS, 16}); f(w.rec_mom, WsDim{NMOM, STAT_ROWS, 16});
  f(w.rec_hs, WsDim{2, STAT_ROWS, 16}); f(w.rec_vad, WsDim{2 * 2, VAD_ROWS, 16});
  f(w.vP, WsDim{2 * HEAD_VAD_N});
}

// The workspace slice of utterances [b0, b0 + Bc) at padded length Tp: every per-utterance array
// is utterance-major, so a chunk is a pointer offset (no copies).
inline Workspace ws_view(const Workspace& w, int b0, int Tp) {
  Workspace v = w;
  ws_each(v, [&](auto*& p, const WsDim& d) { p += d.elems(b0, Tp); });
  return v;
}

// One pass of the planner over the layout: the arrays of w at `base` (null: none is written) for B utterances of Tp
// frames; returns the bytes. ws_bytes: the size pass alone, a pure host function.
inline size_t ws_plan(Workspace& w, char* base, int B, int Tp) {
  ScratchPlan p(base);
  ws_each(w, [&](auto*& a, const WsDim& d) { d.overlay ? p.overlay(a) : p.take(a, d.elems(B, Tp), d.slack); });
  return p.bytes();
}
inline size_t ws_bytes(int B, int Tp) { Workspace w{}; return ws_plan(w, nullptr, B, Tp); }

constexpr int MAX_SPLIT = 4;
constexpr int TCLK_RECS = 4096;  // SEPVAD_TCN_CLOCK records kept (ring)

// Per caller-stream state (include/sepvad.h: concurrent forwards on different streams of one handle are allowed): the
// workspace, the fused TCN's hand-off words, launch salt and give-up words. Weights are shared and read-only.
struct StreamCtx {
  void* stream = nullptr;
  Workspace ws;
  unsigned long long* tgran = nullptr;  // hand-off words [gran_slots][2][NGR]
  unsigned* terr = nullptr;             // device word: tag0 of the last launch whose hand-off wait gave up
  unsigned* herr = nullptr;             // host-mapped copy (pinned, written by the kernel)
  unsigned* herr_dev = nullptr;         // its device address
  unsigned reported = 0;                // last give-up word already returned to the caller
  unsigned pending = 0;                 // a give-up seen when the salt wrapped (words re-zeroed), not yet reported
  unsigned tsalt = 0;                   // launch counter (hand-off tag salt)
  int last_B = 0, last_N = 0;           // shape of the last forward on this stream (sepvad_side_outputs)
  long long seq = 0;                    // handle-wide id of the last forward on this stream (side outputs are tied to one)
  unsigned long long used = 0;          // LRU stamp (context cap, get_ctx)
  ~StreamCtx();  // frees the workspace and the words (context.hip; the handle's device is current)
};

// One weight set of the fused TCN on the device (pack.h WSetDef: its layout and the kernel that reads it)
struct WeightSet {
  __half* blocks = nullptr;                     // [nblk][block] fragment-ordered weights of the blocks
  const __half *hwh = nullptr, *hwl = nullptr;  // the output head's hi and lo planes in the same format
  int prec = 0, lo8 = 0, cap[2] = {};  // the kernel key; co-resident k_tcn workgroups (CUs x per CU) at one, two slices
};
}  // namespace sepvad

struct sepvad_model : sepvad::ModelOff {  // (the packer's offsets and scalars: pack.h)
  SepVadConfig cfg{};
  int device = 0;
  int nblk = 0;
  int prec = sepvad::PREC_F16X3;
  float* dparams = nullptr;   // packed fp32 weights (device)
  __half* dhalf = nullptr;    // packed fp16 split weights (device)
  // batch split: utterance chunks of one forward run concurrently on internal streams (fork/join
  // on the caller's stream); the chunks' kernels fill each other's ramp/drain bubbles
  int split = 1;
  hipStream_t sub[sepvad::MAX_SPLIT] = {};
  hipEvent_t fork = nullptr, join[sepvad::MAX_SPLIT] = {};
  // fused persistent TCN (tcn_kernel.h): one launch for all blocks when an utterance fits one group (T <= 8192)
  bool fused = true;
  sepvad::WeightSet wset[sepvad::NWSET];
  int tcn_cap = 0;              // co-resident k_tcn workgroups, max over the weight sets
  int lo8 = 2;                  // k_tcn's weight lo plane: 0 fp16, 1 e4m3, 2 int8 (default); SEPVAD_WLO / sepvad_set_weight_lo
  int gran_slots = 0;           // member slot pairs of a context's hand-off words: max(capacity, 2 x two-slice capacity)
  float* tprm = nullptr;        // [nblk][PB_SIZE] parameter blobs
  bool last_fused = false;
  int last_nsl = 1;             // 32-frame slices per k_tcn workgroup of the last fused forward (1 or 2)
  float* tdump = nullptr;       // parity probe buffer of the fused TCN (sepvad_set_tcn_dump), caller-owned
  // caller-stream contexts (workspace, hand-off words, give-up words); `mu` serialises the host-side
  // enqueue of concurrent callers (the kernels of different streams still overlap on the device)
  std::vector<std::unique_ptr<sepvad::StreamCtx>> ctx;
  std::mutex mu;
  unsigned long long use_clock = 0;  // LRU clock of the contexts (under mu)
  long long fwd_seq = 0;             // forwards enqueued on this handle (under mu): StreamCtx::seq
  int res_B = 0, res_N = 0;     // sepvad_reserve hint: every context's workspace is sized at least this
  unsigned long long* kprobe = nullptr;  // SEPVAD_TAIL_PROBE diagnostics: [workgroups][8]
  unsigned long long* tprobe = nullptr;  // SEPVAD_TCN_PROBE diagnostics: [tcn_cap][nblk][16]
  unsigned long long* tclk = nullptr;    // SEPVAD_TCN_CLOCK diagnostics: [TCLK_RECS][8] per-launch clock records
  long long tclk_n = 0;                  // k_tcn launches recorded so far
  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev;
  double gemm_ms = 0.0, g2_ms = 0.0, total_ms = 0.0;
  int gemm_launches = 0, g2_launches = 0;
  // diagnostics: per-workgroup timestamps of one block's two GEMMs (env SEPVAD_PROBE_BLOCK=<i>,
  // written to SEPVAD_PROBE_OUT after each forward)
  int probe_blk = -1;
  unsigned long long* probe = nullptr;
  size_t probe_n = 0;

  const float* P(size_t off) const { return dparams + off; }
  const __half* H(size_t off) const { return dhalf + off; }
};

namespace sepvad {
// Restores the caller's current HIP device on scope exit (torch shares this runtime).
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// The per-forward environment knobs (the table and read_knobs: forward.hip KNOBS)
constexpr int KNOB_UNSET = INT_MIN;
constexpr int SALT_MAX = (int)((1u << (32 - TCN_EPOCH_BITS)) - 1);  // the largest launch salt (tag = salt << bits | epoch)
struct Knobs {
  int tcn_slices, tcn_wq16, tcn_xmode, tcn_align8, tcn_max_groups, tcn_max_iter, tcn_salt_max, tcn_force_giveup, tcn_delay,
      vad_feat;
  int tcn_spin_limit, tcn_nblk, tcn_dump_block, tcn_probe_warm, tcn_clock, tcn_info, giveup_info;
  const char *tcn_probe, *tail_probe, *probe_block, *probe_out;
};
int env_int(const char* name, int dflt);
Knobs read_knobs();

// The config's residual-LN mode as the kernels' LD_* code
inline int ld_mode_of(const SepVadConfig& c) {
  return c.ln_mode == SEPVAD_LN_RECURSIVE ? LD_RECURSIVE : (c.ln_mode == SEPVAD_LN_RESIDUAL ? LD_RESIDUAL : LD_ADD);
}

// ---- context.hip ---- (model_create: the device half of sepvad_create, nullptr with the error set)
sepvad_model* model_create(const SepVadConfig& cfg, const Packed& pm, int device);
void model_destroy(sepvad_model* h);
int ws_reserve(StreamCtx* c, int B, int N);
StreamCtx* find_ctx(sepvad_model* h, void* stream);  // nullptr: no context of this stream (the caller holds h->mu)
int get_ctx(sepvad_model* h, void* stream, StreamCtx** out);
int release_ctx(sepvad_model* h, void* stream);
int salt_reserve(sepvad_model* h, StreamCtx* c, hipStream_t s, const Knobs& kn, unsigned n, unsigned* lo);
int check_giveup(StreamCtx* c, const Knobs& kn);

// ---- forward.hip ----
// Utterance u of a forward reads x + (u % nstr) * ldx + (u / nstr) * hopw (nstr = 0: a plain batch, row u at u * ldx)
int forward_impl(sepvad_model* h, const float* x, int ldx, int B, int N, const SepVadOutputs* out,
                 const SepVadInferKw* kw, hipStream_t s, int nstr = 0, long long hopw = 0);
// The forward's own front end, multi-kernel VAD stage and back end on the caller's workspace (X, specdb, S0, rec_gate,
// vy, rec_vad and its frame-major masks) for sepvad_tail_forward: no keywords, knobs, probes or timing, outputs sep and
// vad only. Touches nothing mutable of the handle (no h->mu needed).
int tail_stages(sepvad_model* h, const Workspace& w, const float* x, int ldx, int B, int N, float* sep, float* vad,
                hipStream_t s);
// sepvad_side_outputs with h->mu held by the caller (so a check of the forward's identity and the copies it guards
// are one critical section: no forward can be enqueued on the stream in between)
int side_outputs_locked(sepvad_model* h, const SepVadOutputs* out, void* stream);

// Host-side trace ranges (roctx: `rocprofv3 --marker-trace`), one per forward and per stage of its enqueue,
// so a host timeline shows where the forward's launch time goes; no-ops without a tool attached.
struct TraceRange {
  explicit TraceRange(const char* n) { roctxRangePushA(n); }
  void next(const char* n) { roctxRangePop(), roctxRangePushA(n); }
  ~TraceRange() { roctxRangePop(); }
};

// ---- kernel arguments filled the same way by the forward and by the *_test entries ----
// k_stft_gate on B rows of x: the STFT into X (spec_output window), the gated TCN input and the TCN.LN records into
// workspace w; specdb receives the dB spectrum only when the two STFT windows differ
inline StftArgs stft_gate_args(const sepvad_model* h, const Workspace& w, const float* x, int ldx, int B, int N) {
  StftArgs sa{};
  sa.B = B; sa.N = N; sa.ldx = ldx; sa.T = 1 + N / HOP; sa.Tp = round_up(sa.T, TILE); sa.x = x; sa.nstr = B; sa.hopw = 0;
  sa.tw = (const float2*)h->P(h->tw);
  sa.window = h->P(h->win_out);
  sa.window_db = h->same_stft_window ? sa.window : h->P(h->win_in);
  sa.X = w.X; sa.specdb = h->same_stft_window ? nullptr : w.specdb;
  sa.activity = h->cfg.activity_input; sa.gate_w = h->P(h->gate);
  sa.S0 = w.S0; sa.gate_rec = w.rec_gate;
  return sa;
}
// k_istft_pair without a VAD: est = X * sigmoid(masks) -> iSTFT of B utterances x 2 speakers
inline IstftArgs istft_pair_args(const sepvad_model* h, const float2* X, const float* masks, int B, int N) {
  IstftArgs is{};
  is.BS = B * 2; is.N = N; is.T = 1 + N / HOP; is.Tp = round_up(is.T, TILE);
  is.X = X; is.masks = masks;
  is.window = h->P(h->win_inv); is.tw = (const float2*)h->P(h->tw);
  return is;
}
}  // namespace sepvad
