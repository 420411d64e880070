// The stream-ordered launch sequence of one SeparationModel.forward (reference model/model.py:402-461), its
// per-forward knobs and its diagnostics.
//
// Per forward (B utterances, T frames, 24 blocks), the default fused flow (enqueue_chunk, fused_ok):
//   k_stft_gate (STFT, activity gate, TCN input, TCN.LN records)
//   -> k_tcn: the whole TCN and the output head (with the VAD conv1_1 tap products) as persistent launches
//      (tcn_kernel.h), as many per forward as the epoch budget asks for; "big" launches are ordered across streams
//   -> [k_vad_feat for T > 256] -> k_istft_pair (VAD tail, est = X * sigmoid(mask), iSTFT)
// The fallback, the multi-kernel flow (SEPVAD_FUSED=0 / sepvad_set_fused(0), or an utterance whose group does not fit
// the co-resident capacity or FG_MAX):
//   k_stft_gate -> 24 x [ conv1d GEMM (loader: previous block's residual update)
//                         -> k_dw_stats (d, split) -> res_out GEMM (reg2 folded into W / epilogue)
//                         -> k_att_stats ]
//   -> k_head_stats -> output GEMM (loader: residual update, PReLU, GN) -> k_vad1 -> k_istft_pair
// The stages are the members of Chunk below; the per-forward environment knobs (tests and diagnostics) are one table, KNOBS.
#include <cstdio>
#include <cstdlib>
#include <unordered_map>

#include "handle.h"

namespace sepvad {
// ---- The per-forward environment knobs ----
// Read once per forward (read_knobs at the top of forward_impl; sepvad_fused_status reads them for its report) --
// per forward, not per handle: the tests flip them between two forwards on one handle. None is needed in production.
// Not here: the create-time knobs SEPVAD_SPLIT, SEPVAD_FUSED, SEPVAD_WLO (context.hip model_create) and
// SEPVAD_MAX_STREAM_CTX (context.hip get_ctx: sepvad_reserve reaches it outside a forward).
struct KnobDef {
  const char* name;
  int Knobs::*num;          // an integer knob (atoi of the value), or
  const char* Knobs::*str;  // a string knob (nullptr when unset)
  int dflt;
};
constexpr KnobDef KNOBS[] = {
    // tests (tests/test_gpu_fused.py, tests/test_gpu_boundary.py set them between forwards)
    {"SEPVAD_TCN_SLICES", &Knobs::tcn_slices, nullptr, 0},  // 1 | 2: force one- / two-slice workgroups (2 where it applies)
    {"SEPVAD_TCN_WQ16", &Knobs::tcn_wq16, nullptr, 1},      // 0: two-slice launches stream the int8 lo bytes, not their fp16 copy
    {"SEPVAD_TCN_XMODE", &Knobs::tcn_xmode, nullptr, 0},    // != 0: every hand-off store writes through (no same-XCD L2 path)
    {"SEPVAD_TCN_ALIGN8", &Knobs::tcn_align8, nullptr, 0},  // 1: whole multiples of 8 groups per launch only
    {"SEPVAD_TCN_MAX_GROUPS", &Knobs::tcn_max_groups, nullptr, 0},  // > 0: at most this many groups per launch
    {"SEPVAD_TCN_MAX_ITER", &Knobs::tcn_max_iter, nullptr, 0},  // n: at most n utterances per group and launch
    {"SEPVAD_TCN_SALT_MAX", &Knobs::tcn_salt_max, nullptr, SALT_MAX},  // the salt wraps here (clamped to 2 .. SALT_MAX)
    {"SEPVAD_TCN_FORCE_GIVEUP", &Knobs::tcn_force_giveup, nullptr, 0},  // 1: report a give-up without one happening
    {"SEPVAD_TCN_DELAY", &Knobs::tcn_delay, nullptr, 0},  // n: member 0 of every group sleeps n x ~8k cycles before its polls
    {"SEPVAD_VAD_FEAT", &Knobs::vad_feat, nullptr, KNOB_UNSET},  // 1: k_vad_feat, 0: the tap sums in k_istft_pair; unset: T > 256
    // diagnostics (tools/)
    {"SEPVAD_TCN_SPIN_LIMIT", &Knobs::tcn_spin_limit, nullptr, 1 << 20},  // poll passes before a hand-off wait gives up
    {"SEPVAD_TCN_NBLK", &Knobs::tcn_nblk, nullptr, 0},      // > 0: run only the first n blocks (wrong results)
    {"SEPVAD_TCN_DUMP_BLOCK", &Knobs::tcn_dump_block, nullptr, 0},  // the block whose tensors sepvad_set_tcn_dump receives
    {"SEPVAD_TCN_PROBE", nullptr, &Knobs::tcn_probe, 0},    // path: k_tcn phase stamps of the first launch (tools/tcn_probe.py)
    {"SEPVAD_TCN_PROBE_WARM", &Knobs::tcn_probe_warm, nullptr, 0},  // 1: an unprobed launch before the probed one
    {"SEPVAD_TCN_CLOCK", &Knobs::tcn_clock, nullptr, 0},    // 1: per-launch span and shader clock records (sepvad_tcn_clock)
    {"SEPVAD_TCN_INFO", &Knobs::tcn_info, nullptr, 0},      // 1: print every k_tcn launch's shape to stderr
    {"SEPVAD_GIVEUP_INFO", &Knobs::giveup_info, nullptr, 0},  // 1: print the first timed-out wait of a reported give-up
    {"SEPVAD_TAIL_PROBE", nullptr, &Knobs::tail_probe, 0},  // path prefix: phase stamps of the tail kernels (tools/tail_probe.py)
    {"SEPVAD_PROBE_BLOCK", nullptr, &Knobs::probe_block, 0},  // block index: GEMM wall-clock stamps of that block (tools/probe.py)
    {"SEPVAD_PROBE_OUT", nullptr, &Knobs::probe_out, 0},    // path of the SEPVAD_PROBE_BLOCK dump
};
Knobs read_knobs() {
  Knobs k{};
  for (const KnobDef& d : KNOBS) {
    if (d.num) k.*d.num = env_int(d.name, d.dflt);
    else k.*d.str = getenv(d.name);
  }
  return k;
}

namespace {
static_assert(SEPVAD_PREC_FP32 == PREC_F32 && SEPVAD_PREC_F16X3 == PREC_F16X3 && SEPVAD_PREC_F16 == PREC_F16 &&
              SEPVAD_PREC_BF16 == PREC_BF16, "precision codes");

// The weight set (handle.h WeightSet) of a fused launch with nsl slices per workgroup: the handle's precision and
// lo-plane format pick it. Two slices, int8 lo plane: the same lo values streamed as fp16 (no widening VALU beside the
// MFMAs; at two slices the weight stream is not the bound). Bitwise equal to the int8 kernel: its widening is exact
// (tcn_common.h lo8_widen), so both feed the MFMAs the same fp16 operands; taken where the fp16-lo kernel's two-slice
// capacity is at least the int8 kernel's. SEPVAD_TCN_WQ16=0 (wq16): the int8 kernel.
const WeightSet& wset_of(const sepvad_model* h, int nsl = 1, int wq16 = 0) {
  int k = h->prec == PREC_F16X3 ? h->lo8 : (h->prec == PREC_F16 ? WSET_F16 : (h->prec == PREC_BF16 ? WSET_BF16 : WSET_F32));
  if (k == WSET_X3_I8 && nsl == 2 && wq16 >= 1 && h->wset[WSET_X3_F16].cap[1] >= h->wset[k].cap[1]) k = WSET_X3_Q16;
  return h->wset[k];
}

// The fused TCN runs when an utterance fits one group (T <= 32 * FG_MAX = 8192) and a group fits the co-resident
// capacity of the variant that will run; otherwise the multi-kernel path runs (same results within fp32 rounding).
bool fused_ok(const sepvad_model* h, int T) {
  const int G = (T + FR - 1) / FR;
  return h->fused && G <= FG_MAX && wset_of(h).cap[0] >= G;
}

// Slices (32-frame members) per k_tcn workgroup for a batch of B utterances of G members: two (64 frames, tcn_kernel.h
// TcnSmem2) once one-slice workgroups would need more than one round of the chip (B * G > capacity), so every weight
// fragment a CU streams feeds 64 frames instead of 32; the two give the same bits, so the choice never changes a
// result. SEPVAD_TCN_SLICES = 1 | 2 forces one (2 where the two-slice kernel applies: G even, G <= FG_WAVE).
int tcn_slices(const sepvad_model* h, const Knobs& kn, int B, int G) {
  const WeightSet& ws = wset_of(h);
  if (G % 2 || G > FG_WAVE || ws.cap[1] < G / 2) return 1;
  if (kn.tcn_slices) return kn.tcn_slices == 2 ? 2 : 1;
  const int per_round = std::max(1, ws.cap[0] / G);  // utterances in one round of one-slice groups
  return B > per_round ? 2 : 1;
}

// Progress of concurrent fused launches (include/sepvad.h: concurrent forwards on different streams are allowed).
// A k_tcn group waits for all of its G members, and the grid is dealt in order, so a launch progresses as long as
// 8 G of its workgroups are resident (tcn_kernel.h header). Two launches that each need more than half the chip for
// that can each hold part of the CUs and wait on each other until the give-up bound. Such "big" launches (long
// utterances) are therefore ordered across streams, process-wide per device: each waits on the previous one's
// completion event (stream-ordered, no host sync). Launches of small groups need no ordering: any resident prefix
// of 8 G workgroups completes them, beside a big launch too, and they free their CUs.
bool tcn_big(int cap, int gw) { return 8 * gw > cap / 2; }
// Runs `launch` (which enqueues one big k_tcn launch on s) behind the previous big launch of the device and records
// its completion as the next one's wait, all under one process-wide lock: two handles (or two threads) on the same
// device can then never both wait on the same predecessor and run their big launches side by side.
template <class F>
int tcn_launch_ordered(int device, hipStream_t s, F&& launch) {
  static std::mutex mu;
  static std::unordered_map<int, hipEvent_t> last;  // device -> the last big launch's completion
  std::lock_guard<std::mutex> lk(mu);
  hipEvent_t& e = last[device];
  if (e) HIPCHK(hipStreamWaitEvent(s, e, 0));
  if (const int rc = launch()) return rc;
  // a fresh event per launch: a wait already enqueued never sees a later record of the same event
  hipEvent_t n = nullptr;
  HIPCHK(hipEventCreateWithFlags(&n, hipEventDisableTiming));
  HIPCHK(hipEventRecord(n, s));
  if (e) HIPCHK(hipEventDestroy(e));  // (released once its waits have completed)
  e = n;
  return SEPVAD_OK;
}

// Per-forward timing state (sepvad_set_timing): HIP events around the GEMM launches of chunk 0.
struct TimingRec {
  std::vector<int> gemm_ev, g2_ev;
};

int ev_record(sepvad_model* h, hipStream_t s) {
  if (!h->timing) return 0;
  hipEvent_t e;
  HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(e, s));
  h->ev.push_back(e);
  return 0;
}

// A synchronous stamp dump (tools/probe.py, tools/tcn_probe.py, tools/tail_probe.py): drains s, copies ncopy stamps
// back and writes {hdr, the first nwrite stamps} to path (no file without a path, or where it cannot be opened).
hipError_t dump_stamps(hipStream_t s, const unsigned long long* dev, size_t ncopy, size_t nwrite, const char* path,
                       std::initializer_list<long long> hdr) {
  std::vector<unsigned long long> hp(ncopy);
  hipError_t e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipMemcpy(hp.data(), dev, ncopy * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (e != hipSuccess || !path) return e;
  if (FILE* f = fopen(path, "wb")) {
    fwrite(hdr.begin(), sizeof(long long), hdr.size(), f);
    fwrite(hp.data(), sizeof(unsigned long long), nwrite, f);
    fclose(f);
  }
  return hipSuccess;
}

// Diagnostics (SEPVAD_TAIL_PROBE=<prefix>): per-workgroup phase stamps of a tail kernel, dumped synchronously
// to <prefix>.<kernel> as {grid x, grid y, 8} + [workgroups][8] (tools/tail_probe.py). Inactive otherwise.
struct TailProbe {
  static constexpr size_t N = 8192 * 8;
  hipStream_t s;
  std::string path;
  unsigned long long* buf = nullptr;
  TailProbe(sepvad_model* h, hipStream_t s_, const Knobs& kn, const char* kernel) : s(s_) {
    if (!kn.tail_probe) return;
    path = std::string(kn.tail_probe) + "." + kernel;
    if (!h->kprobe && hipMalloc(&h->kprobe, N * sizeof(unsigned long long)) != hipSuccess) return;
    if (hipMemsetAsync(h->kprobe, 0, N * sizeof(unsigned long long), s) == hipSuccess) buf = h->kprobe;
  }
  hipError_t dump(long long gx, long long gy) {
    const size_t n = (size_t)std::min<long long>(gx * gy * 8, (long long)N);
    return buf ? dump_stamps(s, buf, n, n, path.c_str(), {gx, gy, 8}) : hipSuccess;
  }
};

void set_weights(const sepvad_model* h, GemmArgs& g, const PackedW& w) {
  g.prec = h->prec;
  g.ascale = 1.f;
  g.W32 = h->P(w.w32);
  g.Whi = h->H(w.whi);
  g.Wlo = h->H(w.wlo);
  g.Wbf = h->H(w.wbf);
  g.wscale = h->P(w.scale);
}

// The residual-stream transform that turns (o_i, r_i) of block i into the next block input.
GnSrc gn_src(const double* rec, int nrec, int rstride, int roff, const float* g, const float* be, float eps) {
  return GnSrc{rec, nrec, rstride, roff, g, be, eps};
}

LoadSpec residual_spec(const sepvad_model* h, const Workspace& w, int i, const float* O, const float* R, int Tp) {
  LoadSpec ld{};
  ld.X = O; ld.X2 = R;
  if (h->cfg.tf_attention) { ld.at = w.at; ld.af = w.af; }
  const BlockOff& bo = h->blk[i];
  if (h->cfg.ln_mode == SEPVAD_LN_RECURSIVE) {
    ld.mode = LD_RECURSIVE;
    ld.gn = gn_src(w.rec_mom, Tp / STAT_ROWS, NMOM, 0, h->P(bo.lna_g), h->P(bo.lna_b), 1e-5f);
    ld.g2 = h->P(bo.lnb_g); ld.be2 = h->P(bo.lnb_b); ld.eps2 = 1e-5f;
    for (int j = 0; j < 5; ++j) ld.wsum[j] = bo.wsum[j];
  } else if (h->cfg.ln_mode == SEPVAD_LN_RESIDUAL) {
    ld.mode = LD_RESIDUAL;  // (Σr', Σr'²) at offsets 2, 3 of the moment record
    ld.gn = gn_src(w.rec_mom, Tp / STAT_ROWS, NMOM, 2, h->P(bo.lna_g), h->P(bo.lna_b), 1e-5f);
  } else {
    ld.mode = LD_ADD;
  }
  return ld;
}

// The gated dB spectrum as a side output (self.spectrum), recomputed from the stored STFT (or from specdb when the
// two STFT windows differ): the same arithmetic as k_stft_gate's gate
GateArgs side_gate_args(const sepvad_model* h, const Workspace& w, int B, int T, int Tp, float* spec_side) {
  GateArgs ga{};
  ga.B = B; ga.T = T; ga.Tp = Tp; ga.activity = h->cfg.activity_input;
  ga.X = h->same_stft_window ? w.X : nullptr; ga.specdb = w.specdb; ga.w = h->P(h->gate);
  ga.spec_side = spec_side;  // (no S0, no records: the side pass)
  return ga;
}

// ---- The stages of one chunk ----
// Utterances [b0, b0 + B) of one forward on stream s; what one stage hands to another is an argument.
struct Chunk {
  sepvad_model* h;
  StreamCtx* cx;
  Workspace w;  // the chunk's slice of the context's workspace
  int b0, B, N, T, Tp;
  const SepVadOutputs* out;
  hipStream_t s;
  TimingRec* tr;
  const Knobs& kn;
  int ev() const { return tr ? ev_record(h, s) : 0; }
  int timed_gemm(const GemmArgs& g, int ep, bool res_out = false) const;  // with the timing events around it
  int front_end(const float* x, int ldx, int nstr, long long hopw) const;
  int tcn_fused(bool vad_in_head, unsigned* gsalt_lo_out, unsigned* gsalt_n_out) const;
  int tcn_multi() const;
  int vad_stage(bool has_vad, bool vad_in_head, bool* taps_in_istft) const;
  int back_end(const SepVadInferKw* kw, bool has_vad, bool vad_in_head, bool taps_in_istft, unsigned gsalt_lo,
               unsigned gsalt_n) const;
};
int Chunk::timed_gemm(const GemmArgs& g, int ep, bool res_out) const {
  if (ev()) return SEPVAD_E_HIP;
  HIPCHK(launch_gemm(g, ep, s));
  if (ev()) return SEPVAD_E_HIP;
  if (tr) tr->gemm_ev.push_back((int)h->ev.size() - 2);
  if (tr && res_out) tr->g2_ev.push_back((int)h->ev.size() - 2);
  return SEPVAD_OK;
}

// 1+2. STFT (spec_output for est; spec_input for the spectrum: one transform when the windows are equal)
// fused with the activity gate, the TCN input and the TCN.LN statistics (k_stft_gate)
int Chunk::front_end(const float* x, int ldx, int nstr, long long hopw) const {
  StftArgs sa = stft_gate_args(h, w, x + (size_t)b0 * ldx, ldx, B, N);
  if (nstr > 0) { sa.nstr = nstr; sa.hopw = hopw; }
  TailProbe tp(h, s, kn, "stft");
  sa.probe = tp.buf;
  HIPCHK(launch_stft_gate(sa, s));
  HIPCHK(tp.dump(B, Tp / (2 * GATE_ROWS)));  // k_stft_gate's grid (32 own frames)
  if (out->spectrum)  // eager side output (Handle.forward(return_aux=True))
    HIPCHK(launch_gate(side_gate_args(h, w, B, T, Tp, out->spectrum + (size_t)b0 * NBIN * T), s));
  return SEPVAD_OK;
}

// 3+4, fused: persistent launches of the whole TCN (tcn_kernel.h), the output head inside them. The salts of the
// chunk's launches come back in gsalt_lo / gsalt_n (give-up poisoning, k_istft_pair).
int Chunk::tcn_fused(bool vad_in_head, unsigned* gsalt_lo_out, unsigned* gsalt_n_out) const {
  const int G = (T + FR - 1) / FR;
  const int nsl = h->tdump ? 1 : tcn_slices(h, kn, B, G);  // (the parity-dump instantiation is one-slice only)
  const WeightSet& ws = wset_of(h, nsl, kn.tcn_wq16);
  const int cap = ws.cap[nsl - 1];
  h->last_nsl = nsl;
  const int Gt = G / nsl;  // workgroups per utterance
  TcnArgs ta{};
  ta.T = T; ta.Tp = Tp; ta.G = G; ta.nsl = nsl; ta.nblk = h->nblk; ta.layer = h->cfg.layer;
  if (const int nb = kn.tcn_nblk; nb > 0 && nb < h->nblk) ta.nblk = nb;  // diagnostics: truncated stack
  ta.ln_mode = ld_mode_of(h->cfg);
  ta.tf_att = h->cfg.tf_attention;
  ta.prec = ws.prec;
  ta.lo8 = ws.lo8;
  ta.wfrag = ws.blocks;
  ta.prm = h->tprm;
  ta.inv_ch = 1.0 / ((double)CH * T);
  ta.inv_hid = 1.0 / ((double)HID * T);
  ta.alpha_h = h->out_a;
  ta.gran = cx->tgran; ta.err = cx->terr; ta.herr = cx->herr_dev;
  ta.xmode = kn.tcn_xmode;
  ta.spin_limit = (unsigned)kn.tcn_spin_limit;
  ta.force_err = kn.tcn_force_giveup;
  ta.dbg_delay = (unsigned)std::max(0, kn.tcn_delay);
  ta.dump_blk = std::max(0, std::min(h->nblk - 1, kn.tcn_dump_block));
  // every group the chip holds (the kernel puts the groups of 8 * Gt * floor(groups / 8) blocks on one XCD each and the
  // rest, fewer than 8, on consecutive blocks; SEPVAD_TCN_ALIGN8=1: whole multiples of 8 groups only, as in round 4)
  int ngroups = std::min(B, cap / Gt);
  if (ngroups >= 8 && kn.tcn_align8) ngroups -= ngroups % 8;
  // the output head, inside k_tcn after each utterance's last block (its planes in the blocks' format)
  ta.hg = h->P(h->out_g); ta.hbe = h->P(h->out_b); ta.hsx = h->out_sx;
  ta.hwh = ws.hwh; ta.hwl = ws.hwl;
  ta.hwscale = h->P(h->wout_spk.scale); ta.hbias = h->P(h->bo_spk);
  ta.hnyw = h->P(h->out_nyw); ta.hnyb = h->P(h->out_nyb);
  if (vad_in_head) {
    ta.hvwh = h->H(h->vadw.fhi); ta.hvwl = h->H(h->vadw.flo); ta.hvwscale = h->P(h->vadw.scale);
    ta.hvwf = h->P(h->vadw.ff32);
    ta.hvny = h->P(h->vad_ny);
    ta.hvsx = h->vad_sx;
  }
  // diagnostics (SEPVAD_TCN_MAX_GROUPS): fewer groups per launch, so each loops over more utterances (tests reach
  // the epoch budget below with small batches)
  if (const int mg = kn.tcn_max_groups; mg > 0 && mg < ngroups) ngroups = mg;
  // groups above 32 members (whole files, one slice): XCD runs (tcn_kernel.h RUN: R = ceil(G / 8) consecutive members
  // per XCD, a group on 8 R blocks), where that costs this batch no group of the round
  if (nsl == 1 && G > 32) {
    const int R = (G + 7) / 8;
    if (std::min(B, cap / (8 * R)) >= ngroups) ta.run = R;
  }
  const int gstride = ta.run ? 8 * ta.run : Gt;  // blocks per group
  // epochs per launch and group (tcn_kernel.h): 1 (XCD ids) + per utterance 4 per block with TF-attention (P1..P4;
  // 3 without) + 1 for the output head (P5). The tag is salt << TCN_EPOCH_BITS | epoch, so the last epoch of a
  // launch must stay below 2^TCN_EPOCH_BITS: an epoch carried into the salt bits would repeat the next launch's tags
  // (SEPVAD_TCN_MAX_ITER lowers it: tests force several launches per forward)
  const int ep_utt = 4 * h->nblk + 1;
  int max_iter = ((1 << TCN_EPOCH_BITS) - 2) / ep_utt;
  if (const int mi = kn.tcn_max_iter) max_iter = std::min(max_iter, mi);
  if (max_iter < 1) return fail(SEPVAD_E_ARG, "fused TCN: too many blocks");
  if (1 + (long long)max_iter * ep_utt >= (1 << TCN_EPOCH_BITS)) return fail(SEPVAD_E_ARG, "fused TCN: epoch budget");
  const int per_launch = max_iter * ngroups;
  const char* probe_path = kn.tcn_probe;
  const size_t probe_n = (size_t)h->tcn_cap * h->nblk * 16 * 9;  // wave-0 region + per-wave region
  // this chunk's launch salts, reserved as one range (salt_reserve: never 0, no wrap inside the range)
  const bool warm = probe_path && kn.tcn_probe_warm;
  unsigned gsalt_lo = 0, gsalt_n = 0;
  if (const int rc = salt_reserve(h, cx, s, kn, (unsigned)((B + per_launch - 1) / per_launch + (warm ? 1 : 0)), &gsalt_lo))
    return rc;
  for (int u0 = 0; u0 < B; u0 += per_launch) {
    const int Bl = std::min(per_launch, B - u0);
    const int grid = std::min(ngroups, Bl) * gstride;
    ta.tag0 = (gsalt_lo + gsalt_n++) << TCN_EPOCH_BITS;
    ta.B = Bl;
    ta.S0 = w.S0 + (size_t)u0 * Tp * CH;
    ta.ln = gn_src(w.rec_gate + (size_t)u0 * (Tp / GATE_ROWS) * 2, Tp / GATE_ROWS, 2, 0, h->P(h->ln_g), h->P(h->ln_b), 1e-8f);
    ta.hmasks = w.masks + (size_t)u0 * Tp * MOUT_PAD;
    ta.hvP = vad_in_head ? w.vP + (size_t)u0 * 2 * Tp * HEAD_VAD_N : nullptr;
    ta.probe = nullptr;
    ta.dump = (h->tdump && u0 == 0 && Bl == B) ? h->tdump : nullptr;
    if (probe_path && u0 == 0) {
      if (!h->tprobe) HIPCHK(hipMalloc(&h->tprobe, probe_n * sizeof(unsigned long long)));
      HIPCHK(hipMemsetAsync(h->tprobe, 0, probe_n * sizeof(unsigned long long), s));
      ta.probe = h->tprobe;
      if (warm) {  // diagnostics: an unprobed launch first (warm caches)
        TcnArgs tw = ta;
        tw.probe = nullptr;
        HIPCHK(launch_tcn(tw, grid, s));
        ta.tag0 = (gsalt_lo + gsalt_n++) << TCN_EPOCH_BITS;
      }
    }
    ta.clk = nullptr;
    if (kn.tcn_clock) {  // diagnostics: per-launch span and shader clock (sepvad_tcn_clock)
      if (!h->tclk) {
        HIPCHK(hipMalloc(&h->tclk, (size_t)TCLK_RECS * 8 * sizeof(unsigned long long)));
        HIPCHK(hipMemset(h->tclk, 0, (size_t)TCLK_RECS * 8 * sizeof(unsigned long long)));
      }
      ta.clk = h->tclk + (size_t)(h->tclk_n++ % TCLK_RECS) * 8;
      HIPCHK(hipMemsetAsync(ta.clk, 0, 8 * sizeof(unsigned long long), s));
    }
    if (kn.tcn_info)  // diagnostics: the persistent launch's shape
      fprintf(stderr, "sepvad: k_tcn grid=%d G=%d slices=%d groups=%d B=%d capacity=%d run=%d\n", grid, G, nsl,
              grid / gstride, Bl, cap, ta.run);
    TailProbe thp(h, s, kn, "tcnhead");
    ta.hprobe = u0 == 0 ? thp.buf : nullptr;
    auto run = [&]() -> int {
      if (ev()) return SEPVAD_E_HIP;
      HIPCHK(launch_tcn(ta, grid, s));
      if (ev()) return SEPVAD_E_HIP;
      return SEPVAD_OK;
    };
    if (const int rc = tcn_big(cap, gstride) ? tcn_launch_ordered(h->device, s, run) : run()) return rc;
    if (ta.hprobe) HIPCHK(thp.dump(grid, 1));
    if (tr) {
      tr->gemm_ev.push_back((int)h->ev.size() - 2);
      tr->g2_ev.push_back((int)h->ev.size() - 2);
    }
    if (ta.probe) {  // diagnostics only: {grid, nblk, G, T} + the wave-0 stamps + the per-wave stamps (kernel layout)
      const size_t n0 = (size_t)grid * h->nblk * 16;
      HIPCHK(dump_stamps(s, h->tprobe, probe_n, 9 * n0, probe_path, {grid, h->nblk, Gt, T}));
    }
  }
  // the eager masks_b copy if asked
  if (out->masks_b) {
    MaskSideArgs m{};
    m.B = B; m.T = T; m.Tp = Tp; m.masks = w.masks; m.masks_b = out->masks_b + (size_t)b0 * MOUT * T;
    HIPCHK(launch_mask_side(m, s));
  }
  *gsalt_lo_out = gsalt_lo;
  *gsalt_n_out = gsalt_n;
  return SEPVAD_OK;
}

// 3+4, multi-kernel: the TCN blocks and the output head as GEMMs and statistics kernels
int Chunk::tcn_multi() const {
  const SepVadConfig& c = h->cfg;
  const int ntu = Tp / TILE;
  const size_t g1_grid = (size_t)B * ntu * (CH / TILE);
  const bool probing = tr && h->probe && h->probe_blk >= 0;
  // 3. TCN blocks
  int cur = 0;  // w.O[cur] holds the current block input o once the conv1d GEMM materialized it
  for (int i = 0; i < h->nblk; ++i) {
    const BlockOff& bo = h->blk[i];
    const int nxt = (i == 0) ? 0 : (cur ^ 1);
    GemmArgs g{};
    g.B = B; g.T = T; g.Tp = Tp; g.M = CH; g.Mreal = CH; g.K = CH; g.ldy = CH;
    set_weights(h, g, bo.w1);
    g.ascale = bo.sx;
    g.bias = h->P(bo.b1); g.prelu = bo.a1;
    if (i == 0) {
      g.ld.mode = LD_GN; g.ld.X = w.S0;   // TCN.LN (model/model.py:333)
      g.ld.gn = gn_src(w.rec_gate, Tp / GATE_ROWS, 2, 0, h->P(h->ln_g), h->P(h->ln_b), 1e-8f);
    } else {
      g.ld = residual_spec(h, w, i - 1, w.O[cur], w.R, Tp);
    }
    g.Xmat = w.O[nxt];
    g.Y = w.A;
    g.out_rec = w.rec_g1;
    if (probing && i == h->probe_blk) g.probe = h->probe;
    if (const int rc = timed_gemm(g, EP_PRELU_STATS)) return rc;
    cur = nxt;

    DwStatsArgs d{};
    d.B = B; d.T = T; d.Tp = Tp; d.dil = bo.dil; d.A = w.A;
    const GnSrc gn1 = gn_src(w.rec_g1, ntu * (CH / TILE), 2, 0, h->P(bo.g1), h->P(bo.be1), 1e-8f);
    d.gd1 = gn1; d.wd = h->P(bo.wd); d.bd = h->P(bo.bd); d.alpha = bo.a2;
    d.prec = h->prec; d.Dhi = w.Dhi; d.Dlo = w.Dlo; d.D32 = w.D32;
    d.out_rec = w.rec_dw;
    HIPCHK(launch_dw_stats(d, s));

    GemmArgs g2{};
    g2.B = B; g2.T = T; g2.Tp = Tp; g2.M = CH; g2.Mreal = CH; g2.K = HID; g2.ldy = CH;
    set_weights(h, g2, bo.w2);
    g2.bias = h->P(bo.b2);
    if (h->prec != PREC_F32) {
      g2.ld.mode = LD_SPLIT; g2.ld.Xh = w.Dhi; g2.ld.Xl = w.Dlo;
    } else {
      g2.ld.mode = LD_PLAIN; g2.ld.X = w.D32;
    }
    g2.fold = gn_src(w.rec_dw, Tp / STAT_ROWS, 2, 0, nullptr, nullptr, bo.eps2);  // d pre-scaled (range guard)
    g2.foldK = HID; g2.foldc = h->P(bo.fc2);
    g2.Y = w.R; g2.colsum = w.colsum; g2.rowsum = w.rowsum;
    if (probing && i == h->probe_blk) g2.probe = h->probe + g1_grid * PROBE_SLOTS;
    if (const int rc = timed_gemm(g2, EP_BIAS_ATT, true)) return rc;

    AttStatsArgs at{};
    at.B = B; at.T = T; at.Tp = Tp; at.mtiles = CH / TILE; at.ntiles = ntu; at.tf_att = c.tf_attention;
    at.ln_mode = ld_mode_of(c);
    at.R = w.R; at.O = w.O[cur]; at.colsum = w.colsum; at.rowsum = w.rowsum; at.attp = h->P(bo.attp);
    if (c.ln_mode == SEPVAD_LN_RECURSIVE) { at.ga = h->P(bo.lna_g); at.bea = h->P(bo.lna_b); }
    at.at = w.at; at.af = w.af; at.out_rec = w.rec_mom;
    HIPCHK(launch_att_stats(at, s));
  }
  // 4. output head: PReLU -> GN(1e-5) -> 1x1 256->514 (model/model.py:322-325,357)
  HeadStatsArgs hs{};
  hs.B = B; hs.T = T; hs.Tp = Tp;
  hs.ld = residual_spec(h, w, h->nblk - 1, w.O[cur], w.R, Tp);
  hs.ld.alpha_h = h->out_a;
  hs.out_rec = w.rec_hs;
  HIPCHK(launch_head_stats(hs, s));
  GemmArgs g{};
  g.B = B; g.T = T; g.Tp = Tp; g.M = MOUT_PAD; g.Mreal = MOUT; g.K = CH; g.ldy = MOUT_PAD;
  set_weights(h, g, h->wout);
  g.ascale = h->out_sx;
  g.bias = h->P(h->bo);
  g.ld = hs.ld;
  g.ld.head = 1;
  g.ld.gh = gn_src(w.rec_hs, Tp / STAT_ROWS, 2, 0, h->P(h->out_g), h->P(h->out_b), 1e-5f);
  g.Y = w.masks; g.Yside = out->masks_b ? out->masks_b + (size_t)b0 * MOUT * T : nullptr;
  return timed_gemm(g, EP_BIAS_OUT);
}

// 5. VAD conv1_1 (model/model.py:424-427,434-436): finished from the output head's tap products (k_vad_feat,
// BN_1-normalised features; vad_in_head), or the whole conv on the masks (k_vad1 + records). *taps_in_istft: neither,
// k_istft_pair finishes the tap sums itself.
int Chunk::vad_stage(bool has_vad, bool vad_in_head, bool* taps_in_istft) const {
  // SEPVAD_VAD_FEAT=0: the tap sums finished inside k_istft_pair (one launch fewer, k_vad_feat<4>'s items and order;
  // the BN_1 affine rounds differently: VAD probabilities equal to fp32 rounding), 1: k_vad_feat. Default: inside k_istft_pair for T <= 256, where every k_istft_pair workgroup's
  // whole-utterance BN_1 sums are 2 items per thread (cfg 2: +0.4 %, 152.4k vs 151.9k utt/s interleaved,
  // profiles/r06pv/vadfeat_lines.txt; round 2 had measured equal, profiles/r02av_ab_vadfeat.txt); longer utterances
  // keep k_vad_feat (each of the T / 11 workgroups would sum all 4 T items).
  *taps_in_istft = vad_in_head && !(kn.vad_feat == KNOB_UNSET ? (T > 256 ? 1 : 0) : kn.vad_feat);
  if (vad_in_head && !*taps_in_istft) {
    VadFeatArgs vf{};
    vf.B = B; vf.T = T; vf.Tp = Tp; vf.vP = w.vP;
    vf.b1 = h->P(h->v_b1); vf.alpha = h->v_a;
    vf.g = h->P(h->v_g); vf.be = h->P(h->v_b); vf.eps = 1e-8f;
    vf.feat = w.vy;
    vf.out_rec = T > VF_ONE_T ? w.rec_vad : nullptr;  // long utterances: partial records, BN_1 in k_istft_pair
    HIPCHK(launch_vad_feat(vf, s));
  }
  if (has_vad && !vad_in_head) {
    Vad1Args v{};
    v.B = B; v.T = T; v.Tp = Tp; v.masked_speakers = h->cfg.final_vad_masked_speakers;
    v.masks = w.masks; v.X = w.X;
    v.w1 = h->P(h->v_w1); v.b1 = h->P(h->v_b1); v.alpha = h->v_a;
    v.vy = w.vy; v.out_rec = w.rec_vad;
    TailProbe tp(h, s, kn, "vad1");
    v.probe = tp.buf;
    HIPCHK(launch_vad1(v, s));
    HIPCHK(tp.dump(B * 2, Tp / VAD_ROWS));
  }
  return SEPVAD_OK;
}

// 6. VAD tail + est = X * sigmoid(mask) [* smoothed VAD] -> iSTFT (model/model.py:429-460); gsalt_n > 0: the salts of
// the chunk's fused launches (give-up poisoning)
int Chunk::back_end(const SepVadInferKw* kw, bool has_vad, bool vad_in_head, bool taps_in_istft, unsigned gsalt_lo,
                    unsigned gsalt_n) const {
  const size_t u2 = (size_t)b0 * 2;
  const bool kw_on = kw && kw->enabled && h->cfg.final_vad;
  IstftArgs is = istft_pair_args(h, w.X, w.masks, B, N);
  is.has_vad = has_vad;
  if (has_vad) {
    is.kw_enabled = kw_on;
    is.filt = kw_on && (kw->filter_signals_by_smo_vad || kw->filter_signals_by_unsmo_vad);
    is.ret_smooth = kw_on && kw->return_smoothed_vad;
    is.thr = kw_on ? kw->threshold_activated_vad : 0.5f;
    is.vy = w.vy; is.w2 = h->P(h->v_w2); is.b2 = h->v_b2;
    is.vy_norm = vad_in_head && !taps_in_istft && T <= VF_ONE_T;
    if (taps_in_istft) {
      is.vP = w.vP; is.vb1 = h->P(h->v_b1); is.valpha = h->v_a; is.vy = nullptr;
    }
    is.vgn = gn_src(w.rec_vad, vad_in_head ? vf_nrec(Tp) : Tp / VAD_ROWS, 2, 0, h->P(h->v_g), h->P(h->v_b), 1e-8f);
    is.vad_out = out->vad ? out->vad + u2 * T : w.vad;
  }
  is.est_out = out->est ? (float2*)out->est + u2 * NBIN * T : nullptr;
  is.mask_out = out->mask ? out->mask + u2 * NBIN * T : nullptr;
  is.y = out->sep + u2 * N;
  if (gsalt_n > 0) { is.gerr = cx->terr; is.gsalt_lo = gsalt_lo; is.gsalt_n = gsalt_n; }
  TailProbe tp(h, s, kn, "istft");
  is.probe = tp.buf;
  HIPCHK(launch_istft_pair(is, s));
  HIPCHK(tp.dump(B, (T + 10) / 11));  // k_istft_pair's grid (IP_OWN = 11)
  return SEPVAD_OK;
}

// Enqueues the forward of utterances [b0, b0 + B) on stream s (model/model.py:402-461).
int enqueue_chunk(sepvad_model* h, StreamCtx* cx, const float* x, int ldx, int b0, int B, int N,
                  const SepVadOutputs* out, const SepVadInferKw* kw, hipStream_t s, TimingRec* tr,
                  int nstr, long long hopw, const Knobs& kn) {
  const int T = 1 + N / HOP;
  const int Tp = round_up(T, TILE);
  const SepVadConfig& c = h->cfg;
  const Chunk k{h, cx, ws_view(cx->ws, b0, Tp), b0, B, N, T, Tp, out, s, tr, kn};
  TraceRange stage("sepvad::stft_gate");
  if (const int rc = k.front_end(x, ldx, nstr, hopw)) return rc;
  stage.next("sepvad::tcn_head");
  const bool use_fused = fused_ok(h, T);
  h->last_fused = use_fused;
  const bool has_vad = c.final_vad && (!c.final_vad_masked_speakers || c.noisy_phase);
  // the VAD conv1_1 as the output head's second GEMM (raw masks in; the masked-speakers variant reads |X| too)
  const bool vad_in_head = use_fused && has_vad && !c.final_vad_masked_speakers;
  unsigned gsalt_lo = 0, gsalt_n = 0;
  if (const int rc = use_fused ? k.tcn_fused(vad_in_head, &gsalt_lo, &gsalt_n) : k.tcn_multi()) return rc;
  stage.next("sepvad::vad");
  bool taps_in_istft = false;
  if (const int rc = k.vad_stage(has_vad, vad_in_head, &taps_in_istft)) return rc;
  stage.next("sepvad::istft");
  return k.back_end(kw, has_vad, vad_in_head, taps_in_istft, gsalt_lo, gsalt_n);
}
}  // namespace

int tail_stages(sepvad_model* h, const Workspace& w, const float* x, int ldx, int B, int N, float* sep, float* vad,
                hipStream_t s) {
  const int T = 1 + N / HOP;
  Knobs kn{}; kn.vad_feat = KNOB_UNSET;  // not read_knobs(): no probe may write the handle here
  const SepVadOutputs out{sep, vad};
  const Chunk k{h, nullptr, w, 0, B, N, T, round_up(T, TILE), &out, s, nullptr, kn};
  const bool has_vad = h->cfg.final_vad != 0;  // (its masked-speakers variant is refused by the caller)
  bool taps_in_istft = false;
  if (const int rc = k.front_end(x, ldx, 0, 0)) return rc;
  if (const int rc = k.vad_stage(has_vad, false, &taps_in_istft)) return rc;
  return k.back_end(nullptr, has_vad, false, taps_in_istft, 0, 0);
}

int forward_impl(sepvad_model* h, const float* x, int ldx, int B, int N, const SepVadOutputs* out,
                 const SepVadInferKw* kw, hipStream_t s, int nstr, long long hopw) {
  const int T = 1 + N / HOP;
  const int Tp = round_up(T, TILE);
  const Knobs kn = read_knobs();  // every per-forward environment knob, read once
  StreamCtx* cx = nullptr;
  int rc = get_ctx(h, (void*)s, &cx);
  if (!rc) rc = check_giveup(cx, kn);  // an earlier forward on this stream whose k_tcn gave up: report it now
  if (!rc) rc = ws_reserve(cx, B, N);
  if (rc) return rc;
  cx->last_B = B;
  cx->last_N = N;
  cx->seq = ++h->fwd_seq;
  for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
  h->ev.clear();
  // diagnostics probe (single chunk only)
  const size_t probe_need = 2 * (size_t)B * (Tp / TILE) * (CH / TILE) * PROBE_SLOTS;
  h->probe_blk = -1;
  if (const char* pb = kn.probe_block) {
    if (probe_need > h->probe_n) {
      if (h->probe) (void)hipFree(h->probe);
      h->probe = nullptr;
      h->probe_n = 0;
      HIPCHK(hipMalloc(&h->probe, probe_need * sizeof(unsigned long long)));
      h->probe_n = probe_need;
    }
    HIPCHK(hipMemsetAsync(h->probe, 0, probe_need * sizeof(unsigned long long), s));
    h->probe_blk = atoi(pb);
  }
  const int nsplit = (h->probe_blk >= 0 || h->timing || fused_ok(h, T) || nstr > 0) ? 1
                                                                                       : std::max(1, std::min(h->split, B));
  TimingRec tr;
  if (nsplit == 1) {
    if (ev_record(h, s)) return SEPVAD_E_HIP;
    rc = enqueue_chunk(h, cx, x, ldx, 0, B, N, out, kw, s, h->timing || h->probe_blk >= 0 ? &tr : nullptr, nstr, hopw, kn);
    if (rc) return rc;
    if (ev_record(h, s)) return SEPVAD_E_HIP;
  } else {
    // fork: every internal stream waits for the caller's stream; join: the caller waits for all
    HIPCHK(hipEventRecord(h->fork, s));
    int b0 = 0;
    for (int k = 0; k < nsplit; ++k) {
      const int bc = B / nsplit + (k < B % nsplit ? 1 : 0);
      HIPCHK(hipStreamWaitEvent(h->sub[k], h->fork, 0));
      rc = enqueue_chunk(h, cx, x, ldx, b0, bc, N, out, kw, h->sub[k], nullptr, nstr, hopw, kn);
      HIPCHK(hipEventRecord(h->join[k], h->sub[k]));
      HIPCHK(hipStreamWaitEvent(s, h->join[k], 0));
      if (rc) return rc;
      b0 += bc;
    }
  }
  if (h->timing) {
    HIPCHK(hipEventSynchronize(h->ev.back()));
    h->gemm_ms = h->g2_ms = 0.0;
    for (int k : tr.gemm_ev) { float ms; HIPCHK(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1])); h->gemm_ms += ms; }
    for (int k : tr.g2_ev) { float ms; HIPCHK(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1])); h->g2_ms += ms; }
    float tot; HIPCHK(hipEventElapsedTime(&tot, h->ev.front(), h->ev.back()));
    h->total_ms = tot;
    h->gemm_launches = (int)tr.gemm_ev.size();
    h->g2_launches = (int)tr.g2_ev.size();
  }
  if (h->probe && h->probe_blk >= 0)  // {workgroups per GEMM, slots, B, Tp} + the two GEMMs' stamps (tools/probe.py)
    HIPCHK(dump_stamps(s, h->probe, probe_need, probe_need, kn.probe_out,
                       {(long long)(probe_need / (2 * PROBE_SLOTS)), PROBE_SLOTS, B, Tp}));
  return SEPVAD_OK;
}

int side_outputs_locked(sepvad_model* h, const SepVadOutputs* out, void* stream) {
  StreamCtx* cx = find_ctx(h, stream);
  if (!cx || cx->last_B < 1) return fail(SEPVAD_E_ARG, "sepvad_side_outputs: no forward has run on this stream");
  const int B = cx->last_B, N = cx->last_N, T = 1 + N / HOP, Tp = round_up(T, TILE);
  const hipStream_t s = (hipStream_t)stream;
  const Workspace w = ws_view(cx->ws, 0, Tp);
  if (out->spectrum) HIPCHK(launch_gate(side_gate_args(h, w, B, T, Tp, out->spectrum), s));
  if (out->masks_b || out->mask) {
    MaskSideArgs m{};
    m.B = B; m.T = T; m.Tp = Tp; m.masks = w.masks; m.masks_b = out->masks_b; m.mask = out->mask;
    HIPCHK(launch_mask_side(m, s));
  }
  return SEPVAD_OK;
}
}  // namespace sepvad
