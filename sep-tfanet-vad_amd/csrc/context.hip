// Handle lifetime and per-stream state (handle.h): the device half of sepvad_create and sepvad_destroy, the per-stream
// contexts with their workspace, and the hand-off salts and give-up words of the fused TCN.
#include <cstdio>
#include <cstdlib>

#include "handle.h"

namespace sepvad {
int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

int ws_reserve(StreamCtx* c, int B, int N) {
  const int T = 1 + N / HOP;
  const int Tp = round_up(T, TILE);
  Workspace& w = c->ws;
  if (B <= w.Bmax && Tp <= w.Tpmax) return SEPVAD_OK;
  const int Bm = std::max(B, w.Bmax), Tm = std::max(Tp, w.Tpmax);
  if (w.base) { (void)hipFree(w.base); w.base = nullptr; w.Bmax = w.Tpmax = 0; }
  // two passes over the layout (handle.h ws_each, ws_plan): the size, then the pointers
  const size_t bytes = ws_bytes(Bm, Tm);
  char* base = nullptr;
  HIPCHK(hipMalloc(&base, bytes));
  // zeroed on the context's own stream, ahead of the forward that reserved it: a null-stream hipMemset is not
  // ordered with a non-blocking caller stream, and once zeroed the workspace of a concurrent forward's first launch
  // mid-run (tests/test_gpu_boundary.py::test_two_streams_concurrently_match_serial, round 4)
  HIPCHK(hipMemsetAsync(base, 0, bytes, (hipStream_t)c->stream));
  ws_plan(w, base, Bm, Tm);
  w.base = base; w.bytes = bytes; w.Bmax = Bm; w.Tpmax = Tm;
  return SEPVAD_OK;
}

StreamCtx::~StreamCtx() {
  if (ws.base) (void)hipFree(ws.base);
  if (tgran) (void)hipFree(tgran);
  if (terr) (void)hipFree(terr);
  if (herr) (void)hipHostFree(herr);
}

StreamCtx* find_ctx(sepvad_model* h, void* stream) {
  for (auto& c : h->ctx)
    if (c->stream == stream) return c.get();
  return nullptr;
}

// The context of caller stream `stream` (created on first use; the caller holds h->mu).
int get_ctx(sepvad_model* h, void* stream, StreamCtx** out) {
  if (StreamCtx* c = find_ctx(h, stream)) { c->used = ++h->use_clock; *out = c; return SEPVAD_OK; }
  // cap the per-stream contexts (each holds a workspace, hand-off words and pinned memory): evict the least
  // recently used one after draining the whole device (SEPVAD_MAX_STREAM_CTX, default 32; include/sepvad.h notes the
  // device-wide stall)
  const size_t cap = (size_t)std::max(1, env_int("SEPVAD_MAX_STREAM_CTX", 32));
  while (h->ctx.size() >= cap) {
    size_t lru = 0;
    for (size_t i = 1; i < h->ctx.size(); ++i)
      if (h->ctx[i]->used < h->ctx[lru]->used) lru = i;
    // every enqueued use of its buffers done: the whole device is drained, because the context's stream may already be
    // destroyed with work pending (an event recorded after every forward cost each forward 5.8 us of queue time,
    // profiles/r05_gap/; eviction is rare: more live streams than the cap)
    HIPCHK(hipDeviceSynchronize());
    h->ctx.erase(h->ctx.begin() + lru);
  }
  std::unique_ptr<StreamCtx> c(new StreamCtx());
  c->stream = stream;
  if (h->tcn_cap > 0) {
    const size_t gb = (size_t)h->gran_slots * 2 * NGR * sizeof(unsigned long long);
    HIPCHK(hipMalloc(&c->tgran, gb));
    HIPCHK(hipMemsetAsync(c->tgran, 0, gb, (hipStream_t)stream));  // (ordered before this stream's first launch)
  }
  HIPCHK(hipMalloc(&c->terr, 16));
  HIPCHK(hipMemsetAsync(c->terr, 0, 16, (hipStream_t)stream));
  HIPCHK(hipHostMalloc((void**)&c->herr, 64, hipHostMallocMapped | hipHostMallocCoherent));
  std::memset(c->herr, 0, 64);
  HIPCHK(hipHostGetDevicePointer((void**)&c->herr_dev, c->herr, 0));
  if (h->res_B > 0) {
    const int rc = ws_reserve(c.get(), h->res_B, h->res_N);
    if (rc) return rc;
  }
  c->used = ++h->use_clock;
  *out = c.get();
  h->ctx.push_back(std::move(c));
  return SEPVAD_OK;
}

int release_ctx(sepvad_model* h, void* stream) {
  for (size_t i = 0; i < h->ctx.size(); ++i)
    if (h->ctx[i]->stream == stream) {
      HIPCHK(hipStreamSynchronize((hipStream_t)stream));
      h->ctx.erase(h->ctx.begin() + i);
      break;
    }
  return SEPVAD_OK;  // (or nothing held for this stream)
}

// n consecutive hand-off tag salts for the k_tcn launches of one forward chunk: never 0, and never wrapping inside
// the range (k_istft_pair poisons the outputs when the give-up word holds one of gsalt_lo .. gsalt_lo + n - 1). When
// the 20-bit salt would wrap, the stream is drained and the hand-off words, the device give-up word and its host copy
// restart from zero (a give-up not yet reported is kept in `pending`), so a reused salt never matches an old word.
int salt_reserve(sepvad_model* h, StreamCtx* c, hipStream_t s, const Knobs& kn, unsigned n, unsigned* lo) {
  const unsigned wrap_at = (unsigned)std::max(2, std::min(SALT_MAX, kn.tcn_salt_max));
  if (n > wrap_at) return fail(SEPVAD_E_ARG, "fused TCN: too many launches in one forward");
  if (c->tsalt + n > wrap_at) {
    HIPCHK(hipStreamSynchronize(s));
    const unsigned v = __atomic_load_n(c->herr, __ATOMIC_ACQUIRE);
    if (v != 0 && v != c->reported) c->pending = v;
    HIPCHK(hipMemsetAsync(c->tgran, 0, (size_t)h->gran_slots * 2 * NGR * sizeof(unsigned long long), s));
    HIPCHK(hipMemsetAsync(c->terr, 0, 16, s));
    __atomic_store_n(c->herr, 0u, __ATOMIC_RELEASE);
    c->reported = 0;
    c->tsalt = 0;
  }
  *lo = c->tsalt + 1;
  c->tsalt += n;
  return SEPVAD_OK;
}

// Give-up words written by k_tcn launches of this context that completed since the last check: report
// each once (the word holds the failing launch's salt, so a later give-up is a new value).
int check_giveup(StreamCtx* c, const Knobs& kn) {
  static const char* const msg = "fused TCN: a group hand-off wait gave up in an earlier forward on this stream "
                                 "(that forward's outputs are invalid)";
  if (kn.giveup_info && (c->pending != 0 || (c->herr[0] != 0 && c->herr[0] != c->reported))) {
    unsigned w[4] = {};  // diagnostics: {launch tag0, the timed-out wait's tag, its workgroup, its word index}
    if (hipMemcpy(w, c->terr, sizeof(w), hipMemcpyDeviceToHost) == hipSuccess)
      fprintf(stderr, "sepvad: give-up on stream %p: tag0 %#x, first timed-out wait: tag %#x (salt %u epoch %u) "
              "workgroup %u word %u (slot %u, offset %u)\n", c->stream, w[0], w[1], w[1] >> TCN_EPOCH_BITS,
              w[1] & ((1u << TCN_EPOCH_BITS) - 1), w[2], w[3], w[3] / NGR, w[3] % NGR);
    // reported: clear the diagnostic words (the first timed-out poller sets them by a compare-and-swap from 0), so a
    // later give-up on this context reports its own wait, not this one's
    // (synchronous, not on c->stream: a cached context's caller stream may already be destroyed)
    (void)hipMemset(c->terr + 1, 0, 3 * sizeof(unsigned));
  }
  if (c->pending != 0) {
    c->pending = 0;
    return fail(SEPVAD_E_HIP, msg);
  }
  const unsigned v = __atomic_load_n(c->herr, __ATOMIC_ACQUIRE);
  if (v != 0 && v != c->reported) {
    c->reported = v;
    return fail(SEPVAD_E_HIP, msg);
  }
  return SEPVAD_OK;
}

// A device copy of a host vector in a fresh allocation (*dst: freed with the handle)
template <class T, class U>
static hipError_t upload(T** dst, const std::vector<U>& src) {
  const hipError_t e = hipMalloc(dst, src.size() * sizeof(U));
  return e != hipSuccess ? e : hipMemcpy(*dst, src.data(), src.size() * sizeof(U), hipMemcpyHostToDevice);
}

// The fused TCN's weight-set table (pack.h WSETS), parameter blobs, residency capacities and hand-off slot count
static int init_fused(sepvad_model* h, const Packed& pm) {
  int ncu = 0;
  HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device));
  const FusedBlobs fb = pack_fused(pm, h->cfg);
  const PackedW& head = h->wout_spk;
  for (int k = 0; k < NWSET; ++k) {
    const WSetDef& d = WSETS[k];
    WeightSet& ws = h->wset[k];
    ws.prec = d.prec;
    ws.lo8 = d.lo8;
    // co-resident workgroups of the persistent kernel that will run (one 512-thread workgroup per CU and more); a
    // two-slice workgroup publishes two members' hand-off words
    for (int nsl = 1; nsl <= 2; ++nsl) ws.cap[nsl - 1] = ncu * tcn_blocks_per_cu(ld_mode_of(h->cfg), d.prec, d.cap_lo8, nsl);
    h->tcn_cap = std::max(h->tcn_cap, ws.cap[0]);
    h->gran_slots = std::max({h->gran_slots, ws.cap[0], 2 * ws.cap[1]});
    HIPCHK(upload(&ws.blocks, fb.w[k]));
    ws.hwh = d.prec == PREC_F32 ? reinterpret_cast<const __half*>(h->P(head.*d.hi)) : h->H(head.*d.hi);
    ws.hwl = h->H(head.*(d.lo ? d.lo : &PackedW::flo));
  }
  HIPCHK(upload(&h->tprm, fb.prm));
  if (h->tcn_cap < 1) h->fused = false;
  return SEPVAD_OK;
}

sepvad_model* model_create(const SepVadConfig& c, const Packed& pm, int device) {
  std::unique_ptr<sepvad_model, void (*)(sepvad_model*)> h(new sepvad_model(), model_destroy);
  static_cast<ModelOff&>(*h) = pm.off;
  h->cfg = c;
  h->device = device;
  h->nblk = c.layer * c.stack;
  h->prec = c.precision;  // SEPVAD_PREC_* == PREC_* (static_assert in forward.hip)
  if (const char* sp = getenv("SEPVAD_SPLIT")) h->split = std::max(1, std::min(MAX_SPLIT, atoi(sp)));
  bool streams_ok = hipEventCreateWithFlags(&h->fork, hipEventDisableTiming) == hipSuccess;
  for (int k = 0; k < MAX_SPLIT && streams_ok; ++k)
    streams_ok = hipStreamCreateWithFlags(&h->sub[k], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&h->join[k], hipEventDisableTiming) == hipSuccess;
  if (!streams_ok) {
    set_error("creating the internal streams/events failed");
    return nullptr;
  }
  if (upload(&h->dparams, pm.pk.blob) != hipSuccess || upload(&h->dhalf, pm.pk.hblob) != hipSuccess) {
    set_error("device allocation/upload of the packed weights failed");
    return nullptr;
  }
  if (const char* fz = getenv("SEPVAD_FUSED")) h->fused = atoi(fz) != 0;
  if (const char* wl = getenv("SEPVAD_WLO")) {  // "i8" (default) | "f16" | "e4m3"; anything else is an error
    if (std::strcmp(wl, "e4m3") == 0) h->lo8 = 1;
    else if (std::strcmp(wl, "f16") == 0) h->lo8 = 0;
    else if (std::strcmp(wl, "i8") == 0) h->lo8 = 2;
    else {
      set_error(std::string("SEPVAD_WLO: unknown weight lo-plane format '") + wl + "' (expected i8, f16 or e4m3)");
      return nullptr;
    }
  }
  if (init_fused(h.get(), pm) != SEPVAD_OK) return nullptr;
  return h.release();
}

void model_destroy(sepvad_model* h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
  for (int k = 0; k < MAX_SPLIT; ++k) {
    if (h->sub[k]) (void)hipStreamDestroy(h->sub[k]);
    if (h->join[k]) (void)hipEventDestroy(h->join[k]);
  }
  if (h->fork) (void)hipEventDestroy(h->fork);
  h->ctx.clear();
  for (WeightSet& ws : h->wset)
    if (ws.blocks) (void)hipFree(ws.blocks);
  for (void* p : {(void*)h->probe, (void*)h->tprm, (void*)h->tprobe, (void*)h->tclk, (void*)h->kprobe, (void*)h->dparams,
                  (void*)h->dhalf})
    if (p) (void)hipFree(p);
  delete h;
}
}  // namespace sepvad
