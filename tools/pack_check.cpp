// Stand-alone host check of csrc/pack.h (no GPU, no HIP runtime call); hipcc only because pack.h needs __half:
//   hipcc -std=c++17 -O2 --offload-arch=gfx950 tools/pack_check.cpp -o /tmp/pack_check && /tmp/pack_check
// and for a sanitizer run: -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
// (make -C sep-tfanet-vad_amd/csrc pack_check | pack_check_san build build/pack_check[_san]).
// Packs weights synthesised on demand from a seed (weight-norm g positive, as synth.py) for the smallest stacks that
// reach every branch of the packer (layer 5, stack 1: all dilations; every ln_mode; with and without TF-attention,
// VAD head and activity gate) and checks the fp16 split, the int8 lo plane, the fused TCN's blobs against the planes
// and parameters they are assembled from, and the errors of a missing and of a mis-sized tensor. Prints one digest per
// blob; exits non-zero on the first violation.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>

#include "../sep-tfanet-vad_amd/csrc/pack.h"

using namespace sepvad;

static const char* g_case = "";
static void require(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "pack_check: %s: %s\n", g_case, what);
    std::exit(1);
  }
}

// Tensors made when the packer asks for them, each in its own allocation of exactly the element count asked for (so a
// sanitizer sees any read past one). `missing` / `longer` name a tensor to withhold / to return one element too long.
struct Synth {
  unsigned seed;
  std::string missing, longer;
  std::map<std::string, std::vector<float>> made;
  std::pair<const float*, int64_t> operator()(const std::string& name, int64_t want) {
    if (name == missing) return {nullptr, 0};
    auto it = made.find(name);
    if (it == made.end()) {
      unsigned long long s = 1469598103934665603ull ^ seed;
      // (the three STFT windows share one stream: equal windows, the shipped checkpoints' case)
      for (char ch : name.find("window") != std::string::npos ? std::string("window") : name) s = (s ^ (unsigned char)ch) * 1099511628211ull;
      auto uni = [&]() {  // (-1, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0);
      };
      const bool ends_g = name.size() > 9 && name.compare(name.size() - 9, 9, ".weight_g") == 0;
      const bool bias = name.size() > 5 && name.compare(name.size() - 5, 5, ".bias") == 0;
      std::vector<float> v((size_t)(name == longer ? want + 1 : want));
      for (float& x : v) {
        const float u = uni();
        x = ends_g ? 0.75f + 0.5f * std::fabs(u) : (bias ? 0.1f * u : (want == 1 ? 0.25f + 0.1f * u : u));
      }
      it = made.emplace(name, std::move(v)).first;
    }
    return {it->second.data(), (int64_t)it->second.size()};
  }
};

static unsigned long long fnv(const void* p, size_t bytes) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return h;
}
template <class T>
static void digest(const char* blob, const std::vector<T>& v) {
  std::printf("%s %-7s %016llx %zu\n", g_case, blob, fnv(v.data(), v.size() * sizeof(T)), v.size() * sizeof(T));
}

struct Case {
  const char* name;
  int ln_mode, tf_attention, final_vad, activity_input;
};
static const Case CASES[] = {
    {"recursive", SEPVAD_LN_RECURSIVE, 1, 1, 1},
    {"residual", SEPVAD_LN_RESIDUAL, 1, 1, 1},
    {"plain", SEPVAD_LN_PLAIN, 1, 1, 1},
    {"bare", SEPVAD_LN_RECURSIVE, 0, 0, 0},
};
static SepVadConfig config_of(const Case& k) {
  SepVadConfig c{};
  c.n_fft = NFFT; c.bn_dim = CH; c.h_dim = HID; c.layer = 5; c.stack = 1; c.num_spk = 2;
  c.tf_attention = k.tf_attention; c.ln_mode = k.ln_mode; c.final_vad = k.final_vad; c.activity_input = k.activity_input;
  c.precision = SEPVAD_PREC_F16X3;
  return c;
}

static double h2d(__half h) { return (double)__half2float(h); }
static int exp_of_scale(float s) {  // s == 2^e exactly
  int e = 0;
  require(std::frexp(s, &e) == 0.5f, "a scale is not a power of two");
  return e - 1;
}

// One packed pointwise weight: rows [0, mpad) of cin, `real(o)` tells the rows that hold weights
template <class Real>
static void check_pointwise(const Packer& pk, const PackedW& p, int cin, int mpad, int col_e, Real real) {
  const float* w32 = pk.blob.data() + p.w32;
  const __half *hi = pk.hblob.data() + p.whi, *lo = pk.hblob.data() + p.wlo;
  std::vector<float> res((size_t)mpad * cin);  // the fp32 residual of the row-scaled weight
  for (int o = 0; o < mpad; ++o) {
    float mx = 0.f;
    for (int i = 0; i < cin; ++i) mx = std::max(mx, std::fabs(w32[(size_t)o * cin + i]));
    int e = 0;
    if (mx > 0.f) (void)std::frexp(mx, &e);
    require(real(o) || mx == 0.f, "a padded row holds a weight");
    require(pk.blob[p.scale + o] == std::ldexp(1.f, e + col_e), "row scale is not 2^(e + col_e)");
    for (int i = 0; i < cin; ++i) {
      const size_t x = (size_t)o * cin + i;
      const double ws = std::ldexp((double)w32[x], -e);
      require(ws >= -1.0 && ws < 1.0, "row-scaled weight outside [-1, 1)");
      require(std::fabs(ws - (h2d(hi[x]) + h2d(lo[x]))) <= std::ldexp(1.0, -24), "split error above 2^-24");
      require(real(o) || (h2d(hi[x]) == 0.0 && h2d(lo[x]) == 0.0), "a padded row's planes are not zero");
      res[x] = std::ldexp(w32[x], -e) - __half2float(hi[x]);
    }
  }
  // the int8 lo plane (K-step-pair order) against its fp16 copy (K-step order) and the residual
  const uint8_t* i8 = reinterpret_cast<const uint8_t*>(pk.hblob.data() + p.fi8);
  const __half *fq = pk.hblob.data() + p.fq, *fh = pk.hblob.data() + p.fhi;
  size_t b = 0;
  for (int mt = 0; mt < mpad / 32; ++mt)
    for (int pr = 0; pr < cin / 32; ++pr)
      for (int l = 0; l < 64; ++l)
        for (int h = 0; h < 2; ++h)
          for (int j = 0; j < 8; ++j, ++b) {
            const size_t src = (size_t)(32 * mt + (l & 31)) * cin + 16 * (2 * pr + h) + 8 * (l >> 5) + j;
            const size_t q = (((size_t)mt * (cin / 16) + 2 * pr + h) * 64 + l) * 8 + j;
            const double v = std::ldexp((double)((int)i8[b] - 128), -WQ_LO_SHIFT);
            require(v == h2d(fq[q]), "int8 lo byte and its fp16 copy differ");
            const bool sat = std::nearbyint(std::ldexp((double)res[src], WQ_LO_SHIFT)) > 127.0;
            require(!sat || i8[b] == 255, "a saturated int8 step is not 127");
            require(std::fabs(v - (double)res[src]) <= std::ldexp(1.0, sat ? -19 : -20), "int8 lo plane off the residual");
            require(h2d(fh[q]) == h2d(hi[src]), "fragment-ordered hi plane differs from the row-major one");
          }
}

static bool same(const void* a, const void* b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }

// The fused TCN's blobs against an independent statement of their layout (sepvad_internal.h WF_*, WQ_*, WS_*, PB_*)
static void check_fused(const Packed& pm, const FusedBlobs& fb, const SepVadConfig& c) {
  const Packer& pk = pm.pk;
  const int nblk = (int)pm.off.blk.size();
  const size_t want[NWSET] = {WF_BLOCK, WQ_BLOCK, WQ_BLOCK, WF_BLOCK, WS_BLOCK, WS_BLOCK, WS32_BLOCK};
  for (int k = 0; k < NWSET; ++k) require(fb.w[k].size() == want[k] * nblk, "weight-set blob size");
  require(fb.w[WSET_F32].size() * sizeof(__half) == (size_t)nblk * (WS32_BLOCK / 2) * sizeof(float), "fp32 blob size");
  require(fb.prm.size() == (size_t)PB_SIZE * nblk, "parameter blob size");
  const __half* H = pk.hblob.data();
  for (int i = 0; i < nblk; ++i) {
    const BlockOff& bo = pm.off.blk[i];
    const PackedW &a = bo.w1, &b = bo.w2;
    auto at = [&](int k, size_t off) { return fb.w[k].data() + want[k] * i + off; };
    const size_t n1 = (size_t)CH * CH, n2 = (size_t)CH * HID;  // elements of conv1d, res_out
    for (int k : {WSET_X3_F16, WSET_X3_Q16}) {
      const bool q = k == WSET_X3_Q16;
      require(same(at(k, 0), H + a.fhi, n1 * 2) && same(at(k, WF_W1L), H + (q ? a.fq : a.flo), n1 * 2) &&
              same(at(k, WF_W2H), H + b.fhi, n2 * 2) && same(at(k, WF_W2L), H + (q ? b.fq : b.flo), n2 * 2), "WF_* sub-ranges");
    }
    for (int k : {WSET_X3_E4M3, WSET_X3_I8}) {
      const bool e = k == WSET_X3_E4M3;
      require(same(at(k, 0), H + a.fhi, n1 * 2) && same(at(k, WQ_W1L), H + (e ? a.fl8 : a.fi8), n1) &&
              same(at(k, WQ_W2H), H + b.fhi, n2 * 2) && same(at(k, WQ_W2L), H + (e ? b.fl8 : b.fi8), n2), "WQ_* sub-ranges");
    }
    require(same(at(WSET_F16, 0), H + a.fhi, n1 * 2) && same(at(WSET_F16, WS_W2), H + b.fhi, n2 * 2), "WS_* sub-ranges (fp16)");
    require(same(at(WSET_BF16, 0), H + a.fbf, n1 * 2) && same(at(WSET_BF16, WS_W2), H + b.fbf, n2 * 2), "WS_* sub-ranges (bf16)");
    require(same(at(WSET_F32, 0), pk.blob.data() + a.ff32, n1 * 4) && same(at(WSET_F32, WS32_W2), pk.blob.data() + b.ff32, n2 * 4),
            "WS32_* sub-ranges");
    const float* q = fb.prm.data() + (size_t)PB_SIZE * i;
    auto slot = [&](int off, size_t src, int n) { return same(q + off, pk.blob.data() + src, n * sizeof(float)); };
    auto zero = [&](int off, int n) { return std::all_of(q + off, q + off + n, [](float v) { return v == 0.f; }); };
    require(slot(PB_WS1, a.scale, CH) && slot(PB_B1, bo.b1, CH) && slot(PB_G1, bo.g1, CH) && slot(PB_BE1, bo.be1, CH) &&
            slot(PB_WD, bo.wd, HID * 3) && slot(PB_BD, bo.bd, HID) && slot(PB_WS2, b.scale, CH) && slot(PB_B2, bo.b2, CH) &&
            slot(PB_FC2, bo.fc2, CH) && slot(PB_ATT, bo.attp, 20), "PB_* array slots");
    const bool rec = c.ln_mode == SEPVAD_LN_RECURSIVE, res = c.ln_mode == SEPVAD_LN_RESIDUAL;
    require(rec || res ? slot(PB_LNAG, bo.lna_g, CH) && slot(PB_LNAB, bo.lna_b, CH) : zero(PB_LNAG, 2 * CH), "PB_LNA*");
    require(rec ? slot(PB_LNBG, bo.lnb_g, CH) && slot(PB_LNBB, bo.lnb_b, CH) : zero(PB_LNBG, 2 * CH), "PB_LNB*");
    double sf = 0.0, sb = 0.0;
    for (int k = 0; k < CH; ++k) { sf += pk.blob[bo.fc2 + k]; sb += pk.blob[bo.b2 + k]; }
    require(q[PB_A1] == bo.a1 && q[PB_A2] == bo.a2 && q[PB_SX] == bo.sx && q[PB_EPS2] == bo.eps2 &&
            q[PB_SXN] == (i + 1 < nblk ? pm.off.blk[i + 1].sx : 1.f) && q[PB_SFC2] == (float)sf && q[PB_SB2] == (float)sb &&
            same(q + PB_WSUM, bo.wsum, sizeof(bo.wsum)), "PB_* scalar slots");
    require(bo.dil == (i == 0 ? 1 : i % 4 + 1), "dilation schedule");
  }
}

static void check_errors(const SepVadConfig& c, const char* name, long long numel) {
  Packed pm;
  std::string err;
  Synth miss{1u, name, ""};
  require(!pack_model(c, std::ref(miss), pm, err) && err == std::string("missing state_dict entry: ") + name, "missing-tensor error");
  Packed pm2;
  Synth big{1u, "", name};
  require(!pack_model(c, std::ref(big), pm2, err) &&
          err == std::string("state_dict entry ") + name + " has " + std::to_string(numel + 1) + " elements, expected " + std::to_string(numel),
          "mis-sized-tensor error");
}

int main() {
  for (const Case& k : CASES) {
    g_case = k.name;
    const SepVadConfig c = config_of(k);
    Synth src{20260u, "", ""};
    Packed pm;
    std::string err;
    require(pack_model(c, std::ref(src), pm, err), "pack_model refused a complete checkpoint");
    const ModelOff& m = pm.off;
    require((int)m.blk.size() == c.layer * c.stack && m.same_stft_window, "block count / windows");
    for (const BlockOff& bo : m.blk) {
      check_pointwise(pm.pk, bo.w1, CH, CH, -exp_of_scale(bo.sx), [](int) { return true; });
      check_pointwise(pm.pk, bo.w2, HID, CH, 0, [](int) { return true; });
    }
    const int eh = -exp_of_scale(m.out_sx);
    check_pointwise(pm.pk, m.wout, CH, MOUT_PAD, eh, [](int o) { return o < MOUT; });
    check_pointwise(pm.pk, m.wout_spk, CH, MOUT_PAD, eh, [](int o) { return o % HEAD_SPK < NBIN; });
    if (c.final_vad)
      check_pointwise(pm.pk, m.vadw, HEAD_SPK, 32, -exp_of_scale(m.vad_sx), [](int o) { return o < HEAD_VAD_N; });
    const FusedBlobs fb = pack_fused(pm, c);
    check_fused(pm, fb, c);
    digest("f32", pm.pk.blob);
    digest("f16", pm.pk.hblob);
    static const char* const names[NWSET] = {"x3_f16", "x3_e4m3", "x3_i8", "x3_q16", "f16w", "bf16w", "f32w"};
    for (int s = 0; s < NWSET; ++s) digest(names[s], fb.w[s]);
    digest("prm", fb.prm);
    // the packer's two errors, once per tensor family (every case reads the same names but for its own branches')
    if (k.ln_mode == SEPVAD_LN_RESIDUAL) check_errors(c, "TCN.ln_modules.4.weight", CH);
    if (&k != &CASES[0]) continue;
    check_errors(c, "spec_output.window", NFFT);
    check_errors(c, "TCN.TCN.4.res_out.weight_v", (long long)CH * HID);
    check_errors(c, "TCN.time_freq_attnetion.2.conv1d_f_1.weight", 3);
    check_errors(c, "TCN.ln_second_modules.1.bias", CH);
    check_errors(c, "TCN.output.2.bias", MOUT);
    check_errors(c, "vad.output_layer_vad.weight_v", 12);
    check_errors(c, "prelu.weight", 1);
  }
  std::printf("ok\n");
  return 0;
}
