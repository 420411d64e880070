// Host-only weight folding and packing: checkpoint tensors -> the two device blobs, every offset and scalar the launches
// read from them (ModelOff), and the fused TCN's weight-set and parameter blobs (pack_fused). No HIP runtime call and no
// handle, so tools/pack_check.cpp runs all of it on the CPU under a sanitizer; sepvad_model (handle.h) embeds ModelOff.
#pragma once
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sepvad.h"
#include "sepvad_internal.h"

namespace sepvad {
// Packed pointwise-conv weight: fp32 [M][K] and the fp16 split of the row-scaled copy.
struct PackedW {
  size_t w32 = 0, whi = 0, wlo = 0, scale = 0;
  size_t fhi = 0, flo = 0;  // fused-TCN copies in MFMA B-fragment order (see pack_pointwise)
  size_t wbf = 0, fbf = 0;  // bf16 bits of the row-scaled weight, row-major and in fragment order (PREC_BF16)
  size_t fl8 = 0;           // e4m3 lo plane in K-step-pair fragment order (bytes, stored in hblob; sepvad_internal.h WQ_*)
  size_t fi8 = 0;           // ... the same as int8 steps of 2^-WQ_LO_SHIFT, biased by 128
  size_t fq = 0;            // the int8 lo plane's values (q * 2^-WQ_LO_SHIFT, exact) as fp16 in flo's order (two slices)
  size_t ff32 = 0;          // the row-scaled fp32 weight in the same fragment order (float blob; fused PREC_F32)
};

struct BlockOff {
  PackedW w1, w2;
  size_t b1, g1, be1, wd, bd, b2, g2, be2, attp, lna_g, lna_b, lnb_g, lnb_b;
  size_t fc2;  // res_out with reg2 folded in: w2 = W*gamma2, b2 = bias + W*beta2, fc2[m] = sum_k w2[m][k]
  float a1, a2;
  int dil;
  double wsum[5];  // {Σγa, Σβa, Σβa², Σγa·βa, Σγa²} of ln_first (closed-form recursive-LN stats)
  float sx;        // 2^-ex: fp16 range scale of the conv1d A operand (x'), undone by w1.scale (range guard)
  float eps2;      // reg2 eps * 2^-2ed: d is produced scaled by 2^-ed (dconv weights/bias pre-scaled)
};

// Where everything lies in the two blobs (offsets in floats / halves), and the scalars that travel as kernel arguments.
struct ModelOff {
  std::vector<BlockOff> blk;
  size_t win_in = 0, win_out = 0, win_inv = 0, tw = 0;
  size_t ln_g = 0, ln_b = 0;
  PackedW wout;
  size_t out_g = 0, out_b = 0, bo = 0;
  // k_tcn's copy of the output head: speaker q's 257 rows at rows [288 q, 288 q + 257) (zero rows to 288); its MFMA
  // tiles are rows [288 q, 288 q + 256), bin 256 of each speaker is out_ny (fp32 [2][CH] + bias [2]); the VAD conv1_1
  // as a second GEMM on each masks tile (B[c][4 k + o] = w1[o][c][k], 20 of 32 columns, speaker-local channels
  // c < 256; vad_ny[4 k + o] = w1[o][256][k])
  PackedW wout_spk, vadw;
  size_t bo_spk = 0, out_nyw = 0, out_nyb = 0, vad_ny = 0;
  float vad_sx = 1.f;  // fp16 range scale of the VAD GEMM's A operand (undone by vadw.scale)
  float out_sx = 1.f;  // fp16 range scale of the head GEMM's A operand (undone by wout.scale)
  float out_a = 0.f;
  size_t v_w1 = 0, v_b1 = 0, v_g = 0, v_b = 0, v_w2 = 0;
  float v_a = 0.f, v_b2 = 0.f;
  size_t gate = 0;
  bool same_stft_window = true;
};

// A tensor source of the packer: src(name, want) -> {data, element count} by state-dict name, {nullptr, 0} when there
// is none (`want` is the count the packer expects, for a source that makes its tensors on demand).
struct TensorMap {
  std::unordered_map<std::string, std::pair<const float*, int64_t>> m;
  std::pair<const float*, int64_t> operator()(const std::string& k, int64_t) const {
    auto it = m.find(k);
    return it == m.end() ? std::pair<const float*, int64_t>{nullptr, 0} : it->second;
  }
};

struct Packer {
  std::vector<float> blob;
  std::vector<__half> hblob;
  size_t add(const float* p, size_t n) {
    size_t off = blob.size();
    blob.insert(blob.end(), p, p + n);
    while (blob.size() % 4) blob.push_back(0.f);  // 16-byte aligned arrays (float4 loads)
    return off;
  }
  size_t add(const std::vector<float>& v) { return add(v.data(), v.size()); }
  size_t addh(const std::vector<__half>& v) {
    size_t off = hblob.size();
    hblob.insert(hblob.end(), v.begin(), v.end());
    while (hblob.size() % 8) hblob.push_back(__float2half_rn(0.f));
    return off;
  }
};

// torch.nn.utils.weight_norm (dim=0): w = v * (g / ||v||_2 over all dims but 0).
inline std::vector<float> fold_wn(const float* g, const float* v, int cout, int rest) {
  std::vector<float> w((size_t)cout * rest);
  for (int o = 0; o < cout; ++o) {
    double s = 0.0;
    for (int i = 0; i < rest; ++i) s += (double)v[(size_t)o * rest + i] * v[(size_t)o * rest + i];
    const float nrm = (float)std::sqrt(s);
    const float scale = g[o] / nrm;
    for (int i = 0; i < rest; ++i) w[(size_t)o * rest + i] = v[(size_t)o * rest + i] * scale;
  }
  return w;
}

// float -> bf16 bits, round to nearest even (finite inputs: weights)
inline __half bf16_bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  u = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
  const unsigned short b = (unsigned short)u;
  __half h;
  std::memcpy(&h, &b, 2);
  return h;
}

// float -> e4m3fn (OCP FP8: 1-4-3, bias 7, max 448 = 0x7e, 0x7f NaN, no inf): round to nearest even, saturating.
// The gfx950 conversions (v_cvt_scalef32_pk_f16_fp8) read the same OCP format.
inline uint8_t e4m3_rn(float x) {
  if (std::isnan(x)) return 0x7f;
  const uint8_t sg = std::signbit(x) ? 0x80 : 0x00;
  const double a = std::fabs((double)x);
  if (a >= 448.0) return sg | 0x7e;
  if (a < std::ldexp(1.0, -6)) {                       // subnormal range: m * 2^-9, m = 0..8 (8 = smallest normal)
    const int m = (int)std::nearbyint(std::ldexp(a, 9));  // the default rounding mode: to nearest even
    return sg | (uint8_t)m;
  }
  int k = 0;
  (void)std::frexp(a, &k);                             // a = f * 2^k, f in [0.5, 1): exponent E = k - 1
  int E = k - 1;
  int q = (int)std::nearbyint(std::ldexp(a, 3 - E));   // 8..16
  if (q == 16) { q = 8; ++E; }
  if (E > 8 || (E == 8 && q > 14)) return sg | 0x7e;   // rounded past 448: saturate
  return sg | (uint8_t)(((E + 7) << 3) | (q - 8));
}

// int8 step of a lo residual (|lo| <= 2^-12 -> |q| <= 128; +128, a tie at half an ulp of hi, saturates to 127)
inline int lo_q(float lo) {
  const double q = std::nearbyint(std::ldexp((double)lo, WQ_LO_SHIFT));
  return (int)std::max(-128.0, std::min(127.0, q));
}

// [cout][cin] fp32 -> zero-padded [mpad][cin] fp32 + the fp16 hi/lo split of each row scaled by
// 2^-e (e chosen so the row's max |w| lands in [0.5, 1)); scale[m] = 2^(e + col_e) undoes it exactly, and
// also the 2^-col_e the GEMM applies to its A operand before splitting it (range guard, see range_exp).
inline PackedW pack_pointwise(Packer& pk, const std::vector<float>& w, int cout, int cin, int mpad, int col_e = 0) {
  PackedW p;
  std::vector<float> w32((size_t)mpad * cin, 0.f), sc(mpad, 1.f);
  std::vector<__half> hi((size_t)mpad * cin), lo((size_t)mpad * cin), bf((size_t)mpad * cin);
  std::vector<float> lo32((size_t)mpad * cin);  // the exact fp32 residual (source of the e4m3 lo plane)
  std::vector<float> srow(mpad, 1.f);           // the row scale 2^-e
  for (int o = 0; o < mpad; ++o) {
    float mx = 0.f;
    if (o < cout)
      for (int i = 0; i < cin; ++i) mx = std::max(mx, std::fabs(w[(size_t)o * cin + i]));
    int e = 0;
    if (mx > 0.f) { (void)std::frexp(mx, &e); }  // mx = f * 2^e, f in [0.5, 1)
    const float s = std::ldexp(1.f, -e);
    srow[o] = s;
    sc[o] = std::ldexp(1.f, e + col_e);
    for (int i = 0; i < cin; ++i) {
      const float v = o < cout ? w[(size_t)o * cin + i] : 0.f;
      w32[(size_t)o * cin + i] = v;
      const float vs = v * s;
      const __half hh = __float2half_rn(vs);
      hi[(size_t)o * cin + i] = hh;
      lo32[(size_t)o * cin + i] = vs - __half2float(hh);
      lo[(size_t)o * cin + i] = __float2half_rn(lo32[(size_t)o * cin + i]);
      bf[(size_t)o * cin + i] = bf16_bits(vs);
    }
  }
  p.w32 = pk.add(w32);
  p.scale = pk.add(sc);
  p.whi = pk.addh(hi);
  p.wlo = pk.addh(lo);
  p.wbf = pk.addh(bf);
  // k_tcn streams each wave's 32 output rows as consecutive 1 KB fragments (v_mfma_f32_32x32x16_f16 B operand):
  // [mpad/32 row tiles][cin/16 K steps][64 lanes][8 halves], lane l -> row 32*mt + (l & 31), k = 16*s + 8*(l >> 5) + j.
  if (mpad % 32 == 0 && cin % 16 == 0) {
    std::vector<__half> fh((size_t)mpad * cin), fl((size_t)mpad * cin), fb((size_t)mpad * cin), fqv((size_t)mpad * cin);
    std::vector<float> ff((size_t)mpad * cin);
    size_t q = 0;
    for (int mt = 0; mt < mpad / 32; ++mt)
      for (int st = 0; st < cin / 16; ++st)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j, ++q) {
            const size_t src = (size_t)(32 * mt + (l & 31)) * cin + 16 * st + 8 * (l >> 5) + j;
            fh[q] = hi[src];
            fl[q] = lo[src];
            fb[q] = bf[src];
            fqv[q] = __float2half_rn(std::ldexp((float)lo_q(lo32[src]), -WQ_LO_SHIFT));  // exact in fp16
            // exact: a power-of-two row scale (PREC_F32: v_mfma_f32_32x32x2_f32 pairs k = 8 h + j, tcn_kernel.h)
            ff[q] = w32[src] * srow[src / cin];
          }
    p.ff32 = pk.add(ff);
    p.fhi = pk.addh(fh);
    p.flo = pk.addh(fl);
    p.fbf = pk.addh(fb);
    p.fq = pk.addh(fqv);
    // e4m3 lo plane: lane l, K-step pair pr -> 16 bytes: j = 0..7 of step 2 pr, then of step 2 pr + 1
    if ((cin / 16) % 2 == 0) {
      std::vector<uint8_t> f8((size_t)mpad * cin), i8((size_t)mpad * cin);
      size_t b = 0;
      for (int mt = 0; mt < mpad / 32; ++mt)
        for (int pr = 0; pr < cin / 32; ++pr)
          for (int l = 0; l < 64; ++l)
            for (int h = 0; h < 2; ++h)
              for (int j = 0; j < 8; ++j, ++b) {
                const size_t src = (size_t)(32 * mt + (l & 31)) * cin + 16 * (2 * pr + h) + 8 * (l >> 5) + j;
                f8[b] = e4m3_rn(lo32[src] * (float)(1 << WQ_LO_SHIFT));  // exact power-of-two scaling
                // int8: |lo| <= 2^-12 -> |q| <= 128; +128 (a tie at half an ulp of hi) saturates to 127
                i8[b] = (uint8_t)(lo_q(lo32[src]) + 128);
              }
      std::vector<__half> f8h(f8.size() / 2);
      std::memcpy(f8h.data(), f8.data(), f8.size());
      p.fl8 = pk.addh(f8h);
      std::memcpy(f8h.data(), i8.data(), i8.size());
      p.fi8 = pk.addh(f8h);
    }
  }
  return p;
}

// Range guard of the fp16 split: every A operand of the pointwise GEMMs is an affine image of
// GroupNorm-normalised data, so its magnitude is fixed by the GN affines and weights, not by the utterance:
// |y_k| <~ |gamma_k| * NSIG + |beta_k|. Each operand is scaled by a static power of two 2^-e that brings that bound
// into [0.5, 1); the inverse is folded into the weights' per-row scale (for d: into the dconv weights, the reg2 eps
// rescaled by 2^-2e): exact in fp32 arithmetic, bitwise neutral wherever nothing under- or overflowed.
constexpr double NSIG = 4.0;
inline double gn_bound(const float* g, const float* b, int n) {
  double m = 0.0;
  for (int k = 0; k < n; ++k) m = std::max(m, std::fabs((double)g[k]) * NSIG + std::fabs((double)b[k]));
  return m;
}
inline int range_exp(double bound) {
  if (!(bound > 0.0) || !std::isfinite(bound)) return 0;
  int e = 0;
  (void)std::frexp(bound, &e);  // bound = f * 2^e, f in [0.5, 1)
  return std::max(-60, std::min(60, e));
}

struct Packed {
  Packer pk;     // the fp32 blob and the fp16 blob, as uploaded
  ModelOff off;
};
// Folds and packs every tensor of a checkpoint of configuration c (validated by the caller). False with the
// reason in err when a tensor is missing or has the wrong element count.
template <class Src>
bool pack_model(const SepVadConfig& c, Src&& src, Packed& out, std::string& err) {
  struct Bad : std::runtime_error { using std::runtime_error::runtime_error; };
  auto get = [&](const std::string& k, int64_t numel) -> const float* {
    const auto t = src(k, numel);
    if (!t.first) throw Bad("missing state_dict entry: " + k);
    if (t.second != numel)
      throw Bad("state_dict entry " + k + " has " + std::to_string(t.second) + " elements, expected " + std::to_string(numel));
    return t.first;
  };
  Packer& pk = out.pk;
  ModelOff& h = out.off;
  const int nblk = c.layer * c.stack;
  try {
    // windows (model/model.py:383-387) and FFT twiddles
    const float* wi = get("spec_input.spec.window", NFFT);
    const float* wo = get("spec_output.window", NFFT);
    const float* wv = get("inv_spec.window", NFFT);
    h.win_in = pk.add(wi, NFFT);
    h.win_out = pk.add(wo, NFFT);
    h.win_inv = pk.add(wv, NFFT);
    h.same_stft_window = std::memcmp(wi, wo, NFFT * sizeof(float)) == 0;
    {
      std::vector<float> tw(2 * NFFT);
      for (int m = 0; m < NFFT; ++m) {
        const double ang = -2.0 * M_PI * m / NFFT;
        tw[2 * m] = (float)std::cos(ang);
        tw[2 * m + 1] = (float)std::sin(ang);
      }
      h.tw = pk.add(tw);
    }
    double xbound = 0.0;  // range bound of the current block's x' (range guard)
    {
      const float* lg = get("TCN.LN.weight", CH);
      const float* lb = get("TCN.LN.bias", CH);
      h.ln_g = pk.add(lg, CH);
      h.ln_b = pk.add(lb, CH);
      xbound = gn_bound(lg, lb, CH);  // x'_0 = TCN.LN(S0)
    }
    // blocks (model/model.py:285-295,103-127,182-195,310-319)
    for (int i = 0; i < nblk; ++i) {
      BlockOff bo{};
      const std::string p = "TCN.TCN." + std::to_string(i);
      const float* g1 = get(p + ".conv1d.weight_g", CH);
      const float* v1 = get(p + ".conv1d.weight_v", (int64_t)CH * CH);
      const float* gd = get(p + ".dconv1d.weight_g", HID);
      const float* vd = get(p + ".dconv1d.weight_v", (int64_t)HID * 3);
      const float* g2 = get(p + ".res_out.weight_g", CH);
      const float* v2 = get(p + ".res_out.weight_v", (int64_t)CH * HID);
      const float* b1 = get(p + ".conv1d.bias", CH);
      const float* bd = get(p + ".dconv1d.bias", HID);
      const float* b2 = get(p + ".res_out.bias", CH);
      const float* a1 = get(p + ".nonlinearity1.weight", 1);
      const float* a2 = get(p + ".nonlinearity2.weight", 1);
      const float* r1g = get(p + ".reg1.weight", CH);
      const float* r1b = get(p + ".reg1.bias", CH);
      const float* r2g = get(p + ".reg2.weight", HID);
      const float* r2b = get(p + ".reg2.bias", HID);
      const int ex = range_exp(xbound);
      bo.sx = std::ldexp(1.f, -ex);
      bo.w1 = pack_pointwise(pk, fold_wn(g1, v1, CH, CH), CH, CH, CH, ex);
      bo.b1 = pk.add(b1, CH);
      bo.g1 = pk.add(r1g, CH);
      bo.be1 = pk.add(r1b, CH);
      {
        // d = PReLU(dconv(GN1(h))) produced pre-scaled by 2^-ed: dconv weights and bias scaled (exact), the
        // reg2 GroupNorm eps scaled by 2^-2ed so GN2(d) is unchanged (range guard)
        std::vector<float> wd = fold_wn(gd, vd, HID, 3), bds(bd, bd + HID);
        double dbound = 0.0;
        for (int j = 0; j < HID; ++j) {
          const int k = j / 2;  // groups = CH, depth multiplier 2 (model/model.py:110-113)
          const double nb = std::fabs((double)r1g[k]) * NSIG + std::fabs((double)r1b[k]);
          const double sw = std::fabs((double)wd[3 * j]) + std::fabs((double)wd[3 * j + 1]) + std::fabs((double)wd[3 * j + 2]);
          dbound = std::max(dbound, sw * nb + std::fabs((double)bd[j]));
        }
        dbound *= std::max(1.0, std::fabs((double)a2[0]));
        const int ed = range_exp(dbound);
        for (auto& v : wd) v = std::ldexp(v, -ed);
        for (auto& v : bds) v = std::ldexp(v, -ed);
        bo.wd = pk.add(wd);
        bo.bd = pk.add(bds);
        bo.eps2 = std::ldexp(1e-8f, -2 * ed);
      }
      {
        // reg2 (GroupNorm(1, H) of d, model/model.py:136) folded out of the res_out operand: see gemm.hip
        const std::vector<float> w2 = fold_wn(g2, v2, CH, HID);
        std::vector<float> w2g((size_t)CH * HID), cb(CH), fc(CH);
        for (int m = 0; m < CH; ++m) {
          double sb = b2[m], sg = 0.0;
          for (int k = 0; k < HID; ++k) {
            const float wg = w2[(size_t)m * HID + k] * r2g[k];
            w2g[(size_t)m * HID + k] = wg;
            sg += wg;
            sb += (double)w2[(size_t)m * HID + k] * r2b[k];
          }
          cb[m] = (float)sb;
          fc[m] = (float)sg;
        }
        bo.w2 = pack_pointwise(pk, w2g, CH, HID, CH);
        bo.b2 = pk.add(cb);
        bo.fc2 = pk.add(fc);
      }
      bo.g2 = pk.add(r2g, HID);
      bo.be2 = pk.add(r2b, HID);
      bo.a1 = a1[0];
      bo.a2 = a2[0];
      const int li = i % c.layer;
      bo.dil = li == 0 ? 1 : (li % 4 + 1);
      std::vector<float> attp(20, 0.f);
      if (c.tf_attention) {
        const std::string q = "TCN.time_freq_attnetion." + std::to_string(i);
        const char* convs[4] = {".conv1d_t_1", ".conv1d_t_2", ".conv1d_f_1", ".conv1d_f_2"};
        for (int j = 0; j < 4; ++j) {
          const float* w = get(q + convs[j] + ".weight", 3);
          const float* bb = get(q + convs[j] + ".bias", 1);
          attp[4 * j + 0] = w[0]; attp[4 * j + 1] = w[1]; attp[4 * j + 2] = w[2]; attp[4 * j + 3] = bb[0];
        }
        const float* pt = get(q + ".prelu_t.weight", 1);
        const float* pf = get(q + ".prelu_f.weight", 1);
        attp[16] = pt[0]; attp[17] = pf[0];
      }
      bo.attp = pk.add(attp);
      if (c.ln_mode == SEPVAD_LN_RECURSIVE) {
        const float* fa = get("TCN.ln_first_modules." + std::to_string(i) + ".weight", CH);
        const float* fb = get("TCN.ln_first_modules." + std::to_string(i) + ".bias", CH);
        const float* sa = get("TCN.ln_second_modules." + std::to_string(i) + ".weight", CH);
        const float* sb = get("TCN.ln_second_modules." + std::to_string(i) + ".bias", CH);
        bo.lna_g = pk.add(fa, CH); bo.lna_b = pk.add(fb, CH);
        bo.lnb_g = pk.add(sa, CH); bo.lnb_b = pk.add(sb, CH);
        xbound = gn_bound(sa, sb, CH);  // next block's x' = GN_b(..)
        for (int k = 0; k < CH; ++k) {
          const double g = fa[k], e = fb[k];
          bo.wsum[0] += g; bo.wsum[1] += e; bo.wsum[2] += e * e; bo.wsum[3] += g * e; bo.wsum[4] += g * g;
        }
      } else if (c.ln_mode == SEPVAD_LN_RESIDUAL) {
        const float* fa = get("TCN.ln_modules." + std::to_string(i) + ".weight", CH);
        const float* fb = get("TCN.ln_modules." + std::to_string(i) + ".bias", CH);
        bo.lna_g = pk.add(fa, CH); bo.lna_b = pk.add(fb, CH);
        xbound += gn_bound(fa, fb, CH);  // next block's x' = o + GN_c(..)
      } else {
        xbound = 0.0;  // plain residual add: no static bound, no scale
      }
      h.blk.push_back(bo);
    }
    // output head (model/model.py:322-325); the VAD section below bounds the masks from wh, bb and head_bound
    const float* oa = get("TCN.output.0.weight", 1);
    const float* og = get("TCN.output.1.weight", CH);
    const float* ob = get("TCN.output.1.bias", CH);
    const float* gg = get("TCN.output.2.weight_g", MOUT);
    const float* vv = get("TCN.output.2.weight_v", (int64_t)MOUT * CH);
    const float* bb = get("TCN.output.2.bias", MOUT);
    const double head_bound = gn_bound(og, ob, CH);  // head A operand = GN_out(PReLU(x'))
    const std::vector<float> wh = fold_wn(gg, vv, MOUT, CH);
    h.out_a = oa[0];
    h.out_g = pk.add(og, CH);
    h.out_b = pk.add(ob, CH);
    const int eh = range_exp(head_bound);
    h.out_sx = std::ldexp(1.f, -eh);
    h.wout = pack_pointwise(pk, wh, MOUT, CH, MOUT_PAD, eh);
    std::vector<float> bpad(MOUT_PAD, 0.f);
    std::memcpy(bpad.data(), bb, MOUT * sizeof(float));
    h.bo = pk.add(bpad);
    std::vector<float> ws((size_t)MOUT_PAD * CH, 0.f), bs(MOUT_PAD, 0.f);
    for (int q = 0; q < 2; ++q)
      for (int i = 0; i < NBIN; ++i) {
        std::memcpy(&ws[((size_t)q * HEAD_SPK + i) * CH], &wh[((size_t)q * NBIN + i) * CH], CH * sizeof(float));
        bs[q * HEAD_SPK + i] = bb[q * NBIN + i];
      }
    h.wout_spk = pack_pointwise(pk, ws, MOUT_PAD, CH, MOUT_PAD, eh);
    h.bo_spk = pk.add(bs);
    std::vector<float> nyw((size_t)2 * CH), nyb(2);
    for (int q = 0; q < 2; ++q) {
      std::memcpy(&nyw[(size_t)q * CH], &wh[((size_t)q * NBIN + NBIN - 1) * CH], CH * sizeof(float));
      nyb[q] = bb[q * NBIN + NBIN - 1];
    }
    h.out_nyw = pk.add(nyw);
    h.out_nyb = pk.add(nyb);
    // VAD head (model/model.py:153-171)
    if (c.final_vad) {
      const float* g1 = get("vad.common.conv1_1.weight_g", 4);
      const float* v1 = get("vad.common.conv1_1.weight_v", (int64_t)4 * NBIN * 5);
      const float* b1 = get("vad.common.conv1_1.bias", 4);
      const float* a = get("vad.common.relu_1.weight", 1);
      const float* vg = get("vad.common.BN_1.weight", 4);
      const float* vb = get("vad.common.BN_1.bias", 4);
      const float* g2 = get("vad.output_layer_vad.weight_g", 1);
      const float* v2 = get("vad.output_layer_vad.weight_v", 12);
      const float* b2 = get("vad.output_layer_vad.bias", 1);
      const std::vector<float> w1 = fold_wn(g1, v1, 4, NBIN * 5);  // [o][c][k]
      h.v_w1 = pk.add(w1);
      std::vector<float> wv((size_t)32 * HEAD_SPK, 0.f);  // [4 k + o][speaker-local channel c]
      for (int o = 0; o < 4; ++o)
        for (int c2 = 0; c2 < NBIN; ++c2)
          for (int k = 0; k < 5; ++k) wv[(size_t)(4 * k + o) * HEAD_SPK + c2] = w1[((size_t)o * NBIN + c2) * 5 + k];
      // range guard of the VAD GEMM's A operand (the masks tile, fp16 split): |masks| <= max over rows of
      // sum_c |W| * bound(GN_out(..)) + |bias|; the tile is scaled by 2^-e on its way into the split and the
      // columns' scale carries 2^e back
      double mb = 0.0;
      for (int r = 0; r < MOUT; ++r) {
        double sr = 0.0;
        for (int i = 0; i < CH; ++i) sr += std::fabs((double)wh[(size_t)r * CH + i]);
        mb = std::max(mb, sr * head_bound + std::fabs((double)bb[r]));
      }
      const int ev_ = range_exp(mb);
      h.vad_sx = std::ldexp(1.f, -ev_);
      h.vadw = pack_pointwise(pk, wv, HEAD_VAD_N, HEAD_SPK, 32, ev_);
      std::vector<float> vny(HEAD_VAD_N);
      for (int o = 0; o < 4; ++o)
        for (int k = 0; k < 5; ++k) vny[4 * k + o] = w1[((size_t)o * NBIN + NBIN - 1) * 5 + k];
      h.vad_ny = pk.add(vny);
      h.v_b1 = pk.add(b1, 4);
      h.v_a = a[0];
      h.v_g = pk.add(vg, 4);
      h.v_b = pk.add(vb, 4);
      h.v_w2 = pk.add(fold_wn(g2, v2, 1, 12));
      h.v_b2 = b2[0];
    }
    // activity gate (model/model.py:398-400)
    std::vector<float> gw(12, 0.f);
    if (c.activity_input) {
      const float* w = get("activity_input.weight", 9);
      const float* ab = get("activity_input.bias", 1);
      const float* pa = get("prelu.weight", 1);
      std::memcpy(gw.data(), w, 9 * sizeof(float));
      gw[9] = ab[0];
      gw[10] = pa[0];
    }
    h.gate = pk.add(gw);
  } catch (const Bad& e) {
    err = e.what();
    return false;
  }
  return true;
}

// ---- The fused TCN's weight sets (tcn_kernel.h): per block, the fragment-ordered planes of conv1d and res_out ----
// One row per set: the kernel that reads it (precision, lo-plane format), the PackedW planes it is made of and where
// they go in a block: conv1d hi at 0, conv1d lo at w1l, res_out hi at w2h, res_out lo at w2l (sepvad_internal.h WF_*,
// WQ_*, WS_*; halves). Single-plane sets have no lo plane (w1l == w2h, w2l == block).
enum WSet { WSET_X3_F16 = 0, WSET_X3_E4M3 = 1, WSET_X3_I8 = 2, WSET_X3_Q16, WSET_F16, WSET_BF16, WSET_F32, NWSET };
struct WSetDef {
  int prec, lo8;         // the k_tcn instantiation that streams the set
  int cap_lo8;           // ... and the one whose co-resident capacity bounds its launches
  size_t PackedW::*hi;   // plane offsets into the fp16 blob (PREC_F32: the float blob, sizes in halves all the same)
  size_t PackedW::*lo;   // nullptr: single plane
  size_t w1l, w2h, w2l, block;
};
// WSET_X3_* are indexed by the lo-plane code (SEPVAD_WLO); WSET_X3_Q16 stands in for the int8 set at two slices: the
// int8 plane's values as fp16, streamed by the fp16-lo kernel, launched as the int8 kernel would be.
constexpr WSetDef WSETS[NWSET] = {
    {PREC_F16X3, 0, 0, &PackedW::fhi, &PackedW::flo, WF_W1L, WF_W2H, WF_W2L, WF_BLOCK},
    {PREC_F16X3, 1, 1, &PackedW::fhi, &PackedW::fl8, WQ_W1L, WQ_W2H, WQ_W2L, WQ_BLOCK},
    {PREC_F16X3, 2, 2, &PackedW::fhi, &PackedW::fi8, WQ_W1L, WQ_W2H, WQ_W2L, WQ_BLOCK},
    {PREC_F16X3, 0, 2, &PackedW::fhi, &PackedW::fq, WF_W1L, WF_W2H, WF_W2L, WF_BLOCK},
    {PREC_F16, 0, 0, &PackedW::fhi, nullptr, WS_W2, WS_W2, WS_BLOCK, WS_BLOCK},
    {PREC_BF16, 0, 0, &PackedW::fbf, nullptr, WS_W2, WS_W2, WS_BLOCK, WS_BLOCK},
    {PREC_F32, 0, 0, &PackedW::ff32, nullptr, WS32_W2, WS32_W2, WS32_BLOCK, WS32_BLOCK},
};
struct FusedBlobs {
  std::vector<__half> w[NWSET];  // [nblk][block] per weight set
  std::vector<float> prm;        // [nblk][PB_SIZE] parameter blobs
};

// Weight and parameter blobs of the fused TCN: both contiguous over blocks, so the kernel addresses block i with
// uniform arithmetic (no pointer loads).
inline FusedBlobs pack_fused(const Packed& pm, const SepVadConfig& c) {
  const Packer& pk = pm.pk;
  const std::vector<BlockOff>& blk = pm.off.blk;
  const int nblk = (int)blk.size();
  FusedBlobs fb;
  for (int k = 0; k < NWSET; ++k) {
    const WSetDef& d = WSETS[k];
    const __half* src = d.prec == PREC_F32 ? reinterpret_cast<const __half*>(pk.blob.data()) : pk.hblob.data();
    const size_t unit = d.prec == PREC_F32 ? 2 : 1;  // halves per element of the source blob
    fb.w[k].resize(d.block * nblk);
    for (int i = 0; i < nblk; ++i) {
      __half* w = fb.w[k].data() + d.block * i;
      auto put = [&](size_t at, size_t end, const PackedW& p, size_t PackedW::*plane) {
        std::memcpy(w + at, src + p.*plane * unit, (end - at) * sizeof(__half));
      };
      put(0, d.w1l, blk[i].w1, d.hi);
      put(d.w2h, d.w2l, blk[i].w2, d.hi);
      if (d.lo) {
        put(d.w1l, d.w2h, blk[i].w1, d.lo);
        put(d.w2l, d.block, blk[i].w2, d.lo);
      }
    }
  }
  fb.prm.assign((size_t)PB_SIZE * nblk, 0.f);
  const bool rec = c.ln_mode == SEPVAD_LN_RECURSIVE, res = c.ln_mode == SEPVAD_LN_RESIDUAL;
  for (int i = 0; i < nblk; ++i) {
    const BlockOff& bo = blk[i];
    float* q = fb.prm.data() + (size_t)PB_SIZE * i;
    auto put = [&](int off, size_t src, int n) { std::copy_n(pk.blob.begin() + src, n, q + off); };
    put(PB_WS1, bo.w1.scale, CH); put(PB_B1, bo.b1, CH); put(PB_G1, bo.g1, CH); put(PB_BE1, bo.be1, CH);
    put(PB_WD, bo.wd, HID * 3); put(PB_BD, bo.bd, HID);
    put(PB_WS2, bo.w2.scale, CH); put(PB_B2, bo.b2, CH); put(PB_FC2, bo.fc2, CH);
    if (rec || res) { put(PB_LNAG, bo.lna_g, CH); put(PB_LNAB, bo.lna_b, CH); }
    if (rec) { put(PB_LNBG, bo.lnb_g, CH); put(PB_LNBB, bo.lnb_b, CH); }
    put(PB_ATT, bo.attp, 20);
    q[PB_A1] = bo.a1; q[PB_A2] = bo.a2;
    q[PB_SX] = bo.sx;
    q[PB_SXN] = i + 1 < nblk ? blk[i + 1].sx : 1.f;
    q[PB_EPS2] = bo.eps2;
    {
      double sf = 0.0, sb = 0.0;  // fixed order (bitwise reproducible)
      for (int k = 0; k < CH; ++k) { sf += pk.blob[bo.fc2 + k]; sb += pk.blob[bo.b2 + k]; }
      q[PB_SFC2] = (float)sf;
      q[PB_SB2] = (float)sb;
    }
    std::memcpy(q + PB_WSUM, bo.wsum, sizeof(bo.wsum));
  }
  return fb;
}
}  // namespace sepvad
