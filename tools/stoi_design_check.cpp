// Stand-alone host check of csrc/stoi_design.h (no GPU, no HIP), meant for a sanitizer build:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/stoi_design_check.cpp -o /tmp/stoi_design_check && /tmp/stoi_design_check
// Runs the filter design, the polyphase table, the band edges, the window and twiddle tables for every rate and
// the frame-count arithmetic over a range of lengths; exits non-zero on an inconsistent result.
#include <cstdio>
#include <cstdlib>

#include "../sep-tfanet-vad_amd/csrc/stoi_design.h"

using namespace sepvad;

static void require(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "stoi_design_check: %s\n", what);
    std::exit(1);
  }
}

int main() {
  const int rates[] = {16000, 8000, 10000};
  const int want_taps[] = {581, 365, 0};
  for (int i = 0; i < 3; ++i) {
    StoiDesign d;
    require(stoi_design(rates[i], d), "supported rate refused");
    require((int)d.w.size() == want_taps[i], "tap count");
    double sum = 0.0;
    for (double v : d.w) sum += v;
    require(d.w.empty() || std::fabs(sum - 1.0) < 1e-12, "taps do not sum to one");
    for (size_t k = 0; k < d.w.size(); ++k) require(d.w[k] == d.w[d.w.size() - 1 - k], "taps not symmetric");
    std::vector<double> tp;
    const int Q = d.w.empty() ? 0 : stoi_polyphase(d, tp);
    double psum = 0.0;
    for (double v : tp) psum += v;
    require(d.w.empty() || std::fabs(psum - d.up) < 1e-12, "polyphase table does not sum to up");
    require(d.lo[0] == 7 && d.hi[0] == 9 && d.lo[14] == 174 && d.hi[14] == 219, "band edges");
    for (int b = 1; b < STOI_BANDS; ++b) require(d.lo[b] == d.hi[b - 1], "bands not contiguous");
    for (long long N = 1; N < 3000; N += 7) {
      const long long L = stoi_resampled_len(N, d.up, d.down);
      const long long nF = stoi_num_frames(L);
      require(nF == 0 || (nF - 1) * STOI_HOP + STOI_FRAME < L + 0, "last frame leaves the signal");
      require(nF == 0 || nF * STOI_HOP + STOI_FRAME >= L, "a frame is missing");
    }
    std::printf("fs %d: up %d down %d taps %zu Q %d\n", rates[i], d.up, d.down, d.w.size(), Q);
  }
  StoiDesign d;
  require(!stoi_design(44100, d) && !stoi_design(0, d), "unsupported rate accepted");
  double w[STOI_FRAME], tw[STOI_NFFT];
  stoi_window(w);
  stoi_twiddles(tw);
  require(w[0] > 0.0 && std::fabs(w[127] - w[128]) < 1e-15 && tw[0] == 1.0 && tw[1] == 0.0, "window / twiddles");
  std::printf("ok\n");
  return 0;
}
