// Stand-alone host check of csrc/scratch_plan.h and the workspace layout of csrc/handle.h (no GPU, no HIP runtime call;
// hipcc only because handle.h needs the HIP types):
//   make -C sep-tfanet-vad_amd/csrc scratch_check | scratch_check_san   (build/scratch_check[_san]; the second under
//   the address and undefined-behaviour sanitizers, by hand on a CPU machine)
// Prints "ws_bytes B N bytes" for the shapes tests/test_scratch_host.py pins, then binds the smallest workspace into a
// host allocation of exactly that size and writes every array end to end, so a sanitizer sees an array that leaves
// the block; arrays that share bytes without being an overlay exit non-zero. Ends with "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../sep-tfanet-vad_amd/csrc/handle.h"

using namespace sepvad;

static void require(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "scratch_check: %s\n", what);
    std::exit(1);
  }
}

int main() {
  const long long shapes[][2] = {{1, 257}, {3, 8292}, {64, 32000}, {1, 2100000}};
  for (const auto& s : shapes) {
    const int B = (int)s[0], N = (int)s[1], Tp = round_up(1 + N / HOP, TILE);  // as ws_reserve
    std::printf("ws_bytes %d %d %zu\n", B, N, ws_bytes(B, Tp));
  }
  // the planner's rules on a toy list: 256-byte starts, slack, an empty array, an overlay, a second phase
  {
    ScratchPlan p;
    float* a = nullptr; double* b = nullptr; int* c = nullptr; char* d = nullptr;
    p.take(a, 1); p.take(b, 0); p.overlay(c); p.take(d, 250, 16); p.rewind(); p.take(c, 129);
    require(p.bytes() == 768 && p.off == 768 && !a && !b && !c && !d, "size pass");
    alignas(256) static char buf[768];
    ScratchPlan q(buf);
    q.take(a, 1); q.take(b, 0); q.overlay(c); q.take(d, 250, 16); q.rewind(); q.take(c, 129);
    require((char*)a == buf && (char*)b == buf + 256 && d == buf + 256 && (char*)c == buf && q.bytes() == 768, "bind pass");
    ScratchPlan e(buf, 8);
    q = e;
    q.take(b, 3); q.take(a, 0); q.take(b, 1);
    require((char*)b == buf + 24 && q.bytes() == 32, "alignment 8");
  }
  // the smallest workspace, bound and written end to end
  const int B = 2, Tp = 64;
  const size_t bytes = ws_bytes(B, Tp);
  char* base = (char*)std::malloc(bytes);
  require(base != nullptr, "malloc");
  Workspace w{};
  require(ws_plan(w, base, B, Tp) == bytes, "the bind pass disagrees with the size pass");
  std::vector<std::pair<char*, char*>> spans;
  ws_each(w, [&](auto*& p, const WsDim& d) {
    char* lo = (char*)p;
    char* hi = lo + d.elems(B, Tp) * sizeof(*p) + d.slack;
    require(lo >= base && (size_t)(lo - base) % 256 == 0, "an array off its 256-byte boundary");
    std::memset(lo, 0x5a, (size_t)(hi - lo));
    if (!d.overlay) spans.emplace_back(lo, hi);
  });
  for (size_t i = 1; i < spans.size(); ++i) require(spans[i - 1].second <= spans[i].first, "two arrays share bytes");
  require(spans.back().second <= base + bytes, "the last array leaves the block");
  require((char*)w.D32 == (char*)w.Dhi, "D32 overlays Dhi");
  std::free(base);
  std::printf("ok\n");
  return 0;
}
