// warm_plan_check.cpp — stand-alone host program of tests/test_warm_plan_sanitized.py: the warm
// plan of the one-row fused launch (csrc/lm_kernels.h wgemm_warm_plan / warm_walk) swept under
// the address and undefined-behaviour sanitizers.
//
// Reads cases from stdin, one per line:
//   N K num_cu stages warm_workgroups shift
// For each it takes the library's own gate/up plan (plan_wgemm, one row, SwiGLU), derives the
// warm plan and walks every warm workgroup's blocks as the kernel does, marking each KiB of the
// tiled matrix in a map that is exactly the matrix long (an offset past the end is a sanitizer
// report, not a silent miss).  Checks: every block inside the matrix, no KiB read twice, the
// marked KiB are exactly stages 0 .. stages-1 of every gate/up workgroup's first units, and
// gate/up block g of warm workgroup b has g mod 8 == (b + shift) mod 8.
// Prints one line per case and "OK <cases> <blocks walked>"; exit 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "lm_kernels.h"

using namespace tts;

int main() {
  int N, K, ncu, W, wgs, shift, cases = 0;
  unsigned long long blocks = 0;
  while (scanf("%d %d %d %d %d %d", &N, &K, &ncu, &W, &wgs, &shift) == 6) {
    const WgemmPlan p = plan_wgemm(1, N, K, EPI_SWIGLU, ncu);
    WarmArgs a;
    try {
      a = wgemm_warm_plan(p, nullptr, N, K, W, wgs, shift);
    } catch (const std::exception& e) {
      if (wgs > 0 && wgs < kWarmXcds) {
        printf("N %d K %d wgs %d refused: %s\n", N, K, wgs, e.what());
        ++cases;
        continue;
      }
      printf("FAIL N %d K %d: %s\n", N, K, e.what());
      return 1;
    }
    const size_t kib = (size_t)(N / 16) * (K / 32);
    if ((size_t)a.bytes != kib * 1024) { printf("FAIL bytes %u\n", a.bytes); return 1; }
    std::vector<uint8_t> seen(kib, 0);
    bool ok = true;
    for (int b = 0; b < a.wgs && ok; ++b)
      warm_walk(a, b, [&](uint32_t off, uint32_t len, int g, int st) {
        ++blocks;
        if (off % 1024 || len % 1024 || len == 0 || (unsigned long long)off + len > a.bytes) ok = false;
        if (g < 0 || g >= a.nblk || st < 0 || st >= a.stages || ((g - b - shift) % 8 + 8) % 8 != 0) ok = false;
        if (!ok) return;
        for (uint32_t q = off / 1024; q < (off + len) / 1024; ++q) {
          if (seen[q]) ok = false;
          seen[q] = 1;
        }
      });
    // expected: stage st, gate/up workgroup g of the first round (nr units, upw a workgroup)
    const StreamPlan& s = p.sp;
    const int upw = s.waves / s.ksplit, units = (N / 16) / s.ng, ur = s.ur(), nr = ur < units ? ur : units;
    const size_t T = (size_t)s.ksplit * s.ng * s.ku;  // KiB of one unit's stage
    std::vector<uint8_t> want(kib, 0);
    for (int st = 0; st < a.stages; ++st)
      for (int u = 0; u < nr; ++u)
        for (size_t q = 0; q < T; ++q) want[((size_t)st * nr + u) * T + q] = 1;
    if (a.nblk != (nr + upw - 1) / upw) ok = false;
    if (ok && seen != want) ok = false;
    printf("%s N %d K %d cu %d: stages %d (asked %d) wgs %d shift %d, %d gate/up workgroups, block %u B, last %u B\n",
           ok ? "ok  " : "FAIL", N, K, ncu, a.stages, W, a.wgs, a.shift, a.nblk, a.blk_bytes, a.last_bytes);
    if (!ok) return 1;
    ++cases;
  }
  printf("OK %d %llu\n", cases, blocks);
  return 0;
}
