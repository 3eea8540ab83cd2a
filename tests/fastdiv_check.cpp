// fastdiv_check.cpp — stand-alone host program of tests/test_fastdiv.py: the multiply-high
// pairs the decode GEMM launches with (csrc/fastdiv.h, wgemm_derive) against plain division.
//
// Reads launches from stdin, one per line:
//   M N K epi KVH H D fo_N fo_K
// (KVH > 0: the QKV launch carrying the decode attention, with an o_proj of fo_N x fo_K
// behind it when fo_N > 0).  For each it takes the library's own plan (plan_wgemm), fills the
// launch fields as launch_wgemm does, derives the pairs with wgemm_derive and checks
// fastdiv(n) == n / d for EVERY n from 0 to the bound the pair was made for, which must cover the
// largest dividend the kernel can form (asserted here from the kernel's index ranges).
// Then the refusals: pairs that cannot be exact are rejected, and a pair used beyond its bound
// is reported inexact where a brute-force search does find a wrong quotient.
// Prints one line per launch and "OK <launches> <divisions checked>"; exit 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "fastdiv.h"
#include "lm_kernels.h"

using namespace tts;

static unsigned long long g_checked = 0;

static bool sweep(const char* what, FastDiv f, uint32_t d, uint32_t nmax, bool gt1) {
  if (!fastdiv_exact(f, d, nmax)) {
    printf("FAIL %s: pair {%u, %u} not exact for d %u on 0..%u by the host's own condition\n", what, f.mul, f.shift, d, nmax);
    return false;
  }
  for (uint32_t n = 0;; ++n) {
    if (fastdiv(n, f) != n / d || (gt1 && fastdiv_gt1(n, f) != n / d)) {
      printf("FAIL %s: d %u n %u: %u != %u\n", what, d, n, fastdiv(n, f), n / d);
      return false;
    }
    ++g_checked;
    if (n == nmax) break;
  }
  return true;
}

// first n <= nmax with a wrong quotient, or -1
static long long first_wrong(FastDiv f, uint32_t d, uint32_t nmax) {
  for (uint32_t n = 0;; ++n) {
    if (fastdiv(n, f) != n / d) return n;
    if (n == nmax) break;
  }
  return -1;
}

int main() {
  const int num_cu = 256;
  int M, N, K, epi, KVH, H, D, foN, foK, launches = 0;
  bool ok = true;
  while (scanf("%d %d %d %d %d %d %d %d %d", &M, &N, &K, &epi, &KVH, &H, &D, &foN, &foK) == 9) {
    WgemmPlan p = plan_wgemm(M, N, K, epi, num_cu);
    WgemmArgs a;
    a.M = M; a.K = K; a.ldx = K; a.N = N;
    if (KVH > 0) {  // (launch_wgemm: the fused launch keeps whole units)
      if (p.sliced || !p.a_lds) continue;
      p.csplit = 1;
      p.grid = p.sp.grid;
      a.fattn_wgs = M * KVH;
      a.fa.KVH = KVH; a.fa.H = H; a.fa.D = D;
      if (foN > 0) {
        const WgemmPlan po = plan_wgemm(M, foN, foK, EPI_RESID, num_cu);
        a.fo_units = foN / 16; a.fo_ur = po.sp.ur(); a.fo_kc = po.sp.kc;
        if (M > 1 && ((foK / 32) % (a.fo_kc * p.sp.ksplit * p.sp.ku) != 0)) a.fo_units = 0;
      }
    }
    a.ur = p.sp.ur(); a.kc = p.sp.kc; a.sliced = p.sliced ? 1 : 0; a.csplit = p.csplit;
    if (p.sliced) a.K = K / p.sp.kc;
    wgemm_derive(a, p.sp.ku, p.sp.ng, p.sp.ksplit, p.sp.ksplit, p.grid, p.a_lds);
    ++launches;
    // the kernel's dividends (wgemm_kernel): unit index >> csplit < layout units <= N / 8;
    // A chunk c < M * kch <= 64 * K / 8, LDS-DMA piece p * 64 < M * kch; stage < kc * Sc;
    // fused attention workgroup < M * KVH; fused o_proj stage < its item's stages
    const uint32_t kch = (uint32_t)a.K / 8, bunits = (uint32_t)a.units >> (a.csplit == 2 ? 1 : 0);
    if (bunits > (uint32_t)N / 8 || (uint32_t)M * kch > 64u * (uint32_t)K / 8) { printf("FAIL bounds\n"); ok = false; }
    ok = sweep("ur", a.ur_div, (uint32_t)a.ur, bunits, false) && ok;
    if (p.a_lds) ok = sweep("kch", a.kch_div, kch, (uint32_t)M * kch, true) && ok;  // (A from global memory: no such division)
    ok = sweep("Sc", a.sc_div, (uint32_t)a.Sc, (uint32_t)(a.kc * a.Sc), false) && ok;
    if (a.fattn_wgs) ok = sweep("KVH", a.kvh_div, (uint32_t)KVH, (uint32_t)a.fattn_wgs, false) && ok;
    if (a.fo_Sc) ok = sweep("fo_Sc", a.fo_sc_div, (uint32_t)a.fo_Sc, (uint32_t)(foK / 32 / (p.sp.ksplit * p.sp.ku)), false) && ok;
    printf("launch M %d N %d K %d epi %d%s: ur %d kch %u Sc %d kc %d csplit %d sliced %d%s\n", M, N, K, epi,
           KVH > 0 ? " fused" : "", a.ur, kch, a.Sc, a.kc, a.csplit, a.sliced, a.fo_Sc ? " fo_Sc" : "");
  }

  // ---- refusals
  FastDiv f;
  // no 32-bit pair divides every 32-bit dividend by 7 (the exact multiplier has 33 bits)
  if (fastdiv_make(7, 0xFFFFFFFFu, &f)) { printf("FAIL: 7 over the whole 32-bit range accepted\n"); ok = false; }
  if (fastdiv_make(0, 10, &f)) { printf("FAIL: divisor 0 accepted\n"); ok = false; }
  // TTS-1-Max down's kch: the pair for a small bound, used beyond it, is refused by the host's
  // condition, and indeed wrong somewhere below the larger bound
  const uint32_t d = 1792, big = 0xFFFFFFFFu;
  if (!fastdiv_make(d, 64 * d, &f)) { printf("FAIL: 1792 on 0..64*1792 refused\n"); ok = false; }
  ok = sweep("1792", f, d, 64 * d, true) && ok;
  if (fastdiv_exact(f, d, big)) { printf("FAIL: pair {%u, %u} of the small bound passes for the whole range\n", f.mul, f.shift); ok = false; }
  const long long w = first_wrong(f, d, big);
  if (w < 0) { printf("FAIL: refused pair has no wrong quotient\n"); ok = false; }
  else printf("refused: pair {%u, %u} for d 1792 is wrong first at n = %lld\n", f.mul, f.shift, w);
  // a pair with the wrong multiplier for its divisor, and one for another divisor
  if (fastdiv_exact(FastDiv{f.mul - 1, f.shift}, d, 1000) || fastdiv_exact(f, d + 1, 64 * d)) {
    printf("FAIL: a wrong pair passes\n");
    ok = false;
  }
  // d == 1 and powers of two
  ok = fastdiv_make(1, big, &f) && sweep("1", f, 1, 1 << 20, false) && ok;
  ok = fastdiv_make(64, big, &f) && sweep("64", f, 64, 1 << 22, true) && ok;
  if (!ok) return 1;
  printf("OK %d %llu\n", launches, g_checked);
  return 0;
}
