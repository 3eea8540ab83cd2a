// lm_kernels.h — host-side declarations of the SpeechLM kernels (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "fastdiv.h"

namespace tts {

// Dry run (tts_debug_step_plan): while a recorder is set on this thread, the SpeechLM
// launchers append what they would launch — the wgemm_kernel template arguments, other
// kernels by name — and return without any HIP call, so a decode step's launch list can be
// read on a machine without a GPU (the spill gate, tests/test_kernel_resources.py).
std::vector<std::string>*& dry_launches();
inline bool dry_record(const std::string& what) {
  std::vector<std::string>* v = dry_launches();
  if (!v) return false;
  v->push_back(what);
  return true;
}

typedef uint16_t bf16_t;

// EPI_LOGITS_ROWS: EPI_LOGITS with the penalties read per row (WgemmArgs::row_par)
enum { EPI_STORE = 0, EPI_RESID = 1, EPI_SWIGLU = 2, EPI_LOGITS = 3, EPI_LOGITS_ROWS = 4 };

// One decode row's sampling settings (the per-request slot batch: LmWork::row_par [cap_batch]).
// The per-row kernels of the captured step read these from device memory where the uniform ones
// take launch arguments, so a request with other settings needs no recapture.  Every entry always
// holds valid values (idle rows are computed too): penalty > 0, 1 <= top_k (a greedy row: 1).
struct RowParams {
  float penalty, freq_penalty, temperature, top_p;
  int top_k, eos_id, min_new, sample;
};
static_assert(sizeof(RowParams) == 32, "RowParams is 32 bytes");

// Weight layout + decode launch decomposition of one tiled matrix ("stream plan").
// Work item = (unit of NG n-tiles, K part of KT/ksplit k-tiles); a wave streams its item
// in stages of ku k-tiles.  Units run in rounds of ur() = grid * waves/ksplit (one unit
// per wave group of every workgroup).  Tiles are stored round-major, then STAGE-major:
// at stage s every wave of the launch reads one contiguous block (ur*ksplit*NG*ku KiB),
// the access pattern that streams HBM fastest (scripts/hbm_floor.hip, pipe sweep).
// K is cut into kc chunks of KT/kc k-tiles (chunk-major): a wave's K part is split evenly
// over the chunks, so a launch may also run one chunk per workgroup (grid.y = chunk,
// "K-sliced": the A operand of one chunk fits LDS at batch 17..32; fp32 partials combined
// by a second kernel).
struct StreamPlan {
  int ng = 1, ksplit = 1, ku = 8, waves = 4, grid = 1, kc = 1;
  __host__ __device__ int ur() const { return grid * (waves / ksplit); }
};
// Tile index (1 KiB units) of n-tile nt (unit nt/ng, member nt%ng), k-tile kt.
__host__ __device__ inline long long plan_tile(int ng, int ksplit, int ku, int ur, int units, int KT,
                                               int kc, int nt, int kt) {
  const int u = nt / ng, g = nt - u * ng;
  const int KTc = KT / kc, kt_pc = KTc / ksplit;
  const int c = kt / KTc, rr = kt - c * KTc;
  const int kp = rr / kt_pc, ki = rr - kp * kt_pc;
  const int st = c * (kt_pc / ku) + ki / ku, kk = ki % ku;
  const int r = u / ur, ui = u - r * ur;
  const int nr = (units - r * ur) < ur ? (units - r * ur) : ur;
  return (long long)r * ur * KT * ng +
         (((long long)st * nr * ksplit + (long long)ui * ksplit + kp) * ng + g) * ku + kk;
}
// First tile of stage st of k-part kpart of the unit at place ui of layout round r (nr units in
// that round): the one formula of the stage-major order, read by the decode kernel's weight
// stream (wgemm_kernel: stile / soff) and by the host's warm plan (wgemm_warm_plan)
__host__ __device__ inline long long wgemm_stage_tile(int r, int ui, int nr, int st, int kpart, int ur, int KT,
                                                      int ng, int ksplit, int ku) {
  return (long long)r * ur * KT * ng + (((long long)st * nr + ui) * ksplit + kpart) * ng * ku;
}
StreamPlan stream_plan(int N, int K, int ng, int num_cu);
constexpr int LOGITS_MAX_PARTS = 1024;  // lm_head workgroups = argmax partials per row

struct AttnArgs {
  const bf16_t* qkv = nullptr;  // [rows][ld_qkv]: q (H*D) | k (KVH*D) | v (KVH*D)
  int ld_qkv = 0;
  int rows = 0;
  const int* row_slot = nullptr;  // KV slot (sequence) of each query row
  const int* row_pos = nullptr;   // absolute position of each query row
  bf16_t* kcache = nullptr;       // this layer's K rows: [slots][KVH][max_seq][D]
  bf16_t* vtcache = nullptr;      // this layer's V^T: [slots][KVH] blocks of D x max_seq in 16 x 32 tiles (vt_off)
  int max_seq = 0;                // position stride of the cache (a multiple of 64)
  const bf16_t* rope_cos = nullptr;  // [max_seq][D]
  const bf16_t* rope_sin = nullptr;
  int H = 0, KVH = 0, D = 0;
  float scale = 0.f;
  bf16_t* q_rot = nullptr;  // prefill: roped q [rows][H*D]
  bf16_t* out = nullptr;    // [rows][H*D] bf16 attention output
  const int4* blocks = nullptr;  // prefill: query blocks {first row, rows (<= 16), slot, first position}
  int nblocks = 0;
  unsigned long long* stamps = nullptr;  // diagnostic build only (TTS_STAMPS)
  // decode: q | k | v as fp32 partials of a K-sliced QKV launch ([qkv_nsl][rows][ld_qkv], summed
  // in slice order and rounded to bf16 here, as splitk_combine_kernel would) instead of qkv
  const float* qkv_part = nullptr;
  int qkv_nsl = 0;
};

// ---- sampling / bookkeeping state of a decode step (lm_ops.hip, lm_finalize.h)
struct StepState {
  int* tokens;        // [B] token fed to the next step
  int* pos;           // [B] position of the next token (= current length)
  int* gen_count;     // [B] tokens generated so far
  int* limit;         // [B] max new tokens
  int* done;          // [B]
  int* eos_mask;      // [B] eos id while gen_count < min_new, else -1
  uint32_t* seen;     // [B][seen_stride]
  int seen_stride;
  int* out_ids;       // [B][out_stride]
  int out_stride;
  int* n_active;      // [1]
  uint16_t* counts;   // [B][V] new-token counts (frequency penalty) or nullptr
  unsigned long long* row_seed;  // [B] sampling key of each row
  uint32_t* epoch;    // [1] step counter (+1 by the finalize of every step: the screened head's keys)
  int eos_id;
  int min_new;
  const RowParams* par = nullptr;  // [B] per-row eos_id / min_new (and the kernels' settings), or nullptr: the scalars
};

// Largest tiled weight matrix a wgemm launch streams: one buffer resource with 32-bit byte
// offsets, and the past-the-last-unit sentinel offsets (wgemm_kernel: kWgemmSentinel - the
// stage's tile offsets, at most 15 KiB below it) must stay beyond the matrix
constexpr unsigned long long kWgemmMaxBytes = 0xFFFF0000ull;
constexpr uint32_t kWgemmSentinel = 0xFFFFFFF0u;

// ---- the warm role of the one-row fused QKV + attention + o_proj launch
// Workgroups appended behind the o_proj ones start when the projection workgroups retire, i.e.
// in the window in which only the attention chain runs and HBM idles.  They read the first
// stages of this layer's gate/up stream with the default cache policy and exit: the lines stay
// in the L2 of their XCD, where the gate/up workgroups of the next launch that land on the same
// XCD find them.  They write nothing and wait on nothing; a wrong placement guess costs speed only.
//
// One gate/up workgroup's stage is one contiguous block of the stage-major layout (blk_bytes;
// the last workgroup's may be shorter), a stage stage_bytes after the one before.  Blocks are
// dealt round-robin over the 8 XCDs, so warm workgroup b takes the class c = (b + shift) mod 8
// of gate/up blocks (g mod 8 == c), shares it with the other warm workgroups of the class, and
// they deal its (stage, block) pairs among themselves, stage 0 first.
struct WarmArgs {
  const bf16_t* w = nullptr;  // the layer's tiled gate/up matrix
  uint32_t bytes = 0;         // its size: the range of the buffer resource the reads go through
  int wgs = 0;                // warm workgroups (0: no warm role)
  int stages = 0;             // stages 0 .. stages-1 of every gate/up workgroup
  int nblk = 0;               // gate/up workgroups (those with a unit)
  uint32_t blk_bytes = 0, last_bytes = 0, stage_bytes = 0;
  int shift = 0;
};
constexpr int kWarmXcds = 8;
constexpr uint32_t kWarmMaxBytesPerXcd = 3u << 20;  // of an XCD's 4 MiB of L2
// f(byte offset, bytes, gate/up block, stage) for every block warm workgroup b reads
template <typename F>
__host__ __device__ inline void warm_walk(const WarmArgs& a, int b, F f) {
  const int c = (b + a.shift) & (kWarmXcds - 1);
  const int nw = (a.wgs - (b & (kWarmXcds - 1)) + kWarmXcds - 1) / kWarmXcds;  // warm workgroups of the class
  const int nb = c < a.nblk ? (a.nblk - c + kWarmXcds - 1) / kWarmXcds : 0;    // gate/up blocks of the class
  if (nb == 0 || nw <= 0) return;
  int st = 0, i = b / kWarmXcds;
  for (;;) {
    while (i >= nb && st < a.stages) { i -= nb; ++st; }
    if (st >= a.stages) return;
    const int g = c + kWarmXcds * i;
    f((uint32_t)st * a.stage_bytes + (uint32_t)g * a.blk_bytes, g == a.nblk - 1 ? a.last_bytes : a.blk_bytes, g, st);
    i += nw;
  }
}

// Kernel-argument layout.  Everything a projection workgroup reads before its first weight load
// sits in the first two 64-byte lines (the struct is 64-byte aligned, so is the kernel-argument
// segment): the kernel fetches those two lines in one batch at its very top, ahead of the role
// branch of the fused launch, and waits once.  Quotients of launch constants are computed by the
// host (wgemm_derive below) and divisions by them in the kernel are multiply-high
// pairs (fastdiv.h): the kernel holds no integer division.  Fields are ordered by when the
// kernel needs them, NOT kept at stable offsets: a field added or moved here changes the
// compiled code of every instantiation, deliberately (re-run tests/test_wgemm_prologue_isa.py).
struct alignas(64) WgemmArgs {
  // ---- line 0
  const bf16_t* x = nullptr;  // A: [M][ldx] bf16 activations
  const bf16_t* w = nullptr;  // B: tiled weights (see lm_gemm.hip)
  const bf16_t* normw = nullptr;  // RMSNorm weight [K] (NORM prologue)
  bf16_t* resid = nullptr;  // EPI_RESID: residual stream, updated in place (read ahead of the weight stream)
  unsigned long long* stamps = nullptr;  // diagnostic build only (TTS_STAMPS): [block][32]
  int M = 0, K = 0, ldx = 0;
  int N = 0;
  int ldo = 0;
  int ur = 0;         // layout: units per round (StreamPlan::ur, filled in by launch_wgemm)
  // ---- line 1
  int fattn_wgs = 0;  // attention workgroups appended to the grid (0: not fused), see below
  int fo_units = 0;   // o_proj workgroups appended behind them, see below
  int csplit = 1;     // 2: each 16-column unit runs as two 8-column halves (twice the workgroups; filled in by launch_wgemm)
  int sliced = 0;     // 1: grid.y = K chunk, K = one chunk, ldx = full K (filled in by launch_wgemm)
  int diag = 0;       // timing diagnostics only (TTS_WGEMM_DIAG): 1 no prologue, 2 no epilogue, 8 barrier before the stream, 64 per-wave norm-end stamps
  // derived by the host for the instantiation that runs (wgemm_derive; callers leave them):
  int KT = 0;         // k-tiles of the whole matrix
  int Sc = 0;         // stages of a wave's K part in one K chunk (its k-tiles there: Sc * KU)
  int S = 0;          // stages per item in this launch
  int units = 0;      // work units ((N / 16 / NG) << (csplit == 2))
  int nproj = 0;      // projection workgroups (grid.x without the fused launch's attention / o_proj ones)
  FastDiv ur_div;     // / ur, dividends < layout units
  FastDiv kch_div;    // / (K / 8), dividends <= M * K / 8
  FastDiv sc_div;     // / Sc, dividends < stages of the whole K
  // ---- needed behind the primed weight stages only
  float eps = 0.f;
  bf16_t* out = nullptr;  // [M][ldo]
  int kc = 1;         // layout: K chunks (StreamPlan::kc, filled in by launch_wgemm)
  // EPI_LOGITS
  const uint32_t* seen = nullptr;  // [M][seen_stride] bitmap of ids present in the sequence
  int seen_stride = 0;
  float penalty = 1.f;
  const int* eos_mask = nullptr;  // [M] token id forced to -inf (or -1)
  float* part_val = nullptr;      // [M][part_stride]
  int* part_idx = nullptr;
  int part_stride = 0;
  float* logits_out = nullptr;  // EPI_LOGITS: also store the processed fp32 logits [M][ldl] (sampling)
  const uint16_t* counts = nullptr;  // EPI_LOGITS: new-token counts [M][seen_stride*32] (frequency penalty)
  float freq_penalty = 0.f;
  int ldl = 0;
  const RowParams* row_par = nullptr;  // EPI_LOGITS_ROWS: [M] penalty / freq_penalty of each row (counts always set)
  float* part_out = nullptr;  // K-sliced launches: fp32 partials [kc][M][ldo] (caller's workspace)
  const bf16_t* next_norm = nullptr;  // K-sliced residual launches: RMSNorm the updated rows
  bf16_t* norm_out = nullptr;         //   with next_norm (eps) into norm_out [M][ldo]
  // QKV launch with the decode attention fused in (decode, one row): the projection's
  // workgroups publish q/k/v as data-tagged 8-byte granules {bf16 pair, tag} with
  // agent-scope stores; fattn_wgs extra workgroups (blockIdx.x >= the GEMM grid), one per kv
  // head, load their K / V^T fragments, wait for their q (and the new k/v) granules and
  // attend exactly as attn_decode_kernel does.  tag = (pos << 6) | layer differs between any
  // two consecutive launches, so a granule left by the previous launch never matches.
  uint64_t* gran = nullptr;   // [M][N / 2] q|k|v granules, then (fo_units) [M][H*D / 2] attention rows
  AttnArgs fa;                // the attention of this layer (its output row: fa.out)
  FastDiv kvh_div;            // / fa.KVH, dividends < fattn_wgs (wgemm_derive)
  int fattn_layer = 0;
  // grid order: the projection workgroups, then the attention workgroups, then (fo_units > 0)
  // one o_proj workgroup per o_proj unit: every workgroup waits only on blocks of lower index,
  // and blocks are dispatched in index order, so the launch completes whatever else occupies
  // the GPU (no co-residency needed); the warm workgroups (warm, below) come last and wait on nothing
  int* fattn_err = nullptr;   // set to 1 if a granule wait timed out; later waits then give up at once
  int fattn_spins = 1 << 16;  // polls (s_sleep 1 each, ~0.1 s in all) before a wait gives up
  // o_proj fused behind the attention (fo_units > 0): the attention workgroups also publish
  // the bf16 attention row as granules (gran + N/2, same tag); o_proj unit b (tiled weights
  // fo_w, layout rounds fo_ur, one round) runs on the grid's b-th o_proj workgroup, with the
  // residual epilogue on fo_resid (the hidden row), its o_proj weights loaded while the
  // attention runs
  // (2..16 rows: the attention rows' granules at gran + M*N/2, row m's H*D/2 at m*H*D/2;
  // o_proj's layout K chunks fo_kc; fo_resid holds the M hidden rows)
  const bf16_t* fo_w = nullptr;
  int fo_ur = 0, fo_kc = 1;
  int fo_Sc = 0;              // (2..16 rows) stages of an o_proj wave's K part in one chunk (wgemm_derive)
  FastDiv fo_sc_div;          // / fo_Sc, dividends < the o_proj item's stages
  bf16_t* fo_resid = nullptr;
  int ring = 0;  // (host only) 4: the four-stage ring for the one-row gate/up launch (launch_shape; WgemmPlan::ring)
  // the warm role (one row, o_proj riding): warm.wgs workgroups behind the o_proj ones read the first
  // stages of the layer's gate/up stream into their XCD's L2 (WarmArgs).  Last in the struct: no
  // other role's fetch touches these lines
  WarmArgs warm;
};
static_assert(offsetof(WgemmArgs, eps) == 128, "WgemmArgs: the prologue's fields fill the first two 64-byte lines");
static_assert(offsetof(WgemmArgs, x) == 0 && offsetof(WgemmArgs, w) == 8, "WgemmArgs: x, w lead (tests/test_wgemm_prologue_isa.py)");
static_assert(offsetof(WgemmArgs, fattn_wgs) == 64, "WgemmArgs: line 1 starts at the role split");

// The launch constants the kernel would otherwise divide for (WgemmArgs: "derived by the
// host"), for the instantiation (KU, NG, KSPLIT, KSW) that runs on `nproj` projection
// workgroups: the quotients themselves, and the multiply-high pairs of the divisions whose
// dividend is per workgroup, thread or stage, each made for the largest dividend the kernel
// forms and refused (an error, never a wrong quotient) when no exact pair exists.
// a_lds: the A rows are staged in LDS (only those prologues divide by K / 8).
inline void wgemm_derive(WgemmArgs& a, int ku, int ng, int ksplit, int ksw, int nproj, bool a_lds) {
  const int sl = ksplit / ksw;  // K slices over workgroups of the kc = 1 layouts
  const int kc = a.kc;
  a.KT = a.sliced ? (a.K >> 5) * kc : (a.K >> 5) * sl;
  const int KTc = a.KT / kc, kt_pc = KTc / ksplit;
  a.Sc = kt_pc / ku;
  if (a.ur < 1 || a.Sc < 1 || a.Sc * ku * ksplit * kc != a.KT)
    throw std::runtime_error("wgemm: K does not divide into the plan's stages");
  if (a.csplit != 1 && a.csplit != 2) throw std::runtime_error("wgemm: csplit is 1 or 2");
  a.S = a.sliced ? a.Sc : kc * a.Sc;
  const int bunits = (a.N >> 4) / ng;
  a.units = bunits << (a.csplit == 2 ? 1 : 0);
  a.nproj = nproj;
  const uint32_t kch = (uint32_t)a.K >> 3;
  bool ok = fastdiv_make((uint32_t)a.ur, (uint32_t)bunits, &a.ur_div);  // uu >> cs2 < bunits
  a.kch_div = FastDiv{};
  if (a_lds)  // chunk c < M * kch; piece p * 64 < M * kch (fastdiv_gt1: kch > 1)
    ok = kch > 1 && fastdiv_make(kch, (uint32_t)a.M * kch, &a.kch_div) && ok;
  ok = fastdiv_make((uint32_t)a.Sc, (uint32_t)(kc * a.Sc), &a.sc_div) && ok;  // stage sg < kc * Sc
  if (a.fattn_wgs) {
    ok = a.fa.KVH > 0 && fastdiv_make((uint32_t)a.fa.KVH, (uint32_t)a.fattn_wgs, &a.kvh_div) && ok;
    if (a.fo_units && a.M > 1) {  // the o_proj riding the 2..16-row launch (its shape: this launch's)
      const int HD = a.fa.H * a.fa.D;
      a.fo_Sc = ((HD >> 5) / a.fo_kc) / ksplit / ku;
      const int fo_S = (HD >> 5) / (ksplit * ku);
      ok = a.fo_Sc > 0 && fastdiv_make((uint32_t)a.fo_Sc, (uint32_t)fo_S, &a.fo_sc_div) && ok;
    }
  }
  if (!ok) throw std::runtime_error("wgemm: no exact multiply-high pair for a launch divisor");
}

struct WgemmPlan {
  StreamPlan sp;  // the matrix's layout + launch shape (waves, stage depth, split-K)
  int cfg = 0;    // kernel instantiation of that shape (lm_gemm.hip)
  int grid = 1;
  bool a_lds = true;
  bool sliced = false;  // one K chunk per workgroup (grid.y = sp.kc) + combine kernel
  int csplit = 1;       // 2: units split into 8-column halves over twice the workgroups
  int ring = 0;         // 4: the one-row gate/up launch on the four-stage ring (TTS_GU_RING); 0: the shape's
};

// The warm role's arguments (WarmArgs, above) for the one-row gate/up launch of plan p over the
// tiled N x K matrix w: stages 0 .. W-1 of every gate/up workgroup's stream (its first units),
// read by wgs warm workgroups under the placement rule `shift`.  W is clamped to the item's stage
// count and to what kWarmMaxBytesPerXcd holds of one XCD's blocks; wgs is 0 (no warm role) or at
// least 8 (every class of blocks needs a warm workgroup).  The offsets are wgemm_stage_tile's.
inline WarmArgs wgemm_warm_plan(const WgemmPlan& p, const bf16_t* w, int N, int K, int W, int wgs, int shift) {
  const StreamPlan& s = p.sp;
  if (wgs < 0 || (wgs > 0 && wgs < kWarmXcds)) throw std::runtime_error("warm plan: 0 or at least 8 warm workgroups");
  if (p.sliced || p.csplit != 1 || p.grid != s.grid || N <= 0 || K <= 0 || N % (16 * s.ng) || K % (32 * s.ksplit * s.ku) ||
      (unsigned long long)N * (unsigned long long)K * 2ull > kWgemmMaxBytes)
    throw std::runtime_error("warm plan: not a plain one-round-order launch of a tiled matrix");
  const int upw = s.waves / s.ksplit, units = (N / 16) / s.ng, KT = K / 32, ur = s.ur();
  const int S = KT / (s.ksplit * s.ku);
  const int nr = ur < units ? ur : units;  // the first round's units: where every workgroup's stream starts
  auto at = [&](int ui, int st) {
    return (uint32_t)((unsigned long long)wgemm_stage_tile(0, ui, nr, st, 0, ur, KT, s.ng, s.ksplit, s.ku) * 1024ull);
  };
  WarmArgs a;
  a.w = w;
  a.bytes = (uint32_t)((unsigned long long)(N / 16) * KT * 1024ull);
  a.nblk = (nr + upw - 1) / upw;
  a.blk_bytes = at(upw, 0);
  a.last_bytes = at(nr - (a.nblk - 1) * upw, 0);
  a.stage_bytes = at(0, 1);
  const uint32_t per_xcd = (uint32_t)((a.nblk + kWarmXcds - 1) / kWarmXcds) * a.blk_bytes;
  const int fit = (int)(kWarmMaxBytesPerXcd / per_xcd);
  W = W < S ? W : S;
  W = W < fit ? W : fit;
  a.stages = (wgs > 0 && W > 0) ? W : 0;
  a.wgs = a.stages ? wgs : 0;
  a.shift = ((shift % kWarmXcds) + kWarmXcds) % kWarmXcds;
  return a;
}

void launch_warm_probe(const WarmArgs& warm, hipStream_t s);  // the warm role alone (lm_gemm_swiglu.hip)

// Row-major W [N][K] -> tiles of the matrix's stream plan.  The destination matrix has
// N_total rows; source n-tile nt lands at n-tile nt * nt_mult + nt_off (nt_mult = 2
// interleaves gate/up n-tiles: unit u = (gate tile u, up tile u), ng = 2).
void launch_retile(const bf16_t* w, bf16_t* t, int N, int K, int N_total, int ng, int num_cu,
                   hipStream_t s, int nt_mult = 1, int nt_off = 0);
WgemmPlan plan_wgemm(int M, int N, int K, int epi, int num_cu);
// LDS bytes of a wgemm launch whose A operand (M rows x Kl columns) is staged in LDS
size_t wgemm_lds_bytes(int waves, int ksplit, int ng, int M, int Kl, bool a_in_lds);
// fp32 partial workspace a K-sliced launch of this plan needs (elements)
inline size_t wgemm_part_elems(const WgemmPlan& p, int M, int ldo) {
  return p.sliced ? (size_t)p.sp.kc * M * ldo : 0;
}
bool wgemm_supported(int M, int N, int K, int epi);
bool wgemm_fattn_ok(int N, int K, int num_cu);
bool wgemm_fattn_rows_ok(int M, int N, int K, int D, int num_cu);
void launch_wgemm(const WgemmArgs& a, const WgemmPlan& p, int epi, bool norm, hipStream_t s);
// 17..32 rows of a kc = 1 qkv / o_proj layout (16-wave KSPLIT 16, KU 2), K split over 4
// workgroups (grid.y): fp32 partials [4][M][ldo] to a.part_out; a.K = K / 4 (lm_gemm_store.hip)
void launch_wgemm_kslice(const WgemmArgs& a, int units, hipStream_t s);

// ---- greedy lm_head as an exact two-pass argmax (lm_head_screen.hip): an int8 screen that
// bounds every column's processed score, then (in the same launch) the units that can hold the
// argmax recomputed exactly as the bf16 lm_head computes them
struct HeadScreenArgs {
  const bf16_t* x = nullptr;      // [M][ldx] rows (RMSNorm'ed here when normw)
  int M = 0, K = 0, ldx = 0, V = 0;
  const bf16_t* normw = nullptr;  // final RMSNorm weight, or nullptr (rows already normalised)
  float eps = 0.f;
  const int8_t* xq = nullptr;     // (17..32 rows) the rows pre-quantised [2M][K] (launch_head_rowquant)
  const float* xstat = nullptr;   //   and their {sx, |x|, |x - sx X|, 0} [M][4]
  const int8_t* q = nullptr;      // int8 lm_head in the screen's block layout (launch_head_quant)
  const float4* cst = nullptr;    // [V] {scale, |W - Wh|, |W|, |Wh|}
  int ur = 0;                     // layout units per round = screen grid * head_screen_waves()
  const bf16_t* w = nullptr;      // the tiled bf16 lm_head and its stream plan (ng 1, ksplit 1)
  int hku = 8, hur = 0, hKT = 0, hkc = 1;
  const uint32_t* seen = nullptr;
  int seen_stride = 0;
  float penalty = 1.f;
  const int* eos_mask = nullptr;
  const uint16_t* counts = nullptr;
  float freq_penalty = 0.f;
  const uint32_t* epoch = nullptr;      // the decode-step counter (finalize_greedy_kernel advances it)
  unsigned long long* lbg = nullptr;    // [M][8 shards] maximum lower bound: (step << 32) | order key
  uint32_t* arrive = nullptr;           // [8 shards, 64 B apart] workgroups that added their bounds (only grows)
  int spins = 1 << 14;                  // polls (s_sleep 1 each) before the wait for them gives up (0: no wait)
  float* part_val = nullptr;      // [M][part_stride] argmax partials, one per workgroup
  int* part_idx = nullptr;
  int part_stride = 0;
  int check = 0;                  // 1: recompute every unit, check each score against its bound
  float* ub = nullptr;            // check mode: [M][ldu] upper bound of every processed score
  int ldu = 0;
  int* err = nullptr;             // check mode: set to 1 when a score exceeds its bound
  int diag = 0;                   // probes only (TTS_HEAD_SCREEN_DIAG): 1 skip the recompute (wrong ids), 2 count flagged units
  // top-k mode (the sampled step; top_k > 0): candidates of the top-k set instead of the argmax
  int top_k = 0;
  unsigned long long* slots = nullptr;  // [M][grid] every workgroup's maximum lower bound: (step << 32) | order key
  float* cand_val = nullptr;      // [M][ldc] exact scores >= the row's threshold, in arrival order
  int* cand_idx = nullptr;        // [M][ldc] their ids
  int* cand_cnt = nullptr;        // [M] entries appended (zero at launch: the list's reader clears it)
  int ldc = 0;                    // >= V
  float* lbo = nullptr;           // check mode: [M][ldu] lower bound of every processed score
  // per-row top-k mode: penalty, freq_penalty and top_k of row m from par[m] (counts always set;
  // top_k = the largest top_k the batch admits, for the host checks only)
  const RowParams* par = nullptr;
};
constexpr int HEAD_SCREEN_MAX_TOP_K = 64;  // top-k mode: top_k <= this (and <= the screen's grid)
bool head_screen_supported(int M, int K, int V);
// the sampled step's form: 1..16 rows at K 2048, 1..8 at K 4096, top_k <= min(64, grid)
bool head_screen_topk_supported(int M, int K, int V, int top_k, int grid);
bool head_screen_prequant(int M);  // rows quantised by launch_head_rowquant first (17..32 rows, K 2048)
int head_screen_waves();
void launch_head_rowquant(const bf16_t* x, int ldx, int M, int K, int8_t* xq, float* xstat, hipStream_t s);
void launch_head_quant(const bf16_t* w, int V, int K, int ur, int8_t* q, float* cst, hipStream_t s);
void launch_head_screen(const HeadScreenArgs& a, int grid, hipStream_t s);

// ---- prefill GEMM (lm_pgemm.hip): many rows against the same tiled weights, LDS-staged
// MFMA blocks; epilogues EPI_STORE / EPI_RESID / EPI_SWIGLU; no fused RMSNorm
struct PgemmArgs {
  const bf16_t* x = nullptr;  // [M][ldx]
  int M = 0, K = 0, ldx = 0;
  const bf16_t* w = nullptr;  // tiled weights (the matrix's stream plan, filled in by launch_pgemm)
  int N = 0;
  int ng = 1, ksplit = 1, ku = 1, ur = 1, units = 1, kc = 1;
  bf16_t* out = nullptr;  // [M][ldo]
  int ldo = 0;
  bf16_t* resid = nullptr;  // EPI_RESID: updated in place
  int xcd_order = 0;        // set by launch_pgemm: the XCD-grouped tile order (lm_pgemm.hip)
  float* part = nullptr;    // fp32 partials of the one-chunk-per-workgroup form (null: never used)
  size_t part_bytes = 0;
  // optional (EPI_RESID): the next RMSNorm of the updated rows, written to xn [M][N] by the
  // one-chunk form's combine (launch_pgemm then returns true)
  const bf16_t* next_norm = nullptr;
  float eps = 0.f;
  bf16_t* xn = nullptr;
};
bool pgemm_supported(int M, int N, int K, int epi);
size_t pgemm_part_bytes(int M, int N, int K);  // the one-chunk form's partials of an M x N x K GEMM
bool launch_pgemm(const PgemmArgs& a, int epi, int num_cu, hipStream_t s);  // true: xn written

// ---- tile lm_head (lm_pgemm.hip, head_tile_kernel): the lm_head over 65..256 decode rows with the
// pick's epilogue (EPI_LOGITS / EPI_LOGITS_ROWS, lm_logit_epilogue.h) on the prefill GEMM's tile
// schedule, so the head streams once for every row.  Column blocks are 64 wide; a workgroup owns
// an m-block and a group of consecutive column blocks (all of K each, canonical chunks: the fp32
// sums of pgemm_kernel<.., EPI_STORE>) and carries each row's running argmax over the group: row
// m ends with head_tile_nparts(N) partials (value, id), partial g covering the columns of group g.
struct HeadTileArgs {
  PgemmArgs g;  // x (normalised rows), M, K, ldx, w (the tiled head), N; the rest filled in by the launch
  // the epilogue's operands, named as WgemmArgs names them (logit_epilogue reads either)
  const uint32_t* seen = nullptr;  // [M][seen_stride]
  int seen_stride = 0;
  float penalty = 1.f;
  const int* eos_mask = nullptr;  // [M]
  float* part_val = nullptr;      // [M][part_stride]
  int* part_idx = nullptr;
  int part_stride = 0;
  float* logits_out = nullptr;  // optional: the processed fp32 logits [M][ldl]
  int ldl = 0;
  const uint16_t* counts = nullptr;  // [M][seen_stride*32] or nullptr
  float freq_penalty = 0.f;
  const RowParams* row_par = nullptr;  // the per-row form: [M] (counts set)
  int cb = 1, groups = 1;              // column blocks per group, groups (filled in by the launch)
};
constexpr int kHeadTileMaxRows = 256;
bool head_tile_supported(int M, int N, int K);  // 1 <= M <= 256, N % 64 == 0, K % 128 == 0
int head_tile_nparts(int N);                    // argmax partials per row (<= LOGITS_MAX_PARTS)
void launch_head_tile(const HeadTileArgs& a, bool per_row, int num_cu, hipStream_t s);

// ---- elementwise / small kernels (lm_ops.hip)
void launch_rmsnorm(const bf16_t* x, int ldx, const bf16_t* w, float eps, bf16_t* y, int ldy,
                    int M, int K, hipStream_t s);
void launch_embed(const int* tokens, const bf16_t* table, bf16_t* x, int M, int hidden,
                  hipStream_t s);
void launch_gather_rows(const bf16_t* x, int ld, const int* rows, bf16_t* y, int M, int hidden,
                        hipStream_t s);
void launch_synth_fill(void* dst, int dtype, long long n, unsigned long long seed, float scale,
                       hipStream_t s);
void launch_f32_to_bf16(const float* x, bf16_t* y, long long n, hipStream_t s);
void launch_f16_to_bf16(const void* x, bf16_t* y, long long n, hipStream_t s);  // x: _Float16
// K-sliced GEMM combine: v = bf16(sum_c part[c][m][n]);  resid ? resid += v : out = v
void launch_splitk_combine(const float* part, int kc, int M, int N, int ldp, bf16_t* out,
                           bf16_t* resid, int ldo, hipStream_t s);
// residual combine + the next RMSNorm of the updated rows into xn (N % 8 == 0, N <= 8192)
void launch_splitk_combine_norm(const float* part, int kc, int M, int N, int ldp, bf16_t* resid, int ldo,
                                const bf16_t* normw, float eps, bf16_t* xn, int ldn, hipStream_t s);

// ---- attention (lm_attn.hip)
// Prefill rows of one sequence: positions pos0 .. pos0 + len - 1 of KV slot `slot` become query
// rows row0 .. row0 + len - 1 (appended to row_slot / row_pos) and query blocks of up to 16
// consecutive rows (appended to blk as {first row, rows, slot, first position}, AttnArgs::blocks).
inline void prefill_seq_rows(int slot, int pos0, int len, int row0, std::vector<int>& row_slot,
                             std::vector<int>& row_pos, std::vector<int>& blk) {
  for (int i = 0; i < len; ++i) {
    row_slot.push_back(slot);
    row_pos.push_back(pos0 + i);
  }
  for (int t0 = 0; t0 < len; t0 += 16)
    blk.insert(blk.end(), {row0 + t0, len - t0 < 16 ? len - t0 : 16, slot, pos0 + t0});
}
void launch_rope_append(const AttnArgs& a, hipStream_t s);  // prefill: rope q, k; K rows, V columns
void launch_attn_prefill(const AttnArgs& a, hipStream_t s);  // prefill: causal attention per query block
// decode step: one workgroup per (row, kv head): RoPE, attention over pos + 1 positions,
// bf16 output, KV append
void launch_attn_decode_step(const AttnArgs& a, hipStream_t s);

// ---- sampling head (lm_sample.hip): temperature, top-k, top-p, multinomial draw
struct SampleArgs {
  const float* logits = nullptr;  // processed logits [B][ldl]
  int ldl = 0, V = 0;
  float temperature = 1.f;
  int top_k = 50;                 // 1 .. 1024
  float top_p = 1.f;
  unsigned long long seed = 0;
  const unsigned long long* row_seed = nullptr;  // per-row keys (seed, row ignored) or nullptr
  const int* step = nullptr;      // per-row draw counter (generated count), or step0
  int step0 = 0;
  const int* done = nullptr;      // rows already stopped (skipped)
  const float* part_val = nullptr;  // lm_head workgroup maxima [B][part_stride] (top-k bound)
  int nparts = 0, part_stride = 0;
  float* out_part_val = nullptr;  // chosen token as the single "partial" finalize reads
  int* out_part_idx = nullptr;
  float* probs = nullptr;         // optional: final distribution [B][ldl] (kept ids only)
  int* tokens = nullptr;          // optional: chosen token [B]
  // list form (launch_sample_list): logits = the rows' candidate scores [B][ldl], entry i of row b
  // standing for id list_idx[b][i]; list_cnt[b] entries (at most V = the lists' capacity); vocab =
  // the dense row's length (top_k >= vocab: no top-k cut; probs rows are [vocab] wide)
  const int* list_idx = nullptr;
  int* list_cnt = nullptr;
  int list_clear = 0;             // 1: zero list_cnt[b] once read (the screened head appends from zero)
  int vocab = 0;
  // per-row settings (launch_sample_rows / launch_sample_list_rows): row b reads element
  // b * row_stride of each array (row_stride 1: plain arrays; 8: the fields of a RowParams table)
  const float* row_temp = nullptr;
  const int* row_top_k = nullptr;
  const float* row_top_p = nullptr;
  const int* row_sample = nullptr;  // 0: a greedy row (argmax, lowest id on ties; no warper, no draw)
  int row_stride = 1;
  const int* part_idx = nullptr;    // dense per-row form: the ids of part_val (a greedy row's argmax partials)
};
constexpr int SAMPLE_MAX_TOP_K = 1024;
inline void sample_rows_from_table(SampleArgs& a, const RowParams* par) {
  a.row_temp = &par->temperature; a.row_top_k = &par->top_k; a.row_top_p = &par->top_p; a.row_sample = &par->sample;
  a.row_stride = (int)(sizeof(RowParams) / 4);
}
void launch_sample(const SampleArgs& a, int B, hipStream_t s);
// the same draw from per-row candidate lists that hold (at least) every entry of the top-k set
void launch_sample_list(const SampleArgs& a, int B, hipStream_t s);
// the per-row forms: temperature / top_k / top_p / sample of row b from the row_* arrays
void launch_sample_rows(const SampleArgs& a, int B, hipStream_t s);
void launch_sample_list_rows(const SampleArgs& a, int B, hipStream_t s);

void launch_bump_epoch(uint32_t* epoch, hipStream_t s);  // *epoch += 1 (a decode step without finalize)
void launch_finalize_greedy(const float* part_val, const int* part_idx, int part_stride,
                            int nparts, StepState st, int B, const bf16_t* embed, bf16_t* x,
                            int hidden, hipStream_t s);

}  // namespace tts
