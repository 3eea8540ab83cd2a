// lm_load.cpp — SpeechLM weights and workspaces: tensor upload and re-layout into the stream
// plans' tile order, the RoPE table, the int8 screen of the lm_head, workspace sizing.
#include "lm_step.h"

namespace tts {

// The greedy lm_head as an exact two-pass argmax (lm_head_screen.hip): default on;
// TTS_HEAD_SCREEN=0 streams the full bf16 lm_head for greedy steps too (the same ids)
static bool head_screen_enabled() { static const bool v = env_on("TTS_HEAD_SCREEN"); return v; }

int64_t numel(const tts_tensor_desc& d) {
  int64_t n = 1;
  for (int i = 0; i < d.ndim; ++i) n *= d.shape[i];
  return n;
}

void upload_bf16(const tts_tensor_desc& d, bf16_t* dst, hipStream_t s, DevBuf& staging) {
  const int64_t n = numel(d);
  if (d.dtype == TTS_DT_BF16) {
    HIP_CHECK(hipMemcpyAsync(dst, d.data, n * 2, d.on_device ? hipMemcpyDeviceToDevice
                                                             : hipMemcpyHostToDevice, s));
  } else if (d.dtype == TTS_DT_F32) {
    const float* src = (const float*)d.data;
    if (!d.on_device) {
      if (staging.bytes < (size_t)n * 4) staging.alloc((size_t)n * 4);
      HIP_CHECK(hipMemcpyAsync(staging.p, d.data, n * 4, hipMemcpyHostToDevice, s));
      src = staging.as<float>();
    }
    launch_f32_to_bf16(src, dst, n, s);
  } else if (d.dtype == TTS_DT_F16) {
    const void* src = d.data;
    if (!d.on_device) {
      if (staging.bytes < (size_t)n * 2) staging.alloc((size_t)n * 2);
      HIP_CHECK(hipMemcpyAsync(staging.p, d.data, n * 2, hipMemcpyHostToDevice, s));
      src = staging.p;
    }
    launch_f16_to_bf16(src, dst, n, s);
  } else {
    throw Error(TTS_E_UNSUPPORTED, std::string("tensor ") + d.name + ": dtype must be bf16, f16 or f32");
  }
}

// ------------------------------------------------------------------------ loading -----
namespace {
struct TensorMap {
  std::map<std::string, const tts_tensor_desc*> m;
  const tts_tensor_desc& get(const std::string& name, std::initializer_list<int64_t> shape) const {
    auto it = m.find(name);
    if (it == m.end()) throw Error(TTS_E_INVALID, "missing tensor: " + name);
    const tts_tensor_desc& d = *it->second;
    int i = 0;
    bool ok = (int)shape.size() == d.ndim;
    for (int64_t v : shape) { if (ok && d.shape[i] != v) ok = false; ++i; }
    if (!ok) throw Error(TTS_E_INVALID, "bad shape for tensor: " + name);
    return d;
  }
  bool has(const std::string& n) const { return m.count(n) != 0; }
};

// RoPE table as LlamaRotaryEmbedding computes it (modeling_llama.py:~100-128 and
// modeling_rope_utils.py:580-660 for llama3), evaluated in double then rounded; the Python
// host normally passes the torch-computed table instead ("rope.cos"/"rope.sin").
void compute_rope_table(const tts_lm_config& c, std::vector<bf16_t>& cs, std::vector<bf16_t>& sn) {
  const int D = c.head_dim, S = c.max_seq_len;
  std::vector<float> inv(D / 2);
  for (int i = 0; i < D / 2; ++i) {
    float e = (float)(2 * i) / (float)D;
    inv[i] = 1.0f / powf(c.rope_theta, e);
  }
  if (c.rope_llama3) {
    const double lo_wl = c.rope_original_max_position / c.rope_low_freq_factor;
    const double hi_wl = c.rope_original_max_position / c.rope_high_freq_factor;
    for (int i = 0; i < D / 2; ++i) {
      const float f = inv[i];
      const double wl = 2 * M_PI / f;
      float v = (wl > lo_wl) ? f / c.rope_factor : f;
      if (!(wl < hi_wl) && !(wl > lo_wl)) {
        const float sm = (float)((c.rope_original_max_position / wl - c.rope_low_freq_factor) /
                                 (c.rope_high_freq_factor - c.rope_low_freq_factor));
        v = (1 - sm) * v / c.rope_factor + sm * v;
      }
      inv[i] = v;
    }
  }
  auto to_bf = [](float f) -> bf16_t {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
  };
  cs.resize((size_t)S * D);
  sn.resize((size_t)S * D);
  for (int p = 0; p < S; ++p)
    for (int i = 0; i < D; ++i) {
      const float fr = (float)p * inv[i % (D / 2)];
      cs[(size_t)p * D + i] = to_bf((float)cos((double)fr));
      sn[(size_t)p * D + i] = to_bf((float)sin((double)fr));
    }
}
}  // namespace

// K-sliced GEMMs (store / residual epilogues): fp32 partials of kc = K / 2048 chunks of <= 64 rows
size_t kpart_bytes(const tts_lm_config& c) {
  const int kmax = std::max(c.hidden_size, std::max(c.intermediate_size, c.num_heads * c.head_dim));
  const int QKV = (c.num_heads + 2 * c.num_kv_heads) * c.head_dim;
  return (size_t)std::max(1, kmax / 2048) * kPrefillChunk * std::max(QKV, c.hidden_size) * 4;
}

// prefill GEMMs of <= kPgemmSplitRows rows may take one canonical K chunk per workgroup
// (lm_pgemm.hip): fp32 partials [chunks][rows][N] of the largest of the layer's four GEMMs
static constexpr int kPgemmSplitRows = 256;
size_t ppart_bytes(const tts_lm_config& c) {
  const int H = c.hidden_size, HD = c.num_heads * c.head_dim, FF = c.intermediate_size;
  const int QKV = (c.num_heads + 2 * c.num_kv_heads) * c.head_dim;
  return std::max(std::max(pgemm_part_bytes(kPgemmSplitRows, QKV, H), pgemm_part_bytes(kPgemmSplitRows, H, HD)),
                  std::max(pgemm_part_bytes(kPgemmSplitRows, 2 * FF, H), pgemm_part_bytes(kPgemmSplitRows, H, FF)));
}

// The int8 screen of the lm_head (lm_head_screen.hip; TTS_HEAD_SCREEN=0: none) exists for a
// model whose lm_head streams whole units, one K part: its launch grid, or 0
int head_screen_grid(const tts_lm_config& c, int num_cu) {
  const StreamPlan hp = stream_plan(c.vocab_size, c.hidden_size, 1, num_cu);
  const bool on = head_screen_enabled() && head_screen_supported(1, c.hidden_size, c.vocab_size) &&
                  hp.ng == 1 && hp.ksplit == 1;
  return on ? num_cu : 0;
}

void lm_load(Engine* e, const tts_lm_config* cfgp, const tts_tensor_desc* t, int n) {
  TTS_REQUIRE(cfgp != nullptr, "null config");
  const tts_lm_config c = *cfgp;
  TTS_REQUIRE(c.head_dim == 64 || c.head_dim == 128, "head_dim must be 64 or 128");
  TTS_REQUIRE(c.num_heads == 4 * c.num_kv_heads, "GQA group must be 4 (num_heads == 4*num_kv_heads)");
  TTS_REQUIRE(c.hidden_size % 256 == 0 && c.intermediate_size % 256 == 0 &&
                  (c.num_heads * c.head_dim) % 256 == 0,
              "hidden/intermediate/attention widths must be multiples of 256");
  TTS_REQUIRE(c.vocab_size % 16 == 0, "vocab_size must be a multiple of 16");
  // (the GEMMs stream a matrix through one buffer resource: 32-bit byte offsets)
  TTS_REQUIRE((double)c.vocab_size * c.hidden_size * 2 < 4.0e9 &&
                  (double)2 * c.intermediate_size * c.hidden_size * 2 < 4.0e9,
              "a weight matrix of 4 GB or more is not supported");
  TTS_REQUIRE(c.max_batch >= 1 && c.max_batch <= kHeadTileMaxRows, "max_batch must be in [1, 256]");
  TTS_REQUIRE(c.max_seq_len >= 16, "max_seq_len too small");
  TensorMap tm;
  for (int i = 0; i < n; ++i) tm.m[t[i].name] = &t[i];
  hipStream_t s = e->stream;
  LmModel& M = e->lm;
  M.loaded = false;
  M.cfg = c;
  const int H = c.num_heads, KVH = c.num_kv_heads, D = c.head_dim, HID = c.hidden_size;
  const int FF = c.intermediate_size, V = c.vocab_size, L = c.num_layers;
  const int QKV = M.qkv_n();

  // ---- one slab for everything
  const size_t per_layer = 2 * (size_t)HID + (size_t)QKV * HID + (size_t)HID * H * D +
                           2 * (size_t)FF * HID + (size_t)HID * FF;
  const size_t total = per_layer * L + HID + (size_t)V * HID;
  M.weights.alloc(total * 2);
  bf16_t* p = M.weights.as<bf16_t>();
  M.layers.resize(L);
  for (int l = 0; l < L; ++l) {
    LmLayer& ly = M.layers[l];
    ly.ln1 = p; p += HID;
    ly.ln2 = p; p += HID;
    ly.wqkv = p; p += (size_t)QKV * HID;
    ly.wo = p; p += (size_t)HID * H * D;
    ly.wgu = p; p += 2 * (size_t)FF * HID;
    ly.wd = p; p += (size_t)HID * FF;
  }
  M.final_norm = p; p += HID;
  M.lm_head = p; p += (size_t)V * HID;

  DevBuf staging, staging32;
  staging.alloc((size_t)std::max<size_t>((size_t)V * HID, (size_t)FF * HID) * 2);
  // matrix (N_total rows, ng) <- row block of N rows at n-tile offset `off` (or interleaved)
  const int ncu = e->num_cu;
  auto retiled = [&](const tts_tensor_desc& d, bf16_t* dst, int N, int K, int N_total, int ng,
                     int mult, int off) {
    upload_bf16(d, staging.as<bf16_t>(), s, staging32);
    launch_retile(staging.as<bf16_t>(), dst, N, K, N_total, ng, ncu, s, mult, off);
    HIP_CHECK(hipGetLastError());
  };
  for (int l = 0; l < L; ++l) {
    LmLayer& ly = M.layers[l];
    const std::string pre = "model.layers." + std::to_string(l) + ".";
    upload_bf16(tm.get(pre + "input_layernorm.weight", {HID}), ly.ln1, s, staging32);
    upload_bf16(tm.get(pre + "post_attention_layernorm.weight", {HID}), ly.ln2, s, staging32);
    retiled(tm.get(pre + "self_attn.q_proj.weight", {H * D, HID}), ly.wqkv, H * D, HID, QKV, 1, 1, 0);
    retiled(tm.get(pre + "self_attn.k_proj.weight", {KVH * D, HID}), ly.wqkv, KVH * D, HID, QKV, 1, 1,
            H * D / 16);
    retiled(tm.get(pre + "self_attn.v_proj.weight", {KVH * D, HID}), ly.wqkv, KVH * D, HID, QKV, 1, 1,
            (H + KVH) * D / 16);
    retiled(tm.get(pre + "self_attn.o_proj.weight", {HID, H * D}), ly.wo, HID, H * D, HID, 1, 1, 0);
    retiled(tm.get(pre + "mlp.gate_proj.weight", {FF, HID}), ly.wgu, FF, HID, 2 * FF, 2, 2, 0);
    retiled(tm.get(pre + "mlp.up_proj.weight", {FF, HID}), ly.wgu, FF, HID, 2 * FF, 2, 2, 1);
    retiled(tm.get(pre + "mlp.down_proj.weight", {HID, FF}), ly.wd, HID, FF, HID, 1, 1, 0);
  }
  upload_bf16(tm.get("model.norm.weight", {HID}), M.final_norm, s, staging32);
  const tts_tensor_desc& emb = tm.get("model.embed_tokens.weight", {V, HID});
  M.embed_rows.alloc((size_t)V * HID * 2);
  upload_bf16(emb, M.embed_rows.as<bf16_t>(), s, staging32);
  if (c.tie_word_embeddings) {
    launch_retile(M.embed_rows.as<bf16_t>(), M.lm_head, V, HID, V, 1, ncu, s, 1, 0);
  } else {
    retiled(tm.get("lm_head.weight", {V, HID}), M.lm_head, V, HID, V, 1, 1, 0);
  }
  // the greedy lm_head's int8 screen (lm_head_screen.hip; TTS_HEAD_SCREEN=0: none), made from
  // the row-major matrix (the embedding rows when tied, else the staged upload)
  M.head_grid = head_screen_grid(c, ncu);
  M.head_q.release();
  M.head_c.release();
  if (M.head_grid) {
    M.head_q.alloc((size_t)V * HID);
    M.head_c.alloc((size_t)V * 16);
    launch_head_quant(c.tie_word_embeddings ? M.embed_rows.as<bf16_t>() : staging.as<bf16_t>(), V, HID,
                      M.head_grid * head_screen_waves(), M.head_q.as<int8_t>(), M.head_c.as<float>(), s);
    HIP_CHECK(hipGetLastError());
  }

  // ---- RoPE table
  M.rope.alloc((size_t)2 * c.max_seq_len * D * 2);
  if (tm.has("rope.cos") && tm.has("rope.sin")) {
    upload_bf16(tm.get("rope.cos", {c.max_seq_len, D}), M.rope.as<bf16_t>(), s, staging32);
    upload_bf16(tm.get("rope.sin", {c.max_seq_len, D}),
                M.rope.as<bf16_t>() + (size_t)c.max_seq_len * D, s, staging32);
  } else {
    std::vector<bf16_t> cs, sn;
    compute_rope_table(c, cs, sn);
    HIP_CHECK(hipMemcpy(M.rope.as<bf16_t>(), cs.data(), cs.size() * 2, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(M.rope.as<bf16_t>() + cs.size(), sn.data(), sn.size() * 2,
                        hipMemcpyHostToDevice));
  }
  M.id_to_code.clear();
  if (tm.has("vocab.id_to_code")) {
    const tts_tensor_desc& d = tm.get("vocab.id_to_code", {V});
    TTS_REQUIRE(d.dtype == TTS_DT_I32 && !d.on_device, "vocab.id_to_code must be host int32");
    M.id_to_code.assign((const int*)d.data, (const int*)d.data + V);
  }
  HIP_CHECK(hipStreamSynchronize(s));

  // ---- workspaces
  LmWork& w = e->w;
  if (w.graph) { (void)hipGraphExecDestroy(w.graph); w.graph = nullptr; w.step_key = StepKey(); }
  const int B = c.max_batch, S = c.max_seq_len;
  const int R = std::max(B, std::min(kMaxPrefillRows, B * S));
  w.cap_rows = R;
  w.cap_batch = B;
  w.kv_stride = (S + 63) / 64 * 64;  // (V^T fragments: 8 positions = 16 B, aligned)
  w.kv.alloc((size_t)L * 2 * B * KVH * w.kv_stride * D * 2);
  HIP_CHECK(hipMemsetAsync(w.kv.p, 0, w.kv.bytes, s));  // never-read garbage stays finite
  w.x.alloc((size_t)R * HID * 2);
  w.xn.alloc((size_t)R * HID * 2);
  w.qkv.alloc((size_t)R * QKV * 2);
  w.attn_out.alloc((size_t)R * H * D * 2);
  w.q_rot.alloc((size_t)R * H * D * 2);
  w.act.alloc((size_t)R * FF * 2);
  w.last_x.alloc((size_t)B * HID * 2);
  w.blocks.alloc(((size_t)R / 16 + B + 1) * 16);  // prefill query blocks: <= rows/16 + one per sequence
  // q|k|v granules of every decode row ([B][QKV/2]), and (one-row launches with o_proj fused)
  // the attention row's at row 1's place (a launch uses one form; every prefill resets them all)
  w.gran.alloc((size_t)std::max(B, 2) * (QKV + H * D) / 2 * 8);  // q|k|v, then attention rows
  HIP_CHECK(hipMemsetAsync(w.gran.p, 0xff, w.gran.bytes, s));  // tag 0xffffffff: never a launch's
  w.ferr.alloc(256);  // (FERR_SLOTS ints used)
  w.epoch.alloc(64);
  HIP_CHECK(hipMemsetAsync(w.epoch.p, 0, 64, s));
  HIP_CHECK(hipMemsetAsync(w.ferr.p, 0, 256, s));
  w.kpart.alloc(kpart_bytes(c));
  w.ppart.alloc(ppart_bytes(c));
  w.slogits.alloc((size_t)B * V * 4);
  w.counts.alloc((size_t)B * (V / 32 + 1) * 32 * 2);
  w.lpart_v.alloc((size_t)B * LOGITS_MAX_PARTS * 4);
  w.lpart_i.alloc((size_t)B * LOGITS_MAX_PARTS * 4);
  for (DevBuf* b : {&w.hub, &w.hlb, &w.hxq, &w.hxs, &w.hslot, &w.hcv, &w.hci, &w.hcn, &w.hlo}) b->release();
  if (M.head_grid) {
    if (head_screen_check()) w.hub.alloc((size_t)std::min(B, 32) * V * 4);  // (check mode's bounds)
    w.hxq.alloc((size_t)2 * 32 * HID);
    w.hxs.alloc((size_t)32 * 16);
    w.hlb.alloc(32 * 8 * 8 + 8 * 64);  // 32 rows x 8 shards of bounds + 8 arrival counters (64 B apart)
    HIP_CHECK(hipMemsetAsync(w.hlb.p, 0, w.hlb.bytes, s));  // (below any step's key)
    // the sampled step (1..16 rows): a slot per (row, workgroup), the candidate lists (capacity V a
    // row: they cannot overflow) and their counts (zero between steps: the sampler clears them)
    const int SB = std::min(B, 16);
    w.hslot.alloc((size_t)16 * 512 * 8);
    HIP_CHECK(hipMemsetAsync(w.hslot.p, 0, w.hslot.bytes, s));
    w.hcv.alloc((size_t)SB * V * 4);
    w.hci.alloc((size_t)SB * V * 4);
    w.hcn.alloc(64);
    HIP_CHECK(hipMemsetAsync(w.hcn.p, 0, 64, s));
    if (head_screen_check()) w.hlo.alloc((size_t)SB * V * 4);
  }
  w.row_slot.alloc((size_t)R * 4);
  w.row_pos.alloc((size_t)R * 4);
  w.row_idx.alloc((size_t)R * 4);
  w.st_int.alloc((size_t)B * 8 * 4 + 64);  // (>= the st_zeros(B) ints of the layout, lm_step.h)
  w.row_seed.alloc((size_t)B * 8);
  w.row_par.alloc((size_t)B * sizeof(RowParams));
  w.seen.alloc((size_t)B * (V / 32 + 1) * 4);
  w.out_cap = S;
  w.out_ids.alloc((size_t)B * S * 4);
  if (!w.h_active) HIP_CHECK(hipHostMalloc((void**)&w.h_active, 64, hipHostMallocDefault));
  M.loaded = true;
}

}  // namespace tts
