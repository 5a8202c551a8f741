// Waypoint predictor engine: BinaryDistPredictor_TRM.forward (vlnce_baselines/waypoint_pred/TRM_net.py:62-88) over one flat
// parameter arena, as a chain of the library's GEMM / LayerNorm launches plus the neighbourhood attention of waypoint.hip.
// Forward only (frozen, eval(): ss_trainer_ETP.py:201-202,490,586,711 -- the dropout of 0.3 never acts).
//
//   x      = relu(depth_feats . W_fc^T + b)                                 TRM_net.py:27-31,67-72     [12B, 2048] -> [12B, 768]
//   2 x    qkv = x . [Wq;Wk;Wv]^T + b   (one N = 2304 product)              waypoint_bert.py:57-59
//          ctx = ring attention, window TRM_NEIGHBOR = 1                    waypoint_bert.py:62-86, utils.py:90-102
//          a   = LN(ctx . Wo^T + b + x)                                     modeling_bert.py BertSelfOutput
//          x   = LN(gelu(a . Wi^T + b) . Wd^T + b + a)                      BertIntermediate / BertOutput
//   logits = relu(x . W1^T + b1) . W2^T + b2                                TRM_net.py:55-60,79-81     [12B, 120] = [B, 120, 12]
//   roll the angle axis by HEATMAP_OFFSET = 5                               TRM_net.py:83-86
//
// Launches per call: 18 in fp32 mode (1 + 2 x 7 + 2 + 1), 20 in bf16 mode (two operand casts: depth_feats and x).
#include <string.h>

#include <string>
#include <vector>

#include "arena.h"
#include "kernels.h"

namespace etp {
struct WpLayer { int qkv_w, qkv_b, o_w, o_b, ln1_g, ln1_b, i_w, i_b, d_w, d_b, ln2_g, ln2_b; };
constexpr int WP_H = 768, WP_I = 3072, WP_DEPTH = 2048, WP_OUT = 120, WP_LAYERS = 2, WP_NEIGHBOR = 1;
constexpr float WP_LN_EPS = 1e-12f;
}  // namespace etp

struct etp_waypoint : etp::ArenaEngine {
  int fc_w, fc_b, c1_w, c1_b, c2_w, c2_b;
  etp::WpLayer layer[etp::WP_LAYERS];
};

namespace etp {

// state-dict order of the reference module (TRM_net.py:27-60); region 0 = GEMM matrices (bf16 shadow), 1 = vectors.  The two
// modules the forward never uses (visual_merge, mergefeats_LayerNorm) are in the table so that a strict load sees every key.
static void wp_layout(etp_waypoint* w) {
  auto mat = [&](const std::string& n, long r, long k) { return w->table.add(n, 0, {r, k}); };
  auto vec = [&](const std::string& n, long r) { return w->table.add(n, 1, {r}); };
  w->fc_w = mat("visual_fc_depth.1.weight", WP_H, WP_DEPTH);
  w->fc_b = vec("visual_fc_depth.1.bias", WP_H);
  w->table.add("visual_merge.0.weight", 1, {WP_H, 2 * WP_H});                // unused: kept out of the shadow region
  vec("visual_merge.0.bias", WP_H);
  for (int l = 0; l < WP_LAYERS; ++l) {
    const std::string p = "waypoint_TRM.bert.encoder.layer." + std::to_string(l);
    WpLayer& L = w->layer[l];
    L.qkv_w = mat(p + ".attention.self.query.weight", WP_H, WP_H);
    L.qkv_b = vec(p + ".attention.self.query.bias", WP_H);
    mat(p + ".attention.self.key.weight", WP_H, WP_H);
    vec(p + ".attention.self.key.bias", WP_H);
    mat(p + ".attention.self.value.weight", WP_H, WP_H);
    vec(p + ".attention.self.value.bias", WP_H);
    L.o_w = mat(p + ".attention.output.dense.weight", WP_H, WP_H);
    L.o_b = vec(p + ".attention.output.dense.bias", WP_H);
    L.ln1_g = vec(p + ".attention.output.LayerNorm.weight", WP_H);
    L.ln1_b = vec(p + ".attention.output.LayerNorm.bias", WP_H);
    L.i_w = mat(p + ".intermediate.dense.weight", WP_I, WP_H);
    L.i_b = vec(p + ".intermediate.dense.bias", WP_I);
    L.d_w = mat(p + ".output.dense.weight", WP_H, WP_I);
    L.d_b = vec(p + ".output.dense.bias", WP_H);
    L.ln2_g = vec(p + ".output.LayerNorm.weight", WP_H);
    L.ln2_b = vec(p + ".output.LayerNorm.bias", WP_H);
  }
  vec("mergefeats_LayerNorm.weight", WP_H);
  vec("mergefeats_LayerNorm.bias", WP_H);
  w->c1_w = mat("vis_classifier.0.weight", WP_H, WP_H);
  w->c1_b = vec("vis_classifier.0.bias", WP_H);
  w->c2_w = mat("vis_classifier.2.weight", WP_OUT, WP_H);
  w->c2_b = vec("vis_classifier.2.bias", WP_OUT);
  // matrices first, in declaration order: query / key / value of a layer are adjacent (768 * 768 is a multiple of 64), so the three
  // are one [2304, 768] operand; the same holds for their biases in the vector region
  w->table.layout(2);
}

// the ONE scratch plan of etp_waypoint_fwd (NULL base: sizes only)
struct WpScratch { void* dep; float* xf; void* xt; void* qkv; void* ctx; float* s; float* af; void* at; void* h; void* z; void* r;
                   float* stats; float* raw; size_t bytes; };
static WpScratch wp_plan(int dt, void* base, int B) {
  const size_t es = dtype_size(dt);
  const size_t M = (size_t)B * 12;
  Bump b(base);
  WpScratch s;
  s.dep = dt == ETP_BF16 ? b.take(M * WP_DEPTH * es) : nullptr;      // operand copy of depth_feats
  s.xf = (float*)b.take(M * WP_H * 4);                               // residual stream (fp32) ...
  s.xt = dt == ETP_BF16 ? b.take(M * WP_H * es) : (void*)s.xf;       // ... and its GEMM-operand copy
  s.qkv = b.take(M * 3 * WP_H * es);
  s.ctx = b.take(M * WP_H * es);
  s.s = (float*)b.take(M * WP_H * 4);                                // pre-LayerNorm sums
  s.af = (float*)b.take(M * WP_H * 4);
  s.at = dt == ETP_BF16 ? b.take(M * WP_H * es) : (void*)s.af;
  s.h = b.take(M * WP_I * es);
  s.z = b.take(M * WP_I * es);                                       // the GELU epilogue's second output (unused: no backward)
  s.r = b.take(M * WP_H * es);                                       // classifier hidden
  s.stats = (float*)b.take(M * 2 * 4);
  s.raw = (float*)b.take(M * WP_OUT * 4);                            // logits before the roll
  s.bytes = b.off;
  return s;
}

static int wp_linear(const etp_waypoint* w, int c_dtype, const void* X, long ldx, int wi, int bi, void* Y, long ldy, int M, int N,
                     int K, int act, void* Z, const void* R, hipStream_t st) {
  GemmArgs g = base_args();
  g.A = X; g.lda = ldx; g.B = w->pw(wi); g.ldb = K; g.C = Y; g.ldc = ldy;
  g.M = M; g.N = N; g.K = K;
  g.bias = w->pf(bi);
  g.act = act; g.Z = Z; g.ldz = ldy; g.R = R; g.ldr = ldy;
  return launch_gemm(w->dtype, c_dtype, 0, 0, g, 1, st);
}

}  // namespace etp

using namespace etp;

extern "C" {

etp_waypoint* etp_waypoint_create(int dtype) {
  if (dtype != ETP_F32 && dtype != ETP_BF16) { set_error("etp_waypoint_create: dtype must be ETP_F32 or ETP_BF16"); return nullptr; }
  etp_waypoint* w = new etp_waypoint();
  w->dtype = dtype;
  wp_layout(w);
  return w;
}
void etp_waypoint_destroy(etp_waypoint* w) { delete w; }
int etp_waypoint_param_count(const etp_waypoint* w) { return w ? w->table.size() : 0; }
int etp_waypoint_param_info(const etp_waypoint* w, int i, etp_param_info* out) {
  ETP_REQUIRE(w && out && i >= 0 && i < w->table.size(), "bad index");
  w->table.fill(i, out);
  return ETP_OK;
}
int64_t etp_waypoint_arena_elems(const etp_waypoint* w) { return w ? w->table.total : 0; }
int64_t etp_waypoint_matrix_elems(const etp_waypoint* w) { return w ? w->table.n_matrix : 0; }
int etp_waypoint_bind(etp_waypoint* w, float* params, void* shadow) {
  return bind_arenas(__func__, w, params, shadow, "null engine / params");
}
int etp_waypoint_refresh_weights(etp_waypoint* w, etp_stream_t stream) {
  ETP_REQUIRE(w && w->P, "engine not bound");
  if (w->dtype != ETP_BF16) return ETP_OK;
  return cast_f32_to_bf16(w->P, w->Wc, w->table.n_matrix, (hipStream_t)stream);
}
int64_t etp_waypoint_ws_bytes(const etp_waypoint* w, int B) {
  if (!w || B <= 0) return 0;
  return (int64_t)wp_plan(w->dtype, nullptr, B).bytes + 256;
}

int etp_waypoint_fwd(etp_waypoint* w, const float* depth_feats, int B, float* logits, void* ws, etp_stream_t stream) {
  ETP_REQUIRE(w && w->P && depth_feats && logits && ws && B > 0, "bad arguments");
  ETP_REQUIRE(((uintptr_t)depth_feats | (uintptr_t)logits) % 16 == 0 && (uintptr_t)ws % 256 == 0,
              "depth_feats / logits must be 16-byte aligned, ws 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int dt = w->dtype, M = B * 12;
  const WpScratch s = wp_plan(dt, ws, B);
  const void* dep = depth_feats;
  if (dt == ETP_BF16) {
    ETP_TRY(cast_f32_to_bf16(depth_feats, s.dep, (long)M * WP_DEPTH, st));
    dep = s.dep;
  }
  ETP_TRY(wp_linear(w, ETP_F32, dep, WP_DEPTH, w->fc_w, w->fc_b, s.xf, WP_H, M, WP_H, WP_DEPTH, ETP_ACT_RELU, nullptr, nullptr, st));
  if (dt == ETP_BF16) ETP_TRY(cast_f32_to_bf16(s.xf, s.xt, (long)M * WP_H, st));
  for (int l = 0; l < WP_LAYERS; ++l) {
    const WpLayer& L = w->layer[l];
    ETP_TRY(wp_linear(w, dt, s.xt, WP_H, L.qkv_w, L.qkv_b, s.qkv, 3 * WP_H, M, 3 * WP_H, WP_H, ETP_ACT_NONE, nullptr, nullptr, st));
    const char* q = reinterpret_cast<const char*>(s.qkv);
    const size_t es = dtype_size(dt);
    ETP_TRY(ring_attn_fwd(dt, q, 3 * WP_H, q + WP_H * es, 3 * WP_H, q + 2 * WP_H * es, 3 * WP_H, s.ctx, WP_H, B, WP_NEIGHBOR, 0.125f, st));
    ETP_TRY(wp_linear(w, ETP_F32, s.ctx, WP_H, L.o_w, L.o_b, s.s, WP_H, M, WP_H, WP_H, ETP_ACT_NONE, nullptr, s.xf, st));
    ETP_TRY(ln_fwd_s(dt, s.s, w->pf(L.ln1_g), w->pf(L.ln1_b), s.af, dt == ETP_BF16 ? s.at : nullptr, s.stats, M, WP_H, WP_LN_EPS, st));
    ETP_TRY(wp_linear(w, dt, s.at, WP_H, L.i_w, L.i_b, s.h, WP_I, M, WP_I, WP_H, ETP_ACT_GELU, s.z, nullptr, st));
    ETP_TRY(wp_linear(w, ETP_F32, s.h, WP_I, L.d_w, L.d_b, s.s, WP_H, M, WP_H, WP_I, ETP_ACT_NONE, nullptr, s.af, st));
    ETP_TRY(ln_fwd_s(dt, s.s, w->pf(L.ln2_g), w->pf(L.ln2_b), s.xf, dt == ETP_BF16 ? s.xt : nullptr, s.stats, M, WP_H, WP_LN_EPS, st));
  }
  ETP_TRY(wp_linear(w, dt, s.xt, WP_H, w->c1_w, w->c1_b, s.r, WP_H, M, WP_H, WP_H, ETP_ACT_RELU, nullptr, nullptr, st));
  ETP_TRY(wp_linear(w, ETP_F32, s.r, WP_H, w->c2_w, w->c2_b, s.raw, WP_OUT, M, WP_OUT, WP_H, ETP_ACT_NONE, nullptr, nullptr, st));
  return waypoint_roll(s.raw, logits, B, st);
}

}  // extern "C"
