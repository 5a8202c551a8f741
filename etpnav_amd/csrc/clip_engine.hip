// CLIP ViT-B/32 view encoder engine: CLIPEncoder.forward (vlnce_baselines/models/encoders/resnet_encoders.py:244-278, i.e. OpenAI
// clip/model.py VisionTransformer.forward under encode_image) over one flat parameter arena, as a chain of the library's GEMM /
// LayerNorm / attention launches plus the four kernels of clip.hip.  Forward only: the encoder is frozen and in eval()
// (resnet_encoders.py:259-261).  Width 768, 12 heads, patch 32, output 512 are fixed; the image size S and the number of layers are
// parameters of the engine (ViT-B/32 itself: S = 224, 12 layers), T = (S / 32)^2 + 1 tokens per image.
//
//   rows   = normalise(uint8 views) as patch rows [N P, 3072]                resnet_encoders.py:264-275 (+ the clockwise reorder of
//                                                                            Policy_ViewSelection_ETP.py:182-190 in the 12-view form)
//   prod   = rows . conv1.weight^T                                           clip/model.py conv1 (stride = kernel = 32, no bias)
//   x      = ln_pre([class_embedding; prod] + positional_embedding)          [N T, 768] fp32
//   layers x:  q|k|v = ln_1(x) . in_proj_weight^T + in_proj_bias             one N = 2304 product
//              x'    = x + attention(q, k, v) . out_proj.weight^T + bias     12 heads x 64, no mask, alpha 1/8
//              x     = x' + c_proj(quick_gelu(c_fc(ln_2(x'))))
//   out    = ln_post(x[:, 0]) . proj                                         [N, 512] fp32
//
// The residual stream is fp32 in both modes and alternates between two buffers (a product never has R == C); `dtype` selects the
// GEMM / attention operand precision.  Launches per call: 1 + 1 + 1 + 8 x layers + 2 (101 for ViT-B/32), whatever N is; three more
// (copies) while a probe buffer is installed.
#include <string.h>

#include <string>
#include <vector>

#include "arena.h"
#include "kernels.h"

namespace etp {
struct ClipLayer { int qkv_w, qkv_b, o_w, o_b, ln1_g, ln1_b, fc_w, fc_b, pj_w, pj_b, ln2_g, ln2_b; };
constexpr int CL_W = 768, CL_I = 3072, CL_HEADS = 12, CL_PATCH = 32, CL_PK = 3072, CL_OUT = 512, CL_MAX_LAYERS = 12;
constexpr float CL_LN_EPS = 1e-5f;
}  // namespace etp

struct etp_clip : etp::ArenaEngine {
  int S, layers, T;
  int conv_w, cls, pos, proj, pre_g, pre_b, post_g, post_b;
  etp::ClipLayer layer[etp::CL_MAX_LAYERS];
  float* probe = nullptr;
};

namespace etp {


// state-dict order of OpenAI's VisionTransformer (own parameters first, then conv1, ln_pre, transformer, ln_post); region 0 = GEMM
// matrices (bf16 shadow), 1 = everything the kernels read as fp32
static void cl_layout(etp_clip* w) {
  w->cls = w->table.add("class_embedding", 1, {CL_W});
  w->pos = w->table.add("positional_embedding", 1, {w->T, CL_W});
  w->proj = w->table.add("proj", 0, {CL_W, CL_OUT});
  w->conv_w = w->table.add("conv1.weight", 0, {CL_W, 3, CL_PATCH, CL_PATCH});
  w->pre_g = w->table.add("ln_pre.weight", 1, {CL_W});
  w->pre_b = w->table.add("ln_pre.bias", 1, {CL_W});
  for (int l = 0; l < w->layers; ++l) {
    const std::string p = "transformer.resblocks." + std::to_string(l);
    ClipLayer& L = w->layer[l];
    L.qkv_w = w->table.add(p + ".attn.in_proj_weight", 0, {3 * CL_W, CL_W});
    L.qkv_b = w->table.add(p + ".attn.in_proj_bias", 1, {3 * CL_W});
    L.o_w = w->table.add(p + ".attn.out_proj.weight", 0, {CL_W, CL_W});
    L.o_b = w->table.add(p + ".attn.out_proj.bias", 1, {CL_W});
    L.ln1_g = w->table.add(p + ".ln_1.weight", 1, {CL_W});
    L.ln1_b = w->table.add(p + ".ln_1.bias", 1, {CL_W});
    L.fc_w = w->table.add(p + ".mlp.c_fc.weight", 0, {CL_I, CL_W});
    L.fc_b = w->table.add(p + ".mlp.c_fc.bias", 1, {CL_I});
    L.pj_w = w->table.add(p + ".mlp.c_proj.weight", 0, {CL_W, CL_I});
    L.pj_b = w->table.add(p + ".mlp.c_proj.bias", 1, {CL_W});
    L.ln2_g = w->table.add(p + ".ln_2.weight", 1, {CL_W});
    L.ln2_b = w->table.add(p + ".ln_2.bias", 1, {CL_W});
  }
  w->post_g = w->table.add("ln_post.weight", 1, {CL_W});
  w->post_b = w->table.add("ln_post.bias", 1, {CL_W});
  w->table.layout(2);
}

// the ONE scratch plan of etp_clip_fwd / etp_clip_fwd_views (NULL base: sizes only)
struct ClipScratch { void* rows; float* prod; float* xa; float* xb; void* xt; void* qkv; void* P; void* ctx; void* h; void* cls;
                     size_t bytes; };
static ClipScratch cl_plan(const etp_clip* w, void* base, long N) {
  const size_t es = dtype_size(w->dtype);
  const size_t T = w->T, M = (size_t)N * T, NP = (size_t)N * (T - 1), ldS = round_up(T, 8);
  Bump b(base);
  ClipScratch s;
  s.rows = b.take(NP * CL_PK * es);                   // normalised patch rows (operand dtype)
  s.prod = (float*)b.take(NP * CL_W * 4);             // conv1 product
  s.xa = (float*)b.take(M * CL_W * 4);                // residual stream (fp32), two buffers
  s.xb = (float*)b.take(M * CL_W * 4);
  s.xt = b.take(M * CL_W * es);                       // LayerNorm output = GEMM operand
  s.qkv = b.take(M * 3 * CL_W * es);
  s.P = b.take((size_t)N * CL_HEADS * T * ldS * es);  // attention probabilities / lse, whichever family runs
  s.ctx = b.take(M * CL_W * es);
  s.h = b.take(M * CL_I * es);
  s.cls = b.take((size_t)N * CL_W * es);
  s.bytes = b.off;
  return s;
}

static int cl_linear(const etp_clip* w, int c_dtype, const void* X, long ldx, int wi, int bi, void* Y, long ldy, long M, int N, int K,
                     const void* R, int tb, hipStream_t st) {
  GemmArgs g = base_args();
  g.A = X; g.lda = ldx; g.B = w->pw(wi); g.ldb = tb ? N : K; g.C = Y; g.ldc = ldy;
  g.M = (int)M; g.N = N; g.K = K;
  g.bias = bi >= 0 ? w->pf(bi) : nullptr;
  g.act = ETP_ACT_NONE; g.R = R; g.ldr = ldy;
  return launch_gemm(w->dtype, c_dtype, 0, tb, g, 1, st);
}

static int cl_forward(etp_clip* w, const void* const* views, int n_views, int B, float* out, void* ws, hipStream_t st) {
  const int dt = w->dtype, S = w->S, T = w->T;
  const long N = (long)B * n_views, M = N * T, NP = N * (T - 1);
  ETP_REQUIRE(M * CL_I < (1L << 31), "too many images for one call (rows x 3072 must stay below 2^31)");
  const size_t es = dtype_size(dt);
  const ClipScratch s = cl_plan(w, ws, N);
  ETP_TRY(clip_patch_rows(dt, views, n_views, B, S, s.rows, st));
  ETP_TRY(cl_linear(w, ETP_F32, s.rows, CL_PK, w->conv_w, -1, s.prod, CL_W, NP, CL_W, CL_PK, nullptr, 0, st));
  ETP_TRY(clip_tokens(s.prod, w->pf(w->cls), w->pf(w->pos), w->pf(w->pre_g), w->pf(w->pre_b), s.xa, (int)N, S, CL_LN_EPS, st));
  if (w->probe) ETP_TRY(copy_f32(s.xa, w->probe, M * CL_W, st));
  float* yf = dt == ETP_F32 ? (float*)s.xt : nullptr;      // the LayerNorm writes the operand copy only
  void* yt = dt == ETP_BF16 ? s.xt : nullptr;
  for (int l = 0; l < w->layers; ++l) {
    const ClipLayer& L = w->layer[l];
    ETP_TRY(ln_fwd_s(dt, s.xa, w->pf(L.ln1_g), w->pf(L.ln1_b), yf, yt, nullptr, (int)M, CL_W, CL_LN_EPS, st));
    ETP_TRY(cl_linear(w, dt, s.xt, CL_W, L.qkv_w, L.qkv_b, s.qkv, 3 * CL_W, M, 3 * CL_W, CL_W, nullptr, 0, st));
    const char* q = reinterpret_cast<const char*>(s.qkv);
    AttnBuf a{q, 3L * CL_W, q + CL_W * es, 3L * CL_W, q + 2 * CL_W * es, 3L * CL_W, (int)N, T, T, (int)round_up(T, 8), nullptr, 0, nullptr,
              nullptr, nullptr};
    ETP_TRY(attn_fwd_impl(dt, CL_HEADS, a, s.P, s.ctx, CL_W, 0.125f, st));
    ETP_TRY(cl_linear(w, ETP_F32, s.ctx, CL_W, L.o_w, L.o_b, s.xb, CL_W, M, CL_W, CL_W, s.xa, 0, st));
    ETP_TRY(ln_fwd_s(dt, s.xb, w->pf(L.ln2_g), w->pf(L.ln2_b), yf, yt, nullptr, (int)M, CL_W, CL_LN_EPS, st));
    ETP_TRY(cl_linear(w, dt, s.xt, CL_W, L.fc_w, L.fc_b, s.h, CL_I, M, CL_I, CL_W, nullptr, 0, st));
    ETP_TRY(quick_gelu_inplace(dt, s.h, M * CL_I, st));
    ETP_TRY(cl_linear(w, ETP_F32, s.h, CL_I, L.pj_w, L.pj_b, s.xa, CL_W, M, CL_W, CL_I, s.xb, 0, st));
    if (w->probe && l == 0) ETP_TRY(copy_f32(s.xa, w->probe + M * CL_W, M * CL_W, st));
  }
  if (w->probe) ETP_TRY(copy_f32(s.xa, w->probe + 2 * M * CL_W, M * CL_W, st));
  ETP_TRY(clip_cls_ln(dt, s.xa, w->pf(w->post_g), w->pf(w->post_b), s.cls, (int)N, S, CL_LN_EPS, st));
  return cl_linear(w, ETP_F32, s.cls, CL_W, w->proj, -1, out, CL_OUT, N, CL_OUT, CL_W, nullptr, 1, st);
}

}  // namespace etp

using namespace etp;

extern "C" {

etp_clip* etp_clip_create(int dtype, int image_size, int layers) {
  if (dtype != ETP_F32 && dtype != ETP_BF16) { set_error("etp_clip_create: dtype must be ETP_F32 or ETP_BF16"); return nullptr; }
  if (image_size < 32 || image_size > 224 || image_size % 32 != 0) {
    set_error("etp_clip_create: image_size must be a multiple of 32 in 32 .. 224");
    return nullptr;
  }
  if (layers < 1 || layers > CL_MAX_LAYERS) { set_error("etp_clip_create: layers must be in 1 .. 12"); return nullptr; }
  etp_clip* w = new etp_clip();
  w->dtype = dtype; w->S = image_size; w->layers = layers;
  w->T = (image_size / CL_PATCH) * (image_size / CL_PATCH) + 1;
  cl_layout(w);
  return w;
}
void etp_clip_destroy(etp_clip* w) { delete w; }
int etp_clip_param_count(const etp_clip* w) { return w ? w->table.size() : 0; }
int etp_clip_param_info(const etp_clip* w, int i, etp_clip_tensor_info* out) {
  ETP_REQUIRE(w && out && i >= 0 && i < w->table.size(), "bad index");
  w->table.fill(i, out);
  return ETP_OK;
}
int64_t etp_clip_arena_elems(const etp_clip* w) { return w ? w->table.total : 0; }
int64_t etp_clip_matrix_elems(const etp_clip* w) { return w ? w->table.n_matrix : 0; }
int etp_clip_bind(etp_clip* w, float* params, void* shadow) {
  return bind_arenas(__func__, w, params, shadow, "null engine / params");
}
int etp_clip_refresh_weights(etp_clip* w, etp_stream_t stream) {
  ETP_REQUIRE(w && w->P, "engine not bound");
  if (w->dtype != ETP_BF16) return ETP_OK;
  return cast_f32_to_bf16(w->P, w->Wc, w->table.n_matrix, (hipStream_t)stream);
}
int64_t etp_clip_ws_bytes(const etp_clip* w, int N) {
  if (!w || N <= 0) return 0;
  return (int64_t)cl_plan(w, nullptr, N).bytes;
}
int etp_clip_set_probe(etp_clip* w, float* probe) {
  ETP_REQUIRE(w != nullptr, "null engine");
  ETP_REQUIRE((uintptr_t)probe % 16 == 0, "probe buffer must be 16-byte aligned");
  w->probe = probe;
  return ETP_OK;
}

int etp_clip_fwd(etp_clip* w, const void* views, int N, float* out, void* ws, etp_stream_t stream) {
  ETP_REQUIRE(w && w->P && views && out && ws && N > 0, "bad arguments (engine bound? null pointer? N <= 0?)");
  ETP_REQUIRE(((uintptr_t)views | (uintptr_t)out) % 16 == 0 && (uintptr_t)ws % 256 == 0,
              "views / out must be 16-byte aligned, ws 256-byte aligned");
  const void* one[1] = {views};
  return cl_forward(w, one, 1, N, out, ws, (hipStream_t)stream);
}
int etp_clip_fwd_views(etp_clip* w, const void* const* views, int B, float* out, void* ws, etp_stream_t stream) {
  ETP_REQUIRE(w && w->P && views && out && ws && B > 0, "bad arguments (engine bound? null pointer? B <= 0?)");
  for (int a = 0; a < 12; ++a) ETP_REQUIRE(views[a] != nullptr && (uintptr_t)views[a] % 16 == 0, "12 non-null, 16-byte aligned view tensors");
  ETP_REQUIRE((uintptr_t)out % 16 == 0 && (uintptr_t)ws % 256 == 0, "out must be 16-byte aligned, ws 256-byte aligned");
  return cl_forward(w, views, 12, B, out, ws, (hipStream_t)stream);
}

}  // extern "C"
