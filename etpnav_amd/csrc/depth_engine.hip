// DD-PPO ResNet-50 depth encoder engine: VlnResnetDepthEncoder.forward (vlnce_baselines/models/encoders/resnet_encoders.py:13-107, i.e.
// habitat-lab's rl/ddppo/policy/resnet.py and resnet_policy.py::ResNetEncoder with baseplanes 32, ngroups 16, resnet50, no input
// normalisation, spatial_output False) over one flat parameter arena, as a chain of the library's GEMM launches and the kernels of
// depth.hip.  Forward only: the encoder is frozen.  The image size S, the base planes bp (groups = bp / 2) and the four block counts are
// parameters of the engine (the shipped network: 256, 32, [3, 4, 6, 3]).
//
//   pre   = conv7x7s2(avg_pool2(depth))                     [N, S/4, S/4, bp] fp32                  depth_stem
//   x     = maxpool3x3s2(relu(GN(pre)))                     [N, S/8, S/8, bp]                       gn_stats, gn_apply, maxpool3x3s2
//   block: a = relu(GN(x . W0^T));  b = relu(GN(rows3x3(a, stride) . W3^T));  c = b . W6^T          3 x (GEMM, gn_stats), conv_rows
//          x = relu(GN(c) + identity),  identity = x or GN(rows1x1(x, stride) . Wd^T)               gn_apply folds the downsample's norm
//   out   = relu(GN1(rows3x3(x) . Wc^T)) as NCHW fp32       [N, Cc, S/64, S/64]
//
// Activations are NHWC in the operand dtype, every product writes fp32 (the GroupNorm input), every GroupNorm computes in fp32 and rounds
// once.  Launches per call: 4 + sum over blocks (10; the first block of layer1 12, of layers 2-4 13) + 4 = 19 + 10 x blocks (179 for
// [3, 4, 6, 3]), whatever N is; three more (copies) while a probe buffer is installed.
#include <string.h>

#include <string>
#include <vector>

#include "arena.h"
#include "kernels.h"

namespace etp {
struct DepthConv { int w, g, b, cin, cout, k, stride; };
struct DepthBlock { DepthConv c[3]; DepthConv down; bool has_down; };
constexpr int DP_MAX_BLOCKS = 24;
constexpr float DP_GN_EPS = 1e-5f;
}  // namespace etp

struct etp_depth : etp::ArenaEngine {
  int S, bp, ng, blocks[4], n_blocks, fs, Cc;
  etp::DepthConv stem, comp;
  etp::DepthBlock block[etp::DP_MAX_BLOCKS];
  int block_layer[etp::DP_MAX_BLOCKS];
  float* probe = nullptr;
  etp_depth() { copy_in_f32 = true; }          // the packed copy is the GEMM operand in either dtype
};

namespace etp {

// "<conv>.weight", "<norm>.weight", "<norm>.bias": one bias-free convolution and its GroupNorm.  region 0 = GEMM matrices (packed copy),
// 1 = everything the kernels read as fp32 (the stem's 7x7 weight included)
static DepthConv dp_conv(etp_depth* w, const std::string& conv, const std::string& norm, int cin, int cout, int k, int stride, int region) {
  DepthConv c;
  c.cin = cin; c.cout = cout; c.k = k; c.stride = stride;
  c.w = w->table.add(conv + ".weight", region, {cout, cin, k, k});
  c.g = w->table.add(norm + ".weight", 1, {cout});
  c.b = w->table.add(norm + ".bias", 1, {cout});
  return c;
}

// state-dict order of habitat's ResNetEncoder: backbone.conv1, backbone.layer1..4 (per block convs.0 .. convs.7, then downsample),
// compression
static void dp_layout(etp_depth* w) {
  const int bp = w->bp;
  w->stem = dp_conv(w, "backbone.conv1.0", "backbone.conv1.1", 1, bp, 7, 2, 1);
  int inplanes = bp, nb = 0;
  for (int l = 0; l < 4; ++l) {
    const int planes = bp << l, stride = l == 0 ? 1 : 2;
    for (int i = 0; i < w->blocks[l]; ++i) {
      const std::string p = "backbone.layer" + std::to_string(l + 1) + "." + std::to_string(i);
      DepthBlock& B = w->block[nb];
      w->block_layer[nb++] = l;
      const int s = i == 0 ? stride : 1;
      B.c[0] = dp_conv(w, p + ".convs.0", p + ".convs.1", inplanes, planes, 1, 1, 0);
      B.c[1] = dp_conv(w, p + ".convs.3", p + ".convs.4", planes, planes, 3, s, 0);
      B.c[2] = dp_conv(w, p + ".convs.6", p + ".convs.7", planes, planes * 4, 1, 1, 0);
      B.has_down = i == 0;          // stride != 1 or inplanes != 4 planes: true for the first block of every layer (bp != 4 bp in layer1)
      if (B.has_down) B.down = dp_conv(w, p + ".downsample.0", p + ".downsample.1", inplanes, planes * 4, 1, s, 0);
      inplanes = planes * 4;
    }
  }
  w->n_blocks = nb;
  w->comp = dp_conv(w, "compression.0", "compression.1", inplanes, w->Cc, 3, 1, 0);
  w->table.layout(2);
}

// the ONE scratch plan of etp_depth_fwd / etp_depth_fwd_views (NULL base: sizes only); element counts come from a walk over the network
struct DepthScratch { void* x0; void* x1; void* a1; void* a2; void* rows; float* pre; float* pre2; float* st; float* st2; size_t bytes; };
static long conv_out(int H, int k, int stride) { return (H + 2 * ((k - 1) / 2) - k) / stride + 1; }
static DepthScratch dp_plan(const etp_depth* w, void* base, long N) {
  const size_t es = dtype_size(w->dtype);
  long H = w->S / 4, act = N * H * H * w->bp, mid = 0, rows = 0, pre = act;
  H = w->S / 8;
  auto mx = [](long& a, long b) { if (b > a) a = b; };
  for (int i = 0; i < w->n_blocks; ++i) {
    const DepthBlock& B = w->block[i];
    const long Ho = conv_out(H, 3, B.c[1].stride);
    mx(act, N * H * H * B.c[0].cin);
    mx(mid, N * H * H * B.c[0].cout);
    mx(pre, N * H * H * B.c[0].cout);
    mx(rows, N * Ho * Ho * 9 * B.c[1].cin);
    mx(pre, N * Ho * Ho * B.c[2].cout);
    if (B.has_down && B.down.stride == 2) mx(rows, N * Ho * Ho * B.down.cin);
    mx(act, N * Ho * Ho * B.c[2].cout);
    H = Ho;
  }
  mx(rows, N * H * H * 9 * w->comp.cin);
  mx(pre, N * H * H * w->comp.cout);
  Bump b(base);
  const int G = w->ng > 1 ? w->ng : 1;
  DepthScratch s;
  s.x0 = b.take(act * es);                  // block input / output, alternating (operand dtype, NHWC)
  s.x1 = b.take(act * es);
  s.a1 = b.take(mid * es);                  // after the first and the second convolution of a block
  s.a2 = b.take(mid * es);
  s.rows = b.take(rows * es);               // im2col rows of the 3x3 convolutions / gathered rows of the strided downsample
  s.pre = (float*)b.take(pre * 4);          // pre-norm product (fp32)
  s.pre2 = (float*)b.take(pre * 4);         // the downsample branch's pre-norm product
  s.st = (float*)b.take((size_t)N * G * 2 * 4);
  s.st2 = (float*)b.take((size_t)N * G * 2 * 4);
  s.bytes = b.off;
  return s;
}

static int dp_gemm(const etp_depth* w, const void* X, int wi, float* Y, long M, int N, int K, hipStream_t st) {
  GemmArgs g = base_args();
  g.A = X; g.lda = K; g.B = w->pw(wi); g.ldb = K; g.C = Y; g.ldc = N;
  g.M = (int)M; g.N = N; g.K = K;
  g.act = ETP_ACT_NONE;
  return launch_gemm(w->dtype, ETP_F32, 0, 0, g, 1, st);
}

// pre [n Ho Ho, cout] fp32 = conv(X [n, H, H, cin]);  stats = its GroupNorm statistics.  -> Ho through *Hout
static int dp_conv_stats(const etp_depth* w, const DepthConv& c, const void* X, int n, int H, int groups, const DepthScratch& s, float* pre,
                         float* stats, int* Hout, hipStream_t st) {
  const int Ho = (int)conv_out(H, c.k, c.stride);
  const void* A = X;
  int K = c.cin;
  if (c.k == 3 || c.stride == 2) {
    ETP_TRY(conv_rows(w->dtype, X, s.rows, n, H, H, c.cin, c.k, c.stride, st));
    A = s.rows;
    K = c.k * c.k * c.cin;
  }
  ETP_TRY(dp_gemm(w, A, c.w, pre, (long)n * Ho * Ho, c.cout, K, st));
  ETP_TRY(gn_stats(pre, stats, n, Ho * Ho, c.cout, groups, DP_GN_EPS, st));
  *Hout = Ho;
  return ETP_OK;
}

static int dp_probe(const etp_depth* w, const void* act, long offset, long n, hipStream_t st) {
  if (w->dtype == ETP_BF16) return cast_bf16_to_f32(act, w->probe + offset, n, 1.0f, st);
  return copy_f32(reinterpret_cast<const float*>(act), w->probe + offset, n, st);
}

static int dp_forward(etp_depth* w, const void* const* views, int n_views, int B, float* out, void* ws, hipStream_t st) {
  const int dt = w->dtype, S = w->S, bp = w->bp, ng = w->ng;
  const long N = (long)B * n_views;
  ETP_REQUIRE(N * S * S * bp * 9 / 64 < (1L << 31), "too many images for one call (the im2col rows must stay below 2^31 elements)");
  const int n = (int)N;
  const DepthScratch s = dp_plan(w, ws, N);
  int H = S / 4;
  ETP_TRY(depth_stem(views, n_views, B, S, bp, w->pf(w->stem.w), s.pre, st));
  ETP_TRY(gn_stats(s.pre, s.st, n, H * H, bp, ng, DP_GN_EPS, st));
  ETP_TRY(gn_apply(dt, s.pre, s.st, w->pf(w->stem.g), w->pf(w->stem.b), 0, nullptr, nullptr, nullptr, nullptr, 1, 0, s.x1, n, H * H, bp, ng, st));
  ETP_TRY(maxpool3x3s2(dt, s.x1, s.x0, n, H, H, bp, st));
  H = S / 8;
  void *x = s.x0, *y = s.x1;
  long poff = 0;
  if (w->probe) { ETP_TRY(dp_probe(w, x, poff, N * H * H * bp, st)); poff += N * H * H * bp; }
  for (int i = 0; i < w->n_blocks; ++i) {
    const DepthBlock& Bk = w->block[i];
    int H0, Ho, H2;
    ETP_TRY(dp_conv_stats(w, Bk.c[0], x, n, H, ng, s, s.pre, s.st, &H0, st));
    ETP_TRY(gn_apply(dt, s.pre, s.st, w->pf(Bk.c[0].g), w->pf(Bk.c[0].b), 0, nullptr, nullptr, nullptr, nullptr, 1, 0, s.a1, n, H0 * H0,
                     Bk.c[0].cout, ng, st));
    ETP_TRY(dp_conv_stats(w, Bk.c[1], s.a1, n, H0, ng, s, s.pre, s.st, &Ho, st));
    ETP_TRY(gn_apply(dt, s.pre, s.st, w->pf(Bk.c[1].g), w->pf(Bk.c[1].b), 0, nullptr, nullptr, nullptr, nullptr, 1, 0, s.a2, n, Ho * Ho,
                     Bk.c[1].cout, ng, st));
    ETP_TRY(dp_conv_stats(w, Bk.c[2], s.a2, n, Ho, ng, s, s.pre, s.st, &H2, st));
    if (Bk.has_down) {
      int Hd;
      ETP_TRY(dp_conv_stats(w, Bk.down, x, n, H, ng, s, s.pre2, s.st2, &Hd, st));
      ETP_TRY(gn_apply(dt, s.pre, s.st, w->pf(Bk.c[2].g), w->pf(Bk.c[2].b), 2, s.pre2, s.st2, w->pf(Bk.down.g), w->pf(Bk.down.b), 1, 0, y, n,
                       Ho * Ho, Bk.c[2].cout, ng, st));
    } else {
      ETP_TRY(gn_apply(dt, s.pre, s.st, w->pf(Bk.c[2].g), w->pf(Bk.c[2].b), 1, x, nullptr, nullptr, nullptr, 1, 0, y, n, Ho * Ho,
                       Bk.c[2].cout, ng, st));
    }
    H = Ho;
    void* t = x; x = y; y = t;
    const bool last_of_layer1 = w->block_layer[i] == 0 && (i + 1 == w->n_blocks || w->block_layer[i + 1] != 0);
    if (w->probe && last_of_layer1) { ETP_TRY(dp_probe(w, x, poff, N * H * H * Bk.c[2].cout, st)); poff += N * H * H * Bk.c[2].cout; }
  }
  if (w->probe) ETP_TRY(dp_probe(w, x, poff, N * H * H * w->comp.cin, st));
  int Hc;
  ETP_TRY(dp_conv_stats(w, w->comp, x, n, H, 1, s, s.pre, s.st, &Hc, st));
  return gn_apply(dt, s.pre, s.st, w->pf(w->comp.g), w->pf(w->comp.b), 0, nullptr, nullptr, nullptr, nullptr, 1, 1, out, n, Hc * Hc, w->Cc, 1,
                  st);
}

}  // namespace etp

using namespace etp;

extern "C" {

etp_depth* etp_depth_create(int dtype, int image_size, int base_planes, const int* blocks) {
  if (dtype != ETP_F32 && dtype != ETP_BF16) { set_error("etp_depth_create: dtype must be ETP_F32 or ETP_BF16"); return nullptr; }
  if (image_size < 64 || image_size > 256 || image_size % 64 != 0) {
    set_error("etp_depth_create: image_size must be a multiple of 64 in 64 .. 256");
    return nullptr;
  }
  if (base_planes != 16 && base_planes != 32) { set_error("etp_depth_create: base_planes must be 16 or 32"); return nullptr; }
  if (!blocks) { set_error("etp_depth_create: null block counts"); return nullptr; }
  for (int l = 0; l < 4; ++l)
    if (blocks[l] < 1 || blocks[l] > 6) { set_error("etp_depth_create: each block count must be in 1 .. 6"); return nullptr; }
  etp_depth* w = new etp_depth();
  w->dtype = dtype; w->S = image_size; w->bp = base_planes; w->ng = base_planes / 2;
  for (int l = 0; l < 4; ++l) w->blocks[l] = blocks[l];
  w->fs = image_size / 64;                                           // int((S // 2) / 32)
  w->Cc = (int)((2048.0 / (w->fs * w->fs)) + 0.5);                   // round(2048 / fs^2): 2048, 512, 228, 128
  dp_layout(w);
  return w;
}
void etp_depth_destroy(etp_depth* w) { delete w; }
int etp_depth_param_count(const etp_depth* w) { return w ? w->table.size() : 0; }
int etp_depth_param_info(const etp_depth* w, int i, etp_depth_tensor_info* out) {
  ETP_REQUIRE(w && out && i >= 0 && i < w->table.size(), "bad index");
  w->table.fill(i, out);
  return ETP_OK;
}
int64_t etp_depth_arena_elems(const etp_depth* w) { return w ? w->table.total : 0; }
int64_t etp_depth_matrix_elems(const etp_depth* w) { return w ? w->table.n_matrix : 0; }
int etp_depth_out_channels(const etp_depth* w) { return w ? w->Cc : 0; }
int etp_depth_bind(etp_depth* w, float* params, void* packed) {
  return bind_arenas(__func__, w, params, packed, "null engine / params / packed");
}
int etp_depth_refresh_weights(etp_depth* w, etp_stream_t stream) {
  ETP_REQUIRE(w && w->P, "engine not bound");
  char* pk = reinterpret_cast<char*>(w->Wc);
  const size_t es = dtype_size(w->dtype);
  for (const ParamEntry& p : w->table.e)
    if (p.region == 0)
      ETP_TRY(depth_pack(w->dtype, w->P + p.offset, pk + p.offset * es, (int)p.shape[0], (int)p.shape[1], (int)(p.shape[2] * p.shape[3]),
                         (hipStream_t)stream));
  return ETP_OK;
}
int64_t etp_depth_ws_bytes(const etp_depth* w, int N) {
  if (!w || N <= 0) return 0;
  return (int64_t)dp_plan(w, nullptr, N).bytes;
}
int etp_depth_set_probe(etp_depth* w, float* probe) {
  ETP_REQUIRE(w != nullptr, "null engine");
  ETP_REQUIRE((uintptr_t)probe % 16 == 0, "probe buffer must be 16-byte aligned");
  w->probe = probe;
  return ETP_OK;
}

int etp_depth_fwd(etp_depth* w, const float* depth, int N, float* out, void* ws, etp_stream_t stream) {
  ETP_REQUIRE(w && w->P && depth && out && ws && N > 0, "bad arguments (engine bound? null pointer? N <= 0?)");
  ETP_REQUIRE(((uintptr_t)depth | (uintptr_t)out) % 16 == 0 && (uintptr_t)ws % 256 == 0,
              "depth / out must be 16-byte aligned, ws 256-byte aligned");
  const void* one[1] = {depth};
  return dp_forward(w, one, 1, N, out, ws, (hipStream_t)stream);
}
int etp_depth_fwd_views(etp_depth* w, const void* const* views, int B, float* out, void* ws, etp_stream_t stream) {
  ETP_REQUIRE(w && w->P && views && out && ws && B > 0, "bad arguments (engine bound? null pointer? B <= 0?)");
  for (int a = 0; a < 12; ++a) ETP_REQUIRE(views[a] != nullptr && (uintptr_t)views[a] % 16 == 0, "12 non-null, 16-byte aligned view tensors");
  ETP_REQUIRE((uintptr_t)out % 16 == 0 && (uintptr_t)ws % 256 == 0, "out must be 16-byte aligned, ws 256-byte aligned");
  return dp_forward(w, views, 12, B, out, ws, (hipStream_t)stream);
}

}  // extern "C"
