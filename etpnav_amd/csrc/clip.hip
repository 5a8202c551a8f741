// The four kernels the CLIP ViT-B/32 view encoder needs beside the library's GEMM / LayerNorm / attention launches (clip_engine.hip):
//
//   clip_patch_rows_kernel<T>   uint8 views [.., S, S, 3] -> normalised patch rows [N (S/32)^2, 3072] in the operand dtype, columns in
//                               conv1.weight's own (c, ky, kx) order; with 12 view tensors the clockwise reorder of
//                               Policy_ViewSelection_ETP.py:182-190 is the slot table (resnet_encoders.py:264-275, clip/model.py conv1)
//   clip_tokens_kernel          class token + patch product + positional embedding, then ln_pre -> fp32 residual stream
//   quick_gelu_kernel<T>        v * sigmoid(1.702 v) in place (clip/model.py QuickGELU)
//   clip_cls_ln_kernel<T>       ln_post of the class-token row of every image -> [N, 768] in the operand dtype
//
// All four are HBM-bound: 16-byte accesses, plain vector stores, no atomics.  The file is compiled without floating-point contraction
// (build.py): the pixel normalisation promises torch's fp32 bits, one correctly rounded operation per step.
#include <string.h>

#include "kernels.h"
#include "row.h"

namespace etp {

constexpr int CLIP_W = 768, CLIP_PATCH = 32, CLIP_PK = 3 * CLIP_PATCH * CLIP_PATCH;   // 3072 columns of a patch row
constexpr int CLIP_NCH = CLIP_W / 256;
constexpr int CLIP_GRID_CAP = 2048;

struct ClipViews {              // passed by value: up to 12 view tensors and, per output slot of an episode, the view that fills it
  const uint8_t* p[12];
  int view_of_slot[12];
  int n_views;                  // 1: one [N, S, S, 3] tensor, identity slots; 12: one [B, S, S, 3] tensor per view
};

// (float(x) / 255 - mean[c]) / std[c], each operation rounded in fp32 (transforms.ConvertImageDtype + Normalize, resnet_encoders.py:264-267)
__device__ __forceinline__ float clip_pixel(int v, int c) {
  const float mean = c == 0 ? 0.48145466f : c == 1 ? 0.4578275f : 0.40821073f;
  const float sd = c == 0 ? 0.26862954f : c == 1 ? 0.26130258f : 0.27577711f;
  return ((float)v / 255.0f - mean) / sd;
}

// One workgroup per patch (grid-stride): thread t owns image row ky = t / 8 of the patch and its pixels kx0 = 4 (t % 8) .. + 3, i.e. 12
// consecutive input bytes, and writes 4 consecutive columns in each of the three channel planes of the output row.
template <typename T>
__global__ __launch_bounds__(256) void clip_patch_rows_kernel(ClipViews vw, T* __restrict__ out, int n_img, int S) {
  __shared__ float lut[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) lut[i] = clip_pixel(i & 255, i >> 8);
  __syncthreads();
  const int G = S / CLIP_PATCH, PP = G * G;
  const int ky = threadIdx.x >> 3, kx0 = (threadIdx.x & 7) * 4;
  const long n_patch = (long)n_img * PP;
  for (long patch = blockIdx.x; patch < n_patch; patch += gridDim.x) {
    const int img = (int)(patch / PP), pp = (int)(patch % PP), py = pp / G, px = pp % G;
    const int ep = img / vw.n_views, slot = img % vw.n_views;
    int view = 0;
#pragma unroll
    for (int a = 0; a < 12; ++a) view = slot == a ? vw.view_of_slot[a] : view;
    const uint8_t* base = vw.p[0];
#pragma unroll
    for (int a = 1; a < 12; ++a) base = view == a ? vw.p[a] : base;
    const uint8_t* src = base + ((long)ep * S * S + (long)(py * CLIP_PATCH + ky) * S + px * CLIP_PATCH + kx0) * 3;
    const uint3 w = *reinterpret_cast<const uint3*>(src);          // 4-byte aligned: S % 32 == 0, kx0 % 4 == 0
    const uint32_t words[3] = {w.x, w.y, w.z};
    int byte[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) byte[i] = (words[i >> 2] >> (8 * (i & 3))) & 255;
    T* dst = out + patch * CLIP_PK + ky * CLIP_PATCH + kx0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float o[4] = {lut[c * 256 + byte[c]], lut[c * 256 + byte[3 + c]], lut[c * 256 + byte[6 + c]], lut[c * 256 + byte[9 + c]]};
      store4(dst + c * CLIP_PATCH * CLIP_PATCH, o);
    }
  }
}

// LayerNorm of one row held in registers, on the schedule of ln_fwd_s_kernel (norm.hip): 4 NCH lane-sequential adds, the wave butterfly
template <typename T>
__device__ __forceinline__ void clip_row_ln(Row<CLIP_NCH>& r, const float* __restrict__ gamma, const float* __restrict__ beta,
                                            T* __restrict__ y, int lane, float eps) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CLIP_NCH; ++c) s += r.v[c][0] + r.v[c][1] + r.v[c][2] + r.v[c][3];
  const float mean = wave_sum(s) * (1.0f / CLIP_W);
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < CLIP_NCH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) { r.v[c][e] -= mean; q += r.v[c][e] * r.v[c][e]; }
  const float rstd = rsqrtf(wave_sum(q) * (1.0f / CLIP_W) + eps);
#pragma unroll
  for (int c = 0; c < CLIP_NCH; ++c) {
    const int col = c * 256 + lane * 4;
    const float4 gm = *reinterpret_cast<const float4*>(gamma + col);
    const float4 bt = *reinterpret_cast<const float4*>(beta + col);
    const float o[4] = {r.v[c][0] * rstd * gm.x + bt.x, r.v[c][1] * rstd * gm.y + bt.y, r.v[c][2] * rstd * gm.z + bt.z,
                        r.v[c][3] * rstd * gm.w + bt.w};
    store4(y + col, o);
  }
}

// x[n T + 0] = ln_pre(class_embedding + pos[0]);  x[n T + 1 + p] = ln_pre(prod[n P + p] + pos[1 + p])   (clip/model.py
// VisionTransformer.forward).  One wavefront per row.
__global__ __launch_bounds__(256) void clip_tokens_kernel(const float* __restrict__ prod, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* __restrict__ x, int n_img, int T,
                                                          float eps) {
  const int lane = threadIdx.x & 63;
  const long rows = (long)n_img * T;
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * 4) {
    const long img = row / T;
    const int t = (int)(row % T);
    Row<CLIP_NCH> a, b;
    row_load(a, t == 0 ? cls : prod + (img * (T - 1) + (t - 1)) * CLIP_W, lane);
    row_load(b, pos + (long)t * CLIP_W, lane);
    row_add(a, b);
    clip_row_ln(a, gamma, beta, x + row * CLIP_W, lane, eps);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void clip_cls_ln_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, T* __restrict__ out, int n_img, int Tk,
                                                          float eps) {
  const int lane = threadIdx.x & 63;
  for (long img = (long)blockIdx.x * 4 + (threadIdx.x >> 6); img < n_img; img += (long)gridDim.x * 4) {
    Row<CLIP_NCH> a;
    row_load(a, x + img * Tk * CLIP_W, lane);
    clip_row_ln(a, gamma, beta, out + img * CLIP_W, lane, eps);
  }
}

// v * sigmoid(1.702 v) = v / (1 + exp(-1.702 v)):  t = 1.702 v;  e = v_exp_f32(t * -log2(e));  d = 1 + e;  r = v_rcp_f32(d);  y = v r.
// Three correctly rounded operations and two one-ulp instructions (tests/clip_ref.py counts them).  v = -inf: e = inf, r = 0, y = NaN;
// v = +inf: e = 0, r = 1, y = +inf -- what torch's x * sigmoid(1.702 x) gives.
__device__ __forceinline__ float quick_gelu(float v) {
  const float t = 1.702f * v;
  const float e = __builtin_amdgcn_exp2f(t * -1.4426950408889634f);
  return v * __builtin_amdgcn_rcpf(1.0f + e);
}

// 8 elements per thread and trip (16 bytes of bf16, 2 x 16 bytes of fp32); n % 8 == 0
template <typename T>
__global__ __launch_bounds__(256) void quick_gelu_kernel(T* __restrict__ x, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float a[4], b[4];
    load4(x + i * 8, a);
    load4(x + i * 8 + 4, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] = quick_gelu(a[e]); b[e] = quick_gelu(b[e]); }
    store4(x + i * 8, a);
    store4(x + i * 8 + 4, b);
  }
}
template <>
__global__ __launch_bounds__(256) void quick_gelu_kernel<bf16_t>(bf16_t* __restrict__ x, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const uint4 w = *reinterpret_cast<const uint4*>(x + i * 8);
    const uint32_t in[4] = {w.x, w.y, w.z, w.w};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o[e] = pack_bf16(quick_gelu(__uint_as_float(in[e] << 16)), quick_gelu(__uint_as_float(in[e] & 0xffff0000u)));
    *reinterpret_cast<uint4*>(x + i * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
static bool clip_size_ok(int S) { return S >= 32 && S <= 224 && S % 32 == 0; }
static bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

int clip_patch_rows(int dtype, const void* const* views, int n_views, int B, int S, void* out, hipStream_t st) {
  ETP_REQUIRE(dtype == ETP_F32 || dtype == ETP_BF16, "dtype must be ETP_F32 or ETP_BF16");
  ETP_REQUIRE(views != nullptr && out != nullptr, "null pointer");
  ETP_REQUIRE(n_views == 1 || n_views == 12, "1 tensor [N, S, S, 3] or 12 view tensors [B, S, S, 3]");
  ETP_REQUIRE(clip_size_ok(S), "image size must be a multiple of 32 in 32 .. 224");
  ETP_REQUIRE(B > 0 && (long)B * n_views <= (1L << 20), "batch size must be positive (at most 2^20 images)");
  ETP_REQUIRE(aligned16(out), "out must be 16-byte aligned");
  ClipViews vw;
  memset(&vw, 0, sizeof(vw));
  vw.n_views = n_views;
  for (int a = 0; a < 12; ++a) {
    const void* p = views[a < n_views ? a : 0];
    ETP_REQUIRE(p != nullptr, "null view tensor");
    ETP_REQUIRE(aligned16(p), "view tensors must be 16-byte aligned");
    vw.p[a] = reinterpret_cast<const uint8_t*>(p);
  }
  // view a of every episode goes to slot (12 - a) % 12 (Policy_ViewSelection_ETP.py:182-190)
  for (int a = 0; a < n_views; ++a) vw.view_of_slot[(n_views - a) % n_views] = a;
  const int G = S / CLIP_PATCH, n_img = B * n_views;
  const long n_patch = (long)n_img * G * G;
  const int grid = (int)(n_patch < CLIP_GRID_CAP ? n_patch : CLIP_GRID_CAP);
  if (dtype == ETP_BF16) ETP_LAUNCH((clip_patch_rows_kernel<bf16_t>), dim3(grid), dim3(256), 0, st, vw, (bf16_t*)out, n_img, S);
  else ETP_LAUNCH((clip_patch_rows_kernel<float>), dim3(grid), dim3(256), 0, st, vw, (float*)out, n_img, S);
  ETP_CHECK_LAUNCH("clip_patch_rows");
  return ETP_OK;
}

int clip_tokens(const float* prod, const float* cls, const float* pos, const float* gamma, const float* beta, float* x, int N, int S,
                float eps, hipStream_t st) {
  ETP_REQUIRE(prod && cls && pos && gamma && beta && x, "null pointer");
  ETP_REQUIRE(aligned16(prod) && aligned16(cls) && aligned16(pos) && aligned16(gamma) && aligned16(beta) && aligned16(x),
              "operands must be 16-byte aligned");
  ETP_REQUIRE(clip_size_ok(S), "image size must be a multiple of 32 in 32 .. 224");
  ETP_REQUIRE(N > 0 && N <= (1 << 20), "image count must be positive (at most 2^20)");
  const int T = (S / CLIP_PATCH) * (S / CLIP_PATCH) + 1;
  const long rows = (long)N * T, blocks = (rows + 3) / 4;
  const int grid = (int)(blocks < CLIP_GRID_CAP ? blocks : CLIP_GRID_CAP);
  ETP_LAUNCH(clip_tokens_kernel, dim3(grid), dim3(256), 0, st, prod, cls, pos, gamma, beta, x, N, T, eps);
  ETP_CHECK_LAUNCH("clip_tokens");
  return ETP_OK;
}

int clip_cls_ln(int dtype, const float* x, const float* gamma, const float* beta, void* out, int N, int S, float eps, hipStream_t st) {
  ETP_REQUIRE(dtype == ETP_F32 || dtype == ETP_BF16, "dtype must be ETP_F32 or ETP_BF16");
  ETP_REQUIRE(x && gamma && beta && out, "null pointer");
  ETP_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(out), "operands must be 16-byte aligned");
  ETP_REQUIRE(clip_size_ok(S), "image size must be a multiple of 32 in 32 .. 224");
  ETP_REQUIRE(N > 0 && N <= (1 << 20), "image count must be positive (at most 2^20)");
  const int T = (S / CLIP_PATCH) * (S / CLIP_PATCH) + 1;
  const int blocks = (N + 3) / 4, grid = blocks < CLIP_GRID_CAP ? blocks : CLIP_GRID_CAP;
  if (dtype == ETP_BF16) ETP_LAUNCH((clip_cls_ln_kernel<bf16_t>), dim3(grid), dim3(256), 0, st, x, gamma, beta, (bf16_t*)out, N, T, eps);
  else ETP_LAUNCH((clip_cls_ln_kernel<float>), dim3(grid), dim3(256), 0, st, x, gamma, beta, (float*)out, N, T, eps);
  ETP_CHECK_LAUNCH("clip_cls_ln");
  return ETP_OK;
}

int quick_gelu_inplace(int dtype, void* x, long n, hipStream_t st) {
  ETP_REQUIRE(dtype == ETP_F32 || dtype == ETP_BF16, "dtype must be ETP_F32 or ETP_BF16");
  ETP_REQUIRE(x != nullptr, "null pointer");
  ETP_REQUIRE(aligned16(x), "x must be 16-byte aligned");
  ETP_REQUIRE(n > 0 && n % 8 == 0, "element count must be a positive multiple of 8");
  const long n8 = n / 8, blocks = (n8 + 255) / 256;
  const int grid = (int)(blocks < CLIP_GRID_CAP ? blocks : CLIP_GRID_CAP);
  if (dtype == ETP_BF16) ETP_LAUNCH((quick_gelu_kernel<bf16_t>), dim3(grid), dim3(256), 0, st, (bf16_t*)x, n8);
  else ETP_LAUNCH((quick_gelu_kernel<float>), dim3(grid), dim3(256), 0, st, (float*)x, n8);
  ETP_CHECK_LAUNCH("quick_gelu");
  return ETP_OK;
}

}  // namespace etp

using namespace etp;

extern "C" {

int etp_clip_patch_rows(int dtype, const void* const* views, int n_views, int B, int S, void* out, etp_stream_t stream) {
  return clip_patch_rows(dtype, views, n_views, B, S, out, (hipStream_t)stream);
}
int etp_clip_tokens(const float* prod, const float* class_embedding, const float* pos, const float* gamma, const float* beta, float* x,
                    int N, int S, float eps, etp_stream_t stream) {
  return clip_tokens(prod, class_embedding, pos, gamma, beta, x, N, S, eps, (hipStream_t)stream);
}
int etp_quick_gelu(int dtype, void* x, int64_t n, etp_stream_t stream) { return quick_gelu_inplace(dtype, x, (long)n, (hipStream_t)stream); }
int etp_clip_cls_ln(int dtype, const float* x, const float* gamma, const float* beta, void* out, int N, int S, float eps,
                    etp_stream_t stream) {
  return clip_cls_ln(dtype, x, gamma, beta, out, N, S, eps, (hipStream_t)stream);
}

}  // extern "C"
