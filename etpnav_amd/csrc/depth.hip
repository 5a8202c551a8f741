// The kernels the DD-PPO ResNet-50 depth encoder needs beside the library's GEMM (depth_engine.hip).  Activations are NHWC: a pixel's
// channels are contiguous, so a 1x1 convolution is a plain NT product over [N H W, Cin] and a 3x3 one is the same over im2col rows.
//
//   depth_stem_kernel<BP>     depth views [.., S, S, 1] fp32 -> 2x2 average pool -> 7x7 stride-2 pad-3 convolution (Cin = 1: 49 taps, no
//                             GEMM) -> pre-norm [N, S/4, S/4, BP] fp32; with 12 view tensors the clockwise reorder of
//                             Policy_ViewSelection_ETP.py:182-190 is the slot table (resnet_encoders.py:86-93, habitat resnet.py conv1)
//   gn_stats_kernel           per (image, group) mean and 1 / sqrt(var + eps) of an fp32 NHWC tensor, two passes around a pivot
//   gn_apply_kernel<T>        y = (x - mean) rstd gamma + beta (+ residual: a finished tensor, or a second pre-norm tensor with its own
//                             statistics) (+ ReLU), rounded once; NHWC in the operand dtype or NCHW fp32
//   maxpool3x3s2_kernel<T>    NHWC, pad 1; taps outside the image are skipped (-inf padding)
//   conv_rows_kernel          im2col: NHWC -> rows [N Ho Wo, k k C], columns (ky, kx, c), zeros outside the image; k 1|3, stride 1|2
//   depth_pack_kernel<T>      [Cout, Cin, k, k] fp32 -> [Cout, k, k, Cin] in the operand dtype (the GEMM-ready weight copy)
//
// All are HBM- or latency-bound: 16-byte accesses where the layout allows, plain vector stores, no atomics, fixed summation orders (a
// second run gives the same bits).  The file is compiled without floating-point contraction (build.py): tests/depth_ref.py restates the
// stem's and the statistics' schedules operation by operation.
#include <string.h>

#include "kernels.h"

namespace etp {

constexpr int DEPTH_GRID_CAP = 4096;
constexpr int GN_MAX_C = 2048, GN_MAX_G = 64;

struct DepthViews {             // passed by value: up to 12 view tensors and, per output slot of an episode, the view that fills it
  const float* p[12];
  int view_of_slot[12];
  int n_views;                  // 1: one [N, S, S, 1] tensor, identity slots; 12: one [B, S, S, 1] tensor per view
};

// One workgroup per 8x8 tile of output pixels (grid-stride).  The tile needs 21x21 pooled pixels (7 + 2 * 7 per axis), which the
// workgroup pools from the raw view into LDS ((a + b) + (c + d)) * 0.25, zeros outside the pooled image (the convolution's padding).
// Thread t owns pixel (t / 32, (t / 4) % 8) and BP / 4 consecutive channels; its sum runs over the 49 taps in (ky, kx) order, one
// fused multiply-add per tap: acc = fma(x, w, acc).
template <int BP>
__global__ __launch_bounds__(256) void depth_stem_kernel(DepthViews vw, const float* __restrict__ wgt, float* __restrict__ out, int n_img,
                                                         int S) {
  constexpr int CPT = BP / 4;
  __shared__ float wl[49 * BP];       // [tap][channel]
  __shared__ float tile[21 * 21];
  for (int i = threadIdx.x; i < 49 * BP; i += 256) wl[i] = wgt[(i % BP) * 49 + i / BP];
  const int P = S / 2, Ho = S / 4, TT = Ho / 8;
  const int px = (threadIdx.x >> 2) & 7, py = threadIdx.x >> 5, cq = threadIdx.x & 3;
  const long n_tiles = (long)n_img * TT * TT;
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int img = (int)(t / (TT * TT)), rem = (int)(t % (TT * TT)), ty = rem / TT, tx = rem % TT;
    const int ep = img / vw.n_views, slot = img % vw.n_views;
    int view = 0;
#pragma unroll
    for (int a = 0; a < 12; ++a) view = slot == a ? vw.view_of_slot[a] : view;
    const float* base = vw.p[0];
#pragma unroll
    for (int a = 1; a < 12; ++a) base = view == a ? vw.p[a] : base;
    const float* src = base + (long)ep * S * S;
    __syncthreads();                  // the previous tile is consumed (first trip: the weights are in LDS)
    for (int i = threadIdx.x; i < 21 * 21; i += 256) {
      const int gy = ty * 16 - 3 + i / 21, gx = tx * 16 - 3 + i % 21;
      float v = 0.f;
      if (gy >= 0 && gy < P && gx >= 0 && gx < P) {
        const float2 a = *reinterpret_cast<const float2*>(src + (long)(2 * gy) * S + 2 * gx);       // 8-byte aligned: S and 2 gx are even
        const float2 b = *reinterpret_cast<const float2*>(src + (long)(2 * gy + 1) * S + 2 * gx);
        v = ((a.x + a.y) + (b.x + b.y)) * 0.25f;
      }
      tile[i] = v;
    }
    __syncthreads();
    float acc[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) acc[j] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const float xv = tile[(py * 2 + ky) * 21 + px * 2 + kx];
        const float* wp = wl + (ky * 7 + kx) * BP + cq * CPT;
#pragma unroll
        for (int j = 0; j < CPT; ++j) acc[j] = fmaf(xv, wp[j], acc[j]);
      }
    float* dst = out + (((long)img * Ho + ty * 8 + py) * Ho + tx * 8 + px) * BP + cq * CPT;
#pragma unroll
    for (int j = 0; j < CPT; j += 4) *reinterpret_cast<float4*>(dst + j) = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
  }
}

// One workgroup of 1024 threads per image (grid-stride), two passes over its [HW, C] block, both around a value the data supplies:
//   pass 0: s = sum (x - pivot_g), pivot_g = the group's first element  ->  mean_g = pivot_g + s / n
//   pass 1: q = sum (x - mean_g)^2                                       ->  rstd_g = 1 / sqrt(q / n + eps)        n = HW C / G
// (a constant group gives s = 0 and q = 0 exactly, hence y = beta exactly).  Thread (r, q) = (t / Qc, t % Qc) sums pixels r, r + R, ... of
// channel quad q in order (Qc = C / 4 quads -- one chunk for every C the launcher admits --, R = 1024 / Qc whole pixel rows per trip,
// every load 16 bytes of a contiguous row); the R partials of a channel are added in order of r; the channels of a group are added
// lane-strided by one wavefront and its butterfly.  No atomics: the order is fixed by (HW, C, G) alone.
constexpr int GN_NT = 1024;
__global__ __launch_bounds__(GN_NT) void gn_stats_kernel(const float* __restrict__ x, float* __restrict__ stats, int n_img, int HW, int C,
                                                         int G, float eps) {
  __shared__ float part[4 * GN_NT];
  __shared__ float chs[GN_MAX_C];
  __shared__ float gmean[GN_MAX_G];
  const int Q = C / 4, cg = C / G, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float n = (float)((long)HW * cg);
  for (int img = blockIdx.x; img < n_img; img += gridDim.x) {
    const float* xi = x + (long)img * HW * C;
    for (int pass = 0; pass < 2; ++pass) {
      for (int q0 = 0; q0 < Q; q0 += GN_NT) {
        const int Qc = Q - q0 < GN_NT ? Q - q0 : GN_NT, R = GN_NT / Qc, r = threadIdx.x / Qc, q = threadIdx.x % Qc;
        if (r < R) {
          const int c0 = (q0 + q) * 4;
          float s0, s1, s2, s3;
          if (pass == 0) {
            s0 = xi[(c0 / cg) * cg]; s1 = xi[((c0 + 1) / cg) * cg]; s2 = xi[((c0 + 2) / cg) * cg]; s3 = xi[((c0 + 3) / cg) * cg];
          } else {
            s0 = gmean[c0 / cg]; s1 = gmean[(c0 + 1) / cg]; s2 = gmean[(c0 + 2) / cg]; s3 = gmean[(c0 + 3) / cg];
          }
          float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
          for (int p = r; p < HW; p += R) {
            const float4 v = *reinterpret_cast<const float4*>(xi + (long)p * C + c0);
            const float d0 = v.x - s0, d1 = v.y - s1, d2 = v.z - s2, d3 = v.w - s3;
            if (pass == 0) { a0 += d0; a1 += d1; a2 += d2; a3 += d3; }
            else { a0 += d0 * d0; a1 += d1 * d1; a2 += d2 * d2; a3 += d3 * d3; }
          }
          *reinterpret_cast<float4*>(part + (r * Qc + q) * 4) = make_float4(a0, a1, a2, a3);
        }
        __syncthreads();
        for (int ch = threadIdx.x; ch < Qc * 4; ch += GN_NT) {
          float s = 0.f;
          for (int rr = 0; rr < R; ++rr) s += part[rr * Qc * 4 + ch];
          chs[q0 * 4 + ch] = s;
        }
        __syncthreads();
      }
      for (int g = wave; g < G; g += GN_NT / 64) {
        float s = 0.f;
        for (int c = lane; c < cg; c += 64) s += chs[g * cg + c];
        s = wave_sum(s);
        if (lane == 0) {
          if (pass == 0) {
            const float m = xi[g * cg] + s / n;
            gmean[g] = m;
            stats[((long)img * G + g) * 2] = m;
          } else {
            stats[((long)img * G + g) * 2 + 1] = 1.0f / sqrtf(s / n + eps);
          }
        }
      }
      __syncthreads();
    }
  }
}

struct GnApplyArgs {
  const float* x; const float* stats; const float* gamma; const float* beta;
  int res_kind;                 // 0 none, 1 `res` is a finished tensor in the operand dtype, 2 `x2` is pre-norm fp32 with stats2 / gamma2 / beta2
  const void* res; const float* x2; const float* stats2; const float* gamma2; const float* beta2;
  int relu, nchw;
  void* out;
  long n_pix;                   // N HW
  int HW, C, G;
};

__device__ __forceinline__ float gn_norm(float v, const float* __restrict__ stats, long sg, float gm, float bt) {
  return ((v - stats[sg * 2]) * stats[sg * 2 + 1]) * gm + bt;
}

// 4 consecutive channels of one pixel per thread and trip.  Every step is one rounded fp32 operation, the residual is added in fp32, the
// result is rounded once to the output type.
template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(GnApplyArgs a) {
  const int Q = a.C / 4, cg = a.C / a.G;
  const long total = a.n_pix * Q;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long pix = i / Q;
    const int c0 = (int)(i % Q) * 4;
    const long img = pix / a.HW;
    float v[4];
    load4(a.x + i * 4, v);
    const float4 gm = *reinterpret_cast<const float4*>(a.gamma + c0), bt = *reinterpret_cast<const float4*>(a.beta + c0);
    v[0] = gn_norm(v[0], a.stats, img * a.G + c0 / cg, gm.x, bt.x);
    v[1] = gn_norm(v[1], a.stats, img * a.G + (c0 + 1) / cg, gm.y, bt.y);
    v[2] = gn_norm(v[2], a.stats, img * a.G + (c0 + 2) / cg, gm.z, bt.z);
    v[3] = gn_norm(v[3], a.stats, img * a.G + (c0 + 3) / cg, gm.w, bt.w);
    if (a.res_kind == 1) {
      float r[4];
      load4(reinterpret_cast<const T*>(a.res) + i * 4, r);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += r[e];
    } else if (a.res_kind == 2) {
      float r[4];
      load4(a.x2 + i * 4, r);
      const float4 g2 = *reinterpret_cast<const float4*>(a.gamma2 + c0), b2 = *reinterpret_cast<const float4*>(a.beta2 + c0);
      v[0] += gn_norm(r[0], a.stats2, img * a.G + c0 / cg, g2.x, b2.x);
      v[1] += gn_norm(r[1], a.stats2, img * a.G + (c0 + 1) / cg, g2.y, b2.y);
      v[2] += gn_norm(r[2], a.stats2, img * a.G + (c0 + 2) / cg, g2.z, b2.z);
      v[3] += gn_norm(r[3], a.stats2, img * a.G + (c0 + 3) / cg, g2.w, b2.w);
    }
    if (a.relu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
    }
    if (a.nchw) {
      float* o = reinterpret_cast<float*>(a.out) + (img * a.C + c0) * a.HW + pix % a.HW;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[(long)e * a.HW] = v[e];
    } else {
      store4(reinterpret_cast<T*>(a.out) + i * 4, v);
    }
  }
}

// MaxPool2d(3, stride 2, pad 1) on NHWC: 4 channels of one output pixel per thread and trip.  Taps outside the image are skipped, which is
// -inf padding (the window's centre is always inside, so every output has at least one tap); behind the ReLU, 0 padding gives the same.
template <typename T>
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const T* __restrict__ x, T* __restrict__ out, long n_img, int H, int W, int C) {
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, Q = C / 4;
  const long total = n_img * Ho * Wo * Q;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c0 = (int)(i % Q) * 4;
    long pix = i / Q;
    const int ox = (int)(pix % Wo);
    pix /= Wo;
    const int oy = (int)(pix % Ho);
    const long img = pix / Ho;
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int iy = oy * 2 - 1 + ky, ix = ox * 2 - 1 + kx;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
          float v[4];
          load4(x + ((img * H + iy) * W + ix) * C + c0, v);
#pragma unroll
          for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
        }
      }
    store4(out + i * 4, m);
  }
}

// im2col in 16-byte chunks (4 fp32 or 8 bf16 channels): chunk i of the output is copied from the input or zero
__global__ __launch_bounds__(256) void conv_rows_kernel(const uint4* __restrict__ x, uint4* __restrict__ out, long n_img, int H, int W,
                                                        int CQ, int k, int stride) {
  const int pad = (k - 1) / 2, Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const long total = n_img * Ho * Wo * k * k * CQ;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int cq = (int)(i % CQ);
    long rest = i / CQ;
    const int tap = (int)(rest % (k * k));
    rest /= k * k;
    const int ox = (int)(rest % Wo);
    rest /= Wo;
    const int oy = (int)(rest % Ho);
    const long img = rest / Ho;
    const int iy = oy * stride - pad + tap / k, ix = ox * stride - pad + tap % k;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[((img * H + iy) * W + ix) * CQ + cq];
    out[i] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void depth_pack_kernel(const float* __restrict__ src, T* __restrict__ dst, int Cout, int Cin, int kk) {
  const long total = (long)Cout * Cin * kk;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ci = (int)(i % Cin), tap = (int)((i / Cin) % kk);
    const long co = i / ((long)Cin * kk);
    Elem<T>::st(dst + i, src[(co * Cin + ci) * kk + tap]);
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
static bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }
static bool depth_size_ok(int S) { return S >= 64 && S <= 256 && S % 64 == 0; }
static int grid_for(long work_items) {
  const long blocks = (work_items + 255) / 256;
  return (int)(blocks < 1 ? 1 : blocks < DEPTH_GRID_CAP ? blocks : DEPTH_GRID_CAP);
}
constexpr long LIMIT31 = 1L << 31;

int depth_stem(const void* const* views, int n_views, int B, int S, int bp, const float* weight, float* out, hipStream_t st) {
  ETP_REQUIRE(views != nullptr && weight != nullptr && out != nullptr, "null pointer");
  ETP_REQUIRE(n_views == 1 || n_views == 12, "1 tensor [N, S, S, 1] or 12 view tensors [B, S, S, 1]");
  ETP_REQUIRE(depth_size_ok(S), "image size must be a multiple of 64 in 64 .. 256");
  ETP_REQUIRE(bp == 16 || bp == 32, "base_planes must be 16 or 32");
  ETP_REQUIRE(B > 0 && (long)B * n_views * (S / 4) * (S / 4) * bp < LIMIT31, "batch size must be positive and the output below 2^31 elements");
  ETP_REQUIRE(aligned16(out) && aligned16(weight), "weight / out must be 16-byte aligned");
  DepthViews vw;
  memset(&vw, 0, sizeof(vw));
  vw.n_views = n_views;
  for (int a = 0; a < 12; ++a) {
    const void* p = views[a < n_views ? a : 0];
    ETP_REQUIRE(p != nullptr, "null view tensor");
    ETP_REQUIRE(aligned16(p), "view tensors must be 16-byte aligned");
    vw.p[a] = reinterpret_cast<const float*>(p);
  }
  // view a of every episode goes to slot (12 - a) % 12 (Policy_ViewSelection_ETP.py:182-190)
  for (int a = 0; a < n_views; ++a) vw.view_of_slot[(n_views - a) % n_views] = a;
  const int n_img = B * n_views, TT = S / 32;
  const long n_tiles = (long)n_img * TT * TT;
  const int grid = (int)(n_tiles < DEPTH_GRID_CAP ? n_tiles : DEPTH_GRID_CAP);
  if (bp == 16) ETP_LAUNCH((depth_stem_kernel<16>), dim3(grid), dim3(256), 0, st, vw, weight, out, n_img, S);
  else ETP_LAUNCH((depth_stem_kernel<32>), dim3(grid), dim3(256), 0, st, vw, weight, out, n_img, S);
  ETP_CHECK_LAUNCH("depth_stem");
  return ETP_OK;
}

static int gn_dims_ok(int N, int HW, int C, int G) {
  ETP_REQUIRE(N > 0 && HW > 0, "image and pixel counts must be positive");
  ETP_REQUIRE(C > 0 && C % 4 == 0 && C <= GN_MAX_C, "channels must be a multiple of 4, at most 2048");
  ETP_REQUIRE(G > 0 && G <= GN_MAX_G && C % G == 0, "groups must divide the channels, at most 64");
  ETP_REQUIRE((long)N * HW * C < LIMIT31 && (long)HW * C < (1L << 24), "tensor too large (N HW C below 2^31, HW C below 2^24)");
  return ETP_OK;
}

int gn_stats(const float* x, float* stats, int N, int HW, int C, int G, float eps, hipStream_t st) {
  ETP_REQUIRE(x && stats, "null pointer");
  ETP_REQUIRE(aligned16(x) && aligned16(stats), "operands must be 16-byte aligned");
  ETP_TRY(gn_dims_ok(N, HW, C, G));
  ETP_LAUNCH(gn_stats_kernel, dim3(N < DEPTH_GRID_CAP ? N : DEPTH_GRID_CAP), dim3(GN_NT), 0, st, x, stats, N, HW, C, G, eps);
  ETP_CHECK_LAUNCH("gn_stats");
  return ETP_OK;
}

int gn_apply(int dtype, const float* x, const float* stats, const float* gamma, const float* beta, int res_kind, const void* res,
             const float* stats2, const float* gamma2, const float* beta2, int relu, int nchw, void* out, int N, int HW, int C, int G,
             hipStream_t st) {
  ETP_REQUIRE(dtype == ETP_F32 || dtype == ETP_BF16, "dtype must be ETP_F32 or ETP_BF16");
  ETP_REQUIRE(x && stats && gamma && beta && out, "null pointer");
  ETP_REQUIRE(res_kind >= 0 && res_kind <= 2, "res_kind is 0 (none), 1 (finished tensor) or 2 (pre-norm tensor with its own statistics)");
  ETP_REQUIRE(res_kind == 0 || res != nullptr, "a residual needs its tensor");
  ETP_REQUIRE(res_kind != 2 || (stats2 && gamma2 && beta2), "a pre-norm residual needs its statistics, gamma and beta");
  ETP_REQUIRE(aligned16(x) && aligned16(stats) && aligned16(gamma) && aligned16(beta) && aligned16(out) && aligned16(res) &&
                  aligned16(stats2) && aligned16(gamma2) && aligned16(beta2),
              "operands must be 16-byte aligned");
  ETP_TRY(gn_dims_ok(N, HW, C, G));
  GnApplyArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.stats = stats; a.gamma = gamma; a.beta = beta; a.res_kind = res_kind;
  a.res = res_kind == 1 ? res : nullptr;
  a.x2 = res_kind == 2 ? reinterpret_cast<const float*>(res) : nullptr;
  a.stats2 = stats2; a.gamma2 = gamma2; a.beta2 = beta2; a.relu = relu != 0; a.nchw = nchw != 0; a.out = out;
  a.n_pix = (long)N * HW; a.HW = HW; a.C = C; a.G = G;
  const int grid = grid_for(a.n_pix * (C / 4));
  if (dtype == ETP_BF16) ETP_LAUNCH((gn_apply_kernel<bf16_t>), dim3(grid), dim3(256), 0, st, a);
  else ETP_LAUNCH((gn_apply_kernel<float>), dim3(grid), dim3(256), 0, st, a);
  ETP_CHECK_LAUNCH("gn_apply");
  return ETP_OK;
}

int maxpool3x3s2(int dtype, const void* x, void* out, int N, int H, int W, int C, hipStream_t st) {
  ETP_REQUIRE(dtype == ETP_F32 || dtype == ETP_BF16, "dtype must be ETP_F32 or ETP_BF16");
  ETP_REQUIRE(x && out, "null pointer");
  ETP_REQUIRE(aligned16(x) && aligned16(out), "operands must be 16-byte aligned");
  ETP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "positive sizes, channels a multiple of 8");
  ETP_REQUIRE((long)N * H * W * C < LIMIT31, "tensor too large (N H W C must stay below 2^31)");
  const long items = (long)N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * (C / 4);
  if (dtype == ETP_BF16)
    ETP_LAUNCH((maxpool3x3s2_kernel<bf16_t>), dim3(grid_for(items)), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)out, (long)N, H, W, C);
  else ETP_LAUNCH((maxpool3x3s2_kernel<float>), dim3(grid_for(items)), dim3(256), 0, st, (const float*)x, (float*)out, (long)N, H, W, C);
  ETP_CHECK_LAUNCH("maxpool3x3s2");
  return ETP_OK;
}

int conv_rows(int dtype, const void* x, void* out, int N, int H, int W, int C, int k, int stride, hipStream_t st) {
  ETP_REQUIRE(dtype == ETP_F32 || dtype == ETP_BF16, "dtype must be ETP_F32 or ETP_BF16");
  ETP_REQUIRE(x && out, "null pointer");
  ETP_REQUIRE(aligned16(x) && aligned16(out), "operands must be 16-byte aligned");
  ETP_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2), "kernel size 1 or 3, stride 1 or 2");
  ETP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "positive sizes, channels a multiple of 8");
  const int pad = (k - 1) / 2, Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  ETP_REQUIRE((long)N * H * W * C < LIMIT31 && (long)N * Ho * Wo * k * k * C < LIMIT31, "tensor too large (input and rows must stay below 2^31 elements)");
  const int CQ = C / (dtype == ETP_BF16 ? 8 : 4);
  const long items = (long)N * Ho * Wo * k * k * CQ;
  ETP_LAUNCH(conv_rows_kernel, dim3(grid_for(items)), dim3(256), 0, st, (const uint4*)x, (uint4*)out, (long)N, H, W, CQ, k, stride);
  ETP_CHECK_LAUNCH("conv_rows");
  return ETP_OK;
}

int depth_pack(int dtype, const float* src, void* dst, int Cout, int Cin, int kk, hipStream_t st) {
  const int grid = grid_for((long)Cout * Cin * kk);
  if (dtype == ETP_BF16) ETP_LAUNCH((depth_pack_kernel<bf16_t>), dim3(grid), dim3(256), 0, st, src, (bf16_t*)dst, Cout, Cin, kk);
  else ETP_LAUNCH((depth_pack_kernel<float>), dim3(grid), dim3(256), 0, st, src, (float*)dst, Cout, Cin, kk);
  ETP_CHECK_LAUNCH("depth_pack");
  return ETP_OK;
}

}  // namespace etp

using namespace etp;

extern "C" {

int etp_depth_stem(const void* const* views, int n_views, int B, int S, int base_planes, const float* weight, float* out,
                   etp_stream_t stream) {
  return depth_stem(views, n_views, B, S, base_planes, weight, out, (hipStream_t)stream);
}
int etp_gn_stats(const float* x, float* stats, int N, int HW, int C, int groups, float eps, etp_stream_t stream) {
  return gn_stats(x, stats, N, HW, C, groups, eps, (hipStream_t)stream);
}
int etp_gn_apply(int dtype, const float* x, const float* stats, const float* gamma, const float* beta, int res_kind, const void* res,
                 const float* stats2, const float* gamma2, const float* beta2, int relu, int nchw, void* out, int N, int HW, int C,
                 int groups, etp_stream_t stream) {
  return gn_apply(dtype, x, stats, gamma, beta, res_kind, res, stats2, gamma2, beta2, relu, nchw, out, N, HW, C, groups,
                  (hipStream_t)stream);
}
int etp_maxpool3x3s2(int dtype, const void* x, void* out, int N, int H, int W, int C, etp_stream_t stream) {
  return maxpool3x3s2(dtype, x, out, N, H, W, C, (hipStream_t)stream);
}
int etp_conv_rows(int dtype, const void* x, void* out, int N, int H, int W, int C, int k, int stride, etp_stream_t stream) {
  return conv_rows(dtype, x, out, N, H, W, C, k, stride, (hipStream_t)stream);
}

}  // extern "C"
