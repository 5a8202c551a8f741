// Waypoint head (vlnce_baselines/waypoint_pred/*, models/Policy_ViewSelection_ETP.py:172-342): the two device pieces the GEMM,
// LayerNorm and epilogue kernels do not cover.  Forward only: the predictor is frozen and in eval() (ss_trainer_ETP.py:201-202).
//
//   ring_attn_fwd_kernel   the 12-token neighbourhood attention of waypoint_bert.py:49-90 under the mask of
//                          waypoint_pred/utils.py:90-102 (token i sees i-n .. i+n mod 12)
//   waypoint_tail_kernel   softmax over 1 440 cells, wrap to 122 angle rows, nms (waypoint_pred/utils.py:8-64), candidate
//                          extraction and the training-time regional re-sampling (Policy_ViewSelection_ETP.py:220-282)
//
// Compiled like the other row kernels: no SLP vectoriser, hence no packed fp32 (build.py NO_PACKED_FP32).
#include "common.h"
#include "kernels.h"

namespace etp {

constexpr int WP_TOK = 12;          // views per panorama = tokens per episode
constexpr int WP_HD = 64;           // head dimension
constexpr int WP_HPB = 4;           // heads per workgroup (one wave each)
constexpr int WP_ROW = WP_HD + 4;   // LDS row pitch in floats: 272 B keeps the 16-lane groups of ds_read_b128 on distinct banks

// --------------------------------------------------------------------------------------
// ctx[b, i, h] = sum_{o=-n..n} softmax_o(alpha q_i . k_{i+o}) v_{i+o}        indices mod 12
//
// The reference adds -10000 to the scores outside the window (waypoint_bert.py:184, :69); in fp32 exp(-10000 + d) is exactly 0,
// so those keys are left out instead: they are never read.
//
// One wave per (episode, head), four heads per workgroup, grid = B * 3.  The wave stages its head's K and V (12 x 64 each) in LDS as
// fp32.  Lane = (token t = lane / 4, quarter c = lane % 4): 16 of the 64 head dimensions of one query; lanes 48..63 idle.  A score is
// 16 FMAs per lane and two quad butterfly steps.  Two passes over the window so that no per-key value lives in a run-time-indexed
// register array (n is a run-time argument): pass 1 the row maximum, pass 2 the same scores again (bitwise), p = expf(s - m),
// l += p, acc += p v.  ctx = acc / l, rounded to T once at the store.  Everything in between is fp32; P is never rounded to bf16.
// --------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(WP_HPB * 64) void ring_attn_fwd_kernel(const T* __restrict__ Q, long ldq, const T* __restrict__ K,
                                                                    long ldk, const T* __restrict__ V, long ldv,
                                                                    T* __restrict__ ctx, long ldc, int n, float alpha) {
  __shared__ __attribute__((aligned(16))) float sK[WP_HPB][WP_TOK * WP_ROW];
  __shared__ __attribute__((aligned(16))) float sV[WP_HPB][WP_TOK * WP_ROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / (12 / WP_HPB), h = (blockIdx.x % (12 / WP_HPB)) * WP_HPB + wave;
  const long row0 = (long)b * WP_TOK;
  // stage K, V: 16 lanes x 4 elements = one row, four rows per step
  {
    const int r = lane >> 4, c4 = (lane & 15) * 4;
#pragma unroll
    for (int it = 0; it < WP_TOK / 4; ++it) {
      const int j = it * 4 + r;
      float kv[4], vv[4];
      load4(K + (row0 + j) * ldk + h * WP_HD + c4, kv);
      load4(V + (row0 + j) * ldv + h * WP_HD + c4, vv);
      *reinterpret_cast<float4*>(&sK[wave][j * WP_ROW + c4]) = make_float4(kv[0], kv[1], kv[2], kv[3]);
      *reinterpret_cast<float4*>(&sV[wave][j * WP_ROW + c4]) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    }
  }
  const int t = lane >> 2, c = lane & 3;
  const bool live = t < WP_TOK;
  const int tq = live ? t : 0;                      // idle lanes follow token 0 and store nothing
  float q[16];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v4[4];
    load4(Q + (row0 + tq) * ldq + h * WP_HD + c * 16 + e * 4, v4);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[e * 4 + i] = v4[i];
  }
  __syncthreads();
  const float* kh = sK[wave];
  const float* vh = sV[wave];
  auto score = [&](int j) {
    const float4* kr = reinterpret_cast<const float4*>(kh + j * WP_ROW + c * 16);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float4 k4 = kr[e];
      s = fmaf(q[e * 4 + 0], k4.x, s);
      s = fmaf(q[e * 4 + 1], k4.y, s);
      s = fmaf(q[e * 4 + 2], k4.z, s);
      s = fmaf(q[e * 4 + 3], k4.w, s);
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    return alpha * s;
  };
  float m = -INFINITY;
  for (int o = -n; o <= n; ++o) {
    int j = tq + o;
    j += j < 0 ? WP_TOK : 0;
    j -= j >= WP_TOK ? WP_TOK : 0;
    m = fmaxf(m, score(j));
  }
  float l = 0.f, acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int o = -n; o <= n; ++o) {
    int j = tq + o;
    j += j < 0 ? WP_TOK : 0;
    j -= j >= WP_TOK ? WP_TOK : 0;
    const float p = expf(score(j) - m);
    l += p;
    const float4* vr = reinterpret_cast<const float4*>(vh + j * WP_ROW + c * 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float4 v4 = vr[e];
      acc[e * 4 + 0] = fmaf(p, v4.x, acc[e * 4 + 0]);
      acc[e * 4 + 1] = fmaf(p, v4.y, acc[e * 4 + 1]);
      acc[e * 4 + 2] = fmaf(p, v4.z, acc[e * 4 + 2]);
      acc[e * 4 + 3] = fmaf(p, v4.w, acc[e * 4 + 3]);
    }
  }
  if (live) {
    T* out = ctx + (row0 + t) * ldc + h * WP_HD + c * 16;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float o4[4] = {acc[e * 4 + 0] / l, acc[e * 4 + 1] / l, acc[e * 4 + 2] / l, acc[e * 4 + 3] / l};
      store4(out + e * 4, o4);
    }
  }
}

int ring_attn_fwd(int dtype, const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* ctx, long ldc, int B,
                  int neighbor, float alpha, hipStream_t st) {
  ETP_REQUIRE(Q && K && V && ctx, "null pointer");
  ETP_REQUIRE(dtype == ETP_F32 || dtype == ETP_BF16, "bad dtype");
  ETP_REQUIRE(B > 0 && (long)B * (12 / WP_HPB) <= 0x7fffffffL, "B must be positive");
  ETP_REQUIRE(neighbor >= 0 && neighbor <= 5, "neighbor must be 0 .. 5 (waypoint_pred/utils.py:91)");
  const uintptr_t al = dtype == ETP_BF16 ? 8 : 16;
  ETP_REQUIRE(((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)ctx) % al == 0,
              "Q / K / V / ctx must be aligned to four elements (8 bytes bf16 / 16 bytes fp32)");
  ETP_REQUIRE(ldq >= 768 && ldk >= 768 && ldv >= 768 && ldc >= 768 && (ldq | ldk | ldv | ldc) % 4 == 0,
              "leading dimensions must be multiples of 4 and >= 768");
  const dim3 grid(B * (12 / WP_HPB)), block(WP_HPB * 64);
  if (dtype == ETP_BF16)
    ETP_LAUNCH(ring_attn_fwd_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)Q, ldq, (const bf16_t*)K, ldk, (const bf16_t*)V, ldv,
               (bf16_t*)ctx, ldc, neighbor, alpha);
  else
    ETP_LAUNCH(ring_attn_fwd_kernel<float>, grid, block, 0, st, (const float*)Q, ldq, (const float*)K, ldk, (const float*)V, ldv,
               (float*)ctx, ldc, neighbor, alpha);
  ETP_CHECK_LAUNCH("ring_attn_fwd");
  return ETP_OK;
}

// --------------------------------------------------------------------------------------
// Heat-map tail, one workgroup (256 threads) per episode; the wrapped 122 x 12 map lives in LDS three times: the probabilities
// (`pred`), the suppressed copy the argmax runs on (`supp`) and the output of nms (`outm`).
//
//   heat = softmax(logits[1440])                                  Policy_ViewSelection_ETP.py:220-227
//     max: per thread over its <= 6 cells, wave butterfly, 4 waves.  sum of expf(l - max): per thread serially over its cells
//     (5 additions), wave butterfly (6), the four wave sums serially (3): the longest addition chain is 14.  heat = e / sum.
//   wrap: row 0 = angle 119, rows 1..120 = angles 0..119, row 121 = angle 0                                  :228-232
//   max_pred rounds of nms (waypoint_pred/utils.py:37-64, sigma = (sigma_x, sigma_y)):
//     ix = argmax(supp), the lowest flat index among equal values (torch.max over a contiguous row); outm[ix] = pred[ix];
//     y_mu = float(ix) / 12 (a TRUE division: the centre on the angle axis is fractional), x_mu = ix % 12;
//     supp *= 1 - [min(|x - x_mu|, |x - x_mu + 12|) <= sigma_x  and  |y - y_mu| <= sigma_y]      (neighborhoods, utils.py:8-34)
//   drop rows 0 and 121 (:239), list the non-zero cells in row-major order (:304-305): a pick in a wrap row is lost, so an
//   episode can have fewer than max_pred candidates.
//   uniforms != NULL (:247-282): per candidate the softmax over the 10 x 12 logits of its image sector, taken from the logits
//   rolled back by 5, and an inverse-CDF draw: the first index whose inclusive prefix sum, added serially in index order, exceeds
//   u * total (total = the same serial sum).
// Plain vector stores only, no atomics.
// --------------------------------------------------------------------------------------
constexpr int WP_ANG = 120, WP_DST = 12, WP_CELLS = WP_ANG * WP_DST, WP_WCELLS = (WP_ANG + 2) * WP_DST, WP_MAXP = 8;

__global__ __launch_bounds__(256) void waypoint_tail_kernel(const float* __restrict__ logits, int max_pred, float sigma_x,
                                                            float sigma_y, const float* __restrict__ uniforms,
                                                            float* __restrict__ heat, float* __restrict__ nms_map,
                                                            int32_t* __restrict__ cand_count, int32_t* __restrict__ cand_angle,
                                                            int32_t* __restrict__ cand_dist, int32_t* __restrict__ cand_img_cw,
                                                            int32_t* __restrict__ cand_img_ccw, int32_t* __restrict__ samp_angle,
                                                            int32_t* __restrict__ samp_dist) {
  __shared__ float sL[WP_CELLS], pred[WP_WCELLS], supp[WP_WCELLS], outm[WP_WCELLS];
  __shared__ float sE[WP_MAXP][WP_ANG];      // regional exponentials, one row of 120 per candidate
  __shared__ float redf[4];
  __shared__ int redi[4];
  __shared__ int picks[WP_MAXP], cand[WP_MAXP], s_count;
  const int ep = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lg = logits + (long)ep * WP_CELLS;

  float mx = -INFINITY;
  for (int k = tid; k < WP_CELLS; k += 256) {
    const float v = lg[k];
    sL[k] = v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  if (lane == 0) redf[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
  __syncthreads();
  float sum = 0.f;
  for (int k = tid; k < WP_CELLS; k += 256) {
    const float e = expf(sL[k] - mx);
    pred[WP_DST + k] = e;                     // unnormalised for now
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) redf[wave] = sum;
  __syncthreads();
  sum = ((redf[0] + redf[1]) + redf[2]) + redf[3];
  for (int k = tid; k < WP_CELLS; k += 256) {
    const float p = pred[WP_DST + k] / sum;
    heat[(long)ep * WP_CELLS + k] = p;
    pred[WP_DST + k] = p;
    supp[WP_DST + k] = p;
    if (k < WP_DST) { pred[(WP_ANG + 1) * WP_DST + k] = p; supp[(WP_ANG + 1) * WP_DST + k] = p; }
    if (k >= WP_CELLS - WP_DST) { pred[k - (WP_CELLS - WP_DST)] = p; supp[k - (WP_CELLS - WP_DST)] = p; }
  }
  for (int k = tid; k < WP_WCELLS; k += 256) outm[k] = 0.f;
  __syncthreads();

  for (int r = 0; r < max_pred; ++r) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int k = tid; k < WP_WCELLS; k += 256) {           // ascending k: a strict > keeps the first of equal values
      const float v = supp[k];
      if (v > bv) { bv = v; bi = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { redf[wave] = bv; redi[wave] = bi; }
    __syncthreads();
    bv = redf[0]; bi = redi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (redf[w] > bv || (redf[w] == bv && redi[w] < bi)) { bv = redf[w]; bi = redi[w]; }
    if (bi >= WP_WCELLS) bi = 0;                            // a map of NaNs: every comparison fails; stay in bounds
    if (tid == 0) { outm[bi] = pred[bi]; picks[r] = bi; }
    const float y_mu = (float)bi / 12.0f, x_mu = (float)(bi % WP_DST);
    for (int k = tid; k < WP_WCELLS; k += 256) {
      const float yd = (float)(k / WP_DST) - y_mu;
      float xd = (float)(k % WP_DST) - x_mu;
      xd = fminf(fabsf(xd), fabsf(xd + (float)WP_DST));
      const float g = (fabsf(xd) <= sigma_x && fabsf(yd) <= sigma_y) ? 1.f : 0.f;
      supp[k] *= 1.f - g;
    }
    __syncthreads();
  }

  for (int k = tid; k < WP_CELLS; k += 256) {
    const float v = outm[WP_DST + k];
    nms_map[(long)ep * WP_CELLS + k] = v < 0.f ? 0.f : v;   // utils.py:63
  }
  if (tid == 0) {
    // the picks outside the wrap rows whose recorded value is non-zero, each cell once, in ascending flat index
    int cnt = 0;
    for (int r = 0; r < max_pred; ++r) {
      const int ix = picks[r];
      if (ix < WP_DST || ix >= (WP_ANG + 1) * WP_DST || !(outm[ix] != 0.f)) continue;
      const int cell = ix - WP_DST;
      int pos = 0;
      bool dup = false;
      for (int i = 0; i < cnt; ++i) {
        dup = dup || cand[i] == cell;
        pos += cand[i] < cell ? 1 : 0;
      }
      if (dup) continue;
      for (int i = cnt; i > pos; --i) cand[i] = cand[i - 1];
      cand[pos] = cell;
      ++cnt;
    }
    s_count = cnt;
    cand_count[ep] = cnt;
  }
  __syncthreads();
  const int count = s_count;
  if (tid < max_pred) {
    const long o = (long)ep * max_pred + tid;
    const bool on = tid < count;
    const int a = on ? cand[tid] / WP_DST : 0, d = on ? cand[tid] % WP_DST : 0;
    const int sec = (a + 5) / 10;
    cand_angle[o] = on ? a : -1;
    cand_dist[o] = on ? d : -1;
    cand_img_cw[o] = on ? sec % 12 : -1;
    cand_img_ccw[o] = on ? (12 - sec) % 12 : -1;
  }
  if (uniforms == nullptr) return;

  // regional re-sampling: wave w prepares candidates w and w + 4 (two cells per lane), thread c draws for candidate c
  for (int cidx = wave; cidx < count; cidx += 4) {
    const int sec = ((cand[cidx] / WP_DST + 5) / 10) % 12;
    const int base = sec * 10 - 5 + WP_ANG;                 // first logits row of the sector before the modulo
    const int k0 = lane, k1 = lane + 64;
    const float l0 = sL[((base + k0 / WP_DST) % WP_ANG) * WP_DST + k0 % WP_DST];
    const float l1 = k1 < WP_ANG ? sL[((base + k1 / WP_DST) % WP_ANG) * WP_DST + k1 % WP_DST] : -INFINITY;
    const float m = wave_max(fmaxf(l0, l1));
    sE[cidx][k0] = expf(l0 - m);
    if (k1 < WP_ANG) sE[cidx][k1] = expf(l1 - m);
  }
  __syncthreads();
  if (tid < max_pred) {
    const long o = (long)ep * max_pred + tid;
    int sa = -1, sd = -1;
    if (tid < count) {
      float total = 0.f;
      for (int k = 0; k < WP_ANG; ++k) total += sE[tid][k];
      const float target = uniforms[o] * total;
      float run = 0.f;
      int act = WP_ANG - 1;
      for (int k = 0; k < WP_ANG; ++k) {
        run += sE[tid][k];
        if (run > target) { act = k; break; }
      }
      const int sec = ((cand[tid] / WP_DST + 5) / 10) % 12;
      const int pointer = sec != 0 ? (sec - 1) * 10 + 5 : 0;   // Policy_ViewSelection_ETP.py:275-278
      sa = act / WP_DST + pointer;
      sd = act % WP_DST;
    }
    samp_angle[o] = sa;
    samp_dist[o] = sd;
  }
}

int waypoint_tail(const float* logits, int B, int max_pred, float sigma_x, float sigma_y, const float* uniforms, float* heat,
                  float* nms_map, int32_t* cand_count, int32_t* cand_angle, int32_t* cand_dist, int32_t* cand_img_cw,
                  int32_t* cand_img_ccw, int32_t* samp_angle, int32_t* samp_dist, hipStream_t st) {
  ETP_REQUIRE(logits && heat && nms_map && cand_count && cand_angle && cand_dist && cand_img_cw && cand_img_ccw, "null pointer");
  ETP_REQUIRE(uniforms == nullptr || (samp_angle && samp_dist), "uniforms need samp_angle and samp_dist");
  ETP_REQUIRE(B > 0, "B must be positive");
  ETP_REQUIRE(max_pred >= 1 && max_pred <= WP_MAXP, "max_pred must be 1 .. 8");
  ETP_REQUIRE(((uintptr_t)logits | (uintptr_t)heat | (uintptr_t)nms_map) % 16 == 0, "logits / heat / nms_map must be 16-byte aligned");
  ETP_REQUIRE(((uintptr_t)uniforms | (uintptr_t)cand_count | (uintptr_t)cand_angle | (uintptr_t)cand_dist | (uintptr_t)cand_img_cw |
               (uintptr_t)cand_img_ccw | (uintptr_t)samp_angle | (uintptr_t)samp_dist) % 4 == 0,
              "uniforms and the candidate tables must be 4-byte aligned");
  ETP_LAUNCH(waypoint_tail_kernel, dim3(B), dim3(256), 0, st, logits, max_pred, sigma_x, sigma_y, uniforms, heat, nms_map,
             cand_count, cand_angle, cand_dist, cand_img_cw, cand_img_ccw, samp_angle, samp_dist);
  ETP_CHECK_LAUNCH("waypoint_tail");
  return ETP_OK;
}

// HEATMAP_OFFSET (TRM_net.py:83-86): the classifier's [B*12, 120] rows are [B, 120, 12] angle x distance; rolling the angle axis by 5
// is a cyclic shift of each episode's 1 440 values by 60.
__global__ __launch_bounds__(256) void waypoint_roll_kernel(const float* __restrict__ in, float* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long ep = i / WP_CELLS;
  const int f = (int)(i - ep * WP_CELLS);
  out[i] = in[ep * WP_CELLS + (f + 5 * WP_DST) % WP_CELLS];
}
int waypoint_roll(const float* in, float* out, int B, hipStream_t st) {
  ETP_REQUIRE(in && out && in != out && B > 0, "bad arguments");
  const long n = (long)B * WP_CELLS;
  ETP_LAUNCH(waypoint_roll_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, n);
  ETP_CHECK_LAUNCH("waypoint_roll");
  return ETP_OK;
}

}  // namespace etp
