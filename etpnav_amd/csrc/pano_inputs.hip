// The panorama encoder's inputs from the waypoint head's candidate table and the two view encoders' outputs, in one launch.
//
// Replaces, per rollout step, the end of ETP.forward(mode='waypoint') (vlnce_baselines/models/Policy_ViewSelection_ETP.py:289-342: the
// turn back to counter-clockwise, the two average pools, the per-episode candidate gathers and angle features) followed by
// RLTrainer._vp_feature_variable (vlnce_baselines/ss_trainer_ETP.py:308-342: candidate views first, then the panorama views no
// candidate fell into, padded).  Everything is a pure function of rgb_embedding [12B, Frgb] and depth_embedding [12B, C, HW] (both
// clockwise, as the encoders emit them) and the int32 candidate table, so no host decision sits between the two calls.
//
// One wavefront per output row (b, v), the row idiom of row.h / pano_store.hip with the width a run-time value: each lane owns groups
// of 4 consecutive columns 256 apart (16-byte accesses); Frgb is any multiple of 4, so row.h's Row<NCH> of whole 256-column chunks
// does not fit.  Every wave reads its episode's count and angles for itself (at most max_pred uniform loads) and derives the 12-bit
// mask of candidate views, the view length and every malformed condition as bit arithmetic -- no LDS, no barrier, no atomics, and
// nothing of a malformed episode is indexed.  No transcendental: the angle features come from two tables the host built once.
//
// The depth mean of one channel is ONE lane's sum over its HW values in index order (h = 0, 1, .., HW - 1) into one fp32 accumulator
// that starts at 0.0f, then one true division by (float)HW: the grid has no say in the bits.
#include "kernels.h"

namespace etp {

struct PanoCand {
  unsigned mask;   // bit i: a candidate falls into counter-clockwise view i
  int k, len, err;
};

// Policy_ViewSelection_ETP.py:313-314: the counter-clockwise view of heat-map angle a (0 .. 119)
__device__ __forceinline__ int pano_img_of(int a) {
  const int i = 12 - (a + 5) / 10;
  return i == 12 ? 0 : i;
}

// every lane of the wave returns the same record
__device__ __forceinline__ PanoCand pano_cand(const int32_t* count, const int32_t* angle, int b, int V, int max_pred) {
  PanoCand p;
  p.k = count[(long)b * max_pred];
  p.mask = 0;
  p.len = 0;
  p.err = (p.k < 0 || p.k > max_pred) ? ETP_PINPUTS_ERR_COUNT : 0;
  if (p.err) return p;
  for (int j = 0; j < p.k; ++j) {
    const int a = angle[(long)b * max_pred + j];
    if (a < 0 || a > 119) p.err |= ETP_PINPUTS_ERR_ANGLE;
    else p.mask |= 1u << pano_img_of(a);
  }
  p.len = p.k + 12 - __popc(p.mask);                     // two candidates of one view free that view once
  if (p.len > V) p.err |= ETP_PINPUTS_ERR_VIEWS;
  return p;
}

// grid ceil(B * V / 4) blocks of four waves: wave r writes row (b, v) = (r / V, r % V) of the three feature tensors and of nav_types;
// the wave of v == 0 also writes the episode's status, view length and candidate views
__global__ __launch_bounds__(256) void pano_inputs_kernel(const float* __restrict__ rgb, const float* __restrict__ dep,
                                                          const int32_t* __restrict__ count, const int32_t* __restrict__ angle,
                                                          const float* __restrict__ cand_tab, const float* __restrict__ pano_tab,
                                                          int B, int V, int max_pred, int Frgb, int C, int HW,
                                                          float* __restrict__ rgb_fts, float* __restrict__ dep_fts,
                                                          float* __restrict__ loc_fts, int64_t* __restrict__ nav_types,
                                                          int64_t* __restrict__ view_lens, int32_t* __restrict__ cand_img,
                                                          int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)B * V) return;
  const int b = (int)(row / V), v = (int)(row % V);
  const PanoCand p = pano_cand(count, angle, b, V, max_pred);
  if (v == 0 && lane == 0) status[b] = p.err;
  if (p.err) return;
  if (v == 0) {
    if (lane == 0) view_lens[b] = p.len;
    for (int j = lane; j < max_pred; j += 64)
      cand_img[(long)b * max_pred + j] = j < p.k ? pano_img_of(angle[(long)b * max_pred + j]) : -1;
  }
  float* drgb = rgb_fts + row * Frgb;
  float* ddep = dep_fts + row * C;
  if (v >= p.len) {                                        // padding: exact zeros (pad_tensors_wgrad / pad_sequence)
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane * 4; c < Frgb; c += 256) store4(drgb + c, z);
    for (int c = lane; c < C; c += 64) ddep[c] = 0.f;
    if (lane < 4) loc_fts[row * 4 + lane] = 0.f;
    if (lane == 0) nav_types[row] = 0;
    return;
  }
  int i;
  const float* loc;
  if (v < p.k) {                                           // candidate v, in table order
    const int a = angle[(long)b * max_pred + v];
    i = pano_img_of(a);
    loc = cand_tab + a * 4;
  } else {                                                 // the (v - k)-th view, counter-clockwise, that holds no candidate
    unsigned free = ~p.mask & 0xFFFu;
    for (int j = p.k; j < v; ++j) free &= free - 1;
    i = __ffs((int)free) - 1;
    loc = pano_tab + i * 4;
  }
  const long src = (long)b * 12 + (12 - i) % 12;           // counter-clockwise view i sits at clockwise slot (12 - i) % 12 (:201-213)
  const float* srgb = rgb + src * Frgb;
  for (int c = lane * 4; c < Frgb; c += 256) {
    float t[4];
    load4(srgb + c, t);
    store4(drgb + c, t);
  }
  const float* sdep = dep + src * C * HW;
  const float n = (float)HW;
  for (int c = lane; c < C; c += 64) {
    const float* x = sdep + (long)c * HW;
    float s = 0.f;
    if ((HW & 3) == 0) {
      for (int h = 0; h < HW; h += 4) {
        float t[4];
        load4(x + h, t);
        s += t[0]; s += t[1]; s += t[2]; s += t[3];
      }
    } else {
      for (int h = 0; h < HW; ++h) s += x[h];
    }
    ddep[c] = s / n;
  }
  if (lane < 4) loc_fts[row * 4 + lane] = loc[lane];
  if (lane == 0) nav_types[row] = v < p.k ? 1 : 0;
}

}  // namespace etp

extern "C" int etp_pano_inputs(const float* rgb_embedding, const float* depth_embedding, const int32_t* cand_count,
                               const int32_t* cand_angle, const float* cand_angle_tab, const float* pano_angle_tab, int B, int V,
                               int max_pred, int Frgb, int C, int HW, float* rgb_fts, float* dep_fts, float* loc_fts,
                               int64_t* nav_types, int64_t* view_lens, int32_t* cand_img, int32_t* status, etp_stream_t stream) {
  using namespace etp;
  ETP_REQUIRE(rgb_embedding && depth_embedding && cand_count && cand_angle && cand_angle_tab && pano_angle_tab && rgb_fts && dep_fts &&
                  loc_fts && nav_types && view_lens && cand_img && status, "null pointer");
  ETP_REQUIRE(B >= 1 && V >= 12 && max_pred >= 1, "B >= 1, V >= 12 (a panorama without candidates has 12 rows) and max_pred >= 1");
  ETP_REQUIRE(Frgb >= 4 && Frgb % 4 == 0 && C >= 1 && HW >= 1, "Frgb is a positive multiple of 4, C and HW are positive");
  ETP_REQUIRE((long)B * V <= 0x7FFFFFFFL / 4, "B * V rows exceed the grid");
  ETP_REQUIRE(((uintptr_t)rgb_embedding | (uintptr_t)depth_embedding | (uintptr_t)rgb_fts) % 16 == 0,
              "rgb_embedding, depth_embedding and rgb_fts must be 16-byte aligned");
  ETP_REQUIRE(((uintptr_t)nav_types | (uintptr_t)view_lens) % 8 == 0, "nav_types and view_lens must be 8-byte aligned");
  ETP_REQUIRE(((uintptr_t)cand_count | (uintptr_t)cand_angle | (uintptr_t)cand_angle_tab | (uintptr_t)pano_angle_tab | (uintptr_t)dep_fts |
               (uintptr_t)loc_fts | (uintptr_t)cand_img | (uintptr_t)status) % 4 == 0, "fp32 and int32 operands must be 4-byte aligned");
  const long rows = (long)B * V;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  ETP_LAUNCH(pano_inputs_kernel, grid, block, 0, (hipStream_t)stream, rgb_embedding, depth_embedding, cand_count, cand_angle,
             cand_angle_tab, pano_angle_tab, B, V, max_pred, Frgb, C, HW, rgb_fts, dep_fts, loc_fts, nav_types, view_lens, cand_img,
             status);
  ETP_CHECK_LAUNCH("pano_inputs");
  return ETP_OK;
}
