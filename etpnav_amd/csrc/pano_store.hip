// The embedding store's rows from the panorama encoder's output, and the way back.
//
// Replaces, per rollout step, the trainer's masked panorama mean (vlnce_baselines/ss_trainer_ETP.py:838-839), its candidate
// selection (:864-869) and the tensors GraphMap.update_graph keeps of them (vlnce_baselines/models/graph_utils.py:206,224,233):
// episode b's mean goes to row row_base[b] of the store, its j-th candidate view (nav_types == 1, in view order) to row
// row_base[b] + 1 + j.  DeviceGraphMaps / gather_rows read those rows; the backward turns the store's gradient into d pano_embeds.
//
// One wavefront per row, embed.hip's row idiom (row.h).  V <= 64, so lane v reads view v's mask and type and two ballots hold the
// episode: the view length, the candidates, a candidate's rank and every malformed condition are bit arithmetic that each wave
// repeats for itself -- no LDS, no barrier, no atomics, and nothing of a malformed episode is indexed.  The mean adds the unmasked
// views in view order into one accumulator per column, so the grid has no say in the bits.
#include "kernels.h"
#include "row.h"

namespace etp {

struct PanoViews {
  unsigned long long mask, cand;   // bit v: view v is unmasked / a candidate
  int len, err;
};

// every lane of the wave returns the same record; rows: the rows behind the store pointer
__device__ __forceinline__ PanoViews pano_views(const uint8_t* masks, const int64_t* nav_types, const int32_t* row_base,
                                                const int32_t* n_cand, int b, int V, int rows, int lane) {
  PanoViews p;
  const bool in = lane < V;
  p.mask = __ballot(in && masks[(long)b * V + lane] != 0);
  p.cand = __ballot(in && nav_types[(long)b * V + lane] == 1);
  p.len = __popcll(p.mask);
  const int k = __popcll(p.cand);
  const long base = row_base[b];
  p.err = (p.len == 0 ? ETP_PSTORE_ERR_EMPTY : 0) | ((p.cand & ~p.mask) ? ETP_PSTORE_ERR_MASKED : 0) |
          (k != n_cand[b] ? ETP_PSTORE_ERR_COUNT : 0) | ((base < 0 || base + 1 + k > rows) ? ETP_PSTORE_ERR_ROW : 0);
  return p;
}

// grid (B, 1 + ceil(V / 4)), which holds a wave for the mean and one for each of up to V candidates: wave t of episode b writes the
// mean (t == 0) or candidate t - 1
template <int NCH>
__global__ __launch_bounds__(256) void pano_store_fwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ masks,
                                                             const int64_t* __restrict__ nav_types,
                                                             const int32_t* __restrict__ row_base,
                                                             const int32_t* __restrict__ n_cand, float* __restrict__ store,
                                                             int32_t* __restrict__ status, int V, int R) {
  constexpr int H = NCH * 256;
  const int b = blockIdx.x, lane = threadIdx.x & 63, t = blockIdx.y * 4 + (threadIdx.x >> 6);
  const PanoViews p = pano_views(masks, nav_types, row_base, n_cand, b, V, R, lane);
  if (t == 0 && lane == 0) status[b] = p.err;
  if (p.err || t > __popcll(p.cand)) return;
  const float* xb = x + (long)b * V * H;
  float* dst = store + ((long)row_base[b] + t) * H;
  Row<NCH> acc;
  if (t == 0) {
    row_zero<NCH>(acc);
    for (int v0 = 0; v0 < V; v0 += 4) {                    // four views' loads in flight; the adds stay in view order
      if (((p.mask >> v0) & 0xF) == 0) continue;
      Row<NCH> r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) row_load<NCH>(r[u], xb + (long)min(v0 + u, V - 1) * H, lane);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if ((p.mask >> (v0 + u)) & 1) row_add<NCH>(acc, r[u]);     // selected by the mask, not multiplied: bits 64 .. are zero
    }
    const float n = (float)p.len;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc.v[c][e] = acc.v[c][e] / n;
  } else {
    unsigned long long m = p.cand;
    for (int j = 1; j < t; ++j) m &= m - 1;                // drop the t - 1 lower candidates
    row_load<NCH>(acc, xb + (long)(__ffsll((long long)m) - 1) * H, lane);
  }
  row_store<NCH>(acc, dst, lane);
}

// grid (B, ceil(V / 4)): one wave per view
template <int NCH>
__global__ __launch_bounds__(256) void pano_store_bwd_kernel(const float* __restrict__ d_store, const uint8_t* __restrict__ masks,
                                                             const int64_t* __restrict__ nav_types,
                                                             const int32_t* __restrict__ row_base,
                                                             const int32_t* __restrict__ n_cand, float* __restrict__ dx, int V, int R,
                                                             int accumulate) {
  constexpr int H = NCH * 256;
  const int b = blockIdx.x, lane = threadIdx.x & 63, v = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (v >= V) return;
  const PanoViews p = pano_views(masks, nav_types, row_base, n_cand, b, V, R, lane);
  if (p.err && accumulate) return;
  float* dst = dx + ((long)b * V + v) * H;
  Row<NCH> g, c;
  row_zero<NCH>(g);
  if (!p.err && ((p.mask >> v) & 1)) {
    const float* src = d_store + (long)row_base[b] * H;
    row_load<NCH>(g, src, lane);
    const float n = (float)p.len;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) g.v[k][e] = g.v[k][e] / n;
    if ((p.cand >> v) & 1) {
      const int rank = __popcll(p.cand & ((1ull << v) - 1ull));
      row_load<NCH>(c, src + (long)(1 + rank) * H, lane);
      row_add<NCH>(g, c);
    }
  }
  if (accumulate) {
    row_load<NCH>(c, dst, lane);
    row_add<NCH>(c, g);
    row_store<NCH>(c, dst, lane);
  } else {
    row_store<NCH>(g, dst, lane);
  }
}

static int pano_store_check(const char* fn, const void* rows_a, const void* rows_b, const uint8_t* masks, const int64_t* nav_types,
                            const int32_t* row_base, const int32_t* n_cand, const void* extra, int B, int V, int H, int R) {
  const bool ok_ptr = rows_a && rows_b && masks && nav_types && row_base && n_cand && extra;
  if (!ok_ptr) return fail(ETP_ERR_INVALID, std::string(fn) + ": null pointer");
  if (!(H == 256 || H == 512 || H == 768)) return fail(ETP_ERR_INVALID, std::string(fn) + ": H must be 256, 512 or 768");
  if (V < 1 || V > 64 || B < 1 || R < 1) return fail(ETP_ERR_INVALID, std::string(fn) + ": V must lie in 1 .. 64, B and R must be positive");
  if (((uintptr_t)rows_a | (uintptr_t)rows_b) % 16 != 0 || (uintptr_t)nav_types % 8 != 0 ||
      ((uintptr_t)row_base | (uintptr_t)n_cand | (uintptr_t)extra) % 4 != 0)
    return fail(ETP_ERR_INVALID, std::string(fn) + ": fp32 rows must be 16-byte aligned, nav_types 8-byte, int32 operands 4-byte");
  return ETP_OK;
}

}  // namespace etp

extern "C" int etp_pano_store_fwd(const float* pano_embeds, const uint8_t* pano_masks, const int64_t* nav_types, const int32_t* row_base,
                                  const int32_t* n_cand, int B, int V, int H, float* store, int R, int32_t* status,
                                  etp_stream_t stream) {
  using namespace etp;
  ETP_TRY(pano_store_check(__func__, pano_embeds, store, pano_masks, nav_types, row_base, n_cand, status, B, V, H, R));
  const dim3 grid(B, 1 + (V + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (H == 256) ETP_LAUNCH(pano_store_fwd_kernel<1>, grid, block, 0, st, pano_embeds, pano_masks, nav_types, row_base, n_cand, store, status, V, R);
  else if (H == 512) ETP_LAUNCH(pano_store_fwd_kernel<2>, grid, block, 0, st, pano_embeds, pano_masks, nav_types, row_base, n_cand, store, status, V, R);
  else ETP_LAUNCH(pano_store_fwd_kernel<3>, grid, block, 0, st, pano_embeds, pano_masks, nav_types, row_base, n_cand, store, status, V, R);
  ETP_CHECK_LAUNCH("pano_store_fwd");
  return ETP_OK;
}

extern "C" int etp_pano_store_bwd(const float* d_store, const uint8_t* pano_masks, const int64_t* nav_types, const int32_t* row_base,
                                  const int32_t* n_cand, int B, int V, int H, int R, float* d_pano_embeds, int accumulate,
                                  etp_stream_t stream) {
  using namespace etp;
  ETP_TRY(pano_store_check(__func__, d_store, d_pano_embeds, pano_masks, nav_types, row_base, n_cand, row_base, B, V, H, R));
  ETP_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate is 0 or 1");
  const dim3 grid(B, (V + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (H == 256) ETP_LAUNCH(pano_store_bwd_kernel<1>, grid, block, 0, st, d_store, pano_masks, nav_types, row_base, n_cand, d_pano_embeds, V, R, accumulate);
  else if (H == 512) ETP_LAUNCH(pano_store_bwd_kernel<2>, grid, block, 0, st, d_store, pano_masks, nav_types, row_base, n_cand, d_pano_embeds, V, R, accumulate);
  else ETP_LAUNCH(pano_store_bwd_kernel<3>, grid, block, 0, st, d_store, pano_masks, nav_types, row_base, n_cand, d_pano_embeds, V, R, accumulate);
  ETP_CHECK_LAUNCH("pano_store_bwd");
  return ETP_OK;
}
