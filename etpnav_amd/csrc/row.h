// The row idiom of the H-wide row kernels (embed.hip, pano_store.hip): hidden size H = NCH*256, one 64-lane wavefront owns one row,
// each lane owns NCH groups of 4 consecutive columns (8/16-byte vector accesses, 512 B / 1 KiB contiguous per wave instruction).
#pragma once
#include "common.h"

namespace etp {

template <int NCH> struct Row {  // per-lane slice of one H-wide row
  float v[NCH][4];
};

template <int NCH, typename T> __device__ __forceinline__ void row_load(Row<NCH>& r, const T* p, int lane) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) load4(p + c * 256 + lane * 4, r.v[c]);
}
template <int NCH, typename T> __device__ __forceinline__ void row_store(const Row<NCH>& r, T* p, int lane) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) store4(p + c * 256 + lane * 4, r.v[c]);
}
template <int NCH> __device__ __forceinline__ void row_add(Row<NCH>& a, const Row<NCH>& b) {
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) a.v[c][e] += b.v[c][e];
}
template <int NCH> __device__ __forceinline__ void row_zero(Row<NCH>& a) {
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) a.v[c][e] = 0.f;
}

}  // namespace etp

// CALL with `constexpr int NCH = H / 256` in scope; inside namespace etp or behind `using namespace etp`
#define ETP_DISPATCH_H(H, CALL)                                                         \
  switch ((H) / 256) {                                                                  \
    case 1: { constexpr int NCH = 1; CALL; } break;                                     \
    case 2: { constexpr int NCH = 2; CALL; } break;                                     \
    case 3: { constexpr int NCH = 3; CALL; } break;                                     \
    default: return fail(ETP_ERR_INVALID, "hidden size must be 256, 512 or 768");       \
  }
