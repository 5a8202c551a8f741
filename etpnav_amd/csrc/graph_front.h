// Limits of the per-episode graph kernels and the one piece of arithmetic two of them must share: the nearest front of a ghost.
// gmap_assemble_kernel (graph.hip) uses it for the position features and pairwise distances, nav_decide_kernel (decide.hip) for
// the node the agent walks back to; both include this header so that they cannot pick different fronts.
#pragma once
#include "common.h"

namespace etp {

constexpr int GN = 64;      // max visited nodes per episode
constexpr int GM = 192;     // max ghost nodes per episode

// GraphMap.front_to_ghost_dist (graph_utils.py:259-270): over the fronts fidx[q0 .. q1) of one ghost at gp, in list order, the
// first one at the minimum distance (a strict `<` from 10000, as the reference's loop); no front nearer than 10000: (10000, 0).
__device__ __forceinline__ void nearest_front(const int32_t* fidx, int q0, int q1, const float (*npos)[3], const float* gp,
                                              float& best_d, int& best_v) {
  float best = 10000.f; int bv = 0;
  for (int q = q0; q < q1; ++q) {
    const int f = fidx[q];
    const float dx = npos[f][0] - gp[0], dy = npos[f][1] - gp[1], dz = npos[f][2] - gp[2];
    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
    if (d < best) { best = d; bv = f; }
  }
  best_d = best; best_v = bv;
}

}  // namespace etp
