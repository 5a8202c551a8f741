// The rollout decision on the device: node logits -> everything envs.step needs, one launch per rollout step.
//
// Replaces, per rollout step, the tail of RLTrainer.rollout (vlnce_baselines/ss_trainer_ETP.py:880-977): the softmax over the node
// logits, one .item() per episode for GraphMap.node_stop_scores (:880-882), Categorical.sample / rand_like / where or argmax
// (:895-902), the .cpu() (:903) and the Python loop over gmap.shortest_path / front_to_ghost_dist / node_stop_scores that builds the
// environment actions (:908-977).  Input: the compact graph arrays of graph_inputs.pack_batch (the ones etp_gmap_assemble reads),
// the logits, the episode's row of a device-resident stop-score table.  Output: one int32 record per episode (etpnav_hip.h), so the
// host makes one copy.
//
// One 256-thread workgroup per episode, everything in LDS (<= 64 visited nodes, <= 192 ghosts, G <= 257), plain stores only:
//   wave 0 .. 3   softmax of the <= 257 logits (two per thread), arg-max with the lowest index among equal values
//   thread 64     inverse-CDF draw: the first index whose inclusive prefix sum of p, added serially in index order, exceeds
//                 u0 * total (total = the same serial sum) -- etp_waypoint_tail's convention -- clamped to the last p > 0
//   wave 2        the stop-score row: lane cur takes p[0] and stores it, arg-max over lanes 0 .. n-1 (lowest index among equals)
//   threads < n   single-source shortest paths from cur_node: Jacobi relaxation (two distance buffers, parent pointers; a strict
//                 `<` scanning predecessors in ascending order), at most n rounds, stops after a round without a change
//   thread 0      stop or go, nearest front (graph_front.h, shared with gmap_assemble_kernel), walk of the parent pointers
#include "kernels.h"
#include "graph_front.h"
#include "gemm_shared.h"     // prof_begin / prof_end

namespace etp {

constexpr int DEC_G = 1 + GN + GM;        // 257
constexpr int DEC_HDR = ETP_DECIDE_HDR;   // record header length

struct DecideArgs {
  const float* logits; const float* node_pos; const int32_t* n_nodes; const float* adj; const float* ghost_pos;
  const int32_t* n_ghost; const int32_t* front_ptr; const int32_t* front_idx; const int32_t* cur_node; const int32_t* slot;
  const float* uniforms; const int64_t* teacher; float sample_ratio; int force_stop;
  int Nmax, Mmax, Fmax, G, S;
  float* stop_scores; int32_t* record;
};

__global__ __launch_bounds__(256) void nav_decide_kernel(const DecideArgs a) {
  __shared__ float W[GN][GN + 1];
  __shared__ float npos[GN][3];
  __shared__ float sP[DEC_G + 3];
  __shared__ float dist[2][GN];
  __shared__ int parent[GN], rpath[GN];
  __shared__ float redm[4], reds[4], sgp[3];
  __shared__ int redi[4];
  __shared__ int s_action, s_stop_node, s_hdr[DEC_HDR];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n_nodes[b], m = a.n_ghost[b], G = a.G, cur = a.cur_node[b], sl = a.slot[b];
  const int R = DEC_HDR + a.Nmax;
  int32_t* rec = a.record + (long)b * R;
  // malformed episode (uniform over the workgroup): flag it, touch nothing else
  if (n < 1 || n > a.Nmax || m < 0 || m > a.Mmax || 1 + n + m > G || cur < 0 || cur >= n || sl < 0 || sl >= a.S) {
    for (int t = tid; t < R; t += 256) rec[t] = t == 2 ? ETP_DECIDE_ERR_INPUT : (t == 6 || t == 7) ? 0 : -1;
    return;
  }

  const float* lg = a.logits + (long)b * G;
  float mx = -INFINITY;
  int bi = 0x7fffffff;
  for (int k = tid; k < G; k += 256) {                     // ascending k: a strict > keeps the first of equal values
    const float v = lg[k];
    sP[k] = v;
    if (v > mx) { mx = v; bi = k; }
  }
  const float* adj = a.adj + (long)b * a.Nmax * a.Nmax;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e % n;
    const float w = adj[i * a.Nmax + j];
    W[i][j] = (i != j && w >= 0.f) ? w : INFINITY;
  }
  for (int e = tid; e < n * 3; e += 256) npos[e / 3][e % 3] = a.node_pos[((long)b * a.Nmax) * 3 + e];
  if (tid < GN) { dist[0][tid] = tid == cur ? 0.f : INFINITY; parent[tid] = -1; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > mx || (ov == mx && oi < bi)) { mx = ov; bi = oi; }
  }
  if (lane == 0) { redm[wave] = mx; redi[wave] = bi; }
  __syncthreads();
  mx = redm[0]; bi = redi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (redm[w] > mx || (redm[w] == mx && redi[w] < bi)) { mx = redm[w]; bi = redi[w]; }
  if (bi >= G) bi = 0;                                      // a row of NaNs: every comparison fails; stay in bounds
  const int greedy = bi;

  // p = exp(l - max) / sum: per thread serially over its <= 2 entries (1 addition), wave butterfly (6), the four wave sums
  // serially (3): the longest addition chain is 10.  exp(-inf - max) is an exact 0.
  float sum = 0.f;
  for (int k = tid; k < G; k += 256) {
    const float e = expf(sP[k] - mx);
    sP[k] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) reds[wave] = sum;
  __syncthreads();
  sum = ((reds[0] + reds[1]) + reds[2]) + reds[3];
  for (int k = tid; k < G; k += 256) sP[k] = sP[k] / sum;
  __syncthreads();
  const float stop_prob = sP[0];

  if (tid == 64) {                                          // the action (:895-902)
    int act = greedy;
    if (a.uniforms != nullptr) {
      float total = 0.f;
      int last = 0;
      for (int k = 0; k < G; ++k) {
        total += sP[k];
        if (sP[k] > 0.f) last = k;
      }
      const float target = a.uniforms[2 * b] * total;
      float run = 0.f;
      act = last;
      for (int k = 0; k < G; ++k) {
        run += sP[k];
        if (run > target) { act = k; break; }
      }
      if (act > last) act = last;
      if (a.teacher != nullptr && a.uniforms[2 * b + 1] <= a.sample_ratio) {
        const long tv = a.teacher[b];
        act = (tv < -2147483647L || tv > 2147483647L) ? (int)0x80000000 : (int)tv;
      }
    }
    s_action = act;
  }
  if (wave == 2) {                                          // the stop-score row (:881-882, 911-913)
    float v = -INFINITY;
    int vi = 0x7fffffff;
    if (lane < n) {
      float* cell = a.stop_scores + (long)sl * GN + lane;
      if (lane == cur) { *cell = stop_prob; v = stop_prob; }
      else v = *cell;
      vi = lane;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(vi, o, 64);
      if (ov > v || (ov == v && oi < vi)) { v = ov; vi = oi; }
    }
    if (vi >= n) vi = 0;                                    // unreachable with finite scores (lane 0 < n always holds one)
    if (lane == 0) s_stop_node = vi;
  }

  // shortest paths from cur over the visited-node graph (GraphMap.shortest_path[cur_vp], graph_utils.py:256)
  int cb = 0;
  for (int r = 0; r < n; ++r) {
    int changed = 0;
    if (tid < n) {
      float best = dist[cb][tid];
      int par = -1;
      for (int i = 0; i < n; ++i) {
        const float c = dist[cb][i] + W[i][tid];
        if (c < best) { best = c; par = i; }
      }
      dist[cb ^ 1][tid] = best;
      if (par >= 0) { parent[tid] = par; changed = 1; }
    }
    cb ^= 1;
    if (!__syncthreads_or(changed)) break;
  }

  if (tid == 0) {                                           // stop or go (:909), target, back path (:916-917, 958-959)
    const int action = s_action;
    const bool stop = action == 0 || a.force_stop != 0 || m == 0;
    int flags = stop ? ETP_DECIDE_STOP : 0, ghost = -1, target = stop ? s_stop_node : -1, plen = 0;
    if (!stop) {
      if (action < 1 + n || action >= 1 + n + m) flags |= ETP_DECIDE_ERR_ACTION;
      else {
        ghost = action - 1 - n;
        const int32_t* fp = a.front_ptr + (long)b * (a.Mmax + 1);
        const int32_t* fidx = a.front_idx + (long)b * a.Fmax;
        const int q0 = fp[ghost], q1 = fp[ghost + 1];
        bool ok = q0 >= 0 && q1 > q0 && q1 <= a.Fmax;
        if (ok)
          for (int q = q0; q < q1; ++q) ok = ok && fidx[q] >= 0 && fidx[q] < n;
        if (!ok) flags |= ETP_DECIDE_ERR_INPUT;
        else {
          for (int e = 0; e < 3; ++e) sgp[e] = a.ghost_pos[((long)b * a.Mmax + ghost) * 3 + e];
          float fd;
          nearest_front(fidx, q0, q1, npos, sgp, fd, target);
        }
      }
    }
    if (target >= 0) {
      if (!(dist[cb][target] < INFINITY)) flags |= ETP_DECIDE_ERR_UNREACHABLE;
      else
        for (int k = target; k != cur && k >= 0 && plen < n; k = parent[k]) rpath[plen++] = k;
    }
    s_hdr[0] = action; s_hdr[1] = greedy; s_hdr[2] = flags; s_hdr[3] = s_stop_node; s_hdr[4] = target; s_hdr[5] = ghost;
    s_hdr[6] = plen; s_hdr[7] = __float_as_int(stop_prob);
  }
  __syncthreads();
  const int plen = s_hdr[6];
  for (int t = tid; t < R; t += 256) {
    const int q = t - DEC_HDR;
    rec[t] = t < DEC_HDR ? s_hdr[t] : (q < plen ? rpath[plen - 1 - q] : -1);
  }
}

int nav_decide(const DecideArgs& a, int B, hipStream_t st) {
  ProfRec rec;
  const bool prof = prof_begin("nav_decide_kernel", 0.0, 0.0, st, rec);
  ETP_LAUNCH(nav_decide_kernel, dim3(B), dim3(256), 0, st, a);
  ETP_CHECK_LAUNCH("nav_decide");
  if (prof) prof_end(rec, st);
  return ETP_OK;
}

}  // namespace etp

extern "C" int etp_nav_decide(const float* logits, const float* node_pos, const int32_t* n_nodes, const float* adj,
                              const float* ghost_pos, const int32_t* n_ghost, const int32_t* front_ptr, const int32_t* front_idx,
                              const int32_t* cur_node, const int32_t* slot, const float* uniforms, const int64_t* teacher,
                              float sample_ratio, int force_stop, int B, int Nmax, int Mmax, int Fmax, int G, float* stop_scores,
                              int S, int32_t* record, etp_stream_t stream) {
  using namespace etp;
  ETP_REQUIRE(B > 0, "B must be positive");
  ETP_REQUIRE(G >= 1 && G <= DEC_G && Nmax >= 1 && Nmax <= GN && Mmax >= 0 && Mmax <= GM && Fmax >= 0,
              "graph limits: G <= 257, <= 64 visited nodes and <= 192 ghosts per episode");
  ETP_REQUIRE(stop_scores != nullptr && S > 0, "the stop-score table [S,64] is required");
  ETP_REQUIRE(logits && node_pos && n_nodes && adj && n_ghost && cur_node && slot && record, "null pointer");
  ETP_REQUIRE(Mmax == 0 || (ghost_pos && front_ptr && front_idx), "ghost arrays required when Mmax > 0");
  ETP_REQUIRE(!(uniforms != nullptr && teacher == nullptr && sample_ratio > 0.f),
              "uniforms with sample_ratio > 0 need the teacher labels");
  ETP_REQUIRE(((uintptr_t)logits | (uintptr_t)node_pos | (uintptr_t)n_nodes | (uintptr_t)adj | (uintptr_t)ghost_pos |
               (uintptr_t)n_ghost | (uintptr_t)front_ptr | (uintptr_t)front_idx | (uintptr_t)cur_node | (uintptr_t)slot |
               (uintptr_t)uniforms | (uintptr_t)stop_scores | (uintptr_t)record) % 4 == 0 && (uintptr_t)teacher % 8 == 0,
              "fp32 / int32 operands must be 4-byte aligned, the teacher labels 8-byte aligned");
  DecideArgs a;
  a.logits = logits; a.node_pos = node_pos; a.n_nodes = n_nodes; a.adj = adj; a.ghost_pos = ghost_pos; a.n_ghost = n_ghost;
  a.front_ptr = front_ptr; a.front_idx = front_idx; a.cur_node = cur_node; a.slot = slot; a.uniforms = uniforms; a.teacher = teacher;
  a.sample_ratio = sample_ratio; a.force_stop = force_stop; a.Nmax = Nmax; a.Mmax = Mmax; a.Fmax = Fmax; a.G = G; a.S = S;
  a.stop_scores = stop_scores; a.record = record;
  return nav_decide(a, B, (hipStream_t)stream);
}
