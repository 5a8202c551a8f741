// A pre-training batch's device side, straight from the resident view-feature store: two launches.
//
// traj_views_kernel replaces, per batch, R2RTextPathData.get_traj_pano_fts (pretrain_src/pretrain_src/data/dataset.py:483-526: per
// trajectory step the candidate views in scanvp_cands order, then the panorama views no candidate names, in index order) followed by
// the padding of sap_collate / mlm_collate (tasks.py:331-343, 107-120) and the slice x[:, :image_feat_size] of get_input
// (dataset.py:453-454).  traj_pair_dists_kernel replaces the double loop of get_gmap_inputs (dataset.py:316-320) and the padding of
// tasks.py:350-355.  The host hands over indices and scalars only (etpnav_amd/pretrain_data.py); no feature row crosses the bus.
//
// Both follow pano_inputs.hip: one wavefront per output row, the width a run-time value, each lane owning groups of 4 consecutive
// columns 256 apart (16-byte accesses) in the feature copies.  Every wave derives its step's (its sample's) record and every malformed
// condition for itself from uniform loads -- no LDS, no barrier, no atomics, plain stores -- and nothing of a malformed step or sample
// is indexed.  No transcendental: the angle features come from the host.  The distance is ONE double division rounded once to fp32;
// the file is compiled with -ffp-contract=off (build.py), as gmap_update.hip is.
//
// traj_nodes_fwd_kernel / traj_nodes_bwd_kernel (below) turn the panorama embeddings of those steps into the node features and back
// from the same kind of tables, in the same idiom, on H-wide rows (row.h).
#include "kernels.h"
#include "row.h"

namespace etp {

struct TrajCand {
  unsigned long long mask;   // bit i: a candidate names view i
  int k, len, err;
};

// every lane of the wave returns the same record
__device__ __forceinline__ TrajCand traj_cand(const int32_t* pano_row, const int32_t* count, const int32_t* view, int r, int V, int Kmax,
                                              int P, int N) {
  TrajCand c;
  c.k = count[r];
  c.mask = 0;
  c.len = 0;
  c.err = (c.k < 0 || c.k > Kmax) ? ETP_TRAJ_ERR_COUNT : 0;
  const int row = pano_row[r];
  if (row < 0 || row >= N) c.err |= ETP_TRAJ_ERR_ROW;
  if (c.err & ETP_TRAJ_ERR_COUNT) return c;
  for (int j = 0; j < c.k; ++j) {
    const int i = view[(long)r * Kmax + j];
    if (i < 0 || i >= P) c.err |= ETP_TRAJ_ERR_VIEW;
    else c.mask |= 1ull << i;
  }
  c.len = c.k + P - __popcll(c.mask);                      // two candidates of one view free that view once: the length can exceed P
  if (c.len > V) c.err |= ETP_TRAJ_ERR_VIEWS;
  return c;
}

// grid ceil(R * V / 4) blocks of four waves: wave w writes row (r, v) = (w / V, w % V) of the three feature tensors and of nav_types;
// the wave of v == 0 also writes the step's status and view length
__global__ __launch_bounds__(256) void traj_views_kernel(const float* __restrict__ img, const float* __restrict__ dep,
                                                         const int32_t* __restrict__ pano_row, const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ view, const float* __restrict__ cand_loc,
                                                         const float* __restrict__ view_loc_tab, int R, int V, int Kmax, int P, int Fimg,
                                                         int ld_img, int Fdep, int ld_dep, int N, float* __restrict__ rgb_fts,
                                                         float* __restrict__ dep_fts, float* __restrict__ loc_fts,
                                                         int64_t* __restrict__ nav_types, int64_t* __restrict__ view_lens,
                                                         int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)R * V) return;
  const int r = (int)(row / V), v = (int)(row % V);
  const TrajCand c = traj_cand(pano_row, count, view, r, V, Kmax, P, N);
  if (v == 0 && lane == 0) status[r] = c.err;
  if (c.err) return;
  if (v == 0 && lane == 0) view_lens[r] = c.len;
  float* drgb = rgb_fts + row * Fimg;
  float* ddep = dep ? dep_fts + row * Fdep : nullptr;
  if (v >= c.len) {                                        // padding: exact zeros (pad_tensors / pad_sequence)
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int f = lane * 4; f < Fimg; f += 256) store4(drgb + f, z);
    if (dep)
      for (int f = lane * 4; f < Fdep; f += 256) store4(ddep + f, z);
    if (lane < 4) loc_fts[row * 4 + lane] = 0.f;
    if (lane == 0) nav_types[row] = 0;
    return;
  }
  int i;
  const float* loc;
  if (v < c.k) {                                           // candidate v, in table order
    i = view[(long)r * Kmax + v];
    loc = cand_loc + ((long)r * Kmax + v) * 4;
  } else {                                                 // the (v - k)-th view, in index order, that no candidate names
    unsigned long long free = ~c.mask;
    if (P < 64) free &= (1ull << P) - 1;
    for (int j = c.k; j < v; ++j) free &= free - 1;
    i = __ffsll(free) - 1;
    loc = view_loc_tab + i * 4;
  }
  const long src = (long)pano_row[r] * P + i;
  const float* simg = img + src * ld_img;
  for (int f = lane * 4; f < Fimg; f += 256) {             // x[:, :image_feat_size]: the first Fimg of ld_img columns
    float t[4];
    load4(simg + f, t);
    store4(drgb + f, t);
  }
  if (dep) {
    const float* sdep = dep + src * ld_dep;
    for (int f = lane * 4; f < Fdep; f += 256) {
      float t[4];
      load4(sdep + f, t);
      store4(ddep + f, t);
    }
  }
  if (lane < 4) loc_fts[row * 4 + lane] = loc[lane];
  if (lane == 0) nav_types[row] = v < c.k ? 1 : 0;
}

// grid ceil(B * G / 4) blocks of four waves: wave w writes row (b, i) = (w / G, w % G) of gmap_pair_dists and gmap_masks[b, i]; the wave
// of i == 0 also writes the sample's status.  Every wave checks the whole sample: lane l looks at entries l, l + 64, ..
__global__ __launch_bounds__(256) void traj_pair_dists_kernel(const double* __restrict__ dist, int64_t dist_len,
                                                              const int64_t* __restrict__ scan_off, const int32_t* __restrict__ scan_n,
                                                              const int32_t* __restrict__ gmap_idx, const int32_t* __restrict__ gmap_len,
                                                              int B, int G, float* __restrict__ pair, uint8_t* __restrict__ masks,
                                                              int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)B * G) return;
  const int b = (int)(row / G), i = (int)(row % G);
  const int len = gmap_len[b], n = scan_n[b];
  const int64_t off = scan_off[b];
  const int32_t* idx = gmap_idx + (long)b * G;
  int err = (len < 1 || len > G) ? ETP_TRAJ_ERR_LEN : 0;
  if (n < 1 || off < 0 || off > dist_len || (int64_t)n * n > dist_len - off) err |= ETP_TRAJ_ERR_SCAN;
  if (!err) {
    int bad = 0;
    for (int j = 1 + lane; j < len; j += 64) bad |= (idx[j] < 0 || idx[j] >= n);   // entry 0 is [stop]: never looked up
    if (__any(bad)) err = ETP_TRAJ_ERR_INDEX;
  }
  if (i == 0 && lane == 0) status[b] = err;
  if (err) return;
  if (lane == 0) masks[row] = i < len ? 1 : 0;
  float* out = pair + row * G;
  const bool live = i >= 1 && i < len;
  const int vi = live ? idx[i] : 0;
  for (int j = lane; j < G; j += 64) {
    float d = 0.f;
    if (live && j >= 1 && j < len && j != i) {
      // the reference fills (i, j) and (j, i), i < j, from shortest_distances[vp_i][vp_j]: the lookup is directional
      const int vj = idx[j];
      const int a = i < j ? vi : vj, c = i < j ? vj : vi;
      d = (float)(dist[off + (int64_t)a * n + c] / 30.0);
    }
    out[j] = d;
  }
}

// ---- trajectory node features from the same integer tables: GlobalMapEncoder._aggregate_gmap_features (vilmodel.py:585-619) ----------
// What graph_inputs.pack_traj_csr + gather_sum_kernel (embed.hip) compute, without the CSR: every wave finds its row's sources in the
// sample's tables by uniform loads and ballots, and adds them in the CSR's order with gather_sum_kernel's operation, one fused
// multiply-add per element (this file is built with -ffp-contract=off, so it is spelled out), from +0.

struct TrajSample {
  int t0, t1, len, err;
};

// sample b's step range and node count, and every malformed condition of its steps; every lane returns the same record
__device__ __forceinline__ TrajSample traj_sample(const int32_t* step_off, const int64_t* view_lens, const int32_t* count,
                                                  const int32_t* gmap_len, int b, int R, int V, int Kmax, int G, int lane) {
  TrajSample s;
  s.t0 = step_off[b];
  s.t1 = step_off[b + 1];
  s.len = gmap_len[b];
  s.err = (s.len < 1 || s.len > G) ? ETP_TRAJ_ERR_LEN : 0;
  if (s.t0 < 0 || s.t1 > R || s.t1 <= s.t0) {
    s.err |= ETP_TRAJ_ERR_STEPS;
    return s;
  }
  int bad_k = 0, bad_n = 0;
  for (int t = s.t0 + lane; t < s.t1; t += 64) {
    const int k = count[t];
    const int64_t n = view_lens[t];
    bad_k |= (k < 0 || k > Kmax);
    bad_n |= (n < 1 || n > V);
  }
  if (__any(bad_k)) s.err |= ETP_TRAJ_ERR_COUNT;
  if (__any(bad_n)) s.err |= ETP_TRAJ_ERR_VIEWS;
  return s;
}

// the last step of [t0, t1) at viewpoint id, or -1
__device__ __forceinline__ int traj_last_visit(const int32_t* step_vp, int t0, int t1, int id, int lane) {
  int last = -1;
  for (int base = t0; base < t1; base += 64) {
    const int t = base + lane;
    const unsigned long long m = __ballot(t < t1 && step_vp[t] == id);
    if (m) last = base + 63 - __clzll(m);
  }
  return last;
}

// bit j: slot j of step t names id (Kmax <= 64: one lane per slot)
__device__ __forceinline__ unsigned long long traj_slots(const int32_t* count, const int32_t* cand_vp, int t, int Kmax, int id, int lane) {
  return __ballot(lane < count[t] && cand_vp[(long)t * Kmax + lane] == id);
}

__device__ __forceinline__ int traj_slot_count(const int32_t* count, const int32_t* cand_vp, int t0, int t1, int Kmax, int id, int lane) {
  int n = 0;
  for (int t = t0; t < t1; ++t) n += __popcll(traj_slots(count, cand_vp, t, Kmax, id, lane));
  return n;
}

// the first g of 1 .. len-1 with gmap_id[b, g] == id, or 0
__device__ __forceinline__ int traj_node_of(const int32_t* ids, int len, int id, int lane) {
  for (int base = 1; base < len; base += 64) {
    const int g = base + lane;
    const unsigned long long m = __ballot(g < len && ids[g] == id);
    if (m) return base + __ffsll(m) - 1;
  }
  return 0;
}

template <int NCH> __device__ __forceinline__ void row_fma(Row<NCH>& acc, float w, const Row<NCH>& x) {
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc.v[c][e] = fmaf(w, x.v[c][e], acc.v[c][e]);
}

__device__ __forceinline__ float traj_weight(long n) { return (float)(1.0 / (double)n); }   // torch.tensor(1.0 / n, dtype=float32)

// grid ceil(B * G / 4) blocks of four waves: wave w writes node row (b, g) = (w / G, w % G) and its status word
template <int NCH>
__global__ __launch_bounds__(256) void traj_nodes_fwd_kernel(const float* __restrict__ pano, const int32_t* __restrict__ step_off,
                                                             const int32_t* __restrict__ step_vp, const int64_t* __restrict__ view_lens,
                                                             const int32_t* __restrict__ count, const int32_t* __restrict__ cand_vp,
                                                             const int32_t* __restrict__ gmap_id, const int32_t* __restrict__ gmap_len,
                                                             int B, int R, int V, int Kmax, int G, float* __restrict__ out,
                                                             int32_t* __restrict__ status) {
  constexpr int H = NCH * 256;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)B * G) return;
  const int b = (int)(row / G), g = (int)(row % G);
  const TrajSample s = traj_sample(step_off, view_lens, count, gmap_len, b, R, V, Kmax, G, lane);
  if (s.err) {
    if (lane == 0) status[row] = s.err;
    return;
  }
  Row<NCH> acc, x;
  row_zero<NCH>(acc);
  int err = 0;
  if (g >= 1 && g < s.len) {
    const int id = gmap_id[row];
    const int last = id < 0 ? -1 : traj_last_visit(step_vp, s.t0, s.t1, id, lane);
    if (last >= 0) {                                       // visited: the mean of the valid views of its last visit
      const int n = (int)view_lens[last];
      const float w = traj_weight(n);
      for (int j = 0; j < n; ++j) {
        row_load<NCH>(x, pano + ((long)last * V + j) * H, lane);
        row_fma<NCH>(acc, w, x);
      }
    } else {                                               // a ghost: the mean over the slots that name it
      const int cnt = id < 0 ? 0 : traj_slot_count(count, cand_vp, s.t0, s.t1, Kmax, id, lane);
      if (cnt == 0) err = ETP_TRAJ_ERR_NODE;
      else {
        const float w = traj_weight(cnt);
        for (int t = s.t0; t < s.t1; ++t) {
          const int n = (int)view_lens[t];
          unsigned long long m = traj_slots(count, cand_vp, t, Kmax, id, lane);
          if (n < 64) m &= (1ull << n) - 1;                // a slot beyond the valid views counted above and adds nothing
          for (; m; m &= m - 1) {
            row_load<NCH>(x, pano + ((long)t * V + (__ffsll(m) - 1)) * H, lane);
            row_fma<NCH>(acc, w, x);
          }
        }
      }
    }
  }
  if (lane == 0) status[row] = err;
  if (!err) row_store<NCH>(acc, out + row * H, lane);
}

// grid ceil(R * V / 4) blocks of four waves: wave w writes panorama row (r, j) = (w / V, w % V); the wave of j == 0 also the step's status
template <int NCH>
__global__ __launch_bounds__(256) void traj_nodes_bwd_kernel(const float* __restrict__ dg, const int32_t* __restrict__ step_off,
                                                             const int32_t* __restrict__ step_vp, const int64_t* __restrict__ view_lens,
                                                             const int32_t* __restrict__ count, const int32_t* __restrict__ cand_vp,
                                                             const int32_t* __restrict__ gmap_id, const int32_t* __restrict__ gmap_len,
                                                             int B, int R, int V, int Kmax, int G, float* __restrict__ d_pano,
                                                             int32_t* __restrict__ status) {
  constexpr int H = NCH * 256;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)R * V) return;
  const int r = (int)(row / V), j = (int)(row % V);
  // the step's sample: the one b with step_off[b] <= r < step_off[b+1]
  int b = -1, owners = 0;
  for (int base = 0; base < B; base += 64) {
    const int c = base + lane;
    const unsigned long long m = __ballot(c < B && step_off[c] <= r && r < step_off[c + 1]);
    if (m) {
      if (b < 0) b = base + __ffsll(m) - 1;
      owners += __popcll(m);
    }
  }
  TrajSample s;
  s.err = ETP_TRAJ_ERR_STEPS;
  if (owners == 1) s = traj_sample(step_off, view_lens, count, gmap_len, b, R, V, Kmax, G, lane);
  if (j == 0 && lane == 0) status[r] = s.err;
  if (s.err) return;
  const int n = (int)view_lens[r];
  const int32_t* ids = gmap_id + (long)b * G;
  int ga = 0, gb = 0;
  float wa = 0.f, wb = 0.f;
  if (j < n) {
    const int ida = step_vp[r];
    if (ida >= 0 && traj_last_visit(step_vp, s.t0, s.t1, ida, lane) == r) {                  // (A)
      ga = traj_node_of(ids, s.len, ida, lane);
      wa = traj_weight(n);
    }
    if (j < count[r]) {                                                                      // (B)
      const int idb = cand_vp[(long)r * Kmax + j];
      if (idb >= 0 && traj_last_visit(step_vp, s.t0, s.t1, idb, lane) < 0) {
        gb = traj_node_of(ids, s.len, idb, lane);
        if (gb) wb = traj_weight(traj_slot_count(count, cand_vp, s.t0, s.t1, Kmax, idb, lane));
      }
    }
  }
  Row<NCH> acc, x;
  row_zero<NCH>(acc);
  const float* base = dg + (long)b * G * H;
  const bool a_first = ga && (!gb || ga < gb);
  if (a_first) {
    row_load<NCH>(x, base + (long)ga * H, lane);
    row_fma<NCH>(acc, wa, x);
  }
  if (gb) {
    row_load<NCH>(x, base + (long)gb * H, lane);
    row_fma<NCH>(acc, wb, x);
  }
  if (ga && !a_first) {
    row_load<NCH>(x, base + (long)ga * H, lane);
    row_fma<NCH>(acc, wa, x);
  }
  row_store<NCH>(acc, d_pano + row * H, lane);
}

// ---- the MLM task's masked-row selection: _compute_masked_hidden and the label gather (pretrain_cmt.py:141-163) ------------------------
// What MlmStep built on the host per batch (torch.nonzero, cumsum with a leading 0, the label gather), in one launch of ONE workgroup
// of four waves that walks the n labels in chunks of 256.  In the file's idiom every wave derives everything it needs for itself:
// each wave loads the whole chunk (four coalesced loads, the same lines for all four waves), takes the four ballots and so knows the
// selected count of the sub-chunks below its own and of the whole chunk -- no LDS, no barrier, no atomics; the running count is a
// wave-uniform value every wave carries alike.  Wave w then writes sub-chunk w: ptr_t[i] = the selected entries below i, and for a
// selected entry rows[j] = i, labels[j] = the label, j that same count.  Whatever txt_labels holds, nothing leaves its range: j is
// written only below n_expected (<= cap, checked on the host), ptr_t is clamped to n_expected, a label is clamped into 0 .. vocab-1,
// and the entries count .. n_expected-1 of a short selection are filled with row 0 / label 0.
__global__ __launch_bounds__(256) void mlm_select_kernel(const int32_t* __restrict__ txt_labels, int n, int vocab, int n_expected,
                                                         int32_t* __restrict__ rows, int32_t* __restrict__ ptr_t,
                                                         int64_t* __restrict__ labels, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long lower = (1ull << lane) - 1;
  int run = 0, bad = 0;
  for (int base = 0; base < n; base += 256) {
    int mine = -1, below = 0, all = 0;
    unsigned long long mm = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = base + q * 64 + lane;
      const int v = i < n ? txt_labels[i] : -1;
      const unsigned long long m = __ballot(v != -1);
      bad |= (v < -1 || v >= vocab);
      const int c = __popcll(m);
      below += q < w ? c : 0;
      all += c;
      if (q == w) {
        mine = v;
        mm = m;
      }
    }
    const int i = base + w * 64 + lane;
    const int j = run + below + __popcll(mm & lower);
    if (i < n) {
      ptr_t[i] = j < n_expected ? j : n_expected;
      if (mine != -1 && j < n_expected) {
        rows[j] = i;
        labels[j] = mine < 0 ? 0 : (mine >= vocab ? vocab - 1 : mine);
      }
    }
    run += all;
  }
  for (int j = run + (int)threadIdx.x; j < n_expected; j += 256) {   // a short selection: in-range filler behind it
    rows[j] = 0;
    labels[j] = 0;
  }
  if (w == 0) {
    const int err = (run != n_expected ? ETP_MLM_ERR_COUNT : 0) | (__any(bad) ? ETP_MLM_ERR_LABEL : 0);
    if (lane == 0) {
      ptr_t[n] = run < n_expected ? run : n_expected;
      status[0] = err;
      status[1] = run;
    }
  }
}

}  // namespace etp

extern "C" int etp_mlm_select(const int32_t* txt_labels, int n, int vocab, int n_expected, int cap, int32_t* rows, int32_t* ptr_t,
                              int64_t* labels, int32_t* status, etp_stream_t stream) {
  using namespace etp;
  ETP_REQUIRE(txt_labels && rows && ptr_t && labels && status, "null pointer");
  ETP_REQUIRE(n >= 1 && n <= (1 << 20) && vocab >= 1, "n lies in 1 .. 2^20 and vocab is positive");
  ETP_REQUIRE(n_expected >= 0 && n_expected <= cap, "n_expected lies in 0 .. cap");
  ETP_REQUIRE(((uintptr_t)txt_labels | (uintptr_t)rows | (uintptr_t)ptr_t | (uintptr_t)status) % 4 == 0,
              "int32 operands must be 4-byte aligned");
  ETP_REQUIRE((uintptr_t)labels % 8 == 0, "labels must be 8-byte aligned");
  ETP_LAUNCH(mlm_select_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, txt_labels, n, vocab, n_expected, rows, ptr_t, labels,
             status);
  ETP_CHECK_LAUNCH("mlm_select");
  return ETP_OK;
}

#define ETP_TRAJ_NODES_CHECKS(rows_ptr, out_ptr)                                                                                        \
  ETP_REQUIRE(rows_ptr && step_off && step_vp && view_lens && cand_count && cand_vp && gmap_id && gmap_len && out_ptr && status,        \
              "null pointer");                                                                                                          \
  ETP_REQUIRE(H == 256 || H == 512 || H == 768, "hidden size must be 256, 512 or 768");                                                 \
  ETP_REQUIRE(B >= 1 && R >= 1 && V >= 1 && G >= 1, "B, R, V and G are positive");                                                      \
  ETP_REQUIRE(Kmax >= 1 && Kmax <= 64, "Kmax lies in 1 .. 64");                                                                         \
  ETP_REQUIRE((long)B * G <= 0x7FFFFFFFL / 4 && (long)R * V <= 0x7FFFFFFFL / 4, "B * G or R * V rows exceed the grid");                 \
  ETP_REQUIRE(((uintptr_t)rows_ptr | (uintptr_t)out_ptr) % 16 == 0, "the feature operands must be 16-byte aligned");                    \
  ETP_REQUIRE((uintptr_t)view_lens % 8 == 0, "view_lens must be 8-byte aligned");                                                       \
  ETP_REQUIRE(((uintptr_t)step_off | (uintptr_t)step_vp | (uintptr_t)cand_count | (uintptr_t)cand_vp | (uintptr_t)gmap_id |             \
               (uintptr_t)gmap_len | (uintptr_t)status) % 4 == 0, "int32 operands must be 4-byte aligned")

extern "C" int etp_traj_nodes_fwd(const float* pano, const int32_t* step_off, const int32_t* step_vp, const int64_t* view_lens,
                                  const int32_t* cand_count, const int32_t* cand_vp, const int32_t* gmap_id, const int32_t* gmap_len, int B,
                                  int R, int V, int Kmax, int G, int H, float* gmap_img_fts, int32_t* status, etp_stream_t stream) {
  using namespace etp;
  ETP_TRAJ_NODES_CHECKS(pano, gmap_img_fts);
  const dim3 grid((unsigned)(((long)B * G + 3) / 4)), block(256);
  ETP_DISPATCH_H(H, ETP_LAUNCH((traj_nodes_fwd_kernel<NCH>), grid, block, 0, (hipStream_t)stream, pano, step_off, step_vp, view_lens,
                               cand_count, cand_vp, gmap_id, gmap_len, B, R, V, Kmax, G, gmap_img_fts, status));
  ETP_CHECK_LAUNCH("traj_nodes_fwd");
  return ETP_OK;
}

extern "C" int etp_traj_nodes_bwd(const float* d_gmap_img_fts, const int32_t* step_off, const int32_t* step_vp, const int64_t* view_lens,
                                  const int32_t* cand_count, const int32_t* cand_vp, const int32_t* gmap_id, const int32_t* gmap_len, int B,
                                  int R, int V, int Kmax, int G, int H, float* d_pano, int32_t* status, etp_stream_t stream) {
  using namespace etp;
  ETP_TRAJ_NODES_CHECKS(d_gmap_img_fts, d_pano);
  const dim3 grid((unsigned)(((long)R * V + 3) / 4)), block(256);
  ETP_DISPATCH_H(H, ETP_LAUNCH((traj_nodes_bwd_kernel<NCH>), grid, block, 0, (hipStream_t)stream, d_gmap_img_fts, step_off, step_vp,
                               view_lens, cand_count, cand_vp, gmap_id, gmap_len, B, R, V, Kmax, G, d_pano, status));
  ETP_CHECK_LAUNCH("traj_nodes_bwd");
  return ETP_OK;
}

extern "C" int etp_traj_views(const float* img_store, const float* dep_store, const int32_t* pano_row, const int32_t* cand_count,
                              const int32_t* cand_view, const float* cand_loc, const float* view_loc_tab, int R, int V, int Kmax, int P,
                              int F_img, int ld_img, int F_dep, int ld_dep, int N, float* rgb_fts, float* dep_fts, float* loc_fts,
                              int64_t* nav_types, int64_t* view_lens, int32_t* status, etp_stream_t stream) {
  using namespace etp;
  ETP_REQUIRE(img_store && pano_row && cand_count && cand_view && cand_loc && view_loc_tab && rgb_fts && loc_fts && nav_types &&
                  view_lens && status, "null pointer");
  ETP_REQUIRE((dep_store == nullptr) == (dep_fts == nullptr), "dep_store and dep_fts are given together or both NULL");
  ETP_REQUIRE(R >= 1 && V >= 1 && N >= 1, "R, V and N are positive");
  ETP_REQUIRE(Kmax >= 1 && Kmax <= 64 && P >= 1 && P <= 64, "Kmax and P lie in 1 .. 64");
  ETP_REQUIRE(F_img >= 4 && F_img % 4 == 0 && ld_img % 4 == 0 && F_img <= ld_img, "F_img and ld_img are multiples of 4, 4 <= F_img <= ld_img");
  ETP_REQUIRE(!dep_store || (F_dep >= 4 && F_dep % 4 == 0 && ld_dep % 4 == 0 && F_dep <= ld_dep),
              "F_dep and ld_dep are multiples of 4, 4 <= F_dep <= ld_dep");
  ETP_REQUIRE((long)R * V <= 0x7FFFFFFFL / 4, "R * V rows exceed the grid");
  ETP_REQUIRE(((uintptr_t)img_store | (uintptr_t)dep_store | (uintptr_t)rgb_fts | (uintptr_t)dep_fts) % 16 == 0,
              "img_store, dep_store, rgb_fts and dep_fts must be 16-byte aligned");
  ETP_REQUIRE(((uintptr_t)nav_types | (uintptr_t)view_lens) % 8 == 0, "nav_types and view_lens must be 8-byte aligned");
  ETP_REQUIRE(((uintptr_t)pano_row | (uintptr_t)cand_count | (uintptr_t)cand_view | (uintptr_t)cand_loc | (uintptr_t)view_loc_tab |
               (uintptr_t)loc_fts | (uintptr_t)status) % 4 == 0, "fp32 and int32 operands must be 4-byte aligned");
  const long rows = (long)R * V;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  ETP_LAUNCH(traj_views_kernel, grid, block, 0, (hipStream_t)stream, img_store, dep_store, pano_row, cand_count, cand_view, cand_loc,
             view_loc_tab, R, V, Kmax, P, F_img, ld_img, F_dep, ld_dep, N, rgb_fts, dep_fts, loc_fts, nav_types, view_lens, status);
  ETP_CHECK_LAUNCH("traj_views");
  return ETP_OK;
}

extern "C" int etp_traj_pair_dists(const double* dist_tab, int64_t dist_len, const int64_t* scan_off, const int32_t* scan_n,
                                   const int32_t* gmap_idx, const int32_t* gmap_len, int B, int G, float* gmap_pair_dists,
                                   uint8_t* gmap_masks, int32_t* status, etp_stream_t stream) {
  using namespace etp;
  ETP_REQUIRE(dist_tab && scan_off && scan_n && gmap_idx && gmap_len && gmap_pair_dists && gmap_masks && status, "null pointer");
  ETP_REQUIRE(B >= 1 && G >= 1 && dist_len >= 1, "B, G and dist_len are positive");
  ETP_REQUIRE((long)B * G <= 0x7FFFFFFFL / 4, "B * G rows exceed the grid");
  ETP_REQUIRE(((uintptr_t)dist_tab | (uintptr_t)scan_off) % 8 == 0, "dist_tab and scan_off must be 8-byte aligned");
  ETP_REQUIRE(((uintptr_t)scan_n | (uintptr_t)gmap_idx | (uintptr_t)gmap_len | (uintptr_t)gmap_pair_dists | (uintptr_t)status) % 4 == 0,
              "fp32 and int32 operands must be 4-byte aligned");
  const long rows = (long)B * G;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  ETP_LAUNCH(traj_pair_dists_kernel, grid, block, 0, (hipStream_t)stream, dist_tab, dist_len, scan_off, scan_n, gmap_idx, gmap_len, B, G,
             gmap_pair_dists, gmap_masks, status);
  ETP_CHECK_LAUNCH("traj_pair_dists");
  return ETP_OK;
}
