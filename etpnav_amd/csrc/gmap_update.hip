// The topological map on the device: GraphMap.update_graph in one launch, on state that stays where its consumers run.
//
// Replaces, per rollout step, the host work of GraphMap.update_graph (vlnce_baselines/models/graph_utils.py:193-254) with _localize
// (:163-175) and delete_ghost (:185-191; consume_ghost, vlnce_baselines/ss_trainer_ETP.py:976-977), and the re-serialisation of the
// whole map that followed it (graph_inputs.pack_episode / pack_batch / pack_img_csr and eleven host-to-device copies).  The state is
// one record per ORIGINAL environment (the stop-score table's convention, decide.hip); the kernel maintains it in place and emits,
// in batch order, exactly the compact arrays etp_gmap_assemble and etp_nav_decide read, plus one int32 record per episode from which
// the host keeps its names and positions without any distance arithmetic.
//
// One 256-thread workgroup per episode, the episode's positions, ghost sums / means and front lists in LDS, plain stores only:
//   load        the slot's record into LDS; a pending ghost deletion is applied by the load's index mapping (order is kept)
//   thread 0    appends the visited node and its edge to prev_node
//   candidates  in order (each may create or move a ghost): wave 0 measures the <= 64 visited nodes, waves 1 .. 3 the <= 192 ghost
//               means; a butterfly keeps the smallest distance and, among equal ones, the lowest index (= the reference's strict `<`
//               scan in insertion order); every thread reads the four wave results and takes the same branch
//   thread < m  ghost_aug_pos = mean + clip(noise * (aug, 0, aug), +-aug)
//   store       the slot's record, the compact arrays (fp32, fixed strides 64 / 192 / ETP_GMAP_FMAX) and the record
// Positions, sums, means and distances are double; the file is compiled with floating-point contraction off, so every operation
// is one correctly rounded IEEE operation in numpy's order: dx*dx + dy*dy + dz*dz summed left to right, one sqrt, sum / count.
//
// etp_gmap_embed_csr turns the states of a batch into the CSR over the embedding store that etp_gather_sum takes (graph_inputs
// pack_img_csr) and its transpose: a store row has at most one owner, so the transpose is an owner map and a scan.
#pragma clang fp contract(off)
#include "kernels.h"
#include "graph_front.h"

namespace etp {

constexpr int GF = ETP_GMAP_FMAX;         // absorbed candidates a slot can hold
constexpr int UPD_HDR = ETP_GMAP_HDR;
constexpr int UPD_KMAX = 16;

struct GmapSlot {
  double node_pos[GN][3];
  double gsum[GM][3];
  double gmean[GM][3];
  float adj[GN][GN];                      // edge length rounded to fp32 once (what the consumers read); < 0: no edge
  int32_t node_step[GN], node_row[GN];
  int32_t ghost_id[GM];
  int32_t fptr[GM + 1];                   // CSR of the absorbed candidates, ghosts in order, candidates in absorption order
  int32_t ent_front[GF], ent_row[GF];
  int32_t n, m, ghost_cnt;
};
static_assert(sizeof(GmapSlot) % 16 == 0, "slot records must keep 16-byte alignment");

struct GmapUpdArgs {
  GmapSlot* state; int S;
  const int32_t* slot; const int32_t* prev_node; const int32_t* step_id; const double* cur_pos; const float* cur_heading;
  const double* cand_pos; const int32_t* n_cand; const int32_t* cur_row; const int32_t* cand_row; const int32_t* del_ghost;
  const double* noise; double loc_noise; int merge_ghost; double ghost_aug; int Kmax;
  float* o_node_pos; int32_t* o_node_step; int32_t* o_n_nodes; float* o_adj; float* o_ghost_pos; int32_t* o_n_ghost;
  int32_t* o_front_ptr; int32_t* o_front_idx; int32_t* o_cur_node; float* o_cur_pos; float* o_cur_heading;
  int32_t* record;
};

__device__ __forceinline__ double dist3(const double* a, const double* b) {      // calc_position_distance / _localize
  const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

__global__ __launch_bounds__(256) void gmap_update_kernel(const GmapUpdArgs a) {
  __shared__ double npos[GN][3], gsum[GM][3], gmean[GM][3], gaug[GM][3];
  __shared__ double redd[4];
  __shared__ float erow[GN];              // the new node's row of adj
  __shared__ int32_t gid[GM], fptr[GM + 1], efront[GF], erw[GF];
  __shared__ int redi[4];
  __shared__ int32_t s_rec[UPD_HDR + UPD_KMAX];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = UPD_HDR + a.Kmax;
  int32_t* rec = a.record + (long)b * R;
  const int sl = a.slot[b], K = a.n_cand[b], prev = a.prev_node[b], del = a.del_ghost[b];

  // ---- validation: nothing of the slot is written before it has passed (uniform over the workgroup) ----
  int err = 0, n = 0, m = 0, total = 0, gcnt = 0, c0 = 0, dcnt = 0;
  GmapSlot* S = nullptr;
  if (sl < 0 || sl >= a.S || K < 0 || K > a.Kmax) err = ETP_GMAP_ERR_INPUT;
  else {
    S = a.state + sl;
    n = S->n; m = S->m; gcnt = S->ghost_cnt;
    if (n < 0 || n > GN || m < 0 || m > GM) err = ETP_GMAP_ERR_INPUT;           // a record that was never reset
    else if (prev < -1 || prev >= n || del < -1 || del >= m) err = ETP_GMAP_ERR_INPUT;
    else {
      total = S->fptr[m];
      if (total < m || total > GF) err = ETP_GMAP_ERR_INPUT;
      else {
        if (del >= 0) { c0 = S->fptr[del]; dcnt = S->fptr[del + 1] - c0; }
        if (dcnt < 0 || dcnt > total) err = ETP_GMAP_ERR_INPUT;
        else if (n + 1 > GN || m - (del >= 0 ? 1 : 0) + K > GM || total - dcnt + K > GF) err = ETP_GMAP_ERR_CAPACITY;
      }
    }
  }

  if (!err) {
    // ---- load, with the pending deletion folded into the index mapping (the remaining ghosts keep their order) ----
    if (del >= 0) { m -= 1; total -= dcnt; }
    for (int e = tid; e < n * 3; e += 256) npos[e / 3][e % 3] = S->node_pos[e / 3][e % 3];
    for (int e = tid; e < m * 3; e += 256) {
      const int g = e / 3, c = e % 3, gs = (del >= 0 && g >= del) ? g + 1 : g;
      gsum[g][c] = S->gsum[gs][c];
      gmean[g][c] = S->gmean[gs][c];
    }
    for (int g = tid; g <= m; g += 256) {
      if (del >= 0 && g >= del) { fptr[g] = S->fptr[g + 1] - dcnt; if (g < m) gid[g] = S->ghost_id[g + 1]; }
      else { fptr[g] = S->fptr[g]; if (g < m) gid[g] = S->ghost_id[g]; }
    }
    for (int e = tid; e < total; e += 256) {
      const int es = (del >= 0 && e >= c0) ? e + dcnt : e;
      efront[e] = S->ent_front[es];
      erw[e] = S->ent_row[es];
    }
    if (tid < GN) erow[tid] = -1.f;
    __syncthreads();

    // ---- the visited node (graph_utils.py:198-207) ----
    const int cur = n;
    const double cp[3] = {a.cur_pos[b * 3], a.cur_pos[b * 3 + 1], a.cur_pos[b * 3 + 2]};
    if (tid == 0) {
      npos[cur][0] = cp[0]; npos[cur][1] = cp[1]; npos[cur][2] = cp[2];
      if (prev >= 0) erow[prev] = (float)dist3(npos[prev], cp);
    }
    n += 1;
    __syncthreads();

    // ---- the candidates, in order (:208-246) ----
    for (int k = 0; k < K; ++k) {
      const double* cpk = a.cand_pos + ((long)b * a.Kmax + k) * 3;
      const double q[3] = {cpk[0], cpk[1], cpk[2]};
      double d = 10000.0;                                   // _localize's min_dis: only a smaller distance is a match
      int di = 0x7fffffff;
      if (wave == 0) {
        if (lane < n) { const double v = dist3(q, npos[lane]); if (v < 10000.0) { d = v; di = lane; } }
      } else {
        const int g = tid - 64;
        if (g < m) { const double v = dist3(q, gmean[g]); if (v < 10000.0) { d = v; di = g; } }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o, 64);
        const int oi = __shfl_xor(di, o, 64);
        if (od < d || (od == d && oi < di)) { d = od; di = oi; }
      }
      if (lane == 0) { redd[wave] = d; redi[wave] = di; }
      __syncthreads();
      const double nd = redd[0];
      const int ni = redi[0];
      double gd = redd[1];
      int gi = redi[1];
      if (redd[2] < gd) { gd = redd[2]; gi = redi[2]; }     // ascending ghost ranges: a strict < keeps the first minimum
      if (redd[3] < gd) { gd = redd[3]; gi = redi[3]; }
      const int row = a.cand_row[(long)b * a.Kmax + k];
      if (ni != 0x7fffffff && nd <= a.loc_noise) {          // on a visited node: an edge between the two NODES (:211-213)
        if (tid == 0) {
          erow[ni] = (float)dist3(cp, npos[ni]);
          s_rec[UPD_HDR + k] = (ETP_GMAP_EDGE << 24) | ni;
        }
      } else if (a.merge_ghost && gi != 0x7fffffff && gd <= a.loc_noise) {      // joins a ghost (:229-237)
        const int pos = min(max(fptr[gi + 1], 0), total);   // == fptr[gi + 1] in a record this kernel wrote
        int f0 = 0, r0 = 0, f1 = 0, r1 = 0;
        const int e0 = pos + tid, e1 = pos + tid + 256;
        if (e0 < total) { f0 = efront[e0]; r0 = erw[e0]; }
        if (e1 < total) { f1 = efront[e1]; r1 = erw[e1]; }
        __syncthreads();
        if (e0 < total) { efront[e0 + 1] = f0; erw[e0 + 1] = r0; }
        if (e1 < total) { efront[e1 + 1] = f1; erw[e1 + 1] = r1; }
        if (tid > gi && tid <= m) fptr[tid] += 1;
        if (tid == 0) {
          efront[pos] = cur; erw[pos] = row;
          const double cnt = (double)(pos - fptr[gi] + 1);
#pragma unroll
          for (int c = 0; c < 3; ++c) { gsum[gi][c] = gsum[gi][c] + q[c]; gmean[gi][c] = gsum[gi][c] / cnt; }
          s_rec[UPD_HDR + k] = (ETP_GMAP_MERGED << 24) | gid[gi];
        }
        total += 1;
      } else {                                              // a new ghost at the end of the order (:219-227, 239-246)
        if (tid == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) { gsum[m][c] = q[c]; gmean[m][c] = q[c]; }
          gid[m] = gcnt;
          efront[total] = cur; erw[total] = row;
          fptr[m + 1] = total + 1;
          s_rec[UPD_HDR + k] = (ETP_GMAP_NEW << 24) | gcnt;
        }
        m += 1; total += 1; gcnt += 1;
      }
      __syncthreads();
    }

    // ---- ghost_aug_pos (:248-254) ----
    for (int e = tid; e < m * 3; e += 256) {
      const int g = e / 3, c = e % 3;
      double v = gmean[g][c];
      if (a.ghost_aug != 0.0 && a.noise != nullptr) {
        double z = a.noise[((long)b * GM + g) * 3 + c] * (c == 1 ? 0.0 : a.ghost_aug);
        if (z < -a.ghost_aug) z = -a.ghost_aug;
        if (z > a.ghost_aug) z = a.ghost_aug;
        v = v + z;
      }
      gaug[g][c] = v;
    }

    // ---- the slot's record ----
    for (int e = tid; e < 3; e += 256) S->node_pos[cur][e] = cp[e];
    for (int e = tid; e < m * 3; e += 256) { S->gsum[e / 3][e % 3] = gsum[e / 3][e % 3]; S->gmean[e / 3][e % 3] = gmean[e / 3][e % 3]; }
    for (int g = tid; g <= m; g += 256) { S->fptr[g] = fptr[g]; if (g < m) S->ghost_id[g] = gid[g]; }
    for (int e = tid; e < total; e += 256) { S->ent_front[e] = efront[e]; S->ent_row[e] = erw[e]; }
    if (tid < n) { S->adj[cur][tid] = erow[tid]; S->adj[tid][cur] = erow[tid]; }
    if (tid == 0) {
      S->node_step[cur] = a.step_id[b]; S->node_row[cur] = a.cur_row[b];
      S->n = n; S->m = m; S->ghost_cnt = gcnt;
      s_rec[0] = n; s_rec[1] = m; s_rec[2] = 0; s_rec[3] = cur; s_rec[4] = gcnt; s_rec[5] = total; s_rec[6] = 0; s_rec[7] = 0;
    }
    __syncthreads();                                        // the stores above are visible to the workgroup's loads below
  } else {
    n = 0; m = 0; total = 0;
    if (tid == 0) {
      s_rec[0] = 0; s_rec[1] = 0; s_rec[2] = err; s_rec[3] = -1; s_rec[4] = 0; s_rec[5] = 0; s_rec[6] = 0; s_rec[7] = 0;
    }
    __syncthreads();
  }

  // ---- the compact arrays of etp_gmap_assemble / etp_nav_decide, padded as graph_inputs.pack_batch pads them; an episode that
  //      was refused comes out empty (n = m = 0), which both consumers handle ----
  for (int e = tid; e < GN * 3; e += 256) a.o_node_pos[(long)b * GN * 3 + e] = e < n * 3 ? (float)npos[e / 3][e % 3] : 0.f;
  for (int e = tid; e < GN; e += 256) a.o_node_step[(long)b * GN + e] = e < n ? (e == n - 1 ? a.step_id[b] : S->node_step[e]) : 0;
  for (int e = tid; e < GN * GN; e += 256) {
    const int i = e / GN, j = e % GN;
    a.o_adj[(long)b * GN * GN + e] = (i < n && j < n) ? S->adj[i][j] : -1.f;
  }
  for (int e = tid; e < GM * 3; e += 256) a.o_ghost_pos[(long)b * GM * 3 + e] = e < m * 3 ? (float)gaug[e / 3][e % 3] : 0.f;
  for (int g = tid; g <= GM; g += 256) a.o_front_ptr[(long)b * (GM + 1) + g] = g <= m ? (m ? fptr[g] : 0) : total;
  for (int e = tid; e < GF; e += 256) a.o_front_idx[(long)b * GF + e] = e < total ? efront[e] : 0;
  if (tid == 0) {
    a.o_n_nodes[b] = n; a.o_n_ghost[b] = m; a.o_cur_node[b] = n ? n - 1 : 0;
    a.o_cur_heading[b] = a.cur_heading[b];
  }
  if (tid < 3) a.o_cur_pos[b * 3 + tid] = (float)a.cur_pos[b * 3 + tid];
  for (int t = tid; t < R; t += 256) rec[t] = (t < UPD_HDR || (!err && t - UPD_HDR < K)) ? s_rec[t] : -1;
}

__global__ __launch_bounds__(256) void gmap_reset_kernel(GmapSlot* state, const int32_t* slots, int S) {
  const int sl = slots[blockIdx.x];
  if (sl < 0 || sl >= S) return;
  int32_t* w = reinterpret_cast<int32_t*>(state + sl);
  for (int e = threadIdx.x; e < (int)(sizeof(GmapSlot) / 4); e += 256) w[e] = 0;
  __syncthreads();
  float* adj = &state[sl].adj[0][0];
  for (int e = threadIdx.x; e < GN * GN; e += 256) adj[e] = -1.f;
}

// ---- the embedding CSR -------------------------------------------------------------------------------------------------------
// nodes + absorbed candidates the episode contributes to the forward CSR, with its counts and status: a slot out of range or a
// record whose counts are out of range (never reset) is ETP_GMAP_ERR_INPUT, G < 1 + n + m is ETP_GMAP_ERR_CAPACITY; either way the
// episode comes out empty (n = m = 0), so nothing of such a record is indexed
__device__ __forceinline__ int csr_count(const GmapSlot* state, int S, int sl, int G, int& n, int& m, int& st) {
  n = 0; m = 0; st = ETP_GMAP_ERR_INPUT;
  if (sl < 0 || sl >= S) return 0;
  const int sn = state[sl].n, sm = state[sl].m;
  if (sn < 0 || sn > GN || sm < 0 || sm > GM) return 0;
  const int t = state[sl].fptr[sm];
  if (t < sm || t > GF) return 0;
  if (1 + sn + sm > G) { st = ETP_GMAP_ERR_CAPACITY; return 0; }
  n = sn; m = sm; st = 0;
  return sn + t;
}

__global__ __launch_bounds__(256) void gmap_csr_fill_kernel(int32_t* own, int R) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < R) own[r] = -1;
}

// one workgroup per episode: its segment of the forward CSR and its rows of the owner map (idx_b / w_b, indexed by store row)
__global__ __launch_bounds__(256) void gmap_csr_fwd_kernel(const GmapSlot* state, int S, const int32_t* slot, int B, int G, int R,
                                                           int32_t* ptr_f, int32_t* idx_f, float* w_f, int32_t* own, float* own_w,
                                                           int32_t* status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int base = 0, st = 0, n = 0, m = 0;
  for (int i = 0; i < b; ++i) base += csr_count(state, S, slot[i], G, n, m, st);
  const int sl = slot[b];
  const int cnt = csr_count(state, S, sl, G, n, m, st);
  const GmapSlot* s = state + (st ? 0 : sl);              // n = m = 0 when st is set: s is not read then
  for (int t = tid; t < G; t += 256) {
    int p = base;
    if (t >= 1 && t <= n) p = base + t - 1;
    else if (t > n && t < 1 + n + m) p = base + n + s->fptr[t - 1 - n];
    else if (t >= 1 + n + m) p = base + cnt;
    ptr_f[(long)b * G + t] = p;
  }
  if (b == B - 1 && tid == 0) ptr_f[(long)B * G] = base + cnt;
  int bad = 0;
  for (int i = tid; i < n; i += 256) {
    int r = s->node_row[i];
    float w = 1.f;
    if (r < 0 || r >= R) { bad = 1; r = 0; w = 0.f; }
    else { own[r] = b * G + 1 + i; own_w[r] = 1.f; }
    idx_f[base + i] = r; w_f[base + i] = w;
  }
  for (int g = tid; g < m; g += 256) {
    const int tot = cnt - n;                                // a record this kernel wrote has 0 <= q0 < q1 <= tot
    const int q0 = min(max(s->fptr[g], 0), tot), q1 = min(max(s->fptr[g + 1], q0), tot);
    const float wg = (float)(1.0 / (double)(q1 - q0));
    for (int q = q0; q < q1; ++q) {
      int r = s->ent_row[q];
      float w = wg;
      if (r < 0 || r >= R) { bad = 1; r = 0; w = 0.f; }
      else { own[r] = b * G + 1 + n + g; own_w[r] = wg; }
      idx_f[base + n + q] = r; w_f[base + n + q] = w;
    }
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) status[b] = st | (bad ? ETP_GMAP_ERR_ROW : 0);
}

// one workgroup: ptr_b = exclusive scan of "row r has an owner", the owner map compacted in place (a row's entry moves to a
// position <= r, and every chunk is read into registers before anything of it is written)
__global__ __launch_bounds__(256) void gmap_csr_bwd_kernel(int R, int32_t* ptr_b, int32_t* idx_b, float* w_b) {
  __shared__ int cnt[256];
  const int tid = threadIdx.x;
  int carry = 0;
  for (int r0 = 0; r0 < R; r0 += 256) {
    const int r = r0 + tid;
    int o = -1;
    float w = 0.f;
    if (r < R) { o = idx_b[r]; w = w_b[r]; }
    const int has = o >= 0 ? 1 : 0;
    cnt[tid] = has;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {                     // inclusive scan
      const int v = tid >= s ? cnt[tid - s] : 0;
      __syncthreads();
      cnt[tid] += v;
      __syncthreads();
    }
    const int excl = carry + cnt[tid] - has;
    if (r < R) {
      ptr_b[r] = excl;
      if (has) { idx_b[excl] = o; w_b[excl] = w; }
    }
    carry += cnt[255];
    __syncthreads();
  }
  if (tid == 0) ptr_b[R] = carry;
}

}  // namespace etp

extern "C" int64_t etp_gmap_slot_bytes(void) { return (int64_t)sizeof(etp::GmapSlot); }

extern "C" int etp_gmap_reset(void* state, int S, const int32_t* slots, int n, etp_stream_t stream) {
  using namespace etp;
  ETP_REQUIRE(state && slots && S > 0 && n > 0, "state, slots and positive counts are required");
  ETP_REQUIRE((uintptr_t)state % 16 == 0 && (uintptr_t)slots % 4 == 0, "the state must be 16-byte aligned, slots 4-byte aligned");
  ETP_LAUNCH(gmap_reset_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (GmapSlot*)state, slots, S);
  ETP_CHECK_LAUNCH("gmap_reset");
  return ETP_OK;
}

extern "C" int etp_gmap_update(void* state, int S, const int32_t* slot, const int32_t* prev_node, const int32_t* step_id,
                               const double* cur_pos, const float* cur_heading, const double* cand_pos, const int32_t* n_cand,
                               const int32_t* cur_row, const int32_t* cand_row, const int32_t* del_ghost, const double* noise,
                               double loc_noise, int merge_ghost, double ghost_aug, int B, int Kmax, float* node_pos,
                               int32_t* node_step, int32_t* n_nodes, float* adj, float* ghost_pos, int32_t* n_ghost,
                               int32_t* front_ptr, int32_t* front_idx, int32_t* cur_node, float* cur_pos_out, float* cur_heading_out,
                               int32_t* record, etp_stream_t stream) {
  using namespace etp;
  ETP_REQUIRE(B > 0 && S > 0, "B and S must be positive");
  ETP_REQUIRE(Kmax >= 1 && Kmax <= UPD_KMAX, "Kmax must lie in 1 .. 16");
  ETP_REQUIRE(state && slot && prev_node && step_id && cur_pos && cur_heading && cand_pos && n_cand && cur_row && cand_row && del_ghost &&
                  node_pos && node_step && n_nodes && adj && ghost_pos && n_ghost && front_ptr && front_idx && cur_node && cur_pos_out &&
                  cur_heading_out && record,
              "null pointer");
  ETP_REQUIRE((uintptr_t)state % 16 == 0 && ((uintptr_t)cur_pos | (uintptr_t)cand_pos | (uintptr_t)noise) % 8 == 0,
              "the state must be 16-byte aligned, fp64 operands 8-byte aligned");
  ETP_REQUIRE(((uintptr_t)slot | (uintptr_t)prev_node | (uintptr_t)step_id | (uintptr_t)cur_heading | (uintptr_t)n_cand |
               (uintptr_t)cur_row | (uintptr_t)cand_row | (uintptr_t)del_ghost | (uintptr_t)node_pos | (uintptr_t)node_step |
               (uintptr_t)n_nodes | (uintptr_t)adj | (uintptr_t)ghost_pos | (uintptr_t)n_ghost | (uintptr_t)front_ptr |
               (uintptr_t)front_idx | (uintptr_t)cur_node | (uintptr_t)cur_pos_out | (uintptr_t)cur_heading_out | (uintptr_t)record) % 4 == 0,
              "fp32 / int32 operands must be 4-byte aligned");
  GmapUpdArgs a;
  a.state = (GmapSlot*)state; a.S = S; a.slot = slot; a.prev_node = prev_node; a.step_id = step_id; a.cur_pos = cur_pos;
  a.cur_heading = cur_heading; a.cand_pos = cand_pos; a.n_cand = n_cand; a.cur_row = cur_row; a.cand_row = cand_row;
  a.del_ghost = del_ghost; a.noise = noise; a.loc_noise = loc_noise; a.merge_ghost = merge_ghost; a.ghost_aug = ghost_aug; a.Kmax = Kmax;
  a.o_node_pos = node_pos; a.o_node_step = node_step; a.o_n_nodes = n_nodes; a.o_adj = adj; a.o_ghost_pos = ghost_pos;
  a.o_n_ghost = n_ghost; a.o_front_ptr = front_ptr; a.o_front_idx = front_idx; a.o_cur_node = cur_node; a.o_cur_pos = cur_pos_out;
  a.o_cur_heading = cur_heading_out; a.record = record;
  ETP_LAUNCH(gmap_update_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  ETP_CHECK_LAUNCH("gmap_update");
  return ETP_OK;
}

extern "C" int etp_gmap_embed_csr(const void* state, int S, const int32_t* slot, int B, int G, int R, int32_t* ptr_f, int32_t* idx_f,
                                  float* w_f, int32_t* ptr_b, int32_t* idx_b, float* w_b, int32_t* status, etp_stream_t stream) {
  using namespace etp;
  ETP_REQUIRE(B > 0 && S > 0 && R > 0, "B, S and R must be positive");
  ETP_REQUIRE(G >= 1 && G <= 1 + GN + GM, "G must lie in 1 .. 257");
  ETP_REQUIRE(state && slot && ptr_f && idx_f && w_f && ptr_b && idx_b && w_b && status, "null pointer");
  ETP_REQUIRE((uintptr_t)state % 16 == 0 && ((uintptr_t)slot | (uintptr_t)ptr_f | (uintptr_t)idx_f | (uintptr_t)w_f | (uintptr_t)ptr_b |
                                             (uintptr_t)idx_b | (uintptr_t)w_b | (uintptr_t)status) % 4 == 0,
              "the state must be 16-byte aligned, fp32 / int32 operands 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ETP_LAUNCH(gmap_csr_fill_kernel, dim3((R + 255) / 256), dim3(256), 0, st, idx_b, R);
  ETP_CHECK_LAUNCH("gmap_csr_fill");
  ETP_LAUNCH(gmap_csr_fwd_kernel, dim3(B), dim3(256), 0, st, (const GmapSlot*)state, S, slot, B, G, R, ptr_f, idx_f, w_f, idx_b, w_b,
             status);
  ETP_CHECK_LAUNCH("gmap_csr_fwd");
  ETP_LAUNCH(gmap_csr_bwd_kernel, dim3(1), dim3(256), 0, st, R, ptr_b, idx_b, w_b);
  ETP_CHECK_LAUNCH("gmap_csr_bwd");
  return ETP_OK;
}
