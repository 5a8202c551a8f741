// Register-resident attention for the planner's short sequences (bf16, head dim 64, Lq, Lk <= 128) on gfx950.
//
//   ctx = dropout(softmax(alpha * Q K^T + keymask + (w*dist + b))) V     BertSelfAttention.forward vilmodel_cmt.py:103-141,
//                                                                        BertOutAttention.forward :325-352 (cross attention),
//                                                                        GraphLXRTXLayer :721-741 (sprel bias on the graph),
//                                                                        nn.MultiheadAttention (common/transformer.py:138)
//
// The tile kernels of attn.hip spend their time in VALU work around the MFMAs (about 2 700 instructions per wavefront for an
// 80x80 head: scores leave the accumulators through LDS as single bf16 values, the row statistics travel through 16-lane
// shuffles and two workgroup barriers, the probabilities are written and re-read).  Here every product is arranged so that its
// RESULT is already the operand layout of the next one and nothing but K, V (and Q, dO in backward) touches LDS:
//
//   * one wavefront owns 16 query rows and ALL keys.  S^T = K Q^T (v_mfma 16x16x32: A = K rows from LDS, B = Q rows straight
//     from global) leaves lane (i, g) with keys 16n+4g..+3 of query i: the softmax statistics of a query are an in-lane
//     reduction plus two cross-lane steps, and the four probabilities of a lane are exactly the B operand (k = 4g..4g+3, column i)
//     of the k=16 MFMA.  O^T = V^T P^T then takes V through ds_read_b64_tr_b16 and P from REGISTERS; its result (4
//     consecutive head-dim values of query i per lane) crosses a 2 KB wave-private LDS strip so that global sees full 128-byte
//     rows.  One workgroup barrier (K/V staged), no probability tile.
//   * the probabilities are not written: the forward stores lse = max + log(sum) per query row (fp32, in the front of the
//     probability buffer, the convention of the streaming kernels) and the backward recomputes P = exp(s - lse) on the MFMA
//     accumulators.  Backward, one workgroup per (batch, head), Q, dO, K, V tiles resident in LDS:
//       role A  (wavefront = 16 queries)  S^T, dP^T = V dO^T;  D = sum_k P dP;  dS^T = P^T (dP^T - D);  dQ^T = K^T dS^T
//       role B  (wavefront = 16 keys)     S = Q K^T, dP = dO V^T in the other orientation (query 4g+r, key i), whose P / dS are
//                                         the B operands of  dV^T = dO^T P  and  dK^T = Q^T dS  (reduction over the queries)
//     Two barriers (tiles staged; D published).  Dropout is the counter hash of common.h in both directions.
//
// Host code at the bottom; the planner (planner.hip attn_fwd_impl / attn_bwd_impl) takes this path for every bf16 attention
// with both axes <= 128, the tile kernels of attn.hip keep the fp32 (parity) mode.
#include <stdlib.h>
#include <string.h>

#include "kernels.h"

namespace etp {
namespace {

// Operand tiles ([rows][64] bf16 = 128-byte rows, Q / dO / K / V) sit UNPADDED with the 16-byte chunk swizzle of the GEMM
// kernels (chunk ^= row & 7).  Round 3 used a 144-byte pitch that looked conflict-free for 16 consecutive lanes, but
// ds_read_b128 is served in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... (MI355X_MICROARCH.md, LDS): those mix the
// head-dim chunks g and g+1 of different rows, and at 9 chunks per row 7 of the 8 rows of the g+1 part fell on bank groups of
// the g part (2-way conflicts: SQ_LDS_BANK_CONFLICT 36 % forward / 41 % backward, profiles/r03_gemm_counters.txt).  With the XOR
// layout both the b128 operand fetch (rows 0-3,12-15 at chunk c, rows 4-11 at c+1) and the 8 rows x 32 bytes of a
// ds_read_b64_tr_b16 half-wave land on 16 resp. 8 distinct bank groups.
constexpr int TQ = 128;
// pitch of the wave-private output strips [16][64]: 128-byte row + 16-byte pad (8-byte writes down 16 rows, conflict-free)
constexpr int TP = 144;
constexpr int PROJ_K = 768;                      // fused out-projection dgrad: the reduction (= hidden size of every planner the reference builds)
constexpr int PROJ_SLAB_K = 128;                 // k-rows of W per slab, [128][64] bf16 = 16 KB
constexpr int PROJ_RING = 3;                     // slabs resident (two in flight behind the one being read)
__device__ __forceinline__ int tile_off(int row, int chunk) { return row * TQ + ((chunk ^ (row & 7)) << 4); }

struct RowArgs {
  const bf16_t *Q, *K, *V; long ldq, ldk, ldv;
  float* lse;                                    // [B*heads*Lq] fp32: row max + log(row sum)
  bf16_t* ctx; long ldc;
  int nh, Lq, Lk;
  Drop drop;                                     // on the probabilities; element index = ((b*heads+h)*Lq + q)*Lk + k
  const uint8_t* keymask; int mask_mode; const float* dist; const float* sp_w; const float* sp_b;
  float alpha;
  const bf16_t* dO; long ldd;
  bf16_t *dQ, *dK, *dV; long lddq, lddk, lddv;
  float *d_sp_w, *d_sp_b;
  // PROJ backward (rows_bwd_kernel<.., true>): dO is not read from memory but computed in the kernel's prologue as
  // dO[b, q, h*64 : h*64+64] = dY[b*Lq + q, 0:Kp] . W[0:Kp, h*64 : h*64+64]   (dY = the `dO` pointer with row stride ldd)
  const bf16_t* W; long ldw; int Kp;
  // QKV forward (rows_fwd_kernel<.., true>): Q / K / V are not read but computed in the kernel's prologue from the block's input rows
  //   [Q | K | V][b, l, h*64 : h*64+64] = X[b*L + l, 0:Kp] . Wqkv[sec*H + h*64 + (0..63), 0:Kp]^T + bqkv   (sec = 0, 1, 2; H = nh*64)
  // and WRITTEN to the Q / K / V pointers (the backward's stash).  X = the LayerNorm output in the operand dtype, W reuses `W` above.
  const bf16_t* X; long ldx; const float* bqkv;
  int kv_mod;                                    // > 0: keys / values / key mask of episode b are those of instruction b % kv_mod
};

__device__ __forceinline__ f32x4_t mma32(const uint4& a, const uint4& b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4_t mma16(const short4_t& a, const short4_t& b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ short4_t pack4(float a, float b, float c, float d) {
  const uint2 u = make_uint2(pack_bf16(a, b), pack_bf16(c, d));
  return __builtin_bit_cast(short4_t, u);
}
// operand of the k=32 product: 8 consecutive head-dim values (32*s + 8*(lane>>4) + e) of tile row row0 + (lane&15)
__device__ __forceinline__ uint4 frag(const char* tile, int row0, int s, int lane) {
  return *reinterpret_cast<const uint4*>(tile + tile_off(row0 + (lane & 15), s * 4 + (lane >> 4)));
}
// A operand of the k=16 product taken DOWN the tile rows: lane (i, g) <- tile[row0 + 4g + e][col0 + i], e = 0..3
__device__ __forceinline__ short4_t frag_t4(const char* tile, int row0, int col0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const int col = col0 + (i & 3) * 4;
  const char* p = tile + tile_off(row0 + 4 * g + (i >> 2), col >> 3) + (col & 7) * 2;
  typedef short4_t __attribute__((address_space(3))) * lds_s4;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p));
}

// global [rows_valid][64] (row stride ld) -> registers -> LDS natural tile [rows_pad][64], zero rows beyond rows_valid.  All
// loads of all tiles are issued before the first LDS write (one round trip); the workgroup has >= 256 threads.  The fetch is
// branch-free and unmasked on purpose: a load under a per-thread `if`, or a select right behind it, makes hipcc wait vmcnt(0) after
// EVERY load (the ISA of the earlier form paid one full memory latency per 16-byte piece, 14 in a row for the backward's four
// tiles); pieces past the tile re-read its last valid row (same cache lines) and the zeroing happens in the commit.
template <int MAXROWS> struct TileRegs {
  static constexpr int N = (MAXROWS * 8 + 255) / 256;
  uint4 v[N];
};
template <int MAXROWS>
__device__ __forceinline__ void tile_fetch(TileRegs<MAXROWS>& r, const bf16_t* __restrict__ g, long ld, int rows_valid, int tid, int nthr) {
#pragma unroll
  for (int j = 0; j < TileRegs<MAXROWS>::N; ++j) {
    const int q = tid + j * nthr, row = q >> 3, c = (q & 7) * 8;
    r.v[j] = *reinterpret_cast<const uint4*>(g + (long)min(row, rows_valid - 1) * ld + c);
  }
}
template <int MAXROWS>
__device__ __forceinline__ void tile_commit(char* lds, const TileRegs<MAXROWS>& r, int rows_valid, int rows_pad, int tid, int nthr) {
#pragma unroll
  for (int j = 0; j < TileRegs<MAXROWS>::N; ++j) {
    const int q = tid + j * nthr, row = q >> 3;
    const bool ok = row < rows_valid;
    uint4 v = r.v[j];
    v.x = ok ? v.x : 0u; v.y = ok ? v.y : 0u; v.z = ok ? v.z : 0u; v.w = ok ? v.w : 0u;
    if (row < rows_pad) *reinterpret_cast<uint4*>(lds + tile_off(row, q & 7)) = v;
  }
}

// 16 x 64 result tile of a wavefront (accumulators of O^T / dQ^T / dK^T / dV^T: lane (i, g) holds columns 16t+4g..+3 of row
// i) -> global rows as full 128-byte lines, through a wave-private LDS strip [16][TP] (LDS operations of one wavefront
// complete in order: no barrier)
__device__ __forceinline__ void store_rows16(char* strip, const f32x4_t (&acc)[4], float scale, bf16_t* __restrict__ g0, long ld,
                                             int rows_valid, int lane) {
  const int i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    *reinterpret_cast<uint2*>(strip + i * TP + (16 * t + 4 * g) * 2) =
        make_uint2(pack_bf16(acc[t][0] * scale, acc[t][1] * scale), pack_bf16(acc[t][2] * scale, acc[t][3] * scale));
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = lane + 64 * j, row = c >> 3, part = c & 7;
    const uint4 v = *reinterpret_cast<const uint4*>(strip + row * TP + part * 16);
    if (row < rows_valid) *reinterpret_cast<uint4*>(g0 + (long)row * ld + part * 8) = v;
  }
  __builtin_amdgcn_wave_barrier();
}

// ---- pieces of the fused out-projection dgrad (rows_bwd_kernel<.., PROJ = true>) ----
// One LDS-DMA piece (1 KiB: lane l writes 16 bytes at lds_addr + 16 l) in SADDR form, as in gemm_mm32.hip: inline asm so that the
// piece stays in flight until OUR counted s_waitcnt vmcnt + s_barrier retire it; M0 is written in the statement that consumes it
// (tools/kernel_resources.py::m0_audit checks the ISA around every one of these after each build).
__device__ __forceinline__ void proj_glds(unsigned voff, const char* sbase, unsigned lds_addr) {
  asm volatile(
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %1"
      :
      : "v"(voff), "s"(sbase), "s"(lds_addr)
      : "memory");
}
template <int N> __device__ __forceinline__ void proj_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void proj_wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// this lane's 8 consecutive k per k-step of its own dY row (B operand of the k=32 product), four steps per slab.  Branch-free and
// unmasked on purpose: a load under an `if`, or a select right behind it, makes hipcc wait vmcnt(0) there, which would drain the DMA
// ring; wavefronts without a query tile and rows past Lq read the last row (the tile's padded rows are zeroed where it is stored).
__device__ __forceinline__ void proj_load_y(uint4 (&y)[4], const bf16_t* __restrict__ Yr, int s) {
#pragma unroll
  for (int u = 0; u < 4; ++u) y[u] = *reinterpret_cast<const uint4*>(Yr + s * PROJ_SLAB_K + 32 * u);
}

// ---- pieces of the fused QKV projection (rows_fwd_kernel<.., QKV = true>) ----
// one [192 rows][64 k] slab of Wqkv (rows sec*H + h*64 + 0..63 for sec = 0, 1, 2) -> registers: 1536 16-byte pieces
template <int WN>
__device__ __forceinline__ void qkv_load_w(uint4 (&w)[WN], const bf16_t* __restrict__ W, long ldw, int Hh, int h, int s, int tid, int nthr) {
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int p = tid + j * nthr, row = p >> 3;
    w[j] = make_uint4(0u, 0u, 0u, 0u);
    if (p < 192 * 8) w[j] = *reinterpret_cast<const uint4*>(W + (long)((row >> 6) * Hh + h * 64 + (row & 63)) * ldw + s * 64 + (p & 7) * 8);
  }
}
__device__ __forceinline__ void qkv_load_x(uint4 (&y)[2], const bf16_t* __restrict__ Xr, int s, bool computing, bool ok) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (computing) v = *reinterpret_cast<const uint4*>(Xr + s * 64 + 32 * u);
    v.x = ok ? v.x : 0u; v.y = ok ? v.y : 0u; v.z = ok ? v.z : 0u; v.w = ok ? v.w : 0u;
    y[u] = v;
  }
}
template <int WN>
__device__ __forceinline__ void qkv_commit_w(char* slab, const uint4 (&w)[WN], int tid, int nthr) {
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int p = tid + j * nthr;
    if (p < 192 * 8) *reinterpret_cast<uint4*>(slab + tile_off(p >> 3, p & 7)) = w[j];
  }
}

__device__ __forceinline__ float key_term(const uint8_t* km, int col, int Lk, int mask_mode) {
  if (col >= Lk) return -INFINITY;
  if (km && !km[col]) return mask_mode ? -INFINITY : -10000.0f;
  return 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward: grid = batch*heads, block = 64 * max(4, ceil(Lq/16)) threads; NKT = ceil(Lk/16)
// QKV = true (round 6, self-attention only: Lq == Lk, Q / K / V rows of one token block): the QKV projection (BertSelfAttention.query /
// key / value, vilmodel_cmt.py:108-110,115-117; MHA in_proj, common/transformer.py:138) is no longer a GEMM launch whose [B*L, 3H]
// result this kernel reads back.  The workgroup of (batch b, head h) computes its own 16*NKT x 192 tile first:
//   * C^T = W_h X^T with the k=32 MFMA: A operand = 8 consecutive k of a weight row from a [192 rows][64 k] slab in LDS (the three
//     64-row blocks sec*H + h*64 of Wqkv; plain ds_read_b128 in the swizzled tile layout), B operand = 8 consecutive k of the
//     wavefront's OWN 16 token rows straight from global; 12 accumulators (16 features x 16 tokens each) per wavefront;
//   * slabs travel global -> registers -> LDS one slab ahead of their use, ring of 2 x 24 KB that ALIASES the K / V tiles and
//     the output strips (only needed afterwards);
//   * + bias, rounded to bf16 exactly where the GEMM epilogue stored it; Q / K / V rows go to the stash through the wave's strip as
//     full 128-byte lines, K / V also into the LDS tiles, Q straight into the B-operand registers of S^T = K Q^T.
constexpr int QKV_SLAB_K = 64;                   // k per slab: [192][64] bf16 = 24 KB
constexpr int QKV_RING = 2;
constexpr int QKV_SLAB_BYTES = 192 * TQ;
// LDS of the forward kernel: K / V tiles, key terms, one output strip per wavefront; QKV: the ring aliases all of that and the head's
// 192 bias values sit behind whichever is longer
__host__ __device__ constexpr int rows_fwd_bias_off(int BKV, int nwaves) {
  const int base = 2 * BKV * TQ + BKV * 4 + nwaves * 16 * TP, ring = QKV_RING * QKV_SLAB_BYTES;
  return base < ring ? ring : base;
}
__host__ __device__ constexpr int rows_fwd_lds(int BKV, int nwaves, bool qkv) {
  return qkv ? rows_fwd_bias_off(BKV, nwaves) + 192 * 4 : 2 * BKV * TQ + BKV * 4 + nwaves * 16 * TP;
}

template <int NKT, bool HAS_DIST, bool QKV>
__global__ __launch_bounds__(512) void rows_fwd_kernel(const RowArgs a) {
  constexpr int BKV = NKT * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* kt = smem; char* vt = smem + BKV * TQ;
  float* kadd = reinterpret_cast<float*>(smem + 2 * BKV * TQ);
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x, b = bh / a.nh, h = bh % a.nh;
  char* strip = smem + 2 * BKV * TQ + BKV * 4 + wave * 16 * TP;
  const int q = wave * 16 + i, qc = min(q, a.Lq - 1);
  uint4 qf0, qf1;

  const int bk = a.kv_mod > 0 ? b % a.kv_mod : b;
  if constexpr (!QKV) {
    TileRegs<BKV> rk, rv;
    tile_fetch<BKV>(rk, a.K + (long)bk * a.Lk * a.ldk + h * 64, a.ldk, a.Lk, tid, nthr);
    tile_fetch<BKV>(rv, a.V + (long)bk * a.Lk * a.ldv + h * 64, a.ldv, a.Lk, tid, nthr);
    // this wavefront's 16 queries go straight into the B-operand registers (rows past Lq repeat the last one; never stored)
    const bf16_t* Qr = a.Q + ((long)b * a.Lq + qc) * a.ldq + h * 64 + g * 8;
    qf0 = *reinterpret_cast<const uint4*>(Qr); qf1 = *reinterpret_cast<const uint4*>(Qr + 32);
    if (tid < BKV) kadd[tid] = key_term(a.keymask ? a.keymask + (long)bk * a.Lk : nullptr, tid, a.Lk, a.mask_mode);
    tile_commit<BKV>(kt, rk, a.Lk, BKV, tid, nthr);
    tile_commit<BKV>(vt, rv, a.Lk, BKV, tid, nthr);
  } else {
    constexpr int NS = PROJ_K / QKV_SLAB_K, WN = 6;                 // WN * 256 threads >= 1536 16-byte pieces of a slab
    const int Hh = a.nh * 64;
    float* bias_l = reinterpret_cast<float*>(smem + rows_fwd_bias_off(BKV, nthr >> 6));
    const bool computing = wave < NKT, tok_ok = q < a.Lq;
    const bf16_t* Xr = a.X + ((long)b * a.Lq + qc) * a.ldx + g * 8;
    uint4 wr[WN], yb[2][2];
    f32x4_t acc[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (tid < 192) bias_l[tid] = a.bqkv ? a.bqkv[(tid >> 6) * Hh + h * 64 + (tid & 63)] : 0.f;
    qkv_load_w<WN>(wr, a.W, a.ldw, Hh, h, 0, tid, nthr); qkv_load_x(yb[0], Xr, 0, computing, tok_ok);
    qkv_commit_w<WN>(smem, wr, tid, nthr);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s + 1 < NS) { qkv_load_w<WN>(wr, a.W, a.ldw, Hh, h, s + 1, tid, nthr); qkv_load_x(yb[(s + 1) & 1], Xr, s + 1, computing, tok_ok); }
      if (computing) {
        const char* slab = smem + (s & 1) * QKV_SLAB_BYTES;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int t = 0; t < 12; ++t) acc[t] = mma32(frag(slab, 16 * t, u, lane), yb[s & 1][u], acc[t]);
      }
      if (s + 1 < NS) qkv_commit_w<WN>(smem + ((s + 1) & 1) * QKV_SLAB_BYTES, wr, tid, nthr);
      __syncthreads();                              // after the last slab: the ring is dead, K / V tiles and strips may land on it
    }
    if (tid < BKV) kadd[tid] = key_term(a.keymask ? a.keymask + (long)b * a.Lk : nullptr, tid, a.Lk, a.mask_mode);
    if (computing) {
      const int rows_valid = a.Lq - wave * 16;
#pragma unroll
      for (int sec = 0; sec < 3; ++sec) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float4 bb = *reinterpret_cast<const float4*>(bias_l + sec * 64 + 16 * t + 4 * g);
          const f32x4_t c = acc[sec * 4 + t];
          *reinterpret_cast<uint2*>(strip + i * TP + (16 * t + 4 * g) * 2) =
              make_uint2(pack_bf16(c[0] + bb.x, c[1] + bb.y), pack_bf16(c[2] + bb.z, c[3] + bb.w));
        }
        __builtin_amdgcn_wave_barrier();
        if (sec == 0) {
          qf0 = *reinterpret_cast<const uint4*>(strip + i * TP + g * 16);
          qf1 = *reinterpret_cast<const uint4*>(strip + i * TP + 64 + g * 16);
        }
        bf16_t* dst = const_cast<bf16_t*>(sec == 0 ? a.Q : sec == 1 ? a.K : a.V);
        const long ld = sec == 0 ? a.ldq : sec == 1 ? a.ldk : a.ldv;
        char* tile = sec == 1 ? kt : vt;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int c = lane + 64 * j, row = c >> 3, part = c & 7;
          uint4 v = *reinterpret_cast<const uint4*>(strip + row * TP + part * 16);
          if (row < rows_valid) *reinterpret_cast<uint4*>(dst + ((long)b * a.Lq + wave * 16 + row) * ld + h * 64 + part * 8) = v;
          else v = make_uint4(0u, 0u, 0u, 0u);
          if (sec > 0) *reinterpret_cast<uint4*>(tile + tile_off(wave * 16 + row, part)) = v;
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  __syncthreads();
  if (wave * 16 >= a.Lq) return;               // helper wavefronts of a short query axis only staged K / V

  float w = 0.f, b0 = 0.f;
  // this lane's distances, all in flight at once behind the score products (branch-free: a load under `if (key < Lk)` is waited
  // for with vmcnt(0), one full memory latency per element)
  float dd[HAS_DIST ? NKT : 1][4];
  if constexpr (HAS_DIST) {
    w = a.sp_w[0]; b0 = a.sp_b[0];
    const float* drow = a.dist + ((long)b * a.Lq + qc) * a.Lk;
#pragma unroll
    for (int n = 0; n < NKT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) dd[n][r] = drow[min(16 * n + 4 * g + r, a.Lk - 1)];
  }
  f32x4_t s[NKT];
#pragma unroll
  for (int n = 0; n < NKT; ++n) {
    s[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    s[n] = mma32(frag(kt, 16 * n, 0, lane), qf0, s[n]);
    s[n] = mma32(frag(kt, 16 * n, 1, lane), qf1, s[n]);
  }
  float mx = -INFINITY;
#pragma unroll
  for (int n = 0; n < NKT; ++n) {
    const float4 ka4 = *reinterpret_cast<const float4*>(kadd + 16 * n + 4 * g);
    const float ka[4] = {ka4.x, ka4.y, ka4.z, ka4.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = s[n][r] * a.alpha + ka[r];
      if constexpr (HAS_DIST) {
        const int key = 16 * n + 4 * g + r;
        const float vb = v + (w * dd[n][r] + b0);
        v = key < a.Lk ? vb : v;
      }
      s[n][r] = v;
      mx = fmaxf(mx, v);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int n = 0; n < NKT; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __expf(s[n][r] - mx);
      s[n][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
  if (g == 0 && q < a.Lq) a.lse[(long)bh * a.Lq + q] = mx + __logf(sum);

  short4_t pb[NKT];
  const bool dropping = a.drop.p > 0.f;
  const uint32_t rbase = ((uint32_t)bh * a.Lq + q) * (uint32_t)a.Lk;
#pragma unroll
  for (int n = 0; n < NKT; ++n) {
    float p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = s[n][r] * inv;
    if (dropping) {
      float dm[4];
      drop_mult_run<4>(a.drop.seed, rbase + 16 * n + 4 * g, a.drop.p, a.drop.inv_keep, dm);
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] *= dm[r];
    }
    pb[n] = pack4(p[0], p[1], p[2], p[3]);
  }
  f32x4_t o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int n = 0; n < NKT; ++n)
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = mma16(frag_t4(vt, 16 * n, 16 * t, lane), pb[n], o[t]);
  store_rows16(strip, o, 1.0f, a.ctx + ((long)b * a.Lq + wave * 16) * a.ldc + h * 64, a.ldc, a.Lq - wave * 16, lane);
}

// ---------------------------------------------------------------------------------------------------------------------
// backward: grid = batch*heads, block = 64 * max(4, ceil(Lq/16), ceil(Lk/16)) threads
struct BwdLds {                                  // byte offsets for BQ = 16*ceil(Lq/16) query rows and BKV key rows
  int q, d, k, v, kadd, lse, D, red, strip, ring, total;
  __host__ __device__ BwdLds(int BQ, int BKV, bool proj = false) {
    d = 0; q = BQ * TQ; k = 2 * BQ * TQ; v = k + BKV * TQ; kadd = v + BKV * TQ;
    lse = kadd + BKV * 4; D = lse + 128 * 4; red = D + 128 * 4; strip = red + 16 * 4; total = strip + 8 * 16 * TP;
    // the W slabs of the fused out-projection dgrad live where Q / K / V / the strips go AFTER the prologue (dO stays outside)
    ring = BQ * TQ;
    if (proj && total < ring + PROJ_RING * PROJ_SLAB_K * TQ) total = ring + PROJ_RING * PROJ_SLAB_K * TQ;
  }
};

// PROJ = true: the out-projection's input gradient (BertSelfOutput.dense, vilmodel_cmt.py:150-154; BertOutAttention /
// MHA out_proj alike) is no longer a GEMM launch of its own whose [B*Lq, H] result this kernel reads back as dO.  The workgroup of
// (batch b, head h) computes its own 16*nqt x 64 tile  dO = dY[b rows, 0:Kp] . W[0:Kp, h*64 : h*64+64]  first:
//   * dO^T = W_h^T dY^T with the k=32 MFMA: B operand = 8 consecutive k of the wavefront's OWN 16 rows of dY straight from global
//     (one 16-byte load per lane and k-step, no sharing between wavefronts, nothing staged); A operand = W_h^T taken DOWN the rows
//     of a [128 k][64] slab in LDS by two ds_read_b64_tr_b16 -- the slab's rows are stored permuted (k = 8g+e -> row 4g+e, 16+4g+e-4
//     within each 32) so that the two transposed reads of lane group g return exactly the 8 consecutive k its B operand holds and
//     both reads keep frag_t4's conflict-free row pattern;
//   * slabs travel global -> LDS by LDS-DMA (global_load_lds_dwordx4 in SADDR form, 16 one-KiB pieces per slab issued by wavefronts
//     0..3, no register staging), two slabs in flight behind the one being read, in a ring of 3 x 16 KB that ALIASES the Q / K / V
//     tiles and the output strips (only needed afterwards): the kernel's LDS footprint is unchanged.  The DMA writes lane-linear, so
//     the row permutation and the chunk swizzle are applied to the SOURCE address.  Hand-over per slab: counted s_waitcnt vmcnt (the
//     next slab and its dY landed, the one behind may stay in flight), lgkmcnt(0), raw s_barrier -- never __syncthreads(), whose
//     fence would drain the ring.  Without the 32 staging registers every instantiation up to 80 keys needs <= 116 VGPRs (138 with the
//     distance bias at 65..80 keys, whose plain kernel already takes 126), against 160..164 before: two five-wavefront workgroups
//     co-reside on a CU whatever SIMDs the dispatcher picks;
//   * Q / K / V are fetched behind the last hand-over (no DMA outstanding, so the compiler's own wait counts are exact again) and
//     travel under the last slab's MFMAs.  They cannot come earlier without holding 40 registers through the prologue, and role A's
//     score half cannot start before the ring is dead: its K tile lives where the ring is;
//   * tried and removed: splitting the reduction over the wavefronts that own no query tile (partial tiles summed through LDS).  The
//     prologue waits for slabs, not for MFMAs: graph -> text 16 x 80 at 384 workgroups 16.2 us with the split against 13.7 without,
//     graph 16 x 16 12.6 against 10.6 (profiles/attn_fold_bench.txt);
//   * the result lands in the dO tile as the same bf16 values the GEMM epilogue stored (round-to-nearest-even of the fp32 sum).
// What it removes per attention block: one 128x64-class launch (8 us chained for the text rows) + its boundary, 3.9 MB written
// and read back.
template <int NKT, bool HAS_DIST, bool PROJ>
__global__ __launch_bounds__(512) void rows_bwd_kernel(const RowArgs a) {
  constexpr int BKV = NKT * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nqt = (a.Lq + 15) >> 4, BQ = nqt * 16;
  const BwdLds L(BQ, BKV, PROJ);
  char *qt = smem + L.q, *dt = smem + L.d, *kt = smem + L.k, *vt = smem + L.v;
  float* kadd = reinterpret_cast<float*>(smem + L.kadd);
  float* lse = reinterpret_cast<float*>(smem + L.lse);
  float* Dl = reinterpret_cast<float*>(smem + L.D);
  float* red = reinterpret_cast<float*>(smem + L.red);
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x, b = bh / a.nh, h = bh % a.nh;
  const bool dropping = a.drop.p > 0.f;
  char* strip = smem + L.strip + wave * 16 * TP;

  {
    TileRegs<128> rq, rd;
    TileRegs<BKV> rk, rv;
    const int bk = a.kv_mod > 0 ? b % a.kv_mod : b;
#define FETCH_QKV()                                                                                        \
    tile_fetch<128>(rq, a.Q + (long)b * a.Lq * a.ldq + h * 64, a.ldq, a.Lq, tid, nthr);                     \
    tile_fetch<BKV>(rk, a.K + (long)bk * a.Lk * a.ldk + h * 64, a.ldk, a.Lk, tid, nthr);                    \
    tile_fetch<BKV>(rv, a.V + (long)bk * a.Lk * a.ldv + h * 64, a.ldv, a.Lk, tid, nthr)
    if constexpr (!PROJ) {
      FETCH_QKV();
      tile_fetch<128>(rd, a.dO + (long)b * a.Lq * a.ldd + h * 64, a.ldd, a.Lq, tid, nthr);
    } else {
      constexpr int SLAB = PROJ_SLAB_K * TQ, NS = PROJ_K / PROJ_SLAB_K, NP = 4;     // NP 1-KiB DMA pieces per loader wavefront and slab
      char* ring = smem + L.ring;
      const int wv = __builtin_amdgcn_readfirstlane(wave);
      const bool computing = wv < nqt, loader = wv < 4;
      const int qrow = wv * 16 + i;
      const bool qok = qrow < a.Lq;
      const bf16_t* Yr = a.dO + ((long)b * a.Lq + min(qrow, a.Lq - 1)) * a.ldd + g * 8;
      // DMA plan of the loader wavefronts 0..3: piece 4c + wv of a slab = its LDS rows 32c + 8wv .. +7, lane -> row R = .. + (lane >> 3),
      // physical chunk lane & 7.  The DMA writes lane-linear, so both the row permutation (LDS row R holds k = the inverse of
      // k = 8g+e -> row 4g+e | 16+4g+e-4, inside every 32) and the chunk swizzle go on the SOURCE address
      const int r5 = 8 * (wv & 3) + (lane >> 3);
      const int kk = (r5 & 3) | ((r5 & 0x10) >> 2) | ((r5 & 0xc) << 1);
      const unsigned voff = (unsigned)(((long)kk * a.ldw + (((lane & 7) ^ (r5 & 7)) << 3)) * 2);
      const char* wbase = reinterpret_cast<const char*>(a.W + h * 64);
      const long piece_stride = 32 * a.ldw * 2, slab_stride = (long)PROJ_SLAB_K * a.ldw * 2;
      const unsigned piece0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)ring) + (unsigned)(wv & 3) * 1024u;
      auto issue_slab = [&](int s) {
        if (loader) {
#pragma unroll
          for (int c = 0; c < NP; ++c) proj_glds(voff, wbase + s * slab_stride + c * piece_stride, piece0 + (unsigned)((s % PROJ_RING) * SLAB + c * 4096));
        }
      };
      uint4 yb[2][4];
      f32x4_t acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      // Order of the vector-memory issues (they retire in order, and the compiler does not count the DMA pieces): the dY loads of slab
      // s+1 go out BEFORE the pieces of slab s+2 (those of slabs 0 and 1 before the whole ring), so that "at most the NP youngest
      // outstanding" at a hand-over means slab s+1 and its dY both landed.
      proj_load_y(yb[0], Yr, 0);
      proj_load_y(yb[1], Yr, 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < PROJ_RING; ++s) issue_slab(s);
      __builtin_amdgcn_sched_barrier(0);
      if (loader) proj_wait_vm<2 * NP>(); else proj_wait_vm<0>();
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (s >= 1 && s + 1 < NS) proj_load_y(yb[(s + 1) & 1], Yr, s + 1);
        __builtin_amdgcn_sched_barrier(0);
        // slab s+2 into the slot slab s-1 left (every wavefront's reads of it retired at the hand-over just passed)
        if (s >= 1 && s + 2 < NS) issue_slab(s + 2);
        __builtin_amdgcn_sched_barrier(0);
        // Q / K / V take the load slot behind the last hand-over: no DMA is outstanding any more, the compiler's own counts are exact
        if (s + 1 == NS) { FETCH_QKV(); }
        if (computing) {
          const char* slab = ring + (s % PROJ_RING) * SLAB;
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const short4_t lo = frag_t4(slab, 32 * u, 16 * t, lane), hi = frag_t4(slab, 32 * u + 16, 16 * t, lane);
              const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
              acc[t] = mma32(make_uint4(l2.x, l2.y, h2.x, h2.y), yb[s & 1][u], acc[t]);
            }
        }
        if (s + 1 < NS) {                           // hand-over: slab s+1 landed (slab s+2 may stay in flight), my reads of slab s retired
          __builtin_amdgcn_sched_barrier(0);
          if (loader && s + 2 < NS) proj_wait_vm<NP>(); else proj_wait_vm<0>();
          proj_wait_lgkm0();
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (computing) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          *reinterpret_cast<uint2*>(dt + tile_off(16 * wv + i, 2 * t + (g >> 1)) + (g & 1) * 8) =
              qok ? make_uint2(pack_bf16(acc[t][0], acc[t][1]), pack_bf16(acc[t][2], acc[t][3])) : make_uint2(0u, 0u);
      }
      __syncthreads();                            // the ring is dead: Q / K / V and the row vectors may land on it
    }
#undef FETCH_QKV
    if (tid < BKV) kadd[tid] = key_term(a.keymask ? a.keymask + (long)bk * a.Lk : nullptr, tid, a.Lk, a.mask_mode);
    // padded query rows: lse = +inf makes their recomputed probabilities exactly 0
    if (tid < 128) lse[tid] = tid < a.Lq ? a.lse[(long)bh * a.Lq + tid] : INFINITY;
    tile_commit<128>(qt, rq, a.Lq, BQ, tid, nthr);
    if constexpr (!PROJ) tile_commit<128>(dt, rd, a.Lq, BQ, tid, nthr);
    tile_commit<BKV>(kt, rk, a.Lk, BKV, tid, nthr);
    tile_commit<BKV>(vt, rv, a.Lk, BKV, tid, nthr);
  }
  float w = 0.f, b0 = 0.f;
  if constexpr (HAS_DIST) { w = a.sp_w[0]; b0 = a.sp_b[0]; }
  __syncthreads();

  // ---- role A: 16 queries x all keys -> D, dQ (and the sprel gradients) ----
  float aw = 0.f, ab = 0.f;
  if (wave < nqt) {
    const int q = wave * 16 + i;
    const bool qok = q < a.Lq;
    const uint4 qf0 = frag(qt, 16 * wave, 0, lane), qf1 = frag(qt, 16 * wave, 1, lane);
    const uint4 df0 = frag(dt, 16 * wave, 0, lane), df1 = frag(dt, 16 * wave, 1, lane);
    const float lse_i = lse[q];
    const float* drow = HAS_DIST ? a.dist + ((long)b * a.Lq + min(q, a.Lq - 1)) * a.Lk : nullptr;
    const uint32_t rbase = ((uint32_t)bh * a.Lq + q) * (uint32_t)a.Lk;
    f32x4_t p[NKT], dp[NKT];
    float dv4[NKT][4];                            // pairwise distances of this lane's elements (HAS_DIST only)
    float Dp = 0.f;
#pragma unroll
    for (int n = 0; n < NKT; ++n) {
      f32x4_t st = f32x4_t{0.f, 0.f, 0.f, 0.f}, dpt = f32x4_t{0.f, 0.f, 0.f, 0.f};
      st = mma32(frag(kt, 16 * n, 0, lane), qf0, st);
      st = mma32(frag(kt, 16 * n, 1, lane), qf1, st);
      dpt = mma32(frag(vt, 16 * n, 0, lane), df0, dpt);
      dpt = mma32(frag(vt, 16 * n, 1, lane), df1, dpt);
      const float4 ka4 = *reinterpret_cast<const float4*>(kadd + 16 * n + 4 * g);
      const float ka[4] = {ka4.x, ka4.y, ka4.z, ka4.w};
      float dm[4] = {1.f, 1.f, 1.f, 1.f};
      if (dropping) drop_mult_run<4>(a.drop.seed, rbase + 16 * n + 4 * g, a.drop.p, a.drop.inv_keep, dm);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * n + 4 * g + r;
        float v = st[r] * a.alpha + ka[r];
        if constexpr (HAS_DIST) {
          const float dd = (qok && key < a.Lk) ? drow[key] : 0.f;
          dv4[n][r] = dd;
          if (key < a.Lk) v += w * dd + b0;
        }
        const float pe = __expf(v - lse_i);
        const float dpv = dpt[r] * dm[r];                  // d P = d P_drop * mask/(1-p)
        p[n][r] = pe; dp[n][r] = dpv;
        Dp += pe * dpv;
      }
    }
    Dp += __shfl_xor(Dp, 16, 64);
    Dp += __shfl_xor(Dp, 32, 64);
    if (g == 0) Dl[q] = Dp;
    short4_t dsb[NKT];
#pragma unroll
    for (int n = 0; n < NKT; ++n) {
      float ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ds[r] = p[n][r] * (dp[n][r] - Dp);
        if constexpr (HAS_DIST) { aw += ds[r] * dv4[n][r]; ab += ds[r]; }
      }
      dsb[n] = pack4(ds[0], ds[1], ds[2], ds[3]);
    }
    f32x4_t dq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dq[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < NKT; ++n)
#pragma unroll
      for (int t = 0; t < 4; ++t) dq[t] = mma16(frag_t4(kt, 16 * n, 16 * t, lane), dsb[n], dq[t]);
    store_rows16(strip, dq, a.alpha, a.dQ + ((long)b * a.Lq + wave * 16) * a.lddq + h * 64, a.lddq, a.Lq - wave * 16, lane);
  }
  if constexpr (HAS_DIST) {
    aw = wave_sum(aw); ab = wave_sum(ab);
    if (lane == 0) { red[wave] = aw; red[8 + wave] = ab; }
  }
  __syncthreads();
  if constexpr (HAS_DIST) {     // d sprel_linear.{weight,bias} (vilmodel_cmt.py:732-736): one atomic pair per workgroup
    if (tid == 0 && a.d_sp_w != nullptr) {
      float sw = 0.f, sb = 0.f;
      for (int k = 0; k < (nthr >> 6); ++k) { sw += red[k]; sb += red[8 + k]; }
      atomicAdd(a.d_sp_w, sw);
      atomicAdd(a.d_sp_b, sb);
    }
  }

  // ---- role B: 16 keys x all queries -> dK, dV ----
  if (wave * 16 < a.Lk) {
    const int key = wave * 16 + i;
    const bool kok = key < a.Lk;
    const uint4 kf0 = frag(kt, 16 * wave, 0, lane), kf1 = frag(kt, 16 * wave, 1, lane);
    const uint4 vf0 = frag(vt, 16 * wave, 0, lane), vf1 = frag(vt, 16 * wave, 1, lane);
    const float ka = kadd[key];
    f32x4_t dv[4], dk[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { dv[t] = f32x4_t{0.f, 0.f, 0.f, 0.f}; dk[t] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    for (int m = 0; m < nqt; ++m) {
      f32x4_t s = f32x4_t{0.f, 0.f, 0.f, 0.f}, dpm = f32x4_t{0.f, 0.f, 0.f, 0.f};
      s = mma32(frag(qt, 16 * m, 0, lane), kf0, s);
      s = mma32(frag(qt, 16 * m, 1, lane), kf1, s);
      dpm = mma32(frag(dt, 16 * m, 0, lane), vf0, dpm);
      dpm = mma32(frag(dt, 16 * m, 1, lane), vf1, dpm);
      const float4 l4 = *reinterpret_cast<const float4*>(lse + 16 * m + 4 * g);
      const float4 D4 = *reinterpret_cast<const float4*>(Dl + 16 * m + 4 * g);
      const float lr[4] = {l4.x, l4.y, l4.z, l4.w}, Dr[4] = {D4.x, D4.y, D4.z, D4.w};
      float pd[4], ds[4];
      float dd[4] = {0.f, 0.f, 0.f, 0.f};         // the four distances of this step in flight together (branch-free, see rows_fwd_kernel)
      if constexpr (HAS_DIST) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dd[r] = a.dist[((long)b * a.Lq + min(16 * m + 4 * g + r, a.Lq - 1)) * a.Lk + min(key, a.Lk - 1)];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qq = 16 * m + 4 * g + r;
        float v = s[r] * a.alpha + ka;
        if constexpr (HAS_DIST) {
          const float vb = v + (w * dd[r] + b0);
          v = (kok && qq < a.Lq) ? vb : v;
        }
        const float pe = __expf(v - lr[r]);
        float mult = 1.0f;
        if (dropping) mult = drop_mult(a.drop.seed, ((uint32_t)bh * a.Lq + qq) * (uint32_t)a.Lk + key, a.drop.p, a.drop.inv_keep);
        pd[r] = pe * mult;
        ds[r] = pe * (dpm[r] * mult - Dr[r]);
      }
      const short4_t pb = pack4(pd[0], pd[1], pd[2], pd[3]), dsb = pack4(ds[0], ds[1], ds[2], ds[3]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        dv[t] = mma16(frag_t4(dt, 16 * m, 16 * t, lane), pb, dv[t]);
        dk[t] = mma16(frag_t4(qt, 16 * m, 16 * t, lane), dsb, dk[t]);
      }
    }
    store_rows16(strip, dv, 1.0f, a.dV + ((long)b * a.Lk + wave * 16) * a.lddv + h * 64, a.lddv, a.Lk - wave * 16, lane);
    store_rows16(strip, dk, a.alpha, a.dK + ((long)b * a.Lk + wave * 16) * a.lddk + h * 64, a.lddk, a.Lk - wave * 16, lane);
  }
}

template <int NKT, bool HAS_DIST, bool QKV> int launch_rows_fwd_q(const RowArgs& k, int blocks, int threads, hipStream_t st) {
  const int smem = rows_fwd_lds(NKT * 16, threads / 64, QKV);
  auto kern = rows_fwd_kernel<NKT, HAS_DIST, QKV>;
  if (smem > 64 * 1024) ETP_CHECK_HIP(ensure_dyn_lds(reinterpret_cast<const void*>(kern), smem));
  ETP_LAUNCH_ROW(ROWF_ATTN_FWD, kern, dim3(blocks), dim3(threads), smem, st, k);
  ETP_CHECK_LAUNCH(QKV ? "attn_rows_fwd_qkv" : "attn_rows_fwd");
  return ETP_OK;
}
template <int NKT, bool HAS_DIST> int launch_rows_fwd(const RowArgs& k, int blocks, int threads, hipStream_t st) {
  return k.X ? launch_rows_fwd_q<NKT, HAS_DIST, true>(k, blocks, threads, st) : launch_rows_fwd_q<NKT, HAS_DIST, false>(k, blocks, threads, st);
}
template <int NKT, bool HAS_DIST, bool PROJ> int launch_rows_bwd_p(const RowArgs& k, int blocks, int threads, hipStream_t st) {
  const BwdLds L(((k.Lq + 15) >> 4) * 16, NKT * 16, PROJ);
  auto kern = rows_bwd_kernel<NKT, HAS_DIST, PROJ>;
  ETP_CHECK_HIP(ensure_dyn_lds(reinterpret_cast<const void*>(kern), BwdLds(128, NKT * 16, PROJ).total));
  ETP_LAUNCH_ROW(ROWF_ATTN_BWD, kern, dim3(blocks), dim3(threads), L.total, st, k);
  ETP_CHECK_LAUNCH(PROJ ? "attn_rows_bwd_proj" : "attn_rows_bwd");
  return ETP_OK;
}
template <int NKT, bool HAS_DIST> int launch_rows_bwd(const RowArgs& k, int blocks, int threads, hipStream_t st) {
  return k.W ? launch_rows_bwd_p<NKT, HAS_DIST, true>(k, blocks, threads, st) : launch_rows_bwd_p<NKT, HAS_DIST, false>(k, blocks, threads, st);
}

template <bool HAS_DIST> int dispatch_fwd(int nkt, const RowArgs& k, int blocks, int threads, hipStream_t st) {
  switch (nkt) {
    case 1: return launch_rows_fwd<1, HAS_DIST>(k, blocks, threads, st);
    case 2: return launch_rows_fwd<2, HAS_DIST>(k, blocks, threads, st);
    case 3: return launch_rows_fwd<3, HAS_DIST>(k, blocks, threads, st);
    case 4: return launch_rows_fwd<4, HAS_DIST>(k, blocks, threads, st);
    case 5: return launch_rows_fwd<5, HAS_DIST>(k, blocks, threads, st);
    case 6: return launch_rows_fwd<6, HAS_DIST>(k, blocks, threads, st);
    case 7: return launch_rows_fwd<7, HAS_DIST>(k, blocks, threads, st);
    default: return launch_rows_fwd<8, HAS_DIST>(k, blocks, threads, st);
  }
}
template <bool HAS_DIST> int dispatch_bwd(int nkt, const RowArgs& k, int blocks, int threads, hipStream_t st) {
  switch (nkt) {
    case 1: return launch_rows_bwd<1, HAS_DIST>(k, blocks, threads, st);
    case 2: return launch_rows_bwd<2, HAS_DIST>(k, blocks, threads, st);
    case 3: return launch_rows_bwd<3, HAS_DIST>(k, blocks, threads, st);
    case 4: return launch_rows_bwd<4, HAS_DIST>(k, blocks, threads, st);
    case 5: return launch_rows_bwd<5, HAS_DIST>(k, blocks, threads, st);
    case 6: return launch_rows_bwd<6, HAS_DIST>(k, blocks, threads, st);
    case 7: return launch_rows_bwd<7, HAS_DIST>(k, blocks, threads, st);
    default: return launch_rows_bwd<8, HAS_DIST>(k, blocks, threads, st);
  }
}

RowArgs make_row_args(int nh, const AttnBuf& a, void* P, float alpha, Drop drop) {
  RowArgs k;
  memset(&k, 0, sizeof(k));
  k.Q = (const bf16_t*)a.Q; k.K = (const bf16_t*)a.K; k.V = (const bf16_t*)a.V; k.ldq = a.ldq; k.ldk = a.ldk; k.ldv = a.ldv;
  k.lse = (float*)P; k.nh = nh; k.Lq = a.Lq; k.Lk = a.Lk; k.drop = drop;
  k.keymask = a.keymask; k.mask_mode = a.mask_mode; k.dist = a.dist; k.sp_w = a.sp_w; k.sp_b = a.sp_b; k.alpha = alpha;
  k.kv_mod = a.kv_mod;
  return k;
}

}  // namespace

// bf16, both axes <= 128, 16-byte aligned operands; the probability buffer must hold Lq fp32 per (batch, head)
bool attn_rows_ok(int dt, const AttnBuf& a, long ldc) {
  const bool on = opt_on(OPT_ATTN_ROWS, true);
  if (!on || dt != ETP_BF16) return false;
  if (a.Lq > 128 || a.Lk > 128 || a.Lq < 1 || a.Lk < 1 || a.ldS < 2) return false;
  if (a.ldq % 8 || a.ldk % 8 || a.ldv % 8 || ldc % 8) return false;
  if (((uintptr_t)a.Q | (uintptr_t)a.K | (uintptr_t)a.V) % 16) return false;
  if (a.dist != nullptr && (a.sp_w == nullptr || a.sp_b == nullptr)) return false;
  return true;
}

// MEASUREMENT ONLY (tools/r03_call20.sh): ETP_SKIP_ATTN = "fwd" / "bwd" drops the launches so that the step time shows what
// the attention kernels cost in the step (results are wrong in that mode); see ETP_SKIP_LN in norm.hip.
static bool skip_attn(const char* what) {
#ifdef ETP_EXPERIMENTS       // measurement builds only (tools/build_variant.sh ... -DETP_EXPERIMENTS): never in the shipped library
  const char* e = opt_str(OPT_SKIP_ATTN);
  return e && strstr(e, what) != nullptr;
#else
  (void)what;
  return false;
#endif
}

// fused QKV projection: self-attention blocks (one token axis) of a 768-wide model
bool attn_rows_qkv_ok(int nh, const AttnBuf& a, const void* X, long ldx, const void* W, long ldw) {
  return nh * 64 == PROJ_K && a.Lq == a.Lk && a.kv_mod == 0 && ldx % 8 == 0 && ldw % 8 == 0 &&
         ((uintptr_t)X | (uintptr_t)W) % 16 == 0;
}

int attn_rows_fwd(int nh, const AttnBuf& a, void* P, void* ctx, long ldc, float alpha, hipStream_t st, Drop drop, const void* qkv_x,
                  long qkv_ldx, const void* qkv_w, long qkv_ldw, const float* qkv_b) {
  ETP_REQUIRE((uintptr_t)ctx % 16 == 0, "ctx must be 16-byte aligned");
  ETP_REQUIRE(qkv_x == nullptr || attn_rows_qkv_ok(nh, a, qkv_x, qkv_ldx, qkv_w, qkv_ldw), "fused QKV projection: unsupported shape / alignment");
  if (skip_attn("fwd")) return ETP_OK;
  RowArgs k = make_row_args(nh, a, P, alpha, drop);
  k.ctx = (bf16_t*)ctx; k.ldc = ldc;
  k.X = (const bf16_t*)qkv_x; k.ldx = qkv_ldx; k.bqkv = qkv_b;
  if (qkv_x) { k.W = (const bf16_t*)qkv_w; k.ldw = qkv_ldw; k.Kp = nh * 64; }
  const int nqt = (a.Lq + 15) / 16, nkt = (a.Lk + 15) / 16;
  const int threads = 64 * (nqt > 4 ? nqt : 4);
  return a.dist ? dispatch_fwd<true>(nkt, k, a.B * nh, threads, st) : dispatch_fwd<false>(nkt, k, a.B * nh, threads, st);
}

// the fused form is built for the reduction length 768 (BERT-base / XLM-R-base hidden size: the reference's only planners)
bool attn_rows_proj_ok(int Kp, const void* W, long ldw) {
  return Kp == PROJ_K && ldw % 8 == 0 && (uintptr_t)W % 16 == 0;
}

int attn_rows_bwd(int nh, const AttnBuf& a, const void* P, const void* dctx, long ldd, void* dQ, long lddq, void* dK, long lddk,
                  void* dV, long lddv, float alpha, float* d_sp_w, float* d_sp_b, hipStream_t st, Drop drop, const void* proj_w,
                  long proj_ldw, int proj_k) {
  ETP_REQUIRE(ldd % 8 == 0 && lddq % 8 == 0 && lddk % 8 == 0 && lddv % 8 == 0 &&
                  ((uintptr_t)dctx | (uintptr_t)dQ | (uintptr_t)dK | (uintptr_t)dV) % 16 == 0,
              "gradient operands of the register-resident attention must be 16-byte aligned");
  ETP_REQUIRE(proj_w == nullptr || attn_rows_proj_ok(proj_k, proj_w, proj_ldw), "fused out-projection dgrad: unsupported reduction length / alignment");
  ETP_REQUIRE(!a.dkv_sum, "dK/dV summed per instruction (AttnBuf::dkv_sum) needs the streaming attention kernels (bf16, an axis > 128): "
                          "the register-resident kernels write them per stacked episode");
  if (skip_attn("bwd")) return ETP_OK;
  RowArgs k = make_row_args(nh, a, const_cast<void*>(P), alpha, drop);
  k.dO = (const bf16_t*)dctx; k.ldd = ldd;
  k.W = (const bf16_t*)proj_w; k.ldw = proj_ldw; k.Kp = proj_k;
  k.dQ = (bf16_t*)dQ; k.dK = (bf16_t*)dK; k.dV = (bf16_t*)dV; k.lddq = lddq; k.lddk = lddk; k.lddv = lddv;
  k.d_sp_w = d_sp_w; k.d_sp_b = d_sp_b;
  const int nqt = (a.Lq + 15) / 16, nkt = (a.Lk + 15) / 16;
  int nw = nqt > nkt ? nqt : nkt;
  if (nw < 4) nw = 4;
  return a.dist ? dispatch_bwd<true>(nkt, k, a.B * nh, 64 * nw, st) : dispatch_bwd<false>(nkt, k, a.B * nh, 64 * nw, st);
}

}  // namespace etp
