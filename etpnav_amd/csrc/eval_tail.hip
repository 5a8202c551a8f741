// Validation tails of the two pre-training tasks, and the counters that stay on the device across batches.
//
// Replaces, per validation batch, the statements of validate_mlm / validate_sap (pretrain_src/pretrain_src/train_r2r.py:355-380,
// :416-444): F.cross_entropy(scores, labels, reduction='sum'), scores.max(dim=-1)[1] / torch.argmax(logits, 1), the comparison with
// the labels and the three running sums -- without the gradient-sized dlogits matrix of the training tails, without float atomics and
// without a host synchronisation per batch.
//
// Three kernels.  vocab_eval_kernel and sap_eval_kernel write, per row, the negative log-likelihood (fp32) and the arg-max column
// (int32); eval_accum_kernel folds those rows into one 32-byte record {double loss_sum; int64 n_correct, n_rows, n_counted} that the
// host reads once per task.  Plain vector stores only: no atomics, no scratch, LDS only for the cross-wave combines.  Every order
// of summation is fixed by the thread index, so a second run on the same inputs gives the same bits.
//
// Semantics (pinned to torch on the CPU by tests/test_eval_ref_cpu.py):
//   * ties of the maximum go to the LOWEST column (torch.max / torch.argmax on the CPU);
//   * a label on a -inf logit gives nll = +inf;
//   * a row of only -inf gives pred 0 and a NaN nll;
//   * a label that is neither ignore_index nor a column gives a NaN nll and is never used as an index.
// PRECONDITION: no NaN in the logits (a NaN compares false both ways, so the pair combine below would skip it where torch
// propagates it).
#include "kernels.h"

namespace etp {

namespace {
constexpr int NO_COL = 0x7fffffff;

// (value, column) pairs: the larger value wins, on equal values the smaller column
__device__ __forceinline__ void pair_take(float& v, int& c, float ov, int oc) {
  if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; }
}
__device__ __forceinline__ void wave_argmax(float& v, int& c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oc = __shfl_xor(c, o, 64);
    pair_take(v, c, ov, oc);
  }
}
// a thread's strided columns: the first one is taken as it is (so a row of -inf still names a column), afterwards strict >, which
// keeps the thread's lowest column among equals
__device__ __forceinline__ void strided_argmax(const float* __restrict__ s, int n, int first, int stride, float& v, int& c) {
  v = -INFINITY;
  c = NO_COL;
  for (int k = first; k < n; k += stride) {
    const float x = s[k];
    if (c == NO_COL || x > v) { v = x; c = k; }
  }
}
}  // namespace

// One workgroup of 256 threads per masked row.  logits fp32 [Nm, ldv]; columns >= V are padding and are not read.  The row sum runs in
// vocab_ce_kernel's order (embed.hip): thread-strided, wave_sum, red[0] + red[1] + red[2] + red[3].
__global__ __launch_bounds__(256) void vocab_eval_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                         float* __restrict__ row_nll, int32_t* __restrict__ row_pred, int V, int ldv) {
  __shared__ float red[4];
  __shared__ int redc[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* s = logits + (long)row * ldv;
  float mx;
  int col;
  strided_argmax(s, V, tid, 256, mx, col);
  wave_argmax(mx, col);
  if (lane == 0) { red[wave] = mx; redc[wave] = col; }
  __syncthreads();
  mx = red[0];
  col = redc[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) pair_take(mx, col, red[w], redc[w]);
  __syncthreads();
  float sum = 0.f;
  for (int k = tid; k < V; k += 256) sum += expf(s[k] - mx);
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    const float lse = mx + logf(red[0] + red[1] + red[2] + red[3]);
    const long y = labels[row];
    float nll = __builtin_nanf("");
    if (y >= 0 && y < V) nll = lse - s[y];
    row_nll[row] = nll;
    row_pred[row] = col;
  }
}

// One wavefront per row, four per workgroup.  logits fp32 [B, G] with -inf on the masked nodes; max / sum / lse in sap_ce_kernel's
// order (embed.hip).  A row whose label is ignore_index writes nll = 0; its pred is still the arg-max.
__global__ __launch_bounds__(256) void sap_eval_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                       float* __restrict__ row_nll, int32_t* __restrict__ row_pred, int B, int G,
                                                       long ignore_index) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const float* s = logits + (long)row * G;
  float mx;
  int col;
  strided_argmax(s, G, lane, 64, mx, col);
  wave_argmax(mx, col);
  float sum = 0.f;
  for (int k = lane; k < G; k += 64) sum += expf(s[k] - mx);
  sum = wave_sum(sum);
  if (lane == 0) {
    const float lse = mx + logf(sum);
    const long y = labels[row];
    float nll = __builtin_nanf("");
    if (y == ignore_index) nll = 0.f;
    else if (y >= 0 && y < G) nll = lse - s[y];
    row_nll[row] = nll;
    row_pred[row] = col;
  }
}

// One workgroup of 256 threads: thread t adds rows t, t + 256, ... in ascending order in double (ignored rows add nothing to the loss
// and nothing to n_correct), a fixed-order LDS tree follows, and thread 0 adds the totals to the record.
__global__ __launch_bounds__(256) void eval_accum_kernel(const float* __restrict__ row_nll, const int32_t* __restrict__ row_pred,
                                                         const int64_t* __restrict__ labels, int n, long ignore_index,
                                                         etp_eval_record* __restrict__ acc) {
  __shared__ double sl[256];
  __shared__ int sc[256], sk[256];
  const int t = threadIdx.x;
  double loss = 0.0;
  int correct = 0, counted = 0;
  for (int r = t; r < n; r += 256) {
    const long y = labels[r];
    if (y == ignore_index) continue;
    loss += (double)row_nll[r];
    correct += (long)row_pred[r] == y ? 1 : 0;
    counted += 1;
  }
  sl[t] = loss;
  sc[t] = correct;
  sk[t] = counted;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      sl[t] += sl[t + o];
      sc[t] += sc[t + o];
      sk[t] += sk[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    etp_eval_record r = *acc;
    r.loss_sum += sl[0];
    r.n_correct += sc[0];
    r.n_rows += n;
    r.n_counted += sk[0];
    *acc = r;
  }
}

int vocab_eval(const float* logits, const int64_t* labels, int Nm, int V, int ldv, float* row_nll, int32_t* row_pred, hipStream_t st) {
  ETP_REQUIRE(logits && labels && row_nll && row_pred, "null pointer");
  ETP_REQUIRE(Nm >= 1 && V >= 1 && ldv >= V, "Nm >= 1, V >= 1 and ldv >= V required");
  ETP_LAUNCH(vocab_eval_kernel, dim3(Nm), dim3(256), 0, st, logits, labels, row_nll, row_pred, V, ldv);
  ETP_CHECK_LAUNCH("vocab_eval");
  return ETP_OK;
}

int sap_eval(const float* logits, const int64_t* labels, int B, int G, long ignore_index, float* row_nll, int32_t* row_pred,
             hipStream_t st) {
  ETP_REQUIRE(logits && labels && row_nll && row_pred, "null pointer");
  ETP_REQUIRE(B >= 1 && G >= 1, "B >= 1 and G >= 1 required");
  ETP_LAUNCH(sap_eval_kernel, dim3((B + 3) / 4), dim3(256), 0, st, logits, labels, row_nll, row_pred, B, G, ignore_index);
  ETP_CHECK_LAUNCH("sap_eval");
  return ETP_OK;
}

int eval_accum(const float* row_nll, const int32_t* row_pred, const int64_t* labels, int n, long ignore_index, etp_eval_record* acc,
               hipStream_t st) {
  ETP_REQUIRE(row_nll && row_pred && labels && acc, "null pointer");
  ETP_REQUIRE(n >= 1, "n >= 1 required");
  ETP_REQUIRE((uintptr_t)acc % 8 == 0, "the record must be 8-byte aligned");
  ETP_LAUNCH(eval_accum_kernel, dim3(1), dim3(256), 0, st, row_nll, row_pred, labels, n, ignore_index, acc);
  ETP_CHECK_LAUNCH("eval_accum");
  return ETP_OK;
}

}  // namespace etp
