// The loss of a fine-tuning rollout, its scale and its log, kept on the device.
//
// Replaces, per rollout step, loss += F.cross_entropy(nav_logits, teacher_actions, reduction='sum', ignore_index=-100) and
// total_actions += len(prev_vp) (vlnce_baselines/ss_trainer_ETP.py:892, :820); per rollout, loss = ml_weight * loss / total_actions and
// self.logs['IL_loss'].append(loss.item()) (:1055-1057); and the gradient that autograd sends back into every step's nav_logits.  The
// divisor total_actions is known only when the last environment has stopped, so it cannot be a launch argument of the steps' own
// launches (etp_sap_ce takes its scale from the host): it stays in a 64-byte device record that the per-step launches advance and
// that the backward launches read.  The host never waits for a loss value.
//
// Three kernels.  rollout_ce_fwd_kernel: one workgroup, one wavefront per row, the rows' nll added to the record in row order in
// double by thread 0.  rollout_loss_kernel: one thread, the division and the log.  rollout_ce_bwd_kernel: one wavefront per row, four per
// workgroup.  Plain vector stores only: no atomics, no scratch, LDS only for the rows' hand-over to thread 0.  Every order of
// summation is fixed by lane and row index, so a second run on the same inputs gives the same bits.  The file is compiled with
// -ffp-contract=off: the scale promises one rounded double operation per step.
//
// Semantics: max / sum / lse in sap_eval_kernel's order (eval_tail.hip); an ignored row contributes 0 and gets a zero gradient; a label
// that is neither ignore_index nor a column gives a NaN nll and a NaN gradient row and is never used as an index; a label on a -inf
// logit gives +inf.  n_nonfinite counts the kept rows whose nll is not finite.  PRECONDITION: no NaN in the logits.
#include "kernels.h"

namespace etp {

namespace {
constexpr int FWD_ROWS = 256;      // rows handed to thread 0 per round

// lse of one row by one wavefront: the lanes' strided maxima and sums, then the shuffle trees (sap_ce_kernel / sap_eval_kernel)
__device__ __forceinline__ float row_lse(const float* __restrict__ s, int G, int lane) {
  float mx = -INFINITY;
  for (int k = lane; k < G; k += 64) mx = fmaxf(mx, s[k]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int k = lane; k < G; k += 64) sum += expf(s[k] - mx);
  sum = wave_sum(sum);
  return mx + logf(sum);
}
}  // namespace

// One workgroup of 256 threads.  Rounds of at most 256 rows: wave w takes the round's rows w, w + 4, ... and leaves each nll in LDS;
// thread 0 then adds the round's kept rows in row order in double.  Rounds follow each other in row order, so the whole sum runs in
// row order.
__global__ __launch_bounds__(256) void rollout_ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int B,
                                                             int G, long ignore_index, etp_rollout_record* __restrict__ rec,
                                                             float* __restrict__ row_nll) {
  __shared__ float s_nll[FWD_ROWS];
  __shared__ int s_keep[FWD_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double loss = 0.0;
  long counted = 0, nonfinite = 0;
  for (long base = 0; base < B; base += FWD_ROWS) {
    const int cnt = (int)((long)B - base < FWD_ROWS ? (long)B - base : FWD_ROWS);
    for (int i = wave; i < cnt; i += 4) {
      const long row = base + i;
      const float* s = logits + row * G;
      const float lse = row_lse(s, G, lane);
      if (lane == 0) {
        const long y = labels[row];
        float nll = __builtin_nanf("");
        if (y == ignore_index) nll = 0.f;
        else if (y >= 0 && y < G) nll = lse - s[y];
        s_nll[i] = nll;
        s_keep[i] = y != ignore_index ? 1 : 0;
        if (row_nll != nullptr) row_nll[row] = nll;
      }
    }
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < cnt; ++i) {
        if (s_keep[i] == 0) continue;
        const float v = s_nll[i];
        loss += (double)v;
        counted += 1;
        nonfinite += __builtin_isfinite(v) ? 0 : 1;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    etp_rollout_record r = *rec;
    r.loss_sum += loss;
    r.n_actions += B;
    r.n_counted += counted;
    r.n_steps += 1;
    r.n_nonfinite += nonfinite;
    *rec = r;
  }
}

// One thread: ml_weight * loss / total_actions in double (one product, one quotient), rounded once to fp32; the same fp32 value, as a
// double, onto the log.
__global__ void rollout_loss_kernel(const etp_rollout_record* __restrict__ rec, double ml_weight, float* __restrict__ loss,
                                    etp_rollout_log* __restrict__ log) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double sum = rec->loss_sum;
  const long n = rec->n_actions;
  float v = 0.f;
  if (n != 0) {
    const double w = ml_weight * sum;
    v = (float)(w / (double)n);
  }
  *loss = v;
  if (log != nullptr) {
    etp_rollout_log l = *log;
    l.sum += (double)v;
    l.n += 1;
    l.n_nonfinite += __builtin_isfinite(v) ? 0 : 1;
    *log = l;
  }
}

// One wavefront per row, four per workgroup.  s = (float)(ml_weight / (double)n_actions) * upstream; dlogits = s * (softmax - onehot)
// in sap_ce_kernel's form: expf(-inf) is 0 and s * 0 is 0, so a -inf column that no label points at gets exactly 0.
__global__ __launch_bounds__(256) void rollout_ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int B,
                                                             int G, long ignore_index, const etp_rollout_record* __restrict__ rec,
                                                             double ml_weight, const float* __restrict__ upstream,
                                                             float* __restrict__ dlogits) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const long n = rec->n_actions;
  float scale = 0.f;
  if (n != 0) scale = (float)(ml_weight / (double)n);
  if (upstream != nullptr) scale = scale * upstream[0];
  const float* s = logits + row * G;
  float* d = dlogits + row * G;
  const long y = labels[row];
  if (y == ignore_index) {
    for (int k = lane; k < G; k += 64) d[k] = 0.f;
    return;
  }
  if (y < 0 || y >= G) {
    for (int k = lane; k < G; k += 64) d[k] = __builtin_nanf("");
    return;
  }
  const float lse = row_lse(s, G, lane);
  for (int k = lane; k < G; k += 64) d[k] = scale * (expf(s[k] - lse) - (k == y ? 1.f : 0.f));
}

namespace {
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}
}  // namespace

int rollout_ce_fwd(const float* logits, const int64_t* labels, int B, int G, long ignore_index, etp_rollout_record* rec, float* row_nll,
                   hipStream_t st) {
  ETP_REQUIRE(logits && labels && rec, "null pointer");
  ETP_REQUIRE(B >= 1 && G >= 1, "B >= 1 and G >= 1 required");
  ETP_REQUIRE((uintptr_t)logits % 4 == 0 && (uintptr_t)row_nll % 4 == 0, "logits / row_nll must be 4-byte aligned");
  ETP_REQUIRE((uintptr_t)labels % 8 == 0 && (uintptr_t)rec % 8 == 0, "labels and the record must be 8-byte aligned");
  ETP_REQUIRE(row_nll == nullptr || !overlap(rec, sizeof(etp_rollout_record), row_nll, (size_t)B * 4), "row_nll overlaps the record");
  ETP_LAUNCH(rollout_ce_fwd_kernel, dim3(1), dim3(256), 0, st, logits, labels, B, G, ignore_index, rec, row_nll);
  ETP_CHECK_LAUNCH("rollout_ce_fwd");
  return ETP_OK;
}

int rollout_loss(const etp_rollout_record* rec, double ml_weight, float* loss, etp_rollout_log* log, hipStream_t st) {
  ETP_REQUIRE(rec && loss, "null pointer");
  ETP_REQUIRE((uintptr_t)rec % 8 == 0 && (uintptr_t)log % 8 == 0, "the record and the log must be 8-byte aligned");
  ETP_REQUIRE((uintptr_t)loss % 4 == 0, "loss must be 4-byte aligned");
  ETP_REQUIRE(!overlap(rec, sizeof(etp_rollout_record), loss, 4), "loss lies inside the record");
  ETP_REQUIRE(log == nullptr || (!overlap(log, sizeof(etp_rollout_log), loss, 4) &&
                                 !overlap(log, sizeof(etp_rollout_log), rec, sizeof(etp_rollout_record))),
              "the log overlaps loss or the record");
  ETP_LAUNCH(rollout_loss_kernel, dim3(1), dim3(64), 0, st, rec, ml_weight, loss, log);
  ETP_CHECK_LAUNCH("rollout_loss");
  return ETP_OK;
}

int rollout_ce_bwd(const float* logits, const int64_t* labels, int B, int G, long ignore_index, const etp_rollout_record* rec,
                   double ml_weight, const float* upstream, float* dlogits, hipStream_t st) {
  ETP_REQUIRE(logits && labels && rec && dlogits, "null pointer");
  ETP_REQUIRE(B >= 1 && G >= 1, "B >= 1 and G >= 1 required");
  ETP_REQUIRE((uintptr_t)logits % 4 == 0 && (uintptr_t)dlogits % 4 == 0 && (uintptr_t)upstream % 4 == 0,
              "logits / dlogits / upstream must be 4-byte aligned");
  ETP_REQUIRE((uintptr_t)labels % 8 == 0 && (uintptr_t)rec % 8 == 0, "labels and the record must be 8-byte aligned");
  ETP_REQUIRE(!overlap(rec, sizeof(etp_rollout_record), dlogits, (size_t)B * G * 4), "dlogits overlaps the record");
  ETP_LAUNCH(rollout_ce_bwd_kernel, dim3((unsigned)(((long)B + 3) / 4)), dim3(256), 0, st, logits, labels, B, G, ignore_index, rec,
             ml_weight, upstream, dlogits);
  ETP_CHECK_LAUNCH("rollout_ce_bwd");
  return ETP_OK;
}

}  // namespace etp
