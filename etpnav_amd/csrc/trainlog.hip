// What the pre-training loop tells the user while it trains, kept on the device: running losses, the gradient norm, throughput
// counters and a per-tensor fingerprint of a float arena.
//
// Replaces, per micro-step, task2loss[name](loss.item()) with RunningMeter.__call__ (pretrain_src/pretrain_src/train_r2r.py:259,
// utils/logger.py:68-94) and the three counters n_examples / n_in_units / n_loss_units (:233-234, :246); per optimizer step the
// pre-clip grad_norm of clip_grad_norm_ (:282-290); and, on request, the per-parameter norm loop the authors left commented out
// (:286-289) as the (sum, abs-max, L2) triple of oracle/make_golden.py:69-73 per tensor, in double -- without a host synchronisation
// per step and without a copy of any gradient to the host.  The host reads the records in one copy every log_steps optimizer steps.
//
// Plain vector stores only: no atomics of any kind, no scratch, LDS only for the four waves' combine.  Every order of summation is
// fixed by thread, lane, wave, chunk and segment index, so a second run on the same inputs gives the same bits.  The file is compiled
// with -ffp-contract=off: the meter promises Python's double arithmetic, one rounded operation at a time.
#include "kernels.h"

namespace etp {

namespace {
constexpr int REPORT_CHUNK = ETP_TENSOR_REPORT_CHUNK;      // elements per stage-1 workgroup, a multiple of 4

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one element into a thread's fingerprint: a non-finite value is counted and left out of the three others
struct Finger {
  double sum, sumsq;
  float amax;
  int nf;
};
__device__ __forceinline__ void take(Finger& f, float x) {
  if (__builtin_isfinite(x)) {
    const double d = (double)x;
    f.sum += d;
    f.sumsq += d * d;          // the square of a float is exact in double: only the additions round
    f.amax = fmaxf(f.amax, fabsf(x));
  } else {
    f.nf += 1;
  }
}
}  // namespace

// (a) One workgroup of 256 threads, one launch per micro-step.  The mask bytes are counted thread-strided (integers: any order gives
// the same count); thread 0 then does RunningMeter.__call__ on the record in double.
__global__ __launch_bounds__(256) void train_meter_loss_kernel(const float* __restrict__ loss, double smooth,
                                                               const uint8_t* __restrict__ masks, long n_mask, long n_examples,
                                                               long n_loss_units, etp_train_task_record* __restrict__ rec) {
  __shared__ int red[4];
  const int t = threadIdx.x;
  int cnt = 0;
  for (long i = t; i < n_mask; i += 256) cnt += masks[i] != 0 ? 1 : 0;
  cnt = wave_sum_i32(cnt);
  if ((t & 63) == 0) red[t >> 6] = cnt;
  __syncthreads();
  if (t == 0) {
    etp_train_task_record r = *rec;
    const double value = (double)loss[0];
    // val = value if self._val is None else value*(1-self._sm) + self._val*self._sm            (logger.py:78-79)
    double val = value;
    if (r.n_values > 0) {
      const double keep = 1.0 - smooth;
      const double a = value * keep;
      const double b = r.run_loss * smooth;
      val = a + b;
    }
    if (val != val) {          // math.isnan(val): the value is dropped (logger.py:80); +-inf is taken
      r.n_skipped += 1;
    } else {
      r.run_loss = val;
      r.n_values += 1;
    }
    r.last_loss = value;
    r.n_examples += n_examples;
    r.n_in_units += (long)(red[0] + red[1] + red[2] + red[3]);
    r.n_loss_units += n_loss_units;
    *rec = r;
  }
}

// (b) One thread, one launch per optimizer step, behind the norm pass: grad_norm = sqrt(sumsq) as clip_grad_norm_ returns it, in
// fp32.  The double root of a float rounded once more to float is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits).
__global__ void train_meter_step_kernel(const float* __restrict__ sumsq, const int32_t* __restrict__ nonfinite,
                                        etp_train_step_record* __restrict__ rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  etp_train_step_record r = *rec;
  const float gn = (float)sqrt((double)sumsq[0]);
  const int nf = nonfinite != nullptr ? nonfinite[0] : 0;
  r.n_steps += 1;
  r.norm_last = (double)gn;
  if (__builtin_isfinite(gn) && nf == 0) {
    r.norm_max = r.norm_last > r.norm_max ? r.norm_last : r.norm_max;
    r.norm_sum += r.norm_last;
  } else {
    r.n_nonfinite_steps += 1;
    if (r.first_nonfinite_step < 0) r.first_nonfinite_step = r.n_steps;      // counted from 1
  }
  *rec = r;
}

// (c) stage 1: one workgroup of 256 threads per chunk of at most REPORT_CHUNK elements of ONE segment.  chunk_start [n_seg + 1] is the
// prefix of the segments' chunk counts; the workgroup finds its segment by binary search (uniform: scalar loads).  Thread t takes the
// 16-byte vectors t, t + 256, ... of the chunk in ascending order, four elements each in element order; threads 0 .. 2 then take the
// up to three elements behind the last whole vector.  The wave's shuffle tree and the four waves in wave order follow.  Nothing
// outside [seg_off, seg_off + seg_len) is read.
__global__ __launch_bounds__(256) void tensor_report_chunk_kernel(const float* __restrict__ arena, const int64_t* __restrict__ seg_off,
                                                                  const int64_t* __restrict__ seg_len,
                                                                  const int64_t* __restrict__ chunk_start, int n_seg,
                                                                  double* __restrict__ p_sum, double* __restrict__ p_sumsq,
                                                                  float* __restrict__ p_amax, int32_t* __restrict__ p_nf) {
  __shared__ double s_sum[4], s_sq[4];
  __shared__ float s_amax[4];
  __shared__ int s_nf[4];
  const long chunk = blockIdx.x;
  int lo = 0, hi = n_seg - 1;                    // the last segment whose first chunk is <= chunk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_start[mid] <= chunk) lo = mid; else hi = mid - 1;
  }
  const long first = (chunk - chunk_start[lo]) * REPORT_CHUNK;
  const long left = seg_len[lo] - first;
  const int n = (int)(left < REPORT_CHUNK ? left : REPORT_CHUNK);
  const float* __restrict__ x = arena + seg_off[lo] + first;      // 16-byte aligned: offset % 4 == 0, REPORT_CHUNK % 4 == 0
  const int t = threadIdx.x, n4 = n >> 2;
  Finger f = {0.0, 0.0, 0.f, 0};
  for (int i = t; i < n4; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(x + 4 * i);
    take(f, v.x);
    take(f, v.y);
    take(f, v.z);
    take(f, v.w);
  }
  if (4 * n4 + t < n) take(f, x[4 * n4 + t]);
  f.sum = wave_sum_f64(f.sum);
  f.sumsq = wave_sum_f64(f.sumsq);
  f.amax = wave_max(f.amax);
  f.nf = wave_sum_i32(f.nf);
  if ((t & 63) == 0) {
    s_sum[t >> 6] = f.sum;
    s_sq[t >> 6] = f.sumsq;
    s_amax[t >> 6] = f.amax;
    s_nf[t >> 6] = f.nf;
  }
  __syncthreads();
  if (t == 0) {
    p_sum[chunk] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    p_sumsq[chunk] = ((s_sq[0] + s_sq[1]) + s_sq[2]) + s_sq[3];
    p_amax[chunk] = fmaxf(fmaxf(s_amax[0], s_amax[1]), fmaxf(s_amax[2], s_amax[3]));
    p_nf[chunk] = s_nf[0] + s_nf[1] + s_nf[2] + s_nf[3];
  }
}

// stage 2: one wavefront per segment.  Lane l adds the segment's partials l, l + 64, ... in chunk order, the shuffle tree follows.
__global__ __launch_bounds__(64) void tensor_report_segment_kernel(const int64_t* __restrict__ chunk_start,
                                                                   const double* __restrict__ p_sum, const double* __restrict__ p_sumsq,
                                                                   const float* __restrict__ p_amax, const int32_t* __restrict__ p_nf,
                                                                   etp_tensor_record* __restrict__ out) {
  const int seg = blockIdx.x, lane = threadIdx.x;
  const long c0 = chunk_start[seg], c1 = chunk_start[seg + 1];
  double sum = 0.0, sq = 0.0;
  float amax = 0.f;
  int nf = 0;
  for (long c = c0 + lane; c < c1; c += 64) {
    sum += p_sum[c];
    sq += p_sumsq[c];
    amax = fmaxf(amax, p_amax[c]);
    nf += p_nf[c];
  }
  sum = wave_sum_f64(sum);
  sq = wave_sum_f64(sq);
  amax = wave_max(amax);
  nf = wave_sum_i32(nf);
  if (lane == 0) {
    etp_tensor_record r;
    r.sum = sum;
    r.sumsq = sq;
    r.absmax = amax;
    r.nonfinite = nf;
    r.reserved = 0;
    out[seg] = r;
  }
}

// stage 3: one wavefront.  Lane l adds the records l, l + 64, ... whose include byte is non-zero, in segment order, the shuffle tree
// follows; the pair is STORED.  A non-zero count makes the float a quiet NaN (the scan of optim.hip would hold a non-finite sum too).
__global__ __launch_bounds__(64) void tensor_report_total_kernel(const etp_tensor_record* __restrict__ recs,
                                                                 const uint8_t* __restrict__ include, int n_seg,
                                                                 float* __restrict__ sumsq_out, int32_t* __restrict__ nonfinite_out) {
  const int lane = threadIdx.x;
  double sq = 0.0;
  int nf = 0;
  for (int s = lane; s < n_seg; s += 64) {
    if (include[s] == 0) continue;
    sq += recs[s].sumsq;
    nf += recs[s].nonfinite;
  }
  sq = wave_sum_f64(sq);
  nf = wave_sum_i32(nf);
  if (lane == 0) {
    if (sumsq_out != nullptr) sumsq_out[0] = nf != 0 ? __builtin_nanf("") : (float)sq;
    if (nonfinite_out != nullptr) nonfinite_out[0] = nf;
  }
}

int train_meter_loss(const float* loss, double smooth, const uint8_t* txt_masks, long n_mask_bytes, long n_examples, long n_loss_units,
                     etp_train_task_record* rec, hipStream_t st) {
  ETP_REQUIRE(loss && txt_masks && rec, "null pointer");
  ETP_REQUIRE((uintptr_t)loss % 4 == 0 && (uintptr_t)rec % 8 == 0, "loss must be 4-byte, the record 8-byte aligned");
  ETP_REQUIRE(smooth >= 0.0 && smooth < 1.0, "smooth must lie in [0, 1)");
  ETP_REQUIRE(n_mask_bytes >= 0 && n_examples >= 0 && n_loss_units >= 0, "negative count");
  ETP_LAUNCH(train_meter_loss_kernel, dim3(1), dim3(256), 0, st, loss, smooth, txt_masks, n_mask_bytes, n_examples, n_loss_units, rec);
  ETP_CHECK_LAUNCH("train_meter_loss");
  return ETP_OK;
}

int train_meter_step(const float* sumsq, const int32_t* nonfinite, etp_train_step_record* rec, hipStream_t st) {
  ETP_REQUIRE(sumsq && rec, "null pointer");
  ETP_REQUIRE((uintptr_t)sumsq % 4 == 0 && (uintptr_t)nonfinite % 4 == 0 && (uintptr_t)rec % 8 == 0,
              "sumsq / nonfinite must be 4-byte, the record 8-byte aligned");
  ETP_LAUNCH(train_meter_step_kernel, dim3(1), dim3(64), 0, st, sumsq, nonfinite, rec);
  ETP_CHECK_LAUNCH("train_meter_step");
  return ETP_OK;
}

}  // namespace etp

// ---- the report's plan: host tables, validated once; device copies and the partials made at the first launch -------------------------
struct etp_tensor_report_plan {
  std::vector<int64_t> off, len, chunk_start;      // chunk_start [n_seg + 1]
  std::vector<uint8_t> include;
  int64_t arena_len = 0;
  // device side (one allocation): [seg_off | seg_len | chunk_start | p_sum | p_sumsq | p_amax | p_nf | include]
  void* dev = nullptr;
  int64_t *d_off = nullptr, *d_len = nullptr, *d_chunk_start = nullptr;
  double *d_sum = nullptr, *d_sumsq = nullptr;
  float* d_amax = nullptr;
  int32_t* d_nf = nullptr;
  uint8_t* d_include = nullptr;
};

namespace etp {

int tensor_report_create(const int64_t* seg_off, const int64_t* seg_len, const uint8_t* include, int n_seg, long arena_len,
                         etp_tensor_report_plan** out) {
  ETP_REQUIRE(seg_off && seg_len && out, "null pointer");
  ETP_REQUIRE(n_seg >= 1, "n_seg >= 1 required");
  ETP_REQUIRE(arena_len >= 1, "arena_len >= 1 required");
  int64_t end = 0, chunks = 0;
  for (int s = 0; s < n_seg; ++s) {
    const int64_t o = seg_off[s], l = seg_len[s];
    ETP_REQUIRE(o >= 0 && o % 4 == 0, "segment " + std::to_string(s) + ": the offset must be a non-negative multiple of 4");
    ETP_REQUIRE(l >= 1, "segment " + std::to_string(s) + ": length >= 1 required");
    ETP_REQUIRE(o >= end, "segment " + std::to_string(s) + ": segments must ascend and must not overlap");
    ETP_REQUIRE(l <= arena_len && o <= arena_len - l, "segment " + std::to_string(s) + ": ends behind the arena");
    end = o + l;
    chunks += (l + REPORT_CHUNK - 1) / REPORT_CHUNK;
  }
  ETP_REQUIRE(chunks <= 0x7fffffffL, "more chunks than one grid holds");
  auto* p = new etp_tensor_report_plan;
  p->off.assign(seg_off, seg_off + n_seg);
  p->len.assign(seg_len, seg_len + n_seg);
  p->include.assign(n_seg, 1);
  if (include != nullptr) p->include.assign(include, include + n_seg);
  p->chunk_start.resize(n_seg + 1);
  p->chunk_start[0] = 0;
  for (int s = 0; s < n_seg; ++s) p->chunk_start[s + 1] = p->chunk_start[s] + (seg_len[s] + REPORT_CHUNK - 1) / REPORT_CHUNK;
  p->arena_len = arena_len;
  *out = p;
  return ETP_OK;
}

long tensor_report_chunks(const etp_tensor_report_plan* p) { return p == nullptr ? -1 : (long)p->chunk_start.back(); }

static int tensor_report_upload(etp_tensor_report_plan* p) {
  const size_t n_seg = p->off.size(), nc = (size_t)p->chunk_start.back();
  const size_t b_tab = n_seg * 8, b_cs = (n_seg + 1) * 8;
  const size_t bytes = 2 * b_tab + b_cs + nc * (8 + 8 + 4 + 4) + n_seg;
  void* dev = nullptr;
  ETP_CHECK_HIP(hipMalloc(&dev, bytes));
  char* c = (char*)dev;
  int64_t* d_off = (int64_t*)c;                c += b_tab;
  int64_t* d_len = (int64_t*)c;                c += b_tab;
  int64_t* d_cs = (int64_t*)c;                 c += b_cs;
  double* d_sum = (double*)c;                  c += nc * 8;
  double* d_sumsq = (double*)c;                c += nc * 8;
  float* d_amax = (float*)c;                   c += nc * 4;
  int32_t* d_nf = (int32_t*)c;                 c += nc * 4;
  uint8_t* d_inc = (uint8_t*)c;
  hipError_t e = hipMemcpy(d_off, p->off.data(), b_tab, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_len, p->len.data(), b_tab, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_cs, p->chunk_start.data(), b_cs, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_inc, p->include.data(), n_seg, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    return check_hip(e, "tensor_report: table upload");
  }
  p->dev = dev;
  p->d_off = d_off; p->d_len = d_len; p->d_chunk_start = d_cs;
  p->d_sum = d_sum; p->d_sumsq = d_sumsq; p->d_amax = d_amax; p->d_nf = d_nf; p->d_include = d_inc;
  return ETP_OK;
}

int tensor_report(etp_tensor_report_plan* p, const float* arena, etp_tensor_record* records_out, float* sumsq_out,
                  int32_t* nonfinite_out, hipStream_t st) {
  ETP_REQUIRE(p && arena && records_out, "null pointer");
  ETP_REQUIRE((uintptr_t)arena % 16 == 0, "the arena must be 16-byte aligned");
  ETP_REQUIRE((uintptr_t)records_out % 8 == 0, "the records must be 8-byte aligned");
  ETP_REQUIRE((uintptr_t)sumsq_out % 4 == 0 && (uintptr_t)nonfinite_out % 4 == 0, "sumsq_out / nonfinite_out must be 4-byte aligned");
  if (p->dev == nullptr) ETP_TRY(tensor_report_upload(p));
  const int n_seg = (int)p->off.size();
  ETP_LAUNCH(tensor_report_chunk_kernel, dim3((unsigned)p->chunk_start.back()), dim3(256), 0, st, arena, (const int64_t*)p->d_off,
             (const int64_t*)p->d_len, (const int64_t*)p->d_chunk_start, n_seg, p->d_sum, p->d_sumsq, p->d_amax, p->d_nf);
  ETP_LAUNCH(tensor_report_segment_kernel, dim3(n_seg), dim3(64), 0, st, (const int64_t*)p->d_chunk_start, (const double*)p->d_sum,
             (const double*)p->d_sumsq, (const float*)p->d_amax, (const int32_t*)p->d_nf, records_out);
  if (sumsq_out != nullptr || nonfinite_out != nullptr)
    ETP_LAUNCH(tensor_report_total_kernel, dim3(1), dim3(64), 0, st, (const etp_tensor_record*)records_out,
               (const uint8_t*)p->d_include, n_seg, sumsq_out, nonfinite_out);
  ETP_CHECK_LAUNCH("tensor_report");
  return ETP_OK;
}

int tensor_report_destroy(etp_tensor_report_plan* p) {
  if (p == nullptr) return ETP_OK;
  if (p->dev != nullptr) (void)hipFree(p->dev);
  delete p;
  return ETP_OK;
}

}  // namespace etp
