// Explicit hipGraph construction of a recorded planner step (see launch.h).
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace etp {

namespace {
struct Recorder {
  hipGraph_t graph = nullptr;
  std::unordered_map<hipStream_t, hipGraphNode_t> last;                   // last node of each logical stream
  std::unordered_map<hipStream_t, std::vector<hipGraphNode_t>> pending;   // extra dependencies of its NEXT node
  std::unordered_map<hipEvent_t, hipGraphNode_t> events;                  // node an event stands for (absent: nothing)
  size_t n_kernels = 0, n_edges = 0;
  // introspection (etp_graph_info / _trace / _edges / _linearize): bookkeeping only, nothing of it reaches the graph
  GraphInfo* info = nullptr;
  std::unordered_map<hipStream_t, int> stream_ix;                         // logical streams, counted by first appearance
  std::unordered_map<hipEvent_t, int> event_ix;                           // events, counted by first appearance
};
Recorder* g_rec = nullptr;

int stream_index(Recorder& r, hipStream_t s) {
  auto it = r.stream_ix.find(s);
  if (it != r.stream_ix.end()) return it->second;
  const int i = (int)r.stream_ix.size();
  r.stream_ix.emplace(s, i);
  return i;
}
int event_index(Recorder& r, hipEvent_t e) {
  auto it = r.event_ix.find(e);
  if (it != r.event_ix.end()) return it->second;
  const int i = (int)r.event_ix.size();
  r.event_ix.emplace(e, i);
  return i;
}
void trace_row(Recorder& r, int kind, hipStream_t s, int event, int node) {
  const int32_t row[4] = {kind, stream_index(r, s), event, node};
  r.info->trace.insert(r.info->trace.end(), row, row + 4);
}
// a node the recorder just added on stream s: creation index, kind (the trace's), kernel function or null
void note_node(Recorder& r, int kind, hipStream_t s, hipGraphNode_t node, const void* fn) {
  GraphInfo& g = *r.info;
  g.nodes.push_back(node);
  g.kinds.push_back(kind);
  g.fns.push_back(fn);
  trace_row(r, kind, s, -1, (int)g.nodes.size() - 1);
}
thread_local hipError_t g_launch_err = hipSuccess;

// dependencies of the next node on stream s (consumes the pending list)
std::vector<hipGraphNode_t> take_deps(Recorder& r, hipStream_t s) {
  std::vector<hipGraphNode_t> d;
  auto it = r.last.find(s);
  if (it != r.last.end()) d.push_back(it->second);
  auto pt = r.pending.find(s);
  if (pt != r.pending.end()) {
    for (hipGraphNode_t n : pt->second) {
      bool dup = false;
      for (hipGraphNode_t m : d) dup = dup || (m == n);
      if (!dup) d.push_back(n);
    }
    pt->second.clear();
  }
  r.n_edges += d.size();
  return d;
}
}  // namespace

bool rec_active() { return g_rec != nullptr; }
void set_launch_error(hipError_t e) { g_launch_err = e; }
hipError_t launch_status() {
  hipError_t e = g_launch_err;
  g_launch_err = hipSuccess;
  if (e != hipSuccess) return e;
  return rec_active() ? hipSuccess : hipGetLastError();
}

int rec_kernel(const void* fn, dim3 grid, dim3 block, unsigned smem, hipStream_t st, void** args) {
  Recorder& r = *g_rec;
  std::vector<hipGraphNode_t> deps = take_deps(r, st);
  hipKernelNodeParams p;
  memset(&p, 0, sizeof(p));
  p.func = const_cast<void*>(fn);
  p.gridDim = grid; p.blockDim = block; p.sharedMemBytes = smem; p.kernelParams = args; p.extra = nullptr;
  hipGraphNode_t node;
  ETP_CHECK_HIP(hipGraphAddKernelNode(&node, r.graph, deps.empty() ? nullptr : deps.data(), deps.size(), &p));
  r.last[st] = node;
  ++r.n_kernels;
  note_node(r, 0, st, node, fn);
  return ETP_OK;
}

hipError_t event_record(hipEvent_t e, hipStream_t s) {
  if (!rec_active()) return hipEventRecord(e, s);
  Recorder& r = *g_rec;
  auto pt = r.pending.find(s);
  if (pt != r.pending.end() && !pt->second.empty()) {
    // the stream has waited for other streams since its last node: the event must stand for those too -> join node
    std::vector<hipGraphNode_t> deps = take_deps(r, s);
    hipGraphNode_t node;
    const hipError_t rc = hipGraphAddEmptyNode(&node, r.graph, deps.data(), deps.size());
    if (rc != hipSuccess) return rc;
    r.last[s] = node;
    note_node(r, 2, s, node, nullptr);
  }
  trace_row(r, 3, s, event_index(r, e), -1);
  auto it = r.last.find(s);
  if (it != r.last.end()) r.events[e] = it->second;
  else r.events.erase(e);                                   // nothing recorded on s yet: the event is already complete
  return hipSuccess;
}

hipError_t stream_wait_event(hipStream_t s, hipEvent_t e) {
  if (!rec_active()) return hipStreamWaitEvent(s, e, 0);
  Recorder& r = *g_rec;
  trace_row(r, 4, s, event_index(r, e), -1);
  auto it = r.events.find(e);
  if (it != r.events.end()) r.pending[s].push_back(it->second);
  return hipSuccess;
}

hipError_t memset_async(void* p, int value, size_t bytes, hipStream_t s) {
  if (!rec_active()) return hipMemsetAsync(p, value, bytes, s);
  Recorder& r = *g_rec;
  std::vector<hipGraphNode_t> deps = take_deps(r, s);
  hipMemsetParams m;
  memset(&m, 0, sizeof(m));
  m.dst = p; m.value = (unsigned)value & 0xffu; m.elementSize = 1; m.width = bytes; m.height = 1; m.pitch = bytes;
  hipGraphNode_t node;
  const hipError_t rc = hipGraphAddMemsetNode(&node, r.graph, deps.empty() ? nullptr : deps.data(), deps.size(), &m);
  if (rc == hipSuccess) {
    r.last[s] = node;
    note_node(r, 1, s, node, nullptr);
  }
  return rc;
}

int rec_begin() {
  ETP_REQUIRE(g_rec == nullptr, "a recording is already active");
  Recorder* r = new Recorder();
  const hipError_t e = hipGraphCreate(&r->graph, 0);
  if (e != hipSuccess) { delete r; return check_hip(e, "hipGraphCreate"); }
  r->info = new GraphInfo();
  g_rec = r;
  return ETP_OK;
}

int rec_end(hipGraph_t* graph, hipGraphExec_t* exec, long* n_kernels, long* n_edges, GraphInfo** info) {
  ETP_REQUIRE(g_rec != nullptr, "no active recording");
  Recorder* r = g_rec;
  g_rec = nullptr;
  *graph = r->graph;
  if (n_kernels) *n_kernels = (long)r->n_kernels;
  if (n_edges) *n_edges = (long)r->n_edges;
  r->info->n_streams = (int)r->stream_ix.size();
  if (info) *info = r->info;
  else delete r->info;
  delete r;
  ETP_CHECK_HIP(hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0));
  return ETP_OK;
}

// ---- introspection of a recorded graph (host only) -------------------------------------------------------------------
// edges as the RUNTIME holds them (hipGraphGetEdges), mapped to creation indices: what replays, not what the recorder meant
int graph_edges(hipGraph_t graph, const GraphInfo& info, std::vector<int32_t>* from, std::vector<int32_t>* to) {
  size_t nn = 0, ne = 0;
  ETP_CHECK_HIP(hipGraphGetNodes(graph, nullptr, &nn));
  ETP_REQUIRE(nn == info.nodes.size(), "the runtime's node count differs from the recorder's");
  ETP_CHECK_HIP(hipGraphGetEdges(graph, nullptr, nullptr, &ne));
  std::vector<hipGraphNode_t> f(ne), t(ne);
  if (ne) ETP_CHECK_HIP(hipGraphGetEdges(graph, f.data(), t.data(), &ne));
  std::unordered_map<hipGraphNode_t, int32_t> ix;
  for (size_t i = 0; i < info.nodes.size(); ++i) ix.emplace(info.nodes[i], (int32_t)i);
  from->clear();
  to->clear();
  for (size_t i = 0; i < ne; ++i) {
    auto a = ix.find(f[i]), b = ix.find(t[i]);
    ETP_REQUIRE(a != ix.end() && b != ix.end(), "the runtime reports an edge of a node the recorder did not create");
    from->push_back(a->second);
    to->push_back(b->second);
  }
  return ETP_OK;
}

int graph_node_name(const GraphInfo& info, long i, char* buf, int cap) {
  ETP_REQUIRE(buf && cap > 0 && i >= 0 && i < (long)info.nodes.size(), "bad arguments");
  const char* name = info.kinds[(size_t)i] == 1 ? "memset" : "join";
  if (info.kinds[(size_t)i] == 0) {
    name = hipKernelNameRefByPtr(info.fns[(size_t)i], nullptr);
    if (!name) name = "?";
  }
  strncpy(buf, name, (size_t)cap - 1);
  buf[cap - 1] = 0;
  return ETP_OK;
}

// The same nodes with the same parameters (re-added from the runtime's own copy of them) as one chain order[0] -> order[1] -> ...
int graph_linearize(hipGraph_t graph, const GraphInfo& info, const int32_t* order, long n, hipGraph_t* out_graph,
                    hipGraphExec_t* out_exec, GraphInfo** out_info) {
  const size_t N = info.nodes.size();
  ETP_REQUIRE(order && n == (long)N && N > 0, "order must be a permutation of all nodes");
  std::vector<char> seen(N, 0);
  for (size_t i = 0; i < N; ++i) {
    ETP_REQUIRE(order[i] >= 0 && (size_t)order[i] < N && !seen[(size_t)order[i]], "order must be a permutation of all nodes");
    seen[(size_t)order[i]] = 1;
  }
  (void)graph;
  hipGraph_t g = nullptr;
  ETP_CHECK_HIP(hipGraphCreate(&g, 0));
  GraphInfo* gi = new GraphInfo();
  gi->nodes.resize(N);
  gi->kinds = info.kinds;
  gi->fns = info.fns;
  gi->n_streams = 1;
  hipGraphNode_t prev = nullptr;
  hipError_t e = hipSuccess;
  for (size_t i = 0; i < N && e == hipSuccess; ++i) {
    const size_t k = (size_t)order[i];
    hipGraphNode_t node = nullptr;
    const hipGraphNode_t* dep = prev ? &prev : nullptr;
    const size_t nd = prev ? 1 : 0;
    if (info.kinds[k] == 0) {
      hipKernelNodeParams p;
      e = hipGraphKernelNodeGetParams(info.nodes[k], &p);
      if (e == hipSuccess) e = hipGraphAddKernelNode(&node, g, dep, nd, &p);
    } else if (info.kinds[k] == 1) {
      hipMemsetParams m;
      e = hipGraphMemsetNodeGetParams(info.nodes[k], &m);
      if (e == hipSuccess) e = hipGraphAddMemsetNode(&node, g, dep, nd, &m);
    } else {
      e = hipGraphAddEmptyNode(&node, g, dep, nd);
    }
    gi->nodes[k] = node;                       // creation indices stay those of the recorded graph
    const int32_t row[4] = {info.kinds[k], 0, -1, (int32_t)k};
    gi->trace.insert(gi->trace.end(), row, row + 4);
    prev = node;
  }
  if (e == hipSuccess) e = hipGraphInstantiate(out_exec, g, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(g);
    delete gi;
    return check_hip(e, "etp_graph_linearize");
  }
  *out_graph = g;
  *out_info = gi;
  return ETP_OK;
}

// ---- per-launch timing of every kernel ------------------------------------------------------------------------------
namespace {
struct KRec { const void* fn; unsigned grid, block; hipStream_t st; hipEvent_t a, b; };
bool g_ktime = false;
std::vector<KRec> g_krecs;
}  // namespace
bool ktime_active() { return g_ktime && !rec_active(); }
void ktime_begin(const void* fn, dim3 grid, dim3 block, hipStream_t st) {
  KRec r{fn, grid.x * grid.y * grid.z, block.x * block.y * block.z, st, nullptr, nullptr};
  (void)hipEventCreate(&r.a);
  (void)hipEventCreate(&r.b);
  (void)hipEventRecord(r.a, st);
  g_krecs.push_back(r);
}
void ktime_end(hipStream_t st) {
  if (!g_krecs.empty()) (void)hipEventRecord(g_krecs.back().b, st);
}
void ktime_enable(bool on) { g_ktime = on; }
void ktime_reset() {
  for (auto& r : g_krecs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  g_krecs.clear();
}
// one text line per launch, in launch order: "<us>\t<grid>\t<block>\t<stream>\t<kernel name>"
long ktime_report(char* buf, long cap) {
  long n = 0;
  for (auto& r : g_krecs) {
    if (hipEventSynchronize(r.b) != hipSuccess) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
    const char* name = hipKernelNameRefByPtr(r.fn, r.st);
    char line[512];
    const int len = snprintf(line, sizeof(line), "%.2f\t%u\t%u\t%p\t%s\n", ms * 1e3, r.grid, r.block, (void*)r.st,
                             name ? name : "?");
    if (n + len >= cap) break;
    memcpy(buf + n, line, len);
    n += len;
  }
  if (n < cap) buf[n] = 0;
  return n;
}

void rec_abort() {
  if (!g_rec) return;
  (void)hipGraphDestroy(g_rec->graph);
  delete g_rec->info;
  delete g_rec;
  g_rec = nullptr;
}

}  // namespace etp
