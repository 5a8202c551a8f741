// Host-side core shared by the planner and the three frozen engines (waypoint, CLIP, depth): the parameter table over one flat
// fp32 arena, the engine base with its accessors, the bump allocator of every scratch plan, the GemmArgs preamble and the bind
// checks.  No kernel code.  An engine keeps only what is its own: layer structs, name list, scratch plan, forward chain.
#pragma once
#include <assert.h>
#include <string.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "common.h"

namespace etp {

struct ParamEntry { std::string name; int ndim; long shape[4]; int region; long offset; long numel; };

// Parameters in state-dict order; offsets in region order.  Region 0 holds the GEMM matrices: [0, n_matrix) is what the operand copy
// (bf16 shadow / packed weights) mirrors.  Every slot starts on a multiple of 64 elements: the fused AdamW and the data-parallel
// slice plan rely on it, and adjacent matrices whose sizes are multiples of 64 (query / key / value) form one operand.
struct ParamTable {
  std::vector<ParamEntry> e;
  long total = 0, n_matrix = 0;
  int size() const { return (int)e.size(); }
  int add(const std::string& name, int region, std::initializer_list<long> shape) {
    ParamEntry p;
    p.name = name; p.ndim = (int)shape.size(); p.region = region; p.numel = 1; p.offset = -1;
    int k = 0;
    for (long s : shape) { p.shape[k++] = s; p.numel *= s; }
    for (; k < 4; ++k) p.shape[k] = 0;
    e.push_back(p);
    return size() - 1;
  }
  void layout(int n_regions) {
    long off = 0;
    for (int region = 0; region < n_regions; ++region) {
      for (auto& p : e)
        if (p.region == region) { p.offset = off; off += round_up(p.numel, 64); }
      if (region == 0) n_matrix = off;
    }
    total = off;
  }
  // entry i -> one of the C ABI's info structs (etp_param_info: rank 2; etp_clip_tensor_info / etp_depth_tensor_info: rank 4)
  template <class Info>
  void fill(int i, Info* out) const {
    constexpr int rank = (int)(sizeof(out->shape) / sizeof(out->shape[0]));
    const ParamEntry& q = e[i];
    assert(q.ndim <= rank);
    memset(out, 0, sizeof(*out));
    strncpy(out->name, q.name.c_str(), sizeof(out->name) - 1);
    out->ndim = q.ndim;
    for (int k = 0; k < rank; ++k) out->shape[k] = q.shape[k];
    out->offset = q.offset;
  }
};

// What every engine holds: compute dtype, table, the bound fp32 arena and the bound operand copy of its matrix region.  The
// accessors stay inline vector indexing: they sit on the planner's per-launch path.
struct ArenaEngine {
  int dtype = ETP_F32;
  ParamTable table;
  float* P = nullptr;
  void* Wc = nullptr;             // bf16 shadow (planner, waypoint, CLIP: bf16 mode only) or packed weights (depth: both dtypes)
  bool copy_in_f32 = false;       // depth: GEMM operands come from the copy in fp32 mode too
  long off(int i) const { return table.e[i].offset; }
  const float* pf(int i) const { return P + table.e[i].offset; }            // fp32 parameter
  const void* pw(int i) const {                                             // GEMM operand in compute dtype
    if (dtype == ETP_BF16) return reinterpret_cast<const uint16_t*>(Wc) + table.e[i].offset;
    return (copy_in_f32 ? reinterpret_cast<const float*>(Wc) : P) + table.e[i].offset;
  }
};

// The checks etp_{waypoint,clip,depth}_bind share, refused under the entry point's name `who`.  `null_msg` names the pointers that
// engine may not leave null: the copy is one of them only where it is read in fp32 mode too.
inline int bind_arenas(const char* who, ArenaEngine* w, float* params, void* copy, const char* null_msg) {
  auto refuse = [&](const char* msg) { return fail(ETP_ERR_INVALID, std::string(who) + ": " + msg); };
  if (!w || !params || (w->copy_in_f32 && !copy)) return refuse(null_msg);
  if (w->dtype != ETP_F32 && !copy) return refuse("bf16 mode needs a shadow arena");
  if ((uintptr_t)params % 256 != 0 || (uintptr_t)copy % 256 != 0) return refuse("arenas must be 256-byte aligned");
  w->P = params; w->Wc = copy;
  return ETP_OK;
}

// Bump allocator over a caller-provided stash / workspace (null base: sizes only).  Every piece starts on a 256-byte granule, so
// `off` is the exact size of a plan carved from a 256-byte aligned base.  etp_clip_ws_bytes and etp_depth_ws_bytes return `off`;
// etp_waypoint_ws_bytes and the planner's etp_*_bytes return `off + 256` (a spare granule their callers have always been given).
// A size query and the entry point it serves must run the same plan function.
struct Bump {
  char* base; size_t off = 0;
  explicit Bump(void* b) : base(reinterpret_cast<char*>(b)) {}
  void* take(size_t bytes) {
    void* p = base ? base + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return p;
  }
};

// an unbatched, unsplit product with no epilogue extras: the starting point of every GemmArgs the engines fill in
inline GemmArgs base_args() {
  GemmArgs g{};
  g.nb_inner = 1; g.ksplit = 1; g.alpha = 1.f; g.drop = drop_none();
  return g;
}

}  // namespace etp
