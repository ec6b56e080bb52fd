// The routing decision of one scheduling call as data: which launch path each pod of a batch takes
// (DESIGN.md "Batch routing").  Standard library only -- no HIP, no engine context -- so the decision
// is checked on the CPU (tests/csrc/route_check.cpp); kgpu_api.cpp fills the inputs and issues.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace kgpu_route {

// What a pod asks of its route, from plain per-pod facts.
enum class PodKind : uint8_t {
  kTopo,   // carries topology state: a persistent topology run (k_tbatch) or the topology pipeline
  kNorm,   // needs the normalize pass and nothing else: k_nbatch when the call allows it
  kConst,  // constant normalize maxima: k_batch / k_cbatch when the call allows it
  kChain,  // its scoring fails: always one launch per pod
};
inline PodKind pod_kind(bool has_topo_plan, bool score_error, bool needs_norm) {
  return has_topo_plan ? PodKind::kTopo : score_error ? PodKind::kChain : needs_norm ? PodKind::kNorm : PodKind::kConst;
}

// What the engine and the call look like (every field a plain copy; nothing points into engine state).
struct CycleFacts {
  int32_t n = 0, short_max = 0;  // pods of the call; the longest short cycle
  bool diag = false, run_all = false, in_alias = false;
  bool topo_on = false, has_comm = false, multi_rank = false, xgmi = false, cut_state = false;
  bool nom_listed = false;  // the engine holds nominated pods at all
  bool timing = false, phase_trace = false, arena_on = false;
  bool persistent = false, cut_persistent = false, tfast = false, cut_topo_persistent = false, cut_topo_one = false;
  bool nbatch_row_ok = false, taint_fits = false;  // k_nbatch's profile row and statistics field
  int32_t norm_persistent = 0, K = 0;
};

// The call-level gates, each computed once.
struct CycleRoute {
  bool short_cycle = false;  // one pinned copy in, records straight into pinned memory
  bool xg = false;           // persistent runs exchange granules over xGMI
  bool sharded = false;
  bool cut = false;        // percentageOfNodesToScore trims the feasible set
  bool zc = false;         // pools may stay in pinned memory
  bool zero_diag = false;  // k_eval zeroes the per-plugin score rows itself
  bool inline_q = false;   // the query rides in the launch arguments
  // eligibility first (gates_nominated); the issuer clears one when no geometry fits the node count
  bool batch = false;   // constant-maxima pods run in k_batch / k_cbatch
  bool nbatch = false;  // normalize-pass pods run in k_nbatch (implies batch)
  bool tbatch = false;  // topology pods run in k_tbatch
  bool tb_arena = false;  // a one-pod k_tbatch run keeps its abort word in the arena
  // run-length limits of segment_end
  int32_t norm_persistent = 0;
  int32_t nbatch_max = INT32_MAX, batch_max = INT32_MAX;
};

// Gates known before the pools and the nominated pods are staged.
inline CycleRoute gates_call(const CycleFacts& f) {
  CycleRoute r;
  r.short_cycle = f.n <= f.short_max;
  r.xg = f.multi_rank && f.xgmi;
  r.sharded = f.has_comm || r.xg;
  r.cut = f.cut_state;
  // zc and inline_q describe the same cycles -- the ones whose only kernel is k_eval -- at two moments.
  // zc is needed before the pools are uploaded, when all that is known is whether the engine holds
  // nominated pods at all; it also keeps timed and traced cycles on device pools.  inline_q comes after
  // the nominated pods were staged and asks whether any of them applies to THIS pod.
  r.zc = r.short_cycle && f.n == 1 && f.diag && !f.topo_on && !f.has_comm && !f.multi_rank && !f.cut_state &&
         !f.nom_listed && !f.timing && !f.phase_trace;
  r.zero_diag = f.diag && !f.topo_on && !f.has_comm;
  return r;
}

// Gates that wait for the nominated pods: has_nom says that pass 1 (k_victims) runs for this pod.
inline void gates_nominated(CycleRoute& r, const CycleFacts& f, bool has_nom) {
  r.inline_q = r.short_cycle && f.n == 1 && f.diag && !f.topo_on && !f.has_comm && !f.multi_rank && !f.cut_state &&
               !has_nom;
  r.batch = f.persistent && !f.diag && (!r.cut || f.cut_persistent) && !has_nom && (r.xg || !r.sharded);
  r.nbatch = f.norm_persistent > 0 && r.batch && !r.sharded && !f.diag && !has_nom && f.nbatch_row_ok && f.taint_fits;
  // node-sharded engines take k_tbatch over the xGMI mailboxes, without them the per-pod RCCL pipeline; a
  // diagnostic cycle of one topology pod is a one-pod run; under a cut batch runs need
  // KGPU_OPT_CUT_TOPO_PERSISTENT and diagnostic cycles KGPU_OPT_CUT_TOPO_ONE as well (never the
  // aliased-list loop's cycles)
  r.tbatch = f.topo_on && f.tfast && (!f.diag || (f.n == 1 && !f.run_all)) && (!r.sharded || r.xg) &&
             (!r.cut || (f.cut_topo_persistent && (!f.diag || (f.cut_topo_one && !f.in_alias)))) && !has_nom &&
             f.K <= 64;
  r.norm_persistent = f.norm_persistent;
}

// Granule areas are capped at 64 MiB: a longer run continues in another launch (under a cut it takes
// up the rotation from cut_state).  k_nbatch holds `rounds` granules per pod and group and one
// position word per pod; k_cbatch two granules.
inline int32_t granule_cap(size_t rounds, int groups) {
  return (int32_t)std::max<size_t>(1, ((size_t)64 << 20) / (8 * rounds * (size_t)groups + 8));
}
inline void set_run_limits(CycleRoute& r, int groups, int32_t ring_cap) {
  r.nbatch_max = granule_cap(r.cut ? 3 : 2, groups);
  r.batch_max = r.cut ? granule_cap(2, groups) : r.xg ? ring_cap : INT32_MAX;
}

enum class Route : uint8_t { kTopo, kNBatch, kBatch, kChain };
inline Route route_of(PodKind k, const CycleRoute& r) {
  if (k == PodKind::kTopo) return Route::kTopo;
  if (k == PodKind::kNorm && r.nbatch) return Route::kNBatch;
  if (k == PodKind::kConst && r.batch) return Route::kBatch;
  return Route::kChain;
}

// The end of the run that starts at pod i.  A topology pod is a segment of its own here: how far a
// persistent topology run extends is t_add's decision, which is stateful and may refuse.
inline int32_t segment_end(const PodKind* kinds, int32_t n, int32_t i, const CycleRoute& r) {
  int32_t j = i;
  switch (route_of(kinds[i], r)) {
    case Route::kTopo:
      return i + 1;
    case Route::kNBatch: {
      // extends over the following non-topology pods; a constant-maxima pod is absorbed (exact: its maxima
      // come out 0) only while another normalize-pass pod lies within the next norm_persistent - 1 pods
      auto plain = [&](int32_t k) { return kinds[k] == PodKind::kNorm || kinds[k] == PodKind::kConst; };
      while (j < n && j - i < r.nbatch_max && plain(j)) {
        if (kinds[j] != PodKind::kNorm) {
          bool near = false;
          for (int32_t k = j + 1; k < n && k - j < r.norm_persistent && plain(k) && !near; ++k)
            near = kinds[k] == PodKind::kNorm;
          if (!near) break;
        }
        ++j;
      }
      return j;
    }
    case Route::kBatch:
      while (j < n && kinds[j] == PodKind::kConst && j - i < r.batch_max) ++j;
      return j;
    case Route::kChain:
      while (j < n && route_of(kinds[j], r) == Route::kChain) ++j;
      return j;
  }
  return j;
}

}  // namespace kgpu_route
