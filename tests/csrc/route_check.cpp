// CPU check of kgpu_route.h (tests/test_route.py builds it with ASan + UBSan): the routing plan of a
// scheduling call -- pod kinds, call gates, run segmentation -- against properties stated here
// independently of segment_end's loops, over every kind sequence up to six pods.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "kgpu_route.h"

using namespace kgpu_route;

namespace {
int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
      if (++failures > 20) std::exit(1);                   \
    }                                                      \
  } while (0)

const PodKind T = PodKind::kTopo, N = PodKind::kNorm, C = PodKind::kConst, E = PodKind::kChain;

std::string show(const std::vector<PodKind>& k) {
  std::string s;
  for (PodKind x : k) s += x == T ? 'T' : x == N ? 'N' : x == C ? 'C' : 'E';
  return s;
}

CycleRoute gates(bool batch, int norm_persistent, bool cut, bool tbatch) {
  CycleRoute r;
  r.batch = batch;
  r.nbatch = batch && norm_persistent > 0;
  r.norm_persistent = norm_persistent;
  r.cut = cut;
  r.tbatch = tbatch;
  return r;
}

bool plain(PodKind k) { return k == N || k == C; }

// segment lengths of the walk (empty when the walk itself is broken)
std::vector<int> walk(const std::vector<PodKind>& k, const CycleRoute& r) {
  std::vector<int> out;
  const int32_t n = (int32_t)k.size();
  for (int32_t i = 0; i < n;) {
    const int32_t j = segment_end(k.data(), n, i, r);
    if (j <= i || j > n) return {};
    out.push_back(j - i);
    i = j;
  }
  return out;
}

void check_sequence(const std::vector<PodKind>& k, const CycleRoute& r) {
  const int32_t n = (int32_t)k.size();
  const std::string s = show(k);
  int32_t i = 0;
  while (i < n) {
    const int32_t j = segment_end(k.data(), n, i, r);
    // partition: in order, no empty segment, nothing past the end
    CHECK(j > i && j <= n, "%s at %d: end %d", s.c_str(), i, j);
    if (j <= i || j > n) return;
    const Route route = route_of(k[(size_t)i], r);
    const bool more = j < n;
    switch (route) {
      case Route::kTopo:  // one pod: t_add decides how far a persistent run goes
        CHECK(k[(size_t)i] == T && j == i + 1, "%s at %d", s.c_str(), i);
        break;
      case Route::kBatch:
        CHECK(r.batch, "%s at %d: k_batch while persistent is off", s.c_str(), i);
        for (int32_t p = i; p < j; ++p) CHECK(k[(size_t)p] == C, "%s at %d: k_batch run holds pod %d", s.c_str(), i, p);
        CHECK(j - i <= r.batch_max, "%s at %d: k_batch run of %d", s.c_str(), i, j - i);
        CHECK(!more || k[(size_t)j] != C || j - i == r.batch_max, "%s at %d: k_batch run stops early at %d", s.c_str(), i, j);
        break;
      case Route::kNBatch:
        CHECK(r.nbatch && r.batch, "%s at %d: k_nbatch while it is off", s.c_str(), i);
        CHECK(k[(size_t)i] == N, "%s at %d: k_nbatch run starts at another kind", s.c_str(), i);
        CHECK(j - i <= r.nbatch_max, "%s at %d: k_nbatch run of %d", s.c_str(), i, j - i);
        for (int32_t p = i; p < j; ++p) {
          CHECK(plain(k[(size_t)p]), "%s at %d: k_nbatch run holds pod %d", s.c_str(), i, p);
          if (k[(size_t)p] != C) continue;
          // absorbed: another normalize pod within norm_persistent - 1, reached over plain pods only
          bool near = false;
          for (int32_t q = p + 1; q < n && q - p <= r.norm_persistent - 1 && plain(k[(size_t)q]); ++q)
            near = near || k[(size_t)q] == N;
          CHECK(near, "%s at %d: constant-maxima pod %d absorbed with no normalize pod near", s.c_str(), i, p);
        }
        // the run's last pod is a normalize pod unless the cap cut it
        CHECK(k[(size_t)j - 1] == N || j - i == r.nbatch_max, "%s at %d: k_nbatch run ends on pod %d", s.c_str(), i, j - 1);
        if (more && j - i < r.nbatch_max) {
          CHECK(k[(size_t)j] != N, "%s at %d: k_nbatch run stops before normalize pod %d", s.c_str(), i, j);
          bool near = false;
          for (int32_t q = j + 1; k[(size_t)j] == C && q < n && q - j <= r.norm_persistent - 1 && plain(k[(size_t)q]); ++q)
            near = near || k[(size_t)q] == N;
          CHECK(!near, "%s at %d: constant-maxima pod %d left out with a normalize pod near", s.c_str(), i, j);
        }
        break;
      case Route::kChain:
        for (int32_t p = i; p < j; ++p)
          CHECK(route_of(k[(size_t)p], r) == Route::kChain, "%s at %d: the chain swallowed pod %d", s.c_str(), i, p);
        CHECK(!more || route_of(k[(size_t)j], r) != Route::kChain, "%s at %d: the chain stops early at %d", s.c_str(), i, j);
        break;
    }
    i = j;
  }
}

void exhaustive() {
  const PodKind all[4] = {T, N, C, E};
  long checked = 0;
  for (int n = 1; n <= 6; ++n) {
    int total = 1;
    for (int d = 0; d < n; ++d) total *= 4;
    std::vector<PodKind> k((size_t)n);
    for (int code = 0; code < total; ++code) {
      for (int d = 0, v = code; d < n; ++d, v /= 4) k[(size_t)d] = all[v % 4];
      for (int batch = 0; batch < 2; ++batch)
        for (int np : {0, 1, 3})
          for (int cut = 0; cut < 2; ++cut)
            for (int tb = 0; tb < 2; ++tb)
              for (int capped = 0; capped < 2; ++capped) {
                if (np > 0 && !batch) continue;  // k_nbatch needs the persistent batch geometry
                CycleRoute r = gates(batch != 0, np, cut != 0, tb != 0);
                if (capped) r.batch_max = r.nbatch_max = 2;
                check_sequence(k, r);
                ++checked;
              }
    }
  }
  std::printf("exhaustive: %ld walks\n", checked);
}

void expect(const std::vector<PodKind>& k, const CycleRoute& r, const std::vector<int>& want, const char* what) {
  const std::vector<int> got = walk(k, r);
  std::string g, w;
  for (int x : got) g += std::to_string(x) + " ";
  for (int x : want) w += std::to_string(x) + " ";
  CHECK(got == want, "%s: %s gives [ %s] for [ %s]", what, show(k).c_str(), g.c_str(), w.c_str());
}

void written_out() {
  // every other pod has constant maxima, the first one too, the last is a normalize pod (test_norm_persistent's
  // absorb rule): a window of 8 or 2 puts all but the first into one k_nbatch run, a window of 1 none
  const std::vector<PodKind> alt = {C, N, C, N, C, N};
  expect(alt, gates(true, 8, false, false), {1, 5}, "window 8");
  expect(alt, gates(true, 2, false, false), {1, 5}, "window 2");
  expect(alt, gates(true, 1, false, false), {1, 1, 1, 1, 1, 1}, "window 1");
  expect(alt, gates(true, 0, false, false), {1, 1, 1, 1, 1, 1}, "k_nbatch off: chain and k_batch alternate");
  // absorbed only while another normalize pod lies within the next norm_persistent - 1 pods
  expect({N, C, C, N}, gates(true, 3, false, false), {4}, "two constant pods inside a window of 3");
  expect({N, C, C, N}, gates(true, 2, false, false), {1, 2, 1}, "two constant pods against a window of 2");
  expect({N, C}, gates(true, 8, false, false), {1, 1}, "a trailing constant pod goes to k_batch");
  // the look-ahead does not cross a topology pod or a pod whose scoring fails
  expect({N, C, T, N}, gates(true, 8, false, true), {1, 1, 1, 1}, "look-ahead stops at a topology pod");
  expect({N, C, E, N}, gates(true, 8, false, false), {1, 1, 1, 1}, "look-ahead stops at a failing pod");
  // without a persistent geometry (or in a diagnostic cycle) everything but topology is one chain
  expect({C, N, E, C}, gates(false, 0, false, false), {4}, "persistent off");
  expect({C, N, T, C}, gates(false, 0, false, false), {2, 1, 1}, "persistent off around a topology pod");
  expect({C, C, E, C}, gates(true, 0, false, false), {2, 1, 1}, "a failing pod splits a k_batch run");
  expect({N, N, C, C}, gates(true, 0, true, false), {2, 2}, "a chain of normalize pods, then k_cbatch");
  // caps: the granule area and the xGMI ring split runs
  CycleRoute r = gates(true, 0, false, false);
  r.xg = true;
  set_run_limits(r, 4, 2);
  CHECK(r.batch_max == 2, "ring cap %d", r.batch_max);
  expect({C, C, C, C, C}, r, {2, 2, 1}, "ring cap 2");
  r = gates(true, 3, true, false);
  r.batch_max = r.nbatch_max = 2;
  expect({C, C, C, C, C}, r, {2, 2, 1}, "cut cap 2");
  expect({N, N, N, C, N}, r, {2, 2, 1}, "k_nbatch cap 2");  // N N | N C (absorbed: N follows; the cap ends it) | N
}

void limits() {
  for (int groups : {1, 4, 120, 256}) {
    CycleRoute r = gates(true, 1, false, false);
    set_run_limits(r, groups, 256);
    CHECK(r.batch_max == INT32_MAX, "no cap without a cut");
    CHECK(r.nbatch_max == (int32_t)(((size_t)64 << 20) / (16 * (size_t)groups + 8)), "k_nbatch, two rounds");
    r.cut = true;
    set_run_limits(r, groups, 256);
    CHECK(r.batch_max == (int32_t)(((size_t)64 << 20) / (16 * (size_t)groups + 8)), "k_cbatch");
    CHECK(r.nbatch_max == (int32_t)(((size_t)64 << 20) / (24 * (size_t)groups + 8)), "k_nbatch, three rounds");
  }
}

void kinds_and_gates() {
  CHECK(pod_kind(true, true, true) == T && pod_kind(true, false, false) == T, "a topology plan wins");
  CHECK(pod_kind(false, true, true) == E && pod_kind(false, true, false) == E, "a failing score is the chain's");
  CHECK(pod_kind(false, false, true) == N && pod_kind(false, false, false) == C, "normalize pass or not");

  CycleFacts one;  // kgpu_schedule_one of a plain pod
  one.n = 1;
  one.short_max = 8;
  one.diag = true;
  one.persistent = one.tfast = one.arena_on = true;
  CycleRoute r = gates_call(one);
  gates_nominated(r, one, false);
  CHECK(r.short_cycle && r.zc && r.inline_q && r.zero_diag && !r.batch && !r.nbatch && !r.tbatch, "plain one-pod cycle");
  // zc and inline_q part ways on timing and on nominated pods that do not apply to this pod
  CycleFacts f = one;
  f.timing = true;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(!r.zc && r.inline_q, "timed cycle");
  f = one;
  f.nom_listed = true;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(!r.zc && r.inline_q, "nominated pods, none for this pod");
  gates_nominated(r, f, true);
  CHECK(!r.zc && !r.inline_q, "a nominated pod applies");
  f = one;
  f.cut_state = true;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(!r.zc && !r.inline_q && r.cut, "under a cut");

  CycleFacts b;  // a batch on one GPU
  b.n = 70;
  b.short_max = 8;
  b.persistent = true;
  b.norm_persistent = 1;
  b.nbatch_row_ok = b.taint_fits = true;
  r = gates_call(b);
  gates_nominated(r, b, false);
  CHECK(!r.short_cycle && r.batch && r.nbatch && !r.tbatch && !r.zc && !r.inline_q, "batch");
  f = b;
  f.taint_fits = false;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(r.batch && !r.nbatch, "taint maximum too large for the granule field");
  f = b;
  f.cut_state = true;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(!r.batch && !r.nbatch, "a cut without KGPU_OPT_CUT_PERSISTENT");
  f.cut_persistent = true;
  gates_nominated(r, f, false);
  CHECK(r.batch && r.nbatch, "a cut with it");
  f = b;
  f.has_comm = true;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(r.sharded && !r.xg && !r.batch && !r.nbatch, "RCCL sharding: the per-pod exchange");
  f.multi_rank = f.xgmi = true;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(r.sharded && r.xg && r.batch && !r.nbatch, "xGMI mailboxes carry k_batch, not k_nbatch");
  f = b;
  f.diag = true;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(!r.batch && !r.nbatch, "diagnostic batch");

  CycleFacts t = b;  // topology
  t.topo_on = t.tfast = true;
  t.K = 64;
  r = gates_call(t);
  gates_nominated(r, t, false);
  CHECK(r.tbatch, "topology batch");
  gates_nominated(r, t, true);
  CHECK(!r.tbatch && !r.batch, "nominated pods keep the per-pod launches");
  f = t;
  f.K = 65;
  gates_nominated(r, f, false);
  CHECK(!r.tbatch, "more than 64 classes");
  f = t;
  f.diag = true;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(!r.tbatch && !r.zero_diag, "a diagnostic topology batch");
  f.n = 1;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(r.tbatch, "a diagnostic topology pod");
  f.run_all = true;
  gates_nominated(r, f, false);
  CHECK(!r.tbatch, "runAllFilters");
  f.run_all = false;
  f.cut_state = f.cut_topo_persistent = true;
  r = gates_call(f);
  gates_nominated(r, f, false);
  CHECK(!r.tbatch, "a diagnostic topology pod under a cut");
  f.cut_topo_one = true;
  gates_nominated(r, f, false);
  CHECK(r.tbatch, "... with KGPU_OPT_CUT_TOPO_ONE");
  f.in_alias = true;
  gates_nominated(r, f, false);
  CHECK(!r.tbatch, "... but not inside the aliased-list loop");
}
}  // namespace

int main() {
  exhaustive();
  written_out();
  limits();
  kinds_and_gates();
  if (failures) return 1;
  std::printf("route ok\n");
  return 0;
}
