// Host-side sanitizer check of the in-edge view of the graph
// (rnnlogic_amd/csrc/graph.cpp: build_in_edges, and the view rnnl_graph_create
// uploads from it).
//
// Built with g++ -fsanitize=address,undefined together with graph.cpp by
// tests/test_paths_host.py (CPU, no GPU).  The HIP runtime calls of graph.cpp
// are replaced by host stand-ins, as in graph_host_check.cpp, so the "device"
// arrays are host memory.  Seeded graphs with duplicate edges and isolated
// entities: the view holds every edge once, in (target, relation, source)
// order, copies of one triple in edge-id order, and every in-edge's id leads
// back to the edge tables' (source, target) of its relation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../rnnlogic_amd/csrc/internal.h"

static long g_live = 0;  // allocations not yet freed

extern "C" {
hipError_t hipMalloc(void **p, size_t n) {
  *p = malloc(n);
  if (!*p) return hipErrorOutOfMemory;
  ++g_live;
  return hipSuccess;
}
hipError_t hipFree(void *p) {
  if (p) --g_live;
  free(p);
  return hipSuccess;
}
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) {
  memcpy(d, s, n);
  return hipSuccess;
}
hipError_t hipGetDevice(int *d) {
  *d = 0;
  return hipSuccess;
}
const char *hipGetErrorString(hipError_t) { return "stub error"; }
}

static int g_checks = 0;
#define CHECK(c)                                                             \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(c)) {                                                              \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

// the view against the triples: n edges, hrt in file order
static void check_view(const std::vector<int32_t> &hrt, int E, int R, const int32_t *in_off, const int32_t *in_rel,
                       const int32_t *in_src, const int32_t *in_eid) {
  const int64_t n = (int64_t)hrt.size() / 3;
  // relation-local ids in file order, restated
  std::vector<int32_t> local(n), seen_of_rel(R, 0);
  for (int64_t i = 0; i < n; ++i) local[i] = seen_of_rel[hrt[3 * i + 1]]++;
  CHECK(in_off[0] == 0 && in_off[E] == n);
  std::vector<int> used(n, 0);  // file index -> times the view holds it
  for (int t = 0; t < E; ++t) {
    CHECK(in_off[t + 1] >= in_off[t]);
    for (int b = in_off[t]; b < in_off[t + 1]; ++b) {
      const int r = in_rel[b], s = in_src[b], id = in_eid[b];
      CHECK(r >= 0 && r < R && s >= 0 && s < E && id >= 0 && id < seen_of_rel[r]);
      if (b > in_off[t]) {  // (relation, source, id) strictly ascending inside a target
        const int pr = in_rel[b - 1], ps = in_src[b - 1], pid = in_eid[b - 1];
        CHECK(pr < r || (pr == r && (ps < s || (ps == s && pid < id))));
      }
      // the id leads back to one edge of the file: that edge is (s, r, t)
      int64_t at = -1;
      for (int64_t i = 0; i < n; ++i)
        if (hrt[3 * i + 1] == r && local[i] == id) at = i;
      CHECK(at >= 0 && hrt[3 * at] == s && hrt[3 * at + 2] == t);
      used[at]++;
    }
  }
  for (int64_t i = 0; i < n; ++i) CHECK(used[i] == 1);
}

int main() {
  std::mt19937 rng(11);
  auto U = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  int graphs = 0;
  long doubled = 0, isolated = 0;
  for (int it = 0; it < 40; ++it) {
    const int E = U(1, 40), R = U(1, 40), n = U(0, 250);
    // entities at and above `live` take no part: isolated
    const int live = U(1, E);
    std::vector<int32_t> hrt;
    for (int i = 0; i < n; ++i) {
      if (i > 0 && U(0, 3) == 0) {  // a copy of an earlier triple
        const int j = U(0, i - 1);
        for (int k = 0; k < 3; ++k) hrt.push_back(hrt[3 * j + k]);
        ++doubled;
        continue;
      }
      hrt.push_back(U(0, live - 1));
      hrt.push_back(U(0, R - 1));
      hrt.push_back(U(0, live - 1));
    }
    isolated += E - live;
    // the plain function: vectors in, vectors out
    std::vector<int32_t> in_off, in_rel, in_src, in_eid;
    rnnl::build_in_edges(hrt.data(), n, E, R, in_off, in_rel, in_src, in_eid);
    CHECK((int)in_off.size() == E + 1 && (int)in_rel.size() == n && (int)in_src.size() == n && (int)in_eid.size() == n);
    check_view(hrt, E, R, in_off.data(), in_rel.data(), in_src.data(), in_eid.data());
    // and what the handle holds, against the handle's own edge tables
    rnnl_graph g = nullptr;
    CHECK(rnnl_graph_create(hrt.empty() ? nullptr : hrt.data(), n, E, R, &g) == RNNL_OK);
    const rnnl::GraphDev &d = g->d;
    check_view(hrt, E, R, d.in_off, d.in_rel, d.in_src, d.in_eid);
    for (int t = 0; t < E; ++t)
      for (int b = d.in_off[t]; b < d.in_off[t + 1]; ++b) {
        const int e = d.edge_base[d.in_rel[b]] + d.in_eid[b];
        CHECK(e < d.edge_base[d.in_rel[b] + 1] && d.edge_src[e] == d.in_src[b] && d.edge_dst[e] == t);
      }
    CHECK(rnnl_graph_destroy(g) == RNNL_OK);
    ++graphs;
  }
  CHECK(g_live == 0);
  CHECK(doubled > 0 && isolated > 0);
  printf("in_edges_check: %d graphs, %ld copied triples, %ld isolated entities, %d checks, 0 live blocks\n", graphs,
         doubled, isolated, g_checks);
  return 0;
}
