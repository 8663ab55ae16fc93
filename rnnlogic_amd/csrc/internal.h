// Internal structures shared by the host builders (graph.cpp) and the HIP
// kernels.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rnnlogic_hip.h"

namespace rnnl {

// Vertex-major CSR of the train graph: edges (v --rel--> t) for fixed (v, rel)
// are col[off[v*R+rel] .. off[v*R+rel+1]), in train-file order.
struct GraphDev {
  int32_t E = 0, R = 0;
  int64_t n_edges = 0;
  const int32_t *off = nullptr;        // E*R + 1
  const int32_t *col = nullptr;        // n_edges
  // compact per-vertex view of off (L2-sized): for vertex v and relation word
  // w = rel >> 5, vbits[v * W + w] = (bitmap of v's relations with edges in
  // that word, index into dvoff of the word's first present relation); the
  // edges of (v, rel) are col[dvoff[pos] .. dvoff[pos + 1]) with
  // pos = .y + popcount(.x below rel's bit)
  int32_t W = 0;
  const uint2 *vbits = nullptr;        // E * W
  const int32_t *dvoff = nullptr;      // sum over v of (present relations + 1)
  const int32_t *edge_base = nullptr;  // R + 1: start of relation r's edge table
  const int32_t *edge_src = nullptr;   // relation-major, relation-local file order
  const int32_t *edge_dst = nullptr;
  // in-edge view (rnnl_paths_rows, paths.hip): the edges into t are [in_off[t], in_off[t + 1]), sorted by
  // (relation, source), copies of one triple by edge id; in_eid is the edge's relation-local id (edge_src's index
  // minus edge_base[relation]).  No E*R table: a relation's run is found by binary search in in_rel.
  const int32_t *in_off = nullptr;  // E + 1
  const int32_t *in_rel = nullptr;  // n_edges
  const int32_t *in_src = nullptr;  // n_edges
  const int32_t *in_eid = nullptr;  // n_edges
};

// Rule miner graph (mine.hip): out-edges grouped by source, in-edges grouped
// by target with sources ascending, and the train triples themselves.
struct MinerDev {
  int32_t E = 0, R = 0, n = 0;
  const int32_t *out_off = nullptr, *out_dst = nullptr, *out_rel = nullptr;  // E + 1, n, n
  const int32_t *in_off = nullptr, *in_src = nullptr, *in_rel = nullptr;     // E + 1, n, n
  const int32_t *th = nullptr, *tr = nullptr, *tt = nullptr;                 // n
};

// What the miner's learn / H_score stage adds to the handle (mine_learn.hip):
// the out-edges once more, sorted by (source, relation, target) under the same
// out_off, the in-edges once more, sorted by (target, relation, source) under
// in_off (the head side of mine_ground.h), the current rule lists and one Adam
// parameter + H per rule.
constexpr int RULE_STRIDE = 5;  // body relations stored per rule: the longest body

struct MinerLearnDev {
  const int32_t *so_rel = nullptr, *so_dst = nullptr;  // n, n
  const int32_t *si_rel = nullptr, *si_src = nullptr;  // n, n
  int32_t n_rules = 0;
  int32_t agg_depth = 1;               // RNNL_MINER_AGG_MAX: the classes a key keeps, 1..3 (mine_ground.h)
  const int32_t *rule_off = nullptr;   // R + 1: relation r's rules are [rule_off[r], rule_off[r + 1])
  const int32_t *rule_len = nullptr;   // n_rules, 0..RULE_STRIDE
  const int32_t *rule_body = nullptr;  // n_rules x RULE_STRIDE
  const double *prior = nullptr;       // n_rules
  double *wt = nullptr, *am = nullptr, *av = nullptr, *at = nullptr, *H = nullptr, *val = nullptr;  // n_rules
  // n_rules: the aggregation operand of rnnl_miner_set_aggregation (u_k of noisy-or, the class of max as a double)
  double *op = nullptr;
};

// Rule bodies as one prefix trie per head relation.  Node ids are global;
// the nodes of one head are contiguous, numbered breadth-first, so the
// children of a node are contiguous too.  Node 0 of a head is its root
// (empty prefix, relation -1).
struct RulesDev {
  int32_t n_rules = 0, n_nodes = 0, max_depth = 0, n_heads = 0;
  const int32_t *head_root = nullptr;   // R: root node id, -1 if the head has no rule
  const int32_t *head_depth = nullptr;  // R: deepest body length of the head
  const int32_t *head_nodes = nullptr;  // R: number of trie nodes of the head
  const int32_t *node_rel = nullptr;    // relation of the edge into the node
  const int32_t *node_child = nullptr;  // first child id
  const int32_t *node_nchild = nullptr;
  const int32_t *node_nrules = nullptr;    // rules whose body ends exactly here
  const int32_t *node_rule_ptr = nullptr;  // n_nodes + 1
  const int32_t *node_rules = nullptr;     // member rule ids, ascending
  const uint64_t *node_fp = nullptr;       // sum of mix64(rule id) of members (digest only)
  // leaves (nodes where >= 1 rule ends), numbered per head for LDS staging
  int32_t max_leaves = 0, max_head_nodes = 0;
  const int32_t *head_leaf_ptr = nullptr;   // R + 1
  const int32_t *head_leaf_node = nullptr;  // leaf node ids, head-major, ascending node id
  const int32_t *node_leaf = nullptr;       // n_nodes: local leaf index within its head, -1 if none
  // the grounding walk's per-node fields in one 16-B load: (rel, first child, nchild, nrules)
  const int4 *node_info = nullptr;
  // the rule encoder over the trie (rnnl_lstm_encode_trie): per node its
  // parent (-1 at a root) and LSTM input token (the head relation at a root,
  // else node_rel); the nodes grouped by depth (level_nodes, host level_ptr)
  const int32_t *node_parent = nullptr;
  const int32_t *node_tok = nullptr;
  const int32_t *level_nodes = nullptr;
  // rnnl_paths_rows: the trie node where each rule's body ends (the host's node_of_rule) and each node's depth
  // (the length of the body that ends there)
  const int32_t *rule_node = nullptr;   // n_rules
  const int32_t *node_depth = nullptr;  // n_nodes
};

// Node-weight records (bytes per node); see rnnl_node_weights.
constexpr int kHidden = 16;
constexpr int kStrideSum = 64;   // f32 sum x[16]
constexpr int kStridePna = 256;  // int32 fix(sum x)[16] | int32 fix(sum x^2)[16] | f32 min[16] | f32 max[16]
                                 // (one shift per table and column: trailer[1], trailer[4])

void set_error(const std::string &msg);

// The in-edge view of GraphDev from the triples (n x 3: h r t, checked by the caller to be in range): a plain host
// function, vectors out (graph.cpp; tests/asan/in_edges_check.cpp checks it on its own).
void build_in_edges(const int32_t *hrt, int64_t n, int32_t E, int32_t R, std::vector<int32_t> &in_off,
                    std::vector<int32_t> &in_rel, std::vector<int32_t> &in_src, std::vector<int32_t> &in_eid);

// The SUM node records' fixed-point pass (node_fix_kernel, ground.hip) over
// every node of the table (rnnl_lstm_encode_trie_sum's last launch).
int node_fix_enqueue(rnnl_rules r, void *node_w, void *stream);

// rnnl_rotate_score_pieces with a nullable map from query to score row
// (rotate.hip; the forward over the distinct (h, r) keys of the caller's rows).
int rotate_score_rows(const float *eemb, const void *etab, const float *rtab, int32_t D, float gamma,
                      const int64_t *all_h, const int64_t *all_r, int32_t nq, int32_t E, float *score,
                      int32_t accumulate, int32_t mode, void *workspace, size_t ws_bytes, int32_t pieces_req,
                      float first_share, const int32_t *row_of, void *stream);

}  // namespace rnnl

struct rnnl_miner_s {
  rnnl::MinerDev d;
  rnnl::MinerLearnDev l;
  std::vector<void *> bufs;       // the graph (rnnl_miner_create)
  std::vector<void *> rule_bufs;  // rule lists, parameters, scratch (rnnl_miner_set_rules)
  unsigned char *ground_scratch = nullptr, *chain_scratch = nullptr;
  int32_t ground_blocks = 0;
  unsigned char *eval_scratch = nullptr;  // rnnl_miner_evaluate above its LDS regime; one of bufs
  int32_t eval_blocks = 0;
  // rnnl_miner_predict above its LDS regime: per workgroup a list (int) and a flag byte per entity; one of bufs
  unsigned char *pred_flags = nullptr;
  // rnnl_miner_paths_side above its LDS regime: per workgroup the kept levels of one grounding; one of bufs
  unsigned char *path_scratch = nullptr;
  // how evaluate / predict / explain form val (rnnl_miner_set_aggregation); set_rules puts it back to SUM
  int32_t agg = 0;
};

struct rnnl_graph_s {
  rnnl::GraphDev d;
  int device = 0;
  void *mem[11] = {};
};

struct rnnl_rules_s {
  rnnl::RulesDev d;
  int device = 0;
  int32_t R = 0, E = 0;
  void *mem[20] = {};
  std::vector<int32_t> node_of_rule;  // host: trie node where each rule's body ends
  std::vector<int32_t> level_ptr;     // host: max_depth + 2 offsets into d.level_nodes
  std::vector<int32_t> head_root;     // host copy of d.head_root (R)
  std::vector<int32_t> head_nodes;    // host copy of d.head_nodes (R)
  // the largest head trie without its root where no rule ends there (an empty
  // body): the nodes that can hold a grounding entry (predictor.hip's LDS tables)
  int32_t max_head_slots = 0;
};

#define RNNL_HIP_CHECK(expr)                                                              \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      rnnl::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                 \
      return RNNL_ERR_HIP;                                                                \
    }                                                                                     \
  } while (0)
