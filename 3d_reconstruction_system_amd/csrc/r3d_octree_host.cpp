// OctoMap binary (.bt) export on the host: sorted 48-bit Morton codes of the occupied voxels -> the pruned octree, depth-first.
// A child subtree is a pruned leaf exactly when its code range holds 8^(levels below) codes.  Plain C++ with threads, no device
// code; the device serialiser that produces the same bytes is r3d_octree.hip, which also spells the header.
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "r3d_hostpool.h"
#include "r3d_internal.h"

namespace {

constexpr int kDepth = 16;

struct BtWriter {
  const uint64_t* codes;
  std::string body;
  int64_t n_nodes = 0;

  static bool full(int64_t count, int child_depth) {
    const int levels = kDepth - child_depth;  // 8^levels leaves below a node at child_depth
    return levels <= 20 && count == ((int64_t)1 << (3 * levels));
  }

  // one node record: child boundaries, the two mask bytes, and which children are inner nodes
  int record(int64_t lo, int64_t hi, int depth, int64_t inner[8][2]) {
    ++n_nodes;
    const int shift = 3 * (kDepth - 1 - depth);
    int64_t bounds[9];
    bounds[0] = lo;
    for (int c = 1; c <= 8; ++c) {
      // first index whose child id at this level is >= c
      const uint64_t* first = std::lower_bound(codes + bounds[c - 1], codes + hi, (uint64_t)c,
                                               [shift](uint64_t v, uint64_t cc) { return ((v >> shift) & 7u) < cc; });
      bounds[c] = first - codes;
    }
    unsigned char b[2] = {0, 0};
    int n_inner = 0;
    for (int c = 0; c < 8; ++c) {
      const int64_t clo = bounds[c], chi = bounds[c + 1];
      if (chi == clo) continue;
      if (depth + 1 == kDepth || full(chi - clo, depth + 1)) {
        b[c / 4] |= (unsigned char)(2u << (2 * (c % 4)));  // occupied leaf (possibly a pruned subtree)
        ++n_nodes;
      } else {
        b[c / 4] |= (unsigned char)(3u << (2 * (c % 4)));
        inner[n_inner][0] = clo;
        inner[n_inner][1] = chi;
        ++n_inner;
      }
    }
    body.push_back((char)b[0]);
    body.push_back((char)b[1]);
    return n_inner;
  }

  void node(int64_t lo, int64_t hi, int depth) {
    int64_t inner[8][2];
    const int n_inner = record(lo, hi, depth, inner);
    for (int k = 0; k < n_inner; ++k) node(inner[k][0], inner[k][1], depth + 1);
  }
};

// Depth-first order means a subtree's bytes are one contiguous run: the subtrees hanging below `split_depth`
// are serialised by worker threads and spliced in order.
void build_parallel(const uint64_t* codes, int64_t n, std::string* body, int64_t* n_nodes) {
  constexpr int kSplitDepth = 3;  // up to 512 independent subtrees
  struct Piece {
    bool is_task;
    int64_t lo, hi;
    std::string bytes;
    int64_t nodes = 0;
  };
  std::vector<Piece> pieces;
  BtWriter top;
  top.codes = codes;
  // walk the top levels sequentially; every inner child at kSplitDepth becomes a task
  struct Frame {
    int64_t lo, hi;
    int depth;
  };
  std::vector<Frame> stack;
  stack.push_back({0, n, 0});
  while (!stack.empty()) {
    const Frame f = stack.back();
    stack.pop_back();
    if (f.depth >= kSplitDepth || f.hi - f.lo < 4096) {
      if (!top.body.empty()) {
        pieces.push_back({false, 0, 0, std::move(top.body), 0});
        top.body.clear();
      }
      pieces.push_back({true, f.lo, f.hi, std::string(), 0});
      pieces.back().nodes = f.depth;  // stash the depth until the worker overwrites it
      continue;
    }
    int64_t inner[8][2];
    const int n_inner = top.record(f.lo, f.hi, f.depth, inner);
    for (int k = n_inner - 1; k >= 0; --k) stack.push_back({inner[k][0], inner[k][1], f.depth + 1});  // DFS order
  }
  if (!top.body.empty()) pieces.push_back({false, 0, 0, std::move(top.body), 0});
  unsigned hw = r3d_host::cpu_budget();
  const unsigned n_workers = std::max(1u, std::min(hw == 0 ? 1u : hw, 32u));
  std::vector<std::thread> pool;
  std::atomic<size_t> next{0};
  const r3d_host::Spread spread;
  for (unsigned w = 0; w < n_workers; ++w)
    pool.emplace_back([&, w]() {
      spread.place(w);
      for (;;) {
        const size_t i = next.fetch_add(1);
        if (i >= pieces.size()) return;
        Piece& p = pieces[i];
        if (!p.is_task) continue;
        BtWriter sub;
        sub.codes = codes;
        sub.node(p.lo, p.hi, (int)p.nodes);
        p.bytes = std::move(sub.body);
        p.nodes = sub.n_nodes;
      }
    });
  for (auto& t : pool) t.join();
  size_t total = 0;
  int64_t nodes = top.n_nodes;
  for (const auto& p : pieces) {
    total += p.bytes.size();
    if (p.is_task) nodes += p.nodes;
  }
  body->clear();
  body->reserve(total);
  for (const auto& p : pieces) body->append(p.bytes);
  *n_nodes = nodes;
}

int build_bt(const uint64_t* codes, int64_t n, double res, std::string* out, int64_t* n_nodes) {
  for (int64_t i = 1; i < n; ++i)
    if (codes[i] <= codes[i - 1]) {
      r3d_set_error("octree export needs strictly ascending Morton codes (violated at index %lld)", (long long)i);
      return R3D_ERR_INVALID;
    }
  if (n > 0 && (codes[n - 1] >> 48) != 0) {
    r3d_set_error("Morton code above 48 bits");
    return R3D_ERR_INVALID;
  }
  struct {
    std::string body;
    int64_t n_nodes = 0;
  } w;
  if (n > 0) {
    if (BtWriter::full(n, 0)) {
      w.n_nodes = 1;
      w.body.assign(2, '\0');
    } else {
      build_parallel(codes, n, &w.body, &w.n_nodes);
    }
  }
  char head[256];
  size_t head_bytes = 0;
  int rc = r3d_octree_bt_header(w.n_nodes, res, head, sizeof(head), &head_bytes);   // the one place the header is spelled (r3d_octree.hip)
  if (rc) return rc;
  *out = std::string(head, head_bytes) + w.body;
  *n_nodes = w.n_nodes;
  return R3D_OK;
}

}  // namespace

extern "C" {

int r3d_octree_format_bt(const uint64_t* h_codes_sorted, int64_t n_codes, double resolution, char* h_buf,
                         size_t buf_cap, size_t* n_bytes_out, int64_t* n_nodes_out) {
  if (n_codes < 0 || (n_codes > 0 && !h_codes_sorted) || !n_bytes_out || !(resolution > 0.0)) {
    r3d_set_error("r3d_octree_format_bt: bad argument");
    return R3D_ERR_INVALID;
  }
  std::string out;
  int64_t nodes = 0;
  int rc = build_bt(h_codes_sorted, n_codes, resolution, &out, &nodes);
  if (rc) return rc;
  *n_bytes_out = out.size();
  if (n_nodes_out) *n_nodes_out = nodes;
  if (!h_buf) return R3D_OK;
  if (buf_cap < out.size()) {
    r3d_set_error("r3d_octree_format_bt: buffer of %zu bytes is too small for %zu", buf_cap, out.size());
    return R3D_ERR_NOMEM;
  }
  memcpy(h_buf, out.data(), out.size());
  return R3D_OK;
}

int r3d_octree_write_bt(const char* path, const uint64_t* h_codes_sorted, int64_t n_codes, double resolution,
                        int64_t* n_nodes_out) {
  if (!path || n_codes < 0 || (n_codes > 0 && !h_codes_sorted) || !(resolution > 0.0)) {
    r3d_set_error("r3d_octree_write_bt: bad argument");
    return R3D_ERR_INVALID;
  }
  std::string out;
  int64_t nodes = 0;
  int rc = build_bt(h_codes_sorted, n_codes, resolution, &out, &nodes);
  if (rc) return rc;
  FILE* f = fopen(path, "wb");
  if (!f) {
    r3d_set_error("r3d_octree_write_bt: cannot open '%s'", path);
    return R3D_ERR_INVALID;
  }
  const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
  if (fclose(f) != 0 || !ok) {
    r3d_set_error("r3d_octree_write_bt: short write to '%s'", path);
    return R3D_ERR_INVALID;
  }
  if (n_nodes_out) *n_nodes_out = nodes;
  return R3D_OK;
}

}  // extern "C"
