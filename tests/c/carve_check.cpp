// The layout arithmetic of csrc/r3d_carve.h as a stand-alone host program (plain C++17, no HIP).  For lists of pieces over element
// counts 0, 1, 255, 256, 257, element sizes 1, 4, 8, 12, 16 and alignments 16, 64, 256 it checks that the offsets ascend, that
// every offset is a multiple of its alignment, that the pieces are pairwise disjoint and that `bytes` is the rounded end of the
// last piece; then it carves a heap block of exactly `bytes` bytes and writes every byte of every piece (a sanitizer sees a
// byte too many).  One list passes 2^32 bytes: arithmetic only.  tests/test_host_logic.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "r3d_carve.h"

namespace {

struct E12 {
  char b[12];
};
struct E16 {
  char b[16];
};

struct Rec {
  size_t at, size, align;   // size: the bytes the caller writes (count * sizeof(T))
  std::function<char*(const r3d_carve&)> ptr;
};

int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAILED %s: ", #cond);       \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      ++failures;                              \
    }                                          \
  } while (0)

template <typename T>
void add(r3d_carve& c, std::vector<Rec>& recs, size_t count, size_t align) {
  const auto h = c.take<T>(count, align);
  recs.push_back({h.at, count * sizeof(T), align, [h](const r3d_carve& cc) { return reinterpret_cast<char*>(cc.at(h)); }});
}
void add_sized(r3d_carve& c, std::vector<Rec>& recs, int elem, size_t count, size_t align) {
  switch (elem) {
    case 1: add<uint8_t>(c, recs, count, align); break;
    case 4: add<uint32_t>(c, recs, count, align); break;
    case 8: add<uint64_t>(c, recs, count, align); break;
    case 12: add<E12>(c, recs, count, align); break;
    default: add<E16>(c, recs, count, align); break;
  }
}

// a piece of no elements still owns one byte: its pointer must alias nothing that is written
size_t extent(const Rec& r) { return r.size ? r.size : 1; }

void check_list(const char* name, const r3d_carve& c, const std::vector<Rec>& recs, bool touch) {
  for (size_t i = 0; i < recs.size(); ++i) {
    CHECK(recs[i].at % recs[i].align == 0, "%s piece %zu at %zu align %zu", name, i, recs[i].at, recs[i].align);
    if (i) CHECK(recs[i].at > recs[i - 1].at, "%s piece %zu at %zu after %zu", name, i, recs[i].at, recs[i - 1].at);
    for (size_t j = 0; j < i; ++j)
      CHECK(recs[j].at + extent(recs[j]) <= recs[i].at || recs[i].at + extent(recs[i]) <= recs[j].at, "%s pieces %zu and %zu overlap", name, j, i);
  }
  const Rec& last = recs.back();
  CHECK(c.bytes == r3d_align_up(last.at + extent(last), last.align), "%s bytes %zu, last piece ends at %zu", name, c.bytes, last.at + extent(last));
  if (!touch) return;
  r3d_carve placed = c;
  char* block = static_cast<char*>(std::malloc(placed.bytes));
  if (!block) std::exit(1);
  placed.place(block);
  for (size_t i = 0; i < recs.size(); ++i) {
    char* p = recs[i].ptr(placed);
    CHECK(p == block + recs[i].at, "%s piece %zu pointer", name, i);
    std::memset(p, (int)(i + 1), recs[i].size);
  }
  for (size_t i = 0; i < recs.size(); ++i)   // nobody wrote into another piece
    for (size_t k = 0; k < recs[i].size; ++k)
      if (recs[i].ptr(placed)[k] != (char)(i + 1)) {
        CHECK(false, "%s piece %zu byte %zu was overwritten", name, i, k);
        break;
      }
  std::free(block);
}

}  // namespace

int main() {
  const size_t counts[] = {0, 1, 255, 256, 257}, aligns[] = {16, 64, 256};
  const int elems[] = {1, 4, 8, 12, 16};
  int lists = 0;
  char name[64];
  // every element size in one list; the counts and the alignments rotate through it
  for (int rot = 0; rot < 3; ++rot)
    for (int ci = 0; ci < 5; ++ci) {
      r3d_carve c;
      std::vector<Rec> recs;
      for (int k = 0; k < 5; ++k) add_sized(c, recs, elems[k], counts[(ci + k) % 5], aligns[(k + rot) % 3]);
      std::snprintf(name, sizeof name, "mixed rot %d count %d", rot, ci);
      check_list(name, c, recs, true);
      ++lists;
    }
  // one count, one alignment, every element size (count 0: a list of nothing but empty pieces)
  for (size_t a : aligns)
    for (size_t n : counts) {
      r3d_carve c;
      std::vector<Rec> recs;
      for (int e : elems) add_sized(c, recs, e, n, a);
      std::snprintf(name, sizeof name, "uniform align %zu count %zu", a, n);
      check_list(name, c, recs, true);
      ++lists;
    }
  // the default alignment, an empty piece between two written ones
  {
    r3d_carve c;
    std::vector<Rec> recs;
    add<uint32_t>(c, recs, 257, 256);
    add<uint8_t>(c, recs, 0, 256);
    add<E12>(c, recs, 255, 256);
    check_list("empty between", c, recs, true);
    CHECK(recs[1].at >= recs[0].at + recs[0].size && recs[1].at + 1 <= recs[2].at, "the empty piece aliases a neighbour");
    ++lists;
  }
  // past 2^32 bytes: arithmetic only, nothing is allocated
  {
    r3d_carve c;
    std::vector<Rec> recs;
    add<E16>(c, recs, (size_t)1 << 28, 256);   // 2^32 bytes
    add<E12>(c, recs, ((size_t)1 << 28) + 1, 64);
    add<uint8_t>(c, recs, 257, 16);
    check_list("past 2^32", c, recs, false);
    CHECK(recs[1].at == (size_t)1 << 32 && recs[2].at > ((size_t)7 << 30) && c.bytes > ((size_t)7 << 30), "offsets past 2^32 wrapped: %zu %zu %zu",
          recs[1].at, recs[2].at, c.bytes);
    ++lists;
  }
  if (failures) {
    std::printf("%d checks FAILED\n", failures);
    return 1;
  }
  std::printf("%d lists\ncarve check OK\n", lists);
  return 0;
}
