// The workspace arithmetic of csrc/r3d_compact_dev.h (Counters) as a stand-alone host program: for every (tiles, rows) it carves
// a heap block of exactly `bytes` bytes, writes every counter of every row and the rows' totals (a sanitizer sees a byte
// too many), and prints: tiles rows stride bytes row_offset... totals_offset.  tests/test_host_logic.py checks the numbers.
#include <cstdio>
#include <cstdlib>

#include "r3d_compact_dev.h"

int main() {
  const int tiles[] = {0, 1, 7, 8, 9}, rows[] = {1, 2};
  for (int t : tiles)
    for (int r : rows) {
      r3d_compact::Counters c(t, r);
      char* block = static_cast<char*>(std::malloc(c.bytes));
      if (!block) return 1;
      c.place(block);
      std::printf("%d %d %d %zu", c.tiles, c.rows, c.stride, c.bytes);
      for (int k = 0; k < r; ++k) {
        for (int i = 0; i < c.stride; ++i) c.row(k)[i] = 1u;
        c.totals[k] = 2u;
        std::printf(" %td", reinterpret_cast<char*>(c.row(k)) - block);
      }
      std::printf(" %td\n", reinterpret_cast<char*>(c.totals) - block);
      std::free(block);
    }
  std::printf("layout check OK\n");
  return 0;
}
