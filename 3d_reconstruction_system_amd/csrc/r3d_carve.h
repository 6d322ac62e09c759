// One device block divided into typed pieces laid end to end: the size to ask for and every pointer come from the same list of
// take() calls, so they cannot disagree.  Host only, no HIP: tests/c/carve_check.cpp builds it alone.
//   r3d_carve ws;
//   const auto idx = ws.take<uint32_t>(n), d2 = ws.take<float>(n);   // before the block exists: sizes only
//   r3d_scratch(ctx, kWsIn, ws);                                      // ws.bytes claimed, ws placed (r3d_internal.h)
//   kernel(ws.at(idx), ws.at(d2));                                    // the only casts
// The layout is a pure function of the take() calls.  A piece begins at a multiple of its alignment (a power of two; the block
// itself is 256-byte aligned) and is padded to one, so `bytes` is always the rounded end of the last piece and two pieces whose
// sizes are multiples of the second one's alignment lie back to back (one copy or memset may span them).  A piece of no
// elements still gets one alignment's worth: its pointer aliases nothing that is written.
#pragma once

#include <cstddef>

// bytes rounded up to a multiple of `a`, a power of two
constexpr size_t r3d_align_up(size_t bytes, size_t a) { return (bytes + a - 1) & ~(a - 1); }

struct r3d_carve {
  template <typename T>
  struct piece {
    size_t at;   // byte offset in the block
  };
  size_t bytes = 0;   // the total to ask for
  char* block = nullptr;

  template <typename T>
  piece<T> take(size_t count, size_t align = 256) {
    const size_t at = r3d_align_up(bytes, align);
    bytes = at + r3d_align_up(count ? count * sizeof(T) : 1, align);
    return {at};
  }
  void place(void* b) { block = static_cast<char*>(b); }
  template <typename T>
  T* at(piece<T> p) const {
    return reinterpret_cast<T*>(block + p.at);
  }
};
