// Lock-free union-find over a device array of uint32 parents, for gfx950 (MI355X): the find / hook primitives of the mesh
// component labelling (r3d_mesh_cc.hip), kept apart so that other labellings (clusters over a neighbour graph) can include them.
//
// The array.  parent[v] <= v, always: it starts as parent[v] = v, and every store is an atomicMin with a smaller value.  A vertex
// with parent[v] == v is a root.  Every value parent[v] ever holds is a vertex of v's own component.
//
// Memory model.  Lanes of other compute units hook while this lane reads.  Every access to the array is a relaxed agent-scope
// atomic (loads bypass the compute unit's L1, which another unit's stores never refresh), and nothing here needs more than that:
// no value is published through the array, so there is no release / acquire pair, no fence and no flag.  A STALE parent read is
// still an ancestor: it is a value parent[v] held earlier, the array only ever moves a vertex's parent DOWN its own ancestor
// chain or onto a smaller vertex of the same component, so an old value is a vertex of the same component that is <= v, and a
// walk that continues from it still descends towards that component's smallest vertex.  Staleness costs steps, never the result.
//
// No lane ever waits for another: there is no lock, no spin on a flag, no barrier.  Every loop below walks a strictly decreasing
// sequence of vertex numbers, bounded below by 0, whatever the other lanes do -- that is the whole termination argument, and it
// is repeated at each loop.
//
// When all hooks of a launch have returned (the kernel boundary), the vertices of a component form ONE tree whose root is the
// component's smallest vertex: DESIGN.md section 4.5j' has the argument.  find_root in a LATER launch then
// gives every vertex its label.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace r3d_uf {

__device__ __forceinline__ uint32_t parent_of(const uint32_t* parent, uint32_t v) {
  return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above v as this lane sees it, halving the path on the way: parent[v] <- min(parent[v], its grandparent).  The
// grandparent g was read as parent[p] of the p read as parent[v]: an ancestor, g <= p, of the same component, so the atomicMin
// keeps every property of the array.  The result may be out of date the moment it returns (another lane may hook it): callers
// re-check with the atomicMin of hook().
__device__ __forceinline__ uint32_t find_halving(uint32_t* parent, uint32_t v) {
  uint32_t p = parent_of(parent, v);
  // terminates: p < v whenever the loop runs on (parent[x] <= x, stale or not), so v strictly decreases and is >= 0
  while (p != v) {
    const uint32_t g = parent_of(parent, p);
    if (g != p) atomicMin(parent + v, g);
    v = p;
    p = g;
  }
  return v;
}

// Read-only walk to the root: for the launches after the hooks, where the roots no longer change.
__device__ __forceinline__ uint32_t find_root(const uint32_t* parent, uint32_t v) {
  uint32_t p = parent_of(parent, v);
  // terminates: p < v whenever the loop runs on (parent[x] <= x), so v strictly decreases and is >= 0
  while (p != v) {
    v = p;
    p = parent_of(parent, v);
  }
  return v;
}

// Join the components of a and b: the larger of the two roots goes under the smaller.
__device__ __forceinline__ void hook(uint32_t* parent, uint32_t a, uint32_t b) {
  // terminates: hi strictly decreases from one round to the next.  A round that runs on continues from (old, lo), both < hi, and
  // the roots found above them are <= them; hi >= 0.  No round waits for anybody: a lost race is answered by walking on.
  for (;;) {
    a = find_halving(parent, a);
    b = find_halving(parent, b);
    if (a == b) return;   // (stale reads included: both walks ended on one vertex, an ancestor of both)
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = atomicMin(parent + hi, lo);
    if (old == hi) return;   // hi was a root until this very atomic: it hangs under lo now
    // Lost the race: hi had been hooked under old < hi meanwhile.  The atomicMin has left min(old, lo) in parent[hi]; whichever
    // of the two it is, joining old and lo joins all three -- re-find from there.
    a = old;
    b = lo;
  }
}

}  // namespace r3d_uf
