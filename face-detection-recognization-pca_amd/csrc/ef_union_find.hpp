// Bounded lock-free union-find on the device, shared by the rectangle grouping (ef_haar_group.hip)
// and the gallery clustering (ef_cluster.hip).  parent[x] == x marks a root.  A link always goes
// from a root to a node that `less` orders before it, so the forest is acyclic by construction and
// a chain has at most n - 1 links.
// Termination: every chain walk is cut at n steps and every union at 2 n + 2 attempts (a failed
// compare-and-swap means another thread linked that root, and the next attempt starts from
// strictly smaller roots).  A walk that reaches its bound gives up and says so; nothing waits for
// another workgroup.
#pragma once

#include <hip/hip_runtime.h>

namespace ef {

__device__ __forceinline__ int parent_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's chain, at most n links away, or -1 at the bound.  halve: shorten the chain
// on the way (a non-root never becomes a root again and any ancestor is a valid parent, so the
// store races with nothing that matters).
template <bool HALVE>
__device__ __forceinline__ int group_find(int* parent, int x, int n) {
  for (int s = 0; s <= n; ++s) {
    const int p = parent_load(parent + x);
    if (p == x) return x;
    if (HALVE) {
      const int gp = parent_load(parent + p);
      if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    x = p;
  }
  return -1;
}

// Join the sets of a and b: the root that `less(x, y)` (x before y, a strict order on the nodes)
// puts last is linked below the other.  False when a walk or the attempts reached their bound.
template <typename Less>
__device__ __forceinline__ bool group_union(int* parent, int a, int b, int n, const Less& less) {
  for (long long it = 0; it < 2ll * n + 2; ++it) {
    a = group_find<true>(parent, a, n);
    b = group_find<true>(parent, b, n);
    if (a < 0 || b < 0) return false;
    if (a == b) return true;
    const bool a_low = less(a, b);
    const int lo = a_low ? a : b, hi = a_low ? b : a;
    if (atomicCAS(parent + hi, hi, lo) == hi) return true;  // hi was still a root: linked below lo
    a = lo;
    b = hi;
  }
  return false;
}

}  // namespace ef
