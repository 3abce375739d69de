// The lock-free union-find of the mesh kernels, the one place for it: tn_mesh_components.hip unites the vertices of a triangle,
// tn_mesh_patches.hip the two faces of an edge.  `parent` is an int array over the nodes, parent[x] = x at the start.
//
// THE UNION-FIND.  Invariant I: parent[x] <= x, and parent[x] is only ever replaced by an ANCESTOR of x (a node reachable from x by
// following parent).  x is a root iff parent[x] == x.  Two kinds of writes exist:
//   * hook: atomicCAS(&parent[hi], hi, lo) with lo < hi.  It can only succeed while hi is a root, and then makes it a non-root
//     below lo.  So only roots are ever CAS-written, and a node that has stopped being a root never becomes one again: every later
//     CAS on it compares against hi and fails, and halving (below) never writes x into parent[x].
//   * halving, inside find: parent[x] <- parent[parent[x]], an atomic store to a node that was SEEN as a non-root (hence is one
//     for good), of a value that was an ancestor of x when it was read.  Ancestors stay ancestors: every write replaces a parent by
//     one of ITS ancestors, which keeps the old parent's chain below the new one.  Two racing halvings may leave the farther or the
//     nearer ancestor; both keep I.  Without halving a triangle strip hooks into a chain of depth O(V) and the walks are quadratic.
// Since parent[x] < x for a non-root, the forest has no cycle and every walk ends.  unite(a, b): find both roots; while they differ,
// CAS the higher under the lower; a failed CAS returns the value it found, which is strictly smaller than hi (hi was no longer a
// root: parent[hi] < hi), and the loop continues from find of that value and lo, both below hi — the larger of the pair strictly
// decreases, so the loop ends after at most V rounds whatever the other threads do; nobody waits for anybody.
// A STALE READ IS HARMLESS: every value parent[x] ever held is an ancestor of x for good, so a walk through old values is only
// longer, and it ends at a node r that was a root of x's tree when read.  If r has since been hooked, either the two walks still
// met in the same r (then a and b are connected: both have r as an ancestor) or the CAS, which acts on the true value, fails
// and hands back the fresh one.  A CAS that succeeds with a stale `lo` that is no longer a root links hi below a non-root: lo's
// tree then contains hi's, which is all that is asked.  parent is read in the hook kernels with relaxed agent-scope atomic loads
// (served by the memory side, not by a CU's cache that no other CU's store ever refreshes), so "stale" is a matter of microseconds.
// After a hook kernel every united pair shares a root; roots only merge, so they still do at its end, and no two classes were ever
// joined without a unite.  The root is the smallest index of its tree (I).  The kernel boundary is the only ordering a flatten
// kernel needs; it reads parent with plain loads while other threads already store roots into it, which by the same argument (a
// root is an ancestor) changes no result.
#pragma once
#include "tn_device.h"

namespace tn {

__device__ __forceinline__ int load_parent(const int *parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x as this thread sees it, halving the path on the way
__device__ __forceinline__ int find_root(int *parent, int x) {
    int p = load_parent(parent, x);
    while (p != x) {
        const int g = load_parent(parent, p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // x is a non-root, g an ancestor
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void unite(int *parent, int a, int b) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    while (a != b) {
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int found = atomicCAS(parent + hi, hi, lo);
        if (found == hi) return;
        a = find_root(parent, found);  // found < hi
        b = lo;                        // (a root when read; a stale one is still in its tree)
    }
}

}  // namespace tn
