// The lock-free union-find of the clustering kernels, shared by towers.hip (K8) and dbscan.hip (K10): one discipline, one
// text.  parent[] holds int32 indices, parent[v] == v for a root (ECL-CC).
//   - Every access is relaxed and agent-scope.  A stale value is an earlier parent, which is still an ancestor.
//   - Only a compare-and-swap that finds a root unchanged (it expects the root itself) ever hooks it.
//   - The larger root goes under the smaller: a parent is always a smaller index, a component's root is its smallest
//     index, and every loop is bounded by the data.
//   - A non-root's parent is only ever replaced by another of its ancestors -- always smaller than the node, though a
//     racing halving store may put back a nearer one, never a non-ancestor.
//   - No workgroup waits for another anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

__device__ __forceinline__ int32_t uf_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void uf_store(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of v, halving the path on the way (v strictly decreases: bounded)
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t v) {
    for (;;) {
        const int32_t a = uf_load(parent + v);
        if (a == v) return v;
        const int32_t g = uf_load(parent + a);
        if (g == a) return a;
        uf_store(parent + v, g);
        v = g;
    }
}

__device__ __forceinline__ int32_t uf_find_readonly(const int32_t* parent, int32_t v) {
    for (;;) {
        const int32_t a = uf_load(parent + v);
        if (a == v) return v;
        v = a;
    }
}

// unites the sets of a and b, returns the root seen last.  A failed compare-and-swap means a is no root any more: the
// value it returns is a's parent, a smaller index.
__device__ __forceinline__ int32_t uf_unite(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = atomicCAS(parent + a, a, b);   // the larger root goes under the smaller
        if (old == a) return b;
        a = old;
    }
}

}  // namespace
