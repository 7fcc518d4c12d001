// union_find.hpp -- the lock-free union-find in global memory behind pmn_mesh_components (meshops.hip: vertices joined by faces) and
// pmn_cloud_dbscan (cloud_cluster.hip: core points joined by pairs within eps).  parent[v] = v at first; a unite finds the two roots
// and, if they differ, compare-and-swaps the LARGER root's slot from itself to the smaller root; a failed swap means that slot is no
// root any more, and the value it returned (< the old root) is where the search goes on; a flatten launch then stores every slot's
// root.  The properties and why they hold: the comment at the top of meshops.hip (every stored value is <= its slot, so every walk
// descends and ends whatever it reads; the indices a unite holds fall with every retry; no lane ever waits for another lane: no lock,
// no flag, no spin).  A tree's root is the minimum of its set, so the flattened result is a function of the set of unions alone.
// All accesses of parent[] in a uniting kernel and in flatten are relaxed agent-scope atomics, integer only; flatten is a launch of
// its own and so sees everything the unions wrote.  The two kernels have internal linkage: every file that includes this launches its own.
#pragma once
#include "pmn_common.hpp"

#define MESH_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

namespace {

__global__ __launch_bounds__(256) void mesh_cc_init_kernel(int* parent, int nv) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < nv) parent[v] = v;
}

}  // namespace

// the root of v as far as this lane can see; halves the path on the way (a best-effort store of a smaller ancestor)
__device__ __forceinline__ int mesh_cc_find(int* parent, int v) {
    int p = __hip_atomic_load(parent + v, MESH_RLX_AGENT);
    while (p < v) {  // (p > v cannot be stored; read as a root, it would fail the swap below, never loop here)
        const int g = __hip_atomic_load(parent + p, MESH_RLX_AGENT);
        if (g < p) __hip_atomic_store(parent + v, g, MESH_RLX_AGENT);
        v = p;
        p = g;
    }
    return v;
}

__device__ __forceinline__ void mesh_cc_unite(int* parent, int a, int b) {
    while (true) {
        a = mesh_cc_find(parent, a);
        b = mesh_cc_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, MESH_RLX_AGENT)) return;
        if (!(seen < hi)) return;  // cannot happen (a slot only ever falls); a lane never retries without having descended
        a = seen;
        b = lo;
    }
}

namespace {

__global__ __launch_bounds__(256) void mesh_cc_flatten_kernel(int* parent, int nv) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    int r = v, p = __hip_atomic_load(parent + v, MESH_RLX_AGENT);
    while (p < r) {  // another lane may already have flattened a slot on the way: its value is the same root
        r = p;
        p = __hip_atomic_load(parent + r, MESH_RLX_AGENT);
    }
    __hip_atomic_store(parent + v, r, MESH_RLX_AGENT);
}

}  // namespace
