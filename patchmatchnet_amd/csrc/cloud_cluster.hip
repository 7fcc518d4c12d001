// cloud_cluster.hip -- density clustering of a point cloud, DBSCAN made order-free (cluster_cloud.py,
// pointcloud.cluster_dbscan; tests/dbscan_ref.py restates everything below in numpy and is the yardstick; the reference has no
// counterpart).  The cloud is its own query set over the grid of pointcloud.hip (sorted points, same_cloud semantics: point i IS grid
// point i); a pair's distance is sqrt(pc_dist2), the float64 value of the float32 coordinates, and "within eps" is sqrt(d2) <= eps on the
// rooted value, as pmn_radius_count decides it.
//
//   core     point i is CORE when the points within eps of it, itself included, number at least min_points: RadiusCount's count + 1.
//   link     the clusters are the connected components of the graph on the core points whose edges are the core pairs within eps.
//            parent[i] = i, then one lane per core point i walks its neighbourhood and unites i with every core j < i within eps (each
//            edge is seen from both ends; the higher end makes the union), then flatten: parent[i] = the smallest sorted index of i's
//            component.  A point that is not core keeps parent[i] = i.
//   border   a point that is not core takes the cluster of the core point within eps that is least in (d2, ORIGINAL index) order:
//            label[i] = parent[that point], or -1 (noise) when there is none.  A core point's label is its own parent.
//            The original index (perm) breaks ties because the order of the sorted points inside a cell is not a function of the cloud.
//
// The result -- core flags, the partition, the noise set -- is a function of (points, eps, min_points): the core rule and the border rule
// are per point, the components are a property of a graph, and the union-find (union_find.hpp) returns a set's minimum whatever the
// interleaving.  Only the NAMES of the clusters (smallest sorted index) depend on the grid; the caller replaces them by size ranks.
//
// Launch shape: one lane per point, one-wave workgroups, lanes in cell order, for pointcloud.hip's reasons (the lanes of a wave walk the
// same cells; a far point holds up 63 neighbours, not 255).
//
// Termination of the link launch.  The unions happen inside a divergent walk, and the lanes of a wave do not progress independently: a
// lane that waited for a store of another lane of its own wave would wait for ever.  No lane here waits for anything.  mesh_cc_find
// descends strictly (every value ever stored in slot v is <= v, and < v once v is no root), so it ends after at most v steps whatever
// stale value it reads; mesh_cc_unite retries only after a failed compare-and-swap, which returned an index below the root it held, so
// the indices it holds fall with every retry and it ends after finitely many whatever the other lanes do or do not do meanwhile -- also
// when they never run again.  There is no lock, no flag and no spin: a lane's loop bounds depend on values that only fall, never on a
// value that another lane has yet to write.  The walk itself is pc_walk's, bounded by the grid.  A unite returns only when both ends had
// one root or its own swap joined them, and links are never removed, so after the launch the trees are the components.
// Integer relaxed agent-scope atomics only (loads that bypass the per-CU L1, a 32-bit compare-and-swap, 32-bit stores); core[] and, in
// the border launch, parent[] were written by EARLIER launches, so plain loads read them.  No floating-point atomics, no LDS, no per-lane
// array (hence no scratch).
#include "pc_grid.hpp"
#include "union_find.hpp"

struct ClusterArgs {
    GridArgs g;
    double eps;
    long long min_points;
    const int* orig;        // [n] original index of every sorted point (the grid's perm)
    unsigned char* core;    // [n]
    int* parent;            // [n]
    int* label;             // [n]
};

// ---- core flags -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cluster_core_kernel(ClusterArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.g.n) return;
    const double qx = (double)a.g.xyz[(size_t)i * 3], qy = (double)a.g.xyz[(size_t)i * 3 + 1], qz = (double)a.g.xyz[(size_t)i * 3 + 2];
    RadiusCount b;  // pmn_radius_count's accumulator: the one count in the tree
    b.init(a.eps, i);
    pc_walk(a.g, qx, qy, qz, b);
    a.core[i] = ((long long)b.count + 1 >= a.min_points) ? 1 : 0;
}

// ---- link -----------------------------------------------------------------------------------------------------------------------------
// RadiusCount's constant bound; a candidate is united with the walking point instead of being counted.
struct CoreLink {
    double radius, bound;
    int self;
    const unsigned char* core;
    int* parent;
    __device__ __forceinline__ void init(double r, int self_, const unsigned char* core_, int* parent_) {
#pragma clang fp contract(off)
        radius = r;
        bound = r * r * (1.0 + 1.0 / 1099511627776.0) + 2.2250738585072014e-308;
        self = self_;
        core = core_;
        parent = parent_;
    }
    __device__ __forceinline__ bool beyond(double g2) const { return g2 > bound; }
    __device__ __forceinline__ void offer(double c, int j) {
        if (j < self && core[j] && sqrt(c) <= radius) mesh_cc_unite(parent, self, j);
    }
};

__global__ __launch_bounds__(64) void cluster_link_kernel(ClusterArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.g.n || !a.core[i]) return;
    const double qx = (double)a.g.xyz[(size_t)i * 3], qy = (double)a.g.xyz[(size_t)i * 3 + 1], qz = (double)a.g.xyz[(size_t)i * 3 + 2];
    CoreLink b;
    b.init(a.eps, i, a.core, a.parent);
    pc_walk(a.g, qx, qy, qz, b);
}

// ---- border ---------------------------------------------------------------------------------------------------------------------------
// The nearest core point within eps, least (d2, original index).  Until a candidate is held the bound is RadiusCount's; with one, a
// region is also skipped when its lower bound is strictly above the best d2 (an equal d2 with a lower original index may still come).
struct NearestCore {
    double radius, bound, d2;
    int idx, oidx;  // sorted and original index of the best, idx = -1: none
    const unsigned char* core;
    const int* orig;
    __device__ __forceinline__ void init(double r, const unsigned char* core_, const int* orig_) {
#pragma clang fp contract(off)
        radius = r;
        bound = r * r * (1.0 + 1.0 / 1099511627776.0) + 2.2250738585072014e-308;
        d2 = 0.0;
        idx = -1;
        oidx = 0;
        core = core_;
        orig = orig_;
    }
    __device__ __forceinline__ bool beyond(double g2) const { return g2 > bound || (idx >= 0 && g2 > d2); }
    __device__ __forceinline__ void offer(double c, int j) {
        if (!core[j] || (idx >= 0 && c > d2) || !(sqrt(c) <= radius)) return;
        const int o = orig[j];
        if (idx < 0 || c < d2 || o < oidx) {  // (here c <= d2 when a candidate is held)
            d2 = c;
            idx = j;
            oidx = o;
        }
    }
};

__global__ __launch_bounds__(64) void cluster_border_kernel(ClusterArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.g.n) return;
    if (a.core[i]) {
        a.label[i] = a.parent[i];
        return;
    }
    const double qx = (double)a.g.xyz[(size_t)i * 3], qy = (double)a.g.xyz[(size_t)i * 3 + 1], qz = (double)a.g.xyz[(size_t)i * 3 + 2];
    NearestCore b;  // the point itself is not core, so it is never a candidate
    b.init(a.eps, a.core, a.orig);
    pc_walk(a.g, qx, qy, qz, b);
    a.label[i] = b.idx >= 0 ? a.parent[b.idx] : -1;
}

static int cluster_args(ClusterArgs& a, const float* xyz, const long long* keys, long long n, const double* origin_host, double cell,
                        const int* dims_host, double eps) {
    const int rc = grid_args(a.g, xyz, keys, n, origin_host, cell, dims_host);
    if (rc != PMN_OK) return rc;
    if (n > 2147483647LL - 255) return PMN_ERR_ARG;
    if (!(eps >= 0.0) || !std::isfinite(eps) || !std::isfinite(eps * eps)) return PMN_ERR_ARG;
    a.eps = eps;
    a.min_points = 0;
    a.orig = nullptr;
    a.core = nullptr;
    a.parent = nullptr;
    a.label = nullptr;
    return PMN_OK;
}

extern "C" int pmn_cloud_core(const float* xyz, const long long* keys, long long n, const double* origin_host, double cell,
                              const int* dims_host, double eps, long long min_points, unsigned char* core, void* stream) {
    ClusterArgs a;
    const int rc = cluster_args(a, xyz, keys, n, origin_host, cell, dims_host, eps);
    if (rc != PMN_OK) return rc;
    if (!core || min_points < 1) return PMN_ERR_ARG;
    a.min_points = min_points;
    a.core = core;
    PMN_LAUNCH(cluster_core_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_cloud_dbscan(const float* xyz, const long long* keys, long long n, const double* origin_host, double cell,
                                const int* dims_host, double eps, const unsigned char* core, const int* orig, int* parent, int* label,
                                void* stream) {
    ClusterArgs a;
    const int rc = cluster_args(a, xyz, keys, n, origin_host, cell, dims_host, eps);
    if (rc != PMN_OK) return rc;
    if (!core || !parent || ((label != nullptr) != (orig != nullptr))) return PMN_ERR_ARG;
    a.core = const_cast<unsigned char*>(core);
    a.orig = orig;
    a.parent = parent;
    a.label = label;
    const dim3 wgrid((unsigned)((n + 63) / 64)), vgrid((unsigned)((n + 255) / 256));
    PMN_LAUNCH(mesh_cc_init_kernel, vgrid, dim3(256), 0, (hipStream_t)stream, parent, (int)n);
    PMN_LAUNCH(cluster_link_kernel, wgrid, dim3(64), 0, (hipStream_t)stream, a);
    PMN_LAUNCH(mesh_cc_flatten_kernel, vgrid, dim3(256), 0, (hipStream_t)stream, parent, (int)n);
    if (label) PMN_LAUNCH(cluster_border_kernel, wgrid, dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
