// pointcloud.hip -- the two searches behind the DTU score of a fused point cloud (reference evaluations/dtu/reducePts_haa.m and
// MaxDistCP.m, which use MATLAB's KDTreeSearcher on the CPU): nearest-neighbour distance and one round of the greedy reduction; and
// the two searches behind cloud cleaning (clean_cloud.py): the k nearest neighbours and the number of points within a radius.
//
// Spatial index (built by the caller, patchmatchnet_amd/pointcloud.py): a uniform grid over SORTED points.  A point's cell is
// c = floor((double(p) - origin) / cell) per axis, 0 <= c < dims, its key (c.z * dims.y + c.y) * dims.x + c.x (< 2^63); the points
// and their keys are stored in ascending key order.  x is the fastest axis of the key, so the points of a ROW of cells
// [x0, x1] x {y} x {z} are one contiguous range of the sorted array, found with two binary searches over the keys: there is no
// cell table, and a grid of any extent (cells much smaller than the point spacing, far outliers) costs no memory.
//
// Distances are the float64 value sqrt(dx*dx + dy*dy + dz*dz) of the float32 coordinates widened to float64, products and sums in
// x, y, z order without contraction (#pragma clang fp contract(off)): the bits numpy's float64 gives.  Every decision (nearest,
// "within dst") is taken on that value or its square; nothing is evaluated in fp32.  (The sum of squares is compared before the
// root where only the ORDER matters: sqrt is monotone, so the nearest by square is a nearest by distance; "within dst" is decided
// on the rooted value itself, because sqrt(s) <= dst and s <= dst * dst differ in the last bit.)
//
// The bounds that END a search are geometric (a point of cell c lies in [origin + c * cell, origin + (c + 1) * cell)), while a
// point's cell comes from a rounded division; every such bound is therefore shrunk by PMN_PC_SLACK (relative 2^-20 of a cell) so
// that a point the rounding put one cell off is still visited.  Visiting more never changes a result.
#include "pc_grid.hpp"
#include "pc_jacobi.hpp"

// ---- pmn_nn_distance --------------------------------------------------------------------------------------------------------------
// One lane per query, queries taken in the caller's order (the sorted order of the queries' own cells): the 64 lanes of a wave
// then sit in the same or adjacent cells, their binary searches read the same keys and their candidate ranges overlap, so the loads
// of a wave are broadcasts or L2 hits.  Workgroups are ONE wave: a far query (an outlier walks shells out to max_dist) holds up 63
// neighbours, not 255, and the hardware schedules the many short waves around it.
struct NnArgs {
    GridArgs g;
    QueryArgs q;         // same_cloud is 0: the nearest point may be the query's twin
    double max_dist;
    double* dist;        // [n_from], indexed as query
    int* index;          // [n_from] or null
};

__global__ __launch_bounds__(64) void nn_distance_kernel(NnArgs a) {
#pragma clang fp contract(off)
    PC_QUERY_OR_RETURN(a.q);
    const NnBest b = nn_search(a.g, qx, qy, qz, a.max_dist);  // pc_grid.hpp: the shell walk, shared with registration.hip
    a.dist[q] = b.idx < 0 ? a.max_dist : sqrt(b.d2);
    if (a.index) a.index[q] = b.idx;
}

// ---- pmn_reduce_round ---------------------------------------------------------------------------------------------------------------
// state: 0 undecided, 1 kept, 2 removed.  ONE array, updated in place, and the only transitions are 0 -> 1 and 0 -> 2.  A point is
// decided from the states of its lower-ranked neighbours only: removed as soon as one of them is kept, kept once all of them are
// removed.  Both conclusions rest on FINAL states (by induction over the rank: 1 and 2 are never overwritten), so whether a lane
// reads a neighbour's byte before or after another lane of the same round decided it changes only WHEN this point is decided, never
// WHAT it becomes: a byte load returns 0 (decide later) or the neighbour's final state.  The fixed point is the sequential greedy
// set of the visiting order, whatever the schedule; reading fresh states merely saves rounds against a double-buffered scheme.
struct ReduceArgs {
    GridArgs g;
    const int* rank;        // [n] position in the visiting order, of the sorted points
    unsigned char* state;   // [n]
    unsigned int* counter;  // += points still undecided after this round
    double dst;
    int reach;              // cells a neighbour within dst can be away along an axis
};

__global__ __launch_bounds__(256) void reduce_round_kernel(ReduceArgs a) {
#pragma clang fp contract(off)
    const GridArgs& g = a.g;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int undecided = 0;
    if (i < g.n && a.state[i] == 0) {
        const double qx = (double)g.xyz[(size_t)i * 3], qy = (double)g.xyz[(size_t)i * 3 + 1], qz = (double)g.xyz[(size_t)i * 3 + 2];
        const long long key = g.keys[i];
        const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
        const int cx = (int)(key % nx), cy = (int)((key / nx) % ny), cz = (int)(key / ((long long)nx * ny));
        const int my = a.rank[i];
        const int R = a.reach;
        const int x0 = max(cx - R, 0), x1 = min(cx + R, nx - 1);
        bool removed = false, blocked = false;
        for (int z = max(cz - R, 0); z <= min(cz + R, nz - 1) && !removed; ++z) {
            const double gz = pc_gap(qz, g.origin[2], g.cell, z, z);
            if (gz > a.dst) continue;
            for (int y = max(cy - R, 0); y <= min(cy + R, ny - 1) && !removed; ++y) {
                const double gy = pc_gap(qy, g.origin[1], g.cell, y, y);
                if (sqrt(gy * gy + gz * gz) > a.dst) continue;
                const long long base = ((long long)z * ny + y) * nx;
                const int i0 = pc_lower_bound(g.keys, 0, g.n, base + x0);
                if (i0 >= g.n || g.keys[i0] > base + x1) continue;
                const int i1 = pc_lower_bound(g.keys, i0 + 1, g.n, base + x1 + 1);
                for (int j = i0; j < i1; ++j) {
                    if (a.rank[j] >= my) continue;  // higher rank, or this point itself
                    const unsigned char s = a.state[j];
                    if (s == 2) continue;
                    if (sqrt(pc_dist2(g.xyz + (size_t)j * 3, qx, qy, qz)) > a.dst) continue;
                    if (s == 1) {
                        removed = true;
                        break;
                    }
                    blocked = true;
                }
            }
        }
        if (removed) a.state[i] = 2;
        else if (!blocked) a.state[i] = 1;
        else undecided = 1;
    }
    const int cnt = __popcll(__ballot(undecided));  // one atomic per wave
    if ((threadIdx.x & 63) == 0 && cnt > 0) atomicAdd(a.counter, (unsigned int)cnt);
}

// ---- pmn_knn_distance / pmn_radius_count ------------------------------------------------------------------------------------------
// The same walk with the k-best and the counting accumulator of pc_grid.hpp, launched as nn_distance_kernel is and for its reasons:
// one lane per query, one wave per workgroup, queries in cell order.  The k-best list is register-resident, so the kernel is
// specialised on its capacity (8 / 16 / 32, k rounded up): 3 VGPRs per slot, and a small k does not pay for 32 slots.
struct KnnArgs {
    GridArgs g;
    QueryArgs q;
    int k;
    double max_dist;
    double* d2;          // [n_from][k] or null
    int* index;          // [n_from][k] or null
    double* mean;        // [n_from] or null
};

template <int CAP>
__global__ __launch_bounds__(64) void knn_distance_kernel(KnnArgs a) {
#pragma clang fp contract(off)
    PC_QUERY_OR_RETURN(a.q);
    KBest<CAP> b;
    b.init(a.k, a.max_dist * a.max_dist, self);
    pc_walk(a.g, qx, qy, qz, b);
    const size_t row = (size_t)q * a.k;
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < CAP; ++s) {  // slot s is rank j = s - (CAP - k): static register, run-time address
        const int j = s - (CAP - a.k);
        if (j < 0) continue;
        sum += b.idx[s] < 0 ? a.max_dist : sqrt(b.d2[s]);  // smallest first
        if (a.d2) a.d2[row + j] = b.d2[s];
        if (a.index) a.index[row + j] = b.idx[s];
    }
    if (a.mean) a.mean[q] = sum / (double)a.k;
}

struct RadiusArgs {
    GridArgs g;
    QueryArgs q;
    double radius;
    int* count;  // [n_from]
};

__global__ __launch_bounds__(64) void radius_count_kernel(RadiusArgs a) {
#pragma clang fp contract(off)
    PC_QUERY_OR_RETURN(a.q);
    RadiusCount b;
    b.init(a.radius, self);
    pc_walk(a.g, qx, qy, qz, b);
    a.count[q] = b.count;
}

// ---- pmn_knn_normals ----------------------------------------------------------------------------------------------------------------
// knn_distance_kernel's walk with another epilogue: instead of writing the lists out (12 k n bytes) the lane that found them turns
// them into the covariance of the neighbourhood and that into its eigenvector of least variance (include/pmn_hip.h states every
// operation; tests/cloud_normals_ref.py repeats them in numpy).  The list is read through static slot indices only, as everywhere
// else, and every entry of the 3 x 3 matrix and of the rotation is a named scalar: nothing here may become a per-lane array.

struct NormalArgs {
    GridArgs g;
    QueryArgs q;
    int k;
    double max_dist;
    const double* viewpoints;  // [n_viewpoints][3] or null
    int n_viewpoints;
    double line_ratio;
    float* normal;       // [n_from][3]
    double* variation;   // [n_from] or null
    int* count;          // [n_from] or null
};

// pc_moments, pc_eigen3 and the canonical sign: pc_jacobi.hpp, shared with cloud_mls.hip

template <int CAP>
__global__ __launch_bounds__(64) void knn_normals_kernel(NormalArgs a) {
#pragma clang fp contract(off)
    PC_QUERY_OR_RETURN(a.q);
    KBest<CAP> b;
    b.init(a.k, a.max_dist * a.max_dist, self);
    pc_walk(a.g, qx, qy, qz, b);
    // the moments of the deltas, neighbours in rank order; the query is the zero delta and counts in m alone
    double W = 0.0, sx, sy, sz, mxx, mxy, mxz, myy, myz, mzz;
    const int used = pc_moments<false>(b, a.g.xyz, qx, qy, qz, 0.0, W, sx, sy, sz, mxx, mxy, mxz, myy, myz, mzz);
    const double m = (double)(used + 1);
    double a00 = mxx - (sx * sx) / m, a01 = mxy - (sx * sy) / m, a02 = mxz - (sx * sz) / m;
    double a11 = myy - (sy * sy) / m, a12 = myz - (sy * sz) / m, a22 = mzz - (sz * sz) / m;
    double v00, v01, v02, v10, v11, v12, v20, v21, v22;  // v[row][column]
    pc_eigen3(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    const double l0 = a00, l1 = a11, l2 = a22;
    double nx = 0.0, ny = 0.0, nz = 0.0, var = 0.0;
    if (used >= 2 && l2 != 0.0 && l1 > a.line_ratio * l2) {
        nx = v00;
        ny = v10;
        nz = v20;
        var = l0 / (l0 + l1 + l2);
        bool flip = pc_canonical_flip(nx, ny, nz);
        if (a.n_viewpoints > 0) {  // towards the nearest viewpoint, the lowest index among equals
            double best = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
            bool have = false;
            for (int v = 0; v < a.n_viewpoints; ++v) {  // wave-uniform addresses
                const double dx = a.viewpoints[(size_t)v * 3] - qx, dy = a.viewpoints[(size_t)v * 3 + 1] - qy,
                             dz = a.viewpoints[(size_t)v * 3 + 2] - qz;
                const double d = dx * dx + dy * dy + dz * dz;
                if (!have || d < best) {
                    have = true;
                    best = d;
                    bx = dx;
                    by = dy;
                    bz = dz;
                }
            }
            const double cnx = flip ? -nx : nx, cny = flip ? -ny : ny, cnz = flip ? -nz : nz;
            const double dot = cnx * bx + cny * by + cnz * bz;
            flip = flip != (dot < 0.0);
        }
        pc_flip(flip, nx, ny, nz);
    }
    a.normal[(size_t)q * 3] = (float)nx;
    a.normal[(size_t)q * 3 + 1] = (float)ny;
    a.normal[(size_t)q * 3 + 2] = (float)nz;
    if (a.variation) a.variation[q] = var;
    if (a.count) a.count[q] = used;
}

extern "C" int pmn_knn_normals(const float* to_xyz, const long long* to_keys, long long n_to, const double* origin_host, double cell,
                               const int* dims_host, const float* query, const int* order, long long n_from, int k, double max_dist,
                               int same_cloud, const double* viewpoints, int n_viewpoints, double line_ratio, float* normal,
                               double* variation, int* count, void* stream) {
    NormalArgs a;
    const int rc = grid_args(a.g, to_xyz, to_keys, n_to, origin_host, cell, dims_host);
    if (rc != PMN_OK) return rc;
    if (query_args(a.q, query, order, n_from, same_cloud, n_to) != PMN_OK) return PMN_ERR_ARG;
    if (!normal || !pc_k_ok(k) || !pc_reach_ok(max_dist)) return PMN_ERR_ARG;
    if (n_viewpoints < 0 || n_viewpoints > PMN_NORMAL_MAX_VIEWPOINTS || (n_viewpoints > 0 && !viewpoints)) return PMN_ERR_ARG;
    if (!(line_ratio >= 0.0) || !std::isfinite(line_ratio)) return PMN_ERR_ARG;
    a.k = k;
    a.max_dist = max_dist;
    a.viewpoints = viewpoints;
    a.n_viewpoints = n_viewpoints;
    a.line_ratio = line_ratio;
    a.normal = normal;
    a.variation = variation;
    a.count = count;
    PMN_LAUNCH_KBEST(k, knn_normals_kernel<CAP>, dim3((unsigned)((n_from + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_knn_distance(const float* to_xyz, const long long* to_keys, long long n_to, const double* origin_host, double cell,
                                const int* dims_host, const float* query, const int* order, long long n_from, int k, double max_dist,
                                int same_cloud, double* d2, int* index, double* mean, void* stream) {
    KnnArgs a;
    const int rc = grid_args(a.g, to_xyz, to_keys, n_to, origin_host, cell, dims_host);
    if (rc != PMN_OK) return rc;
    if (query_args(a.q, query, order, n_from, same_cloud, n_to) != PMN_OK) return PMN_ERR_ARG;
    if (!pc_k_ok(k) || !pc_reach_ok(max_dist)) return PMN_ERR_ARG;
    a.k = k;
    a.max_dist = max_dist;
    a.d2 = d2;
    a.index = index;
    a.mean = mean;
    PMN_LAUNCH_KBEST(k, knn_distance_kernel<CAP>, dim3((unsigned)((n_from + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_radius_count(const float* to_xyz, const long long* to_keys, long long n_to, const double* origin_host, double cell,
                                const int* dims_host, const float* query, const int* order, long long n_from, double radius,
                                int same_cloud, int* count, void* stream) {
    RadiusArgs a;
    const int rc = grid_args(a.g, to_xyz, to_keys, n_to, origin_host, cell, dims_host);
    if (rc != PMN_OK) return rc;
    if (query_args(a.q, query, order, n_from, same_cloud, n_to) != PMN_OK || !count) return PMN_ERR_ARG;
    if (!(radius >= 0.0) || !std::isfinite(radius) || !std::isfinite(radius * radius)) return PMN_ERR_ARG;  // 0 is a radius
    a.radius = radius;
    a.count = count;
    PMN_LAUNCH(radius_count_kernel, dim3((unsigned)((n_from + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_nn_distance(const float* to_xyz, const long long* to_keys, long long n_to, const double* origin_host, double cell,
                               const int* dims_host, const float* query, const int* order, long long n_from, double max_dist,
                               double* dist, int* index, void* stream) {
    NnArgs a;
    const int rc = grid_args(a.g, to_xyz, to_keys, n_to, origin_host, cell, dims_host);
    if (rc != PMN_OK) return rc;
    if (query_args(a.q, query, order, n_from, 0, n_to) != PMN_OK || !dist) return PMN_ERR_ARG;
    if (!(max_dist > 0.0) || !std::isfinite(max_dist)) return PMN_ERR_ARG;  // the square is only ever a bound here and may be infinite
    a.max_dist = max_dist;
    a.dist = dist;
    a.index = index;
    PMN_LAUNCH(nn_distance_kernel, dim3((unsigned)((n_from + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_reduce_round(const float* xyz, const long long* keys, long long n, const double* origin_host, double cell,
                                const int* dims_host, double dst, const int* rank, unsigned char* state, unsigned int* counter,
                                void* stream) {
    ReduceArgs a;
    const int rc = grid_args(a.g, xyz, keys, n, origin_host, cell, dims_host);
    if (rc != PMN_OK) return rc;
    if (!rank || !state || !counter || !(dst >= 0.0) || !std::isfinite(dst)) return PMN_ERR_ARG;
    const double reach = floor(dst / cell * (1.0 + 1e-9)) + 1.0;
    if (reach > 1024.0) return PMN_ERR_SHAPE;  // dst far above the cell: the caller wants a coarser grid
    a.rank = rank;
    a.state = state;
    a.counter = counter;
    a.dst = dst;
    a.reach = (int)reach;
    PMN_LAUNCH(reduce_round_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
