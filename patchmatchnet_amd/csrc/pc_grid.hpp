// pc_grid.hpp -- the uniform grid over sorted points and the shell walk over it (nearest, k nearest, count within a radius), shared by
// pointcloud.hip (the DTU score, cloud cleaning) and registration.hip (ICP).  Layout, arithmetic and the slack of the bounds: the comment at the top of pointcloud.hip.
#pragma once
#include <cmath>

#include "pmn_common.hpp"

#define PMN_PC_SLACK (1.0 / 1048576.0)

struct GridArgs {
    const float* xyz;        // [n][3] grid-sorted
    const long long* keys;   // [n] ascending
    int n;
    int dims[3];
    double origin[3];
    double cell;
};

// first index in [lo, n) whose key is >= k
__device__ __forceinline__ int pc_lower_bound(const long long* __restrict__ keys, int lo, int n, long long k) {
    int hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// cell coordinate of a position along one axis, clamped to +-2^30 (a query may lie anywhere)
__device__ __forceinline__ int pc_cell(double p, double origin, double cell) {
    double c = floor((p - origin) / cell);
    c = c < -1073741824.0 ? -1073741824.0 : c;
    c = c > 1073741824.0 ? 1073741824.0 : c;
    return (int)c;
}

// distance from p to the slab of cells [c0, c1] along one axis (0 inside), shrunk by the slack
__device__ __forceinline__ double pc_gap(double p, double origin, double cell, int c0, int c1) {
    const double lo = origin + (double)c0 * cell, hi = origin + ((double)c1 + 1.0) * cell;
    double g = p < lo ? lo - p : (p > hi ? p - hi : 0.0);
    g -= cell * PMN_PC_SLACK;
    return g > 0.0 ? g : 0.0;
}

__device__ __forceinline__ double pc_dist2(const float* __restrict__ p, double qx, double qy, double qz) {
#pragma clang fp contract(off)
    const double dx = (double)p[0] - qx, dy = (double)p[1] - qy, dz = (double)p[2] - qz;
    return dx * dx + dy * dy + dz * dz;
}

// ---- the shell walk: ONE rule over an accumulator ------------------------------------------------------------------------------------
// An accumulator is offered (d2, sorted index) for every candidate the walk visits and tells the walk what can no longer matter:
//   bool beyond(double g2) const   true when no candidate at squared distance >= g2 can change the result;
//   void offer(double d2, int i)   one candidate.
// g2 is always a LOWER bound (a gap to a cell, a row or a shell, shrunk by the slack), so beyond() may only err towards false.
// The nearest neighbour (NnBest), the k nearest (KBest) and the count within a radius (RadiusCount) are its three instances.

struct NnBest {
    double d2;
    int idx;
    __device__ __forceinline__ bool beyond(double g2) const { return g2 >= d2; }
    __device__ __forceinline__ void offer(double c, int i) {
        if (c < d2) {
            d2 = c;
            idx = i;
        }
    }
};

// the points of cells [x0, x1] x {y} x {z} (already inside the grid)
template <class Acc>
__device__ __forceinline__ void pc_scan_row(const GridArgs& g, int x0, int x1, int y, int z, double qx, double qy, double qz, Acc& b) {
    const long long base = ((long long)z * g.dims[1] + y) * g.dims[0];
    const int i0 = pc_lower_bound(g.keys, 0, g.n, base + x0);
    if (i0 >= g.n || g.keys[i0] > base + x1) return;
    const int i1 = pc_lower_bound(g.keys, i0 + 1, g.n, base + x1 + 1);
    for (int i = i0; i < i1; ++i) b.offer(pc_dist2(g.xyz + (size_t)i * 3, qx, qy, qz), i);
}

// The walk of a query at (qx, qy, qz), any position: the query's cell, then shells of growing Chebyshev radius, until everything not
// yet visited is beyond the accumulator's bound (the distance to the nearest face of the next shell) or the grid is exhausted.
template <class Acc>
__device__ __forceinline__ void pc_walk(const GridArgs& g, double qx, double qy, double qz, Acc& b) {
#pragma clang fp contract(off)
    const int cx = pc_cell(qx, g.origin[0], g.cell), cy = pc_cell(qy, g.origin[1], g.cell), cz = pc_cell(qz, g.origin[2], g.cell);
    const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
    // a query outside the grid starts at the first shell that touches it
    int r = 0;
    r = max(r, max(-cx, cx - (nx - 1)));
    r = max(r, max(-cy, cy - (ny - 1)));
    r = max(r, max(-cz, cz - (nz - 1)));
    // position of the query inside its cell: the distance to the nearest face of shell r + 1 is r * cell + face
    const double fx = qx - (g.origin[0] + (double)cx * g.cell), fy = qy - (g.origin[1] + (double)cy * g.cell),
                 fz = qz - (g.origin[2] + (double)cz * g.cell);
    double face = fmin(fmin(fmin(fx, g.cell - fx), fmin(fy, g.cell - fy)), fmin(fz, g.cell - fz));
    face = fmax(face - g.cell * PMN_PC_SLACK, 0.0);
    const int rmax = max(max(max(cx, nx - 1 - cx), max(cy, ny - 1 - cy)), max(cz, nz - 1 - cz));  // last shell that touches the grid
    for (; r <= rmax; ++r) {
        // everything not yet visited is at least (r - 1) * cell + face away
        if (r > 0) {
            const double reach = (double)(r - 1) * g.cell + face;
            if (b.beyond(reach * reach)) break;
        }
        const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
        for (int z = z0; z <= z1; ++z) {
            const double gz = pc_gap(qz, g.origin[2], g.cell, z, z);
            if (b.beyond(gz * gz)) continue;
            const bool zface = z == cz - r || z == cz + r;
            for (int y = y0; y <= y1; ++y) {
                const double gy = pc_gap(qy, g.origin[1], g.cell, y, y);
                const double gyz = gy * gy + gz * gz;
                if (b.beyond(gyz)) continue;
                if (zface || y == cy - r || y == cy + r) {
                    if (x0 <= x1) pc_scan_row(g, x0, x1, y, z, qx, qy, qz, b);
                } else {  // interior (y, z) of the shell: only its two end cells are new
                    if (cx - r >= 0 && cx - r < nx) {
                        const double gx = pc_gap(qx, g.origin[0], g.cell, cx - r, cx - r);
                        if (!b.beyond(gx * gx + gyz)) pc_scan_row(g, cx - r, cx - r, y, z, qx, qy, qz, b);
                    }
                    if (cx + r >= 0 && cx + r < nx) {
                        const double gx = pc_gap(qx, g.origin[0], g.cell, cx + r, cx + r);
                        if (!b.beyond(gx * gx + gyz)) pc_scan_row(g, cx + r, cx + r, y, z, qx, qy, qz, b);
                    }
                }
            }
        }
    }
}

// The nearest grid point of a query: the walk's one-best instance.  The first candidate met wins among equals (the bound is then
// ">= best").  idx = -1 and d2 = max_dist * max_dist where no point is nearer than max_dist.
__device__ __forceinline__ NnBest nn_search(const GridArgs& g, double qx, double qy, double qz, double max_dist) {
#pragma clang fp contract(off)
    NnBest b;
    b.d2 = max_dist * max_dist;  // a point at exactly max_dist or beyond never wins: the result is then max_dist itself
    b.idx = -1;
    pc_walk(g, qx, qy, qz, b);
    return b;
}

// The K nearest, K <= CAP, in registers: CAP (d2, idx) pairs kept in ascending (d2, idx) order and touched ONLY through indices the
// compiler knows (every loop below is fully unrolled), because a per-lane array indexed by a run-time value lives in scratch memory.
// The list is right-aligned: slots [0, CAP - k) hold a sentinel below every candidate (d2 = -1) that never moves, slots
// [CAP - k, CAP) the k best so far, so that the k-th best -- the bound -- is always slot CAP - 1 whatever k is.  Empty slots hold
// the cap (max_dist^2, index -1); a candidate enters only with d2 < cap.  Order is (d2, index) lexicographic: among equal squares
// the lower sorted index wins whatever the visiting order, hence the bound is "> k-th best" (an equal candidate in a cell not yet
// visited may still displace a higher index) once the list is full, and ">= cap" before.
template <int CAP>
struct KBest {
    double d2[CAP];
    int idx[CAP];
    int self;  // sorted index never reported (the query itself under same_cloud), or -1

    __device__ __forceinline__ void init(int k, double cap, int self_) {
        self = self_;
#pragma unroll
        for (int s = 0; s < CAP; ++s) {
            const bool live = s >= CAP - k;
            d2[s] = live ? cap : -1.0;
            idx[s] = live ? -1 : -2;
        }
    }
    __device__ __forceinline__ bool beyond(double g2) const { return g2 > d2[CAP - 1] || (idx[CAP - 1] < 0 && g2 >= d2[CAP - 1]); }
    __device__ __forceinline__ void offer(double c, int i) {
        const double kth = d2[CAP - 1];
        const int kidx = idx[CAP - 1];
        if (!(c < kth || (c == kth && kidx >= 0 && i < kidx)) || i == self) return;
        // the candidate replaces the k-th best and sinks to its place: one pass of compare-and-swap, all indices static
        d2[CAP - 1] = c;
        idx[CAP - 1] = i;
        bool moving = true;
#pragma unroll
        for (int s = CAP - 1; s > 0; --s) {
            moving = moving && (c < d2[s - 1] || (c == d2[s - 1] && i < idx[s - 1]));
            d2[s] = moving ? d2[s - 1] : d2[s];
            idx[s] = moving ? idx[s - 1] : idx[s];
            d2[s - 1] = moving ? c : d2[s - 1];
            idx[s - 1] = moving ? i : idx[s - 1];
        }
    }
};

// The number of grid points with sqrt(d2) <= radius (decided on the rooted value, as reduce_round_kernel decides "within dst").
// The walk's bound is on squares and constant: radius^2 widened by far more than the last-bit difference between the two tests.
struct RadiusCount {
    double radius, bound;
    int self, count;
    __device__ __forceinline__ void init(double r, int self_) {
#pragma clang fp contract(off)
        radius = r;
        bound = r * r * (1.0 + 1.0 / 1099511627776.0) + 2.2250738585072014e-308;
        self = self_;
        count = 0;
    }
    __device__ __forceinline__ bool beyond(double g2) const { return g2 > bound; }
    __device__ __forceinline__ void offer(double c, int i) { count += (i != self && sqrt(c) <= radius) ? 1 : 0; }
};

// ---- what every query search repeats around the walk ---------------------------------------------------------------------------------
// One lane per query, 64-lane workgroups, queries taken in the caller's order.
struct QueryArgs {
    const float* query;  // [n_from][3]
    const int* order;    // [n_from] or null (identity)
    int n_from;
    int same_cloud;      // query i IS grid point i
};

// The prologue of a query kernel `(XArgs a)` with a QueryArgs a.q: lanes past the end return; the others get q (the row of the query
// and of every output), its coordinates widened, and self, the sorted index a search must not report (q itself under same_cloud,
// else -1).  A macro and not a function: with the bound inside a function the compiler lays the kernels out around a second branch,
// and the plain searches were measurably slower for it.
#define PC_QUERY_OR_RETURN(qa)                                                                                                  \
    const int t_ = blockIdx.x * 64 + threadIdx.x;                                                                               \
    if (t_ >= (qa).n_from) return;                                                                                              \
    const int q = (qa).order ? (qa).order[t_] : t_;                                                                             \
    const double qx = (double)(qa).query[(size_t)q * 3], qy = (double)(qa).query[(size_t)q * 3 + 1],                            \
                 qz = (double)(qa).query[(size_t)q * 3 + 2];                                                                    \
    [[maybe_unused]] const int self = (qa).same_cloud ? q : -1

static inline int query_args(QueryArgs& a, const float* query, const int* order, long long n_from, int same_cloud, long long n_to) {
    if (!query || n_from < 1 || n_from >= (1LL << 31) - 64) return PMN_ERR_ARG;
    if (same_cloud && n_from != n_to) return PMN_ERR_ARG;
    a.query = query;
    a.order = order;
    a.n_from = (int)n_from;
    a.same_cloud = same_cloud ? 1 : 0;
    return PMN_OK;
}

// the two checks of a reach (max_dist, radius, boundary) that caps a KBest list: its square is the cap and, where a kernel divides
// by it (the weight 1 - d2 / R2), must not have underflowed to 0
static inline bool pc_reach_ok(double r) { return r > 0.0 && std::isfinite(r) && std::isfinite(r * r); }
static inline bool pc_reach_square_ok(double r) { return pc_reach_ok(r) && r * r > 0.0; }

// PMN_LAUNCH of a kernel specialised on the capacity of its KBest list, for k in 1..32 (pc_k_ok): `kernel` is written with CAP where
// the capacity goes, as in PMN_LAUNCH_KBEST(k, knn_distance_kernel<CAP>, grid, ...) or (knn_mls_kernel<CAP, DEGREE>) in parentheses.
static inline bool pc_k_ok(int k) { return k >= 1 && k <= 32; }
#define PMN_LAUNCH_CAP(cap, kernel, ...) \
    {                                    \
        constexpr int CAP = cap;         \
        PMN_LAUNCH(kernel, __VA_ARGS__); \
    }
#define PMN_LAUNCH_KBEST(k, kernel, ...)                                \
    do {                                                                \
        if ((k) <= 8) PMN_LAUNCH_CAP(8, kernel, __VA_ARGS__)            \
        else if ((k) <= 16) PMN_LAUNCH_CAP(16, kernel, __VA_ARGS__)     \
        else PMN_LAUNCH_CAP(32, kernel, __VA_ARGS__)                    \
    } while (0)

static inline int grid_args(GridArgs& g, const float* xyz, const long long* keys, long long n, const double* origin_host, double cell,
                            const int* dims_host) {
    if (!xyz || !keys || !origin_host || !dims_host || n < 1 || n >= (1LL << 31)) return PMN_ERR_ARG;
    if (!(cell > 0.0) || !std::isfinite(cell)) return PMN_ERR_ARG;
    double cells = 1.0;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(origin_host[k]) || dims_host[k] < 1) return PMN_ERR_ARG;
        if (dims_host[k] > (1 << 30)) return PMN_ERR_SHAPE;
        cells *= (double)dims_host[k];
        g.dims[k] = dims_host[k];
        g.origin[k] = origin_host[k];
    }
    if (cells >= 9223372036854775808.0 / 2.0) return PMN_ERR_SHAPE;  // keys (and base + x1 + 1) stay below 2^63
    g.xyz = xyz;
    g.keys = keys;
    g.n = (int)n;
    g.cell = cell;
    return PMN_OK;
}
