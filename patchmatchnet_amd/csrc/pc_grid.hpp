// pc_grid.hpp -- the uniform grid over sorted points and the nearest-neighbour shell walk over it, shared by pointcloud.hip (the DTU
// score) and registration.hip (ICP).  Layout, arithmetic and the slack of the bounds: the comment at the top of pointcloud.hip.
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

struct NnBest {
    double d2;
    int idx;
};

// the points of cells [x0, x1] x {y} x {z} (already inside the grid)
__device__ __forceinline__ void nn_scan_row(const GridArgs& g, int x0, int x1, int y, int z, double qx, double qy, double qz, NnBest& b) {
    const long long base = ((long long)z * g.dims[1] + y) * g.dims[0];
    const int i0 = pc_lower_bound(g.keys, 0, g.n, base + x0);
    if (i0 >= g.n || g.keys[i0] > base + x1) return;
    const int i1 = pc_lower_bound(g.keys, i0 + 1, g.n, base + x1 + 1);
    for (int i = i0; i < i1; ++i) {
        const double d2 = pc_dist2(g.xyz + (size_t)i * 3, qx, qy, qz);
        if (d2 < b.d2) {
            b.d2 = d2;
            b.idx = i;
        }
    }
}

// The nearest grid point of a query at (qx, qy, qz), any position: the query's cell, then shells of growing Chebyshev radius, until the
// best squared distance is no larger than the distance to the nearest face of the next shell or the shell lies beyond max_dist.
// idx = -1 and d2 = max_dist * max_dist where no point is nearer than max_dist.
__device__ __forceinline__ NnBest nn_search(const GridArgs& g, double qx, double qy, double qz, double max_dist) {
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
    NnBest b;
    b.d2 = max_dist * max_dist;  // a point at exactly max_dist or beyond never wins: the result is then max_dist itself
    b.idx = -1;
    const int rmax = max(max(max(cx, nx - 1 - cx), max(cy, ny - 1 - cy)), max(cz, nz - 1 - cz));  // last shell that touches the grid
    for (; r <= rmax; ++r) {
        // everything not yet visited is at least (r - 1) * cell + face away
        if (r > 0) {
            const double reach = (double)(r - 1) * g.cell + face;
            if (reach * reach >= b.d2) break;
        }
        const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
        for (int z = z0; z <= z1; ++z) {
            const double gz = pc_gap(qz, g.origin[2], g.cell, z, z);
            if (gz * gz >= b.d2) continue;
            const bool zface = z == cz - r || z == cz + r;
            for (int y = y0; y <= y1; ++y) {
                const double gy = pc_gap(qy, g.origin[1], g.cell, y, y);
                const double gyz = gy * gy + gz * gz;
                if (gyz >= b.d2) continue;
                if (zface || y == cy - r || y == cy + r) {
                    if (x0 <= x1) nn_scan_row(g, x0, x1, y, z, qx, qy, qz, b);
                } else {  // interior (y, z) of the shell: only its two end cells are new
                    if (cx - r >= 0 && cx - r < nx) {
                        const double gx = pc_gap(qx, g.origin[0], g.cell, cx - r, cx - r);
                        if (gx * gx + gyz < b.d2) nn_scan_row(g, cx - r, cx - r, y, z, qx, qy, qz, b);
                    }
                    if (cx + r >= 0 && cx + r < nx) {
                        const double gx = pc_gap(qx, g.origin[0], g.cell, cx + r, cx + r);
                        if (gx * gx + gyz < b.d2) nn_scan_row(g, cx + r, cx + r, y, z, qx, qy, qz, b);
                    }
                }
            }
        }
    }
    return b;
}

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
