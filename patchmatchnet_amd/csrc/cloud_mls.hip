// cloud_mls.hip -- pmn_knn_mls: moving least squares on a point cloud.  knn_normals_kernel's walk (pointcloud.hip) with a longer
// epilogue: the lane that found the k nearest turns them into a weighted covariance, that into a local frame with the shared Jacobi
// sweeps (pc_jacobi.hpp), and projects its query onto the plane -- or, at degree 2, onto the quadric -- fitted in that frame.
// include/pmn_hip.h states every operation and its order; tests/mls_ref.py repeats them in numpy, and the kernel's outputs must
// equal that model bit for bit.  DESIGN.md section 36.
//
// Launch shape: one lane per query, one-wave workgroups, queries in cell order through `order`, KBest<CAP> specialised on 8 / 16 /
// 32, and on the degree, so that degree 1 carries none of the quadric's registers.  No LDS, no atomics, plain vector stores.
// The list is read through static slot indices only.  The 3 x 3 matrix and its rotations are named scalars; the quadric's 6 x 6
// normal equations are small arrays that are touched ONLY through indices the compiler knows (every loop over them is fully unrolled,
// exactly as KBest's list is), so they live in registers: the code object's metadata must show no scratch (DESIGN.md 36 has the table).
// The quadric needs the frame before it can form a single term, so its sums are a SECOND pass over the list: it reads the k points
// again, which are L2 hits.
#include "pc_grid.hpp"
#include "pc_jacobi.hpp"

#pragma clang fp contract(off)

struct MlsArgs {
    GridArgs g;
    QueryArgs q;
    int k;
    double radius;
    double line_ratio;
    float* position;       // [n_from][3]
    float* normal;         // [n_from][3] or null
    double* displacement;  // [n_from] or null
    int* status;           // [n_from] or null
    int* count;            // [n_from] or null
};

// entry (i, j), j <= i, of a symmetric or lower-triangular 6 x 6 matrix stored by rows
__device__ __forceinline__ constexpr int mls_at(int i, int j) { return i * (i + 1) / 2 + j; }

// The normal equations of the quadric: G = sum w phi phi^T (lower triangle) and g = sum w phi h over the members of the fit.
struct MlsQuadric {
    double G[21], g[6];

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < 21; ++i) G[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = 0.0;
    }
    // one member with weight w at r = d - x0, in the frame (n, e1, e2) scaled by 1 / radius along e1 and e2
    __device__ __forceinline__ void add(double w, double rx, double ry, double rz, double nx, double ny, double nz, double e1x, double e1y,
                                        double e1z, double e2x, double e2y, double e2z, double radius) {
        const double a = ((e1x * rx + e1y * ry) + e1z * rz) / radius;
        const double b = ((e2x * rx + e2y * ry) + e2z * rz) / radius;
        const double h = (nx * rx + ny * ry) + nz * rz;
        const double phi[6] = {1.0, a, b, a * a, a * b, b * b};
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double wp = j == 0 ? w : w * phi[j];
            g[j] += wp * h;
#pragma unroll
            for (int i = j; i < 6; ++i) G[mls_at(i, j)] += wp * phi[i];
        }
    }
    // Cholesky G = L L^T in place, column by column, then L y = g and L^T c = y; false when a pivot is not above `floor`
    __device__ __forceinline__ bool solve(double floor, double* c) {
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double v = G[mls_at(j, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - G[mls_at(j, k)] * G[mls_at(j, k)];
            ok = ok && v > floor;
            const double ljj = sqrt(v);
            G[mls_at(j, j)] = ljj;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double u = G[mls_at(i, j)];
#pragma unroll
                for (int k = 0; k < j; ++k) u = u - G[mls_at(i, k)] * G[mls_at(j, k)];
                G[mls_at(i, j)] = u / ljj;
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {  // forward: y overwrites g
            double v = g[i];
#pragma unroll
            for (int k = 0; k < i; ++k) v = v - G[mls_at(i, k)] * g[k];
            g[i] = v / G[mls_at(i, i)];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {  // back
            double v = g[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) v = v - G[mls_at(k, i)] * c[k];
            c[i] = v / G[mls_at(i, i)];
        }
        return ok;
    }
};

template <int CAP, int DEGREE>
__global__ __launch_bounds__(64) void knn_mls_kernel(MlsArgs a) {
    PC_QUERY_OR_RETURN(a.q);
    const double R2 = a.radius * a.radius;
    KBest<CAP> b;
    b.init(a.k, R2, self);
    pc_walk(a.g, qx, qy, qz, b);
    // the weighted moments of the deltas, members in rank order; under same_cloud the query comes first: the zero delta, weight 1
    double W = a.q.same_cloud ? 1.0 : 0.0, sx, sy, sz, mxx, mxy, mxz, myy, myz, mzz;
    const int used = pc_moments<true>(b, a.g.xyz, qx, qy, qz, R2, W, sx, sy, sz, mxx, mxy, mxz, myy, myz, mzz);
    const int m = used + (a.q.same_cloud ? 1 : 0);
    const double cx = sx / W, cy = sy / W, cz = sz / W;
    double a00 = mxx - (sx * sx) / W, a01 = mxy - (sx * sy) / W, a02 = mxz - (sx * sz) / W;
    double a11 = myy - (sy * sy) / W, a12 = myz - (sy * sz) / W, a22 = mzz - (sz * sz) / W;
    double v00, v01, v02, v10, v11, v12, v20, v21, v22;  // v[row][column]
    pc_eigen3(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    const double l1 = a11, l2 = a22;
    double nx = v00, ny = v10, nz = v20, e1x = v01, e1y = v11, e1z = v21, e2x = v02, e2y = v12, e2z = v22;
    pc_flip(pc_canonical_flip(nx, ny, nz), nx, ny, nz);  // pmn_knn_normals' sign rule, for every axis of the frame
    pc_flip(pc_canonical_flip(e1x, e1y, e1z), e1x, e1y, e1z);
    pc_flip(pc_canonical_flip(e2x, e2y, e2z), e2x, e2y, e2z);
    const bool valid = m >= 3 && W > 0.0 && l2 != 0.0 && l1 > a.line_ratio * l2;
    // the plane step
    const double tn = (nx * cx + ny * cy) + nz * cz;
    const double x0x = tn * nx, x0y = tn * ny, x0z = tn * nz;
    double mvx = x0x, mvy = x0y, mvz = x0z, onx = nx, ony = ny, onz = nz;
    int status = valid ? 1 : 0;
    if (DEGREE == 2 && valid && m >= PMN_MLS_QUADRIC_MIN) {
        MlsQuadric f;
        f.init();
        if (a.q.same_cloud) f.add(1.0, 0.0 - x0x, 0.0 - x0y, 0.0 - x0z, nx, ny, nz, e1x, e1y, e1z, e2x, e2y, e2z, a.radius);
#pragma unroll
        for (int s = 0; s < CAP; ++s) {
            const int i = b.idx[s];
            if (i < 0) continue;
            const float* p = a.g.xyz + (size_t)i * 3;
            const double dx = (double)p[0] - qx, dy = (double)p[1] - qy, dz = (double)p[2] - qz;
            const double u = 1.0 - b.d2[s] / R2, u2 = u * u, w = u2 * u2;
            f.add(w, dx - x0x, dy - x0y, dz - x0z, nx, ny, nz, e1x, e1y, e1z, e2x, e2y, e2z, a.radius);
        }
        double c[6];
        const bool ok = f.solve(PMN_MLS_PIVOT_MIN * W, c);
        const double gx = x0x + c[0] * nx, gy = x0y + c[0] * ny, gz = x0z + c[0] * nz;
        const double gg = (gx * gx + gy * gy) + gz * gz;
        if (ok && gg <= R2) {  // a move beyond the radius (or one that is not a number) keeps the plane step
            const double k1 = c[1] / a.radius, k2 = c[2] / a.radius;
            const double ux = (nx - k1 * e1x) - k2 * e2x, uy = (ny - k1 * e1y) - k2 * e2y, uz = (nz - k1 * e1z) - k2 * e2z;
            const double len = sqrt((ux * ux + uy * uy) + uz * uz);  // >= 1 up to rounding: e1 and e2 are orthogonal to n
            mvx = gx;
            mvy = gy;
            mvz = gz;
            onx = ux / len;
            ony = uy / len;
            onz = uz / len;
            status = 2;
        }
    }
    const float* qf = a.q.query + (size_t)q * 3;  // a point that stays keeps its float32 bits
    float px = qf[0], py = qf[1], pz = qf[2], fnx = 0.0f, fny = 0.0f, fnz = 0.0f;
    double disp = 0.0;
    if (status > 0) {
        px = (float)(qx + mvx);
        py = (float)(qy + mvy);
        pz = (float)(qz + mvz);
        fnx = (float)onx;
        fny = (float)ony;
        fnz = (float)onz;
        disp = sqrt((mvx * mvx + mvy * mvy) + mvz * mvz);
    }
    a.position[(size_t)q * 3] = px;
    a.position[(size_t)q * 3 + 1] = py;
    a.position[(size_t)q * 3 + 2] = pz;
    if (a.normal) {
        a.normal[(size_t)q * 3] = fnx;
        a.normal[(size_t)q * 3 + 1] = fny;
        a.normal[(size_t)q * 3 + 2] = fnz;
    }
    if (a.displacement) a.displacement[q] = disp;
    if (a.status) a.status[q] = status;
    if (a.count) a.count[q] = used;
}

template <int DEGREE>
static void mls_launch(const MlsArgs& a, hipStream_t stream) {
    PMN_LAUNCH_KBEST(a.k, (knn_mls_kernel<CAP, DEGREE>), dim3((unsigned)((a.q.n_from + 63) / 64)), dim3(64), 0, stream, a);
}

extern "C" int pmn_knn_mls(const float* to_xyz, const long long* to_keys, long long n_to, const double* origin_host, double cell,
                           const int* dims_host, const float* query, const int* order, long long n_from, int k, double radius,
                           int same_cloud, int degree, double line_ratio, float* position, float* normal, double* displacement,
                           int* status, int* count, void* stream) {
    MlsArgs a;
    const int rc = grid_args(a.g, to_xyz, to_keys, n_to, origin_host, cell, dims_host);
    if (rc != PMN_OK) return rc;
    if (query_args(a.q, query, order, n_from, same_cloud, n_to) != PMN_OK) return PMN_ERR_ARG;
    if (!position || !pc_k_ok(k) || !pc_reach_square_ok(radius)) return PMN_ERR_ARG;
    if (degree != 1 && degree != 2) return PMN_ERR_ARG;
    if (!(line_ratio >= 0.0) || !std::isfinite(line_ratio)) return PMN_ERR_ARG;
    a.k = k;
    a.radius = radius;
    a.line_ratio = line_ratio;
    a.position = position;
    a.normal = normal;
    a.displacement = displacement;
    a.status = status;
    a.count = count;
    if (degree == 1) mls_launch<1>(a, (hipStream_t)stream);
    else mls_launch<2>(a, (hipStream_t)stream);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
