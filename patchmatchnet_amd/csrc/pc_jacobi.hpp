// pc_jacobi.hpp -- what the neighbourhood kernels share after the walk (pmn_knn_normals in pointcloud.hip, pmn_knn_mls in
// cloud_mls.hip): the moments of a KBest list, the eigen-solver of a symmetric 3 x 3 matrix (cyclic Jacobi rotations and the
// compare-exchange that sorts the eigenpairs) and the canonical sign of a vector.  Every entry of the matrix and of the rotation is a
// named scalar passed by reference; include/pmn_hip.h (pmn_knn_normals) states the arithmetic and tests/cloud_normals_ref.py repeats
// it in numpy.
#pragma once
#include "pc_grid.hpp"

// The moments of the deltas p - q over the neighbours of a list in rank order (ascending slot): their number is returned, the sums
// s and the upper triangle m start at 0 here.  WEIGHTED: every delta counts with w = (1 - d2 / R2)^4, and W, which the caller has
// started, gains the weights.  Unweighted, R2 and W are not read.  Slots are static registers; a sentinel (-2) or capped (-1) slot is
// no neighbour.
template <bool WEIGHTED, int CAP>
__device__ __forceinline__ int pc_moments(const KBest<CAP>& b, const float* __restrict__ xyz, double qx, double qy, double qz, double R2,
                                          double& W, double& sx, double& sy, double& sz, double& mxx, double& mxy, double& mxz,
                                          double& myy, double& myz, double& mzz) {
#pragma clang fp contract(off)
    sx = sy = sz = mxx = mxy = mxz = myy = myz = mzz = 0.0;
    int used = 0;
#pragma unroll
    for (int s = 0; s < CAP; ++s) {
        const int i = b.idx[s];
        if (i < 0) continue;
        const float* p = xyz + (size_t)i * 3;
        const double dx = (double)p[0] - qx, dy = (double)p[1] - qy, dz = (double)p[2] - qz;
        double wx = dx, wy = dy, wz = dz;  // unweighted: the deltas themselves, no product with 1
        if constexpr (WEIGHTED) {
            const double u = 1.0 - b.d2[s] / R2, u2 = u * u, w = u2 * u2;
            wx = w * dx, wy = w * dy, wz = w * dz;
            W += w;
        }
        sx += wx;
        sy += wy;
        sz += wz;
        mxx += wx * dx;
        mxy += wx * dy;
        mxz += wx * dz;
        myy += wy * dy;
        myz += wy * dz;
        mzz += wz * dz;
        ++used;
    }
    return used;
}

// One Jacobi rotation in the (p, q) plane; r is the third index.  Skipped when the off-diagonal entry is exactly 0.
__device__ __forceinline__ void pc_jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                                 double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
#pragma clang fp contract(off)
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double root = fabs(theta) + sqrt(theta * theta + 1.0);
    const double t = theta < 0.0 ? -1.0 / root : 1.0 / root;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    const double x0 = c * v0p - s * v0q, y0 = s * v0p + c * v0q;
    v0p = x0;
    v0q = y0;
    const double x1 = c * v1p - s * v1q, y1 = s * v1p + c * v1q;
    v1p = x1;
    v1q = y1;
    const double x2 = c * v2p - s * v2q, y2 = s * v2p + c * v2q;
    v2p = x2;
    v2q = y2;
}

// exchanges eigenpair a and b when b's value is strictly the smaller: three of these sort three pairs, equal values keeping their order
__device__ __forceinline__ void pc_eigen_order(double& la, double& ax, double& ay, double& az, double& lb, double& bx, double& by,
                                               double& bz) {
    const bool swap = lb < la;
    const double l = la, x = ax, y = ay, z = az;
    la = swap ? lb : la;
    ax = swap ? bx : ax;
    ay = swap ? by : ay;
    az = swap ? bz : az;
    lb = swap ? l : lb;
    bx = swap ? x : bx;
    by = swap ? y : by;
    bz = swap ? z : bz;
}

// The eigenpairs of the symmetric matrix a (upper triangle): PMN_NORMAL_SWEEPS cyclic sweeps, then (a00, a11, a22) are the values
// ascending, equal values by column, and column c of v (v0c, v1c, v2c; v[row][column], the identity before the first rotation) is
// the vector of the c-th.
__device__ __forceinline__ void pc_eigen3(double& a00, double& a01, double& a02, double& a11, double& a12, double& a22, double& v00,
                                          double& v01, double& v02, double& v10, double& v11, double& v12, double& v20, double& v21,
                                          double& v22) {
    v00 = v11 = v22 = 1.0;
    v01 = v02 = v10 = v12 = v20 = v21 = 0.0;
    for (int sweep = 0; sweep < PMN_NORMAL_SWEEPS; ++sweep) {
        pc_jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1)
        pc_jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2)
        pc_jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2)
    }
    pc_eigen_order(a00, v00, v10, v20, a11, v01, v11, v21);
    pc_eigen_order(a11, v01, v11, v21, a22, v02, v12, v22);
    pc_eigen_order(a00, v00, v10, v20, a11, v01, v11, v21);
}

// Canonical sign of a vector: the component of largest magnitude positive, the lowest axis among equals.  The rule (must the vector
// be negated?) and the step that applies it are apart because knn_normals_kernel turns the answer once more, towards a viewpoint.
__device__ __forceinline__ bool pc_canonical_flip(double x, double y, double z) {
    const double ax = fabs(x), ay = fabs(y), az = fabs(z);
    const double lead = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
    return lead < 0.0;
}

__device__ __forceinline__ void pc_flip(bool flip, double& x, double& y, double& z) {
    x = flip ? -x : x;
    y = flip ? -y : y;
    z = flip ? -z : z;
}
