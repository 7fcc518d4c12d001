// pc_jacobi.hpp -- the eigen-solver of a symmetric 3 x 3 matrix that the neighbourhood kernels share (pmn_knn_normals in pointcloud.hip,
// pmn_knn_mls in cloud_mls.hip): one cyclic Jacobi rotation and the compare-exchange that sorts the eigenpairs.  Every entry of the
// matrix and of the rotation is a named scalar passed by reference; include/pmn_hip.h (pmn_knn_normals) states the arithmetic and
// tests/cloud_normals_ref.py repeats it in numpy.
#pragma once

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
