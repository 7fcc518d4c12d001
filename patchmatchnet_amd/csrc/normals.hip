// normals.hip -- surface normals of a depth map in the camera frame of its image: the normal maps of the COLMAP
// workspace (stereo/normal_maps/<image>.geometric.bin) and the nx ny nz columns of an oriented fused.ply.  The reference has no
// counterpart: its colmap_output.py leaves stereo/normal_maps/ empty and its fused.ply carries positions and colours only.
//
// Estimator.  On a plane nu . X = d, inverse depth is AFFINE in pixel coordinates: 1 / z = (nu / d) . K^-1 (x, y, 1)^T.  So for a
// pixel p the kernel fits 1 / z_q - 1 / z_p ~ a dx + b dy + c by unweighted least squares over the pixels q of the (2r+1)^2 window
// that are inside the image, valid (finite, > 0) and on the same surface as p -- fabsf(z_q - z_p) <= rel_thres * z_p in float32, the
// relative test of the consistency filter -- and maps the coefficients back through K^T:
//     m = (fx a,  s a + fy b,  1 / z_p + c + a (cx - x_p) + b (cy - y_p)),     n = -m / |m|.
// m . ray = 1 / z > 0, so n faces the camera (n . ray < 0): COLMAP's convention.  The normal equations have INTEGER coefficients
// (moments of dx, dy over the accepted set, at most 49 pixels): their determinant D and adjugate are exact int32, D == 0 (fewer than
// three non-collinear accepted pixels) gives the zero normal, and which pixels have a normal is decided without a floating-point
// tolerance -- tests/normals_ref.py restates the decision in numpy and the sets are identical.  An invalid p gives the zero normal.
//
// Arithmetic.  t_q = 1 / z_q - 1 / z_p is evaluated as (z_p - z_q) / (z_p z_q): the numerator is exact for depths that passed the
// relative test, so the fit never sees the cancellation.  Sums run over the window in row-major order; divisions and the square root
// are IEEE (no rcp / rsq shortcuts) and nothing is contracted into FMAs, so a float32 numpy restatement that sums in the same order
// reproduces the kernel's bits; |m| is taken after an EXACT scaling of m by a power of two, so that depths near the ends of the
// float32 range neither overflow nor flush m . m (a float64 evaluation has a normal there, and so has this one).
//
// Shape.  A workgroup of 256 threads (four waves) owns a 64 x 16 tile and stages the tile plus its halo of r pixels in LDS once --
// 4 B read and 12 B written per pixel, so all that matters is that a depth value is fetched from memory once and not (2r+1)^2 times;
// pixels outside the image are staged as 0 (invalid), which is the inside-the-image test.  A wave owns a row of 64 pixels at a time
// (LDS reads of consecutive lanes are consecutive words: conflict-free; the three planar stores are 256 B each) and walks four rows.
#include <cstring>

#include "pmn_common.hpp"

#define NRM_TW 64
#define NRM_TH 16

struct NormalArgs {
    const float* depth;  // [H][W]
    float* normals;      // [3][H][W]
    int H, W;
    float fx, skew, fy, cx, cy, rel_thres;
};

__device__ __forceinline__ bool nrm_valid(float z) { return z > 0.0f && z < __builtin_inff(); }  // NaN fails both

// one rounding on each side, no contraction: the accepted set is reproducible bit for bit by a float32 numpy restatement
__device__ __forceinline__ bool nrm_same_surface(float zq, float zp, float rel_thres) {
#pragma clang fp contract(off)
    const float diff = fabsf(zq - zp);
    const float bound = rel_thres * zp;
    return diff <= bound;
}

template <int R>
__global__ __launch_bounds__(256) void depth_normals_kernel(const NormalArgs a) {
#pragma clang fp contract(off)
    constexpr int LW = NRM_TW + 2 * R, LH = NRM_TH + 2 * R;
    __shared__ float tile[LH * LW];
    const int x0 = blockIdx.x * NRM_TW, y0 = blockIdx.y * NRM_TH;
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = x0 + lx - R, gy = y0 + ly - R;
        tile[i] = (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) ? a.depth[(size_t)gy * a.W + gx] : 0.0f;
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = x0 + tx;
    if (x >= a.W) return;
    const size_t hw = (size_t)a.H * a.W;
    for (int ty = wv; ty < NRM_TH; ty += 4) {
        const int y = y0 + ty;
        if (y >= a.H) break;
        const float* c = tile + (ty + R) * LW + tx + R;
        const float zp = c[0];
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (nrm_valid(zp)) {
            int N = 0, Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0;
            float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
#pragma unroll
            for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    const float zq = c[dy * LW + dx];
                    if (nrm_valid(zq) && nrm_same_surface(zq, zp, a.rel_thres)) {
                        N += 1;
                        Sx += dx;
                        Sy += dy;
                        Sxx += dx * dx;
                        Sxy += dx * dy;
                        Syy += dy * dy;
                        const float t = (zp - zq) / (zp * zq);
                        b0 += (float)dx * t;
                        b1 += (float)dy * t;
                        b2 += t;
                    }
                }
            }
            // adjugate of M = [[Sxx, Sxy, Sx], [Sxy, Syy, Sy], [Sx, Sy, N]] (symmetric) and its determinant: exact, below 2^24
            const int A00 = Syy * N - Sy * Sy, A01 = Sx * Sy - Sxy * N, A02 = Sxy * Sy - Syy * Sx;
            const int A11 = Sxx * N - Sx * Sx, A12 = Sxy * Sx - Sxx * Sy, A22 = Sxx * Syy - Sxy * Sxy;
            const int D = Sxx * A00 + Sxy * A01 + Sx * A02;
            if (D != 0) {
                const float fD = (float)D;
                const float ca = (((float)A00 * b0 + (float)A01 * b1) + (float)A02 * b2) / fD;
                const float cb = (((float)A01 * b0 + (float)A11 * b1) + (float)A12 * b2) / fD;
                const float cc = (((float)A02 * b0 + (float)A12 * b1) + (float)A22 * b2) / fD;
                float mx = a.fx * ca;
                float my = a.skew * ca + a.fy * cb;
                float mz = ((1.0f / zp + cc) + ca * (a.cx - (float)x)) + cb * (a.cy - (float)y);
                const float big = fmaxf(fmaxf(fabsf(mx), fabsf(my)), fabsf(mz));  // (fmaxf drops a NaN: the sum below keeps it)
                if (big > 0.0f && big < __builtin_inff()) {
                    int e;
                    (void)frexpf(big, &e);
                    mx = ldexpf(mx, -e);  // exact: |m| is now in [0.5, sqrt(3))
                    my = ldexpf(my, -e);
                    mz = ldexpf(mz, -e);
                    const float len = sqrtf((mx * mx + my * my) + mz * mz);
                    if (len > 0.0f && len < __builtin_inff()) {
                        nx = -mx / len;
                        ny = -my / len;
                        nz = -mz / len;
                    }
                }
            }
        }
        const size_t p = (size_t)y * a.W + x;
        a.normals[p] = nx;
        a.normals[hw + p] = ny;
        a.normals[2 * hw + p] = nz;
    }
}

extern "C" int pmn_depth_normals(const float* depth, int H, int W, const float* intrinsics_host, int radius, float rel_thres,
                                 float* normals_out, void* stream) {
    if (!depth || !intrinsics_host || !normals_out || H < 1 || W < 1) return PMN_ERR_ARG;
    if (!(rel_thres > 0.0f) || !std::isfinite(rel_thres)) return PMN_ERR_ARG;
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(intrinsics_host[i])) return PMN_ERR_ARG;
    if (radius < 1 || radius > 3) return PMN_ERR_SHAPE;
    NormalArgs a;
    memset(&a, 0, sizeof(a));
    a.depth = depth;
    a.normals = normals_out;
    a.H = H;
    a.W = W;
    a.fx = intrinsics_host[0];
    a.skew = intrinsics_host[1];
    a.cx = intrinsics_host[2];
    a.fy = intrinsics_host[4];
    a.cy = intrinsics_host[5];
    a.rel_thres = rel_thres;
    const dim3 grid((W + NRM_TW - 1) / NRM_TW, (H + NRM_TH - 1) / NRM_TH);
    hipStream_t st = (hipStream_t)stream;
    if (radius == 1) PMN_LAUNCH(depth_normals_kernel<1>, grid, dim3(256), 0, st, a);
    else if (radius == 2) PMN_LAUNCH(depth_normals_kernel<2>, grid, dim3(256), 0, st, a);
    else PMN_LAUNCH(depth_normals_kernel<3>, grid, dim3(256), 0, st, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
