// undistort.hip -- image undistortion of the COLMAP import (colmap_input.py --undistort).
//
// Every pixel (x, y) of the OUTPUT (an ideal pinhole camera fx' fy' cx' cy', patchmatchnet_amd/undistort.py) looks up where its ray
// lands in the distorted SOURCE picture and blends the four pixels around that position:
//     u = ((x + 0.5) - cx') / fx',  v = ((y + 0.5) - cy') / fy'            the ray, pixel centres at +0.5
//     (ud, vd) = the source camera's distortion of (u, v)                     und_distort<KIND> below
//     sx = (fx * ud + cx) - 0.5,  sy = (fy * vd + cy) - 0.5                   position among the source's pixel centres
//     x0 = floor(sx), ax = sx - x0 (y alike);  val = (1 - ay) * ((1 - ax) * s00 + ax * s01) + ay * ((1 - ax) * s10 + ax * s11)
//     out = floor(val + 0.5)
//
// Order contract (as pmn_view_scores, colmap.hip): the whole chain and the blend are float64, IEEE, WITHOUT contraction, in the
// operation order written here, so the positions are numpy's bits for the polynomial models (sqrt and the divisions are correctly
// rounded; atan of the fisheye models is within an ulp or two of libm's) and the bytes can be compared for equality.
//
// Bounds: a pixel is valid iff x0 >= 0, y0 >= 0, x0 + 1 <= Ws - 1 and y0 + 1 <= Hs - 1, decided on the DOUBLES before anything is
// converted to an integer and written so that NaN and the infinities fail (a zero denominator of FULL_OPENCV, a fisheye polynomial
// run wild): such a pixel is black, its `valid` byte 0, and no load is issued for it.
//
// Shape of the work: a thread makes PX = 4 x-adjacent output pixels, so that its output is whole dwords (12 bytes of RGB, 4 bytes
// of grey or of `valid`) wherever the row's bytes start on a dword -- every row when Wd is a multiple of 4; other rows and the
// row's tail are stored bytewise.  A workgroup is 32 x 8 threads = a 128 x 8-pixel tile (a wave: 128 x 2), so vertically adjacent
// outputs read the same source rows from the CU's L1 while they are there.  The two x-taps of a source row are 2 * channels
// contiguous bytes: one (unaligned) load per row, 8 bytes wide for RGB where the image has 8 bytes left, instead of six.
#include "pmn_common.hpp"

#define PMN_UND_PX 4
#define PMN_UND_BX 32
#define PMN_UND_BY 8

// distortion kinds = COLMAP's models with the two pinholes merged (the host spreads f into fx = fy)
enum { UND_NONE = 0, UND_SIMPLE_RADIAL, UND_RADIAL, UND_OPENCV, UND_OPENCV_FISHEYE, UND_FULL_OPENCV, UND_SIMPLE_RADIAL_FISHEYE,
       UND_RADIAL_FISHEYE };

struct UndistortArgs {
    const unsigned char* src;  // [Hs][Ws][CH]
    unsigned char* dst;        // [Hd][Wd][CH]
    unsigned char* valid;      // [Hd][Wd] or null
    double* coords;            // [Hd][Wd][2] (sx, sy) or null
    int Hs, Ws, Hd, Wd;
    double fx, fy, cx, cy;     // source camera
    double k[8];               // its distortion parameters in COLMAP's order (after the intrinsics)
    double dfx, dfy, dcx, dcy; // output pinhole
};

// (u, v) -> the distorted normalised point, per model in the operation order of DESIGN.md section 21
template <int KIND>
__device__ __forceinline__ void und_distort(const UndistortArgs& a, double u, double v, double& ud, double& vd) {
#pragma clang fp contract(off)
    if constexpr (KIND == UND_NONE) {
        ud = u;
        vd = v;
    } else if constexpr (KIND == UND_SIMPLE_RADIAL || KIND == UND_RADIAL) {
        const double r2 = u * u + v * v;
        double rad = a.k[0] * r2;
        if constexpr (KIND == UND_RADIAL) rad = rad + a.k[1] * (r2 * r2);
        ud = u + u * rad;
        vd = v + v * rad;
    } else if constexpr (KIND == UND_OPENCV || KIND == UND_FULL_OPENCV) {
        const double uu = u * u, vv = v * v, uv = u * v;
        const double r2 = uu + vv, r4 = r2 * r2;
        double du, dv;
        if constexpr (KIND == UND_OPENCV) {
            const double rad = a.k[0] * r2 + a.k[1] * r4;
            du = (u * rad + (2.0 * a.k[2]) * uv) + a.k[3] * (r2 + 2.0 * uu);
            dv = (v * rad + (2.0 * a.k[3]) * uv) + a.k[2] * (r2 + 2.0 * vv);
        } else {  // params k1 k2 p1 p2 k3 k4 k5 k6
            const double r6 = r4 * r2;
            const double num = ((1.0 + a.k[0] * r2) + a.k[1] * r4) + a.k[4] * r6;
            const double den = ((1.0 + a.k[5] * r2) + a.k[6] * r4) + a.k[7] * r6;
            const double rad = num / den;
            du = ((u * rad + (2.0 * a.k[2]) * uv) + a.k[3] * (r2 + 2.0 * uu)) - u;
            dv = ((v * rad + (2.0 * a.k[3]) * uv) + a.k[2] * (r2 + 2.0 * vv)) - v;
        }
        ud = u + du;
        vd = v + dv;
    } else if constexpr (KIND == UND_OPENCV_FISHEYE) {
        const double r = sqrt(u * u + v * v);
        double du = 0.0, dv = 0.0;
        if (!(r < 1e-12)) {
            const double th = atan(r);
            const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const double thd = th * ((((1.0 + a.k[0] * t2) + a.k[1] * t4) + a.k[2] * t6) + a.k[3] * t8);
            du = (u * thd) / r - u;
            dv = (v * thd) / r - v;
        }
        ud = u + du;
        vd = v + dv;
    } else {  // SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE: the equidistant point first, then the radial polynomial on it
        const double r = sqrt(u * u + v * v);
        const double th = atan(r);
        double uf = u, vf = v;
        if (!(r < 1e-12)) {
            uf = (u * th) / r;
            vf = (v * th) / r;
        }
        const double t2 = th * th;
        double rad = a.k[0] * t2;
        if constexpr (KIND == UND_RADIAL_FISHEYE) rad = rad + a.k[1] * (t2 * t2);
        ud = uf + uf * rad;
        vd = vf + vf * rad;
    }
}

// the two x-adjacent taps of one source row, every channel: t[c] = the left pixel's, t[CH + c] = the right pixel's
template <int CH>
__device__ __forceinline__ void und_row_taps(const unsigned char* __restrict__ src, size_t off, size_t total, double (&t)[2 * CH]) {
    if constexpr (CH == 1) {
        unsigned short q;
        __builtin_memcpy(&q, src + off, 2);
        t[0] = (double)(q & 0xFF);
        t[1] = (double)(q >> 8);
    } else {
        unsigned long long q = 0;
        if (off + 8 <= total) {
            __builtin_memcpy(&q, src + off, 8);
        } else {  // the last two pixels of the image: only their 6 bytes exist
#pragma unroll
            for (int b = 0; b < 6; ++b) q |= (unsigned long long)src[off + b] << (8 * b);
        }
#pragma unroll
        for (int b = 0; b < 6; ++b) t[b] = (double)((unsigned)(q >> (8 * b)) & 0xFFu);
    }
}

template <int KIND, int CH>
__global__ __launch_bounds__(PMN_UND_BX* PMN_UND_BY) void undistort_kernel(UndistortArgs a, int tiles_x) {
#pragma clang fp contract(off)
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int xb = (tx * PMN_UND_BX + (int)threadIdx.x) * PMN_UND_PX;  // first of this thread's pixels
    const int y = ty * PMN_UND_BY + (int)threadIdx.y;
    if (xb >= a.Wd || y >= a.Hd) return;
    const int n = min(PMN_UND_PX, a.Wd - xb);
    const size_t pix = (size_t)y * a.Wd + xb;
    const size_t total = (size_t)a.Hs * a.Ws * CH;
    const double xmax = (double)(a.Ws - 1), ymax = (double)(a.Hs - 1);
    const double v = (((double)y + 0.5) - a.dcy) / a.dfy;

    unsigned w[CH] = {};  // the PX * CH output bytes, little-endian
    unsigned ok4 = 0;     // the PX valid bytes
#pragma unroll
    for (int p = 0; p < PMN_UND_PX; ++p) {
        if (p < n) {
            const double u = (((double)(xb + p) + 0.5) - a.dcx) / a.dfx;
            double ud, vd;
            und_distort<KIND>(a, u, v, ud, vd);
            const double sx = (a.fx * ud + a.cx) - 0.5, sy = (a.fy * vd + a.cy) - 0.5;
            if (a.coords) {
                a.coords[(pix + p) * 2] = sx;
                a.coords[(pix + p) * 2 + 1] = sy;
            }
            const double x0 = floor(sx), y0 = floor(sy);
            // in double, and false for NaN / infinity: nothing below converts or addresses unless this holds
            const bool ok = sx >= 0.0 && sy >= 0.0 && x0 + 1.0 <= xmax && y0 + 1.0 <= ymax;
            if (ok) {
                const double ax = sx - x0, ay = sy - y0;
                const double bx = 1.0 - ax, by = 1.0 - ay;
                const size_t off = ((size_t)(int)y0 * a.Ws + (size_t)(int)x0) * CH;
                double r0[2 * CH], r1[2 * CH];
                und_row_taps<CH>(a.src, off, total, r0);
                und_row_taps<CH>(a.src, off + (size_t)a.Ws * CH, total, r1);
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const double val = by * (bx * r0[c] + ax * r0[CH + c]) + ay * (bx * r1[c] + ax * r1[CH + c]);
                    const unsigned byte = (unsigned)(int)floor(val + 0.5) & 0xFFu;
                    w[(p * CH + c) >> 2] |= byte << (8 * ((p * CH + c) & 3));
                }
                ok4 |= 1u << (8 * p);
            }
        }
    }

    unsigned char* d = a.dst + pix * CH;
    if (n == PMN_UND_PX && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
#pragma unroll
        for (int i = 0; i < CH; ++i) reinterpret_cast<unsigned*>(d)[i] = w[i];
    } else {
#pragma unroll
        for (int b = 0; b < PMN_UND_PX * CH; ++b)
            if (b < n * CH) d[b] = (unsigned char)(w[b >> 2] >> (8 * (b & 3)));
    }
    if (a.valid) {
        unsigned char* m = a.valid + pix;
        if (n == PMN_UND_PX && (reinterpret_cast<uintptr_t>(m) & 3) == 0) {
            *reinterpret_cast<unsigned*>(m) = ok4;
        } else {
#pragma unroll
            for (int p = 0; p < PMN_UND_PX; ++p)
                if (p < n) m[p] = (unsigned char)(ok4 >> (8 * p));
        }
    }
}

template <int KIND>
static int und_launch(const UndistortArgs& a, int channels, hipStream_t stream) {
    const long long tiles_x = (a.Wd + PMN_UND_BX * PMN_UND_PX - 1) / (PMN_UND_BX * PMN_UND_PX);
    const long long tiles_y = (a.Hd + PMN_UND_BY - 1) / PMN_UND_BY;
    if (tiles_x * tiles_y > 0x7FFFFFFFLL) return PMN_ERR_ARG;
    const dim3 grid((unsigned)(tiles_x * tiles_y)), block(PMN_UND_BX, PMN_UND_BY);
    if (channels == 1)
        PMN_LAUNCH((undistort_kernel<KIND, 1>), grid, block, 0, stream, a, (int)tiles_x);
    else
        PMN_LAUNCH((undistort_kernel<KIND, 3>), grid, block, 0, stream, a, (int)tiles_x);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_undistort_image(const unsigned char* src, int Hs, int Ws, int channels, int model, const double* src_params_host,
                                   const double* dst_pinhole_host, int Hd, int Wd, unsigned char* dst, unsigned char* valid,
                                   double* coords, void* stream) {
    if (!src || !dst || !src_params_host || !dst_pinhole_host) return PMN_ERR_ARG;
    if (Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1 || (channels != 1 && channels != 3)) return PMN_ERR_ARG;
    if ((long long)Hs * Ws * channels >= (1LL << 31) || (long long)Hd * Wd * channels >= (1LL << 31)) return PMN_ERR_ARG;
    // COLMAP's model ids; per model: one focal length or two, the number of distortion parameters, the kernel's kind.
    // 7 (FOV) and 10 (THIN_PRISM_FISHEYE) are refused.
    int two_f, nk, kind;
    switch (model) {
        case 0: two_f = 0, nk = 0, kind = UND_NONE; break;
        case 1: two_f = 1, nk = 0, kind = UND_NONE; break;
        case 2: two_f = 0, nk = 1, kind = UND_SIMPLE_RADIAL; break;
        case 3: two_f = 0, nk = 2, kind = UND_RADIAL; break;
        case 4: two_f = 1, nk = 4, kind = UND_OPENCV; break;
        case 5: two_f = 1, nk = 4, kind = UND_OPENCV_FISHEYE; break;
        case 6: two_f = 1, nk = 8, kind = UND_FULL_OPENCV; break;
        case 8: two_f = 0, nk = 1, kind = UND_SIMPLE_RADIAL_FISHEYE; break;
        case 9: two_f = 0, nk = 2, kind = UND_RADIAL_FISHEYE; break;
        default: return PMN_ERR_ARG;
    }
    UndistortArgs a;
    a.src = src;
    a.dst = dst;
    a.valid = valid;
    a.coords = coords;
    a.Hs = Hs;
    a.Ws = Ws;
    a.Hd = Hd;
    a.Wd = Wd;
    const double* q = src_params_host;
    a.fx = q[0];
    a.fy = two_f ? q[1] : q[0];
    a.cx = q[1 + two_f];
    a.cy = q[2 + two_f];
    for (int i = 0; i < 8; ++i) a.k[i] = i < nk ? q[3 + two_f + i] : 0.0;
    a.dfx = dst_pinhole_host[0];
    a.dfy = dst_pinhole_host[1];
    a.dcx = dst_pinhole_host[2];
    a.dcy = dst_pinhole_host[3];
    hipStream_t s = (hipStream_t)stream;
    switch (kind) {
        case UND_NONE: return und_launch<UND_NONE>(a, channels, s);
        case UND_SIMPLE_RADIAL: return und_launch<UND_SIMPLE_RADIAL>(a, channels, s);
        case UND_RADIAL: return und_launch<UND_RADIAL>(a, channels, s);
        case UND_OPENCV: return und_launch<UND_OPENCV>(a, channels, s);
        case UND_OPENCV_FISHEYE: return und_launch<UND_OPENCV_FISHEYE>(a, channels, s);
        case UND_FULL_OPENCV: return und_launch<UND_FULL_OPENCV>(a, channels, s);
        case UND_SIMPLE_RADIAL_FISHEYE: return und_launch<UND_SIMPLE_RADIAL_FISHEYE>(a, channels, s);
        default: return und_launch<UND_RADIAL_FISHEYE>(a, channels, s);
    }
}
