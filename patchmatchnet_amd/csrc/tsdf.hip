// tsdf.hip -- a surface mesh from a scan's depth maps: truncated-signed-distance integration of the masked depth
// maps into a dense volume, and an indexed, watertight iso-surface by marching tetrahedra on the Kuhn split of every cell.  The
// reference has no mesher; tests/tsdf_ref.py restates everything below in numpy and is the yardstick.
//
// Volume.  nx x ny x nz samples, x fastest; sample (i, j, k) sits at origin_c + (float)index * voxel per coordinate.  Planes (float32,
// the caller's): tsdf (initially 1), weight (0) and, as a group or not at all, rgb [3][nz][ny][nx] and cweight (0).
//
// Integration (tsdf_integrate_kernel), per sample p and per view of the batch, IN VIEW ORDER, float32, nothing contracted, IEEE division:
//     pc_r = ((R_r0 p.x + R_r1 p.y) + R_r2 p.z) + t_r                        skip the view if pc.z <= 0
//     q_r  = (K_r0 pc.x + K_r1 pc.y) + K_r2 pc.z
//     fx = floorf(q.x / q.z + 0.5f), fy likewise                            skip unless 0 <= fx < w and 0 <= fy < h (tested as floats: a
//                                                                            NaN or a huge value is "outside"), then px = (int)fx
//     d = depth[py][px]                                                     skip unless 0 < d < inf and the mask byte (if any) is non-zero
//     sdf = d - pc.z                                                        skip if sdf < -trunc;   obs = fminf(1, sdf / trunc)
//     tsdf = (tsdf * weight + obs) / (weight + 1);  weight = weight + 1
//     if colour and sdf <= trunc:  rgb_c = (rgb_c * cweight + (float)byte_c) / (cweight + 1);  cweight = cweight + 1
// The sample's values stay in registers across the views of a launch, so the volume crosses memory once per batch; a batch of V views
// leaves the bits of V single-view launches because every sample sees the same operations in the same order.  A thread per sample,
// workgroups of 64 x 4 samples (a wave = a 256-byte row of every plane); the per-view block (pointers, size, 21 camera floats) is a
// kernel argument read with a wave-uniform index, i.e. scalar loads.
//
// Marching tetrahedra.  A cell is the cube between samples (i..i+1, j..j+1, k..k+1); it is LIVE iff all eight corners have weight >=
// min_weight.  Corner c of a cell: bit 0 = x, bit 1 = y, bit 2 = z.  The six tetrahedra are {0, a, a|b, 7} for the orders (a, b, c) of
// the axis bits {1, 2, 4}, in lexicographic order of (a, b): all share the body diagonal 0-7 and the face diagonals of neighbouring cells
// coincide, so the surface is closed across cells.  A tetrahedron's orientation is the sign of the permutation (a, b, c):
// + - - + + -.  Every tetrahedron edge joins corners lo < hi with lo a subset of hi; it belongs to the sample at lo and has the class
// hi ^ lo (1..7).  An edge carries a vertex iff tsdf < 0 differs at its ends and one of the cells that contain it (the cells at
// owner - m for the subsets m of the complement of the class) is live.  The vertex is p_lo + t (p_hi - p_lo) per coordinate with
// t = v_lo / (v_lo - v_hi); colours, gradients use the same t.  MT_CASES is the 16-case table of a POSITIVE tetrahedron (bit p = local
// corner p inside): one inside corner i gives (e_ij, e_ik, e_il), j < k < l, with the last two swapped when i is odd; one outside
// corner o gives (e_oj, e_ok, e_ol) swapped when o is even; two inside a < b and two outside c < d give (ac, ad, bd), (ac, bd, bc)
// swapped when the permutation (a, b, c, d) is odd; a negative tetrahedron swaps the last two once more.  Normals point from inside to
// outside.  Order: vertices by owning sample (x fastest) then class; triangles by cell (x fastest), tetrahedron, triangle.
//
// Both per-cell arrays are indexed like the samples (cell (i, j, k) = the cube whose corner 0 is that sample; a sample on the last
// plane of an axis owns no cell and counts 0), so one index serves both.
#include <algorithm>
#include <cstring>

#include "pmn_common.hpp"

#define TSDF_BX 64
#define TSDF_BY 4

struct TsdfView {
    const float* depth;          // [h][w]
    const unsigned char* mask;   // [h][w] or null
    const unsigned char* image;  // [h][w][3] or null
    int h, w;
    float cam[21];  // K row-major, then the upper 3 x 4 of the world-to-camera extrinsic row-major
    int pad;
};

struct TsdfArgs {
    float *tsdf, *weight, *rgb, *cweight;
    int nx, ny, nz, nviews;
    float ox, oy, oz, voxel, trunc;
    TsdfView v[PMN_TSDF_MAX_VIEWS];
};

// One sample of a volume through the views of a launch: the arithmetic of the header comment, shared by the dense kernel and the
// block-sparse one (section 18).  ``a`` holds the planes, trunc and the views; s = the sample's index in a plane, n = the stride between
// the three colour planes, (x, y, z) = its world position.
template <class Args>
__device__ __forceinline__ void tsdf_fold_sample(const Args& a, size_t s, size_t n, float x, float y, float z) {
#pragma clang fp contract(off)
    const bool color = a.rgb != nullptr;
    float tv = a.tsdf[s], wt = a.weight[s], r = 0.0f, g = 0.0f, b = 0.0f, cw = 0.0f;
    if (color) {
        r = a.rgb[s];
        g = a.rgb[n + s];
        b = a.rgb[2 * n + s];
        cw = a.cweight[s];
    }
    bool touched = false;
    for (int vi = 0; vi < a.nviews; ++vi) {
        const TsdfView& v = a.v[vi];
        const float* K = v.cam;
        const float* E = v.cam + 9;
        const float pz = ((E[8] * x + E[9] * y) + E[10] * z) + E[11];
        if (!(pz > 0.0f)) continue;
        const float px = ((E[0] * x + E[1] * y) + E[2] * z) + E[3];
        const float py = ((E[4] * x + E[5] * y) + E[6] * z) + E[7];
        const float qx = (K[0] * px + K[1] * py) + K[2] * pz;
        const float qy = (K[3] * px + K[4] * py) + K[5] * pz;
        const float qz = (K[6] * px + K[7] * py) + K[8] * pz;
        const float fx = floorf(qx / qz + 0.5f), fy = floorf(qy / qz + 0.5f);
        if (!(fx >= 0.0f && fx < (float)v.w && fy >= 0.0f && fy < (float)v.h)) continue;
        const size_t pix = (size_t)(int)fy * v.w + (int)fx;
        const float d = v.depth[pix];
        if (!(d > 0.0f && d < __builtin_inff())) continue;
        if (v.mask && v.mask[pix] == 0) continue;
        const float sdf = d - pz;
        if (sdf < -a.trunc) continue;
        const float obs = fminf(1.0f, sdf / a.trunc);
        tv = (tv * wt + obs) / (wt + 1.0f);
        wt = wt + 1.0f;
        touched = true;
        if (color && v.image && sdf <= a.trunc) {
            const unsigned char* c = v.image + 3 * pix;
            r = (r * cw + (float)c[0]) / (cw + 1.0f);
            g = (g * cw + (float)c[1]) / (cw + 1.0f);
            b = (b * cw + (float)c[2]) / (cw + 1.0f);
            cw = cw + 1.0f;
        }
    }
    if (!touched) return;  // nothing was observed: the planes already hold these bits
    a.tsdf[s] = tv;
    a.weight[s] = wt;
    if (color) {
        a.rgb[s] = r;
        a.rgb[n + s] = g;
        a.rgb[2 * n + s] = b;
        a.cweight[s] = cw;
    }
}

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const TsdfArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * TSDF_BX + (threadIdx.x & 63), j = blockIdx.y * TSDF_BY + (threadIdx.x >> 6), k = blockIdx.z;
    if (i >= a.nx || j >= a.ny) return;
    const size_t n = (size_t)a.nx * a.ny * a.nz, s = ((size_t)k * a.ny + j) * a.nx + i;
    const float x = a.ox + (float)i * a.voxel, y = a.oy + (float)j * a.voxel, z = a.oz + (float)k * a.voxel;
    tsdf_fold_sample(a, s, n, x, y, z);
}

// the per-view block of a launch from the host tables (see pmn_tsdf_integrate in include/pmn_hip.h); ``cams`` = 21 finite floats per view
static int tsdf_fill_views(TsdfView* out, const float* maps, long long slot_stride, const int* slots_host, const int* hw_host,
                           const void* const* masks_host, const void* const* images_host, const float* cams_host, int n_views) {
    for (int v = 0; v < n_views; ++v) {
        const int h = hw_host[2 * v], w = hw_host[2 * v + 1];
        if (slots_host[v] < 0 || h < 1 || w < 1 || (long long)h * w > slot_stride) return PMN_ERR_ARG;
        out[v].depth = maps + (size_t)slots_host[v] * (size_t)slot_stride;
        out[v].mask = masks_host ? (const unsigned char*)masks_host[v] : nullptr;
        out[v].image = images_host ? (const unsigned char*)images_host[v] : nullptr;
        out[v].h = h;
        out[v].w = w;
        for (int c = 0; c < 21; ++c) {
            if (!std::isfinite(cams_host[21 * v + c])) return PMN_ERR_ARG;
            out[v].cam[c] = cams_host[21 * v + c];
        }
    }
    return PMN_OK;
}

extern "C" int pmn_tsdf_integrate(float* tsdf, float* weight, float* rgb, float* cweight, const int* dims_host, const float* origin_host,
                                  float voxel, float trunc, const float* maps, long long slot_stride, const int* slots_host,
                                  const int* hw_host, const void* const* masks_host, const void* const* images_host,
                                  const float* cams_host, int n_views, void* stream) {
    if (!tsdf || !weight || !dims_host || !origin_host || !maps || !slots_host || !hw_host || !cams_host) return PMN_ERR_ARG;
    if ((rgb == nullptr) != (cweight == nullptr)) return PMN_ERR_ARG;
    if (!(voxel > 0.0f) || !(trunc > 0.0f) || !std::isfinite(voxel) || !std::isfinite(trunc) || slot_stride < 1) return PMN_ERR_ARG;
    if (n_views < 1 || n_views > PMN_TSDF_MAX_VIEWS) return PMN_ERR_SHAPE;
    const int nx = dims_host[0], ny = dims_host[1], nz = dims_host[2];
    if (nx < 1 || ny < 1 || nz < 1 || nz > 65535 || (long long)nx * ny * nz > 2147483647LL) return PMN_ERR_SHAPE;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(origin_host[c])) return PMN_ERR_ARG;
    TsdfArgs a;
    memset(&a, 0, sizeof(a));
    a.tsdf = tsdf;
    a.weight = weight;
    a.rgb = rgb;
    a.cweight = cweight;
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    a.nviews = n_views;
    a.ox = origin_host[0];
    a.oy = origin_host[1];
    a.oz = origin_host[2];
    a.voxel = voxel;
    a.trunc = trunc;
    const int rc = tsdf_fill_views(a.v, maps, slot_stride, slots_host, hw_host, masks_host, images_host, cams_host, n_views);
    if (rc != PMN_OK) return rc;
    const dim3 grid((nx + TSDF_BX - 1) / TSDF_BX, (ny + TSDF_BY - 1) / TSDF_BY, nz);
    PMN_LAUNCH(tsdf_integrate_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// ---- marching tetrahedra ------------------------------------------------------------------------------------------------------

struct MtCase {
    unsigned char ntri;
    unsigned char edge[6];  // local corners p | q << 2 of the edge each triangle vertex sits on
};
__constant__ MtCase MT_CASES[16] = {
    {0, {0, 0, 0, 0, 0, 0}},      {1, {4, 8, 12, 0, 0, 0}},     {1, {4, 13, 9, 0, 0, 0}},     {2, {8, 12, 13, 8, 13, 9}},
    {1, {8, 9, 14, 0, 0, 0}},     {2, {4, 14, 12, 4, 9, 14}},   {2, {4, 13, 14, 4, 14, 8}},   {1, {12, 13, 14, 0, 0, 0}},
    {1, {12, 14, 13, 0, 0, 0}},   {2, {4, 8, 14, 4, 14, 13}},   {2, {4, 14, 9, 4, 12, 14}},   {1, {8, 14, 9, 0, 0, 0}},
    {2, {8, 9, 13, 8, 13, 12}},   {1, {4, 9, 13, 0, 0, 0}},     {1, {4, 12, 8, 0, 0, 0}},     {0, {0, 0, 0, 0, 0, 0}}};
__constant__ unsigned char MT_TET[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
// bit t = tetrahedron t is negatively oriented (orders 1,4,2 / 2,1,4 / 4,2,1)
#define MT_NEGATIVE 0x26

struct MtArgs {
    const float *tsdf, *weight, *rgb, *cweight;
    int nx, ny, nz;
    float ox, oy, oz, voxel, min_weight;
    unsigned char *vmask, *ntri;  // count: outputs; emit: inputs
    const int *vincl, *tincl;     // emit: INCLUSIVE scans of popcount(vmask) and of ntri
    float* vertices;
    unsigned char* colors;
    float* normals;
    int* faces;
};

__device__ __forceinline__ bool mt_ok(const MtArgs& a, int i, int j, int k) {
    if (i < 0 || j < 0 || k < 0 || i >= a.nx || j >= a.ny || k >= a.nz) return false;
    return a.weight[((size_t)k * a.ny + j) * a.nx + i] >= a.min_weight;
}

// bit c = corner c of the cell at (i, j, k) is inside (tsdf < 0); the cell must lie in the lattice
__device__ __forceinline__ unsigned mt_inside(const MtArgs& a, int i, int j, int k) {
    unsigned in = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        in |= (a.tsdf[((size_t)(k + (c >> 2)) * a.ny + (j + ((c >> 1) & 1))) * a.nx + (i + (c & 1))] < 0.0f ? 1u : 0u) << c;
    return in;
}

__device__ __forceinline__ unsigned mt_tet_case(unsigned in, int t) {
    return ((in >> MT_TET[t][0]) & 1u) | (((in >> MT_TET[t][1]) & 1u) << 1) | (((in >> MT_TET[t][2]) & 1u) << 2) |
           (((in >> MT_TET[t][3]) & 1u) << 3);
}

__global__ __launch_bounds__(256) void mt_count_kernel(const MtArgs a) {
    const int i = blockIdx.x * TSDF_BX + (threadIdx.x & 63), j = blockIdx.y * TSDF_BY + (threadIdx.x >> 6), k = blockIdx.z;
    if (i >= a.nx || j >= a.ny) return;
    const size_t s = ((size_t)k * a.ny + j) * a.nx + i;
    // which samples of the 3 x 3 x 3 neighbourhood are observed: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
    unsigned okb = 0;
#pragma unroll
    for (int q = 0; q < 27; ++q)
        okb |= (mt_ok(a, i + q % 3 - 1, j + (q / 3) % 3 - 1, k + q / 9 - 1) ? 1u : 0u) << q;
    // live[m]: the cell at this sample - m (m = corner bits) is live
    unsigned live = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int bx = 1 - (m & 1), by = 1 - ((m >> 1) & 1), bz = 1 - (m >> 2);  // the cell's corner 0 in the neighbourhood
        const unsigned base = 1u << (bz * 9 + by * 3 + bx);
        const unsigned need = base * (1u | 2u | 8u | 16u | 512u | 1024u | 4096u | 8192u);
        live |= ((okb & need) == need ? 1u : 0u) << m;
    }
    unsigned mask = 0;
    if (live) {
        const bool in0 = a.tsdf[s] < 0.0f;
#pragma unroll
        for (int c = 1; c < 8; ++c) {
            unsigned users = 0;  // the cells that contain the edge of class c: m a subset of ~c
#pragma unroll
            for (int m = 0; m < 8; ++m)
                if ((m & c) == 0) users |= 1u << m;
            if (live & users) {  // then the far end is inside the lattice
                const bool in1 = a.tsdf[((size_t)(k + (c >> 2)) * a.ny + (j + ((c >> 1) & 1))) * a.nx + (i + (c & 1))] < 0.0f;
                if (in0 != in1) mask |= 1u << (c - 1);
            }
        }
    }
    a.vmask[s] = (unsigned char)mask;
    unsigned nt = 0;
    if (live & 1u) {
        const unsigned in = mt_inside(a, i, j, k);
        if (in != 0u && in != 255u) {
#pragma unroll
            for (int t = 0; t < 6; ++t) nt += MT_CASES[mt_tet_case(in, t)].ntri;
        }
    }
    a.ntri[s] = (unsigned char)nt;
}

__device__ __forceinline__ int mt_vertex_index(const MtArgs& a, size_t owner, int cls) {
    const unsigned m = a.vmask[owner];
    return a.vincl[owner] - __popc(m) + __popc(m & ((1u << (cls - 1)) - 1u));
}

// central-difference gradient of tsdf at a sample; false where a neighbour is outside the lattice or unobserved
__device__ __forceinline__ bool mt_gradient(const MtArgs& a, int i, int j, int k, float& gx, float& gy, float& gz) {
#pragma clang fp contract(off)
    if (!(mt_ok(a, i - 1, j, k) && mt_ok(a, i + 1, j, k) && mt_ok(a, i, j - 1, k) && mt_ok(a, i, j + 1, k) && mt_ok(a, i, j, k - 1) &&
          mt_ok(a, i, j, k + 1)))
        return false;
    const size_t s = ((size_t)k * a.ny + j) * a.nx + i, sy = (size_t)a.nx, sz = (size_t)a.nx * a.ny;
    gx = a.tsdf[s + 1] - a.tsdf[s - 1];
    gy = a.tsdf[s + sy] - a.tsdf[s - sy];
    gz = a.tsdf[s + sz] - a.tsdf[s - sz];
    return true;
}

__global__ __launch_bounds__(256) void mt_emit_kernel(const MtArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * TSDF_BX + (threadIdx.x & 63), j = blockIdx.y * TSDF_BY + (threadIdx.x >> 6), k = blockIdx.z;
    if (i >= a.nx || j >= a.ny) return;
    const size_t n = (size_t)a.nx * a.ny * a.nz, s = ((size_t)k * a.ny + j) * a.nx + i;
    const unsigned mask = a.vmask[s];
    if (mask) {
        int out = a.vincl[s] - __popc(mask);
        const float v0 = a.tsdf[s];
        const float x0 = a.ox + (float)i * a.voxel, y0 = a.oy + (float)j * a.voxel, z0 = a.oz + (float)k * a.voxel;
        float g0x = 0.0f, g0y = 0.0f, g0z = 0.0f;
        const bool have_g0 = a.normals && mt_gradient(a, i, j, k, g0x, g0y, g0z);
        for (int c = 1; c < 8; ++c) {
            if (!((mask >> (c - 1)) & 1u)) continue;
            const int i1 = i + (c & 1), j1 = j + ((c >> 1) & 1), k1 = k + (c >> 2);
            const size_t s1 = ((size_t)k1 * a.ny + j1) * a.nx + i1;
            const float v1 = a.tsdf[s1];
            const float t = v0 / (v0 - v1);
            const float x1 = a.ox + (float)i1 * a.voxel, y1 = a.oy + (float)j1 * a.voxel, z1 = a.oz + (float)k1 * a.voxel;
            a.vertices[3 * (size_t)out + 0] = x0 + t * (x1 - x0);
            a.vertices[3 * (size_t)out + 1] = y0 + t * (y1 - y0);
            a.vertices[3 * (size_t)out + 2] = z0 + t * (z1 - z0);
            if (a.colors) {
                const float cw0 = a.cweight[s], cw1 = a.cweight[s1];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float c0 = a.rgb[ch * n + s], c1 = a.rgb[ch * n + s1];
                    float cv = 128.0f;
                    if (cw0 > 0.0f && cw1 > 0.0f) cv = c0 + t * (c1 - c0);
                    else if (cw0 > 0.0f) cv = c0;
                    else if (cw1 > 0.0f) cv = c1;
                    cv = floorf(cv + 0.5f);
                    a.colors[3 * (size_t)out + ch] = (unsigned char)fminf(fmaxf(cv, 0.0f), 255.0f);
                }
            }
            if (a.normals) {
                float nx = 0.0f, ny = 0.0f, nz = 0.0f, g1x, g1y, g1z;
                if (have_g0 && mt_gradient(a, i1, j1, k1, g1x, g1y, g1z)) {
                    const float gx = g0x + t * (g1x - g0x), gy = g0y + t * (g1y - g0y), gz = g0z + t * (g1z - g0z);
                    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
                    if (len > 0.0f && len < __builtin_inff()) {
                        nx = gx / len;
                        ny = gy / len;
                        nz = gz / len;
                    }
                }
                a.normals[3 * (size_t)out + 0] = nx;
                a.normals[3 * (size_t)out + 1] = ny;
                a.normals[3 * (size_t)out + 2] = nz;
            }
            ++out;
        }
    }
    const unsigned nt = a.ntri[s];
    if (nt) {
        int f = a.tincl[s] - (int)nt;
        const unsigned in = mt_inside(a, i, j, k);
        for (int t = 0; t < 6; ++t) {
            const MtCase& cs = MT_CASES[mt_tet_case(in, t)];
            const bool neg = (MT_NEGATIVE >> t) & 1;
            for (int tri = 0; tri < cs.ntri; ++tri) {
                int idx[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const unsigned code = cs.edge[3 * tri + e];
                    const int lo = MT_TET[t][code & 3u], hi = MT_TET[t][code >> 2];
                    const size_t owner = ((size_t)(k + (lo >> 2)) * a.ny + (j + ((lo >> 1) & 1))) * a.nx + (i + (lo & 1));
                    idx[e] = mt_vertex_index(a, owner, hi ^ lo);
                }
                a.faces[3 * (size_t)f + 0] = idx[0];
                a.faces[3 * (size_t)f + 1] = neg ? idx[2] : idx[1];
                a.faces[3 * (size_t)f + 2] = neg ? idx[1] : idx[2];
                ++f;
            }
        }
    }
}

static int mt_fill(MtArgs& a, const float* tsdf, const float* weight, const int* dims_host, const float* origin_host, float voxel,
                   float min_weight) {
    if (!tsdf || !weight || !dims_host || !origin_host) return PMN_ERR_ARG;
    if (!(voxel > 0.0f) || !std::isfinite(voxel) || !std::isfinite(min_weight)) return PMN_ERR_ARG;
    const int nx = dims_host[0], ny = dims_host[1], nz = dims_host[2];
    if (nx < 1 || ny < 1 || nz < 1 || nz > 65535 || (long long)nx * ny * nz > 2147483647LL) return PMN_ERR_SHAPE;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(origin_host[c])) return PMN_ERR_ARG;
    memset(&a, 0, sizeof(a));
    a.tsdf = tsdf;
    a.weight = weight;
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    a.ox = origin_host[0];
    a.oy = origin_host[1];
    a.oz = origin_host[2];
    a.voxel = voxel;
    a.min_weight = min_weight;
    return PMN_OK;
}

extern "C" int pmn_mt_count(const float* tsdf, const float* weight, const int* dims_host, float min_weight, unsigned char* vertex_mask,
                            unsigned char* cell_triangles, void* stream) {
    static const float origin[3] = {0.0f, 0.0f, 0.0f};
    if (!vertex_mask || !cell_triangles) return PMN_ERR_ARG;
    MtArgs a;
    const int rc = mt_fill(a, tsdf, weight, dims_host, origin, 1.0f, min_weight);
    if (rc != PMN_OK) return rc;
    a.vmask = vertex_mask;
    a.ntri = cell_triangles;
    const dim3 grid((a.nx + TSDF_BX - 1) / TSDF_BX, (a.ny + TSDF_BY - 1) / TSDF_BY, a.nz);
    PMN_LAUNCH(mt_count_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_mt_emit(const float* tsdf, const float* weight, const float* rgb, const float* cweight, const int* dims_host,
                           const float* origin_host, float voxel, float min_weight, const unsigned char* vertex_mask,
                           const unsigned char* cell_triangles, const int* vertex_scan, const int* triangle_scan, float* vertices,
                           unsigned char* colors, float* normals, int* faces, void* stream) {
    if (!vertex_mask || !cell_triangles || !vertex_scan || !triangle_scan || !vertices || !faces) return PMN_ERR_ARG;
    if ((rgb == nullptr) != (cweight == nullptr) || (colors != nullptr && rgb == nullptr)) return PMN_ERR_ARG;
    MtArgs a;
    const int rc = mt_fill(a, tsdf, weight, dims_host, origin_host, voxel, min_weight);
    if (rc != PMN_OK) return rc;
    a.rgb = rgb;
    a.cweight = cweight;
    a.vmask = const_cast<unsigned char*>(vertex_mask);
    a.ntri = const_cast<unsigned char*>(cell_triangles);
    a.vincl = vertex_scan;
    a.tincl = triangle_scan;
    a.vertices = vertices;
    a.colors = colors;
    a.normals = normals;
    a.faces = faces;
    const dim3 grid((a.nx + TSDF_BX - 1) / TSDF_BX, (a.ny + TSDF_BY - 1) / TSDF_BY, a.nz);
    PMN_LAUNCH(mt_emit_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// ---- block-sparse volume -----------------------------------------------------------------------------------
// The same lattice, stored in blocks of 8 x 8 x 8 samples of which only those near some view's surface exist.  dims = (nx, ny, nz) is
// the VIRTUAL lattice (2 <= n < 2^19 per axis, so (float)index is exact); nb = ceil(n / 8) blocks per axis, nbx * nby * nbz <= 2^28.
//   table  int32 [nbz][nby][nbx]   the block's slot in the pool, or -1
//   blocks int32 [B]               the linear block index of every slot, ascending; B * 512 < 2^31
//   pool   float32 tsdf [B][8][8][8] (1), weight (0) and -- both or neither -- rgb [3][B][8][8][8], cweight (0); x fastest in a block
// A sample of a border block whose index is >= n on some axis is outside the lattice: never integrated, never meshed.  A sample outside
// the lattice or in a block without a slot reads as tsdf 1, weight 0, cweight 0, so with min_weight > 0 (required) no cell that touches
// one is live and everything the dense kernels would emit from the same planes comes out of the pool, in pool order.
#define TSDF_SB 8                                   // samples per block side
#define TSDF_SB3 (TSDF_SB * TSDF_SB * TSDF_SB)      // samples per block = threads per workgroup
#define TSDF_MAX_AXIS (1 << 19)
#define TSDF_MAX_TABLE (1LL << 28)

struct TsdfLattice {
    int nx, ny, nz, nbx, nby, nbz;
};

static int tsdf_lattice(TsdfLattice& l, const int* dims_host) {
    if (!dims_host) return PMN_ERR_ARG;
    l.nx = dims_host[0];
    l.ny = dims_host[1];
    l.nz = dims_host[2];
    if (l.nx < 2 || l.ny < 2 || l.nz < 2 || l.nx >= TSDF_MAX_AXIS || l.ny >= TSDF_MAX_AXIS || l.nz >= TSDF_MAX_AXIS) return PMN_ERR_SHAPE;
    l.nbx = (l.nx + TSDF_SB - 1) / TSDF_SB;
    l.nby = (l.ny + TSDF_SB - 1) / TSDF_SB;
    l.nbz = (l.nz + TSDF_SB - 1) / TSDF_SB;
    if ((long long)l.nbx * l.nby * l.nbz > TSDF_MAX_TABLE) return PMN_ERR_SHAPE;
    return PMN_OK;
}

static bool tsdf_pool_size_ok(int n_blocks) { return n_blocks >= 1 && (long long)n_blocks * TSDF_SB3 <= 2147483647LL; }

// Marking: a thread per pixel of every view of the launch (blockIdx.y = the view, so the view block is read with scalar loads).  The
// samples that pmn_tsdf_integrate maps to a valid pixel (u, v) of depth d with |sdf| <= trunc lie in the section of the pyramid through
// the pixel's corners (u +- 0.5, v +- 0.5) between the camera depths max(d - trunc, 0) (0 = the apex: a superset of any positive clamp
// and free of a unit) and d + trunc.  Its eight corners go to the world through K^-1 and E^-1 (v.cam holds K^-1 row-major, then the
// upper 3 x 4 of E^-1, inverted on the host in float64); their axis-aligned box grown by one voxel and clipped to the lattice gives the
// blocks.  flags get plain byte stores of 1: whichever thread writes, the byte is 1.
struct TsdfMarkArgs {
    unsigned char* flags;  // [nbz][nby][nbx]
    int* overflow;
    TsdfLattice l;
    float ox, oy, oz, voxel, trunc;
    TsdfView v[PMN_TSDF_MAX_VIEWS];
};

__global__ __launch_bounds__(256) void tsdf_mark_blocks_kernel(const TsdfMarkArgs a) {
#pragma clang fp contract(off)
    const TsdfView& v = a.v[blockIdx.y];
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= v.h * v.w) return;
    const float d = v.depth[pix];
    if (!(d > 0.0f && d < __builtin_inff())) return;
    if (v.mask && v.mask[pix] == 0) return;
    const float pu = (float)(pix % v.w), pv = (float)(pix / v.w);
    const float* Ki = v.cam;
    const float* Ei = v.cam + 9;
    const float depth[2] = {fmaxf(d - a.trunc, 0.0f), d + a.trunc};
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float cu = pu + ((c & 1) ? 0.5f : -0.5f), cv = pv + ((c & 2) ? 0.5f : -0.5f);
        const float rx = (Ki[0] * cu + Ki[1] * cv) + Ki[2], ry = (Ki[3] * cu + Ki[4] * cv) + Ki[5], rz = (Ki[6] * cu + Ki[7] * cv) + Ki[8];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            // the camera-frame point of depth cz on the ray (settled: no packed op may pick a high half, pmn_common.hpp lesson 46)
            const float s = depth[e] / rz, cx = pmn_settle(rx * s), cy = pmn_settle(ry * s), cz = pmn_settle(depth[e]);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float wc = pmn_settle(((Ei[4 * r] * cx + Ei[4 * r + 1] * cy) + Ei[4 * r + 2] * cz) + Ei[4 * r + 3]);
                finite = finite && fabsf(wc) < __builtin_inff();
                lo[r] = fminf(lo[r], wc);
                hi[r] = fmaxf(hi[r], wc);
            }
        }
    }
    if (!finite) {  // a depth so large that the section has no position (also a NaN from a singular ray)
        atomicAdd(a.overflow, 1);
        return;
    }
    const float org[3] = {a.ox, a.oy, a.oz};
    const int n[3] = {a.l.nx, a.l.ny, a.l.nz};
    int b0[3], b1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float fl = ceilf((lo[r] - org[r]) / a.voxel) - 1.0f, fh = floorf((hi[r] - org[r]) / a.voxel) + 1.0f;  // +- one voxel
        if (fh < 0.0f || fl > (float)(n[r] - 1)) return;  // the box misses the lattice
        b0[r] = (int)fmaxf(fl, 0.0f) / TSDF_SB;
        b1[r] = (int)fminf(fh, (float)(n[r] - 1)) / TSDF_SB;
    }
    if (b1[0] - b0[0] >= PMN_TSDF_MARK_SPAN || b1[1] - b0[1] >= PMN_TSDF_MARK_SPAN || b1[2] - b0[2] >= PMN_TSDF_MARK_SPAN) {
        atomicAdd(a.overflow, 1);  // a wild depth must not loop over the lattice: the host raises
        return;
    }
    for (int bz = b0[2]; bz <= b1[2]; ++bz)
        for (int by = b0[1]; by <= b1[1]; ++by)
            for (int bx = b0[0]; bx <= b1[0]; ++bx) a.flags[((size_t)bz * a.l.nby + by) * a.l.nbx + bx] = 1;
}

static int tsdf_check_grid(const float* origin_host, float voxel, float trunc) {
    if (!origin_host || !(voxel > 0.0f) || !(trunc > 0.0f) || !std::isfinite(voxel) || !std::isfinite(trunc)) return PMN_ERR_ARG;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(origin_host[c])) return PMN_ERR_ARG;
    return PMN_OK;
}

extern "C" int pmn_tsdf_mark_blocks(unsigned char* flags, int* overflow, const int* dims_host, const float* origin_host, float voxel,
                                    float trunc, const float* maps, long long slot_stride, const int* slots_host, const int* hw_host,
                                    const void* const* masks_host, const float* inv_cams_host, int n_views, void* stream) {
    if (!flags || !overflow || !dims_host || !maps || !slots_host || !hw_host || !inv_cams_host || slot_stride < 1) return PMN_ERR_ARG;
    int rc = tsdf_check_grid(origin_host, voxel, trunc);
    if (rc != PMN_OK) return rc;
    if (n_views < 1 || n_views > PMN_TSDF_MAX_VIEWS) return PMN_ERR_SHAPE;
    TsdfMarkArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = tsdf_lattice(a.l, dims_host)) != PMN_OK) return rc;
    a.flags = flags;
    a.overflow = overflow;
    a.ox = origin_host[0];
    a.oy = origin_host[1];
    a.oz = origin_host[2];
    a.voxel = voxel;
    a.trunc = trunc;
    if ((rc = tsdf_fill_views(a.v, maps, slot_stride, slots_host, hw_host, masks_host, nullptr, inv_cams_host, n_views)) != PMN_OK) return rc;
    long long pixels = 0;
    for (int v = 0; v < n_views; ++v) pixels = std::max(pixels, (long long)a.v[v].h * a.v[v].w);
    if (pixels > 2147483647LL) return PMN_ERR_SHAPE;
    const dim3 grid((unsigned)((pixels + 255) / 256), n_views);
    PMN_LAUNCH(tsdf_mark_blocks_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// Integration of the listed blocks: a workgroup per block, a thread per sample (a wave = one 8 x 8 plane = 256 contiguous bytes of
// every pool plane); the sample's lattice index comes from the block list, everything else is tsdf_fold_sample.
struct TsdfBlockArgs {
    float *tsdf, *weight, *rgb, *cweight;
    const int* blocks;
    int nblocks, nviews;
    TsdfLattice l;
    float ox, oy, oz, voxel, trunc;
    TsdfView v[PMN_TSDF_MAX_VIEWS];
};

__global__ __launch_bounds__(TSDF_SB3) void tsdf_integrate_blocks_kernel(const TsdfBlockArgs a) {
#pragma clang fp contract(off)
    const int lb = a.blocks[blockIdx.x];
    if (lb < 0 || lb >= a.l.nbx * a.l.nby * a.l.nbz) return;
    const int i = (lb % a.l.nbx) * TSDF_SB + (threadIdx.x & 7), j = (lb / a.l.nbx % a.l.nby) * TSDF_SB + ((threadIdx.x >> 3) & 7),
              k = (lb / (a.l.nbx * a.l.nby)) * TSDF_SB + (threadIdx.x >> 6);
    if (i >= a.l.nx || j >= a.l.ny || k >= a.l.nz) return;
    const size_t n = (size_t)a.nblocks * TSDF_SB3, s = (size_t)blockIdx.x * TSDF_SB3 + threadIdx.x;
    const float x = a.ox + (float)i * a.voxel, y = a.oy + (float)j * a.voxel, z = a.oz + (float)k * a.voxel;
    tsdf_fold_sample(a, s, n, x, y, z);
}

extern "C" int pmn_tsdf_integrate_blocks(float* tsdf, float* weight, float* rgb, float* cweight, const int* blocks, int n_blocks,
                                         const int* dims_host, const float* origin_host, float voxel, float trunc, const float* maps,
                                         long long slot_stride, const int* slots_host, const int* hw_host, const void* const* masks_host,
                                         const void* const* images_host, const float* cams_host, int n_views, void* stream) {
    if (!tsdf || !weight || !blocks || !dims_host || !maps || !slots_host || !hw_host || !cams_host || slot_stride < 1) return PMN_ERR_ARG;
    if ((rgb == nullptr) != (cweight == nullptr)) return PMN_ERR_ARG;
    int rc = tsdf_check_grid(origin_host, voxel, trunc);
    if (rc != PMN_OK) return rc;
    if (n_views < 1 || n_views > PMN_TSDF_MAX_VIEWS || !tsdf_pool_size_ok(n_blocks)) return PMN_ERR_SHAPE;
    TsdfBlockArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = tsdf_lattice(a.l, dims_host)) != PMN_OK) return rc;
    a.tsdf = tsdf;
    a.weight = weight;
    a.rgb = rgb;
    a.cweight = cweight;
    a.blocks = blocks;
    a.nblocks = n_blocks;
    a.nviews = n_views;
    a.ox = origin_host[0];
    a.oy = origin_host[1];
    a.oz = origin_host[2];
    a.voxel = voxel;
    a.trunc = trunc;
    if ((rc = tsdf_fill_views(a.v, maps, slot_stride, slots_host, hw_host, masks_host, images_host, cams_host, n_views)) != PMN_OK) return rc;
    PMN_LAUNCH(tsdf_integrate_blocks_kernel, dim3(n_blocks), dim3(TSDF_SB3), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// Marching tetrahedra over the pool: the rule of mt_count_kernel / mt_emit_kernel with the block and its halo staged in LDS.  Counting
// reads the samples at -1 .. +1 of every sample, emitting (the gradients of both ends of an edge) at -1 .. +2: both stage the 11^3
// samples at block-local -1 .. 9 -- tsdf and the bit weight >= min_weight, 6.7 KB -- through the slots of the 27 blocks around, read
// from the table once per workgroup, instead of up to 20 table lookups per sample.
#define MT_HALO 11
#define MT_HALO3 (MT_HALO * MT_HALO * MT_HALO)

struct MtBlockArgs {
    const float *tsdf, *weight, *rgb, *cweight;
    const int *table, *blocks;
    int nblocks;
    TsdfLattice l;
    float ox, oy, oz, voxel, min_weight;
    unsigned char *vmask, *ntri;  // [B][8][8][8]; count: outputs; emit: inputs
    const int *vincl, *tincl;     // emit: INCLUSIVE scans of popcount(vmask) and of ntri in pool order
    float* vertices;
    unsigned char* colors;
    float* normals;
    int* faces;
};

struct MtTile {
    float t[MT_HALO3];
    unsigned char ok[MT_HALO3];
    int slot[27];    // of the blocks at -1 .. +1 per axis, x fastest; -1 = none
    int bi, bj, bk;  // this block
};

// block-local coordinates -1 .. 9 per axis
__device__ __forceinline__ int mt_tile_at(int li, int lj, int lk) { return ((lk + 1) * MT_HALO + (lj + 1)) * MT_HALO + (li + 1); }

// index in a pool plane of the sample at block-local (li, lj, lk), -8 .. 15 per axis; -1 where its block has no slot
__device__ __forceinline__ int mt_pool_at(const MtTile& m, int li, int lj, int lk) {
    const int slot = m.slot[(((lk + 8) >> 3) * 3 + ((lj + 8) >> 3)) * 3 + ((li + 8) >> 3)];
    return slot < 0 ? -1 : slot * TSDF_SB3 + (((lk & 7) * TSDF_SB + (lj & 7)) * TSDF_SB + (li & 7));
}

// false (for the whole workgroup) when the list entry is no block of the lattice
__device__ __forceinline__ bool mt_stage(const MtBlockArgs& a, MtTile& m) {
    const int lb = a.blocks[blockIdx.x];
    if (lb < 0 || lb >= a.l.nbx * a.l.nby * a.l.nbz) return false;
    const int bi = lb % a.l.nbx, bj = lb / a.l.nbx % a.l.nby, bk = lb / (a.l.nbx * a.l.nby);
    if (threadIdx.x < 27) {
        const int ni = bi + (int)threadIdx.x % 3 - 1, nj = bj + (int)threadIdx.x / 3 % 3 - 1, nk = bk + (int)threadIdx.x / 9 - 1;
        int slot = -1;
        if (ni >= 0 && nj >= 0 && nk >= 0 && ni < a.l.nbx && nj < a.l.nby && nk < a.l.nbz) {
            slot = a.table[((size_t)nk * a.l.nby + nj) * a.l.nbx + ni];
            if (slot >= a.nblocks) slot = -1;
        }
        m.slot[threadIdx.x] = slot;
    }
    if (threadIdx.x == 0) {
        m.bi = bi;
        m.bj = bj;
        m.bk = bk;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < MT_HALO3; e += TSDF_SB3) {
        const int li = e % MT_HALO - 1, lj = e / MT_HALO % MT_HALO - 1, lk = e / (MT_HALO * MT_HALO) - 1;
        const int gi = bi * TSDF_SB + li, gj = bj * TSDF_SB + lj, gk = bk * TSDF_SB + lk;
        float t = 1.0f;
        bool ok = false;
        if (gi >= 0 && gj >= 0 && gk >= 0 && gi < a.l.nx && gj < a.l.ny && gk < a.l.nz) {
            const int p = mt_pool_at(m, li, lj, lk);
            if (p >= 0) {
                t = a.tsdf[p];
                ok = a.weight[p] >= a.min_weight;
            }
        }
        m.t[e] = t;
        m.ok[e] = ok ? 1 : 0;
    }
    __syncthreads();
    return true;
}

// bit c = corner c of the cell at block-local (li, lj, lk) is inside (tsdf < 0)
__device__ __forceinline__ unsigned mt_tile_inside(const MtTile& m, int li, int lj, int lk) {
    unsigned in = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) in |= (m.t[mt_tile_at(li + (c & 1), lj + ((c >> 1) & 1), lk + (c >> 2))] < 0.0f ? 1u : 0u) << c;
    return in;
}

__global__ __launch_bounds__(TSDF_SB3) void mt_count_blocks_kernel(const MtBlockArgs a) {
    __shared__ MtTile m;
    const int li = threadIdx.x & 7, lj = (threadIdx.x >> 3) & 7, lk = threadIdx.x >> 6;
    const size_t s = (size_t)blockIdx.x * TSDF_SB3 + threadIdx.x;
    if (!mt_stage(a, m)) {  // the scans must not see what the caller's buffers held
        a.vmask[s] = 0;
        a.ntri[s] = 0;
        return;
    }
    unsigned okb = 0;  // as in mt_count_kernel: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
#pragma unroll
    for (int q = 0; q < 27; ++q) okb |= (unsigned)m.ok[mt_tile_at(li + q % 3 - 1, lj + (q / 3) % 3 - 1, lk + q / 9 - 1)] << q;
    unsigned live = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int bx = 1 - (c & 1), by = 1 - ((c >> 1) & 1), bz = 1 - (c >> 2);
        const unsigned need = (1u << (bz * 9 + by * 3 + bx)) * (1u | 2u | 8u | 16u | 512u | 1024u | 4096u | 8192u);
        live |= ((okb & need) == need ? 1u : 0u) << c;
    }
    unsigned mask = 0;
    if (live) {
        const bool in0 = m.t[mt_tile_at(li, lj, lk)] < 0.0f;
#pragma unroll
        for (int c = 1; c < 8; ++c) {
            unsigned users = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if ((q & c) == 0) users |= 1u << q;
            if (live & users) {
                const bool in1 = m.t[mt_tile_at(li + (c & 1), lj + ((c >> 1) & 1), lk + (c >> 2))] < 0.0f;
                if (in0 != in1) mask |= 1u << (c - 1);
            }
        }
    }
    a.vmask[s] = (unsigned char)mask;
    unsigned nt = 0;
    if (live & 1u) {
        const unsigned in = mt_tile_inside(m, li, lj, lk);
        if (in != 0u && in != 255u) {
#pragma unroll
            for (int t = 0; t < 6; ++t) nt += MT_CASES[mt_tet_case(in, t)].ntri;
        }
    }
    a.ntri[s] = (unsigned char)nt;
}

// central-difference gradient at block-local (li, lj, lk), 0 .. 8 per axis; false where a neighbour is outside or unobserved
__device__ __forceinline__ bool mt_tile_gradient(const MtTile& m, int li, int lj, int lk, float& gx, float& gy, float& gz) {
#pragma clang fp contract(off)
    const int c = mt_tile_at(li, lj, lk), sy = MT_HALO, sz = MT_HALO * MT_HALO;
    if (!(m.ok[c - 1] && m.ok[c + 1] && m.ok[c - sy] && m.ok[c + sy] && m.ok[c - sz] && m.ok[c + sz])) return false;
    gx = m.t[c + 1] - m.t[c - 1];
    gy = m.t[c + sy] - m.t[c - sy];
    gz = m.t[c + sz] - m.t[c - sz];
    return true;
}

__global__ __launch_bounds__(TSDF_SB3) void mt_emit_blocks_kernel(const MtBlockArgs a) {
#pragma clang fp contract(off)
    __shared__ MtTile m;
    const size_t n = (size_t)a.nblocks * TSDF_SB3, s = (size_t)blockIdx.x * TSDF_SB3 + threadIdx.x;
    const unsigned mask = a.vmask[s], nt = a.ntri[s];
    if (!__syncthreads_or((int)(mask | nt))) return;  // most blocks of the band hold no surface: nothing to stage
    if (!mt_stage(a, m)) return;
    const int li = threadIdx.x & 7, lj = (threadIdx.x >> 3) & 7, lk = threadIdx.x >> 6;
    const int i = m.bi * TSDF_SB + li, j = m.bj * TSDF_SB + lj, k = m.bk * TSDF_SB + lk;
    if (mask) {
        int out = a.vincl[s] - __popc(mask);
        const float v0 = m.t[mt_tile_at(li, lj, lk)];
        const float x0 = a.ox + (float)i * a.voxel, y0 = a.oy + (float)j * a.voxel, z0 = a.oz + (float)k * a.voxel;
        float g0x = 0.0f, g0y = 0.0f, g0z = 0.0f;
        const bool have_g0 = a.normals && mt_tile_gradient(m, li, lj, lk, g0x, g0y, g0z);
        for (int c = 1; c < 8; ++c) {
            if (!((mask >> (c - 1)) & 1u)) continue;
            const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
            const float v1 = m.t[mt_tile_at(li + dx, lj + dy, lk + dz)];
            const float t = v0 / (v0 - v1);
            const float x1 = a.ox + (float)(i + dx) * a.voxel, y1 = a.oy + (float)(j + dy) * a.voxel, z1 = a.oz + (float)(k + dz) * a.voxel;
            a.vertices[3 * (size_t)out + 0] = x0 + t * (x1 - x0);
            a.vertices[3 * (size_t)out + 1] = y0 + t * (y1 - y0);
            a.vertices[3 * (size_t)out + 2] = z0 + t * (z1 - z0);
            if (a.colors) {
                const int p1 = mt_pool_at(m, li + dx, lj + dy, lk + dz);  // observed, so its block has a slot
                const size_t s1 = p1 < 0 ? s : (size_t)p1;
                const float cw0 = a.cweight[s], cw1 = p1 < 0 ? 0.0f : a.cweight[s1];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float c0 = a.rgb[ch * n + s], c1 = a.rgb[ch * n + s1];
                    float cv = 128.0f;
                    if (cw0 > 0.0f && cw1 > 0.0f) cv = c0 + t * (c1 - c0);
                    else if (cw0 > 0.0f) cv = c0;
                    else if (cw1 > 0.0f) cv = c1;
                    cv = floorf(cv + 0.5f);
                    a.colors[3 * (size_t)out + ch] = (unsigned char)fminf(fmaxf(cv, 0.0f), 255.0f);
                }
            }
            if (a.normals) {
                float nx = 0.0f, ny = 0.0f, nz = 0.0f, g1x, g1y, g1z;
                if (have_g0 && mt_tile_gradient(m, li + dx, lj + dy, lk + dz, g1x, g1y, g1z)) {
                    const float gx = g0x + t * (g1x - g0x), gy = g0y + t * (g1y - g0y), gz = g0z + t * (g1z - g0z);
                    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
                    if (len > 0.0f && len < __builtin_inff()) {
                        nx = gx / len;
                        ny = gy / len;
                        nz = gz / len;
                    }
                }
                a.normals[3 * (size_t)out + 0] = nx;
                a.normals[3 * (size_t)out + 1] = ny;
                a.normals[3 * (size_t)out + 2] = nz;
            }
            ++out;
        }
    }
    if (nt) {
        int f = a.tincl[s] - (int)nt;
        const unsigned in = mt_tile_inside(m, li, lj, lk);
        for (int t = 0; t < 6; ++t) {
            const MtCase& cs = MT_CASES[mt_tet_case(in, t)];
            const bool neg = (MT_NEGATIVE >> t) & 1;
            for (int tri = 0; tri < cs.ntri; ++tri) {
                int idx[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const unsigned code = cs.edge[3 * tri + e];
                    const int lo = MT_TET[t][code & 3u], hi = MT_TET[t][code >> 2], cls = hi ^ lo;
                    const int owner = mt_pool_at(m, li + (lo & 1), lj + ((lo >> 1) & 1), lk + (lo >> 2));  // a corner of a live cell
                    const unsigned om = owner < 0 ? 0u : a.vmask[owner];
                    idx[e] = owner < 0 ? 0 : a.vincl[owner] - __popc(om) + __popc(om & ((1u << (cls - 1)) - 1u));
                }
                a.faces[3 * (size_t)f + 0] = idx[0];
                a.faces[3 * (size_t)f + 1] = neg ? idx[2] : idx[1];
                a.faces[3 * (size_t)f + 2] = neg ? idx[1] : idx[2];
                ++f;
            }
        }
    }
}

static int mt_blocks_fill(MtBlockArgs& a, const float* tsdf, const float* weight, const int* table, const int* blocks, int n_blocks,
                          const int* dims_host, const float* origin_host, float voxel, float min_weight) {
    if (!tsdf || !weight || !table || !blocks || !origin_host) return PMN_ERR_ARG;
    if (!(voxel > 0.0f) || !std::isfinite(voxel) || !(min_weight > 0.0f) || !std::isfinite(min_weight)) return PMN_ERR_ARG;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(origin_host[c])) return PMN_ERR_ARG;
    if (!tsdf_pool_size_ok(n_blocks)) return PMN_ERR_SHAPE;
    memset(&a, 0, sizeof(a));
    const int rc = tsdf_lattice(a.l, dims_host);
    if (rc != PMN_OK) return rc;
    a.tsdf = tsdf;
    a.weight = weight;
    a.table = table;
    a.blocks = blocks;
    a.nblocks = n_blocks;
    a.ox = origin_host[0];
    a.oy = origin_host[1];
    a.oz = origin_host[2];
    a.voxel = voxel;
    a.min_weight = min_weight;
    return PMN_OK;
}

extern "C" int pmn_mt_count_blocks(const float* tsdf, const float* weight, const int* table, const int* blocks, int n_blocks,
                                   const int* dims_host, float min_weight, unsigned char* vertex_mask, unsigned char* cell_triangles,
                                   void* stream) {
    static const float origin[3] = {0.0f, 0.0f, 0.0f};
    if (!vertex_mask || !cell_triangles) return PMN_ERR_ARG;
    MtBlockArgs a;
    const int rc = mt_blocks_fill(a, tsdf, weight, table, blocks, n_blocks, dims_host, origin, 1.0f, min_weight);
    if (rc != PMN_OK) return rc;
    a.vmask = vertex_mask;
    a.ntri = cell_triangles;
    PMN_LAUNCH(mt_count_blocks_kernel, dim3(n_blocks), dim3(TSDF_SB3), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_mt_emit_blocks(const float* tsdf, const float* weight, const float* rgb, const float* cweight, const int* table,
                                  const int* blocks, int n_blocks, const int* dims_host, const float* origin_host, float voxel,
                                  float min_weight, const unsigned char* vertex_mask, const unsigned char* cell_triangles,
                                  const int* vertex_scan, const int* triangle_scan, float* vertices, unsigned char* colors, float* normals,
                                  int* faces, void* stream) {
    if (!vertex_mask || !cell_triangles || !vertex_scan || !triangle_scan || !vertices || !faces) return PMN_ERR_ARG;
    if ((rgb == nullptr) != (cweight == nullptr) || (colors != nullptr && rgb == nullptr)) return PMN_ERR_ARG;
    MtBlockArgs a;
    const int rc = mt_blocks_fill(a, tsdf, weight, table, blocks, n_blocks, dims_host, origin_host, voxel, min_weight);
    if (rc != PMN_OK) return rc;
    a.rgb = rgb;
    a.cweight = cweight;
    a.vmask = const_cast<unsigned char*>(vertex_mask);
    a.ntri = const_cast<unsigned char*>(cell_triangles);
    a.vincl = vertex_scan;
    a.tincl = triangle_scan;
    a.vertices = vertices;
    a.colors = colors;
    a.normals = normals;
    a.faces = faces;
    PMN_LAUNCH(mt_emit_blocks_kernel, dim3(n_blocks), dim3(TSDF_SB3), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
