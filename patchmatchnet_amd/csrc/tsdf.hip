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

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const TsdfArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * TSDF_BX + (threadIdx.x & 63), j = blockIdx.y * TSDF_BY + (threadIdx.x >> 6), k = blockIdx.z;
    if (i >= a.nx || j >= a.ny) return;
    const size_t n = (size_t)a.nx * a.ny * a.nz, s = ((size_t)k * a.ny + j) * a.nx + i;
    const float x = a.ox + (float)i * a.voxel, y = a.oy + (float)j * a.voxel, z = a.oz + (float)k * a.voxel;
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
    for (int v = 0; v < n_views; ++v) {
        const int h = hw_host[2 * v], w = hw_host[2 * v + 1];
        if (slots_host[v] < 0 || h < 1 || w < 1 || (long long)h * w > slot_stride) return PMN_ERR_ARG;
        a.v[v].depth = maps + (size_t)slots_host[v] * (size_t)slot_stride;
        a.v[v].mask = masks_host ? (const unsigned char*)masks_host[v] : nullptr;
        a.v[v].image = images_host ? (const unsigned char*)images_host[v] : nullptr;
        a.v[v].h = h;
        a.v[v].w = w;
        for (int c = 0; c < 21; ++c) {
            if (!std::isfinite(cams_host[21 * v + c])) return PMN_ERR_ARG;
            a.v[v].cam[c] = cams_host[21 * v + c];
        }
    }
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
