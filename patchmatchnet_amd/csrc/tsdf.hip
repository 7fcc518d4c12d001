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

// ---- the grid every entry point is told about ---------------------------------------------------------------------------------
// The block-sparse volume (section 18, below) cuts the lattice into blocks of 8 x 8 x 8 samples; its limits differ from the dense ones.
#define TSDF_SB 8                                   // samples per block side
#define TSDF_SB3 (TSDF_SB * TSDF_SB * TSDF_SB)      // samples per block = threads per workgroup
#define TSDF_MAX_AXIS (1 << 19)
#define TSDF_MAX_TABLE (1LL << 28)

struct TsdfLattice {
    int nx, ny, nz, nbx, nby, nbz;  // samples per axis; blocks per axis (a dense volume has none: 0)
};

// Lattice, placement and the one threshold of the call; every argument struct below derives from it.
struct TsdfGrid {
    TsdfLattice l;
    float ox, oy, oz, voxel;
    float trunc;       // integration and marking
    float min_weight;  // marching tetrahedra
};

// the dense lattice: n >= 1 per axis, nz <= 65535 (it is a launch grid's z), fewer than 2^31 samples
static int tsdf_dense_lattice(TsdfLattice& l, const int* dims_host) {
    l.nx = dims_host[0];
    l.ny = dims_host[1];
    l.nz = dims_host[2];
    if (l.nx < 1 || l.ny < 1 || l.nz < 1 || l.nz > 65535 || (long long)l.nx * l.ny * l.nz > 2147483647LL) return PMN_ERR_SHAPE;
    return PMN_OK;
}

// the virtual lattice of the block-sparse volume: 2 <= n < 2^19 per axis, at most 2^28 blocks
static int tsdf_lattice(TsdfLattice& l, const int* dims_host) {
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

static bool tsdf_positive(float v) { return v > 0.0f && std::isfinite(v); }

// Checks and fills what every entry point shares: the lattice (``blocks`` picks the virtual lattice's limits), a finite origin and a
// positive finite voxel.  The threshold's rule differs per entry point and stays with the caller.
static int tsdf_grid(TsdfGrid& g, bool blocks, const int* dims_host, const float* origin_host, float voxel) {
    if (!dims_host || !origin_host || !tsdf_positive(voxel)) return PMN_ERR_ARG;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(origin_host[c])) return PMN_ERR_ARG;
    const int rc = blocks ? tsdf_lattice(g.l, dims_host) : tsdf_dense_lattice(g.l, dims_host);
    if (rc != PMN_OK) return rc;
    g.ox = origin_host[0];
    g.oy = origin_host[1];
    g.oz = origin_host[2];
    g.voxel = voxel;
    return PMN_OK;
}

static dim3 tsdf_dense_launch(const TsdfLattice& l) { return dim3((l.nx + TSDF_BX - 1) / TSDF_BX, (l.ny + TSDF_BY - 1) / TSDF_BY, l.nz); }

static bool tsdf_pool_size_ok(int n_blocks) { return n_blocks >= 1 && (long long)n_blocks * TSDF_SB3 <= 2147483647LL; }

struct TsdfArgs : TsdfGrid {
    float *tsdf, *weight, *rgb, *cweight;
    int nviews;
    TsdfView v[PMN_TSDF_MAX_VIEWS];
};

struct TsdfBlockArgs : TsdfArgs {
    const int* blocks;  // the linear block index of every slot of the pool
    int nblocks;
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
    if (i >= a.l.nx || j >= a.l.ny) return;
    const size_t n = (size_t)a.l.nx * a.l.ny * a.l.nz, s = ((size_t)k * a.l.ny + j) * a.l.nx + i;
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

// what both integrate kernels are told (``a`` zeroed by the caller): the planes, the grid and the per-view block
static int tsdf_integrate_fill(TsdfArgs& a, bool blocks, float* tsdf, float* weight, float* rgb, float* cweight, const int* dims_host,
                               const float* origin_host, float voxel, float trunc, const float* maps, long long slot_stride,
                               const int* slots_host, const int* hw_host, const void* const* masks_host, const void* const* images_host,
                               const float* cams_host, int n_views) {
    if (!tsdf || !weight || !maps || !slots_host || !hw_host || !cams_host || slot_stride < 1) return PMN_ERR_ARG;
    if ((rgb == nullptr) != (cweight == nullptr) || !tsdf_positive(trunc)) return PMN_ERR_ARG;
    if (n_views < 1 || n_views > PMN_TSDF_MAX_VIEWS) return PMN_ERR_SHAPE;
    const int rc = tsdf_grid(a, blocks, dims_host, origin_host, voxel);
    if (rc != PMN_OK) return rc;
    a.tsdf = tsdf;
    a.weight = weight;
    a.rgb = rgb;
    a.cweight = cweight;
    a.nviews = n_views;
    a.trunc = trunc;
    return tsdf_fill_views(a.v, maps, slot_stride, slots_host, hw_host, masks_host, images_host, cams_host, n_views);
}

extern "C" int pmn_tsdf_integrate(float* tsdf, float* weight, float* rgb, float* cweight, const int* dims_host, const float* origin_host,
                                  float voxel, float trunc, const float* maps, long long slot_stride, const int* slots_host,
                                  const int* hw_host, const void* const* masks_host, const void* const* images_host,
                                  const float* cams_host, int n_views, void* stream) {
    TsdfArgs a;
    memset(&a, 0, sizeof(a));
    const int rc = tsdf_integrate_fill(a, false, tsdf, weight, rgb, cweight, dims_host, origin_host, voxel, trunc, maps, slot_stride,
                                       slots_host, hw_host, masks_host, images_host, cams_host, n_views);
    if (rc != PMN_OK) return rc;
    PMN_LAUNCH(tsdf_integrate_kernel, tsdf_dense_launch(a.l), dim3(256), 0, (hipStream_t)stream, a);
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

struct MtArgs : TsdfGrid {
    const float *tsdf, *weight, *rgb, *cweight;
    unsigned char *vmask, *ntri;  // count: outputs; emit: inputs
    const int *vincl, *tincl;     // emit: INCLUSIVE scans of popcount(vmask) and of ntri
    float* vertices;
    unsigned char* colors;
    float* normals;
    int* faces;
};

__device__ __forceinline__ unsigned mt_tet_case(unsigned in, int t) {
    return ((in >> MT_TET[t][0]) & 1u) | (((in >> MT_TET[t][1]) & 1u) << 1) | (((in >> MT_TET[t][2]) & 1u) << 2) |
           (((in >> MT_TET[t][3]) & 1u) << 3);
}

// The rule is written once, over a SAMPLER: the thread's own sample -- (i, j, k) in the lattice, ``self`` its index in a plane,
// ``planes`` the stride between the three colour planes -- and, for the sample at the offset (dx, dy, dz), -1 .. +2 per axis, from it:
//     ok(dx, dy, dz)     1 if it is observed (inside the lattice, present, weight >= min_weight), else 0
//     tsdf(dx, dy, dz)   its value; asked only where the rule has established that the sample is inside the lattice
//     index(dx, dy, dz)  its index in a plane; -1 where its block has no slot, which only a sampler with kHoles may answer
// MtDenseSampler reads the planes of a dense volume from global memory; MtPoolSampler (section 18, below) the LDS tile of a block.
struct MtDenseSampler {
    static constexpr bool kHoles = false;
    const MtArgs& a;
    const int i, j, k;
    const size_t self, planes;
    __device__ __forceinline__ MtDenseSampler(const MtArgs& a_, int i_, int j_, int k_)
        : a(a_), i(i_), j(j_), k(k_), self(((size_t)k_ * a_.l.ny + j_) * a_.l.nx + i_), planes((size_t)a_.l.nx * a_.l.ny * a_.l.nz) {}
    __device__ __forceinline__ size_t index(int dx, int dy, int dz) const {
        return ((size_t)(k + dz) * a.l.ny + (j + dy)) * a.l.nx + (i + dx);
    }
    __device__ __forceinline__ unsigned ok(int dx, int dy, int dz) const {
        const int x = i + dx, y = j + dy, z = k + dz;
        if (x < 0 || y < 0 || z < 0 || x >= a.l.nx || y >= a.l.ny || z >= a.l.nz) return 0u;
        return a.weight[index(dx, dy, dz)] >= a.min_weight ? 1u : 0u;
    }
    __device__ __forceinline__ float tsdf(int dx, int dy, int dz) const { return a.tsdf[index(dx, dy, dz)]; }
};

// bit c = corner c of the sample's cell is inside (tsdf < 0); the cell must lie in the lattice
template <class Sampler>
__device__ __forceinline__ unsigned mt_inside(const Sampler& s) {
    unsigned in = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) in |= (s.tsdf(c & 1, (c >> 1) & 1, c >> 2) < 0.0f ? 1u : 0u) << c;
    return in;
}

// One sample's share of the count: the mask of the edge classes that carry a vertex, and the triangles of its cell.
template <class Sampler>
__device__ __forceinline__ void mt_count_sample(const MtArgs& a, const Sampler& s) {
    // which samples of the 3 x 3 x 3 neighbourhood are observed: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
    unsigned okb = 0;
#pragma unroll
    for (int q = 0; q < 27; ++q) okb |= s.ok(q % 3 - 1, (q / 3) % 3 - 1, q / 9 - 1) << q;
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
        const bool in0 = s.tsdf(0, 0, 0) < 0.0f;
#pragma unroll
        for (int c = 1; c < 8; ++c) {
            unsigned users = 0;  // the cells that contain the edge of class c: m a subset of ~c
#pragma unroll
            for (int m = 0; m < 8; ++m)
                if ((m & c) == 0) users |= 1u << m;
            if (live & users) {  // then the far end is inside the lattice
                const bool in1 = s.tsdf(c & 1, (c >> 1) & 1, c >> 2) < 0.0f;
                if (in0 != in1) mask |= 1u << (c - 1);
            }
        }
    }
    a.vmask[s.self] = (unsigned char)mask;
    unsigned nt = 0;
    if (live & 1u) {
        const unsigned in = mt_inside(s);
        if (in != 0u && in != 255u) {
#pragma unroll
            for (int t = 0; t < 6; ++t) nt += MT_CASES[mt_tet_case(in, t)].ntri;
        }
    }
    a.ntri[s.self] = (unsigned char)nt;
}

template <class Index>
__device__ __forceinline__ int mt_vertex_index(const MtArgs& a, Index owner, int cls) {
    const unsigned m = a.vmask[owner];
    return a.vincl[owner] - __popc(m) + __popc(m & ((1u << (cls - 1)) - 1u));
}

// central-difference gradient of tsdf at the sample at (dx, dy, dz), 0 .. 1 per axis; false where a neighbour is outside the lattice or
// unobserved
template <class Sampler>
__device__ __forceinline__ bool mt_gradient(const Sampler& s, int dx, int dy, int dz, float& gx, float& gy, float& gz) {
#pragma clang fp contract(off)
    if (!(s.ok(dx - 1, dy, dz) && s.ok(dx + 1, dy, dz) && s.ok(dx, dy - 1, dz) && s.ok(dx, dy + 1, dz) && s.ok(dx, dy, dz - 1) &&
          s.ok(dx, dy, dz + 1)))
        return false;
    gx = s.tsdf(dx + 1, dy, dz) - s.tsdf(dx - 1, dy, dz);
    gy = s.tsdf(dx, dy + 1, dz) - s.tsdf(dx, dy - 1, dz);
    gz = s.tsdf(dx, dy, dz + 1) - s.tsdf(dx, dy, dz - 1);
    return true;
}

// The vertices the sample owns (mask = its vmask, non-zero): position, colour and normal of every class in the mask, in class order.
template <class Sampler>
__device__ __forceinline__ void mt_emit_vertices(const MtArgs& a, const Sampler& s, unsigned mask) {
#pragma clang fp contract(off)
    int out = a.vincl[s.self] - __popc(mask);
    const float v0 = s.tsdf(0, 0, 0);
    const float x0 = a.ox + (float)s.i * a.voxel, y0 = a.oy + (float)s.j * a.voxel, z0 = a.oz + (float)s.k * a.voxel;
    float g0x = 0.0f, g0y = 0.0f, g0z = 0.0f;
    const bool have_g0 = a.normals && mt_gradient(s, 0, 0, 0, g0x, g0y, g0z);
    for (int c = 1; c < 8; ++c) {
        if (!((mask >> (c - 1)) & 1u)) continue;
        const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
        const float v1 = s.tsdf(dx, dy, dz);
        const float t = v0 / (v0 - v1);
        const float x1 = a.ox + (float)(s.i + dx) * a.voxel, y1 = a.oy + (float)(s.j + dy) * a.voxel, z1 = a.oz + (float)(s.k + dz) * a.voxel;
        a.vertices[3 * (size_t)out + 0] = x0 + t * (x1 - x0);
        a.vertices[3 * (size_t)out + 1] = y0 + t * (y1 - y0);
        a.vertices[3 * (size_t)out + 2] = z0 + t * (z1 - z0);
        if (a.colors) {
            const auto p1 = s.index(dx, dy, dz);             // observed, so a pool has a slot for its block;
            const bool hole = Sampler::kHoles && p1 < 0;     // constant false for a sampler without holes
            const size_t s1 = hole ? s.self : (size_t)p1;
            const float cw0 = a.cweight[s.self], cw1 = hole ? 0.0f : a.cweight[s1];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float c0 = a.rgb[ch * s.planes + s.self], c1 = a.rgb[ch * s.planes + s1];
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
            if (have_g0 && mt_gradient(s, dx, dy, dz, g1x, g1y, g1z)) {
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

// The triangles of the sample's cell (nt = its ntri, non-zero), by tetrahedron, then triangle.
template <class Sampler>
__device__ __forceinline__ void mt_emit_faces(const MtArgs& a, const Sampler& s, unsigned nt) {
    int f = a.tincl[s.self] - (int)nt;
    const unsigned in = mt_inside(s);
    for (int t = 0; t < 6; ++t) {
        const MtCase& cs = MT_CASES[mt_tet_case(in, t)];
        const bool neg = (MT_NEGATIVE >> t) & 1;
        for (int tri = 0; tri < cs.ntri; ++tri) {
            int idx[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const unsigned code = cs.edge[3 * tri + e];
                const int lo = MT_TET[t][code & 3u], hi = MT_TET[t][code >> 2];
                const auto owner = s.index(lo & 1, (lo >> 1) & 1, lo >> 2);  // a corner of a live cell, so a pool has its block
                idx[e] = Sampler::kHoles && owner < 0 ? 0 : mt_vertex_index(a, owner, hi ^ lo);
            }
            a.faces[3 * (size_t)f + 0] = idx[0];
            a.faces[3 * (size_t)f + 1] = neg ? idx[2] : idx[1];
            a.faces[3 * (size_t)f + 2] = neg ? idx[1] : idx[2];
            ++f;
        }
    }
}

__global__ __launch_bounds__(256) void mt_count_kernel(const MtArgs a) {
    const int i = blockIdx.x * TSDF_BX + (threadIdx.x & 63), j = blockIdx.y * TSDF_BY + (threadIdx.x >> 6), k = blockIdx.z;
    if (i >= a.l.nx || j >= a.l.ny) return;
    mt_count_sample(a, MtDenseSampler(a, i, j, k));
}

__global__ __launch_bounds__(256) void mt_emit_kernel(const MtArgs a) {
    const int i = blockIdx.x * TSDF_BX + (threadIdx.x & 63), j = blockIdx.y * TSDF_BY + (threadIdx.x >> 6), k = blockIdx.z;
    if (i >= a.l.nx || j >= a.l.ny) return;
    const MtDenseSampler s(a, i, j, k);
    const unsigned mask = a.vmask[s.self];
    if (mask) mt_emit_vertices(a, s, mask);
    const unsigned nt = a.ntri[s.self];
    if (nt) mt_emit_faces(a, s, nt);
}

// What count and emit share (``a`` zeroed by the caller).  A pool sample without a slot has weight 0 and must stay unobserved, so
// there min_weight must be positive.
static int mt_fill(MtArgs& a, bool blocks, const float* tsdf, const float* weight, const int* dims_host, const float* origin_host,
                   float voxel, float min_weight, const unsigned char* vertex_mask, const unsigned char* cell_triangles) {
    if (!tsdf || !weight || !vertex_mask || !cell_triangles) return PMN_ERR_ARG;
    if (blocks ? !tsdf_positive(min_weight) : !std::isfinite(min_weight)) return PMN_ERR_ARG;
    const int rc = tsdf_grid(a, blocks, dims_host, origin_host, voxel);
    if (rc != PMN_OK) return rc;
    a.tsdf = tsdf;
    a.weight = weight;
    a.min_weight = min_weight;
    a.vmask = const_cast<unsigned char*>(vertex_mask);
    a.ntri = const_cast<unsigned char*>(cell_triangles);
    return PMN_OK;
}

// what emit adds to mt_fill
static int mt_fill_emit(MtArgs& a, const float* rgb, const float* cweight, const int* vertex_scan, const int* triangle_scan,
                        float* vertices, unsigned char* colors, float* normals, int* faces) {
    if (!vertex_scan || !triangle_scan || !vertices || !faces) return PMN_ERR_ARG;
    if ((rgb == nullptr) != (cweight == nullptr) || (colors != nullptr && rgb == nullptr)) return PMN_ERR_ARG;
    a.rgb = rgb;
    a.cweight = cweight;
    a.vincl = vertex_scan;
    a.tincl = triangle_scan;
    a.vertices = vertices;
    a.colors = colors;
    a.normals = normals;
    a.faces = faces;
    return PMN_OK;
}

static const float MT_NO_ORIGIN[3] = {0.0f, 0.0f, 0.0f};  // counting places nothing

extern "C" int pmn_mt_count(const float* tsdf, const float* weight, const int* dims_host, float min_weight, unsigned char* vertex_mask,
                            unsigned char* cell_triangles, void* stream) {
    MtArgs a;
    memset(&a, 0, sizeof(a));
    const int rc = mt_fill(a, false, tsdf, weight, dims_host, MT_NO_ORIGIN, 1.0f, min_weight, vertex_mask, cell_triangles);
    if (rc != PMN_OK) return rc;
    PMN_LAUNCH(mt_count_kernel, tsdf_dense_launch(a.l), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_mt_emit(const float* tsdf, const float* weight, const float* rgb, const float* cweight, const int* dims_host,
                           const float* origin_host, float voxel, float min_weight, const unsigned char* vertex_mask,
                           const unsigned char* cell_triangles, const int* vertex_scan, const int* triangle_scan, float* vertices,
                           unsigned char* colors, float* normals, int* faces, void* stream) {
    MtArgs a;
    memset(&a, 0, sizeof(a));
    int rc = mt_fill(a, false, tsdf, weight, dims_host, origin_host, voxel, min_weight, vertex_mask, cell_triangles);
    if (rc == PMN_OK) rc = mt_fill_emit(a, rgb, cweight, vertex_scan, triangle_scan, vertices, colors, normals, faces);
    if (rc != PMN_OK) return rc;
    PMN_LAUNCH(mt_emit_kernel, tsdf_dense_launch(a.l), dim3(256), 0, (hipStream_t)stream, a);
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
// (TSDF_SB, the lattice limits and the pool's argument struct of the integration are with the grid, at the top.)
//
// Marking: a thread per pixel of every view of the launch (blockIdx.y = the view, so the view block is read with scalar loads).  The
// samples that pmn_tsdf_integrate maps to a valid pixel (u, v) of depth d with |sdf| <= trunc lie in the section of the pyramid through
// the pixel's corners (u +- 0.5, v +- 0.5) between the camera depths max(d - trunc, 0) (0 = the apex: a superset of any positive clamp
// and free of a unit) and d + trunc.  Its eight corners go to the world through K^-1 and E^-1 (v.cam holds K^-1 row-major, then the
// upper 3 x 4 of E^-1, inverted on the host in float64); their axis-aligned box grown by one voxel and clipped to the lattice gives the
// blocks.  flags get plain byte stores of 1: whichever thread writes, the byte is 1.
struct TsdfMarkArgs : TsdfGrid {
    unsigned char* flags;  // [nbz][nby][nbx]
    int* overflow;
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

extern "C" int pmn_tsdf_mark_blocks(unsigned char* flags, int* overflow, const int* dims_host, const float* origin_host, float voxel,
                                    float trunc, const float* maps, long long slot_stride, const int* slots_host, const int* hw_host,
                                    const void* const* masks_host, const float* inv_cams_host, int n_views, void* stream) {
    if (!flags || !overflow || !maps || !slots_host || !hw_host || !inv_cams_host || slot_stride < 1 || !tsdf_positive(trunc)) return PMN_ERR_ARG;
    if (n_views < 1 || n_views > PMN_TSDF_MAX_VIEWS) return PMN_ERR_SHAPE;
    TsdfMarkArgs a;
    memset(&a, 0, sizeof(a));
    int rc = tsdf_grid(a, true, dims_host, origin_host, voxel);
    if (rc != PMN_OK) return rc;
    a.flags = flags;
    a.overflow = overflow;
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
    if (!blocks) return PMN_ERR_ARG;
    if (!tsdf_pool_size_ok(n_blocks)) return PMN_ERR_SHAPE;
    TsdfBlockArgs a;
    memset(&a, 0, sizeof(a));
    const int rc = tsdf_integrate_fill(a, true, tsdf, weight, rgb, cweight, dims_host, origin_host, voxel, trunc, maps, slot_stride,
                                       slots_host, hw_host, masks_host, images_host, cams_host, n_views);
    if (rc != PMN_OK) return rc;
    a.blocks = blocks;
    a.nblocks = n_blocks;
    PMN_LAUNCH(tsdf_integrate_blocks_kernel, dim3(n_blocks), dim3(TSDF_SB3), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// Marching tetrahedra over the pool: mt_count_sample / mt_emit_vertices / mt_emit_faces, the very code of the dense kernels, over a
// sampler that reads the block and its halo from LDS.  Counting reads the samples at -1 .. +1 of every sample, emitting (the gradients
// of both ends of an edge) at -1 .. +2: both stage the 11^3 samples at block-local -1 .. 9 -- tsdf and the bit weight >= min_weight,
// 6.7 KB -- through the slots of the 27 blocks around, read from the table once per workgroup, instead of up to 20 table lookups per
// sample.
#define MT_HALO 11
#define MT_HALO3 (MT_HALO * MT_HALO * MT_HALO)

struct MtBlockArgs : MtArgs {  // the planes are the pool's: [B][8][8][8], the scans in pool order
    const int *table, *blocks;
    int nblocks;
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

// the sampler of mt_count_sample / mt_emit_* over a staged tile: neighbours come from LDS, plane indices through the 27 slots
struct MtPoolSampler {
    static constexpr bool kHoles = true;
    const MtTile& m;
    const int li, lj, lk;  // block-local
    const int i, j, k;
    const size_t self, planes;
    __device__ __forceinline__ MtPoolSampler(const MtBlockArgs& a, const MtTile& m_, size_t self_)
        : m(m_), li(threadIdx.x & 7), lj((threadIdx.x >> 3) & 7), lk(threadIdx.x >> 6), i(m_.bi * TSDF_SB + li), j(m_.bj * TSDF_SB + lj),
          k(m_.bk * TSDF_SB + lk), self(self_), planes((size_t)a.nblocks * TSDF_SB3) {}
    __device__ __forceinline__ int index(int dx, int dy, int dz) const { return mt_pool_at(m, li + dx, lj + dy, lk + dz); }
    __device__ __forceinline__ unsigned ok(int dx, int dy, int dz) const { return m.ok[mt_tile_at(li + dx, lj + dy, lk + dz)]; }
    __device__ __forceinline__ float tsdf(int dx, int dy, int dz) const { return m.t[mt_tile_at(li + dx, lj + dy, lk + dz)]; }
};

__global__ __launch_bounds__(TSDF_SB3) void mt_count_blocks_kernel(const MtBlockArgs a) {
    __shared__ MtTile m;
    const size_t s = (size_t)blockIdx.x * TSDF_SB3 + threadIdx.x;
    if (!mt_stage(a, m)) {  // the scans must not see what the caller's buffers held
        a.vmask[s] = 0;
        a.ntri[s] = 0;
        return;
    }
    mt_count_sample(a, MtPoolSampler(a, m, s));
}

__global__ __launch_bounds__(TSDF_SB3) void mt_emit_blocks_kernel(const MtBlockArgs a) {
    __shared__ MtTile m;
    const size_t s = (size_t)blockIdx.x * TSDF_SB3 + threadIdx.x;
    const unsigned mask = a.vmask[s], nt = a.ntri[s];
    if (!__syncthreads_or((int)(mask | nt))) return;  // most blocks of the band hold no surface: nothing to stage
    if (!mt_stage(a, m)) return;
    const MtPoolSampler smp(a, m, s);
    if (mask) mt_emit_vertices(a, smp, mask);
    if (nt) mt_emit_faces(a, smp, nt);
}

// mt_fill, then what the pool adds
static int mt_blocks_fill(MtBlockArgs& a, const float* tsdf, const float* weight, const int* table, const int* blocks, int n_blocks,
                          const int* dims_host, const float* origin_host, float voxel, float min_weight, const unsigned char* vertex_mask,
                          const unsigned char* cell_triangles) {
    if (!table || !blocks) return PMN_ERR_ARG;
    if (!tsdf_pool_size_ok(n_blocks)) return PMN_ERR_SHAPE;
    a.table = table;
    a.blocks = blocks;
    a.nblocks = n_blocks;
    return mt_fill(a, true, tsdf, weight, dims_host, origin_host, voxel, min_weight, vertex_mask, cell_triangles);
}

extern "C" int pmn_mt_count_blocks(const float* tsdf, const float* weight, const int* table, const int* blocks, int n_blocks,
                                   const int* dims_host, float min_weight, unsigned char* vertex_mask, unsigned char* cell_triangles,
                                   void* stream) {
    MtBlockArgs a;
    memset(&a, 0, sizeof(a));
    const int rc = mt_blocks_fill(a, tsdf, weight, table, blocks, n_blocks, dims_host, MT_NO_ORIGIN, 1.0f, min_weight, vertex_mask,
                                  cell_triangles);
    if (rc != PMN_OK) return rc;
    PMN_LAUNCH(mt_count_blocks_kernel, dim3(n_blocks), dim3(TSDF_SB3), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_mt_emit_blocks(const float* tsdf, const float* weight, const float* rgb, const float* cweight, const int* table,
                                  const int* blocks, int n_blocks, const int* dims_host, const float* origin_host, float voxel,
                                  float min_weight, const unsigned char* vertex_mask, const unsigned char* cell_triangles,
                                  const int* vertex_scan, const int* triangle_scan, float* vertices, unsigned char* colors, float* normals,
                                  int* faces, void* stream) {
    MtBlockArgs a;
    memset(&a, 0, sizeof(a));
    int rc = mt_blocks_fill(a, tsdf, weight, table, blocks, n_blocks, dims_host, origin_host, voxel, min_weight, vertex_mask, cell_triangles);
    if (rc == PMN_OK) rc = mt_fill_emit(a, rgb, cweight, vertex_scan, triangle_scan, vertices, colors, normals, faces);
    if (rc != PMN_OK) return rc;
    PMN_LAUNCH(mt_emit_blocks_kernel, dim3(n_blocks), dim3(TSDF_SB3), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
