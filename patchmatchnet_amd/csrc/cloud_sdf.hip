// cloud_sdf.hip -- a signed distance from an ORIENTED point cloud, written into the pool planes of the block-sparse volume (tsdf.hip,
// DESIGN.md section 18) so that pmn_mt_count_blocks / pmn_mt_emit_blocks mesh a cloud as they mesh integrated depth maps (DESIGN.md
// section 32; include/pmn_hip.h states every operation; tests/cloud_sdf_ref.py repeats them in numpy).
//
// Per lattice sample of the listed blocks: the k nearest points within `radius` (pc_grid.hpp: the shell walk and the register-resident
// k-best list of pmn_knn_distance, unchanged), then f = sum_j w_j n_j . (x - p_j) / sum_j w_j with the polynomial weight
// w = (1 - d2 / R2)^4 -- an implicit moving-least-squares surface (Hoppe et al. 1992's signed distance to tangent planes, blended as
// in Kolluri 2005) -- summed in RANK order by the lane that found the neighbours, as knn_normals_kernel does: the lists are never
// written, and the result does not depend on the search grid.  No exp, no rsqrt: every operation is an IEEE float64 +, -, *, / that
// numpy repeats bit for bit.
//
// Launch: one lane per sample, one ONE-WAVE workgroup per 8 x 8 layer of a block (blockIdx.x = slot * 8 + layer): the 64 lanes are
// spatial neighbours at most 7 voxels apart, so they walk the same cells, their binary searches read the same keys (broadcasts and L2
// hits) and no order array is needed; and, as in pointcloud.hip, a layer with a long walk holds up nobody but itself.  A wave writes 256
// contiguous bytes of every pool plane.  The plain walk is kept: a variant that stages a block's candidates in LDS was not built
// (DESIGN.md section 32 says why).
#include "pc_grid.hpp"

#define SDF_SB 8                            // samples per block side (tsdf.hip TSDF_SB)
#define SDF_SB3 (SDF_SB * SDF_SB * SDF_SB)  // samples per block
#define SDF_MAX_AXIS (1 << 19)              // the virtual lattice's limits (tsdf.hip TSDF_MAX_AXIS, TSDF_MAX_TABLE)
#define SDF_MAX_TABLE (1LL << 28)

struct CloudSdfArgs {
    GridArgs g;
    const float* normals;         // [n][3], the grid's sorted order
    const unsigned char* colors;  // [n][3] or null
    const int* blocks;            // [nblocks]
    int nblocks;
    int nx, ny, nz, nbx, nby, nbz;
    float ox, oy, oz, voxel, trunc;
    int k;
    double radius, boundary;
    float *tsdf, *weight, *rgb, *cweight;  // pool planes; rgb and cweight both or neither
};

template <int CAP>
__global__ __launch_bounds__(64) void cloud_sdf_blocks_kernel(const CloudSdfArgs a) {
#pragma clang fp contract(off)
    const int slot = blockIdx.x >> 3, lk = blockIdx.x & 7;
    if (slot >= a.nblocks) return;
    const int lb = a.blocks[slot];
    if (lb < 0 || lb >= a.nbx * a.nby * a.nbz) return;
    const int i = (lb % a.nbx) * SDF_SB + (threadIdx.x & 7), j = (lb / a.nbx % a.nby) * SDF_SB + (threadIdx.x >> 3),
              kk = (lb / (a.nbx * a.nby)) * SDF_SB + lk;
    if (i >= a.nx || j >= a.ny || kk >= a.nz) return;  // a border block's overhang: outside the lattice, never written
    const size_t planes = (size_t)a.nblocks * SDF_SB3, s = (size_t)slot * SDF_SB3 + (size_t)lk * (SDF_SB * SDF_SB) + threadIdx.x;
    // the sample's position as tsdf.hip forms it, in float32; everything after is float64
    const float xf = a.ox + (float)i * a.voxel, yf = a.oy + (float)j * a.voxel, zf = a.oz + (float)kk * a.voxel;
    const double qx = (double)xf, qy = (double)yf, qz = (double)zf;
    const double R2 = a.radius * a.radius;
    KBest<CAP> b;
    b.init(a.k, R2, -1);
    pc_walk(a.g, qx, qy, qz, b);
    double sw = 0.0, sws = 0.0, cr = 0.0, cg = 0.0, cb = 0.0, d2_0 = 0.0, s_0 = 0.0;
    int c = 0;
#pragma unroll
    for (int t = 0; t < CAP; ++t) {  // static register; a sentinel (-2) or capped (-1) slot is no neighbour; ascending slot = rank order
        const int n = b.idx[t];
        if (n < 0) continue;
        const float* p = a.g.xyz + (size_t)n * 3;
        const float* m = a.normals + (size_t)n * 3;
        const double u = 1.0 - b.d2[t] / R2;
        const double u2 = u * u;
        const double w = u2 * u2;
        const double sj = ((double)m[0] * (qx - (double)p[0]) + (double)m[1] * (qy - (double)p[1])) + (double)m[2] * (qz - (double)p[2]);
        if (c == 0) {
            d2_0 = b.d2[t];
            s_0 = sj;
        }
        sw += w;
        sws += w * sj;
        if (a.colors) {
            const unsigned char* col = a.colors + (size_t)n * 3;
            cr += w * (double)col[0];
            cg += w * (double)col[1];
            cb += w * (double)col[2];
        }
        ++c;
    }
    // Hoppe's rule for open boundaries: the nearest point's tangent plane must be met within `boundary` of the point
    const double t2 = d2_0 - s_0 * s_0;
    const bool observed = c > 0 && sw > 0.0 && !(t2 > a.boundary * a.boundary);
    float tsdf = 1.0f, weight = 0.0f, r = 0.0f, g = 0.0f, bl = 0.0f;
    if (observed) {
        tsdf = (float)fmin(1.0, fmax(-1.0, (sws / sw) / (double)a.trunc));
        weight = (float)c;
        r = (float)(cr / sw);
        g = (float)(cg / sw);
        bl = (float)(cb / sw);
    }
    a.tsdf[s] = tsdf;
    a.weight[s] = weight;
    if (a.rgb) {
        a.rgb[s] = r;
        a.rgb[planes + s] = g;
        a.rgb[2 * planes + s] = bl;
        a.cweight[s] = weight;
    }
}

extern "C" int pmn_cloud_sdf_blocks(const float* to_xyz, const long long* to_keys, long long n_to, const double* origin_host, double cell,
                                    const int* dims_host, const float* normals, const unsigned char* colors, const int* blocks,
                                    int n_blocks, const int* volume_dims_host, const float* volume_origin_host, float voxel, float trunc,
                                    int k, double radius, double boundary, float* tsdf, float* weight, float* rgb, float* cweight,
                                    void* stream) {
    CloudSdfArgs a;
    const int rc = grid_args(a.g, to_xyz, to_keys, n_to, origin_host, cell, dims_host);
    if (rc != PMN_OK) return rc;
    if (!normals || !blocks || !volume_dims_host || !volume_origin_host || !tsdf || !weight || !pc_k_ok(k)) return PMN_ERR_ARG;
    if ((rgb == nullptr) != (cweight == nullptr) || (colors == nullptr) != (rgb == nullptr)) return PMN_ERR_ARG;
    if (!(voxel > 0.0f) || !std::isfinite(voxel) || !(trunc > 0.0f) || !std::isfinite(trunc)) return PMN_ERR_ARG;
    if (!pc_reach_square_ok(radius) || !pc_reach_ok(boundary)) return PMN_ERR_ARG;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(volume_origin_host[c])) return PMN_ERR_ARG;
    // the virtual lattice and the pool, with tsdf.hip's limits
    a.nx = volume_dims_host[0];
    a.ny = volume_dims_host[1];
    a.nz = volume_dims_host[2];
    if (a.nx < 2 || a.ny < 2 || a.nz < 2 || a.nx >= SDF_MAX_AXIS || a.ny >= SDF_MAX_AXIS || a.nz >= SDF_MAX_AXIS) return PMN_ERR_SHAPE;
    a.nbx = (a.nx + SDF_SB - 1) / SDF_SB;
    a.nby = (a.ny + SDF_SB - 1) / SDF_SB;
    a.nbz = (a.nz + SDF_SB - 1) / SDF_SB;
    if ((long long)a.nbx * a.nby * a.nbz > SDF_MAX_TABLE) return PMN_ERR_SHAPE;
    if (n_blocks < 1 || (long long)n_blocks * SDF_SB3 > 2147483647LL) return PMN_ERR_SHAPE;
    a.normals = normals;
    a.colors = colors;
    a.blocks = blocks;
    a.nblocks = n_blocks;
    a.ox = volume_origin_host[0];
    a.oy = volume_origin_host[1];
    a.oz = volume_origin_host[2];
    a.voxel = voxel;
    a.trunc = trunc;
    a.k = k;
    a.radius = radius;
    a.boundary = boundary;
    a.tsdf = tsdf;
    a.weight = weight;
    a.rgb = rgb;
    a.cweight = cweight;
    const dim3 grid((unsigned)n_blocks * SDF_SB);  // < 2^25
    PMN_LAUNCH_KBEST(k, cloud_sdf_blocks_kernel<CAP>, grid, dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
