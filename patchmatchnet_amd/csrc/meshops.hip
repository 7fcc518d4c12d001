// meshops.hip -- operations on an indexed triangle mesh: the connected components of its vertices, and points drawn
// on its triangles at a fixed density per unit area.  The reference has neither; tests/meshops_ref.py restates everything below in numpy
// and is the yardstick.  A mesh is faces [Nt][3] int32 into vertices [Nv][3] float32.  A face with an index outside [0, Nv) is never
// dereferenced: the kernel that meets it skips it and adds 1 to *invalid (int32, zeroed by the caller), which the caller reads together
// with the host read it needs anyway.
//
// Components (pmn_mesh_components).  label[v] = the smallest vertex index of v's component; two vertices are connected when a face names
// both.  Union-find in global memory, parent = label itself, three launches:
//   init     parent[v] = v
//   hook     a thread per face unites (a, b) and (b, c): find the two roots; if they differ, compare-and-swap the LARGER root's slot from
//            itself to the smaller root; if the swap fails the slot is no root any more and the value it returned (< the old root) is
//            where the search goes on
//   flatten  parent[v] = the root of v
// Every value ever stored in slot v is <= v, and < v once v is no root (init stores v; a hook stores a smaller root; halving stores a
// smaller ancestor).  So (1) every walk towards a root strictly descends and ends after at most v steps WHATEVER it reads -- a stale
// line can cost steps, never a cycle; (2) a failed swap returns a smaller index, so the sum of the two indices a unite holds falls with
// every retry and the retry loop ends; (3) no lane ever waits for another lane: there is no lock, no flag, no spin, only the restart from
// the value a failed swap returned.  A unite returns only when both ends had one root or its own swap joined them, links are never
// removed (halving replaces a link by a link to an ancestor), so after the hook launch the trees are the components, and a tree's root,
// being smaller than all its descendants, is the component's minimum: the result is a function of the mesh alone -- not of the face
// order, the launch shape, the interleaving or the run.  All accesses of parent[] in hook and flatten are relaxed agent-scope atomics
// (loads that bypass the per-CU L1, a 32-bit compare-and-swap, 32-bit stores); flatten is a launch of its own and so sees everything
// hook wrote.  Integer atomics only.
//
// Sampling (pmn_mesh_face_samples, then the caller's inclusive int64 scan, then pmn_mesh_sample).  All randomness is a function of
// (seed, face, k), k = the sample's rank in its face, through the splitmix64 finaliser
//   mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31           (mod 2^64)
//   h = mix(mix(seed + G) + (((uint64)face << 32 | k) + 1) * G),   G = 0x9E3779B97F4A7C15
//   r1 = (float)(h >> 40) * 2^-24,   r2 = (float)((h >> 16) & 0xFFFFFF) * 2^-24        integers below 2^24 times 2^-24: exact, in [0, 1)
// No state, nothing depends on a thread or a launch shape.  Float32, nothing contracted, IEEE sqrtf:
//   count    e1 = B - A, e2 = C - A;  c = (e1.y e2.z - e1.z e2.y,  e1.z e2.x - e1.x e2.z,  e1.x e2.y - e1.y e2.x);
//            area = sqrtf((c.x c.x + c.y c.y) + c.z c.z) * 0.5f;  n_f = floor((double)area * density + (double)u_f) in float64 (two
//            roundings), u_f = the r1 of k = 2^32 - 1 (unbiased rounding); an area that is not finite or not > 0 gives 0; clamped at
//            2^31 - 1
//   emit     a thread per SAMPLE i: f = the first face whose inclusive scan exceeds i (binary search), k = i - scan[f - 1];
//            s = sqrtf(r1);  b0 = 1 - s;  b1 = s * (1 - r2);  b2 = s * r2;  p = (b0 * A + b1 * B) + b2 * C per coordinate; a colour
//            channel is the same blend of the three bytes as floats, floorf(c + 0.5f) clamped to 0..255 (as pmn_mt_emit rounds)
// Samples are ordered by face, then k.
//
// Distance to the surface (pmn_mesh_distance).  For every query the minimum over ALL faces of the exact
// point-triangle distance, the face that attains it and the nearest point on it.  Float64 from the float32 vertices, nothing contracted,
// IEEE division and sqrt; A, B, C the face's vertices in its order, every sum of three products left to right in x, y, z order:
//   segment(P, Q)  e = Q - P, w = q - P;  l2 = e.e;  t = l2 > 0 ? (w.e) / l2 : 0, clamped to [0, 1];  c = P + t * e;  d2 = |q - c|^2
//   plane          e1 = B - A, e2 = C - A, n = e1 x e2, nn = n.n, w = q - A;  only if nn > 0:  u = ((e1 x w).n) / nn,
//                  v = ((w x e2).n) / nn;  only if u >= 0, v >= 0 and u + v <= 1:  s = (w.n) / nn;  c = q - s * n;  d2 = (w.n)(w.n) / nn
//   face           the least d2 of segment(A, B), segment(B, C), segment(C, A), plane, in this order, the first among equals
// A face without area is thereby the union of its segments (a segment, or a point), never an error, and a face's value is a function of
// (its three vertices, q) alone.  Among faces with bit-equal d2 the lower face index wins, so the result is a function of (mesh, query).
//
// Search.  The caller (meshops.build_face_grid) sorts REFERENCE POINTS of the faces into an ordinary grid (pc_grid.hpp) -- the centroids of
// a face's conceptual 4^L midpoint split, every one labelled with the ORIGINAL face (entry_face) -- and states a covering radius R: every
// point of every face lies within R of one of that face's reference points as stored (float32).  The shell walk runs over the reference
// points with the accumulator MeshBest.  Why the result is the true minimum: let the walk end with best distance b, and suppose a face F
// has a point p with |q - p| = d < b (or d = b bit-equal with a lower index).  Some reference point r of F has |p - r| <= R, hence
// |q - r| <= d + R <= b + R.  The walk skips a region only when its lower bound g exceeds (sqrt(best) + R)(1 + 2^-20) for the best OF
// THAT MOMENT, which is never below b; offer() skips r under the same test.  So r was offered, F evaluated, and F's value d compared with
// the best -- a contradiction.  Skipping the face that already is the best is safe because a face's value does not depend on the entry.
// One lane per query in the order of the queries' cells, one-wave workgroups (pointcloud.hip says why); the state of a lane is the best
// d2, its face, three doubles of closest point and the bound: no array, no scratch.
#include <cmath>

#include "pc_grid.hpp"
#include "union_find.hpp"

__device__ __forceinline__ bool mesh_index_ok(int v, int nv) { return (unsigned)v < (unsigned)nv; }

// ---- components ------------------------------------------------------------------------------------------------------------------

// init, find, unite and flatten: union_find.hpp (shared with cloud_cluster.hip)

__global__ __launch_bounds__(256) void mesh_cc_hook_kernel(const int* __restrict__ faces, int nt, int nv, int* parent, int* invalid) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nt) return;
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if (!(mesh_index_ok(a, nv) && mesh_index_ok(b, nv) && mesh_index_ok(c, nv))) {
        atomicAdd(invalid, 1);
        return;
    }
    if (a != b) mesh_cc_unite(parent, a, b);
    if (b != c) mesh_cc_unite(parent, b, c);
}

extern "C" int pmn_mesh_components(const int* faces, int n_faces, int n_vertices, int* label, int* invalid, void* stream) {
    if (!label || !invalid || (n_faces > 0 && !faces)) return PMN_ERR_ARG;
    if (n_faces < 0 || n_vertices < 1 || n_vertices > 2147483647 - 255 || n_faces > 2147483647 - 255) return PMN_ERR_SHAPE;
    const dim3 vgrid((unsigned)((n_vertices + 255) / 256));
    PMN_LAUNCH(mesh_cc_init_kernel, vgrid, dim3(256), 0, (hipStream_t)stream, label, n_vertices);
    if (n_faces > 0)
        PMN_LAUNCH(mesh_cc_hook_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, n_faces,
                   n_vertices, label, invalid);
    PMN_LAUNCH(mesh_cc_flatten_kernel, vgrid, dim3(256), 0, (hipStream_t)stream, label, n_vertices);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// ---- surface sampling ------------------------------------------------------------------------------------------------------------

#define MESH_GOLDEN 0x9E3779B97F4A7C15ULL

__host__ __device__ __forceinline__ unsigned long long mesh_mix(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ULL;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}

// key = mesh_mix(seed + MESH_GOLDEN), computed once on the host
__device__ __forceinline__ void mesh_uniforms(unsigned long long key, int face, unsigned k, float& r1, float& r2) {
    const unsigned long long h = mesh_mix(key + ((((unsigned long long)(unsigned)face << 32) | k) + 1ULL) * MESH_GOLDEN);
    r1 = (float)(unsigned)(h >> 40) * 5.9604644775390625e-8f;  // 2^-24: exact
    r2 = (float)(unsigned)((h >> 16) & 0xFFFFFFu) * 5.9604644775390625e-8f;
}

__global__ __launch_bounds__(256) void mesh_face_samples_kernel(const float* __restrict__ vertices, int nv, const int* __restrict__ faces,
                                                                int nt, double density, unsigned long long key, int* counts,
                                                                int* invalid) {
#pragma clang fp contract(off)
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nt) return;
    const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    if (!(mesh_index_ok(ia, nv) && mesh_index_ok(ib, nv) && mesh_index_ok(ic, nv))) {
        atomicAdd(invalid, 1);
        counts[f] = 0;
        return;
    }
    const float* A = vertices + 3 * (size_t)ia;
    const float* B = vertices + 3 * (size_t)ib;
    const float* C = vertices + 3 * (size_t)ic;
    const float ax = A[0], ay = A[1], az = A[2];
    const float e1x = B[0] - ax, e1y = B[1] - ay, e1z = B[2] - az;
    const float e2x = C[0] - ax, e2y = C[1] - ay, e2z = C[2] - az;
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const float area = sqrtf((cx * cx + cy * cy) + cz * cz) * 0.5f;
    int n = 0;
    if (area > 0.0f && area < __builtin_inff()) {
        float u, unused;
        mesh_uniforms(key, f, 0xFFFFFFFFu, u, unused);
        const double x = floor((double)area * density + (double)u);
        n = x >= 2147483647.0 ? 2147483647 : (int)x;
    }
    counts[f] = n;
}

struct MeshSampleArgs {
    const float* vertices;
    const int* faces;
    const unsigned char* colors;  // [nv][3] or null
    const long long* scan;        // [nt] inclusive
    int nv, nt;
    long long n;  // samples
    unsigned long long key;
    float* points;
    int* face;
    unsigned char* out_colors;
};

__global__ __launch_bounds__(256) void mesh_sample_kernel(const MeshSampleArgs a) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    int lo = 0, hi = a.nt;  // the first face with scan[f] > i
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (a.scan[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    const int f = lo;
    if (f >= a.nt) return;  // a scan that does not cover n samples: the caller's error, nothing is written
    const long long before = f ? a.scan[f - 1] : 0;
    const int ia = a.faces[3 * (size_t)f], ib = a.faces[3 * (size_t)f + 1], ic = a.faces[3 * (size_t)f + 2];
    if (!(mesh_index_ok(ia, a.nv) && mesh_index_ok(ib, a.nv) && mesh_index_ok(ic, a.nv))) return;  // (pmn_mesh_face_samples counts it 0)
    float r1, r2;
    mesh_uniforms(a.key, f, (unsigned)(i - before), r1, r2);
    const float s = sqrtf(r1);
    const float b0 = 1.0f - s, b1 = s * (1.0f - r2), b2 = s * r2;
    const float* A = a.vertices + 3 * (size_t)ia;
    const float* B = a.vertices + 3 * (size_t)ib;
    const float* C = a.vertices + 3 * (size_t)ic;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.points[3 * (size_t)i + c] = (b0 * A[c] + b1 * B[c]) + b2 * C[c];
    a.face[i] = f;
    if (a.out_colors) {
        const unsigned char* CA = a.colors + 3 * (size_t)ia;
        const unsigned char* CB = a.colors + 3 * (size_t)ib;
        const unsigned char* CC = a.colors + 3 * (size_t)ic;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float cv = floorf(((b0 * (float)CA[c] + b1 * (float)CB[c]) + b2 * (float)CC[c]) + 0.5f);
            a.out_colors[3 * (size_t)i + c] = (unsigned char)fminf(fmaxf(cv, 0.0f), 255.0f);
        }
    }
}

static int mesh_check(const float* vertices, int n_vertices, const int* faces, int n_faces) {
    if (!vertices || !faces) return PMN_ERR_ARG;
    if (n_vertices < 1 || n_faces < 1 || n_vertices > 2147483647 - 255 || n_faces > 2147483647 - 255) return PMN_ERR_SHAPE;
    return PMN_OK;
}

extern "C" int pmn_mesh_face_samples(const float* vertices, int n_vertices, const int* faces, int n_faces, double density,
                                     unsigned long long seed, int* counts, int* invalid, void* stream) {
    if (!counts || !invalid || !(density > 0.0) || !std::isfinite(density)) return PMN_ERR_ARG;
    const int rc = mesh_check(vertices, n_vertices, faces, n_faces);
    if (rc != PMN_OK) return rc;
    PMN_LAUNCH(mesh_face_samples_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, n_vertices,
               faces, n_faces, density, mesh_mix(seed + MESH_GOLDEN), counts, invalid);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_mesh_sample(const float* vertices, int n_vertices, const int* faces, int n_faces, const unsigned char* colors,
                               const long long* sample_scan, long long n_samples, unsigned long long seed, float* points, int* face,
                               unsigned char* out_colors, void* stream) {
    if (!sample_scan || !points || !face || (out_colors != nullptr && colors == nullptr)) return PMN_ERR_ARG;
    const int rc = mesh_check(vertices, n_vertices, faces, n_faces);
    if (rc != PMN_OK) return rc;
    if (n_samples < 1 || n_samples > 2147483647LL) return PMN_ERR_SHAPE;
    MeshSampleArgs a;
    a.vertices = vertices;
    a.faces = faces;
    a.colors = colors;
    a.scan = sample_scan;
    a.nv = n_vertices;
    a.nt = n_faces;
    a.n = n_samples;
    a.key = mesh_mix(seed + MESH_GOLDEN);
    a.points = points;
    a.face = face;
    a.out_colors = out_colors;
    PMN_LAUNCH(mesh_sample_kernel, dim3((unsigned)((n_samples + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// ---- distance to the surface -----------------------------------------------------------------------------------------------------

struct MeshDistArgs {
    GridArgs g;              // the reference points, grid-sorted
    const int* entry_face;   // [g.n] face of every sorted reference point
    const float* vertices;   // [nv][3]
    const int* faces;        // [nt][3]
    int nv, nt;
    double radius;           // R
    const float* query;      // [n][3]
    const int* order;        // [n] or null
    int n;
    double max_dist;
    double* dist;            // [n]
    int* face;               // [n] or null
    double* closest;         // [n][3] or null
};

// one point-segment candidate: replaces (d2, c) when strictly nearer
__device__ __forceinline__ void mesh_seg(const double px, const double py, const double pz, const double rx, const double ry,
                                         const double rz, const double qx, const double qy, const double qz, double& d2, double& cx,
                                         double& cy, double& cz) {
#pragma clang fp contract(off)
    const double ex = rx - px, ey = ry - py, ez = rz - pz;
    const double wx = qx - px, wy = qy - py, wz = qz - pz;
    const double l2 = ex * ex + ey * ey + ez * ez;
    double t = l2 > 0.0 ? (wx * ex + wy * ey + wz * ez) / l2 : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double sx = px + t * ex, sy = py + t * ey, sz = pz + t * ez;
    const double dx = qx - sx, dy = qy - sy, dz = qz - sz;
    const double s2 = dx * dx + dy * dy + dz * dz;
    if (s2 < d2) {
        d2 = s2;
        cx = sx;
        cy = sy;
        cz = sz;
    }
}

// the exact squared distance from q to the triangle (A, B, C) and the nearest point: the formulation of the header comment
__device__ __forceinline__ double mesh_point_triangle(const float* __restrict__ A, const float* __restrict__ B,
                                                      const float* __restrict__ C, const double qx, const double qy, const double qz,
                                                      double& cx, double& cy, double& cz) {
#pragma clang fp contract(off)
    const double ax = (double)A[0], ay = (double)A[1], az = (double)A[2];
    const double bx = (double)B[0], by = (double)B[1], bz = (double)B[2];
    const double gx = (double)C[0], gy = (double)C[1], gz = (double)C[2];
    double d2 = __builtin_inf();
    mesh_seg(ax, ay, az, bx, by, bz, qx, qy, qz, d2, cx, cy, cz);
    mesh_seg(bx, by, bz, gx, gy, gz, qx, qy, qz, d2, cx, cy, cz);
    mesh_seg(gx, gy, gz, ax, ay, az, qx, qy, qz, d2, cx, cy, cz);
    const double e1x = bx - ax, e1y = by - ay, e1z = bz - az;
    const double e2x = gx - ax, e2y = gy - ay, e2z = gz - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double nn = nx * nx + ny * ny + nz * nz;
    if (nn > 0.0) {
        const double wx = qx - ax, wy = qy - ay, wz = qz - az;
        const double ux = e1y * wz - e1z * wy, uy = e1z * wx - e1x * wz, uz = e1x * wy - e1y * wx;  // e1 x w
        const double vx = wy * e2z - wz * e2y, vy = wz * e2x - wx * e2z, vz = wx * e2y - wy * e2x;  // w x e2
        const double u = (ux * nx + uy * ny + uz * nz) / nn, v = (vx * nx + vy * ny + vz * nz) / nn;
        if (u >= 0.0 && v >= 0.0 && u + v <= 1.0) {
            const double dp = wx * nx + wy * ny + wz * nz;
            const double p2 = (dp * dp) / nn;
            if (p2 < d2) {
                const double s = dp / nn;
                d2 = p2;
                cx = qx - s * nx;
                cy = qy - s * ny;
                cz = qz - s * nz;
            }
        }
    }
    return d2;
}

// The walk's accumulator that turns it into a triangle search (pc_grid.hpp: "ONE rule over an accumulator").  reach2 is
// ((sqrt(d2) + R)(1 + 2^-20))^2 of the current best: a reference point, or a region, whose squared distance exceeds it belongs to no face
// that can beat or tie the best.  The slack errs towards visiting, as PMN_PC_SLACK does.
struct MeshBest {
    double d2, reach2, cx, cy, cz, qx, qy, qz, radius;
    int face;
    const int* entry_face;
    const int* faces;
    const float* vertices;
    int nv, nt;

    __device__ __forceinline__ void bound() {
#pragma clang fp contract(off)
        const double reach = (sqrt(d2) + radius) * (1.0 + PMN_PC_SLACK);
        reach2 = reach * reach;
    }
    __device__ __forceinline__ bool beyond(double g2) const { return g2 > reach2; }
    __device__ __forceinline__ void offer(double r2, int i) {
        if (r2 > reach2) return;
        const int f = entry_face[i];
        if (f == face || !mesh_index_ok(f, nt)) return;
        const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
        if (!(mesh_index_ok(ia, nv) && mesh_index_ok(ib, nv) && mesh_index_ok(ic, nv))) return;  // (mesh_dist_check_kernel counts it)
        double px, py, pz;
        const double c = mesh_point_triangle(vertices + 3 * (size_t)ia, vertices + 3 * (size_t)ib, vertices + 3 * (size_t)ic, qx, qy, qz,
                                             px, py, pz);
        if (c < d2 || (c == d2 && face >= 0 && f < face)) {
            d2 = c;
            face = f;
            cx = px;
            cy = py;
            cz = pz;
            bound();
        }
    }
};

__global__ __launch_bounds__(256) void mesh_dist_check_kernel(const int* __restrict__ faces, int nt, int nv, int* invalid) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nt) return;
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if (!(mesh_index_ok(a, nv) && mesh_index_ok(b, nv) && mesh_index_ok(c, nv))) atomicAdd(invalid, 1);
}

__global__ __launch_bounds__(64) void mesh_distance_kernel(const MeshDistArgs a) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.n) return;
    const int q = a.order ? a.order[t] : t;
    MeshBest b;
    b.qx = (double)a.query[(size_t)q * 3];
    b.qy = (double)a.query[(size_t)q * 3 + 1];
    b.qz = (double)a.query[(size_t)q * 3 + 2];
    b.d2 = a.max_dist * a.max_dist;  // a face at exactly max_dist or beyond never wins (pmn_nn_distance's convention)
    b.face = -1;
    b.cx = b.cy = b.cz = __builtin_nan("");
    b.radius = a.radius;
    b.entry_face = a.entry_face;
    b.faces = a.faces;
    b.vertices = a.vertices;
    b.nv = a.nv;
    b.nt = a.nt;
    b.bound();
    pc_walk(a.g, b.qx, b.qy, b.qz, b);
    a.dist[q] = b.face < 0 ? a.max_dist : sqrt(b.d2);
    if (a.face) a.face[q] = b.face;
    if (a.closest) {
        a.closest[(size_t)q * 3] = b.cx;
        a.closest[(size_t)q * 3 + 1] = b.cy;
        a.closest[(size_t)q * 3 + 2] = b.cz;
    }
}

extern "C" int pmn_mesh_distance(const float* ref_xyz, const long long* ref_keys, long long n_ref, const double* origin_host, double cell,
                                 const int* dims_host, const int* entry_face, double radius, const float* vertices, int n_vertices,
                                 const int* faces, int n_faces, const float* query, const int* order, long long n_query, double max_dist,
                                 double* dist, int* face, double* closest, int* invalid, void* stream) {
    MeshDistArgs a;
    int rc = grid_args(a.g, ref_xyz, ref_keys, n_ref, origin_host, cell, dims_host);
    if (rc != PMN_OK) return rc;
    rc = mesh_check(vertices, n_vertices, faces, n_faces);
    if (rc != PMN_OK) return rc;
    if (!entry_face || !query || !dist || !invalid || n_query < 1 || n_query >= (1LL << 31) - 64) return PMN_ERR_ARG;
    if (!(radius >= 0.0) || !std::isfinite(radius)) return PMN_ERR_ARG;
    if (!(max_dist > 0.0) || !std::isfinite(max_dist) || !std::isfinite(max_dist * max_dist)) return PMN_ERR_ARG;
    a.entry_face = entry_face;
    a.vertices = vertices;
    a.faces = faces;
    a.nv = n_vertices;
    a.nt = n_faces;
    a.radius = radius;
    a.query = query;
    a.order = order;
    a.n = (int)n_query;
    a.max_dist = max_dist;
    a.dist = dist;
    a.face = face;
    a.closest = closest;
    PMN_LAUNCH(mesh_dist_check_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, n_faces,
               n_vertices, invalid);
    PMN_LAUNCH(mesh_distance_kernel, dim3((unsigned)((n_query + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// ---- simplification by vertex clustering --------------------------------------------------------------------
// meshops.simplify_clustering sorts the vertices into cubic cells (a cluster per occupied cell, numbered in ascending key order), takes
// every cluster's mean from pmn_voxel_mean, and calls the two kernels below.  tests/simplify_ref.py restates both in numpy.
//
// pmn_mesh_remap_faces, a thread per face (a, b, c): corner_cluster = (cluster[a], cluster[b], cluster[c]) in the face's own order;
// flag 1 and that triple if two of the three agree; else flag 0 and the triple rotated so that its smallest entry comes first -- a
// rotation, so the orientation stays.  A face with an index outside [0, nv) is counted into *invalid, gets flag 2, the triple
// (-1, -1, -1) and corner_cluster (m, m, m), and nothing is read through it.
//
// pmn_mesh_cluster_place, a lane per cluster r.  corners holds 3 f + c for every face corner, stably sorted by corner_cluster, so the run
// [corner_starts[r], corner_starts[r + 1]) of cluster r is in ascending (face, corner) order.  Everything is float64, nothing contracted,
// IEEE division and sqrt, and RELATIVE TO THE CELL'S CENTRE ctr_k = origin_k + ((double)cell_k + 0.5) * cell (cell_k decoded from the
// cluster's key), so that a scene at coordinates of 10^4 keeps the plane offsets.  Per corner of face (A, B, C), f = entry / 3:
//   a = (double)A - ctr (likewise b, c);  e1 = b - a, e2 = c - a;
//   n = (e1.y e2.z - e1.z e2.y,  e1.z e2.x - e1.x e2.z,  e1.x e2.y - e1.y e2.x);  w = sqrt((n.x n.x + n.y n.y) + n.z n.z);
//   nothing if w is zero or not finite;  h = n / w;  q = (h.x a.x + h.y a.y) + h.z a.z  (the plane is h.p = q);  g = w * h;
//   Sxx += g.x h.x, Sxy += g.x h.y, Sxz += g.x h.z, Syy += g.y h.y, Syz += g.y h.z, Szz += g.z h.z;  t += q * g;  W += w
// in this order of accumulators, each starting from 0.0.  A face with two or three corners in the cluster is in its run once per
// corner and so contributes twice or three times: the weight of a face is its area times the number of its corners in the cluster.
// A run of at most PMN_MESH_PLACE_LONG_RUN corners is summed by its lane in run order; a longer one by the wave, lane l taking the
// entries l, l + 64, ... in run order and the 64 partial sums meeting in pmn_voxel_mean's butterfly (x_l += x_(l ^ 32), 16, 8, 4, 2, 1;
// every lane then holds the same bits).  No atomics, no LDS, no lane waits for another: the result is a function of the mesh alone.
// Then with lambda = stiffness * W and mt = (double)mean - ctr:  (S + lambda I) x = t + lambda mt  by LDL^T in the order
//   d0 = Sxx + lambda;  l10 = Sxy / d0;  l20 = Sxz / d0;  d1 = (Syy + lambda) - l10 * Sxy;  u = Syz - l10 * Sxz;  l21 = u / d1;
//   d2 = ((Szz + lambda) - l20 * Sxz) - l21 * u;  b = t + lambda * mt;  y0 = b.x;  y1 = b.y - l10 * y0;  y2 = (b.z - l20 * y0) - l21 * y1;
//   x.z = y2 / d2;  x.y = y1 / d1 - l21 * x.z;  x.x = (y0 / d0 - l10 * x.y) - l20 * x.z
// S is positive semi-definite with trace W (up to rounding), so the matrix has eigenvalues in [lambda, W + lambda]: its condition number
// is at most (1 + stiffness) / stiffness whatever the faces.  W zero or not finite gives x = mt.  x is clamped per component to
// [-cell / 2, cell / 2] (a projection onto the cell: continuous, no fallback branch) and out = (float)(ctr + x).

#define MESH_Q 10  // Sxx Sxy Sxz Syy Syz Szz tx ty tz W

struct MeshPlaceArgs {
    const float* vertices;       // [nv][3]
    const int* faces;            // [nt][3]
    const int* corners;          // [3 nt]
    const long long* starts;     // [m + 1]
    const long long* keys;       // [m]
    const float* mean;           // [m][3]
    float* out;                  // [m][3]
    int nv, nt, m;
    long long dx, dy;            // the lattice's first two dimensions
    double origin[3], cell, stiffness;
};

// adds the quadric of corner entry e, seen from (cx, cy, cz), to q[]
__device__ __forceinline__ void mesh_place_corner(const MeshPlaceArgs& a, int e, double cx, double cy, double cz, double* q) {
#pragma clang fp contract(off)
    if ((unsigned)e >= 3u * (unsigned)a.nt) return;
    const int f = e / 3;
    const int ia = a.faces[3 * (size_t)f], ib = a.faces[3 * (size_t)f + 1], ic = a.faces[3 * (size_t)f + 2];
    if (!(mesh_index_ok(ia, a.nv) && mesh_index_ok(ib, a.nv) && mesh_index_ok(ic, a.nv))) return;
    const float* A = a.vertices + 3 * (size_t)ia;
    const float* B = a.vertices + 3 * (size_t)ib;
    const float* C = a.vertices + 3 * (size_t)ic;
    const double ax = (double)A[0] - cx, ay = (double)A[1] - cy, az = (double)A[2] - cz;
    const double bx = (double)B[0] - cx, by = (double)B[1] - cy, bz = (double)B[2] - cz;
    const double gx = (double)C[0] - cx, gy = (double)C[1] - cy, gz = (double)C[2] - cz;
    const double e1x = bx - ax, e1y = by - ay, e1z = bz - az;
    const double e2x = gx - ax, e2y = gy - ay, e2z = gz - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double w = sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(w > 0.0) || !(w < __builtin_inf())) return;
    const double hx = nx / w, hy = ny / w, hz = nz / w;
    const double p = (hx * ax + hy * ay) + hz * az;
    const double wx = w * hx, wy = w * hy, wz = w * hz;
    q[0] += wx * hx;
    q[1] += wx * hy;
    q[2] += wx * hz;
    q[3] += wy * hy;
    q[4] += wy * hz;
    q[5] += wz * hz;
    q[6] += p * wx;
    q[7] += p * wy;
    q[8] += p * wz;
    q[9] += w;
}

__global__ __launch_bounds__(256) void mesh_cluster_place_kernel(const MeshPlaceArgs a) {
#pragma clang fp contract(off)
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = r < a.m;
    const long long n_corners = 3LL * a.nt;
    long long s = 0, len = 0;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (live) {
        s = a.starts[r];
        long long e = a.starts[r + 1];
        s = s < 0 ? 0 : s;
        e = e > n_corners ? n_corners : e;
        len = e > s ? e - s : 0;
        const long long key = a.keys[r];
        const long long kx = key % a.dx, ky = (key / a.dx) % a.dy, kz = key / (a.dx * a.dy);
        cx = a.origin[0] + ((double)kx + 0.5) * a.cell;
        cy = a.origin[1] + ((double)ky + 0.5) * a.cell;
        cz = a.origin[2] + ((double)kz + 0.5) * a.cell;
    }
    double q[MESH_Q];
#pragma unroll
    for (int i = 0; i < MESH_Q; ++i) q[i] = 0.0;
    const bool is_long = len > PMN_MESH_PLACE_LONG_RUN;
    if (live && !is_long)
        for (long long i = s; i < s + len; ++i) mesh_place_corner(a, a.corners[i], cx, cy, cz, q);
    // the wave's long runs, one after the other (as voxel_mean_kernel walks them)
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const long long rs = __shfl(s, owner, 64), rl = __shfl(len, owner, 64);
        const double ox = __shfl(cx, owner, 64), oy = __shfl(cy, owner, 64), oz = __shfl(cz, owner, 64);
        double part[MESH_Q];
#pragma unroll
        for (int i = 0; i < MESH_Q; ++i) part[i] = 0.0;
        for (long long i = rs + lane; i < rs + rl; i += 64) mesh_place_corner(a, a.corners[i], ox, oy, oz, part);
#pragma unroll
        for (int i = 0; i < MESH_Q; ++i) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part[i] += __shfl_xor(part[i], o, 64);
            if (lane == owner) q[i] = part[i];
        }
    }
    if (!live) return;
    const double mx = (double)a.mean[3 * (size_t)r] - cx, my = (double)a.mean[3 * (size_t)r + 1] - cy,
                 mz = (double)a.mean[3 * (size_t)r + 2] - cz;
    double x = mx, y = my, z = mz;
    const double W = q[9];
    if (W > 0.0 && W < __builtin_inf()) {
        const double lam = a.stiffness * W;
        const double d0 = q[0] + lam;
        const double l10 = q[1] / d0, l20 = q[2] / d0;
        const double d1 = (q[3] + lam) - l10 * q[1];
        const double u = q[4] - l10 * q[2];
        const double l21 = u / d1;
        const double d2 = ((q[5] + lam) - l20 * q[2]) - l21 * u;
        const double y0 = q[6] + lam * mx;
        const double y1 = (q[7] + lam * my) - l10 * y0;
        const double y2 = ((q[8] + lam * mz) - l20 * y0) - l21 * y1;
        z = y2 / d2;
        y = y1 / d1 - l21 * z;
        x = (y0 / d0 - l10 * y) - l20 * z;
    }
    const double half = a.cell * 0.5;
    x = x > half ? half : x;
    x = x < -half ? -half : x;
    y = y > half ? half : y;
    y = y < -half ? -half : y;
    z = z > half ? half : z;
    z = z < -half ? -half : z;
    a.out[3 * (size_t)r] = (float)(cx + x);
    a.out[3 * (size_t)r + 1] = (float)(cy + y);
    a.out[3 * (size_t)r + 2] = (float)(cz + z);
}

__global__ __launch_bounds__(256) void mesh_remap_faces_kernel(const int* __restrict__ faces, int nt, int nv,
                                                               const int* __restrict__ cluster, int m, int* corner_cluster,
                                                               int* out_faces, unsigned char* flag, int* invalid) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nt) return;
    const size_t o = 3 * (size_t)f;
    const int a = faces[o], b = faces[o + 1], c = faces[o + 2];
    if (!(mesh_index_ok(a, nv) && mesh_index_ok(b, nv) && mesh_index_ok(c, nv))) {
        atomicAdd(invalid, 1);
        corner_cluster[o] = corner_cluster[o + 1] = corner_cluster[o + 2] = m;
        out_faces[o] = out_faces[o + 1] = out_faces[o + 2] = -1;
        flag[f] = 2;
        return;
    }
    const int ca = cluster[a], cb = cluster[b], cc = cluster[c];
    corner_cluster[o] = ca;
    corner_cluster[o + 1] = cb;
    corner_cluster[o + 2] = cc;
    int r0 = ca, r1 = cb, r2 = cc;
    if (cb < ca && cb < cc) {
        r0 = cb;
        r1 = cc;
        r2 = ca;
    } else if (cc < ca && cc < cb) {
        r0 = cc;
        r1 = ca;
        r2 = cb;
    }
    out_faces[o] = r0;
    out_faces[o + 1] = r1;
    out_faces[o + 2] = r2;
    flag[f] = (ca == cb || cb == cc || ca == cc) ? 1 : 0;
}

extern "C" int pmn_mesh_remap_faces(const int* faces, int n_faces, int n_vertices, const int* cluster, int n_clusters,
                                    int* corner_cluster, int* out_faces, unsigned char* flag, int* invalid, void* stream) {
    if (!cluster || !corner_cluster || !out_faces || !flag || !invalid) return PMN_ERR_ARG;
    if (!faces) return PMN_ERR_ARG;
    if (n_vertices < 1 || n_faces < 1 || n_vertices > 2147483647 - 255 || n_faces > PMN_MESH_SIMPLIFY_MAX_FACES) return PMN_ERR_SHAPE;
    if (n_clusters < 1 || n_clusters > n_vertices) return PMN_ERR_ARG;
    PMN_LAUNCH(mesh_remap_faces_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, n_faces,
               n_vertices, cluster, n_clusters, corner_cluster, out_faces, flag, invalid);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_mesh_cluster_place(const float* vertices, int n_vertices, const int* faces, int n_faces, const int* corners,
                                      const long long* corner_starts, const long long* cluster_keys, int n_clusters, const float* mean,
                                      const double* origin_host, double cell, const int* dims_host, double stiffness, float* out,
                                      void* stream) {
    if (!vertices || !faces || !corners || !corner_starts || !cluster_keys || !mean || !origin_host || !dims_host || !out)
        return PMN_ERR_ARG;
    if (n_vertices < 1 || n_faces < 1 || n_vertices > 2147483647 - 255 || n_faces > PMN_MESH_SIMPLIFY_MAX_FACES) return PMN_ERR_SHAPE;
    if (n_clusters < 1 || n_clusters > n_vertices) return PMN_ERR_ARG;
    if (!(cell > 0.0) || !std::isfinite(cell) || !(stiffness > 0.0) || !std::isfinite(stiffness)) return PMN_ERR_ARG;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(origin_host[i]) || dims_host[i] < 1 || dims_host[i] > (1 << 30)) return PMN_ERR_ARG;
    MeshPlaceArgs a;
    a.vertices = vertices;
    a.faces = faces;
    a.corners = corners;
    a.starts = corner_starts;
    a.keys = cluster_keys;
    a.mean = mean;
    a.out = out;
    a.nv = n_vertices;
    a.nt = n_faces;
    a.m = n_clusters;
    a.dx = dims_host[0];
    a.dy = dims_host[1];
    for (int i = 0; i < 3; ++i) a.origin[i] = origin_host[i];
    a.cell = cell;
    a.stiffness = stiffness;
    PMN_LAUNCH(mesh_cluster_place_kernel, dim3((unsigned)((n_clusters + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// ---- smoothing and vertex normals ---------------------------------------------------------------------------
// meshops.vertex_adjacency builds the CSR of the vertices' neighbours (integer torch); pmn_mesh_smooth applies umbrella steps over it and
// pmn_mesh_vertex_normals sums the faces' cross products per vertex.  tests/smooth_ref.py restates both in numpy; the arithmetic is
// spelled out in include/pmn_hip.h.  Both kernels are a lane per vertex and follow ONE rule for a row: at most PMN_MESH_SMOOTH_LONG_ROW
// entries are summed by the row's lane in row order; a longer row by the wave, lane l taking the entries l, l + 64, ... in row order and
// the 64 partial sums meeting in pmn_voxel_mean's butterfly, exactly as mesh_cluster_place_kernel does.  No atomics on floats, no LDS.

struct MeshRowSum {
    double x, y, z;
};

// the wave's long rows, one after the other (as voxel_mean_kernel walks them): `add(entry index, the owner's own value, sums)` adds one
// entry; the owner's lane ends with the butterfly's result.  Every shuffle stands where the whole wave is active.
template <typename Add>
__device__ __forceinline__ void mesh_long_rows(bool is_long, long long s, long long len, const MeshRowSum& own, int lane, MeshRowSum& q,
                                               Add add) {
#pragma clang fp contract(off)
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const long long rs = __shfl(s, owner, 64), rl = __shfl(len, owner, 64);
        const MeshRowSum o = {__shfl(own.x, owner, 64), __shfl(own.y, owner, 64), __shfl(own.z, owner, 64)};
        MeshRowSum part = {0.0, 0.0, 0.0};
        for (long long i = rs + lane; i < rs + rl; i += 64) add(i, o, part);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            part.x += __shfl_xor(part.x, o, 64);
            part.y += __shfl_xor(part.y, o, 64);
            part.z += __shfl_xor(part.z, o, 64);
        }
        if (lane == owner) q = part;
    }
}

struct MeshSmoothArgs {
    const float* src;            // [nv][3]
    float* dst;                  // [nv][3]
    const long long* starts;     // [nv + 1]
    const int* neighbours;       // [n_entries]
    const unsigned char* pinned; // [nv] or null
    int* invalid;                // counted in the first step only, else null
    long long n_entries;
    int nv;
    double factor;
};

__global__ __launch_bounds__(256) void mesh_smooth_kernel(const MeshSmoothArgs a) {
#pragma clang fp contract(off)
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = v < a.nv;
    long long s = 0, len = 0;
    float fx = 0.0f, fy = 0.0f, fz = 0.0f;
    bool moves = false;
    if (live) {
        s = a.starts[v];
        long long e = a.starts[v + 1];
        s = s < 0 ? 0 : s;
        e = e > a.n_entries ? a.n_entries : e;
        len = e > s ? e - s : 0;
        fx = a.src[3 * (size_t)v];
        fy = a.src[3 * (size_t)v + 1];
        fz = a.src[3 * (size_t)v + 2];
        moves = len > 0 && !(a.pinned && a.pinned[v]);
    }
    // (a pinned or empty row still counts its bad entries: *invalid is a property of the CSR, not of the mask)
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    MeshRowSum q = {0.0, 0.0, 0.0};
    int bad = 0;
    const bool is_long = len > PMN_MESH_SMOOTH_LONG_ROW;
    if (live && !is_long)
        for (long long i = s; i < s + len; ++i) {
            const int j = a.neighbours[i];
            if (!mesh_index_ok(j, a.nv)) {
                ++bad;
                continue;
            }
            const float* P = a.src + 3 * (size_t)j;
            q.x += (double)P[0] - px;
            q.y += (double)P[1] - py;
            q.z += (double)P[2] - pz;
        }
    const MeshRowSum own = {px, py, pz};
    mesh_long_rows(is_long, s, len, own, lane, q, [&](long long i, const MeshRowSum& o, MeshRowSum& part) {
        const int j = a.neighbours[i];
        if (!mesh_index_ok(j, a.nv)) {
            ++bad;
            return;
        }
        const float* P = a.src + 3 * (size_t)j;
        part.x += (double)P[0] - o.x;
        part.y += (double)P[1] - o.y;
        part.z += (double)P[2] - o.z;
    });
    if (bad && a.invalid) atomicAdd(a.invalid, bad);
    if (!live) return;
    if (moves) {
        const double d = (double)len;
        fx = (float)(px + a.factor * (q.x / d));
        fy = (float)(py + a.factor * (q.y / d));
        fz = (float)(pz + a.factor * (q.z / d));
    }
    a.dst[3 * (size_t)v] = fx;
    a.dst[3 * (size_t)v + 1] = fy;
    a.dst[3 * (size_t)v + 2] = fz;
}

__global__ __launch_bounds__(256) void mesh_copy_xyz_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

static bool mesh_overlap(const void* p, const void* q, size_t bytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + bytes && b < a + bytes;
}

extern "C" int pmn_mesh_smooth(const float* xyz, int n_vertices, const long long* starts, const int* neighbours, long long n_entries,
                               const unsigned char* pinned, const double* factors_host, int n_steps, float* out, float* scratch,
                               int* invalid, void* stream) {
    if (!xyz || !starts || !out || !invalid || n_entries < 0 || (n_entries > 0 && !neighbours)) return PMN_ERR_ARG;
    if (n_steps < 0 || n_steps > PMN_MESH_SMOOTH_MAX_STEPS || (n_steps > 0 && !factors_host) || (n_steps > 1 && !scratch))
        return PMN_ERR_ARG;
    if (n_vertices < 1 || n_vertices > 2147483647 - 255) return PMN_ERR_SHAPE;
    for (int k = 0; k < n_steps; ++k)
        if (!std::isfinite(factors_host[k])) return PMN_ERR_ARG;
    const size_t bytes = 3 * sizeof(float) * (size_t)n_vertices;
    if (mesh_overlap(out, xyz, bytes)) return PMN_ERR_ARG;
    if (scratch && (mesh_overlap(scratch, xyz, bytes) || mesh_overlap(scratch, out, bytes))) return PMN_ERR_ARG;
    const dim3 grid((unsigned)((n_vertices + 255) / 256));
    if (n_steps == 0) {
        const long long n = 3LL * n_vertices;
        PMN_LAUNCH(mesh_copy_xyz_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, xyz, out, n);
        PMN_CHECK_LAUNCH();
        return PMN_OK;
    }
    MeshSmoothArgs a;
    a.starts = starts;
    a.neighbours = neighbours;
    a.pinned = pinned;
    a.n_entries = n_entries;
    a.nv = n_vertices;
    const float* src = xyz;
    for (int k = 0; k < n_steps; ++k) {
        a.src = src;
        a.dst = ((n_steps - 1 - k) & 1) ? scratch : out;
        a.invalid = k == 0 ? invalid : nullptr;
        a.factor = factors_host[k];
        PMN_LAUNCH(mesh_smooth_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
        src = a.dst;
    }
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

struct MeshNormalArgs {
    const float* vertices;       // [nv][3]
    const int* faces;            // [nt][3]
    const int* corners;          // [3 nt]
    const long long* starts;     // [nv + 1]
    float* out;                  // [nv][3]
    int nv, nt, flip;
};

// adds (B - A) x (C - A) of corner entry e's face to q
__device__ __forceinline__ void mesh_normal_corner(const MeshNormalArgs& a, int e, MeshRowSum& q) {
#pragma clang fp contract(off)
    if ((unsigned)e >= 3u * (unsigned)a.nt) return;
    const int f = e / 3;
    const int ia = a.faces[3 * (size_t)f], ib = a.faces[3 * (size_t)f + 1], ic = a.faces[3 * (size_t)f + 2];
    if (!(mesh_index_ok(ia, a.nv) && mesh_index_ok(ib, a.nv) && mesh_index_ok(ic, a.nv))) return;
    const float* A = a.vertices + 3 * (size_t)ia;
    const float* B = a.vertices + 3 * (size_t)ib;
    const float* C = a.vertices + 3 * (size_t)ic;
    const double ax = (double)A[0], ay = (double)A[1], az = (double)A[2];
    const double e1x = (double)B[0] - ax, e1y = (double)B[1] - ay, e1z = (double)B[2] - az;
    const double e2x = (double)C[0] - ax, e2y = (double)C[1] - ay, e2z = (double)C[2] - az;
    q.x += e1y * e2z - e1z * e2y;
    q.y += e1z * e2x - e1x * e2z;
    q.z += e1x * e2y - e1y * e2x;
}

__global__ __launch_bounds__(256) void mesh_vertex_normals_kernel(const MeshNormalArgs a) {
#pragma clang fp contract(off)
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = v < a.nv;
    const long long n_corners = 3LL * a.nt;
    long long s = 0, len = 0;
    if (live) {
        s = a.starts[v];
        long long e = a.starts[v + 1];
        s = s < 0 ? 0 : s;
        e = e > n_corners ? n_corners : e;
        len = e > s ? e - s : 0;
    }
    MeshRowSum q = {0.0, 0.0, 0.0};
    const bool is_long = len > PMN_MESH_SMOOTH_LONG_ROW;
    if (live && !is_long)
        for (long long i = s; i < s + len; ++i) mesh_normal_corner(a, a.corners[i], q);
    const MeshRowSum none = {0.0, 0.0, 0.0};
    mesh_long_rows(is_long, s, len, none, lane, q,
                   [&](long long i, const MeshRowSum&, MeshRowSum& part) { mesh_normal_corner(a, a.corners[i], part); });
    if (!live) return;
    const double length = sqrt((q.x * q.x + q.y * q.y) + q.z * q.z);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (length > 0.0 && length < __builtin_inf()) {
        nx = (float)(q.x / length);
        ny = (float)(q.y / length);
        nz = (float)(q.z / length);
        if (a.flip) {
            nx = -nx;
            ny = -ny;
            nz = -nz;
        }
    }
    a.out[3 * (size_t)v] = nx;
    a.out[3 * (size_t)v + 1] = ny;
    a.out[3 * (size_t)v + 2] = nz;
}

extern "C" int pmn_mesh_vertex_normals(const float* vertices, int n_vertices, const int* faces, int n_faces, const int* corners,
                                       const long long* corner_starts, int flip, float* out, int* invalid, void* stream) {
    if (!vertices || !faces || !corners || !corner_starts || !out || !invalid) return PMN_ERR_ARG;
    if (n_vertices < 1 || n_faces < 1 || n_vertices > 2147483647 - 255 || n_faces > PMN_MESH_SIMPLIFY_MAX_FACES) return PMN_ERR_SHAPE;
    MeshNormalArgs a;
    a.vertices = vertices;
    a.faces = faces;
    a.corners = corners;
    a.starts = corner_starts;
    a.out = out;
    a.nv = n_vertices;
    a.nt = n_faces;
    a.flip = flip;
    PMN_LAUNCH(mesh_dist_check_kernel, dim3((unsigned)((n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, n_faces,
               n_vertices, invalid);
    PMN_LAUNCH(mesh_vertex_normals_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
