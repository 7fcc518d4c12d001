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
#include <cmath>

#include "pmn_common.hpp"

#define MESH_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ bool mesh_index_ok(int v, int nv) { return (unsigned)v < (unsigned)nv; }

// ---- components ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void mesh_cc_init_kernel(int* parent, int nv) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < nv) parent[v] = v;
}

// the root of v as far as this lane can see; halves the path on the way (a best-effort store of a smaller ancestor)
__device__ __forceinline__ int mesh_cc_find(int* parent, int v) {
    int p = __hip_atomic_load(parent + v, MESH_RLX_AGENT);
    while (p < v) {  // (p > v cannot be stored; read as a root, it would fail the swap below, never loop here)
        const int g = __hip_atomic_load(parent + p, MESH_RLX_AGENT);
        if (g < p) __hip_atomic_store(parent + v, g, MESH_RLX_AGENT);
        v = p;
        p = g;
    }
    return v;
}

__device__ __forceinline__ void mesh_cc_unite(int* parent, int a, int b) {
    while (true) {
        a = mesh_cc_find(parent, a);
        b = mesh_cc_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, MESH_RLX_AGENT)) return;
        if (!(seen < hi)) return;  // cannot happen (a slot only ever falls); a lane never retries without having descended
        a = seen;
        b = lo;
    }
}

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

__global__ __launch_bounds__(256) void mesh_cc_flatten_kernel(int* parent, int nv) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    int r = v, p = __hip_atomic_load(parent + v, MESH_RLX_AGENT);
    while (p < r) {  // another lane may already have flattened a slot on the way: its value is the same root
        r = p;
        p = __hip_atomic_load(parent + r, MESH_RLX_AGENT);
    }
    __hip_atomic_store(parent + v, r, MESH_RLX_AGENT);
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
