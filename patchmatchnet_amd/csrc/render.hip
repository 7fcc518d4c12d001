// render.hip -- a triangle mesh or a point cloud drawn into one of a scan's cameras: the direction the rest of the
// pipeline lacks, 3-D back to the image.  The reference has no renderer; tests/render_ref.py restates everything below in numpy and is
// the yardstick.
//
// Z-buffer.  One uint64 key per pixel, all ones where nothing was drawn: key = (uint64)float_bits(depth) << 32 | primitive index, updated
// with a 64-bit global atomic MIN (positive floats order like their bits).  The smallest key wins: the nearest depth and, among equal
// depths, the lowest index, whatever the order in which primitives arrive, the launch shape or the run.  The compiled code object holds
// ONE global_atomic_umin_x2 per update and no compare-and-swap loop (checked in the disassembly: DESIGN.md section 16).  A plain load of
// the key precedes it and skips the atomic when the pixel already holds a smaller key: keys only ever decrease, so a stale value can
// only make the atomic happen needlessly, never suppress one that would win.
//
// Projection of a world point p (r_project), float32, nothing contracted, IEEE division, the operand order of pmn_tsdf_integrate:
//     pc_r = ((R_r0 p.x + R_r1 p.y) + R_r2 p.z) + t_r          NOT DRAWN (counter 0) unless pc is finite and pc.z > 0
//     q_r  = (K_r0 pc.x + K_r1 pc.y) + K_r2 pc.z;  u = q.x / q.z, v = q.y / q.z         (pixel centres at integer coordinates)
//     X = rintf(u * 256.0f), Y = rintf(v * 256.0f)              (round half to even; units of 1/256 px)
//                                                               NOT DRAWN (counter 1) unless |X| <= 2^22 and |Y| <= 2^22 (NaN fails)
// Guard band 2^22 units = 16384 px.  Every coordinate difference then lies within 2^23, every product within 2^46 and an edge function
// (a difference of two products) within 2^47: the 64-bit edge functions cannot overflow (they could not below 2^30 either; 2^22 is
// chosen so that u * 256 is still an exactly representable float32 integer after rintf and differences fit int32, which makes every
// product one v_mad_i64_i32).  h, w <= 16384 keeps every pixel centre inside the band.  There is NO near-plane clipping: a triangle
// with one vertex behind the camera is not drawn at all.
//
// Coverage of pixel centre P = (256 px, 256 py), all in integers:
//     orient(a, b, c) = (b.X - a.X) (c.Y - a.Y) - (b.Y - a.Y) (c.X - a.X)
//     w0 = orient(v1, v2, P), w1 = orient(v2, v0, P), w2 = orient(v0, v1, P), area = orient(v0, v1, v2) = w0 + w1 + w2
//     area == 0: dropped (counter 2).  s = sign(area); both windings are drawn.
//     edge i runs v1->v2, v2->v0, v0->v1 with (dx, dy) = s * (end - start); it is TOP-LEFT iff dy < 0 or (dy == 0 and dx > 0)
//     covered iff for all i: s w_i > 0, or s w_i == 0 and edge i is top-left
// so two triangles that share an edge cover every pixel centre on it exactly once.
// Depth (float32): b_i = (float)(s w_i) / (float)(s area) (int64 -> float32 round to nearest), c_i = b_i / z_i with z_i = pc.z of
// vertex i, depth = 1.0f / ((c0 + c1) + c2); a pixel is written only if 0 < depth < inf.
//
// Work distribution.  raster_small_kernel: a thread per triangle; it walks the triangle's bounding box (clipped to the image) if that
// holds at most `max_box` pixels and otherwise appends the triangle to a worklist (one atomic per wave).  raster_large_kernel: a fixed
// grid whose waves take items wave, wave + nwaves, ... where an item is (worklist entry, one of 8 slices = every 8th row of 8 x 8 tiles
// of the box); a wave walks its rows tile by tile, a lane per pixel (one evaluation of the three edge
// functions per lane and tile: a test of the tile's corners first cost more than it saved).  The key is order-independent, so the worklist's order does not matter.
//
// Points (splat_kernel): a thread per point, the same projection and key (index = the point's).  Footprint: the nearest pixel
// ((X + 128) >> 8, i.e. floorf(u + 0.5f) on the snapped coordinate) always, and with a radius r > 0 every pixel whose centre satisfies
// (256 px - X)^2 + (256 py - Y)^2 <= Rq^2, Rq = (int)rintf(r * 256.0f), r = radius_px or fminf((radius_world * K_00) / pc.z,
// PMN_SPLAT_MAX_RADIUS).
//
// Resolve (resolve_kernel): a thread per pixel; see pmn_raster_resolve in include/pmn_hip.h for the arithmetic.
#include "pmn_common.hpp"

#pragma clang fp contract(off)

#define R_GUARD 4194304.0f  // 2^22 units of 1/256 px
#define R_LARGE_BLOCKS 2048  // 8192 waves = 8 per SIMD of the 256 CUs: every wave slot the kernel's 110 VGPRs allow (occupancy 4) twice over
#define R_SLICES 8           // a large triangle is shared by 8 waves, so even one frame-filling triangle is not one wave's work

struct RCam {
    float c[21];  // K row-major, then the upper 3 x 4 of the world-to-camera extrinsic row-major
};

struct RVert {
    float px, py, pz;  // camera frame
    int X, Y;          // snapped image position, 1/256 px
    int state;         // 0 drawable, 1 behind / non-finite, 2 outside the guard band
};

__device__ __forceinline__ RVert r_project(const RCam& cam, const float* __restrict__ p) {
    const float* K = cam.c;
    const float* E = cam.c + 9;
    // (pmn_settle: lesson 46 -- no packed-fp32 op_sel form may come out of these broadcasts; it changes no value)
    const float x = pmn_settle(p[0]), y = pmn_settle(p[1]), z = pmn_settle(p[2]);
    RVert v;
    v.px = ((E[0] * x + E[1] * y) + E[2] * z) + E[3];
    v.py = ((E[4] * x + E[5] * y) + E[6] * z) + E[7];
    v.pz = ((E[8] * x + E[9] * y) + E[10] * z) + E[11];
    v.px = pmn_settle(v.px), v.py = pmn_settle(v.py), v.pz = pmn_settle(v.pz);
    v.X = 0;
    v.Y = 0;
    const float inf = __builtin_inff();
    if (!(fabsf(v.px) < inf && fabsf(v.py) < inf && v.pz > 0.0f && v.pz < inf)) {
        v.state = 1;
        return v;
    }
    const float qx = (K[0] * v.px + K[1] * v.py) + K[2] * v.pz;
    const float qy = (K[3] * v.px + K[4] * v.py) + K[5] * v.pz;
    const float qz = (K[6] * v.px + K[7] * v.py) + K[8] * v.pz;
    const float su = rintf((qx / qz) * 256.0f), sv = rintf((qy / qz) * 256.0f);
    if (!(fabsf(su) <= R_GUARD && fabsf(sv) <= R_GUARD)) {
        v.state = 2;
        return v;
    }
    v.X = (int)su;
    v.Y = (int)sv;
    v.state = 0;
    return v;
}

struct RTri {
    int X0, Y0, X1, Y1, X2, Y2;
    float z0, z1, z2;
    long long area;  // s * orient(v0, v1, v2) > 0
    int s;
    int tl0, tl1, tl2;  // 0 if edge i is top-left, else 1 (subtracted from s * w_i before the >= 0 test)
    int px0, px1, py0, py1;
};

__device__ __forceinline__ long long r_orient(int ax, int ay, int bx, int by, int cx, int cy) {
    return (long long)(bx - ax) * (long long)(cy - ay) - (long long)(by - ay) * (long long)(cx - ax);
}

__device__ __forceinline__ int r_not_top_left(int dx, int dy) { return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1; }

// state: 0 drawable, 1 behind / non-finite / a vertex index out of range, 2 outside the guard band, 3 zero area
__device__ __forceinline__ int r_setup(const RCam& cam, const float* __restrict__ vertices, int nv, const int* __restrict__ faces, int t,
                                       int h, int w, RTri& tri, RVert* verts) {
    const unsigned i0 = (unsigned)faces[3 * (size_t)t], i1 = (unsigned)faces[3 * (size_t)t + 1], i2 = (unsigned)faces[3 * (size_t)t + 2];
    if (i0 >= (unsigned)nv || i1 >= (unsigned)nv || i2 >= (unsigned)nv) return 1;
    const RVert a = r_project(cam, vertices + 3 * (size_t)i0), b = r_project(cam, vertices + 3 * (size_t)i1),
                c = r_project(cam, vertices + 3 * (size_t)i2);
    if (verts) {
        verts[0] = a;
        verts[1] = b;
        verts[2] = c;
    }
    if (a.state == 1 || b.state == 1 || c.state == 1) return 1;
    if (a.state == 2 || b.state == 2 || c.state == 2) return 2;
    const long long area = r_orient(a.X, a.Y, b.X, b.Y, c.X, c.Y);
    if (area == 0) return 3;
    const int s = area > 0 ? 1 : -1;
    tri.X0 = a.X, tri.Y0 = a.Y, tri.X1 = b.X, tri.Y1 = b.Y, tri.X2 = c.X, tri.Y2 = c.Y;
    tri.z0 = a.pz, tri.z1 = b.pz, tri.z2 = c.pz;
    tri.area = s * area;
    tri.s = s;
    tri.tl0 = r_not_top_left(s * (c.X - b.X), s * (c.Y - b.Y));
    tri.tl1 = r_not_top_left(s * (a.X - c.X), s * (a.Y - c.Y));
    tri.tl2 = r_not_top_left(s * (b.X - a.X), s * (b.Y - a.Y));
    const int minX = min(a.X, min(b.X, c.X)), maxX = max(a.X, max(b.X, c.X));
    const int minY = min(a.Y, min(b.Y, c.Y)), maxY = max(a.Y, max(b.Y, c.Y));
    tri.px0 = max((minX + 255) >> 8, 0);  // ceil(minX / 256): >> is the floor division
    tri.px1 = min(maxX >> 8, w - 1);
    tri.py0 = max((minY + 255) >> 8, 0);
    tri.py1 = min(maxY >> 8, h - 1);
    return 0;
}

// s * w_i at pixel (px, py); true if the centre is covered
__device__ __forceinline__ bool r_cover(const RTri& t, int px, int py, long long& w0, long long& w1, long long& w2) {
    const int Px = px << 8, Py = py << 8;
    w0 = t.s * r_orient(t.X1, t.Y1, t.X2, t.Y2, Px, Py);
    w1 = t.s * r_orient(t.X2, t.Y2, t.X0, t.Y0, Px, Py);
    w2 = t.s * r_orient(t.X0, t.Y0, t.X1, t.Y1, Px, Py);
    return ((w0 - t.tl0) | (w1 - t.tl1) | (w2 - t.tl2)) >= 0;
}

__device__ __forceinline__ void r_bary(const RTri& t, long long w0, long long w1, long long w2, float& c0, float& c1, float& c2) {
    const float fa = (float)t.area;
    c0 = ((float)w0 / fa) / t.z0;
    c1 = ((float)w1 / fa) / t.z1;
    c2 = ((float)w2 / fa) / t.z2;
}

__device__ __forceinline__ void r_put(unsigned long long* __restrict__ keys, size_t pix, float depth, unsigned index) {
    if (!(depth > 0.0f && depth < __builtin_inff())) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | index;
    if (key < keys[pix]) atomicMin(keys + pix, key);
}

__device__ __forceinline__ void r_pixel(const RTri& t, int px, int py, int w, unsigned index, unsigned long long* __restrict__ keys) {
    long long w0, w1, w2;
    if (!r_cover(t, px, py, w0, w1, w2)) return;
    float c0, c1, c2;
    r_bary(t, w0, w1, w2, c0, c1, c2);
    r_put(keys, (size_t)py * w + px, 1.0f / ((c0 + c1) + c2), index);
}

// one add per wave of the number of lanes with `flag`
__device__ __forceinline__ void r_count(int* counter, bool flag) {
    const unsigned long long m = __ballot(flag);
    if (m != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)__ballot(true)) - 1)) atomicAdd(counter, __popcll(m));
}

struct RasterArgs {
    const float* vertices;
    const int* faces;
    int nv, nt, h, w;
    long long max_box;
    unsigned long long* keys;
    int* counters;  // [0] behind / non-finite / bad index, [1] outside the guard band, [2] zero area, [3] worklist length
    int* worklist;  // [nt]
    RCam cam;
};

__global__ __launch_bounds__(256) void raster_small_kernel(const RasterArgs a) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int t = (int)gid;
    RTri tri;
    int state = 4;
    if (gid < a.nt) state = r_setup(a.cam, a.vertices, a.nv, a.faces, t, a.h, a.w, tri, nullptr);
    r_count(a.counters + 0, state == 1);
    r_count(a.counters + 1, state == 2);
    r_count(a.counters + 2, state == 3);
    bool draw = state == 0 && tri.px0 <= tri.px1 && tri.py0 <= tri.py1;
    const bool large = draw && (long long)(tri.px1 - tri.px0 + 1) * (long long)(tri.py1 - tri.py0 + 1) > a.max_box;
    const unsigned long long m = __ballot(large);
    if (m != 0ull) {  // wave-uniform
        const int lane = threadIdx.x & 63;
        const int leader = __ffsll((long long)m) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(a.counters + 3, __popcll(m));
        base = __shfl(base, leader, 64);
        if (large) {
            const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
            if (slot >= 0 && slot < a.nt) a.worklist[slot] = t;
        }
    }
    if (!draw || large) return;
    for (int py = tri.py0; py <= tri.py1; ++py)
        for (int px = tri.px0; px <= tri.px1; ++px) r_pixel(tri, px, py, a.w, (unsigned)t, a.keys);
}

__global__ __launch_bounds__(256) void raster_large_kernel(const RasterArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * 256 + threadIdx.x) >> 6), nwaves = (int)(gridDim.x * 4);
    const long long n = (long long)min(max(a.counters[3], 0), a.nt) * R_SLICES;
    for (long long i = wave; i < n; i += nwaves) {  // item = (worklist entry, slice): a slice is every R_SLICES-th row of tiles
        const int t = a.worklist[i / R_SLICES];
        const int slice = (int)(i % R_SLICES);
        if (t < 0 || t >= a.nt) continue;
        RTri tri;
        if (r_setup(a.cam, a.vertices, a.nv, a.faces, t, a.h, a.w, tri, nullptr) != 0) continue;
        for (int ty = tri.py0 + 8 * slice; ty <= tri.py1; ty += 8 * R_SLICES)
            for (int tx = tri.px0; tx <= tri.px1; tx += 8) {
                const int px = tx + (lane & 7), py = ty + (lane >> 3);
                if (px <= tri.px1 && py <= tri.py1) r_pixel(tri, px, py, a.w, (unsigned)t, a.keys);
            }
    }
}

static int r_camera(RCam& cam, const float* cam_host, int h, int w) {
    if (!cam_host) return PMN_ERR_ARG;
    if (h < 1 || w < 1 || h > PMN_RASTER_MAX_DIM || w > PMN_RASTER_MAX_DIM) return PMN_ERR_SHAPE;
    for (int c = 0; c < 21; ++c) {
        if (!std::isfinite(cam_host[c])) return PMN_ERR_ARG;
        cam.c[c] = cam_host[c];
    }
    return PMN_OK;
}

extern "C" int pmn_raster_triangles(const float* vertices, int n_vertices, const int* faces, int n_faces, const float* cam_host, int h,
                                    int w, long long max_box, unsigned long long* keys, int* counters, int* worklist, void* stream) {
    if (!vertices || !faces || !keys || !counters || !worklist) return PMN_ERR_ARG;
    if (n_vertices < 1 || n_faces < 1 || max_box < 0) return PMN_ERR_ARG;
    RasterArgs a;
    const int rc = r_camera(a.cam, cam_host, h, w);
    if (rc != PMN_OK) return rc;
    a.vertices = vertices;
    a.faces = faces;
    a.nv = n_vertices;
    a.nt = n_faces;
    a.h = h;
    a.w = w;
    a.max_box = max_box == 0 ? PMN_RASTER_MAX_BOX : max_box;
    a.keys = keys;
    a.counters = counters;
    a.worklist = worklist;
    PMN_LAUNCH(raster_small_kernel, dim3((unsigned)(((long long)n_faces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    PMN_LAUNCH(raster_large_kernel, dim3(R_LARGE_BLOCKS), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// ---- points ---------------------------------------------------------------------------------------------------------------------

struct SplatArgs {
    const float* points;
    long long n;
    int h, w;
    float radius_px, radius_world;
    unsigned long long* keys;
    int* counters;
    RCam cam;
};

__global__ __launch_bounds__(256) void splat_kernel(const SplatArgs a) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    RVert v;
    v.state = 4;
    if (gid < a.n) v = r_project(a.cam, a.points + 3 * (size_t)gid);
    r_count(a.counters + 0, v.state == 1);
    r_count(a.counters + 1, v.state == 2);
    if (v.state != 0) return;
    const unsigned index = (unsigned)gid;
    const int nx = (v.X + 128) >> 8, ny = (v.Y + 128) >> 8;
    float r = a.radius_px;
    if (a.radius_world > 0.0f) r = fminf((a.radius_world * a.cam.c[0]) / v.pz, (float)PMN_SPLAT_MAX_RADIUS);
    const int Rq = (int)rintf(r * 256.0f);
    if (Rq < 128) {  // no centre other than the nearest can lie within less than half a pixel
        if (nx >= 0 && nx < a.w && ny >= 0 && ny < a.h) r_put(a.keys, (size_t)ny * a.w + nx, v.pz, index);
        return;
    }
    const long long R2 = (long long)Rq * Rq;
    const int px0 = max((v.X - Rq + 255) >> 8, 0), px1 = min((v.X + Rq) >> 8, a.w - 1);
    const int py0 = max((v.Y - Rq + 255) >> 8, 0), py1 = min((v.Y + Rq) >> 8, a.h - 1);
    for (int py = py0; py <= py1; ++py)
        for (int px = px0; px <= px1; ++px) {
            const long long dx = (px << 8) - v.X, dy = (py << 8) - v.Y;
            if (dx * dx + dy * dy <= R2 || (px == nx && py == ny)) r_put(a.keys, (size_t)py * a.w + px, v.pz, index);
        }
    // (with Rq >= 128 the nearest pixel's centre is within the disc's box, so the loop has visited it)
}

extern "C" int pmn_splat_points(const float* points, long long n_points, const float* cam_host, int h, int w, float radius_px,
                                float radius_world, unsigned long long* keys, int* counters, void* stream) {
    if (!points || !keys || !counters) return PMN_ERR_ARG;
    if (n_points < 1 || n_points > 2147483647LL) return PMN_ERR_ARG;  // the index plane is int32
    if (!(radius_px >= 0.0f && radius_px <= (float)PMN_SPLAT_MAX_RADIUS) || !(radius_world >= 0.0f) || !std::isfinite(radius_world))
        return PMN_ERR_ARG;
    if (radius_px > 0.0f && radius_world > 0.0f) return PMN_ERR_ARG;
    SplatArgs a;
    const int rc = r_camera(a.cam, cam_host, h, w);
    if (rc != PMN_OK) return rc;
    a.points = points;
    a.n = n_points;
    a.h = h;
    a.w = w;
    a.radius_px = radius_px;
    a.radius_world = radius_world;
    a.keys = keys;
    a.counters = counters;
    PMN_LAUNCH(splat_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

// ---- resolve --------------------------------------------------------------------------------------------------------------------

struct ResolveArgs {
    const unsigned long long* keys;
    const float* vertices;
    const int* faces;  // null: the primitives are points
    const unsigned char* colors;
    const float* normals;
    long long nv, nt;
    int h, w, shade;
    float* depth;
    int* index;
    unsigned char* rgb;
    float* normal;
    RCam cam;
};

__device__ __forceinline__ unsigned char r_byte(float c) { return (unsigned char)fminf(fmaxf(floorf(c + 0.5f), 0.0f), 255.0f); }

__global__ __launch_bounds__(256) void resolve_kernel(const ResolveArgs a) {
    const int px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= a.w || py >= a.h) return;
    const size_t pix = (size_t)py * a.w + px;
    const unsigned long long key = a.keys[pix];
    const unsigned idx = (unsigned)(key & 0xffffffffull);
    float depth = pmn_settle(__uint_as_float((unsigned)(key >> 32)));
    bool hit = key != ~0ull && (long long)idx < (a.faces ? a.nt : a.nv);
    float col[3] = {128.0f, 128.0f, 128.0f}, n[3] = {0.0f, 0.0f, 0.0f}, p[3] = {0.0f, 0.0f, 0.0f};
    const bool want_n = a.normal != nullptr || (a.rgb != nullptr && a.shade != 0);
    if (hit && (a.rgb || want_n)) {
        const float* E = a.cam.c + 9;
        if (a.faces) {
            RTri tri;
            RVert v[3];
            hit = r_setup(a.cam, a.vertices, (int)a.nv, a.faces, (int)idx, a.h, a.w, tri, v) == 0;
            if (hit) {
                long long w0, w1, w2;
                r_cover(tri, px, py, w0, w1, w2);
                float c[3];
                r_bary(tri, w0, w1, w2, c[0], c[1], c[2]);
                c[0] = pmn_settle(c[0]), c[1] = pmn_settle(c[1]), c[2] = pmn_settle(c[2]);
                const int* f = a.faces + 3 * (size_t)idx;
                if (a.colors)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch)
                        col[ch] = ((c[0] * (float)a.colors[3 * (size_t)f[0] + ch] + c[1] * (float)a.colors[3 * (size_t)f[1] + ch]) +
                                   c[2] * (float)a.colors[3 * (size_t)f[2] + ch]) * depth;
                if (want_n) {
                    p[0] = ((c[0] * v[0].px + c[1] * v[1].px) + c[2] * v[2].px) * depth;
                    p[1] = ((c[0] * v[0].py + c[1] * v[1].py) + c[2] * v[2].py) * depth;
                    p[2] = ((c[0] * v[0].pz + c[1] * v[1].pz) + c[2] * v[2].pz) * depth;
                    if (a.normals) {
                        float nw[3];
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch)
                            nw[ch] = ((c[0] * a.normals[3 * (size_t)f[0] + ch] + c[1] * a.normals[3 * (size_t)f[1] + ch]) +
                                      c[2] * a.normals[3 * (size_t)f[2] + ch]) * depth;
                        nw[0] = pmn_settle(nw[0]), nw[1] = pmn_settle(nw[1]), nw[2] = pmn_settle(nw[2]);
#pragma unroll
                        for (int r = 0; r < 3; ++r) n[r] = (E[4 * r] * nw[0] + E[4 * r + 1] * nw[1]) + E[4 * r + 2] * nw[2];
                    } else {  // the face's own normal in the camera frame
                        const float ax = pmn_settle(v[1].px - v[0].px), ay = pmn_settle(v[1].py - v[0].py), az = pmn_settle(v[1].pz - v[0].pz);
                        const float bx = pmn_settle(v[2].px - v[0].px), by = pmn_settle(v[2].py - v[0].py), bz = pmn_settle(v[2].pz - v[0].pz);
                        n[0] = ay * bz - az * by;
                        n[1] = az * bx - ax * bz;
                        n[2] = ax * by - ay * bx;
                    }
                }
            }
        } else {
            const RVert v = r_project(a.cam, a.vertices + 3 * (size_t)idx);
            p[0] = v.px, p[1] = v.py, p[2] = v.pz;
            if (a.colors)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) col[ch] = (float)a.colors[3 * (size_t)idx + ch];
            if (want_n && a.normals) {
                const float* np_ = a.normals + 3 * (size_t)idx;
                const float nw[3] = {pmn_settle(np_[0]), pmn_settle(np_[1]), pmn_settle(np_[2])};
#pragma unroll
                for (int r = 0; r < 3; ++r) n[r] = (E[4 * r] * nw[0] + E[4 * r + 1] * nw[1]) + E[4 * r + 2] * nw[2];
            }
        }
    }
    if (!hit) {
        a.depth[pix] = 0.0f;
        a.index[pix] = -1;
        if (a.rgb) a.rgb[3 * pix] = a.rgb[3 * pix + 1] = a.rgb[3 * pix + 2] = 0;
        if (a.normal) a.normal[3 * pix] = a.normal[3 * pix + 1] = a.normal[3 * pix + 2] = 0.0f;
        return;
    }
    a.depth[pix] = depth;
    a.index[pix] = (int)idx;
    float lambert = 1.0f;
    if (want_n) {
        n[0] = pmn_settle(n[0]), n[1] = pmn_settle(n[1]), n[2] = pmn_settle(n[2]);
        p[0] = pmn_settle(p[0]), p[1] = pmn_settle(p[1]), p[2] = pmn_settle(p[2]);
        const float len = pmn_settle(sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]));
        if (len > 0.0f && len < __builtin_inff()) {
            n[0] = n[0] / len, n[1] = n[1] / len, n[2] = n[2] / len;
            const float d = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2];
            if (d > 0.0f) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];  // COLMAP's convention: the normal faces the camera
            const float plen = sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
            if (a.shade && plen > 0.0f) lambert = fabsf(d) / plen;
        } else {
            n[0] = n[1] = n[2] = 0.0f;
        }
    }
    if (a.rgb)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a.rgb[3 * pix + ch] = r_byte(pmn_settle(col[ch]) * pmn_settle(lambert));
    if (a.normal)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a.normal[3 * pix + ch] = n[ch];
}

extern "C" int pmn_raster_resolve(const unsigned long long* keys, int h, int w, const float* cam_host, const float* vertices,
                                  long long n_vertices, const int* faces, long long n_faces, const unsigned char* colors,
                                  const float* normals, int shade, float* depth, int* index, unsigned char* rgb, float* normal,
                                  void* stream) {
    if (!keys || !vertices || !depth || !index) return PMN_ERR_ARG;
    if (n_vertices < 1 || n_vertices > 2147483647LL || (faces && (n_faces < 1 || n_faces > 2147483647LL)) ||
        (!faces && n_faces != 0))
        return PMN_ERR_ARG;
    ResolveArgs a;
    const int rc = r_camera(a.cam, cam_host, h, w);
    if (rc != PMN_OK) return rc;
    a.keys = keys;
    a.vertices = vertices;
    a.faces = faces;
    a.colors = colors;
    a.normals = normals;
    a.nv = n_vertices;
    a.nt = n_faces;
    a.h = h;
    a.w = w;
    a.shade = shade != 0;
    a.depth = depth;
    a.index = index;
    a.rgb = rgb;
    a.normal = normal;
    PMN_LAUNCH(resolve_kernel, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
