// cloud_plane.hip -- the two kernels behind plane segmentation of a point cloud, seeded RANSAC with a least-squares refit (DESIGN.md
// section 34; segment_cloud.py, pointcloud.segment_plane / segment_planes; tests/plane_ref.py restates everything below in numpy and is
// the yardstick; the reference has no counterpart).
//
// Arithmetic: float64 throughout, products and sums in the written order without contraction (#pragma clang fp contract(off)): the bits
// numpy's float64 gives for the same expressions.  x, y, z are (double) of the float32 coordinates, nx, ny, nz of the float32 normals.
//
//   residual   r = a * x + b * y + c * z + d of a plane (a, b, c, d), from left to right.
//   inlier     fabs(r) <= threshold and, when normals are given and min_cos > 0, fabs(a * nx + b * ny + c * nz) >= min_cos (a normal of
//              0 0 0 gives 0 >= min_cos: false).  A point with active[i] == 0 is never an inlier.
//   score      counts[h] = the number of inliers of plane h.  A plane with a non-finite entry scores 0 without a test of its own: a
//              NaN or an infinity among a, b, c, d makes r NaN or infinite for every finite point (inf * 0 = NaN, inf - inf = NaN, anything
//              else stays infinite), and neither is <= the finite threshold.
//
// pmn_plane_score.  A lane holds SCORE_SLOTS points as doubles in registers, converted once per tile (a point that is out of range or
// not active is held as NaN: never an inlier), and walks the hypotheses of its GROUP of 64.  A hypothesis is the same for every lane:
// its four doubles come through uniform read-only loads into scalar registers.  The wave's count of a hypothesis over one slot is the
// popcount of a ballot; lane j keeps the wave's running count of hypothesis 64 * group + j in ONE register, over all the tiles the
// persistent wave takes (tile = blockIdx.x, then + gridDim.x ...; group = blockIdx.y), and ends with one relaxed agent-scope integer
// atomicAdd per lane.  The counts are integer sums of integers: no floating-point value, and no count, depends on the launch shape, on the
// order in which the waves arrive or on the run.  No LDS, no per-lane array (hence no scratch).
//
// pmn_plane_inliers.  One plane: the inlier mask and the ten sums a least-squares refit needs -- the count, the sum of a = p - centre and
// the six sums of a_c * a_d, c <= d -- EXACT by exact_sum.hpp's digits: a lane splits each of its points' ten terms into five digits
// and adds them to fifty integer registers of its own (PLANE_PASSES points: far below a carry), the 64 lanes meet in one butterfly per
// digit word, lane w stores word w of the workgroup into the caller's scratch and the finishing launch adds the workgroups, carries
// and rounds once.  The power of two of each sum comes from extent, the caller's bound of |p_c - centre_c| over the active points, and
// from nothing else, so the sums are a function of (points, active, plane, threshold, min_cos, centre, extent).  No atomics.
#include "exact_sum.hpp"

#define SCORE_SLOTS 4                                    // points per lane and tile
#define SCORE_TILE (64 * SCORE_SLOTS)
#define SCORE_MAX_WAVES_X 2048                           // persistent waves per hypothesis group
#define PLANE_SUMS PMN_PLANE_SUMS
#define PLANE_WORDS (PLANE_SUMS * PMN_PLANE_LIMBS)       // 50 digit sums per workgroup: one per lane, lanes 50.. idle
#define PLANE_PASSES (PMN_PLANE_BLOCK_POINTS / 64)       // points per lane
static_assert(PMN_PLANE_LIMBS == EXACT_LIMBS, "pmn_plane_inliers' scratch is laid out in exact_sum.hpp's digits");
static_assert(PLANE_WORDS <= 64, "one digit word per lane");

#define PLANE_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

typedef ExactScale<PLANE_SUMS> PlaneScale;

struct ScoreArgs {
    const float* xyz;             // [n][3]
    const float* normals;         // [n][3] or null
    const unsigned char* active;  // [n] or null
    long long n;
    int ntiles;
    const double* planes;         // [H][4]
    int H;
    double threshold, min_cos;
    int* counts;                  // [H]
};

struct InlierArgs {
    const float* xyz;
    const float* normals;
    const unsigned char* active;
    long long n;
    double plane[4];
    double threshold, min_cos;
    double centre[3];
    PlaneScale scale;
    unsigned char* mask;          // [n] or null
    long long* partial;           // [PLANE_WORDS][nb]
    int nb;
};

__global__ __launch_bounds__(256) void plane_zero_kernel(int* counts, int H) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h < H) counts[h] = 0;
}

template <bool NORMALS>
__global__ __launch_bounds__(64) void plane_score_kernel(ScoreArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int h0 = blockIdx.y * 64;                       // the group's first hypothesis
    const int hn = min(64, a.H - h0);                     // wave-uniform, >= 1 by the launch shape
    const double nan = __builtin_nan("");
    int keep = 0;                                         // the wave's count of hypothesis h0 + lane
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        double x[SCORE_SLOTS], y[SCORE_SLOTS], z[SCORE_SLOTS], nx[SCORE_SLOTS], ny[SCORE_SLOTS], nz[SCORE_SLOTS];
#pragma unroll
        for (int s = 0; s < SCORE_SLOTS; ++s) {
            const long long t = (long long)tile * SCORE_TILE + s * 64 + lane;
            x[s] = nan, y[s] = 0.0, z[s] = 0.0, nx[s] = 0.0, ny[s] = 0.0, nz[s] = 0.0;
            if (t < a.n && (!a.active || a.active[t])) {
                x[s] = (double)a.xyz[(size_t)t * 3], y[s] = (double)a.xyz[(size_t)t * 3 + 1], z[s] = (double)a.xyz[(size_t)t * 3 + 2];
                if (NORMALS) {
                    nx[s] = (double)a.normals[(size_t)t * 3], ny[s] = (double)a.normals[(size_t)t * 3 + 1];
                    nz[s] = (double)a.normals[(size_t)t * 3 + 2];
                }
            }
        }
        for (int j = 0; j < hn; ++j) {  // uniform: the plane's four doubles are scalar loads
            const double* __restrict__ p = a.planes + (size_t)(h0 + j) * 4;
            const double pa = p[0], pb = p[1], pc = p[2], pd = p[3];
            int c = 0;
#pragma unroll
            for (int s = 0; s < SCORE_SLOTS; ++s) {
                const double r = pa * x[s] + pb * y[s] + pc * z[s] + pd;
                bool in = fabs(r) <= a.threshold;
                if (NORMALS) in = in && fabs(pa * nx[s] + pb * ny[s] + pc * nz[s]) >= a.min_cos;
                c += __popcll(__ballot(in));
            }
            if (lane == j) keep += c;
        }
    }
    if (lane < hn && keep != 0) __hip_atomic_fetch_add(a.counts + h0 + lane, keep, PLANE_RLX_AGENT);
}

// digit K .. 0 of y added to the lane's own digit sums dig[0 .. K]
template <int K>
__device__ __forceinline__ void plane_digits(double& y, long long* dig) {
    dig[K] += exact_split<K>(y);
    if constexpr (K > 0) plane_digits<K - 1>(y, dig);
}

template <bool NORMALS>
__global__ __launch_bounds__(64) void plane_inliers_kernel(InlierArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    long long dig[PLANE_SUMS][PMN_PLANE_LIMBS];  // statically indexed throughout: registers
#pragma unroll
    for (int i = 0; i < PLANE_SUMS; ++i)
#pragma unroll
        for (int k = 0; k < PMN_PLANE_LIMBS; ++k) dig[i][k] = 0;
#pragma unroll 1
    for (int pass = 0; pass < PLANE_PASSES; ++pass) {
        const long long t = (long long)blockIdx.x * PMN_PLANE_BLOCK_POINTS + pass * 64 + lane;
        if (t >= a.n) break;
        bool in = false;
        double ax = 0.0, ay = 0.0, az = 0.0;
        if (!a.active || a.active[t]) {
            const double x = (double)a.xyz[(size_t)t * 3], y = (double)a.xyz[(size_t)t * 3 + 1], z = (double)a.xyz[(size_t)t * 3 + 2];
            const double r = a.plane[0] * x + a.plane[1] * y + a.plane[2] * z + a.plane[3];
            in = fabs(r) <= a.threshold;
            if (NORMALS) {
                const double nx = (double)a.normals[(size_t)t * 3], ny = (double)a.normals[(size_t)t * 3 + 1];
                const double nz = (double)a.normals[(size_t)t * 3 + 2];
                in = in && fabs(a.plane[0] * nx + a.plane[1] * ny + a.plane[2] * nz) >= a.min_cos;
            }
            ax = x - a.centre[0], ay = y - a.centre[1], az = z - a.centre[2];
        }
        if (a.mask) a.mask[t] = in ? 1 : 0;
        if (!in) continue;
        double term[PLANE_SUMS];
        term[0] = 1.0;
        term[1] = ax, term[2] = ay, term[3] = az;
        term[4] = ax * ax, term[5] = ax * ay, term[6] = ax * az;
        term[7] = ay * ay, term[8] = ay * az, term[9] = az * az;
#pragma unroll
        for (int i = 0; i < PLANE_SUMS; ++i) {
            double y = term[i] * a.scale.to_digits[i];  // exact: a power of two
            plane_digits<PMN_PLANE_LIMBS - 1>(y, dig[i]);
        }
    }
    long long mine = 0;  // digit word `lane` of the workgroup
#pragma unroll
    for (int i = 0; i < PLANE_SUMS; ++i)
#pragma unroll
        for (int k = 0; k < PMN_PLANE_LIMBS; ++k) {
            const long long v = exact_wave_sum(dig[i][k]);
            if (lane == i * PMN_PLANE_LIMBS + k) mine = v;
        }
    if (lane < PLANE_WORDS) a.partial[(size_t)lane * a.nb + blockIdx.x] = mine;
}

__global__ __launch_bounds__(EXACT_FINISH_THREADS) void plane_finish_kernel(const long long* __restrict__ partial, int nb, PlaneScale scale,
                                                                            double* __restrict__ sums) {
    exact_finish<PLANE_SUMS>(partial, nb, scale, sums);
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------------
static int plane_point_args(const float* xyz, const float* normals, long long n, double threshold, double min_cos) {
    if (!xyz || n < 1 || n >= (1LL << 31) - 64) return PMN_ERR_ARG;
    if (!(threshold >= 0.0) || !std::isfinite(threshold)) return PMN_ERR_ARG;
    if (!(min_cos >= 0.0 && min_cos <= 1.0)) return PMN_ERR_ARG;
    if (min_cos > 0.0 && !normals) return PMN_ERR_ARG;
    return PMN_OK;
}

extern "C" int pmn_plane_score(const float* xyz, const float* normals, const unsigned char* active, long long n, const double* planes,
                               int n_planes, double threshold, double min_cos, int* counts, void* stream) {
    const int rc = plane_point_args(xyz, normals, n, threshold, min_cos);
    if (rc != PMN_OK) return rc;
    if (!planes || !counts) return PMN_ERR_ARG;
    if (n_planes < 1 || n_planes > PMN_PLANE_MAX_HYPOTHESES) return PMN_ERR_SHAPE;
    ScoreArgs a;
    a.xyz = xyz;
    a.normals = min_cos > 0.0 ? normals : nullptr;  // with min_cos == 0 the test on the normals does not exist
    a.active = active;
    a.n = n;
    a.ntiles = (int)((n + SCORE_TILE - 1) / SCORE_TILE);
    a.planes = planes;
    a.H = n_planes;
    a.threshold = threshold;
    a.min_cos = min_cos;
    a.counts = counts;
    const dim3 grid((unsigned)(a.ntiles < SCORE_MAX_WAVES_X ? a.ntiles : SCORE_MAX_WAVES_X), (unsigned)((n_planes + 63) / 64));
    PMN_LAUNCH(plane_zero_kernel, dim3((unsigned)((n_planes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, counts, n_planes);
    if (a.normals) PMN_LAUNCH(plane_score_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, a);
    else PMN_LAUNCH(plane_score_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_plane_inliers(const float* xyz, const float* normals, const unsigned char* active, long long n, const double* plane_host,
                                 double threshold, double min_cos, const double* centre_host, const double* extent_host, double* scratch,
                                 long long scratch_doubles, unsigned char* mask, double* sums, void* stream) {
    const int rc = plane_point_args(xyz, normals, n, threshold, min_cos);
    if (rc != PMN_OK) return rc;
    if (!plane_host || !centre_host || !extent_host || !scratch || !sums) return PMN_ERR_ARG;
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(plane_host[i])) return PMN_ERR_ARG;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(centre_host[c]) || !(extent_host[c] >= 0.0) || !std::isfinite(extent_host[c])) return PMN_ERR_ARG;
    if (scratch_doubles < PMN_PLANE_SCRATCH(n)) return PMN_ERR_ARG;
    InlierArgs a;
    // bounds of an inlier's terms: |a_c| <= extent_c
    const double* E = extent_host;
    const double bound[PLANE_SUMS] = {1.0, E[0], E[1], E[2], E[0] * E[0], E[0] * E[1], E[0] * E[2], E[1] * E[1], E[1] * E[2], E[2] * E[2]};
    for (int i = 0; i < PLANE_SUMS; ++i)
        if (!exact_scale(bound[i], a.scale.to_digits[i])) return PMN_ERR_SHAPE;  // the scaling must stay a normal float64
    a.xyz = xyz;
    a.normals = min_cos > 0.0 ? normals : nullptr;
    a.active = active;
    a.n = n;
    for (int i = 0; i < 4; ++i) a.plane[i] = plane_host[i];
    a.threshold = threshold;
    a.min_cos = min_cos;
    for (int c = 0; c < 3; ++c) a.centre[c] = centre_host[c];
    a.mask = mask;
    a.partial = reinterpret_cast<long long*>(scratch);
    a.nb = (int)PMN_PLANE_BLOCKS(n);
    if (a.normals) PMN_LAUNCH(plane_inliers_kernel<true>, dim3((unsigned)a.nb), dim3(64), 0, (hipStream_t)stream, a);
    else PMN_LAUNCH(plane_inliers_kernel<false>, dim3((unsigned)a.nb), dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    PMN_LAUNCH(plane_finish_kernel, dim3(PLANE_SUMS), dim3(EXACT_FINISH_THREADS), 0, (hipStream_t)stream, (const long long*)a.partial, a.nb,
               a.scale, sums);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
