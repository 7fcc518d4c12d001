// registration.hip -- the kernels behind the Tanks and Temples F-score (patchmatchnet_amd/registration.py and
// eval_tnt.py are the callers, tests/tnt_ref.py the numpy form): one ICP iteration's search + accumulation in one pass
// (pmn_icp_accumulate), the voxel-mean downsample (pmn_voxel_mean) and the crop volume (pmn_crop_prism).
//
// Arithmetic: float64 throughout, products and sums in the written order without contraction (#pragma clang fp contract(off)): the bits
// numpy's float64 gives for the same expressions.  A posed point is p' = r0 * x + r1 * y + r2 * z + t per row, left to right.
//
// pmn_icp_accumulate's sums are EXACT, which is how they come to be independent of the schedule, of the launch shape and of `order`: a
// floating-point sum depends on the order of its terms, an integer sum does not.  Every term (a float64) is scaled by a power of two
// chosen on the host from the geometry -- the target's bounding box, centre and max_dist bound every term of a matched pair -- and cut
// into PMN_ICP_LIMBS signed 32-bit digits held in int64 words; digits are added with integer adds (64 lanes by a butterfly, up to 2^31
// terms without a carry), a workgroup stores its digit sums into the caller's scratch, and a second launch adds the workgroups' digits,
// propagates the carries once and rounds the 160-bit total to float64, once.  No atomics of any kind.  What is lost: the part of a term
// below 2^-157 of the bound of its sum (truncated toward zero), and the one rounding of the total.  The digit split, the butterfly and
// the finish live in exact_sum.hpp, which pmn_plane_inliers (cloud_plane.hip) shares.
#include "exact_sum.hpp"
#include "pc_grid.hpp"

#define ICP_SUMS PMN_ICP_SUMS
#define ICP_LIMBS PMN_ICP_LIMBS
#define ICP_WORDS (ICP_SUMS * ICP_LIMBS)                      // 85 digit sums per workgroup
#define ICP_PASSES (PMN_ICP_BLOCK_POINTS / 64)                // points per lane
static_assert(ICP_LIMBS == EXACT_LIMBS, "pmn_icp_accumulate's scratch is laid out in exact_sum.hpp's digits");

typedef ExactScale<ICP_SUMS> IcpScale;

struct IcpArgs {
    GridArgs g;
    const float* src;       // [n][3]
    const int* order;       // [n] or null
    int n;
    double pose[12];        // row-major 3 x 4 [R | t]
    double centre[3];
    double max_dist;
    IcpScale scale;
    long long* partial;     // [ICP_WORDS][nb]
    int nb;
};

// p' = R p + t, float64, each row r0 * x + r1 * y + r2 * z + t from left to right
__device__ __forceinline__ void reg_pose(const double* __restrict__ P, double x, double y, double z, double& ox, double& oy, double& oz) {
#pragma clang fp contract(off)
    ox = P[0] * x + P[1] * y + P[2] * z + P[3];
    oy = P[4] * x + P[5] * y + P[6] * z + P[7];
    oz = P[8] * x + P[9] * y + P[10] * z + P[11];
}

// Digits K .. 0 of y into the wave's running sums: after the butterfly every lane holds the wave's sum of digit w = i * ICP_LIMBS + K;
// lane w % 64 keeps it.
template <int K>
__device__ __forceinline__ void icp_digits(double& y, int i, int lane, long long& keep0, long long& keep1) {
    const long long v = exact_wave_sum(exact_split<K>(y));
    const int word = i * ICP_LIMBS + K;
    if (word < 64) {
        if (lane == word) keep0 += v;
    } else {
        if (lane == word - 64) keep1 += v;
    }
    if constexpr (K > 0) icp_digits<K - 1>(y, i, lane, keep0, keep1);
}

// One wave per workgroup, as nn_distance_kernel (a far query holds up 63 neighbours, not 255); a wave takes ICP_PASSES groups of 64
// consecutive positions of the order.  After the butterfly every lane holds the wave's sum of digit w; lane w % 64 keeps it, so the
// 85 running sums cost two registers per lane.
__global__ __launch_bounds__(64) void icp_accumulate_kernel(IcpArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    long long keep0 = 0, keep1 = 0;  // digit sums lane and 64 + lane
    for (int pass = 0; pass < ICP_PASSES; ++pass) {
        const long long t = (long long)blockIdx.x * PMN_ICP_BLOCK_POINTS + pass * 64 + lane;
        if ((long long)blockIdx.x * PMN_ICP_BLOCK_POINTS + pass * 64 >= a.n) break;  // wave-uniform
        double term[ICP_SUMS];
#pragma unroll
        for (int i = 0; i < ICP_SUMS; ++i) term[i] = 0.0;
        if (t < a.n) {
            const int q = a.order ? a.order[t] : (int)t;
            double px, py, pz;
            reg_pose(a.pose, (double)a.src[(size_t)q * 3], (double)a.src[(size_t)q * 3 + 1], (double)a.src[(size_t)q * 3 + 2], px, py, pz);
            const NnBest b = nn_search(a.g, px, py, pz, a.max_dist);
            if (b.idx >= 0) {
                const float* __restrict__ tq = a.g.xyz + (size_t)b.idx * 3;
                const double ax = px - a.centre[0], ay = py - a.centre[1], az = pz - a.centre[2];
                const double bx = (double)tq[0] - a.centre[0], by = (double)tq[1] - a.centre[1], bz = (double)tq[2] - a.centre[2];
                term[0] = 1.0;
                term[1] = ax, term[2] = ay, term[3] = az;
                term[4] = bx, term[5] = by, term[6] = bz;
                term[7] = ax * bx, term[8] = ax * by, term[9] = ax * bz;
                term[10] = ay * bx, term[11] = ay * by, term[12] = ay * bz;
                term[13] = az * bx, term[14] = az * by, term[15] = az * bz;
                term[16] = b.d2;  // dx * dx + dy * dy + dz * dz of (double)q - p': the squared distance the search decided on
            }
        }
#pragma unroll
        for (int i = 0; i < ICP_SUMS; ++i) {
            double y = term[i] * a.scale.to_digits[i];  // exact: a power of two
            icp_digits<ICP_LIMBS - 1>(y, i, lane, keep0, keep1);
        }
    }
    a.partial[(size_t)lane * a.nb + blockIdx.x] = keep0;
    if (lane + 64 < ICP_WORDS) a.partial[(size_t)(lane + 64) * a.nb + blockIdx.x] = keep1;
}

// sums[i]: one workgroup (one wave) per sum (exact_sum.hpp)
__global__ __launch_bounds__(EXACT_FINISH_THREADS) void icp_finish_kernel(const long long* __restrict__ partial, int nb, IcpScale scale,
                                                                          double* __restrict__ sums) {
    exact_finish<ICP_SUMS>(partial, nb, scale, sums);
}

// ---- pmn_voxel_mean ---------------------------------------------------------------------------------------------------------------------
struct VoxelArgs {
    const float* xyz;          // [n][3]
    const float* attr;         // [n][C] or null
    const long long* starts;   // [m + 1]
    long long m;
    int C;
    float* out_xyz;            // [m][3]
    float* out_attr;           // [m][C]
};

// channel c of point i: 0..2 the position, 3.. the attribute
__device__ __forceinline__ double voxel_value(const VoxelArgs& a, long long i, int c) {
    return c < 3 ? (double)a.xyz[(size_t)i * 3 + c] : (double)a.attr[(size_t)i * a.C + (c - 3)];
}
__device__ __forceinline__ void voxel_store(const VoxelArgs& a, long long r, int c, double sum, long long len) {
    const float v = (float)(sum / (double)len);
    if (c < 3) a.out_xyz[(size_t)r * 3 + c] = v;
    else a.out_attr[(size_t)r * a.C + (c - 3)] = v;
}

__global__ __launch_bounds__(256) void voxel_mean_kernel(VoxelArgs a) {
#pragma clang fp contract(off)
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int nc = 3 + (a.attr ? a.C : 0);
    long long s = 0, len = 0;
    if (r < a.m) {
        s = a.starts[r];
        len = a.starts[r + 1] - s;
    }
    const bool is_long = len > PMN_VOXEL_LONG_RUN;
    if (r < a.m && !is_long) {  // a lane per run, in index order
        for (int c = 0; c < nc; ++c) {
            double sum = 0.0;
            for (long long i = s; i < s + len; ++i) sum += voxel_value(a, i, c);
            voxel_store(a, r, c, sum, len);
        }
    }
    // the wave's long runs, one after the other: lane l sums the points l, l + 64, ... of the run in index order, the 64 sums meet in a
    // butterfly (x += x of lane ^ 32, ^ 16, ... ^ 1)
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const long long rs = __shfl(s, owner, 64), rl = __shfl(len, owner, 64), rr = __shfl(r, owner, 64);
        for (int c = 0; c < nc; ++c) {
            double sum = 0.0;
            for (long long i = rs + lane; i < rs + rl; i += 64) sum += voxel_value(a, i, c);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            if (lane == 0) voxel_store(a, rr, c, sum, rl);
        }
    }
}

// ---- pmn_crop_prism ---------------------------------------------------------------------------------------------------------------------
struct CropArgs {
    const float* xyz;       // [n][3]
    long long n;
    const double* polygon;  // [k][2]
    int k, axis, u, v, has_pose;
    double axis_min, axis_max;
    double pose[12];
    unsigned char* mask;    // [n]
};

__global__ __launch_bounds__(256) void crop_prism_kernel(CropArgs a) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    double p[3] = {(double)a.xyz[(size_t)t * 3], (double)a.xyz[(size_t)t * 3 + 1], (double)a.xyz[(size_t)t * 3 + 2]};
    if (a.has_pose) reg_pose(a.pose, p[0], p[1], p[2], p[0], p[1], p[2]);
    const double c = a.axis == 0 ? p[0] : a.axis == 1 ? p[1] : p[2];
    const double px = a.u == 0 ? p[0] : p[1], py = a.v == 1 ? p[1] : p[2];  // (u, v) is (1, 2), (0, 2) or (0, 1)
    bool inside = false;
    if (a.axis_min <= c && c <= a.axis_max) {
        double xj = a.polygon[(size_t)(a.k - 1) * 2], yj = a.polygon[(size_t)(a.k - 1) * 2 + 1];
        for (int i = 0; i < a.k; ++i) {  // the polygon is the same for every lane: uniform loads
            const double xi = a.polygon[(size_t)i * 2], yi = a.polygon[(size_t)i * 2 + 1];
            if ((yi > py) != (yj > py) && px < (xj - xi) * (py - yi) / (yj - yi) + xi) inside = !inside;
            xj = xi;
            yj = yi;
        }
    }
    a.mask[t] = inside ? 1 : 0;
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------------
static bool reg_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

extern "C" int pmn_icp_accumulate(const float* to_xyz, const long long* to_keys, long long n_to, const double* origin_host, double cell,
                                  const int* dims_host, const float* src, const int* order, long long n, const double* pose_host,
                                  const double* centre_host, double max_dist, double* scratch, long long scratch_doubles, double* sums,
                                  void* stream) {
    IcpArgs a;
    const int rc = grid_args(a.g, to_xyz, to_keys, n_to, origin_host, cell, dims_host);
    if (rc != PMN_OK) return rc;
    if (!src || !pose_host || !centre_host || !scratch || !sums || n < 1 || n >= (1LL << 31) - 64) return PMN_ERR_ARG;
    if (!(max_dist > 0.0) || !std::isfinite(max_dist) || !reg_finite(pose_host, 12) || !reg_finite(centre_host, 3)) return PMN_ERR_ARG;
    if (scratch_doubles < PMN_ICP_SCRATCH(n)) return PMN_ERR_ARG;
    // bounds of the terms of a matched pair: the target lies in [origin, origin + dims * cell] (one cell of margin for the rounding of a
    // point's cell), so |b_c| <= B_c; |p' - q| < max_dist, so |a_c| < B_c + max_dist
    double A[3], B[3];
    for (int c = 0; c < 3; ++c) {
        const double lo = origin_host[c] - cell, hi = origin_host[c] + ((double)dims_host[c] + 1.0) * cell;
        B[c] = std::fmax(std::fabs(lo - centre_host[c]), std::fabs(hi - centre_host[c]));
        A[c] = B[c] + max_dist;
    }
    double bound[ICP_SUMS];
    bound[0] = 1.0;
    for (int c = 0; c < 3; ++c) {
        bound[1 + c] = A[c];
        bound[4 + c] = B[c];
        for (int d = 0; d < 3; ++d) bound[7 + 3 * c + d] = A[c] * B[d];
    }
    bound[16] = max_dist * max_dist;
    for (int i = 0; i < ICP_SUMS; ++i) {
        if (!exact_scale(bound[i], a.scale.to_digits[i])) return PMN_ERR_SHAPE;  // the scaling must stay a normal float64
    }
    a.src = src;
    a.order = order;
    a.n = (int)n;
    for (int i = 0; i < 12; ++i) a.pose[i] = pose_host[i];
    for (int i = 0; i < 3; ++i) a.centre[i] = centre_host[i];
    a.max_dist = max_dist;
    a.partial = reinterpret_cast<long long*>(scratch);
    a.nb = (int)PMN_ICP_BLOCKS(n);
    PMN_LAUNCH(icp_accumulate_kernel, dim3((unsigned)a.nb), dim3(64), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    PMN_LAUNCH(icp_finish_kernel, dim3(ICP_SUMS), dim3(EXACT_FINISH_THREADS), 0, (hipStream_t)stream, (const long long*)a.partial, a.nb,
               a.scale, sums);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_voxel_mean(const float* xyz, const float* attr, int channels, long long n, const long long* starts, long long m,
                              float* out_xyz, float* out_attr, void* stream) {
    if (!xyz || !starts || !out_xyz || n < 1 || n >= (1LL << 31) - 64 || m < 1 || m > n) return PMN_ERR_ARG;
    if (attr && (!out_attr || channels < 1)) return PMN_ERR_ARG;
    if (attr && channels > PMN_VOXEL_MAX_CHANNELS) return PMN_ERR_SHAPE;
    VoxelArgs a;
    a.xyz = xyz;
    a.attr = attr;
    a.starts = starts;
    a.m = m;
    a.C = attr ? channels : 0;
    a.out_xyz = out_xyz;
    a.out_attr = out_attr;
    PMN_LAUNCH(voxel_mean_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}

extern "C" int pmn_crop_prism(const float* xyz, long long n, const double* polygon, int k, int axis, double axis_min, double axis_max,
                              const double* pose_host, unsigned char* mask, void* stream) {
    if (!xyz || !polygon || !mask || n < 1 || n >= (1LL << 31) - 64 || axis < 0 || axis > 2) return PMN_ERR_ARG;
    if (k < 3 || k > PMN_CROP_MAX_VERTICES) return PMN_ERR_SHAPE;
    if (std::isnan(axis_min) || std::isnan(axis_max) || (pose_host && !reg_finite(pose_host, 12))) return PMN_ERR_ARG;
    CropArgs a;
    a.xyz = xyz;
    a.n = n;
    a.polygon = polygon;
    a.k = k;
    a.axis = axis;
    a.u = axis == 0 ? 1 : 0;
    a.v = axis == 2 ? 1 : 2;
    a.has_pose = pose_host ? 1 : 0;
    for (int i = 0; i < 12; ++i) a.pose[i] = pose_host ? pose_host[i] : 0.0;
    a.axis_min = axis_min;
    a.axis_max = axis_max;
    a.mask = mask;
    PMN_LAUNCH(crop_prism_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
