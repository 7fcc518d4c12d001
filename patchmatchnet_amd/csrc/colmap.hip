// colmap.hip -- view selection of the COLMAP import (reference colmap_input.py:336-366, calc_score and its pair loop).
//
// The reference scores every image pair (i < j) from image i's point3D_id list: each id of that list that is also in image j's list
// adds exp(-(theta - theta0)^2 / (2 sigma^2)), theta = the triangulation angle at the point in degrees, sigma = sigma1 below theta0
// and sigma2 above.  It finds the shared ids by a Python list-membership test, O(|keypoints_i| x |keypoints_j|) per pair.  Here the
// intersection is read off the point's track instead: observation k of image i (point p) contributes to exactly the images j > i
// of p's distinct-observer list.  patchmatchnet_amd/colmap.py builds both lists (CSR) on the host.
//
// Order contract: score(i, j) is the SEQUENTIAL fp64 sum of its terms in the order of image i's observations -- the reference's
// order -- so the matrix is the same bits on every run and for every launch geometry, and differs from numpy only by the ulps of
// acos / exp and of BLAS's 3-term dot.  IEEE throughout (no fast-math, no contraction, no clamping): a point at a camera centre or
// an acos argument beyond +-1 gives NaN as numpy does.
//
// One wave owns the tile (row i, column block [j0, j0 + PMN_VS_COLS)) with its fp64 accumulators in LDS.  It walks row i's
// observations 64 at a time, one lane per observation: each lane counts its track entries j > i inside the block, a wave scan
// places the lanes' (j, term) lists one after another in an LDS staging area (as many leading lanes as fit), the lanes compute and
// stage their terms in parallel, and the wave then adds the staged terms in observation order -- one observation per step, its
// entries spread over the lanes (the j of one observation are distinct, so the lanes of a step never collide).  An observation
// whose entries alone exceed the staging area is computed and added by the whole wave directly.  The owning wave finally writes
// score[i][j] and score[j][i] for its j > i (and the diagonal zero), so every entry of the N x N matrix is written exactly once.
#include "pmn_common.hpp"

#define PMN_VS_COLS 4096   // columns per tile: 32 KiB of fp64 accumulators
#define PMN_VS_STAGE 1024  // staged (j, term) pairs per chunk: 12 KiB

struct ViewScoreArgs {
    const double* cam_centers;  // [N][3]
    const double* xyz;          // [P][3]
    const long long* obs_ptr;   // [N + 1]
    const int* obs_pt;          // [obs_ptr[N]] dense point indices, image order, -1 dropped, duplicates kept
    const long long* trk_ptr;   // [P + 1]
    const int* trk_img;         // [trk_ptr[P]] distinct observing images per point, ascending
    double* score;              // [N][N]
    long long n_obs, n_trk;     // sizes of obs_pt / trk_img (reads are clamped to them)
    int N, P, cols;             // cols = accumulators per tile = min(N, PMN_VS_COLS)
    double theta0, sigma1, sigma2;
};

// one term of calc_score, in numpy's operation order
__device__ __forceinline__ double view_term(const double* __restrict__ ci, const double* __restrict__ cj,
                                            const double* __restrict__ p, double theta0, double sigma1, double sigma2) {
#pragma clang fp contract(off)
    const double a0 = ci[0] - p[0], a1 = ci[1] - p[1], a2 = ci[2] - p[2];
    const double b0 = cj[0] - p[0], b1 = cj[1] - p[1], b2 = cj[2] - p[2];
    const double dot = a0 * b0 + a1 * b1 + a2 * b2;
    const double na = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
    const double nb = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    constexpr double kDeg = 180.0 / 3.141592653589793;  // (180 / np.pi): the same correctly rounded quotient
    const double theta = kDeg * acos(dot / na / nb);
    const double d = theta - theta0;
    const double s = theta <= theta0 ? sigma1 : sigma2;  // NaN theta takes sigma2, as the reference's comparison does
    return exp(-d * d / (2.0 * (s * s)));
}

// first index in [lo, hi) whose image is >= v (tracks are ascending)
__device__ __forceinline__ long long track_lower_bound(const int* __restrict__ trk, long long lo, long long hi, int v) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (trk[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void view_scores_kernel(ViewScoreArgs a) {
    extern __shared__ double vs_lds[];
    double* acc = vs_lds;                                        // [cols] (only [lo - j0, j1 - j0) used)
    double* st_term = vs_lds + a.cols;                           // [PMN_VS_STAGE]
    int* st_j = reinterpret_cast<int*>(st_term + PMN_VS_STAGE);  // [PMN_VS_STAGE]
    const int i = blockIdx.x, lane = threadIdx.x;
    const int j0 = blockIdx.y * PMN_VS_COLS, j1 = min(j0 + PMN_VS_COLS, a.N);
    const int lo = max(i + 1, j0);
    if (lane == 0 && i >= j0 && i < j1) a.score[(size_t)i * a.N + i] = 0.0;
    if (lo >= j1) return;  // nothing above the diagonal in this block
    for (int j = lo + lane; j < j1; j += 64) acc[j - j0] = 0.0;
    __syncthreads();

    const double* ci = a.cam_centers + (size_t)i * 3;
    long long cur = max(a.obs_ptr[i], 0LL);
    const long long end = min(a.obs_ptr[i + 1], a.n_obs);
    while (cur < end) {  // wave-uniform
        const long long k = cur + lane;
        long long t0 = 0, t1 = 0;
        int p = -1;
        if (k < end) {
            p = a.obs_pt[k];
            if (p >= 0 && p < a.P) {
                const long long b0 = min(max(a.trk_ptr[p], 0LL), a.n_trk), b1 = min(max(a.trk_ptr[p + 1], b0), a.n_trk);
                t0 = track_lower_bound(a.trk_img, b0, b1, lo);
                t1 = track_lower_bound(a.trk_img, t0, b1, j1);
            }
        }
        const int cnt = (int)min(t1 - t0, (long long)PMN_VS_STAGE + 1);
        int incl = cnt;  // inclusive wave scan of the counts
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        const int excl = incl - cnt;
        // leading lanes whose lists fit the staging area (incl is non-decreasing, so they are a prefix of the valid lanes)
        const int take = __popcll(__ballot(k < end && incl <= PMN_VS_STAGE));
        if (take == 0) {
            // observation `cur` alone overflows the staging area: the whole wave computes and adds its entries directly
            const int p0 = __shfl(p, 0, 64);
            const long long s0 = __shfl(t0, 0, 64), s1 = __shfl(t1, 0, 64);
            const double* pp = a.xyz + (size_t)p0 * 3;
            for (long long e = s0 + lane; e < s1; e += 64) {
                const int j = a.trk_img[e];
                if (j >= lo && j < j1)
                    acc[j - j0] += view_term(ci, a.cam_centers + (size_t)j * 3, pp, a.theta0, a.sigma1, a.sigma2);
            }
            __syncthreads();
            cur += 1;
            continue;
        }
        if (lane < take && cnt > 0) {
            const double* pp = a.xyz + (size_t)p * 3;
            for (int e = 0; e < cnt; ++e) {
                const int j = a.trk_img[t0 + e];
                const bool in = j >= lo && j < j1;
                st_j[excl + e] = in ? j : -1;
                st_term[excl + e] = in ? view_term(ci, a.cam_centers + (size_t)j * 3, pp, a.theta0, a.sigma1, a.sigma2) : 0.0;
            }
        }
        __syncthreads();
        for (int s = 0; s < take; ++s) {  // observation order
            const int off = __shfl(excl, s, 64), n = __shfl(cnt, s, 64);
            for (int e = lane; e < n; e += 64) {
                const int j = st_j[off + e];
                if (j >= 0) acc[j - j0] += st_term[off + e];
            }
            __syncthreads();  // the next observation may add to the same accumulators
        }
        cur += take;
    }
    for (int j = lo + lane; j < j1; j += 64) {
        const double v = acc[j - j0];
        a.score[(size_t)i * a.N + j] = v;
        a.score[(size_t)j * a.N + i] = v;
    }
}

extern "C" int pmn_view_scores(const double* cam_centers, const double* xyz, const long long* obs_ptr, const int* obs_pt,
                               const long long* trk_ptr, const int* trk_img, int N, int P, long long n_obs, long long n_trk,
                               double theta0, double sigma1, double sigma2, double* score, void* stream) {
    if (!cam_centers || !obs_ptr || !trk_ptr || !score || N < 1 || P < 0 || n_obs < 0 || n_trk < 0) return PMN_ERR_ARG;
    if ((P > 0 && !xyz) || (n_obs > 0 && !obs_pt) || (n_trk > 0 && !trk_img)) return PMN_ERR_ARG;
    if ((long long)N * N > (1LL << 40)) return PMN_ERR_ARG;
    ViewScoreArgs a;
    a.cam_centers = cam_centers;
    a.xyz = xyz;
    a.obs_ptr = obs_ptr;
    a.obs_pt = obs_pt;
    a.trk_ptr = trk_ptr;
    a.trk_img = trk_img;
    a.score = score;
    a.n_obs = n_obs;
    a.n_trk = n_trk;
    a.N = N;
    a.P = P;
    a.theta0 = theta0;
    a.sigma1 = sigma1;
    a.sigma2 = sigma2;
    a.cols = N < PMN_VS_COLS ? N : PMN_VS_COLS;
    const size_t lds = (size_t)a.cols * sizeof(double) + (size_t)PMN_VS_STAGE * (sizeof(double) + sizeof(int));  // <= 44 KiB
    PMN_LAUNCH(view_scores_kernel, dim3(N, (N + PMN_VS_COLS - 1) / PMN_VS_COLS), dim3(64), lds, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
