// metrics.hip -- ground-truth depth metrics of validation (reference train.py:127-181 process_sample, utils.py:170-221
// threshold_metrics / absolute_depth_error_metrics, models/net.py:321-342 patchmatchnet_loss).
//
// The reference scores every stage's maps against F.interpolate(gt, scale_factor=2^-s, mode="nearest") under the same down-sampled
// mask, through boolean indexing (depth[mask]) -- a device synchronisation per call, ten per batch.  Here one pass over the stage-0
// pixels reads each ground-truth value once and folds in every coarser stage at the pixels where y % 2^s == 0 && x % 2^s == 0 (the
// nearest down-sampling reads gt[y << s][x << s]); the sample's row of raw sums and exact counts stays on the device and the host turns
// it into the reference's scalars (patchmatchnet_amd/validate.py).
//
// Arithmetic: difference, absolute value and smooth-L1 (beta = 1: 0.5 * z * z for z < 1, else z - 0.5) in fp32 as torch's elementwise
// kernels compute them; IEEE comparisons (a NaN estimate is "not above t" but makes the sums NaN; a NaN ground truth is not valid);
// only the accumulation is fp64.
//
// Determinism: the number of workgroups per sample is a function of H and W only (PMN_METRICS_BLOCKS), every thread walks a fixed set
// of pixels, a workgroup reduces its threads in a fixed tree and stores its partial row into the caller's scratch (no atomics), and
// a second launch adds each sample's partial rows in workgroup order.  The rows are the same bits on every run and stream.
#include "pmn_common.hpp"

#define PMN_METRICS_THREADS 256

struct MetricsArgs {
    const float* gt;                                // [B][H][W]
    const float* dmin;                              // [B]
    const float* maps[PMN_METRICS_MAX_STAGES][PMN_METRICS_MAX_ITERS];  // [B][hs][ws] each; unused entries null
    int iters[PMN_METRICS_MAX_STAGES];              // 0 for stages >= stages
    int hs[PMN_METRICS_MAX_STAGES], ws[PMN_METRICS_MAX_STAGES];
    float thr[PMN_METRICS_MAX_THRESHOLDS];
    int n_thr, H, W, nb, vec;                       // vec: gt and the stage-0 maps are read as float4 (H*W % 4 == 0, 16-byte aligned)
    double* partial;                                // [B][nb][PMN_METRICS_ROW]
};

// 4 consecutive pixels [p, p + 4) of one map; pixels at or beyond n read as NaN (an invalid ground truth)
__device__ __forceinline__ float4 metrics_load4(const float* __restrict__ base, int p, int n, int vec) {
    if (vec) return *reinterpret_cast<const float4*>(base + p);
    const float nan = __builtin_nanf("");
    return make_float4(p < n ? base[p] : nan, p + 1 < n ? base[p + 1] : nan, p + 2 < n ? base[p + 2] : nan, p + 3 < n ? base[p + 3] : nan);
}

__device__ __forceinline__ float metrics_get(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

__global__ __launch_bounds__(PMN_METRICS_THREADS) void depth_metrics_kernel(MetricsArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = a.H * a.W, W = a.W;
    const float dmin = a.dmin[b];
    const float* __restrict__ gt = a.gt + (size_t)b * n;
    unsigned cnt[PMN_METRICS_MAX_STAGES], tcnt[PMN_METRICS_MAX_THRESHOLDS];
    double sabs[PMN_METRICS_MAX_STAGES], sl1[PMN_METRICS_MAX_STAGES][PMN_METRICS_MAX_ITERS];
#pragma unroll
    for (int s = 0; s < PMN_METRICS_MAX_STAGES; ++s) {
        cnt[s] = 0u;
        sabs[s] = 0.0;
#pragma unroll
        for (int k = 0; k < PMN_METRICS_MAX_ITERS; ++k) sl1[s][k] = 0.0;
    }
#pragma unroll
    for (int t = 0; t < PMN_METRICS_MAX_THRESHOLDS; ++t) tcnt[t] = 0u;

    for (int p0 = (blockIdx.x * PMN_METRICS_THREADS + tid) * 4; p0 < n; p0 += a.nb * PMN_METRICS_THREADS * 4) {
        const float4 g4 = metrics_load4(gt, p0, n, a.vec);
        float4 d0[PMN_METRICS_MAX_ITERS];  // stage 0: read as the ground truth is, 4 pixels at a time
#pragma unroll
        for (int k = 0; k < PMN_METRICS_MAX_ITERS; ++k)
            if (k < a.iters[0]) d0[k] = metrics_load4(a.maps[0][k] + (size_t)b * n, p0, n, a.vec);
        int y = p0 / W, x = p0 - y * W;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float g = metrics_get(g4, j);
            if (g >= dmin) {  // mask = depth_gt >= depth_min (NaN and the pixels past the end fail it)
#pragma unroll
                for (int s = 0; s < PMN_METRICS_MAX_STAGES; ++s) {
                    const int ys = y >> s, xs = x >> s;
                    if (a.iters[s] == 0 || ((y | x) & ((1 << s) - 1)) != 0 || ys >= a.hs[s] || xs >= a.ws[s]) continue;
                    cnt[s] += 1u;
                    const size_t off = ((size_t)b * a.hs[s] + ys) * a.ws[s] + xs;
#pragma unroll
                    for (int k = 0; k < PMN_METRICS_MAX_ITERS; ++k) {
                        if (k >= a.iters[s]) break;
                        const float d = s == 0 ? metrics_get(d0[k], j) : a.maps[s][k][off];
                        const float z = fabsf(d - g);
                        sl1[s][k] += (double)(z < 1.0f ? 0.5f * z * z : z - 0.5f);
                        if (k == a.iters[s] - 1) {
                            sabs[s] += (double)z;
                            if (s == 0) {
#pragma unroll
                                for (int t = 0; t < PMN_METRICS_MAX_THRESHOLDS; ++t)
                                    if (t < a.n_thr && z > a.thr[t]) tcnt[t] += 1u;
                            }
                        }
                    }
                }
            }
            if (++x == W) { x = 0; ++y; }
        }
    }

    // the workgroup's partial row: a fixed butterfly inside each wave, then the waves in order
    __shared__ double red[PMN_METRICS_THREADS / 64][PMN_METRICS_ROW];
    const int lane = tid & 63, wave = tid >> 6;
    double v[PMN_METRICS_ROW];
#pragma unroll
    for (int s = 0; s < PMN_METRICS_MAX_STAGES; ++s) {
        v[PMN_METRICS_COUNT + s] = (double)cnt[s];
        v[PMN_METRICS_ABS + s] = sabs[s];
#pragma unroll
        for (int k = 0; k < PMN_METRICS_MAX_ITERS; ++k) v[PMN_METRICS_SL1 + s * PMN_METRICS_MAX_ITERS + k] = sl1[s][k];
    }
#pragma unroll
    for (int t = 0; t < PMN_METRICS_MAX_THRESHOLDS; ++t) v[PMN_METRICS_THR + t] = (double)tcnt[t];
#pragma unroll
    for (int i = 0; i < PMN_METRICS_ROW; ++i) {
        double x = v[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        v[i] = x;
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < PMN_METRICS_ROW; ++i) red[wave][i] = v[i];
    }
    __syncthreads();
    if (tid < PMN_METRICS_ROW) {
        double x = red[0][tid];
#pragma unroll
        for (int w = 1; w < PMN_METRICS_THREADS / 64; ++w) x += red[w][tid];
        a.partial[((size_t)b * a.nb + blockIdx.x) * PMN_METRICS_ROW + tid] = x;
    }
}

// rows[b][i] = the sum over the sample's workgroups, in workgroup order
__global__ __launch_bounds__(64) void depth_metrics_finish_kernel(const double* __restrict__ partial, int nb, double* __restrict__ rows) {
    const int b = blockIdx.x, i = threadIdx.x;
    if (i >= PMN_METRICS_ROW) return;
    const double* p = partial + (size_t)b * nb * PMN_METRICS_ROW + i;
    double x = 0.0;
#pragma unroll 16  // (the loads of a group are issued together; the additions stay in workgroup order)
    for (int k = 0; k < nb; ++k) x += p[(size_t)k * PMN_METRICS_ROW];
    rows[(size_t)b * PMN_METRICS_ROW + i] = x;
}

extern "C" int pmn_depth_metrics(const float* depth_gt, const float* depth_min, const float* const* maps_host, const int* iters_host,
                                 const int* hw_host, int stages, const float* thresholds_host, int n_thresholds, int B, int H, int W,
                                 double* scratch, long long scratch_doubles, double* rows, void* stream) {
    if (!depth_gt || !depth_min || !maps_host || !iters_host || !hw_host || !scratch || !rows) return PMN_ERR_ARG;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)H * W > (1LL << 30)) return PMN_ERR_ARG;
    if (stages < 1 || stages > PMN_METRICS_MAX_STAGES || n_thresholds < 0 || n_thresholds > PMN_METRICS_MAX_THRESHOLDS)
        return PMN_ERR_SHAPE;
    if (n_thresholds > 0 && !thresholds_host) return PMN_ERR_ARG;
    if (scratch_doubles < PMN_METRICS_SCRATCH(B, H, W)) return PMN_ERR_ARG;
    MetricsArgs a = {};
    int m = 0;
    for (int s = 0; s < stages; ++s) {
        // stage s must be the nearest down-sampling of the ground truth: floor(H / 2^s) x floor(W / 2^s), at least one pixel
        if (iters_host[s] < 1 || iters_host[s] > PMN_METRICS_MAX_ITERS) return PMN_ERR_SHAPE;
        if (hw_host[2 * s] != (H >> s) || hw_host[2 * s + 1] != (W >> s) || (H >> s) < 1 || (W >> s) < 1) return PMN_ERR_SHAPE;
        a.iters[s] = iters_host[s];
        a.hs[s] = H >> s;
        a.ws[s] = W >> s;
        for (int k = 0; k < iters_host[s]; ++k, ++m) {
            if (!maps_host[m]) return PMN_ERR_ARG;
            a.maps[s][k] = maps_host[m];
        }
    }
    for (int t = 0; t < n_thresholds; ++t) a.thr[t] = thresholds_host[t];
    a.gt = depth_gt;
    a.dmin = depth_min;
    a.n_thr = n_thresholds;
    a.H = H;
    a.W = W;
    a.nb = PMN_METRICS_BLOCKS(H, W);
    bool vec = (H * W) % 4 == 0 && reinterpret_cast<uintptr_t>(depth_gt) % 16 == 0;
    for (int k = 0; k < a.iters[0]; ++k) vec = vec && reinterpret_cast<uintptr_t>(a.maps[0][k]) % 16 == 0;
    a.vec = vec ? 1 : 0;
    a.partial = scratch;
    PMN_LAUNCH(depth_metrics_kernel, dim3(a.nb, B), dim3(PMN_METRICS_THREADS), 0, (hipStream_t)stream, a);
    PMN_CHECK_LAUNCH();
    PMN_LAUNCH(depth_metrics_finish_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)scratch, a.nb, rows);
    PMN_CHECK_LAUNCH();
    return PMN_OK;
}
