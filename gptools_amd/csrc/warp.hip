// warp.hip -- the input warp on the device (gpt_set_warp / gpt_predict / gpt_kbuild with layers set): O(N D) work in front of
// the builders, which then run on the warped points unchanged and take the chain-rule factor S_i S_j on tiles that carry a
// derivative order (kbuild_kernel.hpp, WARP).  ref: gptools/kernel/warping.py:491-505.
#include "common.hpp"
#include "warp.hpp"

#define WP_THREADS 256

// One lane per (point, dimension): a workgroup takes WP_THREADS / D whole points, so the D slopes of a point sit in one
// workgroup; lane d == 0 multiplies them in dimension order (one fixed order: the same bits wherever the point is evaluated).
__global__ __launch_bounds__(WP_THREADS) void warp_points_kernel(WarpLayers wl, const double *X, const int32_t *__restrict__ n,
                                                                 int64_t N, double *Xw, double *__restrict__ S)
{
    __shared__ double sl[WP_THREADS];
    const int D = wl.D;
    const int per = WP_THREADS / D;
    const int t = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * per + t / D;
    const int d = t % D;
    const bool live = t < per * D && i < N;
    double s = 1.0;
    if (live) {
        const double w = gpt_warp_coord(wl, d, X[i * D + d], &s);
        if (n[i * D + d] != 1) s = 1.0;
        Xw[i * D + d] = w;
    }
    sl[t] = s;
    __syncthreads();
    if (live && d == 0) {
        double p = sl[t];
        for (int q = 1; q < D; q++) p *= sl[t + q];
        S[i] = p;
    }
}

// Element blockIdx.y of a batch: the same lanes, the layers' parameters from device memory (gpt_set_warp_batch).
__global__ __launch_bounds__(WP_THREADS) void warp_points_batch_kernel(WarpLayers wl, const double *__restrict__ params,
                                                                       const double *__restrict__ X, const int32_t *__restrict__ n,
                                                                       int64_t N, double *__restrict__ Xw, double *__restrict__ S)
{
    __shared__ double sl[WP_THREADS];
    const int D = wl.D;
    const int per = WP_THREADS / D;
    const int t = (int)threadIdx.x;
    const int64_t b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * per + t / D;
    const int d = t % D;
    const bool live = t < per * D && i < N;
    double s = 1.0;
    if (live) {
        const double w = gpt_warp_chain(wl.nlayers, wl.type, params + b * wl.nlayers * 2 * D, 2 * D, d, X[i * D + d], &s);
        if (n[i * D + d] != 1) s = 1.0;
        Xw[(b * N + i) * D + d] = w;
    }
    sl[t] = s;
    __syncthreads();
    if (live && d == 0) {
        double p = sl[t];
        for (int q = 1; q < D; q++) p *= sl[t + q];
        S[b * N + i] = p;
    }
}

__global__ __launch_bounds__(256) void warp_scale_diag_kernel(double *__restrict__ v, const double *__restrict__ S, int64_t M)
{
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a < M) v[a] *= S[a] * S[a];
}

int launch_warp_points(hipStream_t st, const WarpLayers &wl, const double *dX, const int32_t *dn, int64_t N, double *dXw,
                       double *dS)
{
    if (N <= 0) return GPT_OK;
    if (wl.nlayers < 1 || wl.nlayers > GPT_WARP_MAX_LAYERS || wl.D < 1 || wl.D > GPT_MAX_DIM) {
        gpt_set_error("warp: %d layers over %d dimensions", wl.nlayers, wl.D);
        return GPT_E_ARG;
    }
    const int per = WP_THREADS / wl.D;
    dim3 grid((unsigned)((N + per - 1) / per)), block(WP_THREADS);
    hipLaunchKernelGGL(warp_points_kernel, grid, block, 0, st, wl, dX, dn, N, dXw, dS);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_warp_points_batch(hipStream_t st, const WarpLayers &wl, const double *d_params, int64_t nbatch, const double *dX,
                             const int32_t *dn, int64_t N, double *dXw, double *dS)
{
    if (N <= 0 || nbatch <= 0) return GPT_OK;
    if (wl.nlayers < 1 || wl.nlayers > GPT_WARP_MAX_LAYERS || wl.D < 1 || wl.D > GPT_MAX_DIM || nbatch > 65535) {
        gpt_set_error("warp batch: %d layers over %d dimensions, %lld elements", wl.nlayers, wl.D, (long long)nbatch);
        return GPT_E_ARG;
    }
    const int per = WP_THREADS / wl.D;
    dim3 grid((unsigned)((N + per - 1) / per), (unsigned)nbatch), block(WP_THREADS);
    hipLaunchKernelGGL(warp_points_batch_kernel, grid, block, 0, st, wl, d_params, dX, dn, N, dXw, dS);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_warp_scale_diag(hipStream_t st, double *dv, const double *dS, int64_t M)
{
    if (M <= 0) return GPT_OK;
    hipLaunchKernelGGL(warp_scale_diag_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, dv, dS, M);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}
