// k_camera.inc — the camera model of ofk.h (ofk_set_camera): lens distortion undone (and applied) per point.  Included by k_tracks.hip.
// One thread per point, grid (ceil(pts_stride / 256), batch, arrays): the resident chains hand pts_prev and pts_next of a call to ONE
// launch as arrays 0 and 1.  float64 in the order ofk.h states (the build has no FMA contraction), one rounding to f32 at the end; the
// iteration count is a kernel argument, so the loop is wave-uniform.  Nothing is written beyond counts[b]; no atomics, no LDS.  The
// kernel is latency-bound and tiny (a few hundred points per image): it is not tuned beyond the launch count.
// src and dst may be the same buffer (the seeds are distorted in place): each thread reads its point before it writes it.
#include "k_camera_map.inc"                                     // cam_xy, cam_distort: the forward map, shared with the rectifying warp

template <int MODEL> __device__ __forceinline__ cam_xy cam_undistort(const ofk_camera &c, double x0, double y0)
{
    if (MODEL == OFK_CAMERA_BROWN) {
        const double k1 = c.k[0], k2 = c.k[1], p1 = c.k[2], p2 = c.k[3], k3 = c.k[4], k4 = c.k[5], k5 = c.k[6], k6 = c.k[7];
        double x = x0, y = y0;
        for (int it = 0; it < c.iters; ++it) {
            const double r2 = x * x + y * y;
            const double icd = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
            const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
            const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
            x = (x0 - dx) * icd;
            y = (y0 - dy) * icd;
        }
        return {x, y};
    }
    const double k1 = c.k[0], k2 = c.k[1], k3 = c.k[2], k4 = c.k[3];
    const double td = sqrt(x0 * x0 + y0 * y0);
    double t = td;
    for (int it = 0; it < c.iters; ++it) {
        const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
        t = t - (t * (1.0 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8) - td) / (1.0 + 3.0 * k1 * t2 + 5.0 * k2 * t4 + 7.0 * k3 * t6 + 9.0 * k4 * t8);
    }
    const double s = td < 1e-8 ? 1.0 : tan(t) / td;
    return {x0 * s, y0 * s};
}

// the one rounding to f32 and the fallback: a result LK or the solve could not use is the linear map of the input (lx, ly)
__device__ __forceinline__ float2 cam_finish(double rx, double ry, double lx, double ly)
{
    const float tx = (float)rx, ty = (float)ry;
    if (fabsf(tx) <= 1e6f && fabsf(ty) <= 1e6f) return make_float2(tx, ty);      // false for NaN and infinity too
    return make_float2((float)lx, (float)ly);
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_camera_undistort(const float *src0, const float *src1, float *dst0, float *dst1,
                                                          const int *__restrict__ counts, int pts_stride, ofk_camera c)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pts_stride || p >= counts[b]) return;
    const float2 *src = (const float2 *)(blockIdx.z ? src1 : src0);
    float2 *dst = (float2 *)(blockIdx.z ? dst1 : dst0);
    const size_t pi = (size_t)b * pts_stride + p;
    const float2 q = src[pi];
    const double x0 = ((double)q.x - c.cx) / c.fx, y0 = ((double)q.y - c.cy) / c.fy;
    const cam_xy u = cam_undistort<MODEL>(c, x0, y0);
    dst[pi] = cam_finish(u.x * c.fo_x + c.co_x, u.y * c.fo_y + c.co_y, x0 * c.fo_x + c.co_x, y0 * c.fo_y + c.co_y);
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_camera_distort(const float *src0, const float *src1, float *dst0, float *dst1,
                                                        const int *__restrict__ counts, int pts_stride, ofk_camera c)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pts_stride || p >= counts[b]) return;
    const float2 *src = (const float2 *)(blockIdx.z ? src1 : src0);
    float2 *dst = (float2 *)(blockIdx.z ? dst1 : dst0);
    const size_t pi = (size_t)b * pts_stride + p;
    const float2 q = src[pi];
    const double x = ((double)q.x - c.co_x) / c.fo_x, y = ((double)q.y - c.co_y) / c.fo_y;
    const cam_xy d = cam_distort<MODEL>(c, x, y);
    dst[pi] = cam_finish(d.x * c.fx + c.cx, d.y * c.fy + c.cy, x * c.fx + c.cx, y * c.fy + c.cy);
}

// arrays 1: src0 -> dst0; arrays 2: src1 -> dst1 in the same launch.  cam->model is BROWN or FISHEYE (the entry points check).
void ofk_launch_camera(hipStream_t s, const ofk_camera *cam, int distort, const float *src0, float *dst0, const float *src1, float *dst1,
                       const int *counts, int pts_stride, int batch)
{
    const dim3 grid((pts_stride + 255) / 256, batch, src1 ? 2 : 1), block(256);
    const bool fish = cam->model == OFK_CAMERA_FISHEYE;
    if (distort) {
        if (fish) hipLaunchKernelGGL(k_camera_distort<OFK_CAMERA_FISHEYE>, grid, block, 0, s, src0, src1, dst0, dst1, counts, pts_stride, *cam);
        else hipLaunchKernelGGL(k_camera_distort<OFK_CAMERA_BROWN>, grid, block, 0, s, src0, src1, dst0, dst1, counts, pts_stride, *cam);
    } else {
        if (fish) hipLaunchKernelGGL(k_camera_undistort<OFK_CAMERA_FISHEYE>, grid, block, 0, s, src0, src1, dst0, dst1, counts, pts_stride, *cam);
        else hipLaunchKernelGGL(k_camera_undistort<OFK_CAMERA_BROWN>, grid, block, 0, s, src0, src1, dst0, dst1, counts, pts_stride, *cam);
    }
}
