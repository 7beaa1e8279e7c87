// k_tracks.hip — feature lifecycle of a video stream on the device:
// velocity_measurment_node:131-173 with its ''' blocks restored — track the previous positions, keep status==1, and when
// few features were left re-detect with a mask of discs around the old positions and append.  gfx950.
#include "ofk_internal.h"
#include <stdlib.h>
#include "k_rows.inc"

// mask := 1, then zero a disc of `radius` around every track (centre = truncated position, dx^2+dy^2 <= r^2).
// grid (pts_stride, batch); block 256.  Streams whose limit is <= 0 (no re-detection this step) are skipped.
__global__ __launch_bounds__(256) void k_disc_mask(uint8_t *__restrict__ mask, size_t mask_stride, int h, int w,
                                                   const float *__restrict__ pts, const int *__restrict__ counts,
                                                   int pts_stride, int radius, const int *__restrict__ limit)
{
    const int b = blockIdx.y, p = blockIdx.x;
    if (limit[b] <= 0 || p >= counts[b]) return;
    const float *q = pts + ((size_t)b * pts_stride + p) * 2;
    const int cx = (int)q[0], cy = (int)q[1];
    const int side = 2 * radius + 1;
    uint8_t *m = mask + (size_t)b * mask_stride;
    for (int i = threadIdx.x; i < side * side; i += 256) {
        const int dy = i / side - radius, dx = i - (i / side) * side - radius;
        const int x = cx + dx, y = cy + dy;
        if (dx * dx + dy * dy <= radius * radius && x >= 0 && x < w && y >= 0 && y < h) m[(size_t)y * w + x] = 0;
    }
}

void ofk_launch_disc_mask(hipStream_t s, uint8_t *mask, size_t mask_stride, int h, int w, const float *pts, const int *counts,
                          int pts_stride, int radius, const int *limit, int batch)
{
    hipLaunchKernelGGL(k_disc_mask, dim3(pts_stride, batch), dim3(256), 0, s, mask, mask_stride, h, w, pts, counts, pts_stride, radius, limit);
}

// limit[b] = max_feat - count[b] if count[b] <= min_feat else 0   (node:157-163)
__global__ void k_redetect_limits(const int *__restrict__ counts, int min_feat, int max_feat, int *__restrict__ limit, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) limit[b] = counts[b] <= min_feat ? max(0, max_feat - counts[b]) : 0;
}

void ofk_launch_redetect_limits(hipStream_t s, const int *counts, int min_feat, int max_feat, int *limit, int batch)
{
    hipLaunchKernelGGL(k_redetect_limits, dim3((batch + 63) / 64), dim3(64), 0, s, counts, min_feat, max_feat, limit, batch);
}

// tracks := next_pts[status == 1] in order (node:134), then the re-detected corners appended (node:166).  One block per stream, k_rows.inc's walk.
__global__ __launch_bounds__(256) void k_update_tracks(const float *__restrict__ next_pts, const uint8_t *__restrict__ status,
                                                       const int *__restrict__ counts_in, int pts_stride,
                                                       const float *__restrict__ new_pts, const int *__restrict__ new_counts,
                                                       float *__restrict__ tracks, int *__restrict__ counts_out, int max_total)
{
    __shared__ row_walk s_rows;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = counts_in[b];
    const float *src = next_pts + (size_t)b * pts_stride * 2;
    const uint8_t *st = status + (size_t)b * pts_stride;
    float *dst = tracks + (size_t)b * pts_stride * 2;
    rows_begin(s_rows);
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool keep = i < n && st[i] != 0;
        const float x = keep ? src[2 * i] : 0.f, y = keep ? src[2 * i + 1] : 0.f;
        const int pos = rows_place(s_rows, keep);
        if (keep) { dst[2 * pos] = x; dst[2 * pos + 1] = y; }
        rows_next(s_rows);
    }
    const int total = s_rows.base;
    const int extra = rows_extra(new_counts, b, max_total, pts_stride, total);   // pts_stride >= max_total on the stream path: its clamp is idle there
    for (int i = tid; i < extra; i += 256) {
        dst[2 * (total + i)] = new_pts[((size_t)b * pts_stride + i) * 2];
        dst[2 * (total + i) + 1] = new_pts[((size_t)b * pts_stride + i) * 2 + 1];
    }
    if (tid == 0) counts_out[b] = total + extra;
}

void ofk_launch_update_tracks(hipStream_t s, const float *next_pts, const uint8_t *status, const int *counts_in, int pts_stride,
                              const float *new_pts, const int *new_counts, float *tracks, int *counts_out, int max_total, int batch)
{
    hipLaunchKernelGGL(k_update_tracks, dim3(batch), dim3(256), 0, s, next_pts, status, counts_in, pts_stride, new_pts, new_counts, tracks,
                       counts_out, max_total);
}

// of_module.py:83-86: a stream that was left with <= min_feat tracks REPLACES them by a fresh detection (maxCorners = max_feat -
// count, no mask) on its previous frame.  One block per stream; streams whose budget (limit) is 0 keep their tracks.
__global__ __launch_bounds__(256) void k_replace_tracks(const int *__restrict__ limit, const float *__restrict__ new_pts,
                                                        const int *__restrict__ new_counts, int pts_stride, float *__restrict__ tracks,
                                                        int *__restrict__ counts)
{
    const int b = blockIdx.x;
    if (!rows_stream_on(b, 0, gridDim.x, limit)) return;
    const int n = max(new_counts[b], 0);
    for (int i = threadIdx.x; i < 2 * n; i += 256) tracks[(size_t)b * pts_stride * 2 + i] = new_pts[(size_t)b * pts_stride * 2 + i];
    if (threadIdx.x == 0) counts[b] = n;
}

void ofk_launch_replace_tracks(hipStream_t s, const int *limit, const float *new_pts, const int *new_counts, int pts_stride, float *tracks,
                               int *counts, int batch)
{
    hipLaunchKernelGGL(k_replace_tracks, dim3(batch), dim3(256), 0, s, limit, new_pts, new_counts, pts_stride, tracks, counts);
}

// Start positions of a seeded LK (ofk.h: ofk_set_lk_seed): the flow the pair's sensors predict, added to every point.  One thread
// per point, float64 in the order ofk.h states (the build has no FMA contraction); k_flow_model's expression with the pixel
// scaling folded in.  mode OFK_SEED_ROTATION drops the translational part (v = 0).  imu != NULL: normal, omega and velocity come
// from the resident IMU state, as k_stream_fuse takes them.  A seed LK could not use (scaling or d zero, not finite, beyond
// 1e6) is replaced by the point itself, which is the unseeded start.
__global__ __launch_bounds__(256) void k_seed_points(const float *__restrict__ pts, const int *__restrict__ counts, int pts_stride,
                                                     const double *__restrict__ sensors, const double *__restrict__ imu, int mode,
                                                     double gain, float *__restrict__ seed)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pts_stride || p >= counts[b]) return;
    const double *sn = sensors + (size_t)b * OFK_SENSOR_DOUBLES;
    const double *ist = imu ? imu + (size_t)b * OFK_IMU_STATE : nullptr;
    const double d = sn[0], scaling = sn[19], cx = sn[20], cy = sn[21];
    const double n0 = ist ? ist[15] : sn[1], n1 = ist ? ist[16] : sn[2], n2 = ist ? ist[17] : sn[3];
    const double o0 = ist ? ist[18] : sn[4], o1 = ist ? ist[19] : sn[5], o2 = ist ? ist[20] : sn[6];
    const bool rot = mode == OFK_SEED_ROTATION;
    const double v0 = rot ? 0.0 : ist ? ist[0] : sn[22], v1 = rot ? 0.0 : ist ? ist[1] : sn[23], v2 = rot ? 0.0 : ist ? ist[2] : sn[24];
    const size_t pi = (size_t)b * pts_stride + p;
    const float fpx = pts[2 * pi], fpy = pts[2 * pi + 1];
    float sx = fpx, sy = fpy;
    if (scaling != 0.0 && d != 0.0) {
        const double px = (double)fpx, py = (double)fpy;
        const double x = (px - cx) * scaling, y = (py - cy) * scaling;
        const double k = (n0 * x + n1 * y + n2) / d;
        const double w0 = o1 - o2 * y, w1 = o2 * x - o0, w2 = o0 * y - o1 * x;
        const double fx = k * (v0 - v2 * x) + (w0 - w2 * x), fy = k * (v1 - v2 * y) + (w1 - w2 * y);
        const float tx = (float)(px + gain * fx / scaling), ty = (float)(py + gain * fy / scaling);
        if (fabsf(tx) <= 1e6f && fabsf(ty) <= 1e6f) { sx = tx; sy = ty; }      // false for NaN and infinity too
    }
    seed[2 * pi] = sx; seed[2 * pi + 1] = sy;
}

void ofk_launch_seed_points(hipStream_t s, const float *pts, const int *counts, int pts_stride, const double *sensors,
                            const double *imu_state, int mode, double gain, float *seed_out, int batch)
{
    hipLaunchKernelGGL(k_seed_points, dim3((pts_stride + 255) / 256, batch), dim3(256), 0, s, pts, counts, pts_stride, sensors, imu_state,
                       mode, gain, seed_out);
}

// The track gates (ofk.h: ofk_set_track_gate, rules 3-5): per used point the squared forward-backward distance in float32 as
// written there (the build has no FMA contraction), status := keep, and the image's four counts.  One workgroup per image, threads
// stride over its points; the counts are ballots summed per wave, then across the four waves through LDS, and written by one thread
// with plain stores: no atomics, so a second launch on the same buffers gives the same bits.
__global__ __launch_bounds__(256) void k_track_gate(const float *__restrict__ prev_pts, const float *__restrict__ back_pts,
                                                    const uint8_t *__restrict__ st_back, const float *__restrict__ err,
                                                    const int *__restrict__ counts, int pts_stride, int fb_on, float thr2, int err_on,
                                                    float err_max, uint8_t *__restrict__ status, float *__restrict__ fb2,
                                                    int *__restrict__ stats)
{
    __shared__ int s_cnt[4][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(counts[b], pts_stride);
    const size_t base = (size_t)b * pts_stride;
    int c_fwd = 0, c_lost = 0, c_far = 0, c_cap = 0;             // wave-uniform
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool in = i < n;
        const size_t pi = base + (in ? i : 0);
        const bool fwd = in && status[pi] == 1;
        bool lost = false, far = false;
        if (fb_on) {
            const bool sb = st_back[pi] == 1;
            const float dx = back_pts[2 * pi] - prev_pts[2 * pi], dy = back_pts[2 * pi + 1] - prev_pts[2 * pi + 1];
            const float d2 = dx * dx + dy * dy;
            lost = fwd && !sb;
            far = fwd && sb && !(d2 <= thr2);                    // a NaN fails the comparison
            if (in) fb2[pi] = fwd && sb ? d2 : __builtin_inff();
        }
        const bool cap = fwd && !lost && !far && err_on && !(err[pi] <= err_max);
        if (in) status[pi] = fwd && !lost && !far && !cap;
        c_fwd += __popcll(__ballot(fwd)); c_lost += __popcll(__ballot(lost));
        c_far += __popcll(__ballot(far)); c_cap += __popcll(__ballot(cap));
    }
    if (lane == 0) { s_cnt[wave][0] = c_fwd; s_cnt[wave][1] = c_lost; s_cnt[wave][2] = c_far; s_cnt[wave][3] = c_cap; }
    __syncthreads();
    if (tid == 0)
        for (int k = 0; k < 4; ++k) stats[4 * b + k] = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
}

void ofk_launch_track_gate(hipStream_t s, const float *prev_pts, const float *back_pts, const uint8_t *st_back, const float *err,
                           const int *counts, int pts_stride, int fb_on, float thr2, int err_on, float err_max, uint8_t *status, float *fb2,
                           int *stats, int batch)
{
    hipLaunchKernelGGL(k_track_gate, dim3(batch), dim3(256), 0, s, prev_pts, back_pts, st_back, err, counts, pts_stride, fb_on, thr2, err_on,
                       err_max, status, fb2, stats);
}

#include "k_zones.inc"
#include "k_camera.inc"
#include "k_rshutter.inc"
#include "k_finite.inc"
#include "k_track_table.inc"
#include "k_lstsq.inc"
#include "k_track_depth.inc"
#include "k_track_template.inc"
#include "k_keyframe.inc"
#include "k_keyframe_rot.inc"
#include "k_keyframe_map.inc"
#include "k_pos_filter.inc"
#include "k_stabilise.inc"
