// k_finite.inc — the finite motion of ofk.h (ofk_set_finite_motion): per point the pair (position, flow) for which the solves' first-order
// system is the exact relation of a frame pair P1 = R P0 + T on the plane.  Included by k_tracks.hip behind k_rshutter.inc, whose
// rs_rotate3 is the rotation.
// One thread per point, grid (ceil(pts_stride / 256), batch); ONE launch writes both output arrays, since a point's rewrite needs
// both of its ends.  float64 in the order ofk.h states (the build has no FMA contraction), one rounding to f32 at the end.  Nothing
// is written beyond counts[b]; no atomics, no LDS, no scratch.  The kernel is latency-bound and tiny (a few hundred points per
// image): it is not tuned beyond the launch count.
// in and out may be the same buffers (the resident chains rewrite the camera's / the rolling shutter's output in place): each thread
// reads both ends of its point before it writes them.

__global__ __launch_bounds__(256) void k_finite_correct(const float *in0, const float *in1, float *out0, float *out1,
                                                        const int *__restrict__ counts, int pts_stride, const double *__restrict__ sensors,
                                                        const double *__restrict__ imu, double min_depth)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pts_stride || p >= counts[b]) return;
    const size_t pi = (size_t)b * pts_stride + p;
    const float2 f0 = ((const float2 *)in0)[pi], f1 = ((const float2 *)in1)[pi];
    const double *sn = sensors + (size_t)b * OFK_SENSOR_DOUBLES;
    const double *ist = imu ? imu + (size_t)b * OFK_IMU_STATE : nullptr;
    const double sc = sn[19], cx = sn[20], cy = sn[21];
    const double n0 = ist ? ist[15] : sn[1], n1 = ist ? ist[16] : sn[2], n2 = ist ? ist[17] : sn[3];
    const double om0 = ist ? ist[18] : sn[4], om1 = ist ? ist[19] : sn[5], om2 = ist ? ist[20] : sn[6];
    float2 o0 = f0, o1 = f1;                                     // the fallback: the points as they came
    const double x0 = ((double)f0.x - cx) * sc, y0 = ((double)f0.y - cy) * sc, x1 = ((double)f1.x - cx) * sc, y1 = ((double)f1.y - cy) * sc;
    const rs_xyz r = rs_rotate3(x0, y0, -1.0, om0, om1, om2);    // the previous point rotated by +omega
    const double den = n0 * x1 + n1 * y1 + n2;
    if (sc != 0.0 && r.Z >= min_depth && fabs(den) >= 1e-12) {   // each false for NaN
        const double a = r.X / r.Z, bb = r.Y / r.Z;
        const double s = (n0 * a + n1 * bb + n2) / den;
        const double c0 = om1 - om2 * bb, c1 = om2 * a - om0, c2 = om0 * bb - om1 * a;            // omega x (a, b, 1)
        const double ux = s * (x1 - a) + (c0 - c2 * a), uy = s * (y1 - bb) + (c1 - c2 * bb);
        const float tnx = (float)(a / sc + cx), tny = (float)(bb / sc + cy);
        const float tpx = (float)((a - ux) / sc + cx), tpy = (float)((bb - uy) / sc + cy);
        if (s > 0.0 && fabsf(tnx) <= 1e6f && fabsf(tny) <= 1e6f && fabsf(tpx) <= 1e6f && fabsf(tpy) <= 1e6f) {   // false for NaN and infinity too
            o0 = make_float2(tpx, tpy); o1 = make_float2(tnx, tny);
        }
    }
    ((float2 *)out0)[pi] = o0; ((float2 *)out1)[pi] = o1;
}

// in0 / in1: the points the solve would otherwise have read; out may be in.  imu_state != NULL: normal and omega from the resident IMU
// state, as k_stream_fuse takes them.
void ofk_launch_finite_correct(hipStream_t s, const ofk_finite_motion *fm, const float *in0, const float *in1, float *out0, float *out1,
                               const int *counts, int pts_stride, const double *sensors, const double *imu_state, int batch)
{
    const dim3 grid((pts_stride + 255) / 256, batch), block(256);
    hipLaunchKernelGGL(k_finite_correct, grid, block, 0, s, in0, in1, out0, out1, counts, pts_stride, sensors, imu_state, fm->min_depth);
}
