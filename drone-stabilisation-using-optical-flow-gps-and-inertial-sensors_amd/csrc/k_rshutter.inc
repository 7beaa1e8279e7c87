// k_rshutter.inc — the rolling shutter of ofk.h (ofk_set_rolling_shutter): per point the row times of its two observations and the
// positions a global shutter would have seen at the two time stamps.  Included by k_tracks.hip.
// One thread per point, grid (ceil(pts_stride / 256), batch); ONE launch writes both output arrays, since a point's correction needs
// both of its ends.  float64 in the order ofk.h states (the build has no FMA contraction), one rounding to f32 at the end; rho, H,
// alpha and the gain are kernel arguments.  Nothing is written beyond counts[b]; no atomics, no LDS, no scratch.  The kernel is
// latency-bound and tiny (a few hundred points per image): it is not tuned beyond the launch count.
// raw: the image's pixels (the rows the readout runs over); id: the ideal pixels of the same points (the raw ones with no camera);
// id and out may be the same buffers (the resident chains correct the camera's output in place): each thread reads its point
// before it writes it.

struct rs_xy { double x, y; };
struct rs_xyz { double X, Y, Z; };

// the exact rotation of P = (x, y, 1) by phi = -t * omega (Rodrigues), before the projection; k_finite.inc reads Z
__device__ __forceinline__ rs_xyz rs_rotate3(double x, double y, double t, double o0, double o1, double o2)
{
    const double p0 = -t * o0, p1 = -t * o1, p2 = -t * o2;
    const double th2 = p0 * p0 + p1 * p1 + p2 * p2;
    double A = 1.0, B = 0.5;
    if (!(th2 < 1e-16)) {
        const double th = sqrt(th2);
        A = sin(th) / th;
        B = (1.0 - cos(th)) / th2;
    }
    const double c0 = p1 - p2 * y, c1 = p2 * x - p0, c2 = p0 * y - p1 * x;                       // phi x P
    const double d0 = p1 * c2 - p2 * c1, d1 = p2 * c0 - p0 * c2, d2 = p0 * c1 - p1 * c0;          // phi x (phi x P)
    const double X = x + A * c0 + B * d0, Y = y + A * c1 + B * d1, Z = 1.0 + A * c2 + B * d2;
    return {X, Y, Z};
}

// projected back: where the rotation had the point t frame intervals earlier
__device__ __forceinline__ rs_xy rs_rotate(double x, double y, double t, double o0, double o1, double o2)
{
    const rs_xyz r = rs_rotate3(x, y, t, o0, o1, o2);
    return {r.X / r.Z, r.Y / r.Z};
}

template <int MODE>
__global__ __launch_bounds__(256) void k_rs_correct(const float *raw0, const float *raw1, const float *id0, const float *id1, float *out0,
                                                    float *out1, const int *__restrict__ counts, int pts_stride,
                                                    const double *__restrict__ sensors, const double *__restrict__ imu, double rho,
                                                    double rows, double alpha, double gain)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pts_stride || p >= counts[b]) return;
    const size_t pi = (size_t)b * pts_stride + p;
    const float2 r0 = ((const float2 *)raw0)[pi], r1 = ((const float2 *)raw1)[pi];
    const float2 f0 = ((const float2 *)id0)[pi], f1 = ((const float2 *)id1)[pi];
    const double t0 = rho * ((double)r0.y / rows - alpha), t1 = rho * ((double)r1.y / rows - alpha);
    const double span = 1.0 + (t1 - t0);
    const double q0x = (double)f0.x, q0y = (double)f0.y, q1x = (double)f1.x, q1y = (double)f1.y;
    float2 o0 = f0, o1 = f1;                                     // the fallback: the ideal points as they came
    if (span >= 0.5 && span <= 1.7976931348623157e308) {         // false for NaN
        double ax, ay, bx, by;
        bool ok = true;
        if (MODE == OFK_RS_FLOW) {
            const double fx = (q1x - q0x) / span, fy = (q1y - q0y) / span;
            ax = q0x - t0 * fx; ay = q0y - t0 * fy;
            bx = q1x - t1 * fx; by = q1y - t1 * fy;
        } else {
            const double *sn = sensors + (size_t)b * OFK_SENSOR_DOUBLES;
            const double *ist = imu ? imu + (size_t)b * OFK_IMU_STATE : nullptr;
            const double sc = sn[19], cx = sn[20], cy = sn[21];
            const double om0 = gain * (ist ? ist[18] : sn[4]), om1 = gain * (ist ? ist[19] : sn[5]), om2 = gain * (ist ? ist[20] : sn[6]);
            ok = sc != 0.0;
            const double x0 = (q0x - cx) * sc, y0 = (q0y - cy) * sc, x1 = (q1x - cx) * sc, y1 = (q1y - cy) * sc;
            const double hs = span / 2.0;                        // the rotation alone carries both observations to the middle of the span:
            const rs_xy r = rs_rotate(x0, y0, -hs, om0, om1, om2), m = rs_rotate(x1, y1, hs, om0, om1, om2);      // what parts them there is the rest
            const double ftx = (m.x - r.x) / span, fty = (m.y - r.y) / span;
            const rs_xy a = rs_rotate(x0, y0, t0, om0, om1, om2), e = rs_rotate(x1, y1, t1, om0, om1, om2);
            ax = (a.x - t0 * ftx) / sc + cx; ay = (a.y - t0 * fty) / sc + cy;
            bx = (e.x - t1 * ftx) / sc + cx; by = (e.y - t1 * fty) / sc + cy;
        }
        const float tax = (float)ax, tay = (float)ay, tbx = (float)bx, tby = (float)by;
        if (ok && fabsf(tax) <= 1e6f && fabsf(tay) <= 1e6f && fabsf(tbx) <= 1e6f && fabsf(tby) <= 1e6f) {      // false for NaN and infinity too
            o0 = make_float2(tax, tay); o1 = make_float2(tbx, tby);
        }
    }
    ((float2 *)out0)[pi] = o0; ((float2 *)out1)[pi] = o1;
}

// id0 / id1 NULL: the raw points are the ideal ones.  rs->mode is FLOW or GYRO and rs->rows > 0 (the callers check); sensors may be
// NULL for FLOW; imu_state != NULL: omega from the resident IMU state, as k_seed_points takes it.
void ofk_launch_rs_correct(hipStream_t s, const ofk_rshutter *rs, const float *raw0, const float *raw1, const float *id0, const float *id1,
                           float *out0, float *out1, const int *counts, int pts_stride, const double *sensors, const double *imu_state, int batch)
{
    const dim3 grid((pts_stride + 255) / 256, batch), block(256);
    if (!id0) { id0 = raw0; id1 = raw1; }
    if (rs->mode == OFK_RS_GYRO)
        hipLaunchKernelGGL(k_rs_correct<OFK_RS_GYRO>, grid, block, 0, s, raw0, raw1, id0, id1, out0, out1, counts, pts_stride, sensors, imu_state,
                           rs->readout, (double)rs->rows, rs->anchor, rs->omega_gain);
    else
        hipLaunchKernelGGL(k_rs_correct<OFK_RS_FLOW>, grid, block, 0, s, raw0, raw1, id0, id1, out0, out1, counts, pts_stride, sensors, imu_state,
                           rs->readout, (double)rs->rows, rs->anchor, rs->omega_gain);
}
