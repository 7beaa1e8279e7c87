// k_camera_map.inc — the lens's forward map of ofk.h (ofk_set_camera: "Distort"), ideal normalised coordinates -> (pixel - c) / f of the
// image.  Included by k_camera.inc (k_tracks.hip: the point kernels) and k_warp_lens.inc (k_image.hip: the rectifying warp), so both read
// the same expressions.  float64 in the order ofk.h states; the build has no FMA contraction.
#pragma once

struct cam_xy { double x, y; };

// RATIONAL false (Brown only): the caller has seen k4 = k5 = k6 = 0, the denominator is exactly 1.0 and the divide is left out - the
// quotient's bits are the numerator's
template <int MODEL, bool RATIONAL = true> __device__ __forceinline__ cam_xy cam_distort(const ofk_camera &c, double x, double y)
{
    if (MODEL == OFK_CAMERA_BROWN) {
        const double k1 = c.k[0], k2 = c.k[1], p1 = c.k[2], p2 = c.k[3], k3 = c.k[4], k4 = c.k[5], k5 = c.k[6], k6 = c.k[7];
        const double r2 = x * x + y * y;
        const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
        const double cd = RATIONAL ? num / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) : num;
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        return {x * cd + dx, y * cd + dy};
    }
    const double k1 = c.k[0], k2 = c.k[1], k3 = c.k[2], k4 = c.k[3];
    const double r = sqrt(x * x + y * y);
    const double t = atan(r);
    const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    const double td = t * (1.0 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8);
    const double s = r < 1e-8 ? 1.0 : td / r;
    return {x * s, y * s};
}
