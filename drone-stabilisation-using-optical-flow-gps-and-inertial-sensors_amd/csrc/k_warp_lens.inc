// k_warp_lens.inc — k_warp_lens_u8: the perspective warp with the lens's forward map behind the homography (ofk.h: ofk_warp_lens states
// the rule; this file follows its order of operations).  Included by k_image.hip behind k_warp.inc, whose decomposition and tail it keeps:
// block = 4 waves = 4 destination rows, lane = 4 adjacent pixels, the row's products formed once, byte gathers at clamped coordinates,
// dword stores where aligned, one integer atomicAdd per block for the covered count (wp_sample, wp_store, wp_count ARE k_warp_u8's).
// M [B][9] f64 (NULL: the identity) maps a destination pixel to an IDEAL pixel of the source camera.  The normalised matrix Mn is formed
// once per wave: lane i < 9 forms entry i (one divide per lane, not six per thread) and v_readlane hands the nine entries to SGPRs.  The
// camera comes in as a kernel argument, so its fields are scalar too.  Per pixel, f64 without contraction: three entries of Mn (x, y, 1),
// 1 / W, the lens (cam_distort of k_camera_map.inc, the point kernels' expressions), the camera matrix and the scale by 32.  Brown costs
// one more divide per pixel, none where the rational terms are zero (RATIONAL false, chosen on the host); the fisheye a square root, an
// atan and a divide.

__device__ __forceinline__ double wl_lane(double v, int lane)     // lane: a constant; the value in SGPRs
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

template <int CH, int MODEL, bool RATIONAL>
__global__ __launch_bounds__(64 * WP_ROWS) void k_warp_lens_u8(const uint8_t *__restrict__ src, size_t src_stride, int sh, int sw,
                                                               const double *__restrict__ M, uint8_t *__restrict__ dst, size_t dst_stride,
                                                               int dh, int dw, int border, int bval, int *__restrict__ covered, int b0,
                                                               ofk_camera c, double r_max)
{
    __shared__ int s_cnt[WP_ROWS];
    const int b = b0 + blockIdx.z;
    double e = 0.0;                                             // lane i < 9: Mn[i]
    if (threadIdx.x < 9) {
        const int i = threadIdx.x, col = i % 3;
        const double mi = M ? M[9 * (size_t)b + i] : (i % 4 == 0 ? 1.0 : 0.0);
        const double mw = M ? M[9 * (size_t)b + 6 + col] : (col == 2 ? 1.0 : 0.0);
        e = i < 3 ? (mi - c.co_x * mw) / c.fo_x : i < 6 ? (mi - c.co_y * mw) / c.fo_y : mi;
    }
    const double m0 = wl_lane(e, 0), m1 = wl_lane(e, 1), m2 = wl_lane(e, 2), m3 = wl_lane(e, 3), m4 = wl_lane(e, 4), m5 = wl_lane(e, 5);
    const double m6 = wl_lane(e, 6), m7 = wl_lane(e, 7), m8 = wl_lane(e, 8);
    const double r_max2 = r_max * r_max;
    const uint8_t *img = src + (size_t)b * src_stride;
    const int y = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * WP_ROWS + threadIdx.y));     // blockDim.x = 64: one row per wave
    const int x0 = (int)(blockIdx.x * 64 + threadIdx.x) * WP_PX;
    const double yd = (double)y;
    const double ry0 = m1 * yd, ry1 = m4 * yd, ry2 = m7 * yd;
    unsigned out[WP_PX][CH];
    unsigned cov = 0;                                           // bit j: pixel x0 + j is covered
    if (y < dh && x0 < dw) {
#pragma unroll
        for (int j = 0; j < WP_PX; ++j) {
            const double xd = (double)(x0 + j);
            const double X = (m0 * xd + ry0) + m2, Y = (m3 * xd + ry1) + m5, W = (m6 * xd + ry2) + m8;
            const double iw = (W != 0.0) ? 1.0 / W : 0.0;
            const double xn = X * iw, yn = Y * iw;
            const cam_xy d = cam_distort<MODEL, RATIONAL>(c, xn, yn);
            const double fx = (d.x * c.fx + c.cx) * 32.0, fy = (d.y * c.fy + c.cy) * 32.0;
            bool ok = fabs(fx) <= 1073741824.0 && fabs(fy) <= 1073741824.0;                     // false for NaN
            if (r_max > 0.0) ok = ok && (xn * xn + yn * yn <= r_max2);                           // kernel-uniform; false for NaN
            wp_sample<CH>(img, sh, sw, fx, fy, ok, border, bval, out[j], cov, x0 + j < dw ? 1u << j : 0u);
        }
        const size_t row = (size_t)y * dw * CH;                                                 // images start 4-byte aligned
        wp_store<CH>(dst + (size_t)b * dst_stride + row, (row & 3) == 0, x0, dw, out);
    }
    if (covered) wp_count(covered + b, cov, s_cnt);            // kernel-uniform
}

template <int CH>
static void warp_lens_launch(hipStream_t s, dim3 grid, dim3 block, const ofk_camera &c, double r_max, const uint8_t *src, size_t src_stride, int sh,
                             int sw, const double *M, uint8_t *dst, size_t dst_stride, int dh, int dw, int border, int bval, int *covered, int b0)
{
    if (c.model == OFK_CAMERA_FISHEYE)
        hipLaunchKernelGGL((k_warp_lens_u8<CH, OFK_CAMERA_FISHEYE, true>), grid, block, 0, s, src, src_stride, sh, sw, M, dst, dst_stride, dh, dw, border, bval, covered, b0, c, r_max);
    else if (c.k[5] != 0.0 || c.k[6] != 0.0 || c.k[7] != 0.0)
        hipLaunchKernelGGL((k_warp_lens_u8<CH, OFK_CAMERA_BROWN, true>), grid, block, 0, s, src, src_stride, sh, sw, M, dst, dst_stride, dh, dw, border, bval, covered, b0, c, r_max);
    else
        hipLaunchKernelGGL((k_warp_lens_u8<CH, OFK_CAMERA_BROWN, false>), grid, block, 0, s, src, src_stride, sh, sw, M, dst, dst_stride, dh, dw, border, bval, covered, b0, c, r_max);
}

// ofk_launch_warp's buffers; M may be NULL (the identity: plain rectification); cam->model is BROWN or FISHEYE (the entry points check)
void ofk_launch_warp_lens(hipStream_t s, const ofk_camera *cam, double r_max, const uint8_t *src, size_t src_stride, int sh, int sw, int ch,
                          const double *M, uint8_t *dst, size_t dst_stride, int dh, int dw, int border, int bval, int *covered, int batch)
{
    if (covered) hipMemsetAsync(covered, 0, (size_t)batch * sizeof(int), s);
    const dim3 block(64, WP_ROWS);
    for (int b0 = 0; b0 < batch; b0 += 65535) {                 // gridDim.z
        const dim3 grid((dw + 64 * WP_PX - 1) / (64 * WP_PX), (dh + WP_ROWS - 1) / WP_ROWS, min(batch - b0, 65535));
        if (ch == 3) warp_lens_launch<3>(s, grid, block, *cam, r_max, src, src_stride, sh, sw, M, dst, dst_stride, dh, dw, border, bval, covered, b0);
        else warp_lens_launch<1>(s, grid, block, *cam, r_max, src, src_stride, sh, sw, M, dst, dst_stride, dh, dw, border, bval, covered, b0);
    }
}
