// k_warp.inc — k_warp_u8: perspective warp of 1- or 3-channel u8 images, cv2's 5-bit INTER_LINEAR arithmetic (ofk.h:
// ofk_warp_perspective states the rule; this file follows its order of operations).  Included by k_image.hip.
//
// Destination-driven, one launch for a batch: block = 4 waves, wave = one destination row, lane = 4 adjacent pixels of that row
// (a block covers 256 x 4 destination pixels; for a homography near a rigid motion its source footprint is a few rows of a few
// hundred bytes).  M [B][9] f64 maps a destination pixel to a source pixel; blockIdx.z picks the image, so the nine entries come
// in through scalar loads and stay in SGPRs.  The coordinates are f64 with no contraction (the Makefile's -ffp-contract=off); the
// row's products M1 y, M4 y, M7 y are formed once.  Taps are byte gathers at CLAMPED coordinates (no load ever leaves the source
// image), the constant border is patched in afterwards.  Stores: the lane's 4 pixels as one dword (three for 3 channels) where the
// row starts on a 4-byte boundary and the 4 pixels lie inside the row, bytes otherwise.  Covered pixels: one ballot + popcount per
// pixel slot and wave, summed over the block's waves in LDS, one integer atomicAdd per block.
// Everything behind the coordinates (wp_sample, wp_store, wp_count) is shared with k_warp_lens_u8 (k_warp_lens.inc).
#define WP_ROWS 4                       // rows (= waves) per block
#define WP_PX 4                         // pixels per lane

// One destination pixel from its fixed-point source coordinates (fx, fy in 1/32 pixels; ok false: border value, not covered): rint to
// even, 5 fractional bits, four byte taps at clamped coordinates, the integer sum.  bit: what cov takes where the pixel is covered (0: a
// pixel beyond the row's end).
template <int CH>
__device__ __forceinline__ void wp_sample(const uint8_t *img, int sh, int sw, double fx, double fy, bool ok, int border, int bval,
                                          unsigned (&out)[CH], unsigned &cov, unsigned bit)
{
    if (!ok) fx = fy = 0.0;
    const int ix = (int)rint(fx), iy = (int)rint(fy);                                           // ties to even; |.| <= 2^30
    const int sx = ix >> 5, sy = iy >> 5, ax = ix & 31, ay = iy & 31;
    const bool in_x0 = sx >= 0 && sx < sw, in_x1 = sx + 1 >= 0 && sx + 1 < sw;
    const bool in_y0 = sy >= 0 && sy < sh, in_y1 = sy + 1 >= 0 && sy + 1 < sh;
    if (ok && in_x0 && in_x1 && in_y0 && in_y1) cov |= bit;
    const int cx0 = min(max(sx, 0), sw - 1), cx1 = min(max(sx + 1, 0), sw - 1);
    const int cy0 = min(max(sy, 0), sh - 1), cy1 = min(max(sy + 1, 0), sh - 1);
    const uint8_t *r0 = img + (size_t)cy0 * sw * CH, *r1 = img + (size_t)cy1 * sw * CH;
    const bool constant = border == OFK_BORDER_CONSTANT;
    const bool k00 = !constant || (in_x0 && in_y0), k01 = !constant || (in_x1 && in_y0);
    const bool k10 = !constant || (in_x0 && in_y1), k11 = !constant || (in_x1 && in_y1);
    const unsigned w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const unsigned p00 = k00 ? r0[cx0 * CH + c] : bval, p01 = k01 ? r0[cx1 * CH + c] : bval;
        const unsigned p10 = k10 ? r1[cx0 * CH + c] : bval, p11 = k11 ? r1[cx1 * CH + c] : bval;
        const unsigned v = (w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512u) >> 10;
        out[c] = ok ? v : (unsigned)bval;
    }
}

// the lane's 4 pixels: one dword per channel where the row starts on a 4-byte boundary and the pixels lie inside it, bytes otherwise
template <int CH>
__device__ __forceinline__ void wp_store(uint8_t *row, bool row_aligned, int x0, int dw, const unsigned (&out)[WP_PX][CH])
{
    if (row_aligned && x0 + WP_PX <= dw) {
        unsigned bytes[WP_PX * CH];
#pragma unroll
        for (int j = 0; j < WP_PX; ++j)
#pragma unroll
            for (int c = 0; c < CH; ++c) bytes[j * CH + c] = out[j][c];
        unsigned *p = reinterpret_cast<unsigned *>(row + (size_t)x0 * CH);
#pragma unroll
        for (int q = 0; q < CH; ++q)
            p[q] = bytes[4 * q] | (bytes[4 * q + 1] << 8) | (bytes[4 * q + 2] << 16) | (bytes[4 * q + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < WP_PX; ++j)
            if (x0 + j < dw)
#pragma unroll
                for (int c = 0; c < CH; ++c) row[(size_t)(x0 + j) * CH + c] = (uint8_t)out[j][c];
    }
}

// cov bit j: the lane's pixel j is covered.  Every thread of the block calls it (there is a barrier inside); one atomicAdd per block.
__device__ __forceinline__ void wp_count(int *covered, unsigned cov, int (&s_cnt)[WP_ROWS])
{
    int n = 0;
#pragma unroll
    for (int j = 0; j < WP_PX; ++j) n += __popcll(__ballot((cov >> j) & 1u));
    if (threadIdx.x == 0) s_cnt[threadIdx.y] = n;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < WP_ROWS; ++k) t += s_cnt[k];
        if (t) atomicAdd(covered, t);
    }
}

template <int CH>
__global__ __launch_bounds__(64 * WP_ROWS) void k_warp_u8(const uint8_t *__restrict__ src, size_t src_stride, int sh, int sw,
                                                          const double *__restrict__ M, uint8_t *__restrict__ dst, size_t dst_stride,
                                                          int dh, int dw, int border, int bval, int *__restrict__ covered, int b0)
{
    __shared__ int s_cnt[WP_ROWS];
    const int b = b0 + blockIdx.z;
    const double *m = M + 9 * (size_t)b;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6], m7 = m[7], m8 = m[8];
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
            const double iw = (W != 0.0) ? 32.0 / W : 0.0;
            const double fx = X * iw, fy = Y * iw;
            const bool ok = fabs(fx) <= 1073741824.0 && fabs(fy) <= 1073741824.0;              // false for NaN
            wp_sample<CH>(img, sh, sw, fx, fy, ok, border, bval, out[j], cov, x0 + j < dw ? 1u << j : 0u);
        }
        const size_t row = (size_t)y * dw * CH;                                                 // images start 4-byte aligned
        wp_store<CH>(dst + (size_t)b * dst_stride + row, (row & 3) == 0, x0, dw, out);
    }
    if (covered) wp_count(covered + b, cov, s_cnt);            // kernel-uniform
}

// src [batch] images `src_stride` bytes apart, sh x sw x ch u8, rows tight; dst likewise, dh x dw x ch, every image 4-byte aligned;
// M [batch][9] f64 and covered [batch] i32 (NULL: not counted; zeroed here) in device memory; ch 1 or 3
void ofk_launch_warp(hipStream_t s, const uint8_t *src, size_t src_stride, int sh, int sw, int ch, const double *M, uint8_t *dst,
                     size_t dst_stride, int dh, int dw, int border, int bval, int *covered, int batch)
{
    if (covered) hipMemsetAsync(covered, 0, (size_t)batch * sizeof(int), s);
    const dim3 block(64, WP_ROWS);
    for (int b0 = 0; b0 < batch; b0 += 65535) {                 // gridDim.z
        const dim3 grid((dw + 64 * WP_PX - 1) / (64 * WP_PX), (dh + WP_ROWS - 1) / WP_ROWS, min(batch - b0, 65535));
        if (ch == 3) hipLaunchKernelGGL((k_warp_u8<3>), grid, block, 0, s, src, src_stride, sh, sw, M, dst, dst_stride, dh, dw, border, bval, covered, b0);
        else hipLaunchKernelGGL((k_warp_u8<1>), grid, block, 0, s, src, src_stride, sh, sw, M, dst, dst_stride, dh, dw, border, bval, covered, b0);
    }
}
