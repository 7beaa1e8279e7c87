    constexpr int NPL = (WMAX * WMAX + 63) / 64;               // window pixels per lane
    constexpr int IW = WMAX + 3;                               // staged prev neighbourhood
    constexpr int DW = WMAX + 1;                               // derivative core
    constexpr int JW = WMAX + 1 + 2 * LK_M;                    // staged next region
    __shared__ uint8_t s_I[IW * IW];
    __shared__ unsigned s_D[DW * DW];
    __shared__ uint8_t s_J[JW * JW];

    const int b = blockIdx.y, p = blockIdx.x, lane = threadIdx.x;
    if (p >= counts[b]) return;
    const size_t pi = (size_t)b * pts_stride + p;
    const float ptx = prev_pts[2 * pi], pty = prev_pts[2 * pi + 1];
    const uint8_t *Pb = prev + (size_t)b * pyr_stride, *Nb = next + (size_t)b * pyr_stride;
    const float half = (float)(win - 1) * 0.5f;
    const float eps2_lo = (float)(eps2 * (1.0 - 1e-5)), eps2_hi = (float)(eps2 * (1.0 + 1e-5));
    const int ww = win * win;
    const int iw_ = win + 3, dw_ = win + 1, jw_ = win + 1 + 2 * LK_M;

    int st = 1;
    float errv = 0.f, nx = 0.f, ny = 0.f;
    if (FLAGS & LK_SEED) { nx = next_pts[2 * pi]; ny = next_pts[2 * pi + 1]; }      // the start position travels in the carry
    short pI[NPL], pIx[NPL], pIy[NPL];

    for (int l = lv.n; l >= 0; --l) {
        const int lh = lv.h[l], lw = lv.w[l];
        const uint8_t *I = Pb + lv.off[l], *J = Nb + lv.off[l];
        const float sc = __int_as_float((127 - l) << 23);           // 2^-l, exactly what (float)(1.0 / (double)(1 << l)) is
        float px = ptx * sc, py = pty * sc, qx, qy;
        if (l == lv.n) { qx = px; qy = py; } else { qx = nx * 2.f; qy = ny * 2.f; }
        if ((FLAGS & LK_SEED) && l == lv.n) { qx = nx * sc; qy = ny * sc; }
        nx = qx; ny = qy;
        px -= half; py -= half;
        const int ipx = __builtin_amdgcn_readfirstlane((int)floorf(px)), ipy = __builtin_amdgcn_readfirstlane((int)floorf(py));
        if (ipx < -win || ipx >= lw || ipy < -win || ipy >= lh) {
            if (l == 0) { st = 0; errv = 0.f; }
            continue;
        }
        // stage prev neighbourhood (origin ipx-1, ipy-1) and its Scharr derivatives
        __syncthreads();
        for (int i = lane; i < iw_ * iw_; i += 64) {
            const int r = i / iw_, c = i - r * iw_;
            s_I[i] = I[(size_t)reflect101(ipy - 1 + r, lh) * lw + reflect101(ipx - 1 + c, lw)];
        }
        __syncthreads();
        for (int i = lane; i < dw_ * dw_; i += 64) {
            const int r = i / dw_, c = i - r * dw_;
            const int X = ipx + c, Y = ipy + r;
            unsigned pk = 0;
            if (X >= 0 && X < lw && Y >= 0 && Y < lh) {       // derivative image has a constant-0 border
                const uint8_t *r0 = s_I + r * iw_ + c, *r1 = r0 + iw_, *r2 = r1 + iw_;
                const int dx = 3 * (r0[2] - r0[0]) + 10 * (r1[2] - r1[0]) + 3 * (r2[2] - r2[0]);
                const int dy = 3 * (r2[0] - r0[0]) + 10 * (r2[1] - r0[1]) + 3 * (r2[2] - r0[2]);
                pk = ((unsigned)dx & 0xffffu) | ((unsigned)dy << 16);
            }
            s_D[i] = pk;
        }
        __syncthreads();
        int w00, w01, w10, w11;
        lk_weights(px - (float)ipx, py - (float)ipy, w00, w01, w10, w11);
        int a11 = 0, a12 = 0, a22 = 0;
        long long A11s = 0, A12s = 0, A22s = 0;
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int k = lane + 64 * j;
            pI[j] = 0; pIx[j] = 0; pIy[j] = 0;
            if (k < ww) {
                const int y = k / win, x = k - y * win;
                const uint8_t *i0 = s_I + (y + 1) * iw_ + x + 1, *i1 = i0 + iw_;
                const int iv = descale(i0[0] * w00 + i0[1] * w01 + i1[0] * w10 + i1[1] * w11, 9);
                const unsigned d00 = s_D[y * dw_ + x], d01 = s_D[y * dw_ + x + 1], d10 = s_D[(y + 1) * dw_ + x],
                               d11 = s_D[(y + 1) * dw_ + x + 1];
                const int ix = descale((int)(short)(d00 & 0xffffu) * w00 + (int)(short)(d01 & 0xffffu) * w01 +
                                           (int)(short)(d10 & 0xffffu) * w10 + (int)(short)(d11 & 0xffffu) * w11, 14);
                const int iy = descale(((int)d00 >> 16) * w00 + ((int)d01 >> 16) * w01 + ((int)d10 >> 16) * w10 +
                                           ((int)d11 >> 16) * w11, 14);
                pI[j] = (short)iv; pIx[j] = (short)ix; pIy[j] = (short)iy;
                if (NPL <= 8) { a11 += ix * ix; a12 += ix * iy; a22 += iy * iy; }
                else { A11s += (long long)ix * ix; A12s += (long long)ix * iy; A22s += (long long)iy * iy; }
            }
        }
        if (NPL <= 8) { A11s = a11; A12s = a12; A22s = a22; }
        A11s = wave_sum_i64(A11s); A12s = wave_sum_i64(A12s); A22s = wave_sum_i64(A22s);
        const float A11 = (float)((double)A11s * 0x1p-20), A12 = (float)((double)A12s * 0x1p-20),
                    A22 = (float)((double)A22s * 0x1p-20);
        float D = A11 * A22 - A12 * A12;
        const float dd = A11 - A22;
        const float minEig = (A22 + A11 - sqrtf(dd * dd + 4.f * A12 * A12)) / (float)(2 * ww);
        if ((FLAGS & LK_EIG) && l == 0) errv = minEig;
        if ((double)minEig < min_eig_thr || D < FLT_EPSILON) {
            if (l == 0) st = 0;
            continue;
        }
        D = 1.f / D;
        qx -= half; qy -= half;
        float pdx = 0.f, pdy = 0.f;
        int jx0 = 0, jy0 = 0;
        bool jvalid = false;
        int jwx = 0, jwy = 0;                                  // window origin inside the staged region
        auto stage_J = [&](int iqx, int iqy) {
            jx0 = iqx - LK_M; jy0 = iqy - LK_M;
            __syncthreads();
            for (int i = lane; i < jw_ * jw_; i += 64) {
                const int r = i / jw_, c = i - r * jw_;
                s_J[i] = J[(size_t)reflect101(jy0 + r, lh) * lw + reflect101(jx0 + c, lw)];
            }
            __syncthreads();
            jvalid = true;
        };
        for (int j = 0; j < max_count; ++j) {
            // every lane holds the same position: move the integer part to the scalar unit (bounds tests, LDS offsets)
            const int iqx = __builtin_amdgcn_readfirstlane((int)floorf(qx)), iqy = __builtin_amdgcn_readfirstlane((int)floorf(qy));
            if (iqx < -win || iqx >= lw || iqy < -win || iqy >= lh) {
                if (l == 0) st = 0;
                break;
            }
            if (!jvalid || iqx < jx0 || iqx > jx0 + 2 * LK_M || iqy < jy0 || iqy > jy0 + 2 * LK_M) stage_J(iqx, iqy);
            jwx = iqx - jx0; jwy = iqy - jy0;
            lk_weights(qx - (float)iqx, qy - (float)iqy, w00, w01, w10, w11);
            int b1 = 0, b2 = 0;
            long long B1 = 0, B2 = 0;
#pragma unroll
            for (int jj = 0; jj < NPL; ++jj) {
                const int k = lane + 64 * jj;
                if (k < ww) {
                    const int y = k / win, x = k - y * win;
                    const uint8_t *j0 = s_J + (jwy + y) * jw_ + jwx + x, *j1 = j0 + jw_;
                    const int diff = descale(j0[0] * w00 + j0[1] * w01 + j1[0] * w10 + j1[1] * w11, 9) - pI[jj];
                    if (NPL <= 8) { b1 += diff * pIx[jj]; b2 += diff * pIy[jj]; }
                    else { B1 += (long long)diff * pIx[jj]; B2 += (long long)diff * pIy[jj]; }
                }
            }
            if (NPL <= 8) { B1 = b1; B2 = b2; }
            B1 = wave_sum_i64(B1); B2 = wave_sum_i64(B2);
            const float fb1 = (float)((double)B1 * 0x1p-20), fb2 = (float)((double)B2 * 0x1p-20);
            const float dx = (A12 * fb2 - A22 * fb1) * D, dy = (A12 * fb1 - A11 * fb2) * D;
            qx += dx; qy += dy;
            nx = qx + half; ny = qy + half;
            // |delta|^2 <= eps^2 is defined in f64; the f32 value decides it unless it falls within 1e-5 of the threshold
            // (its own error is 2e-7), so the half-rate f64 instructions only run in that band
            const float d2 = dx * dx + dy * dy;
            if (d2 < eps2_lo) break;
            if (d2 <= eps2_hi && (double)dx * (double)dx + (double)dy * (double)dy <= eps2) break;
            // an f32 x satisfies |x| < 0.01 (the f64 constant) iff |x| <= 0.01f: 0.01f is the largest f32 below 0.01
            if (j > 0 && fabsf(dx + pdx) <= 0.01f && fabsf(dy + pdy) <= 0.01f) {
                nx -= dx * 0.5f; ny -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
        if (st && l == 0) {
            const float ex = nx - half, ey = ny - half;
            const int iex = __builtin_amdgcn_readfirstlane((int)floorf(ex)), iey = __builtin_amdgcn_readfirstlane((int)floorf(ey));
            if (iex < -win || iex >= lw || iey < -win || iey >= lh) { st = 0; continue; }
            if (FLAGS & LK_EIG) continue;
            if (!jvalid || iex < jx0 || iex > jx0 + 2 * LK_M || iey < jy0 || iey > jy0 + 2 * LK_M) stage_J(iex, iey);
            jwx = iex - jx0; jwy = iey - jy0;
            lk_weights(ex - (float)iex, ey - (float)iey, w00, w01, w10, w11);
            int se = 0;
#pragma unroll
            for (int jj = 0; jj < NPL; ++jj) {
                const int k = lane + 64 * jj;
                if (k < ww) {
                    const int y = k / win, x = k - y * win;
                    const uint8_t *j0 = s_J + (jwy + y) * jw_ + jwx + x, *j1 = j0 + jw_;
                    const int diff = descale(j0[0] * w00 + j0[1] * w01 + j1[0] * w10 + j1[1] * w11, 9) - pI[jj];
                    se += diff < 0 ? -diff : diff;
                }
            }
            se = wave_sum_i32(se);
            errv = (float)se / (float)(32 * ww);
        }
    }
    if (lane == 0) {
        next_pts[2 * pi] = nx; next_pts[2 * pi + 1] = ny;
        status[pi] = (uint8_t)st;
        err[pi] = (FLAGS & LK_EIG) ? errv : st ? errv : 0.f;
    }
