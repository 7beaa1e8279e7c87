    // Body of k_lk_light<WMAX, FLAGS>: k_lk_generic.inc's one-wave-per-point tracker with the per-window gain and bias of
    // ofk.h (ofk_lk_light).  Pyramid walk, staging, bounds tests, weights, Ip / Ixp / Iyp, the normal matrix, minEig, the status
    // rules, the 2x2 solve and both stopping rules are that file's; what differs is how the mismatch vector is formed (rules 1-5)
    // and the residual err (rule 6).  Every sum is an exact 64-bit integer reduced with shuffles, so it is order-free; the f64
    // part (one divide, one square root, the clamp, the mismatch expression) runs on wave-uniform values once per Newton step.
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
    const long long N = ww;
    const int iw_ = win + 3, dw_ = win + 1, jw_ = win + 1 + 2 * LK_M;

    int st = 1;
    float errv = 0.f, nx = 0.f, ny = 0.f;
    if (FLAGS & LK_SEED) { nx = next_pts[2 * pi]; ny = next_pts[2 * pi + 1]; }      // the start position travels in the carry
    short pI[NPL], pIx[NPL], pIy[NPL], pJ[NPL];

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
        long long A11s = 0, A12s = 0, A22s = 0;
        long long SI = 0, SII = 0, SIx = 0, SIy = 0, SIIx = 0, SIIy = 0;      // rule 1: the template sums of the level
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int k = lane + 64 * j;
            pI[j] = 0; pIx[j] = 0; pIy[j] = 0; pJ[j] = 0;
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
                A11s += (long long)ix * ix; A12s += (long long)ix * iy; A22s += (long long)iy * iy;
                SI += iv; SII += (long long)iv * iv; SIx += ix; SIy += iy;
                SIIx += (long long)iv * ix; SIIy += (long long)iv * iy;
            }
        }
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
        SI = wave_sum_i64(SI); SII = wave_sum_i64(SII); SIx = wave_sum_i64(SIx); SIy = wave_sum_i64(SIy);
        SIIx = wave_sum_i64(SIIx); SIIy = wave_sum_i64(SIIy);
        const long long vI = N * SII - SI * SI;                                // rule 3
        const long long cIx = N * SIIx - SI * SIx, cIy = N * SIIy - SI * SIy;  // rule 5, the template's half
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
        // rule 2 at the window origin (jwx, jwy) of the staged region: the lane's samples go to pJ, the four sums come back reduced
        auto sums_J = [&](long long &SJ, long long &SJJ, long long &SJx, long long &SJy) {
            if constexpr (NPL <= 4) {
                // windows <= 15: a 16-lane DPP row holds at most 64 samples, and 64 * 8160 * 4080 < 2^31, 64 * 8160^2 < 2^32, so the
                // row sums are exact in 32 bits (J^2 as unsigned) and k_lk15's DPP tree + 4 v_readlane + scalar 64-bit adds replace
                // 48 ds_bpermute per step; both factors of every product fit 24 bits (full-rate v_mad_i32_i24)
                int sj = 0, sjx = 0, sjy = 0;
                unsigned sjj = 0;
#pragma unroll
                for (int jj = 0; jj < NPL; ++jj) {
                    const int k = lane + 64 * jj;
                    if (k < ww) {
                        const int y = k / win, x = k - y * win;
                        const uint8_t *j0 = s_J + (jwy + y) * jw_ + jwx + x, *j1 = j0 + jw_;
                        const int jv = descale(j0[0] * w00 + j0[1] * w01 + j1[0] * w10 + j1[1] * w11, 9);
                        pJ[jj] = (short)jv;
                        sj += jv; sjj += (unsigned)__mul24(jv, jv); sjx += __mul24(jv, (int)pIx[jj]); sjy += __mul24(jv, (int)pIy[jj]);
                    }
                }
                SJ = wave_sum_rows(sj); SJx = wave_sum_rows(sjx); SJy = wave_sum_rows(sjy);
                const int t = row_sum16((int)sjj);
                SJJ = ((long long)(unsigned)__builtin_amdgcn_readlane(t, 0) + (long long)(unsigned)__builtin_amdgcn_readlane(t, 16)) +
                      ((long long)(unsigned)__builtin_amdgcn_readlane(t, 32) + (long long)(unsigned)__builtin_amdgcn_readlane(t, 48));
                return;
            }
            SJ = 0; SJJ = 0; SJx = 0; SJy = 0;
#pragma unroll
            for (int jj = 0; jj < NPL; ++jj) {
                const int k = lane + 64 * jj;
                if (k < ww) {
                    const int y = k / win, x = k - y * win;
                    const uint8_t *j0 = s_J + (jwy + y) * jw_ + jwx + x, *j1 = j0 + jw_;
                    const int jv = descale(j0[0] * w00 + j0[1] * w01 + j1[0] * w10 + j1[1] * w11, 9);
                    pJ[jj] = (short)jv;
                    SJ += jv; SJJ += (long long)jv * jv; SJx += (long long)jv * pIx[jj]; SJy += (long long)jv * pIy[jj];
                }
            }
            SJ = wave_sum_i64(SJ); SJJ = wave_sum_i64(SJJ); SJx = wave_sum_i64(SJx); SJy = wave_sum_i64(SJy);
        };
        // rules 3-4: wave-uniform f64
        auto gain_of = [&](long long SJ, long long SJJ) {
            if (light_mode != OFK_LIGHT_GAIN) return 1.0;
            const long long vJ = N * SJJ - SJ * SJ;
            if (vI <= 0 || vJ <= 0) return 1.0;
            double a = sqrt((double)vI / (double)vJ);
            if (a < gain_lo) a = gain_lo;
            if (a > gain_hi) a = gain_hi;
            return a;
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
            long long SJ, SJJ, SJx, SJy;
            sums_J(SJ, SJJ, SJx, SJy);
            const double a = gain_of(SJ, SJJ);
            const long long cJx = N * SJx - SJ * SIx, cJy = N * SJy - SJ * SIy;
            const float fb1 = (float)(((a * (double)cJx - (double)cIx) / (double)N) * 0x1p-20),
                        fb2 = (float)(((a * (double)cJy - (double)cIy) / (double)N) * 0x1p-20);
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
            // rule 6: the residual of the compensated window, all integer
            long long SJ, SJJ, SJx, SJy;
            sums_J(SJ, SJJ, SJx, SJy);
            const long long a12 = llrint(gain_of(SJ, SJJ) * 4096.0);
            long long se = 0;
#pragma unroll
            for (int jj = 0; jj < NPL; ++jj) {
                const int k = lane + 64 * jj;
                if (k < ww) {
                    const long long r = a12 * (N * pJ[jj] - SJ) - 4096 * (N * pI[jj] - SI);
                    se += r < 0 ? -r : r;
                }
            }
            se = wave_sum_i64(se);
            errv = (float)((double)se / (4096.0 * (double)N * 32.0 * (double)N));
        }
    }
    if (lane == 0) {
        next_pts[2 * pi] = nx; next_pts[2 * pi + 1] = ny;
        status[pi] = (uint8_t)st;
        err[pi] = (FLAGS & LK_EIG) ? errv : st ? errv : 0.f;
    }
