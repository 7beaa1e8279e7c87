    __shared__ __attribute__((aligned(16))) uint8_t s_I[20 * LKF_IP];
    __shared__ __attribute__((aligned(16))) uint8_t s_J[(LKF_JW + 1) * LKF_JP];

    // XCD-aware block -> (image, point) map.  Workgroups are dealt round-robin over the 8 XCDs (blocks n and n + 8 share one),
    // each with its own L2.  The windows of an image's points overlap heavily (at the coarse levels every point reads most
    // of the level), so all points of an image go to ONE XCD — image b to the XCD of blocks n = b (mod 8) — and its pyramid
    // lines are fetched from HBM once instead of once per XCD.  Speed only; any placement gives the same results.
    const int lane = threadIdx.x;
    int b = blockIdx.y, p = blockIdx.x;
    if ((gridDim.y & 7) == 0) {
        const unsigned n = blockIdx.y * gridDim.x + blockIdx.x, k = n >> 3;
        b = 8 * (int)(k / gridDim.x) + (int)(n & 7);
        p = (int)(k % gridDim.x);
    }
    if (p >= counts[b]) return;
    const size_t pi = (size_t)b * pts_stride + p;
    const float ptx = prev_pts[2 * pi], pty = prev_pts[2 * pi + 1];
    const uint8_t *Pb = prev + (size_t)b * pyr_stride, *Nb = next + (size_t)b * pyr_stride;
    const float half = (float)(win - 1) * 0.5f;
    const int ww = win * win;
    const int iw_ = win + 3, jw_ = win + 1 + 2 * LK_M;
    const int wy = lane >> 2, wx0 = (lane & 3) * 4;            // this lane's window row and first column
    const int npx = wy < win ? min(4, max(0, win - wx0)) : 0;  // pixels owned by the lane

    int st = 1;
    float errv = 0.f, nx = 0.f, ny = 0.f;
    if (FLAGS & LK_SEED) { nx = next_pts[2 * pi]; ny = next_pts[2 * pi + 1]; }      // the start position travels in the carry
    int pI[4], pIx[4], pIy[4];

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
        qx -= half; qy -= half;
        int jx0 = 0, jy0 = 0;
        bool jvalid = false;
        // ---- staging.  One wave per workgroup: the LDS operations of a wave execute in order, so staging and reading need no
        //      s_barrier and, unlike __syncthreads(), no wait for outstanding GLOBAL loads — LDS_FENCE only keeps the compiler
        //      from moving LDS accesses across it.  The loads of the previous-frame neighbourhood and of the next-frame region
        //      are issued back to back (one memory round trip per level instead of two), then both are written to LDS.
        unsigned jd0 = 0, jd1 = 0, jd2 = 0, jd3 = 0, jd4 = 0, jsh = 0;
        bool jinner = false;
        auto J_issue = [&](int iqx, int iqy) {
            jx0 = iqx - LK_M; jy0 = iqy - LK_M;
            // dword path whenever the COLUMNS lie inside the image; rows are mirrored per lane (at the coarse levels a third
            // of the regions cross the top or bottom border, and the byte-wise path costs ~400 VALU instructions)
            jinner = jx0 >= 4 && jx0 + jw_ + 8 <= lw && (lw & 3) == 0 && jw_ == LKF_JW;
            if (jinner) {
                const int r = lane >> 1, hf = lane & 1;                   // 32 rows x 2 halves of 16 bytes
                const size_t addr = (size_t)reflect101(jy0 + r, lh) * lw + jx0 + 16 * hf;
                jsh = (unsigned)addr & 3u;
                const unsigned *g = reinterpret_cast<const unsigned *>(J + (addr & ~(size_t)3));
                jd0 = g[0]; jd1 = g[1]; jd2 = g[2]; jd3 = g[3]; jd4 = g[4];
            }
        };
        auto J_commit = [&]() {
            LDS_FENCE();                                                  // earlier readers of s_J are done
            if (jinner) {
                const int r = lane >> 1, hf = lane & 1;
                uint2 *dstp = reinterpret_cast<uint2 *>(s_J + r * LKF_JP + 16 * hf);      // the pitch keeps 8-byte alignment only
                dstp[0] = make_uint2(__builtin_amdgcn_alignbyte(jd1, jd0, jsh), __builtin_amdgcn_alignbyte(jd2, jd1, jsh));
                dstp[1] = make_uint2(__builtin_amdgcn_alignbyte(jd3, jd2, jsh), __builtin_amdgcn_alignbyte(jd4, jd3, jsh));
            } else {
                for (int i = lane; i < jw_ * jw_; i += 64) {
                    const int r = i / jw_, c = i - r * jw_;
                    s_J[r * LKF_JP + c] = J[(size_t)reflect101(jy0 + r, lh) * lw + reflect101(jx0 + c, lw)];
                }
            }
            LDS_FENCE();
            jvalid = true;
        };
        auto stage_J = [&](int iqx, int iqy) { J_issue(iqx, iqy); J_commit(); };
        {
            // the prev neighbourhood (origin ipx-1, ipy-1), (win+3)^2: one row of <= 18 bytes per lane, 6 dwords in, 5 out
            const bool inner = ipx >= 5 && ipx - 1 + 28 <= lw && (lw & 3) == 0;         // columns inside; rows mirrored per lane
            unsigned d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0, d5 = 0, sh = 0;
            if (inner && lane < iw_) {
                const size_t addr = (size_t)reflect101(ipy - 1 + lane, lh) * lw + (ipx - 1);
                sh = (unsigned)addr & 3u;
                const unsigned *g = reinterpret_cast<const unsigned *>(I + (addr & ~(size_t)3));
                d0 = g[0]; d1 = g[1]; d2 = g[2]; d3 = g[3]; d4 = g[4]; d5 = g[5];
            }
            // every lane holds the same position: move the integer part to the scalar unit (bounds tests, LDS offsets)
            const int iqx = __builtin_amdgcn_readfirstlane((int)floorf(qx)), iqy = __builtin_amdgcn_readfirstlane((int)floorf(qy));
            const bool doJ = !(iqx < -win || iqx >= lw || iqy < -win || iqy >= lh);
            if (doJ) J_issue(iqx, iqy);
            LDS_FENCE();                                                  // the previous level's readers of s_I are done
            if (inner) {
                if (lane < iw_) {
                    unsigned *o = reinterpret_cast<unsigned *>(s_I + lane * LKF_IP);
                    o[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
                    o[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
                    o[2] = __builtin_amdgcn_alignbyte(d3, d2, sh);
                    o[3] = __builtin_amdgcn_alignbyte(d4, d3, sh);
                    o[4] = __builtin_amdgcn_alignbyte(d5, d4, sh);
                }
            } else {
                for (int i = lane; i < iw_ * iw_; i += 64) {
                    const int r = i / iw_, c = i - r * iw_;
                    s_I[r * LKF_IP + c] = I[(size_t)reflect101(ipy - 1 + r, lh) * lw + reflect101(ipx - 1 + c, lw)];
                }
            }
            if (doJ) J_commit();
            else LDS_FENCE();
        }
        // ---- patch: I (5 fractional bits), Ix, Iy of the lane's pixels; exact integer normal matrix
        int w00, w01, w10, w11;
        lk_weights(px - (float)ipx, py - (float)ipy, w00, w01, w10, w11);
        int a11 = 0, a12 = 0, a22 = 0;
        pI[0] = pI[1] = pI[2] = pI[3] = 0; pIx[0] = pIx[1] = pIx[2] = pIx[3] = 0; pIy[0] = pIy[1] = pIy[2] = pIy[3] = 0;
        if (npx > 0) {
            // rows wy..wy+3 of s_I, columns wx0..wx0+7 (the staged rows are dword aligned): P[r][k] = (n[r][k], n[r][k+1])
            unsigned P[4][7];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned *pr = reinterpret_cast<const unsigned *>(s_I + (wy + r) * LKF_IP + wx0);
                const unsigned d0 = pr[0], d1 = pr[1];
#pragma unroll
                for (int k = 0; k < 7; ++k) P[r][k] = __builtin_amdgcn_perm(d1, d0, LK_PAIR_SEL(k));
            }
            // Scharr at the window taps (rows wy, wy+1; columns wx0..wx0+4), separable and two columns per instruction:
            // slot s = columns (2s, 2s+1).  hd = n[c+2] - n[c], hs = 3 (n[c] + n[c+2]) + 10 n[c+1] per neighbourhood row,
            // dx = 3 (hd_r + hd_{r+2}) + 10 hd_{r+1}, dy = hs_{r+2} - hs_r.  (The upper half of slot 2 is column 5: unused.)
            unsigned DX[2][3], DY[2][3];
#pragma unroll
            for (int sl = 0; sl < 3; ++sl) {
                lk_s2 hd[4], hs[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const lk_s2 a = lk_as_s2(P[r][2 * sl]), m = lk_as_s2(P[r][2 * sl + 1]), c2 = lk_as_s2(P[r][2 * sl + 2]);
                    hd[r] = c2 - a;
                    hs[r] = (a + c2) * (short)3 + m * (short)10;
                }
                DX[0][sl] = lk_as_u((hd[0] + hd[2]) * (short)3 + hd[1] * (short)10); DX[1][sl] = lk_as_u((hd[1] + hd[3]) * (short)3 + hd[2] * (short)10);
                DY[0][sl] = lk_as_u(hs[2] - hs[0]); DY[1][sl] = lk_as_u(hs[3] - hs[1]);
            }
            if (!(ipx >= 0 && ipx + win < lw && ipy >= 0 && ipy + win < lh)) {      // wave-uniform: the window touches the border
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int sl = 0; sl < 3; ++sl) {
                        const int X = ipx + wx0 + 2 * sl, Y = ipy + wy + r;
                        const bool rowok = Y >= 0 && Y < lh;
                        const unsigned keep = ((rowok && X >= 0 && X < lw) ? 0x0000ffffu : 0u) | ((rowok && X + 1 >= 0 && X + 1 < lw) ? 0xffff0000u : 0u);
                        DX[r][sl] &= keep; DY[r][sl] &= keep;                   // constant-0 derivative border
                    }
            }
            // pairs starting at column k = 0..3: (k, k+1)
            unsigned QX[2][4], QY[2][4];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                QX[r][0] = DX[r][0]; QX[r][1] = __builtin_amdgcn_alignbit(DX[r][1], DX[r][0], 16); QX[r][2] = DX[r][1];
                QX[r][3] = __builtin_amdgcn_alignbit(DX[r][2], DX[r][1], 16);
                QY[r][0] = DY[r][0]; QY[r][1] = __builtin_amdgcn_alignbit(DY[r][1], DY[r][0], 16); QY[r][2] = DY[r][1];
                QY[r][3] = __builtin_amdgcn_alignbit(DY[r][2], DY[r][1], 16);
            }
            const unsigned W0 = (unsigned)w00 | ((unsigned)w01 << 16), W1 = (unsigned)w10 | ((unsigned)w11 << 16);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < npx) {
                    // descale(a w00 + b w01 + c w10 + d w11, n) = (two dot products + 2^(n-1)) >> n
                    const int iv = lk_dot2(P[1][k + 1], W0, lk_dot2(P[2][k + 1], W1, 1 << 8)) >> 9;
                    const int ix = lk_dot2(QX[0][k], W0, lk_dot2(QX[1][k], W1, 1 << 13)) >> 14;
                    const int iy = lk_dot2(QY[0][k], W0, lk_dot2(QY[1][k], W1, 1 << 13)) >> 14;
                    pI[k] = iv; pIx[k] = ix; pIy[k] = iy;
                    a11 += __mul24(ix, ix); a12 += __mul24(ix, iy); a22 += __mul24(iy, iy);
                }
        }
        const float A11 = wave_sum_rows_scaled(a11), A12 = wave_sum_rows_scaled(a12), A22 = wave_sum_rows_scaled(a22);
        float D = A11 * A22 - A12 * A12;
        const float dd = A11 - A22;
        const float minEig = (A22 + A11 - sqrtf(dd * dd + 4.f * A12 * A12)) / (float)(2 * ww);
        if ((FLAGS & LK_EIG) && l == 0) errv = minEig;
        if ((double)minEig < min_eig_thr || D < FLT_EPSILON) {
            if (l == 0) st = 0;
            continue;
        }
        D = 1.f / D;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < max_count; ++j) {
            // every lane holds the same position: move the integer part to the scalar unit (bounds tests, LDS offsets)
            const int iqx = __builtin_amdgcn_readfirstlane((int)floorf(qx)), iqy = __builtin_amdgcn_readfirstlane((int)floorf(qy));
            if (iqx < -win || iqx >= lw || iqy < -win || iqy >= lh) {
                if (l == 0) st = 0;
                break;
            }
            if (!jvalid || iqx < jx0 || iqx > jx0 + 2 * LK_M || iqy < jy0 || iqy > jy0 + 2 * LK_M) stage_J(iqx, iqy);
            lk_weights(qx - (float)iqx, qy - (float)iqy, w00, w01, w10, w11);
            int b1 = 0, b2 = 0;
            if (npx > 0) {
                // two rows of 5 bytes at byte offset sh = (iqx - jx0) & 3 of two dwords each; the offset is wave-uniform, so the
                // v_perm selectors that expand the byte pairs (t[k], t[k+1]) come from the scalar unit
                const int off = (iqy - jy0 + wy) * LKF_JP + (iqx - jx0) + wx0;
                const unsigned *r0 = reinterpret_cast<const unsigned *>(s_J + (off & ~3)), *r1 = reinterpret_cast<const unsigned *>(s_J + ((off + LKF_JP) & ~3));
                const unsigned d0 = r0[0], d1 = r0[1], e0 = r1[0], e1 = r1[1];
                const unsigned shs = (unsigned)__builtin_amdgcn_readfirstlane((iqx - jx0) & 3) * 0x00010001u;
                const unsigned W0 = (unsigned)w00 | ((unsigned)w01 << 16), W1 = (unsigned)w10 | ((unsigned)w11 << 16);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < npx) {
                        const unsigned sel = LK_PAIR_SEL(k) + shs;
                        const int diff = (lk_dot2(__builtin_amdgcn_perm(d1, d0, sel), W0, lk_dot2(__builtin_amdgcn_perm(e1, e0, sel), W1, 1 << 8)) >> 9) - pI[k];
                        b1 += __mul24(diff, pIx[k]); b2 += __mul24(diff, pIy[k]);
                    }
            }
            const float fb1 = wave_sum_rows_scaled(b1), fb2 = wave_sum_rows_scaled(b2);
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
            lk_weights(ex - (float)iex, ey - (float)iey, w00, w01, w10, w11);
            int se = 0;
            if (npx > 0) {
                const int off = (iey - jy0 + wy) * LKF_JP + (iex - jx0) + wx0;
                const unsigned *r0 = reinterpret_cast<const unsigned *>(s_J + (off & ~3)), *r1 = reinterpret_cast<const unsigned *>(s_J + ((off + LKF_JP) & ~3));
                const unsigned d0 = r0[0], d1 = r0[1], e0 = r1[0], e1 = r1[1];
                const unsigned shs = (unsigned)__builtin_amdgcn_readfirstlane((iex - jx0) & 3) * 0x00010001u;
                const unsigned W0 = (unsigned)w00 | ((unsigned)w01 << 16), W1 = (unsigned)w10 | ((unsigned)w11 << 16);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < npx) {
                        const unsigned sel = LK_PAIR_SEL(k) + shs;
                        const int diff = (lk_dot2(__builtin_amdgcn_perm(d1, d0, sel), W0, lk_dot2(__builtin_amdgcn_perm(e1, e0, sel), W1, 1 << 8)) >> 9) - pI[k];
                        se += diff < 0 ? -diff : diff;
                    }
            }
            const long long SE = wave_sum_rows(se);
            errv = (float)(int)SE / (float)(32 * ww);
        }
    }
    if (lane == 0) {
        next_pts[2 * pi] = nx; next_pts[2 * pi + 1] = ny;
        status[pi] = (uint8_t)st;
        err[pi] = (FLAGS & LK_EIG) ? errv : st ? errv : 0.f;
    }
