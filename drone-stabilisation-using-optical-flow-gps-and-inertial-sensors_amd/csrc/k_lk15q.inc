    constexpr int win = 15, ww = 225;
    constexpr float half = 7.f;
    __shared__ __attribute__((aligned(16))) uint8_t s_I[4 * LKQ_ISZ];
    __shared__ __attribute__((aligned(16))) uint8_t s_J[4 * LKQ_JSZ];
    __shared__ unsigned s_dump[64];                                // where the staging writes of slots outside a row go (one word per lane)

    const int lane = threadIdx.x, g = lane >> 4, r = lane & 15;
    unsigned *dump = s_dump + lane;
    int b = blockIdx.y, chunk = blockIdx.x;                        // XCD-aware map as in k_lk15: the points of an image stay on one XCD
    if ((gridDim.y & 7) == 0) {
        const unsigned n = blockIdx.y * gridDim.x + blockIdx.x, k = n >> 3;
        b = 8 * (int)(k / gridDim.x) + (int)(n & 7);
        chunk = (int)(k % gridDim.x);
    }
    const int cnt = counts[b];
    if (chunk * 4 >= cnt) return;
    const int p = chunk * 4 + g;
    const bool live = p < cnt;
    const size_t pi = (size_t)b * pts_stride + min(p, cnt - 1);
    const float ptx = prev_pts[2 * pi], pty = prev_pts[2 * pi + 1];
    const uint8_t *Pb = prev + (size_t)b * pyr_stride, *Nb = next + (size_t)b * pyr_stride;
    uint8_t *sI = s_I + g * LKQ_ISZ, *sJ = s_J + g * LKQ_JSZ;
    const bool rowact = r < win;                                   // lane 15 of a row only stages and computes derivative row 15

    int st = 1;
    float errv = 0.f, nx = 0.f, ny = 0.f;
    if (FLAGS & LK_SEED) { nx = next_pts[2 * pi]; ny = next_pts[2 * pi + 1]; }      // the start position travels in the carry
    // Ix and Iy of the lane's 15 window pixels as int16 PAIRS OF NEIGHBOURING PIXELS: pxx[j] = (Ix[2j], Ix[2j+1]), pyy likewise (the last
    // pair's upper half is zero).  Every sum over the row is then a v_dot2_i32_i16 per pixel pair: the normal matrix (3 per pair where
    // round 2 spent 3 multiplies + 3 adds per pixel) and the mismatch vector (pack the two interpolated values with one v_lshl_or, two
    // dot2: 1.5 per pixel where two v_mad_i32_i16 stood) - 7 % fewer instructions per point, sums bit for bit the same integers.
    unsigned pxx[8], pyy[8];

    for (int l = lv.n; l >= 0; --l) {
        const int lh = lv.h[l], lw = lv.w[l];
        const uint8_t *I = Pb + lv.off[l], *J = Nb + lv.off[l];
        const float sc = __int_as_float((127 - l) << 23);
        float px = ptx * sc, py = pty * sc, qx, qy;
        if (l == lv.n) { qx = px; qy = py; } else { qx = nx * 2.f; qy = ny * 2.f; }
        if ((FLAGS & LK_SEED) && l == lv.n) { qx = nx * sc; qy = ny * sc; }
        nx = qx; ny = qy;
        px -= half; py -= half;
        const int ipx = lkq_floor_i(px), ipy = lkq_floor_i(py);
        const bool lev = live && !(ipx < -win || ipx >= lw || ipy < -win || ipy >= lh);
        if (live && !lev && l == 0) { st = 0; errv = 0.f; }
        if (__builtin_amdgcn_ballot_w64(lev) == 0) continue;
        qx -= half; qy -= half;

        int jx0 = 0, jy0 = 0, jA = 0;
        bool jvalid = false;
        // The next-frame region of the lanes that are `on`: rows jy0 + r and jy0 + r + 16 from column jA.  At the start of a level
        // both rows are loaded before the first wait (J_issue / J_commit around the prev-frame staging); a re-staging inside the
        // Newton loop (the window walked out of the region: rare) goes row by row to keep 9 registers fewer alive in the loop.
        unsigned jd[2][9];
        auto J_place = [&](int iqx, int iqy, bool on) {
            if (on) { jx0 = iqx - LK_M; jy0 = iqy - LK_M; jA = jx0 & ~3; jvalid = true; }
        };
        auto J_load = [&](int h, bool on) {
            if (on) lkq_load_row<9>(J + (size_t)lkq_reflect(jy0 + r + 16 * h, lh) * lw, lw, jA, jd[h]);
        };
        auto J_store = [&](int h, bool on, bool border) {
            if (on) lkq_store_row<9>(reinterpret_cast<unsigned *>(sJ + (r + 16 * h) * LKQ_JP), dump, lw, jA, border, jd[h]);
        };
        auto J_border = [&](bool on) { return __builtin_amdgcn_ballot_w64(on && (jA < 0 || jA + 36 > lw)) != 0; };
        auto J_restage = [&](int iqx, int iqy, bool on) {
            J_place(iqx, iqy, on);
            const bool border = J_border(on);
            LDS_FENCE();                                                  // earlier readers of s_J are done
            J_load(0, on); J_store(0, on, border);
            LDS_FENCE();
            J_load(1, on); J_store(1, on, border);
            LDS_FENCE();
        };
        // ---- staging: prev neighbourhood rows ipy-1 .. ipy+16 (lane r: row r; lanes 0, 1 also rows 16, 17), columns from
        //      iA = (ipx-1) & ~3; then the next-frame region around the start position.  All loads are issued before the first wait.
        const int iA = (ipx - 1) & ~3;
        {
            const bool iborder = __builtin_amdgcn_ballot_w64(lev && (iA < 0 || iA + 24 > lw)) != 0;
            unsigned id0[6], id1[6];
            if (lev) {
                lkq_load_row<6>(I + (size_t)lkq_reflect(ipy - 1 + r, lh) * lw, lw, iA, id0);
                if (r < 2) lkq_load_row<6>(I + (size_t)lkq_reflect(ipy + 15 + r, lh) * lw, lw, iA, id1);
            }
            const int iqx = lkq_floor_i(qx), iqy = lkq_floor_i(qy);
            const bool doJ = lev && !(iqx < -win || iqx >= lw || iqy < -win || iqy >= lh);
            J_place(iqx, iqy, doJ);
            J_load(0, doJ); J_load(1, doJ);
            LDS_FENCE();                                                  // the previous level's readers of s_I and s_J are done
            if (lev) {
                lkq_store_row<6>(reinterpret_cast<unsigned *>(sI + r * LKQ_IP), dump, lw, iA, iborder, id0);
                if (r < 2) lkq_store_row<6>(reinterpret_cast<unsigned *>(sI + (r + 16) * LKQ_IP), dump, lw, iA, iborder, id1);
            }
            const bool jborder = J_border(doJ);
            J_store(0, doJ, jborder); J_store(1, doJ, jborder);
            LDS_FENCE();
        }
        // taps of the lane's window row: two LDS rows (pitch `pitch`) from byte offset `off` of `base`, 5 raw dwords each, and the
        // byte-pair selectors; value k = interpolated pixel k with 5 fractional bits (descale by 9 of the four weighted taps)
        unsigned jr0[5], jr1[5], jsel[4];
        auto taps_read = [&](const uint8_t *base, unsigned off, int pitch) {
            const unsigned *q = reinterpret_cast<const unsigned *>(base + (off & ~3u));
#pragma unroll
            for (int i = 0; i < 5; ++i) { jr0[i] = q[i]; jr1[i] = q[i + pitch / 4]; }
            const unsigned shs = (off & 3u) | ((off & 3u) << 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) jsel[i] = LK_PAIR_SEL(i) + shs;
        };
        auto tap_value = [&](int k, unsigned W0_, unsigned W1_) {
            return lk_dot2(__builtin_amdgcn_perm(jr0[(k >> 2) + 1], jr0[k >> 2], jsel[k & 3]), W0_,
                           lkq_dot2_k(__builtin_amdgcn_perm(jr1[(k >> 2) + 1], jr1[k >> 2], jsel[k & 3]), W1_, 1 << 8)) >> 9;
        };
        auto J_read = [&](int ix_, int iy_, bool on) {
            taps_read(sJ, on && rowact ? __umul24((unsigned)(iy_ - jy0 + r), LKQ_JP) + (unsigned)(ix_ - jA) : 0u, LKQ_JP);
        };
        // previous-frame window row r: neighbourhood rows r+1, r+2 from column 1
        auto I_read = [&]() { taps_read(sI, (unsigned)((r + 1) * LKQ_IP + ((ipx - 1) & 3) + 1), LKQ_IP); };
        // ---- patch.  Neighbourhood rows r, r+1, r+2 -> derivative row r (16 columns); window row r = derivative rows r, r+1.
        int w00, w01, w10, w11;
        lk_weights(px - (float)ipx, py - (float)ipy, w00, w01, w10, w11);
        const unsigned W0 = (unsigned)w00 | ((unsigned)w01 << 16), W1 = (unsigned)w10 | ((unsigned)w11 << 16);
        unsigned a11 = 0, a22 = 0;
        int a12 = 0, c1 = 0, c2 = 0;
        {
            const unsigned ishs = (unsigned)((ipx - 1) & 3) * 0x00010001u;
            const unsigned sel0 = LK_PAIR_SEL(0) + ishs, sel1 = LK_PAIR_SEL(1) + ishs, sel2 = LK_PAIR_SEL(2) + ishs, sel3 = LK_PAIR_SEL(3) + ishs;
            unsigned R[3][6];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned *q = reinterpret_cast<const unsigned *>(sI + (r + j) * LKQ_IP);
#pragma unroll
                for (int i = 0; i < 6; ++i) R[j][i] = q[i];
            }
            // pair (n[c], n[c+1]) of neighbourhood row j: bytes c + ish, c + 1 + ish of the row's dwords
            auto pair = [&](int j, int c) {
                const unsigned sel = (c & 3) == 0 ? sel0 : (c & 3) == 1 ? sel1 : (c & 3) == 2 ? sel2 : sel3;
                return __builtin_amdgcn_perm(R[j][(c >> 2) + 1], R[j][c >> 2], sel);
            };
            lk_s2 VS[9], VD[9];
#pragma unroll
            for (int s = 0; s < 9; ++s) {
                const lk_s2 e0 = lk_as_s2(pair(0, 2 * s)), e1 = lk_as_s2(pair(1, 2 * s)), e2 = lk_as_s2(pair(2, 2 * s));
                VS[s] = (e0 + e2) * (short)3 + e1 * (short)10;
                VD[s] = e2 - e0;
            }
            unsigned DX[8], DY[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                DX[s] = lk_as_u(VS[s + 1] - VS[s]);
                const lk_s2 m = lk_as_s2(__builtin_amdgcn_alignbit(lk_as_u(VD[s + 1]), lk_as_u(VD[s]), 16));
                DY[s] = lk_as_u((VD[s] + VD[s + 1]) * (short)3 + m * (short)10);
            }
            // constant-0 border of the derivative image: taps (ipx + x, ipy + r) outside the level are zero
            if (__builtin_amdgcn_ballot_w64(lev && !(ipx >= 0 && ipx + win < lw && ipy >= 0 && ipy + win < lh)) != 0) {
                const int Y = ipy + r;
                const bool rowok = Y >= 0 && Y < lh;
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int X = ipx + 2 * s;
                    const unsigned keep = ((rowok && X >= 0 && X < lw) ? 0x0000ffffu : 0u) | ((rowok && X + 1 >= 0 && X + 1 < lw) ? 0xffff0000u : 0u);
                    DX[s] &= keep; DY[s] &= keep;
                }
            }
            int ixp = 0, iyp = 0;
#pragma unroll
            for (int k = 0; k < 15; ++k) {
                const unsigned qx_ = (k & 1) ? __builtin_amdgcn_alignbit(DX[(k + 1) >> 1], DX[k >> 1], 16) : DX[k >> 1];
                const unsigned qy_ = (k & 1) ? __builtin_amdgcn_alignbit(DY[(k + 1) >> 1], DY[k >> 1], 16) : DY[k >> 1];
                // own derivative row with the upper weights; the lower-weight half comes from the lane below (row r + 1)
                const int hx = lkq_dot2_k(qx_, W0, 1 << 13), gx = lk_dot2(qx_, W1, 0);
                const int hy = lkq_dot2_k(qy_, W0, 1 << 13), gy = lk_dot2(qy_, W1, 0);
                const int ix = (hx + __builtin_amdgcn_update_dpp(0, gx, 0x101, 0xF, 0xF, true)) >> 14;     // row_shl:1
                const int iy = (hy + __builtin_amdgcn_update_dpp(0, gy, 0x101, 0xF, 0xF, true)) >> 14;
                if (k & 1) {
                    pxx[k >> 1] = __builtin_amdgcn_perm((unsigned)ix, (unsigned)ixp, 0x05040100u);
                    pyy[k >> 1] = __builtin_amdgcn_perm((unsigned)iy, (unsigned)iyp, 0x05040100u);
                } else if (k == 14) {
                    pxx[7] = (unsigned)ix & 0xffffu; pyy[7] = (unsigned)iy & 0xffffu;
                }
                ixp = ix; iyp = iy;
            }
            if (!(lev && rowact)) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { pxx[j] = 0u; pyy[j] = 0u; }
            }
            // |Ix|, |Iy| <= 4080: a lane's 15 squares sum below 2.5e8, so the signed dot products are exact
            int s11 = 0, s22 = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) { s11 = lk_dot2(pxx[j], pxx[j], s11); s22 = lk_dot2(pyy[j], pyy[j], s22); a12 = lk_dot2(pxx[j], pyy[j], a12); }
            a11 = (unsigned)s11; a22 = (unsigned)s22;
        }
        // c = sum(I * Ix), sum(I * Iy) over the lane's row: the constant part of the mismatch sums (pxy is zero on idle lanes)
        I_read();
#pragma unroll
        for (int j = 0; j < 8; ++j) {                            // interpolated values are 13-bit and non-negative: two per register
            const unsigned ivp = j < 7 ? (unsigned)tap_value(2 * j, W0, W1) | ((unsigned)tap_value(2 * j + 1, W0, W1) << 16) : (unsigned)tap_value(14, W0, W1);
            c1 = lk_dot2(ivp, pxx[j], c1); c2 = lk_dot2(ivp, pyy[j], c2);
        }
        const unsigned A11u = (unsigned)lkq_row_sum((int)a11), A22u = (unsigned)lkq_row_sum((int)a22);
        float A12 = (float)lkq_row_sum(a12) * 0x1p-20f;
        if (__builtin_amdgcn_ballot_w64(lev && max(A11u, A22u) >= 0x80000000u) != 0) {
            const float A12x = lkq_row_sum_split(a12);
            if (max(A11u, A22u) >= 0x80000000u) A12 = A12x;
        }
        const float A11 = (float)A11u * 0x1p-20f, A22 = (float)A22u * 0x1p-20f;
        const bool safe = A11u < LKQ_SAFE_LIM && A22u < LKQ_SAFE_LIM;
        float D = A11 * A22 - A12 * A12;
        const float dd = A11 - A22;
        const float minEig = (A22 + A11 - sqrtf(dd * dd + 4.f * A12 * A12)) / (float)(2 * ww);
        const bool solv = lev && !((double)minEig < min_eig_thr || D < FLT_EPSILON);
        if ((FLAGS & LK_EIG) && lev && l == 0) errv = minEig;
        if (lev && !solv && l == 0) st = 0;
        D = 1.f / D;

        bool act = solv;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < max_count; ++j) {
            if (__builtin_amdgcn_ballot_w64(act) == 0) break;
            const int iqx = lkq_floor_i(qx), iqy = lkq_floor_i(qy);
            if (act && (iqx < -win || iqx >= lw || iqy < -win || iqy >= lh)) {
                if (l == 0) st = 0;
                act = false;
            }
            const bool need = act && (!jvalid || (unsigned)(iqx - jx0) > 2u * LK_M || (unsigned)(iqy - jy0) > 2u * LK_M);
            if (__builtin_amdgcn_ballot_w64(need) != 0) J_restage(iqx, iqy, need);
            lk_weights(qx - (float)iqx, qy - (float)iqy, w00, w01, w10, w11);
            const unsigned V0 = (unsigned)w00 | ((unsigned)w01 << 16), V1 = (unsigned)w10 | ((unsigned)w11 << 16);
            J_read(iqx, iqy, act);
            int b1 = -c1, b2 = -c2;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned jvp = j < 7 ? (unsigned)tap_value(2 * j, V0, V1) | ((unsigned)tap_value(2 * j + 1, V0, V1) << 16) : (unsigned)tap_value(14, V0, V1);
                b1 = lk_dot2(jvp, pxx[j], b1); b2 = lk_dot2(jvp, pyy[j], b2);
            }
            float fb1 = (float)lkq_row_sum(b1) * 0x1p-20f, fb2 = (float)lkq_row_sum(b2) * 0x1p-20f;
            if (__builtin_amdgcn_ballot_w64(act && !safe) != 0) {
                const float x1 = lkq_row_sum_split(b1), x2 = lkq_row_sum_split(b2);
                if (!safe) { fb1 = x1; fb2 = x2; }
            }
            const float dx = (A12 * fb2 - A22 * fb1) * D, dy = (A12 * fb1 - A11 * fb2) * D;
            if (act) {
                qx += dx; qy += dy;
                nx = qx + half; ny = qy + half;
                const float d2 = dx * dx + dy * dy;
                bool done = d2 < eps2_lo;
                if (!done && d2 <= eps2_hi && (double)dx * (double)dx + (double)dy * (double)dy <= eps2) done = true;
                if (!done && j > 0 && fabsf(dx + pdx) <= 0.01f && fabsf(dy + pdy) <= 0.01f) {
                    nx -= dx * 0.5f; ny -= dy * 0.5f;
                    done = true;
                }
                act = !done;
                pdx = dx; pdy = dy;
            }
        }
        if (l == 0) {
            bool eact = solv && st != 0;
            const float ex = nx - half, ey = ny - half;
            const int iex = lkq_floor_i(ex), iey = lkq_floor_i(ey);
            if (eact && (iex < -win || iex >= lw || iey < -win || iey >= lh)) { st = 0; eact = false; }
            if (!(FLAGS & LK_EIG) && __builtin_amdgcn_ballot_w64(eact) != 0) {
                const bool need = eact && (!jvalid || (unsigned)(iex - jx0) > 2u * LK_M || (unsigned)(iey - jy0) > 2u * LK_M);
                if (__builtin_amdgcn_ballot_w64(need) != 0) J_restage(iex, iey, need);
                lk_weights(ex - (float)iex, ey - (float)iey, w00, w01, w10, w11);
                const unsigned V0 = (unsigned)w00 | ((unsigned)w01 << 16), V1 = (unsigned)w10 | ((unsigned)w11 << 16);
                // the previous-frame values are recomputed from the staged neighbourhood (level 0 is still in s_I): keeping them in
                // registers through the Newton loop would cost 15 VGPRs for one use per point
                int pv[15];
                I_read();
#pragma unroll
                for (int k = 0; k < 15; ++k) pv[k] = tap_value(k, W0, W1);
                J_read(iex, iey, eact);
                int se = 0;
#pragma unroll
                for (int k = 0; k < 15; ++k) {
                    const int diff = tap_value(k, V0, V1) - pv[k];
                    se += diff < 0 ? -diff : diff;
                }
                if (!(eact && rowact)) se = 0;
                se = lkq_row_sum(se);
                if (eact) errv = (float)se / (float)(32 * ww);
            }
        }
    }
    if (live && r == 0) {
        next_pts[2 * pi] = nx; next_pts[2 * pi + 1] = ny;
        status[pi] = (uint8_t)st;
        err[pi] = (FLAGS & LK_EIG) ? errv : st ? errv : 0.f;
    }
