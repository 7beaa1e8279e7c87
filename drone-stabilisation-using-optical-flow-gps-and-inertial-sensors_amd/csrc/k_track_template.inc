// k_track_template.inc — a template per track of a video stream (ofk.h: ofk_set_track_template): the patch a track was born with, the
// accumulated linear map from that patch to the current frame, the score of the current window against it and the position pulled
// back onto it.  Included by k_tracks.hip behind k_lstsq.inc (the step map's block_sums, Jacobi, rank_cut and eig_solve3).  Every
// image sum is a sum of integers in int64, so its result does not depend on the order of the additions; the f32 and f64 steps are in
// the order ofk.h states (the build has no FMA contraction).  No atomics: a second launch on the same inputs gives the same bits.

struct tp_cfg { int win, iters, outside, fit_min; double ncc_min, anchor_max, fit_gate, scale_max; };

// ---------------------------------------------------------------------------------------------- rule 1: the step map
#define TP_SUMS 13
struct tp_sums { double v[TP_SUMS]; };                        // xx xy x yy y n | x*Y0 y*Y0 Y0 | x*Y1 y*Y1 Y1 | rr

// the 3 x 3 normal equations of both image coordinates at once: k_lstsq.inc's Jacobi and rank rule over `n` rows.  fit: M (row-major), t.
__device__ bool tp_solve(const tp_sums &a, double *fit)
{
    const double *s = a.v;
    if (!all_finite_sum(s, 12)) return false;
    double A[3][3], lam[3], V[3][3]; sym3_from6(s, A);
    jacobi3(A, lam, V);
    if (!all_finite_sum(lam, 3)) return false;
    const double tol = rank_cut(lam[0], s[5]);
    for (int k = 0; k < 3; ++k)
        if (!(lam[k] > tol && lam[k] > 0.0)) return false;       // rank below 3
    for (int r = 0; r < 2; ++r) {
        double u[3];
        eig_solve3(lam, V, s + 6 + 3 * r, nullptr, u);
        fit[2 * r] = u[0]; fit[2 * r + 1] = u[1]; fit[4 + r] = u[2];
    }
    return true;
}

// One workgroup per stream, behind LK and the track gates.  Three passes over the rows i = tid + 256 k: the sums of all tracked rows,
// the sums of the rows inside fit_gate of the first fit, the squared residuals of the rows of the fit that stands.  Thread 0 solves
// between the passes and hands the fit on through LDS.
__global__ __launch_bounds__(256) void k_track_affine(const float *__restrict__ prev_pts, const float *__restrict__ next_pts,
                                                      const uint8_t *__restrict__ status, const int *__restrict__ counts, int stride, int h,
                                                      int w, tp_cfg cfg, float *__restrict__ L, double *__restrict__ rec)
{
    __shared__ double s_part[4][TP_SUMS];
    __shared__ double s_fit[6];
    __shared__ int s_ok;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[b], 0), stride);
    const size_t base = (size_t)b * stride;
    const double cx = (double)w * 0.5, cy = (double)h * 0.5, g2 = cfg.fit_gate * cfg.fit_gate;
    double fit[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 0.0}, fit2[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 0.0};   // the first fit (the gate), the second
    double n1 = 0.0, n2 = 0.0, rms = 0.0;
    bool ok = false, second = false;
    for (int pass = 0; pass < 3; ++pass) {
        if (pass == 1 && !(ok && cfg.fit_gate > 0.0)) continue;  // uniform: ok came through LDS
        if (pass == 2 && !ok) continue;
        tp_sums a;
#pragma unroll
        for (int k = 0; k < TP_SUMS; ++k) a.v[k] = 0.0;
        for (int i = tid; i < n; i += 256) {
            const size_t r = base + i;
            if (status[r] == 0) continue;
            const double x = (double)prev_pts[2 * r] - cx, y = (double)prev_pts[2 * r + 1] - cy;
            const double X = (double)next_pts[2 * r] - cx, Y = (double)next_pts[2 * r + 1] - cy;
            if (pass == 0) {
                a.v[0] += x * x; a.v[1] += x * y; a.v[2] += x; a.v[3] += y * y; a.v[4] += y; a.v[5] += 1.0;
                a.v[6] += x * X; a.v[7] += y * X; a.v[8] += X; a.v[9] += x * Y; a.v[10] += y * Y; a.v[11] += Y;
                continue;
            }
            const double rx = ((fit[0] * x + fit[1] * y) + fit[4]) - X, ry = ((fit[2] * x + fit[3] * y) + fit[5]) - Y;
            double rr = rx * rx + ry * ry;
            if ((pass == 1 || second) && !(rr <= g2)) continue;  // the rows of the second fit
            if (pass == 1) {
                a.v[0] += x * x; a.v[1] += x * y; a.v[2] += x; a.v[3] += y * y; a.v[4] += y; a.v[5] += 1.0;
                a.v[6] += x * X; a.v[7] += y * X; a.v[8] += X; a.v[9] += x * Y; a.v[10] += y * Y; a.v[11] += Y;
                continue;
            }
            if (second) {
                const double qx = ((fit2[0] * x + fit2[1] * y) + fit2[4]) - X, qy = ((fit2[2] * x + fit2[3] * y) + fit2[5]) - Y;
                rr = qx * qx + qy * qy;
            }
            a.v[12] += rr; a.v[5] += 1.0;
        }
        block_sums<TP_SUMS, TP_SUMS>(a.v, s_part);
        if (pass == 2) { rms = a.v[5] > 0.0 ? sqrt(a.v[12] / a.v[5]) : 0.0; continue; }
        if (tid == 0) {
            double f[6];
            const bool o = a.v[5] >= (double)cfg.fit_min && tp_solve(a, f);
            s_ok = o ? 1 : 0;
            if (o) for (int k = 0; k < 6; ++k) s_fit[k] = f[k];
        }
        __syncthreads();
        const bool o = s_ok != 0;
        if (pass == 0) { n1 = a.v[5]; ok = o; if (o) for (int k = 0; k < 6; ++k) fit[k] = s_fit[k]; }
        else { n2 = a.v[5]; second = o; if (o) for (int k = 0; k < 6; ++k) fit2[k] = s_fit[k]; }
        __syncthreads();
    }
    if (tid == 0) {
        double *o = rec + (size_t)b * OFK_TPL_DOUBLES;
        if (second) for (int k = 0; k < 6; ++k) fit[k] = fit2[k];
        for (int k = 0; k < 6; ++k) o[k] = fit[k];
        o[6] = ok ? 0.0 : 1.0; o[7] = n1; o[8] = n2; o[9] = rms;
        for (int k = 20; k < OFK_TPL_DOUBLES; ++k) o[k] = 0.0;
        for (int k = 0; k < 4; ++k) L[4 * b + k] = (float)fit[k];
    }
}

// ---------------------------------------------------------------------------------------------- rules 2-5: capture, score, re-anchor, verdict
__device__ __forceinline__ long long tp_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int lo = __shfl_xor((int)(v & 0xffffffffll), o), hi = __shfl_xor((int)(v >> 32), o);
        v += (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    }
    return v;
}

// The sampler S(img, p, A, o) of ofk.h: the bilinear value at scale 1024, or -1 outside.
__device__ __forceinline__ int tp_sample(const uint8_t *__restrict__ img, int h, int w, float px, float py, float a00, float a01, float a10,
                                         float a11, int ox, int oy)
{
    const float fx = (float)ox, fy = (float)oy;
    const float sx = (a00 * fx + a01 * fy) + px, sy = (a10 * fx + a11 * fy) + py;
    const float ixf = floorf(sx), iyf = floorf(sy);
    if (!(ixf >= 0.f && iyf >= 0.f && ixf + 1.f <= (float)(w - 1) && iyf + 1.f <= (float)(h - 1))) return -1;   // false for NaN and infinity too
    const int ix = (int)ixf, iy = (int)iyf;
    const int qx = (int)rintf((sx - ixf) * 32.f), qy = (int)rintf((sy - iyf) * 32.f);
    const uint8_t *r0 = img + (size_t)iy * w + ix, *r1 = r0 + w;
    return ((int)r0[0] * (32 - qx) * (32 - qy) + (int)r0[1] * qx * (32 - qy)) + ((int)r1[0] * (32 - qx) * qy + (int)r1[1] * qx * qy);
}

struct tp_img_sums { long long J, JJ, TJ, gxD, gyD; bool outside; };

// the sums of one sampling of the next frame at p through A, over the lanes of the wave; T: the wave's template in LDS, pitch win + 2
__device__ __forceinline__ tp_img_sums tp_sample_window(const uint8_t *__restrict__ img, int h, int w, float px, float py, const float *A,
                                                        const uint8_t *T, int win, int lane)
{
    const int hw = (win - 1) / 2, tp = win + 2, N = win * win;
    long long sJ = 0, sJJ = 0, sTJ = 0, sgx = 0, sgy = 0;
    bool out = false;
    for (int k = lane; k < N; k += 64) {
        const int oy = k / win, ox = k - oy * win;
        const int J = tp_sample(img, h, w, px, py, A[0], A[1], A[2], A[3], ox - hw, oy - hw);
        if (J < 0) { out = true; continue; }
        const uint8_t *c = T + (oy + 1) * tp + ox + 1;
        const int t = c[0], gx = (int)c[1] - (int)c[-1], gy = (int)c[tp] - (int)c[-tp];
        const long long D = (long long)J - 1024ll * t;
        sJ += J; sJJ += (long long)J * J; sTJ += (long long)t * J; sgx += gx * D; sgy += gy * D;
    }
    tp_img_sums s;
    s.outside = __ballot(out) != 0ull;
    s.J = tp_wave_sum(sJ); s.JJ = tp_wave_sum(sJJ); s.TJ = tp_wave_sum(sTJ); s.gxD = tp_wave_sum(sgx); s.gyD = tp_wave_sum(sgy);
    return s;
}

struct tp_state {                                              // the state's arrays, rows `stride` apart per stream in the table's row order
    uint8_t *tmpl, *tmpl_next; int tstride;                    // bytes between templates; the compaction moves them into tmpl_next
    float *A, *A_new, *ncc, *ncc_new, *move;                   // *_new, move, flag_new: what this step found, per row as tracked
    uint8_t *flag, *flag_new, *tstate;
};

// One wave per row, four rows per workgroup; grid (ceil(stride / 4), batch).  Phase 1 brings the row's template into the wave's LDS
// slab, capturing it from the previous frame where rule 2 says so; phase 2 scores and re-anchors with wave-uniform control flow: the
// int64 sums reach every lane through the xor butterfly, and every lane computes the 2 x 2 step.
__global__ __launch_bounds__(256) void k_track_template(tp_state t, const uint8_t *__restrict__ prev_img, const uint8_t *__restrict__ next_img,
                                                        size_t img_stride, int h, int w, const float *__restrict__ prev_pts, float *next_pts,
                                                        uint8_t *status, const int *__restrict__ age, const int *__restrict__ counts, int stride,
                                                        const float *__restrict__ L, tp_cfg cfg)
{
    __shared__ uint8_t s_T[4][33 * 33 + 3];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wave;
    const int n = min(max(counts[b], 0), stride);
    const bool live = i < n;
    const size_t r = (size_t)b * stride + (live ? i : 0);
    const int win = cfg.win, tp = win + 2, tn = tp * tp, hw = (win - 1) / 2, N = win * win;
    uint8_t *T = s_T[wave], *gT = t.tmpl + r * t.tstride;
    const uint8_t *pimg = prev_img + (size_t)b * img_stride, *nimg = next_img + (size_t)b * img_stride;
    bool has = false, captured = false;
    if (live) {
        has = t.tstate[r] != 0 && age[r] != 0;
        if (!has) {                                              // rule 2
            const float px = prev_pts[2 * r], py = prev_pts[2 * r + 1];
            bool out = false;
            for (int k = lane; k < tn; k += 64) {
                const int oy = k / tp, ox = k - oy * tp;
                const int S = tp_sample(pimg, h, w, px, py, 1.f, 0.f, 0.f, 1.f, ox - hw - 1, oy - hw - 1);
                if (S < 0) out = true;
                else T[k] = (uint8_t)((S + 512) >> 10);
            }
            captured = has = __ballot(out) == 0ull;
            if (has) for (int k = lane; k < tn; k += 64) gT[k] = T[k];
            if (lane == 0) {
                t.tstate[r] = has ? 1 : 0;
                if (has) { t.A[4 * r] = 1.f; t.A[4 * r + 1] = 0.f; t.A[4 * r + 2] = 0.f; t.A[4 * r + 3] = 1.f; }
            }
        } else
            for (int k = lane; k < tn; k += 64) T[k] = gT[k];
    }
    __syncthreads();                                             // the templates are in LDS; a captured row's A is read back from registers below
    if (!live) return;
    const float l0 = L[4 * b], l1 = L[4 * b + 1], l2 = L[4 * b + 2], l3 = L[4 * b + 3];
    float a[4] = {1.f, 0.f, 0.f, 1.f};
    if (has && !captured) { a[0] = t.A[4 * r]; a[1] = t.A[4 * r + 1]; a[2] = t.A[4 * r + 2]; a[3] = t.A[4 * r + 3]; }
    const float An[4] = {l0 * a[0] + l1 * a[2], l0 * a[1] + l1 * a[3], l2 * a[0] + l3 * a[2], l2 * a[1] + l3 * a[3]};   // A' = L A
    const float p0x = next_pts[2 * r], p0y = next_pts[2 * r + 1];
    float px = p0x, py = p0y, ncc = 0.f;
    int flag = OFK_TPL_NOT_TRACKED;
    bool drop = false;
    if (status[r] != 0) {
        if (!has) flag = OFK_TPL_NO_TEMPLATE;
        else {
            // the template's own sums
            long long sT = 0, sTT = 0, sgx = 0, sgy = 0, sxx = 0, sxy = 0, syy = 0;
            for (int k = lane; k < N; k += 64) {
                const int oy = k / win, ox = k - oy * win;
                const uint8_t *c = T + (oy + 1) * tp + ox + 1;
                const int v = c[0], gx = (int)c[1] - (int)c[-1], gy = (int)c[tp] - (int)c[-tp];
                sT += v; sTT += v * v; sgx += gx; sgy += gy; sxx += gx * gx; sxy += gx * gy; syy += gy * gy;
            }
            sT = tp_wave_sum(sT); sTT = tp_wave_sum(sTT); sgx = tp_wave_sum(sgx); sgy = tp_wave_sum(sgy);
            sxx = tp_wave_sum(sxx); sxy = tp_wave_sum(sxy); syy = tp_wave_sum(syy);
            const long long vT = (long long)N * sTT - sT * sT;
            const double G00 = (double)((long long)N * sxx - sgx * sgx), G01 = (double)((long long)N * sxy - sgx * sgy),
                         G11 = (double)((long long)N * syy - sgy * sgy);
            const double det = G00 * G11 - G01 * G01;
            tp_img_sums s = tp_sample_window(nimg, h, w, px, py, An, T, win, lane);
            if (s.outside) { flag = OFK_TPL_OUTSIDE; drop = cfg.outside == OFK_TPL_DROP; }
            else if (vT <= 0 || (long long)N * s.JJ - s.J * s.J <= 0) flag = OFK_TPL_FLAT;
            else {
                tp_img_sums s0 = s;
                bool abandoned = false;
                if (det > 0.0)
                    for (int it = 0; it < cfg.iters; ++it) {
                        const long long sD = s.J - 1024ll * sT;
                        const double bx = (double)((long long)N * s.gxD - sgx * sD), by = (double)((long long)N * s.gyD - sgy * sD);
                        const double dx = (G11 * bx - G01 * by) / det / 512.0, dy = (G00 * by - G01 * bx) / det / 512.0;
                        const double sx = (double)An[0] * dx + (double)An[1] * dy, sy = (double)An[2] * dx + (double)An[3] * dy;
                        const float qx = (float)((double)px - sx), qy = (float)((double)py - sy);
                        if (!(isfinite(sx) && isfinite(sy)) || !(fabsf(qx - p0x) <= (float)cfg.anchor_max && fabsf(qy - p0y) <= (float)cfg.anchor_max)) {
                            abandoned = true; break;
                        }
                        const tp_img_sums sn = tp_sample_window(nimg, h, w, qx, qy, An, T, win, lane);
                        if (sn.outside) { abandoned = true; break; }
                        px = qx; py = qy; s = sn;
                        if (sx * sx + sy * sy < 1e-4) break;
                    }
                if (abandoned) { px = p0x; py = p0y; s = s0; }
                const long long vJ = (long long)N * s.JJ - s.J * s.J, cTJ = (long long)N * s.TJ - sT * s.J;
                if (vJ <= 0) { flag = OFK_TPL_FLAT; px = p0x; py = p0y; }
                else {
                    const double rho = (double)cTJ / sqrt((double)vT * (double)vJ);
                    ncc = (float)rho;
                    if (rho < cfg.ncc_min) { flag = OFK_TPL_FAIL; drop = true; px = p0x; py = p0y; }
                    else flag = abandoned ? OFK_TPL_ABANDONED : OFK_TPL_PASS;
                }
            }
        }
    }
    if (lane == 0) {
        if (captured) flag |= OFK_TPL_CAPTURED;
        t.A_new[4 * r] = An[0]; t.A_new[4 * r + 1] = An[1]; t.A_new[4 * r + 2] = An[2]; t.A_new[4 * r + 3] = An[3];
        t.ncc_new[r] = ncc; t.flag_new[r] = (uint8_t)flag;
        t.move[r] = fmaxf(fabsf(px - p0x), fabsf(py - p0y));
        if (drop) status[r] = 0;
        else if (px != p0x || py != p0y) { next_pts[2 * r] = px; next_pts[2 * r + 1] = py; }
    }
}

// ---------------------------------------------------------------------------------------------- rule 6: compaction
// A fresh row at index q: no template yet (rule 2 captures one), the identity map, nothing scored.
__device__ __forceinline__ void tp_fresh_row(const tp_state &t, size_t q)
{
    t.A[4 * q] = 1.f; t.A[4 * q + 1] = 0.f; t.A[4 * q + 2] = 0.f; t.A[4 * q + 3] = 1.f;
    t.ncc[q] = 0.f; t.flag[q] = OFK_TPL_NOT_TRACKED; t.tstate[q] = 0;
}

// In front of k_track_table_update, with its keep rule and its walk (k_rows.inc).  One workgroup per stream.  The scalars of a step
// (A_new, ncc_new, flag_new) move into the state's arrays at the kept rows' new places; tstate moves in place; the templates move from
// one buffer into the other, a wave per row in 4-byte words (the host swaps the two), their places reaching the waves through s_pos behind
// rows_next's barrier and changing only behind the next rows_place's, when every wave has copied.  The counts are ballots summed per wave.
__global__ __launch_bounds__(256) void k_track_template_update(tp_state t, const uint8_t *__restrict__ status, const int *__restrict__ counts_in,
                                                               int stride, const int *__restrict__ new_counts, int max_total, tp_cfg cfg,
                                                               double *__restrict__ rec)
{
    __shared__ row_walk s_rows;
    __shared__ int s_cnt[4][9], s_pos[256];
    __shared__ float s_move[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(counts_in[b], 0), stride);
    const size_t base = (size_t)b * stride;
    const float s2 = (float)(cfg.scale_max * cfg.scale_max), s2i = (float)(1.0 / (cfg.scale_max * cfg.scale_max));
    int cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};                    // scored dropped moved abandoned outside flat captured no-template refresh
    float mv = 0.f;
    rows_begin(s_rows);
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool in = i < n;
        const size_t r = base + (in ? i : 0);
        const bool keep = in && status[r] != 0;
        const int fl = in ? t.flag_new[r] : 0, verdict = fl & 15;
        const float a0 = t.A_new[4 * r], a1 = t.A_new[4 * r + 1], a2 = t.A_new[4 * r + 2], a3 = t.A_new[4 * r + 3];
        const float ncc = t.ncc_new[r], move = t.move[r];
        int ts = t.tstate[r];
        const float det = a0 * a3 - a1 * a2;
        const bool refresh = keep && ts != 0 && cfg.scale_max > 0.0 && !(det <= s2 && det >= s2i);
        if (refresh) ts = 0;
        const bool moved = in && verdict == OFK_TPL_PASS && move > 0.f;
        if (moved) mv = fmaxf(mv, move);
        const bool f[9] = {in && (verdict == OFK_TPL_PASS || verdict == OFK_TPL_FAIL || verdict == OFK_TPL_ABANDONED),
                           in && (verdict == OFK_TPL_FAIL || (verdict == OFK_TPL_OUTSIDE && cfg.outside == OFK_TPL_DROP)), moved, in && verdict == OFK_TPL_ABANDONED,
                           in && verdict == OFK_TPL_OUTSIDE, in && verdict == OFK_TPL_FLAT, in && (fl & OFK_TPL_CAPTURED) != 0,
                           in && verdict == OFK_TPL_NO_TEMPLATE, refresh};
#pragma unroll
        for (int k = 0; k < 9; ++k) cnt[k] += __popcll(__ballot(f[k]));
        const int pos = rows_place(s_rows, keep);
        s_pos[tid] = keep ? pos : -1;
        if (keep) {
            const size_t q = base + pos;
            t.A[4 * q] = a0; t.A[4 * q + 1] = a1; t.A[4 * q + 2] = a2; t.A[4 * q + 3] = a3;
            t.ncc[q] = ncc; t.flag[q] = (uint8_t)fl; t.tstate[q] = (uint8_t)ts;
        }
        rows_next(s_rows);
        const int words = t.tstride >> 2;
        for (int j = wave; j < 256; j += 4) {
            const int q = s_pos[j];
            if (q < 0) continue;
            const uint32_t *src = (const uint32_t *)(t.tmpl + (base + i0 + j) * t.tstride);
            uint32_t *dst = (uint32_t *)(t.tmpl_next + (base + q) * t.tstride);
            for (int k = lane; k < words; k += 64) dst[k] = src[k];
        }
    }
    const int kept = s_rows.base;
    const int extra = rows_extra(new_counts, b, max_total, stride, kept);
    for (int i = tid; i < extra; i += 256) tp_fresh_row(t, base + kept + i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mv = fmaxf(mv, __shfl_xor(mv, o));
    if (lane == 0) {
        for (int k = 0; k < 9; ++k) s_cnt[wave][k] = cnt[k];
        s_move[wave] = mv;
    }
    __syncthreads();
    if (tid == 0) {
        double *o = rec + (size_t)b * OFK_TPL_DOUBLES;
        for (int k = 0; k < 9; ++k) o[10 + k] = (double)(s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k]);
        o[19] = (double)fmaxf(fmaxf(s_move[0], s_move[1]), fmaxf(s_move[2], s_move[3]));
    }
}

static tp_cfg tp_make_cfg(const ofk_track_template *d)
{
    tp_cfg c;
    c.win = d->win; c.iters = d->anchor_iters; c.outside = d->outside; c.fit_min = d->fit_min;
    c.ncc_min = d->ncc_min; c.anchor_max = d->anchor_max; c.fit_gate = d->fit_gate; c.scale_max = d->scale_max;
    return c;
}

void ofk_launch_track_affine(hipStream_t s, const float *prev_pts, const float *next_pts, const uint8_t *status, const int *counts, int stride,
                             int h, int w, const ofk_track_template *d, float *L, double *rec, int batch)
{
    hipLaunchKernelGGL(k_track_affine, dim3(batch), dim3(256), 0, s, prev_pts, next_pts, status, counts, stride, h, w, tp_make_cfg(d), L, rec);
}

void ofk_launch_track_template(hipStream_t s, const ofk_tp_rows &t, const uint8_t *prev_img, const uint8_t *next_img, size_t img_stride, int h,
                               int w, const float *prev_pts, float *next_pts, uint8_t *status, const int *age, const int *counts, int stride,
                               const ofk_track_template *d, int batch)
{
    const tp_state st = {t.tmpl[t.cur], t.tmpl[t.cur ^ 1], t.tstride, t.A, t.A_new, t.ncc, t.ncc_new, t.move, t.flag, t.flag_new, t.tstate};
    hipLaunchKernelGGL(k_track_template, dim3((stride + 3) / 4, batch), dim3(256), 0, s, st, prev_img, next_img, img_stride, h, w, prev_pts,
                       next_pts, status, age, counts, stride, t.L, tp_make_cfg(d));
}

void ofk_launch_track_template_update(hipStream_t s, const ofk_tp_rows &t, const uint8_t *status, const int *counts, int stride,
                                      const int *new_counts, int max_total, const ofk_track_template *d, int batch)
{
    const tp_state st = {t.tmpl[t.cur], t.tmpl[t.cur ^ 1], t.tstride, t.A, t.A_new, t.ncc, t.ncc_new, t.move, t.flag, t.flag_new, t.tstate};
    hipLaunchKernelGGL(k_track_template_update, dim3(batch), dim3(256), 0, s, st, status, counts, stride, new_counts, max_total, tp_make_cfg(d),
                       t.rec);
}
