/* Test-side reference of the lighting-insensitive Lucas-Kanade (include/ofk.h: ofk_lk_light): tests/lk_seed_reference.c - itself
 * oracle/image_oracle.c:orc_lk_pyr with the seed and min-eigenvalue flags - restated with rules 1-6 of the header.  Compiled by
 * tests/lk_light_reference.py into a temporary directory with the oracle Makefile's flags (no contraction).
 *
 * With mode 0 every operation, its precision and its order are those of ref_lk_seeded, so the results are the same bits
 * (tests/test_lk_light_reference.py holds it to that).  With mode 1 (bias) or 2 (gain and bias) the mismatch vector and the
 * residual err are formed from exact 64-bit integer sums and a handful of f64 operations in the header's order.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define REF_USE_INITIAL_FLOW 4
#define REF_GET_MIN_EIGENVALS 8
#define REF_LIGHT_GAIN 2

typedef struct { const uint8_t *img; const int16_t *der; int h, w; } lvl_t;

static inline int refl(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}
static inline int dsc(int v, int n) { return (v + (1 << (n - 1))) >> n; }
static inline int rhe(float v) { return (int)lrintf(v); }
static inline int pixel(const lvl_t *L, int y, int x) { return L->img[(long)refl(y, L->h) * L->w + refl(x, L->w)]; }
static inline void deriv(const lvl_t *L, int y, int x, int *dx, int *dy)
{
    if (x < 0 || y < 0 || x >= L->w || y >= L->h) { *dx = 0; *dy = 0; return; }
    *dx = L->der[2 * ((long)y * L->w + x)]; *dy = L->der[2 * ((long)y * L->w + x) + 1];
}
static void wts(float a, float b, int iw[4])
{
    iw[0] = rhe((1.f - a) * (1.f - b) * 16384.f);
    iw[1] = rhe(a * (1.f - b) * 16384.f);
    iw[2] = rhe((1.f - a) * b * 16384.f);
    iw[3] = 16384 - iw[0] - iw[1] - iw[2];
}
static inline int interp(const lvl_t *J, int Y, int X, const int iw[4])
{
    return dsc(pixel(J, Y, X) * iw[0] + pixel(J, Y, X + 1) * iw[1] + pixel(J, Y + 1, X) * iw[2] + pixel(J, Y + 1, X + 1) * iw[3], 14 - 5);
}

/* rules 3-4: the gain of one step from the template's and the step's sums */
static double gain_of(int mode, int64_t N, int64_t vI, int64_t SJ, int64_t SJJ, double lo, double hi)
{
    if (mode != REF_LIGHT_GAIN) return 1.0;
    const int64_t vJ = N * SJJ - SJ * SJ;
    if (vI <= 0 || vJ <= 0) return 1.0;
    double a = sqrt((double)vI / (double)vJ);
    if (a < lo) a = lo;
    if (a > hi) a = hi;
    return a;
}

/* prev/next/der: L + 1 level pointers (level 0 first), hs/ws their sizes; seed may be NULL unless flag 4 is set;
 * iters (nullable): Newton steps of point p on level l at iters[p * 9 + l]; mode 0 / 1 / 2 = OFK_LIGHT_OFF / _BIAS / _GAIN,
 * gain_max as in ofk_lk_light (read with mode 2 only). */
int ref_lk_light(const uint8_t *const *prev, const uint8_t *const *next, const int16_t *const *der, const int *hs, const int *ws,
                  int L, const float *prev_pts, const float *seed, int n, int win, int max_count, double eps, double min_eig_thr,
                  int flags, int mode, double gain_max, float *next_pts, uint8_t *status, float *err, int *iters)
{
    if (mode < 0 || mode > 2 || (mode && !(gain_max > 1.0 && gain_max <= DBL_MAX))) return -3;
    const double g_lo = 1.0 / gain_max, g_hi = gain_max;
    if (win < 3 || win > 31 || (win & 1) == 0 || L < 0 || L > 8) return -1;
    if ((flags & REF_USE_INITIAL_FLOW) && !seed) return -2;
    if (max_count < 0) max_count = 0;
    if (max_count > 100) max_count = 100;
    if (eps < 0) eps = 0;
    if (eps > 10) eps = 10;
    const double eps2 = eps * eps;
    const int geteig = (flags & REF_GET_MIN_EIGENVALS) != 0;
    lvl_t P[9], Q[9];
    for (int l = 0; l <= L; ++l) {
        P[l].img = prev[l]; P[l].der = der[l]; Q[l].img = next[l]; Q[l].der = 0;
        P[l].h = Q[l].h = hs[l]; P[l].w = Q[l].w = ws[l];
    }
    const float half = (float)(win - 1) * 0.5f;
    const int ww = win * win;
    const int64_t N = ww;
    int16_t *Jp = (int16_t *)malloc(ww * 2);
    int16_t *Ip = (int16_t *)malloc(ww * 2), *Ixp = (int16_t *)malloc(ww * 2), *Iyp = (int16_t *)malloc(ww * 2);

    for (int p = 0; p < n; ++p) {
        status[p] = 1;
        err[p] = 0.f;
        float nx = 0.f, ny = 0.f;
        for (int l = L; l >= 0; --l) {
            const lvl_t *I = &P[l], *J = &Q[l];
            const float sc = (float)(1.0 / (double)(1 << l));
            float px = prev_pts[2 * p] * sc, py = prev_pts[2 * p + 1] * sc;
            float qx, qy;
            if (l == L) {
                if (flags & REF_USE_INITIAL_FLOW) { qx = seed[2 * p] * sc; qy = seed[2 * p + 1] * sc; }
                else { qx = px; qy = py; }
            } else { qx = nx * 2.f; qy = ny * 2.f; }
            nx = qx; ny = qy;
            px -= half; py -= half;
            const int ipx = (int)floorf(px), ipy = (int)floorf(py);
            if (ipx < -win || ipx >= I->w || ipy < -win || ipy >= I->h) {
                if (l == 0) { status[p] = 0; err[p] = 0.f; }
                continue;
            }
            int iw[4];
            wts(px - (float)ipx, py - (float)ipy, iw);
            int64_t sA11 = 0, sA12 = 0, sA22 = 0;
            int64_t SI = 0, SII = 0, SIx = 0, SIy = 0, SIIx = 0, SIIy = 0;       /* rule 1 */
            for (int y = 0; y < win; ++y)
                for (int x = 0; x < win; ++x) {
                    const int Y = ipy + y, X = ipx + x;
                    const int iv = interp(I, Y, X, iw);
                    int ax, ay, bx, by, cx, cy, dx, dy;
                    deriv(I, Y, X, &ax, &ay); deriv(I, Y, X + 1, &bx, &by);
                    deriv(I, Y + 1, X, &cx, &cy); deriv(I, Y + 1, X + 1, &dx, &dy);
                    const int ix = dsc(ax * iw[0] + bx * iw[1] + cx * iw[2] + dx * iw[3], 14);
                    const int iy = dsc(ay * iw[0] + by * iw[1] + cy * iw[2] + dy * iw[3], 14);
                    Ip[y * win + x] = (int16_t)iv; Ixp[y * win + x] = (int16_t)ix; Iyp[y * win + x] = (int16_t)iy;
                    sA11 += (int64_t)ix * ix; sA12 += (int64_t)ix * iy; sA22 += (int64_t)iy * iy;
                    SI += iv; SII += (int64_t)iv * iv; SIx += ix; SIy += iy; SIIx += (int64_t)iv * ix; SIIy += (int64_t)iv * iy;
                }
            const float A11 = (float)((double)sA11 * 0x1p-20), A12 = (float)((double)sA12 * 0x1p-20),
                        A22 = (float)((double)sA22 * 0x1p-20);
            float D = A11 * A22 - A12 * A12;
            const float dd = A11 - A22;
            const float minEig = (A22 + A11 - sqrtf(dd * dd + 4.f * A12 * A12)) / (float)(2 * ww);
            if (geteig && l == 0) err[p] = minEig;
            if ((double)minEig < min_eig_thr || D < FLT_EPSILON) {
                if (l == 0) status[p] = 0;
                continue;
            }
            D = 1.f / D;
            const int64_t vI = N * SII - SI * SI, cIx = N * SIIx - SI * SIx, cIy = N * SIIy - SI * SIy;
            qx -= half; qy -= half;
            float pdx = 0.f, pdy = 0.f;
            for (int j = 0; j < max_count; ++j) {
                const int iqx = (int)floorf(qx), iqy = (int)floorf(qy);
                if (iqx < -win || iqx >= J->w || iqy < -win || iqy >= J->h) {
                    if (l == 0) status[p] = 0;
                    break;
                }
                if (iters) iters[p * 9 + l] = j + 1;
                wts(qx - (float)iqx, qy - (float)iqy, iw);
                float b1, b2;
                if (!mode) {
                    int64_t sb1 = 0, sb2 = 0;
                    for (int y = 0; y < win; ++y)
                        for (int x = 0; x < win; ++x) {
                            const int diff = interp(J, iqy + y, iqx + x, iw) - Ip[y * win + x];
                            sb1 += (int64_t)diff * Ixp[y * win + x]; sb2 += (int64_t)diff * Iyp[y * win + x];
                        }
                    b1 = (float)((double)sb1 * 0x1p-20); b2 = (float)((double)sb2 * 0x1p-20);
                } else {
                    int64_t SJ = 0, SJJ = 0, SJx = 0, SJy = 0;                   /* rule 2 */
                    for (int y = 0; y < win; ++y)
                        for (int x = 0; x < win; ++x) {
                            const int jv = interp(J, iqy + y, iqx + x, iw);
                            SJ += jv; SJJ += (int64_t)jv * jv; SJx += (int64_t)jv * Ixp[y * win + x]; SJy += (int64_t)jv * Iyp[y * win + x];
                        }
                    const double a = gain_of(mode, N, vI, SJ, SJJ, g_lo, g_hi);
                    const int64_t cJx = N * SJx - SJ * SIx, cJy = N * SJy - SJ * SIy;        /* rule 5 */
                    b1 = (float)(((a * (double)cJx - (double)cIx) / (double)N) * 0x1p-20);
                    b2 = (float)(((a * (double)cJy - (double)cIy) / (double)N) * 0x1p-20);
                }
                const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
                qx += dx; qy += dy;
                nx = qx + half; ny = qy + half;
                if ((double)dx * dx + (double)dy * dy <= eps2) break;
                if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
                    nx -= dx * 0.5f; ny -= dy * 0.5f;
                    break;
                }
                pdx = dx; pdy = dy;
            }
            if (status[p] && l == 0) {
                const float ex = nx - half, ey = ny - half;
                const int iex = (int)floorf(ex), iey = (int)floorf(ey);
                if (iex < -win || iex >= J->w || iey < -win || iey >= J->h) { status[p] = 0; if (!geteig) err[p] = 0.f; continue; }
                if (geteig) continue;
                wts(ex - (float)iex, ey - (float)iey, iw);
                int64_t se = 0;
                if (!mode) {
                    for (int y = 0; y < win; ++y)
                        for (int x = 0; x < win; ++x) {
                            const int diff = interp(J, iey + y, iex + x, iw) - Ip[y * win + x];
                            se += diff < 0 ? -diff : diff;
                        }
                    err[p] = (float)se / (float)(32 * ww);
                } else {                                                         /* rule 6 */
                    int64_t SJ = 0, SJJ = 0;
                    for (int y = 0; y < win; ++y)
                        for (int x = 0; x < win; ++x) {
                            const int jv = interp(J, iey + y, iex + x, iw);
                            Jp[y * win + x] = (int16_t)jv;
                            SJ += jv; SJJ += (int64_t)jv * jv;
                        }
                    const int64_t a12 = (int64_t)llrint(gain_of(mode, N, vI, SJ, SJJ, g_lo, g_hi) * 4096);
                    for (int k = 0; k < ww; ++k) {
                        const int64_t r = a12 * (N * Jp[k] - SJ) - 4096 * (N * Ip[k] - SI);
                        se += r < 0 ? -r : r;
                    }
                    err[p] = (float)((double)se / (4096.0 * N * 32 * N));
                }
            }
        }
        next_pts[2 * p] = nx; next_pts[2 * p + 1] = ny;
    }
    free(Ip); free(Ixp); free(Iyp); free(Jp);
    return 0;
}
