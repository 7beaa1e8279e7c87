// k_epi.inc — the epipolar solve (ofk.h: ofk_set_epipolar): velocity and per-point inverse depths over ground that is no plane.
// Included by k_estimate.hip, whose helpers (point_terms, pair_point, cross_p, wave_sum, jacobi3, lever_rotate, the Kalman recursions)
// it shares.  DESIGN.md, "epipolar solve", has the derivation.
//
// One team per problem behind whichever solve kernel ran, plain or robust: a single wave (NW = 1) or a 256-thread workgroup (NW = 4).
// With p = (x, y, 1), X = [p]x and the solve's q = (u, 0) + p x omega the flow equation is rho X v = X q, rho the point's inverse
// depth; c = p x q is orthogonal to v whatever rho is.  The first walk over the kept points sums
//   E = sum w c c^T                       6
//   N0 = sum w X D X^T, D = diag(1, 1, 0) 6: the covariance of c under unit flow noise
//   the count                             1
// and one lane takes t^ as the generalised eigenvector of (E, N0) for the smallest eigenvalue: W = N0^(-1/2) and the smallest
// eigenvector of W E W, both from jacobi3, t^ = W y / |W y|; it broadcasts t^ through LDS.  The second walk writes each point's row
// (kappa, r, |b|, flag) with a = (q - q_z p)_xy, b = (t_x - t_z x, t_y - t_z y), kappa = a.b / |b|^2, r = (a x b) / |b|, and sums
//   H = sum w c c^T / |b|^2               6
//   sum w r^2, sum w a.b                  2
//   over the anchor set: sum w kappa m, sum w m^2, sum w m^2 / |b|^2, the count, m = (n0.p) / d0      4
//   the counts of kappa <= 0 and of kappa >= 0                                                        2
//   sum w (c.t^)^2 = sum w (a x b)^2: lambda_1 as t^'s Rayleigh quotient, t^^T E t^ / t^^T N0 t^, from residuals - the eigenvalue the
//   decomposition returns carries a rounding floor of eps lambda_max, this one none                   1
// The same lane then fixes the sign and the scale and writes the record; every thread revisits the rows it wrote and turns kappa
// into rho = kappa / s (or zeroes the row where the record carries a flag).  All sums are added as the solve adds its own - four
// "virtual waves" take the points vw * 64 + lane + 256 k, each is reduced by the shuffle butterfly, the partial sums are added as
// (s0 + s1) + (s2 + s3) - so records and rows are the same bit for bit across forms, slice counts and overlap settings.  No atomics,
// no MFMA, vector stores only.
#define EPI_SUMS1 13
#define EPI_SUMS2 15
#define EPI_E 0
#define EPI_N 6
#define EPI_CNT 12
#define EPI_H 0
#define EPI_RSS 6
#define EPI_AB 7
#define EPI_AKM 8
#define EPI_AMM 9
#define EPI_AMB 10
#define EPI_ACNT 11
#define EPI_NLE 12
#define EPI_NGE 13
#define EPI_CT2 14

struct epi_cfg { double anchor, smax, e[3]; int amin, wmode; };

// Flag 1's rule on the inputs: range, scale and n0.e are finite and not 0, the beam leaves the image plane.
__device__ __forceinline__ bool epi_usable(double d, double scaling, double ne, double ez)
{
    return isfinite(d) && d != 0.0 && isfinite(scaling) && scaling != 0.0 && isfinite(ne) && ne != 0.0 && ez != 0.0;
}

// One lane, after the first walk: t^ from the 13 sums, and tnt = t^^T N0 t^.  er is written in full (flag 1); returns whether the second
// walk runs.
__device__ bool epi_direction(const double *s, bool usable, const double *rec03, double *t, double &tnt, double *er)
{
    for (int k = 0; k < OFK_EPI_DOUBLES; ++k) er[k] = 0.0;
    for (int k = 0; k < 4; ++k) er[6 + k] = rec03[k];
    er[10] = 1.0; er[11] = s[EPI_CNT];
    t[0] = t[1] = t[2] = 0.0; tnt = 0.0;
    bool fin = usable;
    for (int k = 0; k < EPI_SUMS1; ++k) fin = fin && isfinite(s[k]);
    const double m = s[EPI_CNT];
    if (!fin || !(m >= 3.0)) return false;
    double A[3][3] = {{s[EPI_N], s[EPI_N + 1], s[EPI_N + 2]}, {s[EPI_N + 1], s[EPI_N + 3], s[EPI_N + 4]}, {s[EPI_N + 2], s[EPI_N + 4], s[EPI_N + 5]}};
    double ln[3], Vn[3][3], W[3][3];
    jacobi3(A, ln, Vn);
    if (!(isfinite(ln[0]) && ln[2] > 2.220446049250313e-16 * 3.0 * m * ln[0])) return false;
    const double is[3] = {1.0 / sqrt(ln[0]), 1.0 / sqrt(ln[1]), 1.0 / sqrt(ln[2])};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W[i][j] = Vn[i][0] * Vn[j][0] * is[0] + Vn[i][1] * Vn[j][1] * is[1] + Vn[i][2] * Vn[j][2] * is[2];
    const double E[3][3] = {{s[EPI_E], s[EPI_E + 1], s[EPI_E + 2]}, {s[EPI_E + 1], s[EPI_E + 3], s[EPI_E + 4]}, {s[EPI_E + 2], s[EPI_E + 4], s[EPI_E + 5]}};
    double T[3][3], G[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T[i][j] = E[i][0] * W[0][j] + E[i][1] * W[1][j] + E[i][2] * W[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) G[i][j] = G[j][i] = W[i][0] * T[0][j] + W[i][1] * T[1][j] + W[i][2] * T[2][j];
    double lg[3], Y[3][3];
    jacobi3(G, lg, Y);
    double th[3], nn = 0.0;
    for (int i = 0; i < 3; ++i) { th[i] = W[i][0] * Y[0][2] + W[i][1] * Y[1][2] + W[i][2] * Y[2][2]; nn += th[i] * th[i]; }
    nn = sqrt(nn);
    if (!(isfinite(lg[0]) && isfinite(lg[2]) && isfinite(nn) && nn > 0.0)) return false;
    for (int i = 0; i < 3; ++i) t[i] = th[i] / nn;
    tnt = 1.0 / (nn * nn);                                       // W N0 W = I and |y| = 1
    er[14] = lg[0]; er[15] = lg[1];
    return true;
}

// The same lane, after the second walk: sign, gate, scale and the record.  t holds t^ on entry and the signed t^ on return; v = s t^.
// Returns the flag; out[0] = kappa's divisor (s with t^'s first sign), out[1] = the sign.
__device__ int epi_finish(const double *s, const epi_cfg &ec, double tnt, double *t, double *v, double *out, double *er)
{
    v[0] = v[1] = v[2] = 0.0; out[0] = out[1] = 1.0;
    bool fin = true;
    for (int k = 0; k < EPI_SUMS2; ++k) fin = fin && isfinite(s[k]);
    if (!fin) { er[14] = er[15] = 0.0; return 1; }
    const double sgn = s[EPI_AB] >= 0.0 ? 1.0 : -1.0, m = er[11], l1 = s[EPI_CT2] / tnt, sig2 = l1 * m / (m - 2.0);
    er[4] = sqrt(sig2); er[16] = l1;
    for (int k = 0; k < 3; ++k) { t[k] *= sgn; er[k] = t[k]; }
    er[5] = s[EPI_RSS]; er[12] = s[EPI_ACNT]; er[13] = sgn > 0.0 ? s[EPI_NLE] : s[EPI_NGE];
    const double Hm[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    double P[3][3], T[3][3], G[3][3], lh[3], Vh[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) P[i][j] = (i == j ? 1.0 : 0.0) - t[i] * t[j];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T[i][j] = Hm[i][0] * P[0][j] + Hm[i][1] * P[1][j] + Hm[i][2] * P[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) G[i][j] = G[j][i] = P[i][0] * T[0][j] + P[i][1] * T[1][j] + P[i][2] * T[2][j];
    jacobi3(G, lh, Vh);
    if (!(lh[1] > 0.0 && isfinite(lh[0]))) { er[17] = INFINITY; return 2; }
    double Ct[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Ct[i][j] = sig2 * (Vh[i][0] * Vh[j][0] / lh[0] + Vh[i][1] * Vh[j][1] / lh[1]);
    const double pred = sqrt(Ct[0][0] + Ct[1][1] + Ct[2][2]);
    er[17] = pred;
    if (!(pred <= ec.smax)) return 2;
    er[18] = Ct[0][0]; er[19] = Ct[0][1]; er[20] = Ct[0][2]; er[21] = Ct[1][1]; er[22] = Ct[1][2]; er[23] = Ct[2][2];
    if (s[EPI_ACNT] < (double)ec.amin) return 3;
    const double sraw = s[EPI_AKM] / s[EPI_AMM], sc = sgn * sraw;
    if (!(isfinite(sc) && sc > 0.0)) return 3;
    const double vs = sig2 * s[EPI_AMB] / (s[EPI_AMM] * s[EPI_AMM]);
    er[3] = sc; er[24] = vs;
    for (int k = 0; k < 3; ++k) v[k] = sc * t[k];
    int o = 25;
    for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) er[o++] = sc * sc * Ct[i][j] + vs * t[i] * t[j];
    out[0] = sraw; out[1] = sgn;
    return 0;
}

// The two walks and the rows' last visit: terms(i, x, y, ux, uy, w) -> point i enters.  Returns, in every thread, whether the record is to
// be rewritten; then v and rss hold v = s t^ and sum w r^2.  rows: the problem's [stride][4]; er: its record, written by thread 0.
// anchor in the units of the points.  bc: 8 doubles of LDS.
template <int NW, class Terms>
__device__ __forceinline__ bool epi_core(double (*part)[EPI_SUMS2], double *bc, int n, int stride, const double *nrm, const double *om, double d,
                                         const double *rec03, bool usable, double anchor, const epi_cfg &ec, double *er, double *rows,
                                         double *v, double &rss, Terms terms)
{
    const int lane = threadIdx.x & 63, wave = NW == 1 ? 0 : (int)(threadIdx.x >> 6);
    double tnt = 0.0;                                            // thread 0's, from the first finish to the second
#pragma unroll 1
    for (int vw = wave; vw < 4; vw += NW) {
        double s[EPI_SUMS1];
#pragma unroll
        for (int k = 0; k < EPI_SUMS1; ++k) s[k] = 0.0;
#pragma unroll 1
        for (int i = vw * 64 + lane; i < n; i += 256) {
            double x, y, ux, uy, w, q0, q1, q2, a, b, c0, c1, c2;
            if (!terms(i, x, y, ux, uy, w)) continue;
            point_terms(OFK_SOLVE_NODE, x, y, ux, uy, nrm, om, d, 1.0, q0, q1, q2, a, b);
            cross_p(x, y, q0, q1, q2, c0, c1, c2);
            s[EPI_E + 0] += w * (c0 * c0); s[EPI_E + 1] += w * (c0 * c1); s[EPI_E + 2] += w * (c0 * c2);
            s[EPI_E + 3] += w * (c1 * c1); s[EPI_E + 4] += w * (c1 * c2); s[EPI_E + 5] += w * (c2 * c2);
            s[EPI_N + 0] += w; s[EPI_N + 1] += w * 0.0; s[EPI_N + 2] += w * (-x);     // X D X^T's xy entry is 0: the slot keeps the layout of six
            s[EPI_N + 3] += w; s[EPI_N + 4] += w * (-y); s[EPI_N + 5] += w * (x * x + y * y);
            s[EPI_CNT] += 1.0;
        }
#pragma unroll
        for (int k = 0; k < EPI_SUMS1; ++k) { const double t = wave_sum(s[k]); if (lane == 0) part[vw][k] = t; }
    }
    if (NW == 1) __builtin_amdgcn_wave_barrier(); else __syncthreads();
    if (threadIdx.x == 0) {
        double t[EPI_SUMS1], th[3];
        for (int k = 0; k < EPI_SUMS1; ++k) t[k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
        const bool go = epi_direction(t, usable, rec03, th, tnt, er);
        bc[0] = th[0]; bc[1] = th[1]; bc[2] = th[2]; bc[3] = go ? 1.0 : 0.0;
    }
    if (NW == 1) __builtin_amdgcn_wave_barrier(); else __syncthreads();
    const double t0 = bc[0], t1 = bc[1], t2 = bc[2];
    const bool go = bc[3] != 0.0;
    const double pe0 = ec.e[0] / ec.e[2], pe1 = ec.e[1] / ec.e[2], an2 = anchor * anchor;
    if (go) {
#pragma unroll 1
        for (int vw = wave; vw < 4; vw += NW) {
            double s[EPI_SUMS2];
#pragma unroll
            for (int k = 0; k < EPI_SUMS2; ++k) s[k] = 0.0;
#pragma unroll 1
            for (int i = vw * 64 + lane; i < n; i += 256) {
                double x, y, ux, uy, w, q0, q1, q2, a, b, c0, c1, c2;
                double *row = rows + (size_t)i * 4;
                if (!terms(i, x, y, ux, uy, w)) { row[0] = 0.0; row[1] = 0.0; row[2] = 0.0; row[3] = 1.0; continue; }
                point_terms(OFK_SOLVE_NODE, x, y, ux, uy, nrm, om, d, 1.0, q0, q1, q2, a, b);
                cross_p(x, y, q0, q1, q2, c0, c1, c2);
                const double a0 = q0 - q2 * x, a1 = q1 - q2 * y, b0 = t0 - t2 * x, b1 = t1 - t2 * y;
                const double bb = b0 * b0 + b1 * b1, ab = a0 * b0 + a1 * b1, nb = sqrt(bb);
                const double cr = a0 * b1 - a1 * b0, kap = ab / bb, r = cr / nb, wb = w / bb;
                s[EPI_H + 0] += wb * (c0 * c0); s[EPI_H + 1] += wb * (c0 * c1); s[EPI_H + 2] += wb * (c0 * c2);
                s[EPI_H + 3] += wb * (c1 * c1); s[EPI_H + 4] += wb * (c1 * c2); s[EPI_H + 5] += wb * (c2 * c2);
                s[EPI_RSS] += w * (r * r); s[EPI_AB] += w * ab; s[EPI_CT2] += w * (cr * cr);
                const double ex = x - pe0, ey = y - pe1;
                if (ex * ex + ey * ey <= an2) {
                    const double m = (nrm[0] * x + nrm[1] * y + nrm[2]) / d;
                    s[EPI_AKM] += w * (kap * m); s[EPI_AMM] += w * (m * m); s[EPI_AMB] += wb * (m * m); s[EPI_ACNT] += 1.0;
                }
                s[EPI_NLE] += kap <= 0.0 ? 1.0 : 0.0; s[EPI_NGE] += kap >= 0.0 ? 1.0 : 0.0;
                row[0] = kap; row[1] = r; row[2] = nb; row[3] = 0.0;
            }
#pragma unroll
            for (int k = 0; k < EPI_SUMS2; ++k) { const double t = wave_sum(s[k]); if (lane == 0) part[vw][k] = t; }
        }
    }
    if (NW == 1) __builtin_amdgcn_wave_barrier(); else __syncthreads();
    if (threadIdx.x == 0) {
        double tv[3] = {0.0, 0.0, 0.0}, o[2] = {1.0, 1.0};
        int flag = 1;
        if (go) {
            double t[EPI_SUMS2], th[3] = {t0, t1, t2};
            for (int k = 0; k < EPI_SUMS2; ++k) t[k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
            flag = epi_finish(t, ec, tnt, th, tv, o, er);
            er[10] = (double)flag;
            bc[7] = t[EPI_RSS];
        }
        bc[0] = tv[0]; bc[1] = tv[1]; bc[2] = tv[2]; bc[4] = flag == 0 ? 1.0 : 0.0; bc[5] = o[0]; bc[6] = o[1];
    }
    if (NW == 1) __builtin_amdgcn_wave_barrier(); else __syncthreads();
    const bool rw = bc[4] != 0.0;
    const double sraw = bc[5], sgn = bc[6];
    for (int k = 0; k < 3; ++k) v[k] = bc[k];
    rss = rw ? bc[7] : 0.0;
    // every thread revisits the rows it wrote itself (i = its lane + 64 k, or its thread + 256 k)
#pragma unroll 1
    for (int i = threadIdx.x; i < stride; i += 64 * NW) {
        double *row = rows + (size_t)i * 4;
        if (!rw) { row[0] = 0.0; row[1] = 0.0; row[2] = 0.0; row[3] = 0.0; }
        else if (i >= n) { row[0] = 0.0; row[1] = 0.0; row[2] = 0.0; row[3] = 1.0; }
        else if (row[3] == 0.0) {
            const double kap = row[0];
            row[0] = kap / sraw; row[1] = sgn * row[1]; row[3] = sgn * kap <= 0.0 ? 2.0 : 0.0;
        }
    }
    return rw;
}

static epi_cfg epi_make_cfg(const ofk_epipolar *e)
{
    epi_cfg ec;
    ec.anchor = e->anchor; ec.smax = e->sigma_max; ec.amin = e->anchor_min; ec.wmode = e->weights;
    const double nn = sqrt(e->beam[0] * e->beam[0] + e->beam[1] * e->beam[1] + e->beam[2] * e->beam[2]);
    for (int k = 0; k < 3; ++k) ec.e[k] = e->beam[k] / nn;
    return ec;
}

// ------------------------------------------------------------------------------------------------ stage entry (host buffers)
// Behind k_solve / k_solve_robust: out holds the solve's eight doubles (v less omega x t when t is given) and is rewritten in place,
// weights (nullable) the robust solve's, read only under OFK_EPI_W_ROBUST.  anchor is in the units of x and u.
__global__ __launch_bounds__(256) void k_epi_solve(const double *__restrict__ x, const double *__restrict__ u, const uint8_t *__restrict__ valid,
                                                   int n, const double *__restrict__ d, const double *__restrict__ nrm,
                                                   const double *__restrict__ omega, const double *__restrict__ t,
                                                   const double *__restrict__ weights, epi_cfg ec, double *__restrict__ out,
                                                   double *__restrict__ epi, double *__restrict__ pts)
{
    __shared__ double part[4][EPI_SUMS2];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    const double *xb = x + (size_t)b * n * 2, *ub = u + (size_t)b * n * 2;
    const uint8_t *vb = valid ? valid + (size_t)b * n : nullptr;
    const double *wb = weights && ec.wmode == OFK_EPI_W_ROBUST ? weights + (size_t)b * n : nullptr;
    const double nb[3] = {nrm[3 * b], nrm[3 * b + 1], nrm[3 * b + 2]}, ob[3] = {omega[3 * b], omega[3 * b + 1], omega[3 * b + 2]};
    const double db = d[b];
    double *o = out + (size_t)b * OFK_SOLVE_DOUBLES;
    const double rec03[4] = {o[0], o[1], o[2], o[3]};
    const double ne = nb[0] * ec.e[0] + nb[1] * ec.e[1] + nb[2] * ec.e[2];
    double v[3], rss;
    const bool rw = epi_core<4>(part, bc, n, n, nb, ob, db, rec03, epi_usable(db, 1.0, ne, ec.e[2]), ec.anchor, ec,
                                epi + (size_t)b * OFK_EPI_DOUBLES, pts + (size_t)b * n * 4, v, rss,
                                [&](int i, double &px, double &py, double &ux, double &uy, double &w) {
        if (vb && !vb[i]) return false;
        w = wb ? wb[i] : 1.0;
        if (!(w > 0.0)) return false;
        px = xb[2 * i]; py = xb[2 * i + 1]; ux = ub[2 * i]; uy = ub[2 * i + 1];
        return true;
    });
    if (rw && threadIdx.x == 0) {
        if (t) sub_cross(v, ob, t + 3 * b, o);
        else { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }
        o[3] = rss;
    }
}

void ofk_launch_epi_solve(hipStream_t s, const double *x, const double *u, const uint8_t *valid, int batch, int n, const double *d,
                          const double *nrm, const double *omega, const double *t, const double *weights, const ofk_epipolar *e,
                          double *out, double *epi, double *pts)
{
    hipLaunchKernelGGL(k_epi_solve, dim3(batch), dim3(256), 0, s, x, u, valid, n, d, nrm, omega, t, weights, epi_make_cfg(e), out, epi, pts);
}

// ------------------------------------------------------------------------------------------------ frame pairs / plain stream step
// Behind k_pairs_solve[_wg] / k_pairs_robust: the same inputs, the pair's record (rewritten in place) and (robust) weight row.
// anchor is pixels: the points are scaled by the pair's `scaling`, so is it.
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_pairs_epi(const float *__restrict__ prev_pts, const float *__restrict__ next_pts,
                                                       const uint8_t *__restrict__ status, const int *__restrict__ counts, int pts_stride,
                                                       const double *__restrict__ sensors, int use_feas, double feas_T,
                                                       const double *__restrict__ weights, epi_cfg ec, double *__restrict__ records,
                                                       double *__restrict__ epi, double *__restrict__ pts)
{
    __shared__ double part[4][EPI_SUMS2];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    const double *sn = sensors + (size_t)b * OFK_SENSOR_DOUBLES;
    const double d = sn[0], nrm[3] = {sn[1], sn[2], sn[3]}, om[3] = {sn[4], sn[5], sn[6]};
    const double scaling = sn[19], cx = sn[20], cy = sn[21], vp[3] = {sn[22], sn[23], sn[24]};
    const int n = min(max(counts[b], 0), pts_stride);
    const float *pp = prev_pts + (size_t)b * pts_stride * 2, *np_ = next_pts + (size_t)b * pts_stride * 2;
    const uint8_t *st = status + (size_t)b * pts_stride;
    const double *wrow = weights && ec.wmode == OFK_EPI_W_ROBUST ? weights + (size_t)b * pts_stride : nullptr;
    double *r = records + (size_t)b * OFK_RECORD_DOUBLES;
    const double rec03[4] = {r[0], r[1], r[2], r[3]};
    const double ne = nrm[0] * ec.e[0] + nrm[1] * ec.e[1] + nrm[2] * ec.e[2];
    double v[3], rss;
    const bool rw = epi_core<NW>(part, bc, n, pts_stride, nrm, om, d, rec03, epi_usable(d, scaling, ne, ec.e[2]),
                                 ec.anchor * scaling, ec, epi + (size_t)b * OFK_EPI_DOUBLES, pts + (size_t)b * pts_stride * 4, v, rss,
                                 [&](int i, double &x, double &y, double &ux, double &uy, double &w) {
        if (!st[i]) return false;
        w = wrow ? wrow[i] : 1.0;
        if (!(w > 0.0)) return false;
        return pair_point(pp, np_, i, cx, cy, scaling, use_feas, feas_T, nrm, vp, d, x, y, ux, uy);
    });
    if (rw && threadIdx.x == 0) {
        double vu[3];
        lever_rotate(v, om, sn + 16, sn + 7, vu);
        r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = rss; r[8] = vu[0]; r[9] = vu[1]; r[10] = vu[2];
    }
}

void ofk_launch_pairs_epi(hipStream_t s, const float *prev_pts, const float *next_pts, const uint8_t *status, const int *counts,
                          int pts_stride, const double *sensors, int use_feas, double feas_T, const double *weights, const ofk_epipolar *e,
                          double *records, double *epi, double *pts, int batch)
{
    const epi_cfg ec = epi_make_cfg(e);
    // ofk_launch_pairs_solve's rule and reason
    if (batch >= 128)
        hipLaunchKernelGGL(k_pairs_epi<1>, dim3(batch), dim3(64), 0, s, prev_pts, next_pts, status, counts, pts_stride, sensors, use_feas, feas_T,
                           weights, ec, records, epi, pts);
    else
        hipLaunchKernelGGL(k_pairs_epi<4>, dim3(batch), dim3(256), 0, s, prev_pts, next_pts, status, counts, pts_stride, sensors, use_feas, feas_T,
                           weights, ec, records, epi, pts);
}

// ------------------------------------------------------------------------------------------------ fused stream step
// Behind k_stream_fuse / k_stream_fuse_robust, which with the setting on leave the filter at its prediction (fuse_args.defer): `status`
// holds the keep flags by now, so the set is status (and, under OFK_EPI_W_ROBUST, w > 0).  A step whose solve did not solve
// (record[15] == 0) is not attempted.  The correct runs here with the epipolar v / v_uav (the solve's own where the record was left
// alone), fused[0..7] is rewritten and vel_overwrite is repeated with the epipolar v_uav.
__global__ __launch_bounds__(256) void k_stream_epi(fuse_args g, const double *__restrict__ weights, epi_cfg ec, double *__restrict__ epi,
                                                    double *__restrict__ pts)
{
    __shared__ double part[4][EPI_SUMS2];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    const double *sn = g.sensors + (size_t)b * OFK_SENSOR_DOUBLES;
    const double d = sn[0], scaling = sn[19], cx = sn[20], cy = sn[21];
    double *ist = g.f.use_imu && g.imu_state ? g.imu_state + (size_t)b * OFK_IMU_STATE : nullptr;
    double nrm[3], om[3];
    for (int k = 0; k < 3; ++k) { nrm[k] = ist ? ist[15 + k] : sn[1 + k]; om[k] = ist ? ist[18 + k] : sn[4 + k]; }
    const int n = min(max(g.counts[b], 0), g.pts_stride);
    const float *pp = g.prev_pts + (size_t)b * g.pts_stride * 2, *np_ = g.next_pts + (size_t)b * g.pts_stride * 2;
    const uint8_t *st = g.status + (size_t)b * g.pts_stride;
    const double *wrow = weights && ec.wmode == OFK_EPI_W_ROBUST ? weights + (size_t)b * g.pts_stride : nullptr;
    double *r = g.records + (size_t)b * OFK_RECORD_DOUBLES;
    const double rec03[4] = {r[0], r[1], r[2], r[3]};
    const bool solved = r[15] != 0.0;
    const double ne = nrm[0] * ec.e[0] + nrm[1] * ec.e[1] + nrm[2] * ec.e[2];
    double v[3], rss;
    const bool rw = epi_core<4>(part, bc, n, g.pts_stride, nrm, om, d, rec03,
                                solved && epi_usable(d, scaling, ne, ec.e[2]), ec.anchor * scaling, ec,
                                epi + (size_t)b * OFK_EPI_DOUBLES, pts + (size_t)b * g.pts_stride * 4, v, rss,
                                [&](int i, double &x, double &y, double &ux, double &uy, double &w) {
        if (!st[i]) return false;
        w = wrow ? wrow[i] : 1.0;
        if (!(w > 0.0)) return false;
        return pair_point(pp, np_, i, cx, cy, scaling, 0, 0.0, nrm, rec03, d, x, y, ux, uy);  // fuse_terms' x, y, u of OFK_FLOW_LK
    });
    if (threadIdx.x == 0) {
        double vu[3] = {r[8], r[9], r[10]};
        if (rw) {
            lever_rotate(v, om, sn + 16, ist ? ist + 6 : sn + 7, vu);
            r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = rss; r[8] = vu[0]; r[9] = vu[1]; r[10] = vu[2];
        }
        double *fu = g.fused + (size_t)b * 8;
        if (g.f.filter && g.defer) {
            double kx[KF_MAX], kP[KF_MAX][KF_MAX];
            kf_load(g.ns, b, g.kf_x, g.kf_P, kx, kP);
            if (solved) {
                double z[KF_MAX] = {0, 0, 0, 0, 0, 0};
                for (int k = 0; k < 3; ++k) z[k] = g.f.z_sign * r[(g.f.z_source ? 8 : 0) + k];
                for (int k = 3; k < g.nm; ++k) z[k] = sn[22 + (k - 3)];
                kf_correct_dev(g.ns, g.nm, g.H, g.Rm, z, kx, kP);
                kf_store(g.ns, b, kx, kP, g.kf_x, g.kf_P);
            }
            double tr = 0.0;
            for (int i = 0; i < g.ns; ++i) tr += kP[i][i];
            for (int k = 0; k < 6; ++k) fu[k] = k < g.ns ? kx[k] : 0.0;
            fu[6] = tr; fu[7] = solved ? 1.0 : 0.0;
        } else if (!g.f.filter && rw) {
            fu[0] = vu[0]; fu[1] = vu[1]; fu[2] = vu[2];
        }
        if (g.f.vel_overwrite && solved && ist && rw) { ist[0] = vu[0]; ist[1] = vu[1]; ist[2] = vu[2]; }   // node:261
    }
}

void ofk_launch_stream_epi(hipStream_t s, const float *prev_pts, const float *next_pts, uint8_t *status, const int *counts, int pts_stride,
                           const double *sensors, double *imu_state, int ns, int nm, int nc, const double *kf_mats, double *kf_x, double *kf_P,
                           const ofk_fusion *f, int variant, double *records, double *fused, const double *weights, const ofk_epipolar *e,
                           double *epi, double *pts, int batch, int defer)
{
    fuse_args g;
    g.prev_pts = prev_pts; g.next_pts = next_pts; g.status = status; g.counts = counts; g.pts_stride = pts_stride; g.sensors = sensors;
    g.imu_state = imu_state; g.imu_dv = nullptr; g.ns = ns; g.nm = nm; g.nc = nc;
    g.F = kf_mats; g.Bm = kf_mats + 36; g.H = kf_mats + 72; g.Q = kf_mats + 108; g.Rm = kf_mats + 144; g.kf_x = kf_x; g.kf_P = kf_P;
    g.f = *f; g.variant = variant; g.use_feas = 0; g.feas_T = 0.0; g.records = records; g.fused = fused; g.defer = defer;
    hipLaunchKernelGGL(k_stream_epi, dim3(batch), dim3(256), 0, s, g, weights, epi_make_cfg(e), epi, pts);
}
