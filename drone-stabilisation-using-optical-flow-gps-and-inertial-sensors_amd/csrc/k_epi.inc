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
__device__ __forceinline__ bool epi_usable(const epi_cfg &ec, const double *nrm, double d, double scaling)
{
    const double ne = nrm[0] * ec.e[0] + nrm[1] * ec.e[1] + nrm[2] * ec.e[2];
    return isfinite(d) && d != 0.0 && isfinite(scaling) && scaling != 0.0 && isfinite(ne) && ne != 0.0 && ec.e[2] != 0.0;
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
    double A[3][3], ln[3], Vn[3][3], W[3][3]; sym3_from6(s + EPI_N, A);
    jacobi3(A, ln, Vn);
    if (!(isfinite(ln[0]) && ln[2] > 2.220446049250313e-16 * 3.0 * m * ln[0])) return false;
    const double is[3] = {1.0 / sqrt(ln[0]), 1.0 / sqrt(ln[1]), 1.0 / sqrt(ln[2])};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W[i][j] = Vn[i][0] * Vn[j][0] * is[0] + Vn[i][1] * Vn[j][1] * is[1] + Vn[i][2] * Vn[j][2] * is[2];
    double E[3][3], T[3][3], G[3][3]; sym3_from6(s + EPI_E, E);
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
    double Hm[3][3], P[3][3], T[3][3], G[3][3], lh[3], Vh[3][3]; sym3_from6(s + EPI_H, Hm);
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
        team_put<EPI_SUMS1>(part[vw], s);
    }
    team_barrier<NW>();
    if (threadIdx.x == 0) {
        double t[EPI_SUMS1], th[3];
        team_sums<EPI_SUMS1>(part, t);
        const bool go = epi_direction(t, usable, rec03, th, tnt, er);
        bc[0] = th[0]; bc[1] = th[1]; bc[2] = th[2]; bc[3] = go ? 1.0 : 0.0;
    }
    team_barrier<NW>();
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
            team_put<EPI_SUMS2>(part[vw], s);
        }
    }
    team_barrier<NW>();
    if (threadIdx.x == 0) {
        double tv[3] = {0.0, 0.0, 0.0}, o[2] = {1.0, 1.0};
        int flag = 1;
        if (go) {
            double t[EPI_SUMS2], th[3] = {t0, t1, t2};
            team_sums<EPI_SUMS2>(part, t);
            flag = epi_finish(t, ec, tnt, th, tv, o, er);
            er[10] = (double)flag;
            bc[7] = t[EPI_RSS];
        }
        bc[0] = tv[0]; bc[1] = tv[1]; bc[2] = tv[2]; bc[4] = flag == 0 ? 1.0 : 0.0; bc[5] = o[0]; bc[6] = o[1];
    }
    team_barrier<NW>();
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

// ------------------------------------------------------------------------------------------------ the three forms (k_second.inc)
// The robust weights are read only under OFK_EPI_W_ROBUST.  anchor is in the units of the points: of x and u at the stage entry, pixels
// scaled by the pair's `scaling` in the resident forms.  A stream step whose solve did not solve (record[15] == 0) is not attempted.
__device__ __forceinline__ const double *epi_weights(const epi_cfg &ec, const double *weights)
{
    return ec.wmode == OFK_EPI_W_ROBUST ? weights : nullptr;
}

__global__ __launch_bounds__(256) void k_epi_solve(const double *__restrict__ x, const double *__restrict__ u, const uint8_t *__restrict__ valid,
                                                   int n, const double *__restrict__ d, const double *__restrict__ nrm,
                                                   const double *__restrict__ omega, const double *__restrict__ t,
                                                   const double *__restrict__ weights, epi_cfg ec, double *__restrict__ out,
                                                   double *__restrict__ epi, double *__restrict__ pts)
{
    __shared__ double part[4][EPI_SUMS2];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    stage_problem q;
    stage_unpack(q, b, x, u, valid, n, d, nrm, omega, t, epi_weights(ec, weights), out);
    double v[3], rss;
    const bool rw = epi_core<4>(part, bc, n, n, q.nrm, q.om, q.d, q.rec03, epi_usable(ec, q.nrm, q.d, 1.0), ec.anchor, ec,
                                epi + (size_t)b * OFK_EPI_DOUBLES, pts + (size_t)b * n * 4, v, rss, q.pts);
    stage_write(q, rw, v, q.om, rss, out + (size_t)b * OFK_SOLVE_DOUBLES);
}

void ofk_launch_epi_solve(hipStream_t s, const ofk_stage_in &in, const double *weights, const ofk_epipolar *e, double *out, double *epi,
                          double *pts)
{
    hipLaunchKernelGGL(k_epi_solve, dim3(in.batch), dim3(256), 0, s, in.x, in.u, in.valid, in.n, in.d, in.nrm, in.omega, in.t, weights,
                       epi_make_cfg(e), out, epi, pts);
}

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
    resident_problem q;
    resident_unpack(q, b, prev_pts, next_pts, status, counts, pts_stride, sensors, nullptr, false, use_feas, feas_T, epi_weights(ec, weights),
                    records);
    double v[3], rss;
    const bool rw = epi_core<NW>(part, bc, q.n, pts_stride, q.nrm, q.om, q.d, q.rec03, epi_usable(ec, q.nrm, q.d, q.scaling),
                                 ec.anchor * q.scaling, ec, epi + (size_t)b * OFK_EPI_DOUBLES, pts + (size_t)b * pts_stride * 4, v, rss, q.pts);
    pairs_write(q, rw, v, q.om, rss, records + (size_t)b * OFK_RECORD_DOUBLES);
}

void ofk_launch_pairs_epi(hipStream_t s, const ofk_pairs_in &in, const double *weights, const ofk_epipolar *e, double *epi, double *pts)
{
    launch_pairs_form(s, in.batch, k_pairs_epi<1>, k_pairs_epi<4>, in.prev_pts, in.next_pts, in.status, in.counts, in.pts_stride, in.sensors,
                      in.use_feas, in.feas_T, weights, epi_make_cfg(e), in.records, epi, pts);
}

__global__ __launch_bounds__(256) void k_stream_epi(fuse_args g, const double *__restrict__ weights, epi_cfg ec, double *__restrict__ epi,
                                                    double *__restrict__ pts)
{
    __shared__ double part[4][EPI_SUMS2];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    resident_problem q;
    stream_unpack(q, b, g, epi_weights(ec, weights));
    double v[3], rss;
    const bool rw = epi_core<4>(part, bc, q.n, g.pts_stride, q.nrm, q.om, q.d, q.rec03, q.solved && epi_usable(ec, q.nrm, q.d, q.scaling),
                                ec.anchor * q.scaling, ec, epi + (size_t)b * OFK_EPI_DOUBLES, pts + (size_t)b * g.pts_stride * 4, v, rss, q.pts);
    stream_tail(g, q, b, rw, v, q.om, rss);
}

void ofk_launch_stream_epi(hipStream_t s, const ofk_stream_in &in, const double *weights, const ofk_epipolar *e, double *epi, double *pts)
{
    hipLaunchKernelGGL(k_stream_epi, dim3(in.batch), dim3(256), 0, s, make_fuse_args(in, nullptr, 0, 0.0), weights, epi_make_cfg(e), epi, pts);
}
