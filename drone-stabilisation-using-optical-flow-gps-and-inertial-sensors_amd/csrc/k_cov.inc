// k_cov.inc — the velocity covariance (ofk.h: ofk_set_cov): first-order error propagation through the velocity solve, and the filter
// correct that uses it.  Included by k_estimate.hip, whose helpers (point_terms, pair_point, fuse_terms, wave_sum, jacobi3,
// eig_inverse3, the Kalman recursions) it shares.  DESIGN.md, "velocity covariance", has the derivation.
//
// One team per problem behind whichever solve kernel ran, plain or robust: a single wave (NW = 1, beside the response kernel / LK of
// large batches) or a 256-thread workgroup (NW = 4).  The team reads v from the record, walks the kept points once and sums, with
// p = (x, y, 1), N = |p|^2 I - p p^T, q, a = sA, b = sB the solve's per-point terms and w the final robust weight (or 1):
//   M   = sum w a^2 N                                       in the solve's own order, so jacobi3 sees the solve's bits
//   Sf  = sum_k e e^T, e = w a b N e_k                      flow u_k (2 per point)
//   Sp  = sum_k e e^T, e = n_k h + w [a b (dN q + N (e_k x omega)) - a^2 dN v]      position x_k (2 per point, u held fixed)
//   Eg_k = sum w a b |p|^2 (p x e_k)                        gyro omega_k
//   Ed  = sum w a db N q                                    range d: db = 1 / (n.p) (NODE), 1 (SIM)
//   En_k = sum p_k h                                        normal n_k
// where h = w [(A b + a B) N q - 2 a A N v] is the response to a unit change of n.p: (A, B) = (0, -d / (n.p)^2) (NODE), (1, 0) (SIM),
// and dN r = 2 p_k r - e_k (p.r) - p r_k.  That is 40 sums.  Both forms add them as the solve adds its own - four "virtual waves" take
// the points vw * 64 + lane + 256 k, each is reduced by the shuffle butterfly, the partial sums are added as (s0 + s1) + (s2 + s3) -
// so the records are the same bit for bit across forms, slice counts and overlap settings.  One lane applies M^-1 from the
// eigen-decomposition and writes the record.  No atomics, no MFMA, vector stores only.
#define COV_SUMS 40
#define COV_M 0
#define COV_CNT 6
#define COV_SF 7
#define COV_SP 13
#define COV_EG 19
#define COV_ED 28
#define COV_EN 31

struct cov_cfg { int mode; double sf, sp, sd, so[3], sn, soff; int omega_from_imu, filter_r; double r_floor, nis_max; };

__device__ __forceinline__ void cov_outer(double *s, const double *e)
{
    s[0] += e[0] * e[0]; s[1] += e[0] * e[1]; s[2] += e[0] * e[2]; s[3] += e[1] * e[1]; s[4] += e[1] * e[2]; s[5] += e[2] * e[2];
}

// One kept point's contributions to the 40 sums.
__device__ __forceinline__ void cov_point(double *s, int variant, double x, double y, double ux, double uy, double w, const double *nrm,
                                          const double *om, double d, const double *v)
{
    double q0, q1, q2, a, b;
    point_terms(variant, x, y, ux, uy, nrm, om, d, 1.0, q0, q1, q2, a, b);
    const double pp = x * x + y * y + 1.0, sa2 = a * a * w;
    s[COV_M + 0] += sa2 * (pp - x * x); s[COV_M + 1] += sa2 * (-x * y); s[COV_M + 2] += sa2 * (-x);
    s[COV_M + 3] += sa2 * (pp - y * y); s[COV_M + 4] += sa2 * (-y);     s[COV_M + 5] += sa2 * (pp - 1.0);
    s[COV_CNT] += 1.0;
    const double p[3] = {x, y, 1.0}, q[3] = {q0, q1, q2};
    const double pq = x * q0 + y * q1 + q2, pv = x * v[0] + y * v[1] + v[2];
    const double Nq[3] = {pp * q0 - x * pq, pp * q1 - y * pq, pp * q2 - pq}, Nv[3] = {pp * v[0] - x * pv, pp * v[1] - y * pv, pp * v[2] - pv};
    const double wab = w * a * b, wa2 = w * a * a;
    // flow
    const double f0[3] = {wab * (pp - x * x), wab * (-x * y), wab * (-x)}, f1[3] = {wab * (-x * y), wab * (pp - y * y), wab * (-y)};
    cov_outer(s + COV_SF, f0); cov_outer(s + COV_SF, f1);
    // gyro: N (p x e_k) = |p|^2 (p x e_k)
    const double g = wab * pp;
    s[COV_EG + 1] += g;      s[COV_EG + 2] += g * (-y);
    s[COV_EG + 3] += -g;     s[COV_EG + 5] += g * x;
    s[COV_EG + 6] += g * y;  s[COV_EG + 7] += g * (-x);
    // range, and the response h to n.p
    const double ndp = nrm[0] * x + nrm[1] * y + nrm[2];
    double h[3];
    if (variant == OFK_SOLVE_SIM) {
        const double wa = w * a;
#pragma unroll
        for (int j = 0; j < 3; ++j) { s[COV_ED + j] += wa * Nq[j]; h[j] = w * (b * Nq[j] - 2.0 * a * Nv[j]); }
    } else {
        const double wa = w * a, dbd = 1.0 / ndp, B = -d / (ndp * ndp);
#pragma unroll
        for (int j = 0; j < 3; ++j) { s[COV_ED + j] += wa * dbd * Nq[j]; h[j] = wa * B * Nq[j]; }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) s[COV_EN + 3 * k + j] += p[k] * h[j];
    // position
    const double dq[2][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double pdq = x * dq[k][0] + y * dq[k][1] + dq[k][2];
        double e[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double ek = j == k ? 1.0 : 0.0;
            const double dNq = 2.0 * p[k] * q[j] - ek * pq - p[j] * q[k], dNv = 2.0 * p[k] * v[j] - ek * pv - p[j] * v[k];
            const double Ndq = pp * dq[k][j] - p[j] * pdq;
            e[j] = nrm[k] * h[j] + (wab * (dNq + Ndq) - wa2 * dNv);
        }
        cov_outer(s + COV_SP, e);
    }
}

// The walk and the reduction: terms(i, x, y, ux, uy, w) -> point i enters (the set the solve used).  The sums end in part[0], for
// thread 0 alone (it wrote them: no barrier behind this).
template <int NW, class Terms>
__device__ __forceinline__ void cov_core(double (*part)[COV_SUMS], int n, int variant, const double *nrm, const double *om, double d,
                                         const double *v, Terms terms)
{
    const int lane = threadIdx.x & 63, wave = NW == 1 ? 0 : (int)(threadIdx.x >> 6);
#pragma unroll 1
    for (int vw = wave; vw < 4; vw += NW) {
        double s[COV_SUMS];
#pragma unroll
        for (int k = 0; k < COV_SUMS; ++k) s[k] = 0.0;
#pragma unroll 1
        for (int i = vw * 64 + lane; i < n; i += 256) {
            double x, y, ux, uy, w;
            if (terms(i, x, y, ux, uy, w)) cov_point(s, variant, x, y, ux, uy, w, nrm, om, d, v);
        }
        team_put<COV_SUMS>(part[vw], s);
    }
    team_barrier<NW>();
    if (threadIdx.x == 0) team_sums<COV_SUMS>(part, part[0]);
}

__device__ __forceinline__ void cov_void(double *o)
{
    for (int k = 0; k < OFK_COV_DOUBLES; ++k) o[k] = 0.0;
    o[13] = 1.0;
}

// A (symmetric, upper triangle s6) sandwiched: Mi S Mi, scaled; Mi full 3x3.
__device__ void cov_sandwich(const double Mi[3][3], const double *s6, double scale, double C[3][3])
{
    double S[3][3], T[3][3]; sym3_from6(s6, S);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T[i][j] = Mi[i][0] * S[0][j] + Mi[i][1] * S[1][j] + Mi[i][2] * S[2][j];
    for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) C[i][j] = C[j][i] = scale * (T[i][0] * Mi[j][0] + T[i][1] * Mi[j][1] + T[i][2] * Mi[j][2]);
}

// One lane: the record from the sums.  sf, sp: sigma_flow / sigma_pos in the units of the points; ovar: the gyro's variances;
// t: lever arm (NULL: none, C_uav = C_v); R: rotation (NULL: I); rss, rank: the solve's own.  Slots 14, 15 (NIS, gated) are zeroed.
__device__ void cov_finish(const double *s, const cov_cfg &cc, double sf, double sp, const double *ovar, const double *om, const double *t,
                           const double *R, double rss, double rank, bool usable, double *o)
{
    const double m = s[COV_CNT];
    if (!usable || !(rank >= 3.0) || !(m > 0.0) || (cc.mode == OFK_COV_RESIDUAL && !(2.0 * m > 3.0))) { cov_void(o); return; }
    double A[3][3], lam[3], V[3][3], Mi[3][3]; sym3_from6(s, A);
    jacobi3(A, lam, V);
    if (!(lam[2] > 0.0)) { cov_void(o); return; }
    eig_inverse3(lam, V, Mi);
    const double s2 = 2.0 * m > 3.0 ? rss / (2.0 * m - 3.0) : 0.0;
    double Cf[3][3], Cx[3][3];
    if (cc.mode == OFK_COV_RESIDUAL) {
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { Cf[i][j] = s2 * Mi[i][j]; Cx[i][j] = 0.0; }
    } else {
        cov_sandwich(Mi, s + COV_SF, sf * sf, Cf);
        cov_sandwich(Mi, s + COV_SP, sp * sp, Cx);
    }
    double Jw[3][3], Jn[3][3], Jd[3];                            // column k: dv / d omega_k, dv / d n_k
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) {
            Jw[i][k] = Mi[i][0] * s[COV_EG + 3 * k] + Mi[i][1] * s[COV_EG + 3 * k + 1] + Mi[i][2] * s[COV_EG + 3 * k + 2];
            Jn[i][k] = Mi[i][0] * s[COV_EN + 3 * k] + Mi[i][1] * s[COV_EN + 3 * k + 1] + Mi[i][2] * s[COV_EN + 3 * k + 2];
        }
        Jd[i] = Mi[i][0] * s[COV_ED] + Mi[i][1] * s[COV_ED + 1] + Mi[i][2] * s[COV_ED + 2];
    }
    double Jt[3][3];                                             // the gyro's total Jacobian into v - omega x t: Jw + [t]x
    const double tt[3] = {t ? t[0] : 0.0, t ? t[1] : 0.0, t ? t[2] : 0.0};
    const double Tx[3][3] = {{0.0, -tt[2], tt[1]}, {tt[2], 0.0, -tt[0]}, {-tt[1], tt[0], 0.0}};
    const double Wx[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Jt[i][j] = Jw[i][j] + Tx[i][j];
    const double sd2 = cc.sd * cc.sd, sn2 = cc.sn * cc.sn, so2 = t ? cc.soff * cc.soff : 0.0;
    double Cv[3][3], Cu[3][3], tr[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double cg = Jw[i][0] * ovar[0] * Jw[j][0] + Jw[i][1] * ovar[1] * Jw[j][1] + Jw[i][2] * ovar[2] * Jw[j][2];
            const double cgt = Jt[i][0] * ovar[0] * Jt[j][0] + Jt[i][1] * ovar[1] * Jt[j][1] + Jt[i][2] * ovar[2] * Jt[j][2];
            const double cd = sd2 * (Jd[i] * Jd[j]);
            const double cn = sn2 * (Jn[i][0] * Jn[j][0] + Jn[i][1] * Jn[j][1] + Jn[i][2] * Jn[j][2]);
            const double cl = so2 * (Wx[i][0] * Wx[j][0] + Wx[i][1] * Wx[j][1] + Wx[i][2] * Wx[j][2]);
            Cv[i][j] = Cf[i][j] + Cx[i][j] + cg + cd + cn;
            Cu[i][j] = Cf[i][j] + Cx[i][j] + cgt + cd + cn + cl;
            if (i == j) { tr[0] += Cf[i][i]; tr[1] += Cx[i][i]; tr[2] += cg; tr[3] += cd; tr[4] += cn; tr[5] += cl; }
        }
    if (R) {                                                     // C_uav = R Cu R^T, R taken as exact
        double T[3][3];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T[i][j] = R[3 * i] * Cu[0][j] + R[3 * i + 1] * Cu[1][j] + R[3 * i + 2] * Cu[2][j];
        for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) Cu[i][j] = Cu[j][i] = T[i][0] * R[3 * j] + T[i][1] * R[3 * j + 1] + T[i][2] * R[3 * j + 2];
    }
    o[0] = Cv[0][0]; o[1] = Cv[0][1]; o[2] = Cv[0][2]; o[3] = Cv[1][1]; o[4] = Cv[1][2]; o[5] = Cv[2][2];
    o[6] = Cu[0][0]; o[7] = Cu[0][1]; o[8] = Cu[0][2]; o[9] = Cu[1][1]; o[10] = Cu[1][2]; o[11] = Cu[2][2];
    o[12] = s2; o[13] = 0.0; o[14] = 0.0; o[15] = 0.0;
    for (int k = 0; k < 6; ++k) o[16 + k] = tr[k];
    o[22] = 0.0; o[23] = 0.0;
    bool fin = true;
    for (int k = 0; k < OFK_COV_DOUBLES; ++k) fin = fin && isfinite(o[k]);
    if (!fin) cov_void(o);
}

static cov_cfg cov_make_cfg(const ofk_cov *c)
{
    cov_cfg cc;
    cc.mode = c->mode; cc.sf = c->sigma_flow; cc.sp = c->sigma_pos; cc.sd = c->sigma_d;
    for (int k = 0; k < 3; ++k) cc.so[k] = c->sigma_omega[k];
    cc.sn = c->sigma_normal; cc.soff = c->sigma_offset; cc.omega_from_imu = c->omega_from_imu; cc.filter_r = c->filter_r;
    cc.r_floor = c->r_floor; cc.nis_max = c->nis_max;
    return cc;
}

// ------------------------------------------------------------------------------------------------ the filter's correct with R_eff
// R_eff = Rm with its top-left 3x3 block replaced by z_sign^2 C + r_floor I (filter_r, a covariance that is not void), else Rm;
// NIS = nu^T S^-1 nu of the correct; with nis_max > 0 a correct whose NIS exceeds it is skipped (x, P stay at the prediction).
// The correct itself is kf_correct_dev: with R_eff = Rm it is the constant-R correct bit for bit.  Returns whether it was gated.
__device__ bool kf_correct_cov_dev(int ns, int nm, const double *H, const double *Rm, const double *z, const double *cv, const cov_cfg &cc,
                                   double z_sign, int z_source, double *x, double (*P)[KF_MAX], double &nis)
{
    double Re[KF_MAX * KF_MAX];
    for (int i = 0; i < nm * nm; ++i) Re[i] = Rm[i];
    if (cc.filter_r && cv[13] == 0.0) {
        const double *t6 = cv + (z_source ? 6 : 0);
        double C[3][3]; sym3_from6(t6, C);
        for (int i = 0; i < 3 && i < nm; ++i)
            for (int j = 0; j < 3 && j < nm; ++j) Re[i * nm + j] = z_sign * z_sign * C[i][j] + (i == j ? cc.r_floor : 0.0);
    }
    double S[KF_MAX][KF_MAX + 1];                                // [S | nu], solved in place
    for (int i = 0; i < nm; ++i) {
        double hx = 0;
        for (int k = 0; k < ns; ++k) hx += H[i * ns + k] * x[k];
        S[i][nm] = z[i] - hx;
        for (int j = 0; j < nm; ++j) {
            double s = 0;
            for (int k = 0; k < ns; ++k) for (int l = 0; l < ns; ++l) s += H[i * ns + k] * P[k][l] * H[j * ns + l];
            S[i][j] = s + Re[i * nm + j];
        }
    }
    double nu[KF_MAX];
    for (int i = 0; i < nm; ++i) nu[i] = S[i][nm];
    for (int c = 0; c < nm; ++c) {
        int piv = c; double best = fabs(S[c][c]);
        for (int r2 = c + 1; r2 < nm; ++r2) if (fabs(S[r2][c]) > best) { best = fabs(S[r2][c]); piv = r2; }
        if (piv != c) for (int j = 0; j <= nm; ++j) { const double tmp = S[c][j]; S[c][j] = S[piv][j]; S[piv][j] = tmp; }
        const double inv = 1.0 / S[c][c];
        for (int j = 0; j <= nm; ++j) S[c][j] *= inv;
        for (int r2 = 0; r2 < nm; ++r2) if (r2 != c) {
            const double f = S[r2][c];
            if (f != 0.0) for (int j = 0; j <= nm; ++j) S[r2][j] -= f * S[c][j];
        }
    }
    nis = 0.0;
    for (int i = 0; i < nm; ++i) nis += nu[i] * S[i][nm];
    if (cc.nis_max > 0.0 && nis > cc.nis_max) return true;
    kf_correct_dev(ns, nm, H, Re, z, x, P);
    return false;
}

// k_kf_records with R_eff, NIS and the gate: one thread per pair, behind the pairs' covariance kernel.
__global__ void k_kf_records_cov(int ns, int nm, const double *__restrict__ mats, double *__restrict__ xs, double *__restrict__ Ps,
                                 const double *__restrict__ records, double *__restrict__ cov, cov_cfg cc, double z_sign, int z_source, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const double *F = mats, *H = mats + 72, *Q = mats + 108, *Rm = mats + 144;
    double x[KF_MAX], P[KF_MAX][KF_MAX];
    kf_load(ns, b, xs, Ps, x, P);
    kf_predict_dev(ns, 0, F, nullptr, Q, nullptr, x, P);
    const double *r = records + (size_t)b * OFK_RECORD_DOUBLES;
    double *cv = cov + (size_t)b * OFK_COV_DOUBLES;
    double nis = 0.0, gated = 0.0;
    if (r[4] == 3.0) {
        double z[KF_MAX] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 3; ++k) z[k] = z_sign * r[(z_source ? 8 : 0) + k];
        for (int k = 3; k < nm; ++k) z[k] = z[k - 3];
        gated = kf_correct_cov_dev(ns, nm, H, Rm, z, cv, cc, z_sign, z_source, x, P, nis) ? 1.0 : 0.0;
    }
    cv[14] = nis; cv[15] = gated;
    kf_store(ns, b, x, P, xs, Ps);
}

void ofk_launch_kf_records_cov(hipStream_t s, int ns, int nm, const double *mats, double *x, double *P, const double *records, double *cov,
                               const ofk_cov *c, double z_sign, int z_source, int batch)
{
    hipLaunchKernelGGL(k_kf_records_cov, dim3((batch + 63) / 64), dim3(64), 0, s, ns, nm, mats, x, P, records, cov, cov_make_cfg(c), z_sign,
                       z_source, batch);
}

// ------------------------------------------------------------------------------------------------ the three forms (k_second.inc)
// The covariance never rewrites the record: no write-back.  sigma_flow / sigma_pos are in the units of the points: of x and u at the
// stage entry, pixels scaled by the pair's `scaling` in the resident forms.
__global__ __launch_bounds__(256) void k_cov_solve(int variant, const double *__restrict__ x, const double *__restrict__ u,
                                                   const uint8_t *__restrict__ valid, int n, const double *__restrict__ d,
                                                   const double *__restrict__ nrm, const double *__restrict__ omega,
                                                   const double *__restrict__ t, const double *__restrict__ weights, cov_cfg cc,
                                                   const double *__restrict__ out, double *__restrict__ cov)
{
    __shared__ double part[4][COV_SUMS];
    const int b = blockIdx.x;
    stage_problem q;
    stage_unpack(q, b, x, u, valid, n, d, nrm, omega, t, weights, out);
    cov_core<4>(part, n, variant, q.nrm, q.om, q.d, q.vs, q.pts);
    if (threadIdx.x == 0) {
        double ovar[3];
        gyro_variances(cc, nullptr, ovar);
        cov_finish(part[0], cc, cc.sf, cc.sp, ovar, q.om, q.t, nullptr, q.rec03[3], q.rank, q.d != 0.0, cov + (size_t)b * OFK_COV_DOUBLES);
    }
}

void ofk_launch_cov_solve(hipStream_t s, const ofk_stage_in &in, const double *weights, const ofk_cov *c, const double *out, double *cov)
{
    hipLaunchKernelGGL(k_cov_solve, dim3(in.batch), dim3(256), 0, s, in.variant, in.x, in.u, in.valid, in.n, in.d, in.nrm, in.omega, in.t,
                       weights, cov_make_cfg(c), out, cov);
}

// thread 0, behind cov_core: the problem's record
__device__ __forceinline__ void cov_resident_finish(const double *sums, const cov_cfg &cc, const resident_problem &q, double *cv)
{
    double ovar[3];
    gyro_variances(cc, q.ist, ovar);
    cov_finish(sums, cc, cc.sf * q.scaling, cc.sp * q.scaling, ovar, q.om, q.sn + 16, q.R, q.rec03[3], q.rank, q.scaling != 0.0 && q.d != 0.0, cv);
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_pairs_cov(const float *__restrict__ prev_pts, const float *__restrict__ next_pts,
                                                       const uint8_t *__restrict__ status, const int *__restrict__ counts, int pts_stride,
                                                       const double *__restrict__ sensors, int variant, int use_feas, double feas_T,
                                                       const double *__restrict__ weights, cov_cfg cc,
                                                       const double *__restrict__ records, double *__restrict__ cov)
{
    __shared__ double part[4][COV_SUMS];
    const int b = blockIdx.x;
    resident_problem q;
    resident_unpack(q, b, prev_pts, next_pts, status, counts, pts_stride, sensors, nullptr, false, use_feas, feas_T, weights, records);
    cov_core<NW>(part, q.n, variant, q.nrm, q.om, q.d, q.rec03, q.pts);
    if (threadIdx.x == 0) cov_resident_finish(part[0], cc, q, cov + (size_t)b * OFK_COV_DOUBLES);
}

void ofk_launch_pairs_cov(hipStream_t s, const ofk_pairs_in &in, const double *weights, const ofk_cov *c, double *cov)
{
    launch_pairs_form(s, in.batch, k_pairs_cov<1>, k_pairs_cov<4>, in.prev_pts, in.next_pts, in.status, in.counts, in.pts_stride, in.sensors,
                      in.variant, in.use_feas, in.feas_T, weights, cov_make_cfg(c), (const double *)in.records, cov);
}

// With the filter on the fused kernel deferred its correct: it runs here, with R_eff, and writes NIS and the gate into the record.
__global__ __launch_bounds__(256) void k_stream_cov(fuse_args g, const double *__restrict__ weights, cov_cfg cc, double *__restrict__ cov)
{
    __shared__ double part[4][COV_SUMS];
    const int b = blockIdx.x;
    resident_problem q;
    stream_unpack(q, b, g, weights);
    cov_core<4>(part, q.n, g.variant, q.nrm, q.om, q.d, q.rec03, q.pts);
    if (threadIdx.x == 0) {
        double *cv = cov + (size_t)b * OFK_COV_DOUBLES;
        cov_resident_finish(part[0], cc, q, cv);
        if (g.f.filter && g.defer) {
            double kx[KF_MAX], kP[KF_MAX][KF_MAX], z[KF_MAX], nis = 0.0;
            bool gated = false;
            deferred_load(g, q, b, g.records + (size_t)b * OFK_RECORD_DOUBLES, kx, kP, z);
            if (q.solved) gated = kf_correct_cov_dev(g.ns, g.nm, g.H, g.Rm, z, cv, cc, g.f.z_sign, g.f.z_source, kx, kP, nis);
            cv[14] = nis; cv[15] = gated ? 1.0 : 0.0;
            deferred_store(g, q, b, kx, kP);
        }
    }
}

void ofk_launch_stream_cov(hipStream_t s, const ofk_stream_in &in, const double *weights, const ofk_cov *c, double *cov)
{
    hipLaunchKernelGGL(k_stream_cov, dim3(in.batch), dim3(256), 0, s, make_fuse_args(in, nullptr, 0, 0.0), weights, cov_make_cfg(c), cov);
}
