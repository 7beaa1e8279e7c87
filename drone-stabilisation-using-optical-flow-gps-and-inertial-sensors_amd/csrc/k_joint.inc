// k_joint.inc — the joint velocity and rotation solve (ofk.h: ofk_set_joint): the gyro refined from the flow.  Included by
// k_estimate.hip, whose helpers (point_terms, pair_point, resid_point, wave_sum, jacobi3, joint_inverse, lever_rotate, the Kalman
// recursions) it shares.  DESIGN.md, "joint solve", has the derivation.
//
// One team per problem behind whichever solve kernel ran, plain or robust: a single wave (NW = 1) or a 256-thread workgroup (NW = 4).
// The flow is linear in (v, omega): with omega = omega0 + delta point i's rows are a X v + b N delta = b X q0, p = (x, y, 1), X = [p]x,
// N = |p|^2 I - p p^T, q0, a = sA, b = sB the solve's per-point terms at omega0 and w the final robust weight (or 1).  The team reads
// the solve's v_s from the record, walks the kept points once and sums
//   M = sum w a^2 N                       6, in the solve's own order, so jacobi3 sees the solve's bits
//   K = -sum w a b |p|^2 X                3: sum g, sum g x, sum g y with g = w a b |p|^2
//   D = sum w b^2 |p|^2 N                 6
//   c = sum w b |p|^2 X (b q0 - a v_s)    3: the reduced right-hand side g_delta - K^T v_s
// and the count: 19 sums, added as the solve adds its own - four "virtual waves" take the points vw * 64 + lane + 256 k, each is
// reduced by the shuffle butterfly, the partial sums are added as (s0 + s1) + (s2 + s3) - so the records are the same bit for bit
// across forms, slice counts and overlap settings.  One lane forms S = D + Lambda - K^T M^-1 K, delta = S^-1 c, v = v_s - M^-1 K delta
// (both inverses from jacobi3) and broadcasts v and omega0 + delta through LDS; a second walk in the same order sums the residual
// there.  No atomics, no MFMA, vector stores only.
#define JOINT_SUMS 19
#define JOINT_M 0
#define JOINT_CNT 6
#define JOINT_K 7
#define JOINT_D 10
#define JOINT_C 16

struct joint_cfg { double sf, so[3]; int omega_from_imu; };

// One kept point's contributions to the 19 sums.
__device__ __forceinline__ void joint_point(double *s, int variant, double x, double y, double ux, double uy, double w, const double *nrm,
                                            const double *om, double d, const double *vs)
{
    double q0, q1, q2, a, b;
    point_terms(variant, x, y, ux, uy, nrm, om, d, 1.0, q0, q1, q2, a, b);
    const double pp = x * x + y * y + 1.0, sa2 = a * a * w;
    s[JOINT_M + 0] += sa2 * (pp - x * x); s[JOINT_M + 1] += sa2 * (-x * y); s[JOINT_M + 2] += sa2 * (-x);
    s[JOINT_M + 3] += sa2 * (pp - y * y); s[JOINT_M + 4] += sa2 * (-y);     s[JOINT_M + 5] += sa2 * (pp - 1.0);
    s[JOINT_CNT] += 1.0;
    const double g = w * a * b * pp;
    s[JOINT_K + 0] += g; s[JOINT_K + 1] += g * x; s[JOINT_K + 2] += g * y;
    const double sb2 = w * b * b * pp;
    s[JOINT_D + 0] += sb2 * (pp - x * x); s[JOINT_D + 1] += sb2 * (-x * y); s[JOINT_D + 2] += sb2 * (-x);
    s[JOINT_D + 3] += sb2 * (pp - y * y); s[JOINT_D + 4] += sb2 * (-y);     s[JOINT_D + 5] += sb2 * (pp - 1.0);
    double c0, c1, c2;
    cross_p(x, y, b * q0 - a * vs[0], b * q1 - a * vs[1], b * q2 - a * vs[2], c0, c1, c2);
    const double wb = w * b * pp;
    s[JOINT_C + 0] += wb * c0; s[JOINT_C + 1] += wb * c1; s[JOINT_C + 2] += wb * c2;
}

// One lane: the joint record from the sums.  vs: the solve's v; usable: the solve solved with rank 3, scaling and d are not 0;
// dsf2 = (d sigma_f)^2 in the units of the points; ovar: the prior variances (+inf: free, 0: held).  jr is written in full.  Returns
// whether (v, omh) replace the record's fields (flag 0 with at least one axis estimated).
__device__ bool joint_finish(const double *s, bool usable, const double *vs, const double *rec03, const double *om, double dsf2,
                             const double *ovar, double *v, double *omh, double *jr)
{
    for (int k = 0; k < OFK_JOINT_DOUBLES; ++k) jr[k] = 0.0;
    for (int k = 0; k < 3; ++k) { jr[k] = om[k]; jr[6 + k] = rec03[k]; v[k] = vs[k]; omh[k] = om[k]; }
    jr[9] = rec03[3]; jr[10] = 1.0; jr[11] = s[JOINT_CNT];
    bool fin = isfinite(dsf2) && isfinite(vs[0]) && isfinite(vs[1]) && isfinite(vs[2]);
    for (int k = 0; k < JOINT_SUMS; ++k) fin = fin && isfinite(s[k]);
    if (!usable || !fin || !(s[JOINT_CNT] > 0.0)) return false;
    double A[3][3], lam[3], V[3][3], Mi[3][3]; sym3_from6(s, A);
    jacobi3(A, lam, V);
    if (!(lam[2] > 0.0)) return false;
    joint_inverse(lam, V, 3, Mi);
    const double k0 = s[JOINT_K], kx = s[JOINT_K + 1], ky = s[JOINT_K + 2];
    const double K[3][3] = {{0.0, k0, -ky}, {-k0, 0.0, kx}, {ky, -kx, 0.0}};   // -sum g X
    double G[3][3];                                              // M^-1 K
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) G[i][j] = Mi[i][0] * K[0][j] + Mi[i][1] * K[1][j] + Mi[i][2] * K[2][j];
    bool held[3]; int ne = 0;
    for (int k = 0; k < 3; ++k) { held[k] = !(ovar[k] > 0.0); ne += held[k] ? 0 : 1; }
    double Dm[3][3], S[3][3]; sym3_from6(s + JOINT_D, Dm);
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            double t = Dm[i][j] - (K[0][i] * G[0][j] + K[1][i] * G[1][j] + K[2][i] * G[2][j]);
            if (i == j && !isinf(ovar[i])) t += dsf2 / ovar[i];
            if (held[i] || held[j]) t = 0.0;
            S[i][j] = S[j][i] = t;
        }
    double Si[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, delta[3] = {0, 0, 0}, ls[3] = {0, 0, 0};
    if (ne > 0) {
        double W[3][3], Sc[3][3];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { Sc[i][j] = S[i][j]; fin = fin && isfinite(S[i][j]); }
        if (!fin) return false;
        jacobi3(Sc, ls, W);
        for (int k = 0; k < 3; ++k) jr[12 + k] = ls[k];
        // the rank rule of the solve on the estimated axes: an eigenvalue below sqrt(eps 3m) of the largest is unobservable
        const double cut = sqrt(2.220446049250313e-16 * 3.0 * s[JOINT_CNT]) * ls[0];
        for (int k = 0; k < ne; ++k)
            if (!(ls[k] > 0.0) || ls[k] < cut) { jr[10] = 2.0; return false; }
        joint_inverse(ls, W, ne, Si);
        for (int i = 0; i < 3; ++i)
            delta[i] = held[i] ? 0.0 : Si[i][0] * s[JOINT_C] + Si[i][1] * s[JOINT_C + 1] + Si[i][2] * s[JOINT_C + 2];
    }
    double vn[3], on[3];
    for (int i = 0; i < 3; ++i) {
        vn[i] = vs[i] - (G[i][0] * delta[0] + G[i][1] * delta[1] + G[i][2] * delta[2]);
        on[i] = om[i] + delta[i];
        fin = fin && isfinite(vn[i]) && isfinite(on[i]);
    }
    if (!fin) { jr[12] = jr[13] = jr[14] = 0.0; return false; }
    double T[3][3], Cw[3][3], Cv[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T[i][j] = G[i][0] * Si[0][j] + G[i][1] * Si[1][j] + G[i][2] * Si[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            Cw[i][j] = dsf2 * Si[i][j];
            Cv[i][j] = dsf2 * (Mi[i][j] + (T[i][0] * G[j][0] + T[i][1] * G[j][1] + T[i][2] * G[j][2]));
        }
    for (int k = 0; k < 3; ++k) { jr[k] = on[k]; jr[3 + k] = delta[k]; v[k] = vn[k]; omh[k] = on[k]; }
    jr[10] = 0.0;
    jr[15] = Cw[0][0]; jr[16] = Cw[0][1]; jr[17] = Cw[0][2]; jr[18] = Cw[1][1]; jr[19] = Cw[1][2]; jr[20] = Cw[2][2];
    jr[21] = Cv[0][0]; jr[22] = Cv[0][1]; jr[23] = Cv[0][2]; jr[24] = Cv[1][1]; jr[25] = Cv[1][2]; jr[26] = Cv[2][2];
    return ne > 0;
}

// The two walks: terms(i, x, y, ux, uy, w) -> point i enters (the set the solve used).  Returns, in every thread, whether the record is
// to be rewritten; then v, omh and rss (thread 0's alone is the sum) hold the joint solution and its residual sum of squares.
// bc: 8 doubles of LDS.  jr: the problem's joint record, written by thread 0.  RSS false (k_bias.inc): the sums and the record alone, no
// second walk, rss stays 0.
template <int NW, bool RSS = true, class Terms>
__device__ __forceinline__ bool joint_core(double (*part)[JOINT_SUMS], double *bc, int n, int variant, const double *nrm, const double *om,
                                           double d, const double *vs, const double *rec03, bool usable, double dsf2, const double *ovar,
                                           double *jr, double *v, double *omh, double &rss, Terms terms)
{
    const int lane = threadIdx.x & 63, wave = NW == 1 ? 0 : (int)(threadIdx.x >> 6);
#pragma unroll 1
    for (int vw = wave; vw < 4; vw += NW) {
        double s[JOINT_SUMS];
#pragma unroll
        for (int k = 0; k < JOINT_SUMS; ++k) s[k] = 0.0;
#pragma unroll 1
        for (int i = vw * 64 + lane; i < n; i += 256) {
            double x, y, ux, uy, w;
            if (terms(i, x, y, ux, uy, w)) joint_point(s, variant, x, y, ux, uy, w, nrm, om, d, vs);
        }
        team_put<JOINT_SUMS>(part[vw], s);
    }
    team_barrier<NW>();
    if (threadIdx.x == 0) {
        double t[JOINT_SUMS], tv[3], to[3];
        team_sums<JOINT_SUMS>(part, t);
        const bool rw = joint_finish(t, usable, vs, rec03, om, dsf2, ovar, tv, to, jr);
        for (int k = 0; k < 3; ++k) { bc[k] = tv[k]; bc[3 + k] = to[k]; }
        bc[6] = rw ? 1.0 : 0.0;
    }
    team_barrier<NW>();
    for (int k = 0; k < 3; ++k) { v[k] = bc[k]; omh[k] = bc[3 + k]; }
    const bool rw = bc[6] != 0.0;
    rss = 0.0;
    if (!rw) return false;
    if (!RSS) return true;
#pragma unroll 1
    for (int vw = wave; vw < 4; vw += NW) {
        double r = 0.0;
#pragma unroll 1
        for (int i = vw * 64 + lane; i < n; i += 256) {
            double x, y, ux, uy, w, q0, q1, q2, a, b;
            if (!terms(i, x, y, ux, uy, w)) continue;
            point_terms(variant, x, y, ux, uy, nrm, omh, d, 1.0, q0, q1, q2, a, b);
            r += w * resid_point(x, y, q0, q1, q2, a, b, v);
        }
        team_put<1>(part[vw], &r);
    }
    team_barrier<NW>();
    if (threadIdx.x == 0) team_sums<1>(part, &rss);
    return true;
}

static joint_cfg joint_make_cfg(const ofk_joint *j)
{
    joint_cfg jc;
    jc.sf = j->sigma_flow; jc.omega_from_imu = j->omega_from_imu;
    for (int k = 0; k < 3; ++k) jc.so[k] = j->sigma_omega[k];
    return jc;
}

// ------------------------------------------------------------------------------------------------ the three forms (k_second.inc)
// sigma_flow is in the units of the points: of x and u at the stage entry, pixels scaled by the pair's `scaling` in the resident forms.
__global__ __launch_bounds__(256) void k_joint_solve(int variant, const double *__restrict__ x, const double *__restrict__ u,
                                                     const uint8_t *__restrict__ valid, int n, const double *__restrict__ d,
                                                     const double *__restrict__ nrm, const double *__restrict__ omega,
                                                     const double *__restrict__ t, const double *__restrict__ weights, joint_cfg jc,
                                                     double *__restrict__ out, double *__restrict__ joint)
{
    __shared__ double part[4][JOINT_SUMS];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    stage_problem q;
    stage_unpack(q, b, x, u, valid, n, d, nrm, omega, t, weights, out);
    double ovar[3], v[3], omh[3], rss;
    gyro_variances(jc, nullptr, ovar);
    const bool rw = joint_core<4>(part, bc, n, variant, q.nrm, q.om, q.d, q.vs, q.rec03, q.rank >= 3.0 && q.d != 0.0,
                                  (q.d * jc.sf) * (q.d * jc.sf), ovar, joint + (size_t)b * OFK_JOINT_DOUBLES, v, omh, rss, q.pts);
    stage_write(q, rw, v, omh, rss, out + (size_t)b * OFK_SOLVE_DOUBLES);
}

void ofk_launch_joint_solve(hipStream_t s, const ofk_stage_in &in, const double *weights, const ofk_joint *j, double *out, double *joint)
{
    hipLaunchKernelGGL(k_joint_solve, dim3(in.batch), dim3(256), 0, s, in.variant, in.x, in.u, in.valid, in.n, in.d, in.nrm, in.omega, in.t,
                       weights, joint_make_cfg(j), out, joint);
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_pairs_joint(const float *__restrict__ prev_pts, const float *__restrict__ next_pts,
                                                         const uint8_t *__restrict__ status, const int *__restrict__ counts, int pts_stride,
                                                         const double *__restrict__ sensors, int variant, int use_feas, double feas_T,
                                                         const double *__restrict__ weights, joint_cfg jc, double *__restrict__ records,
                                                         double *__restrict__ joint)
{
    __shared__ double part[4][JOINT_SUMS];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    resident_problem q;
    resident_unpack(q, b, prev_pts, next_pts, status, counts, pts_stride, sensors, nullptr, false, use_feas, feas_T, weights, records);
    double ovar[3], v[3], omh[3], rss;
    gyro_variances(jc, nullptr, ovar);
    const double dsf = q.d * jc.sf * q.scaling;
    const bool rw = joint_core<NW>(part, bc, q.n, variant, q.nrm, q.om, q.d, q.rec03, q.rec03, q.rank >= 3.0 && q.scaling != 0.0 && q.d != 0.0,
                                   dsf * dsf, ovar, joint + (size_t)b * OFK_JOINT_DOUBLES, v, omh, rss, q.pts);
    pairs_write(q, rw, v, omh, rss, records + (size_t)b * OFK_RECORD_DOUBLES);
}

void ofk_launch_pairs_joint(hipStream_t s, const ofk_pairs_in &in, const double *weights, const ofk_joint *j, double *joint)
{
    launch_pairs_form(s, in.batch, k_pairs_joint<1>, k_pairs_joint<4>, in.prev_pts, in.next_pts, in.status, in.counts, in.pts_stride, in.sensors,
                      in.variant, in.use_feas, in.feas_T, weights, joint_make_cfg(j), in.records, joint);
}

__global__ __launch_bounds__(256) void k_stream_joint(fuse_args g, const double *__restrict__ weights, joint_cfg jc, double *__restrict__ joint)
{
    __shared__ double part[4][JOINT_SUMS];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    resident_problem q;
    stream_unpack(q, b, g, weights);
    double ovar[3], v[3], omh[3], rss;
    gyro_variances(jc, q.ist, ovar);
    const double dsf = q.d * jc.sf * q.scaling;
    const bool rw = joint_core<4>(part, bc, q.n, g.variant, q.nrm, q.om, q.d, q.rec03, q.rec03,
                                  q.solved && q.rank >= 3.0 && q.scaling != 0.0 && q.d != 0.0, dsf * dsf, ovar,
                                  joint + (size_t)b * OFK_JOINT_DOUBLES, v, omh, rss, q.pts);
    stream_tail(g, q, b, rw, v, omh, rss);
}

void ofk_launch_stream_joint(hipStream_t s, const ofk_stream_in &in, const double *weights, const ofk_joint *j, double *joint)
{
    hipLaunchKernelGGL(k_stream_joint, dim3(in.batch), dim3(256), 0, s, make_fuse_args(in, nullptr, 0, 0.0), weights, joint_make_cfg(j), joint);
}
