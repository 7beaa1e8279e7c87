// k_plane.inc — the plane solve (ofk.h: ofk_set_plane): the ground normal refined from the flow.  Included by k_estimate.hip, whose
// helpers (point_terms, pair_point, cross_p, wave_sum, jacobi3, eig_inverse3, lever_rotate, the Kalman recursions) it shares.
// DESIGN.md, "plane solve", has the derivation.
//
// One team per problem behind whichever solve kernel ran, plain or robust: a single wave (NW = 1) or a 256-thread workgroup (NW = 4).
// With m = n / d the plane's inverse-distance vector, p = (x, y, 1), X = [p]x and the solve's q, sA, sB at the sensors' n0, d0, point
// i's rows are r = sB [(m.p) X v - X q]: bilinear in (v, m), the solve's own rows at m0 = n0 / d0.  The range along the beam e holds
// m.e, so m = m0 + T tau with T = [t1 t2] orthogonal to e, and the five unknowns (v, tau) come from a Gauss-Newton iteration started
// at the solve's v and tau = 0.  Every walk over the kept points sums, at the current (v, tau), with c = m.p, a = sB c (the first
// walk: a = sA, the solve's own rows and matrix), h = T^T p, y = X v:
//   M = sum w a^2 N                  6, in the solve's own order
//   K = sum w sB a (X^T y) h^T       6
//   D = sum w sB^2 |y|^2 h h^T       3
//   g_v = -sum w a X^T r             3
//   g_tau = -sum w sB (y.r) h        2
//   sum w |r|^2 and the count        2
// 22 sums, added as the solve adds its own - four "virtual waves" take the points vw * 64 + lane + 256 k, each is reduced by the
// shuffle butterfly, the partial sums are added as (s0 + s1) + (s2 + s3) - so the records are the same bit for bit across forms, slice
// counts and overlap settings.  After each walk but the last one lane takes the step by the Schur complement, S = D + Lambda -
// K^T M^-1 K (2 x 2, inverted in closed form from its eigen-decomposition; M^-1 from jacobi3), and broadcasts (v, tau) through LDS;
// the last walk gives the residual and the Hessian at the solution.  No atomics, no MFMA, vector stores only.
#define PLANE_SUMS 22
#define PLANE_M 0
#define PLANE_CNT 6
#define PLANE_K 7
#define PLANE_D 13
#define PLANE_GV 16
#define PLANE_GT 19
#define PLANE_RSS 21

struct plane_cfg { double sf, sn, smax, e[3], t1[3], t2[3]; int iters; };

// One kept point's contributions to the 22 sums at (v, m).
__device__ __forceinline__ void plane_point(double *s, int variant, bool first, double x, double y, double ux, double uy, double w,
                                            const double *nrm, const double *om, double d, const double *m, const plane_cfg &pc,
                                            const double *v)
{
    double q0, q1, q2, sA, sB;
    point_terms(variant, x, y, ux, uy, nrm, om, d, 1.0, q0, q1, q2, sA, sB);
    const double c = m[0] * x + m[1] * y + m[2];
    const double a = first ? sA : sB * c;
    double y0, y1, y2, c0, c1, c2;
    cross_p(x, y, v[0], v[1], v[2], y0, y1, y2);               // y = X v
    cross_p(x, y, q0, q1, q2, c0, c1, c2);                     // X q
    const double r0 = a * y0 - sB * c0, r1 = a * y1 - sB * c1, r2 = a * y2 - sB * c2;
    const double h0 = pc.t1[0] * x + pc.t1[1] * y + pc.t1[2], h1 = pc.t2[0] * x + pc.t2[1] * y + pc.t2[2];
    double z0, z1, z2, e0, e1, e2;
    cross_p(x, y, y0, y1, y2, z0, z1, z2);                     // X y = -X^T y
    cross_p(x, y, r0, r1, r2, e0, e1, e2);                     // X r = -X^T r
    const double pp = x * x + y * y + 1.0, sa2 = a * a * w;
    s[PLANE_M + 0] += sa2 * (pp - x * x); s[PLANE_M + 1] += sa2 * (-x * y); s[PLANE_M + 2] += sa2 * (-x);
    s[PLANE_M + 3] += sa2 * (pp - y * y); s[PLANE_M + 4] += sa2 * (-y);     s[PLANE_M + 5] += sa2 * (pp - 1.0);
    s[PLANE_CNT] += 1.0;
    const double g = -(w * sB * a);
    s[PLANE_K + 0] += g * z0 * h0; s[PLANE_K + 1] += g * z0 * h1; s[PLANE_K + 2] += g * z1 * h0;
    s[PLANE_K + 3] += g * z1 * h1; s[PLANE_K + 4] += g * z2 * h0; s[PLANE_K + 5] += g * z2 * h1;
    const double dy = w * sB * sB * (y0 * y0 + y1 * y1 + y2 * y2);
    s[PLANE_D + 0] += dy * (h0 * h0); s[PLANE_D + 1] += dy * (h0 * h1); s[PLANE_D + 2] += dy * (h1 * h1);
    const double wa = w * a;
    s[PLANE_GV + 0] += wa * e0; s[PLANE_GV + 1] += wa * e1; s[PLANE_GV + 2] += wa * e2;
    const double gy = -(w * sB * (y0 * r0 + y1 * r1 + y2 * r2));
    s[PLANE_GT + 0] += gy * h0; s[PLANE_GT + 1] += gy * h1;
    s[PLANE_RSS] += w * (r0 * r0 + r1 * r1 + r2 * r2);
}

// The symmetric 2 x 2 [[a, b], [b, c]] by its eigen-decomposition in closed form: l1 >= l2; false where one is not positive.
__device__ __forceinline__ bool plane_sym2(double a, double b, double c, double &l1, double &l2, double Si[2][2])
{
    const double mean = 0.5 * (a + c), hd = 0.5 * (a - c), rad = sqrt(hd * hd + b * b);
    l1 = mean + rad; l2 = 0.0;
    if (!(l1 > 0.0)) return false;
    l2 = (a * c - b * b) / l1;
    if (!(l2 > 0.0)) return false;
    double e0, e1;
    if (b == 0.0) { e0 = a >= c ? 1.0 : 0.0; e1 = a >= c ? 0.0 : 1.0; }
    else {
        e0 = a >= c ? l1 - c : b; e1 = a >= c ? b : l1 - a;
        const double nn = sqrt(e0 * e0 + e1 * e1);
        e0 /= nn; e1 /= nn;
    }
    Si[0][0] = e0 * e0 / l1 + e1 * e1 / l2; Si[0][1] = Si[1][0] = e0 * e1 / l1 - e1 * e0 / l2; Si[1][1] = e1 * e1 / l1 + e0 * e0 / l2;
    return true;
}

// What the finishing lane carries from walk to walk.
struct plane_state { double v[3], tau[2], f0, step, l1, l2; };

// One lane, after walk k: the step (k < iters) or the record (k == iters, or an earlier end).  Returns 0 = walk on at the new (v, tau),
// 1 = ended with the record rewritten at st.v (rss = the last walk's sum w |r|^2), 2 = ended with the record untouched.  pr is written
// in full whenever the result is not 0.  usable: the solve solved with rank 3, scaling, d and n0.e are not 0; dsf2 = (d sigma_f)^2 in
// the units of the points; lam = Lambda's diagonal (0: free); held: sigma_normal == 0.
__device__ int plane_finish(const double *s, int k, bool usable, const double *rec03, const double *nrm, double d, double dsf2, double lam,
                            bool held, const plane_cfg &pc, plane_state &st, double *pr)
{
    int flag = 1;
    double Mi[3][3], G[3][2], Si[2][2] = {{0, 0}, {0, 0}}, F = 0.0;
    bool fin = usable && isfinite(dsf2) && isfinite(lam) && isfinite(d);
    for (int i = 0; i < PLANE_SUMS; ++i) fin = fin && isfinite(s[i]);
    for (int i = 0; i < 3; ++i) fin = fin && isfinite(st.v[i]);
    bool done = false;                                          // reached the end of the last walk with every gate passed
    if (fin && s[PLANE_CNT] > 0.0) {
        F = s[PLANE_RSS] + lam * (st.tau[0] * st.tau[0] + st.tau[1] * st.tau[1]);
        if (k == 0) st.f0 = F;
        double A[3][3], lm[3], V[3][3]; sym3_from6(s, A);
        jacobi3(A, lm, V);
        if (lm[2] > 0.0 && isfinite(lm[0])) {
            eig_inverse3(lm, V, Mi);
            if (held) { flag = 0; done = true; }
            else {
                const double *K = s + PLANE_K, *gv = s + PLANE_GV, *gt = s + PLANE_GT;
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 2; ++j) G[i][j] = Mi[i][0] * K[j] + Mi[i][1] * K[2 + j] + Mi[i][2] * K[4 + j];
                const double S00 = s[PLANE_D] + lam - (K[0] * G[0][0] + K[2] * G[1][0] + K[4] * G[2][0]);
                const double S01 = s[PLANE_D + 1] - (K[0] * G[0][1] + K[2] * G[1][1] + K[4] * G[2][1]);
                const double S11 = s[PLANE_D + 2] + lam - (K[1] * G[0][1] + K[3] * G[1][1] + K[5] * G[2][1]);
                const bool pos = plane_sym2(S00, S01, S11, st.l1, st.l2, Si);
                if (!(isfinite(st.l1) && isfinite(st.l2))) flag = 1;
                else if (!pos) flag = 2;
                else if (k < pc.iters) {
                    double mg[3], rhs[2], dt[2], t3[3], dv[3];
                    for (int i = 0; i < 3; ++i) mg[i] = Mi[i][0] * gv[0] + Mi[i][1] * gv[1] + Mi[i][2] * gv[2];
                    for (int j = 0; j < 2; ++j) rhs[j] = gt[j] - lam * st.tau[j] - (K[j] * mg[0] + K[2 + j] * mg[1] + K[4 + j] * mg[2]);
                    for (int j = 0; j < 2; ++j) dt[j] = Si[j][0] * rhs[0] + Si[j][1] * rhs[1];
                    for (int i = 0; i < 3; ++i) t3[i] = gv[i] - (K[2 * i] * dt[0] + K[2 * i + 1] * dt[1]);
                    for (int i = 0; i < 3; ++i) dv[i] = Mi[i][0] * t3[0] + Mi[i][1] * t3[1] + Mi[i][2] * t3[2];
                    for (int i = 0; i < 3; ++i) st.v[i] += dv[i];
                    st.tau[0] += dt[0]; st.tau[1] += dt[1];
                    const double vn = sqrt(st.v[0] * st.v[0] + st.v[1] * st.v[1] + st.v[2] * st.v[2]);
                    st.step = vn > 0.0 ? sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2] + d * d * (dt[0] * dt[0] + dt[1] * dt[1])) / vn : 0.0;
                    if (isfinite(st.v[0]) && isfinite(st.v[1]) && isfinite(st.v[2]) && isfinite(st.tau[0]) && isfinite(st.tau[1])) return 0;
                } else { flag = 0; done = true; }
            }
        }
    }
    // the record
    for (int i = 0; i < OFK_PLANE_DOUBLES; ++i) pr[i] = 0.0;
    for (int i = 0; i < 3; ++i) { pr[i] = nrm[i]; pr[6 + i] = rec03[i]; }
    pr[3] = d; pr[9] = rec03[3]; pr[11] = s[PLANE_CNT];
    double m[3], nh[3], dh = 0.0, sig = 0.0, ang = 0.0, Cv[6] = {0, 0, 0, 0, 0, 0};
    if (done) {
        for (int i = 0; i < 3; ++i) m[i] = nrm[i] / d + (pc.t1[i] * st.tau[0] + pc.t2[i] * st.tau[1]);
        const double mm = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
        for (int i = 0; i < 3; ++i) nh[i] = m[i] / mm;
        dh = 1.0 / mm;
        fin = isfinite(nh[0]) && isfinite(nh[1]) && isfinite(nh[2]) && isfinite(dh) && isfinite(F) && isfinite(st.step);
        int q = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j, ++q) {
                double t = Mi[i][j];
                if (!held) t += (G[i][0] * Si[0][0] + G[i][1] * Si[1][0]) * G[j][0] + (G[i][0] * Si[0][1] + G[i][1] * Si[1][1]) * G[j][1];
                Cv[q] = dsf2 * t;
                fin = fin && isfinite(Cv[q]);
            }
        if (!held) {
            sig = fabs(d) * sqrt(dsf2 / st.l2);
            const double x0 = nh[1] * nrm[2] - nh[2] * nrm[1], x1 = nh[2] * nrm[0] - nh[0] * nrm[2], x2 = nh[0] * nrm[1] - nh[1] * nrm[0];
            ang = atan2(sqrt(x0 * x0 + x1 * x1 + x2 * x2), nh[0] * nrm[0] + nh[1] * nrm[1] + nh[2] * nrm[2]);
            fin = fin && isfinite(sig) && isfinite(ang);
        }
        if (!fin) flag = 1;
        else if (!held && sig > pc.smax) flag = 2;
        else if (!held && F > st.f0) flag = 3;
    }
    pr[10] = (double)flag;
    if (isfinite(st.l1) && isfinite(st.l2)) { pr[12] = st.l1; pr[13] = st.l2; }
    if (isfinite(st.f0)) pr[26] = st.f0;
    if (done && isfinite(F)) pr[27] = F;
    if (flag != 0) return 2;
    pr[0] = nh[0]; pr[1] = nh[1]; pr[2] = nh[2]; pr[3] = dh;
    for (int i = 0; i < 6; ++i) pr[20 + i] = Cv[i];
    if (held) return 2;                                         // nothing estimated: the solve's record stands
    pr[4] = st.tau[0]; pr[5] = st.tau[1]; pr[14] = sig; pr[15] = ang; pr[16] = st.step;
    pr[17] = dsf2 * Si[0][0]; pr[18] = dsf2 * Si[0][1]; pr[19] = dsf2 * Si[1][1];
    return 1;
}

// The walks: terms(i, x, y, ux, uy, w) -> point i enters (the set the solve used).  Returns, in every thread, whether the record is to
// be rewritten; then v and rss (thread 0's alone is the sum) hold the solution and its residual sum of squares.
// bc: 8 doubles of LDS.  pr: the problem's plane record, written by thread 0.
template <int NW, class Terms>
__device__ __forceinline__ bool plane_core(double (*part)[PLANE_SUMS], double *bc, int n, int variant, const double *nrm, const double *om,
                                           double d, const double *vs, const double *rec03, bool usable, double sf, const plane_cfg &pc,
                                           double *pr, double *v, double &rss, Terms terms)
{
    const int lane = threadIdx.x & 63, wave = NW == 1 ? 0 : (int)(threadIdx.x >> 6);
    const bool held = !(pc.sn > 0.0);
    const double dsf = d * sf, lroot = held || isinf(pc.sn) ? 0.0 : d * dsf / pc.sn;
    const double ne = nrm[0] * pc.e[0] + nrm[1] * pc.e[1] + nrm[2] * pc.e[2];
    usable = usable && d != 0.0 && ne != 0.0 && isfinite(ne);
    plane_state st;
    st.v[0] = vs[0]; st.v[1] = vs[1]; st.v[2] = vs[2]; st.tau[0] = st.tau[1] = 0.0; st.f0 = st.step = st.l1 = st.l2 = 0.0;
    double tau0 = 0.0, tau1 = 0.0;
    v[0] = vs[0]; v[1] = vs[1]; v[2] = vs[2];
    int end = 0;
    rss = 0.0;
#pragma unroll 1
    for (int k = 0; k <= pc.iters && !end; ++k) {
        const double m[3] = {nrm[0] / d + (pc.t1[0] * tau0 + pc.t2[0] * tau1), nrm[1] / d + (pc.t1[1] * tau0 + pc.t2[1] * tau1),
                             nrm[2] / d + (pc.t1[2] * tau0 + pc.t2[2] * tau1)};
#pragma unroll 1
        for (int vw = wave; vw < 4; vw += NW) {
            double s[PLANE_SUMS];
#pragma unroll
            for (int j = 0; j < PLANE_SUMS; ++j) s[j] = 0.0;
#pragma unroll 1
            for (int i = vw * 64 + lane; i < n; i += 256) {
                double x, y, ux, uy, w;
                if (terms(i, x, y, ux, uy, w)) plane_point(s, variant, k == 0, x, y, ux, uy, w, nrm, om, d, m, pc, v);
            }
            team_put<PLANE_SUMS>(part[vw], s);
        }
        team_barrier<NW>();
        if (threadIdx.x == 0) {
            double t[PLANE_SUMS];
            team_sums<PLANE_SUMS>(part, t);
            const int e = plane_finish(t, k, usable, rec03, nrm, d, dsf * dsf, lroot * lroot, held, pc, st, pr);
            for (int j = 0; j < 3; ++j) bc[j] = st.v[j];
            bc[3] = st.tau[0]; bc[4] = st.tau[1]; bc[5] = (double)e; bc[6] = t[PLANE_RSS];
        }
        team_barrier<NW>();
        for (int j = 0; j < 3; ++j) v[j] = bc[j];
        tau0 = bc[3]; tau1 = bc[4]; end = (int)bc[5]; rss = bc[6];
    }
    return end == 1;
}

static plane_cfg plane_make_cfg(const ofk_plane *p)
{
    plane_cfg pc;
    pc.sf = p->sigma_flow; pc.sn = p->sigma_normal; pc.smax = p->sigma_max; pc.iters = p->iters;
    const double nn = std::sqrt(p->beam[0] * p->beam[0] + p->beam[1] * p->beam[1] + p->beam[2] * p->beam[2]);
    for (int k = 0; k < 3; ++k) pc.e[k] = p->beam[k] / nn;
    int ax = 0;                                                 // the coordinate axis of smallest |e_k|, lowest index on a tie
    for (int k = 1; k < 3; ++k) if (std::fabs(pc.e[k]) < std::fabs(pc.e[ax])) ax = k;
    double a[3] = {0, 0, 0};
    a[ax] = 1.0;
    double t[3] = {pc.e[1] * a[2] - pc.e[2] * a[1], pc.e[2] * a[0] - pc.e[0] * a[2], pc.e[0] * a[1] - pc.e[1] * a[0]};
    const double tn = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int k = 0; k < 3; ++k) pc.t1[k] = t[k] / tn;
    pc.t2[0] = pc.e[1] * pc.t1[2] - pc.e[2] * pc.t1[1]; pc.t2[1] = pc.e[2] * pc.t1[0] - pc.e[0] * pc.t1[2];
    pc.t2[2] = pc.e[0] * pc.t1[1] - pc.e[1] * pc.t1[0];
    return pc;
}

// ------------------------------------------------------------------------------------------------ the three forms (k_second.inc)
// sigma_flow is in the units of the points: of x and u at the stage entry, pixels scaled by the pair's `scaling` in the resident forms.
__global__ __launch_bounds__(256) void k_plane_solve(int variant, const double *__restrict__ x, const double *__restrict__ u,
                                                     const uint8_t *__restrict__ valid, int n, const double *__restrict__ d,
                                                     const double *__restrict__ nrm, const double *__restrict__ omega,
                                                     const double *__restrict__ t, const double *__restrict__ weights, plane_cfg pc,
                                                     double *__restrict__ out, double *__restrict__ plane)
{
    __shared__ double part[4][PLANE_SUMS];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    stage_problem q;
    stage_unpack(q, b, x, u, valid, n, d, nrm, omega, t, weights, out);
    double v[3], rss;
    const bool rw = plane_core<4>(part, bc, n, variant, q.nrm, q.om, q.d, q.vs, q.rec03, q.rank >= 3.0, pc.sf, pc,
                                  plane + (size_t)b * OFK_PLANE_DOUBLES, v, rss, q.pts);
    stage_write(q, rw, v, q.om, rss, out + (size_t)b * OFK_SOLVE_DOUBLES);
}

void ofk_launch_plane_solve(hipStream_t s, const ofk_stage_in &in, const double *weights, const ofk_plane *p, double *out, double *plane)
{
    hipLaunchKernelGGL(k_plane_solve, dim3(in.batch), dim3(256), 0, s, in.variant, in.x, in.u, in.valid, in.n, in.d, in.nrm, in.omega, in.t,
                       weights, plane_make_cfg(p), out, plane);
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_pairs_plane(const float *__restrict__ prev_pts, const float *__restrict__ next_pts,
                                                         const uint8_t *__restrict__ status, const int *__restrict__ counts, int pts_stride,
                                                         const double *__restrict__ sensors, int variant, int use_feas, double feas_T,
                                                         const double *__restrict__ weights, plane_cfg pc, double *__restrict__ records,
                                                         double *__restrict__ plane)
{
    __shared__ double part[4][PLANE_SUMS];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    resident_problem q;
    resident_unpack(q, b, prev_pts, next_pts, status, counts, pts_stride, sensors, nullptr, false, use_feas, feas_T, weights, records);
    double v[3], rss;
    const bool rw = plane_core<NW>(part, bc, q.n, variant, q.nrm, q.om, q.d, q.rec03, q.rec03, q.rank >= 3.0 && q.scaling != 0.0,
                                   pc.sf * q.scaling, pc, plane + (size_t)b * OFK_PLANE_DOUBLES, v, rss, q.pts);
    pairs_write(q, rw, v, q.om, rss, records + (size_t)b * OFK_RECORD_DOUBLES);
}

void ofk_launch_pairs_plane(hipStream_t s, const ofk_pairs_in &in, const double *weights, const ofk_plane *p, double *plane)
{
    launch_pairs_form(s, in.batch, k_pairs_plane<1>, k_pairs_plane<4>, in.prev_pts, in.next_pts, in.status, in.counts, in.pts_stride, in.sensors,
                      in.variant, in.use_feas, in.feas_T, weights, plane_make_cfg(p), in.records, plane);
}

__global__ __launch_bounds__(256) void k_stream_plane(fuse_args g, const double *__restrict__ weights, plane_cfg pc, double *__restrict__ plane)
{
    __shared__ double part[4][PLANE_SUMS];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    resident_problem q;
    stream_unpack(q, b, g, weights);
    double v[3], rss;
    const bool rw = plane_core<4>(part, bc, q.n, g.variant, q.nrm, q.om, q.d, q.rec03, q.rec03, q.solved && q.rank >= 3.0 && q.scaling != 0.0,
                                  pc.sf * q.scaling, pc, plane + (size_t)b * OFK_PLANE_DOUBLES, v, rss, q.pts);
    stream_tail(g, q, b, rw, v, q.om, rss);
}

void ofk_launch_stream_plane(hipStream_t s, const ofk_stream_in &in, const double *weights, const ofk_plane *p, double *plane)
{
    hipLaunchKernelGGL(k_stream_plane, dim3(in.batch), dim3(256), 0, s, make_fuse_args(in, nullptr, 0, 0.0), weights, plane_make_cfg(p), plane);
}
