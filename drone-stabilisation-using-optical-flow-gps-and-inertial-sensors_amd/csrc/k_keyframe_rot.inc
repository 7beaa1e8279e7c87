// k_keyframe_rot.inc — the keyframe's rotation refined from the flow (ofk.h: ofk_set_keyframe_rotation): k_keyframe_step's rules with
// the key solve widened to (T, delta), R^ = exp([delta]x) R_acc, under a Gaussian prior on delta.  Included by k_tracks.hip behind
// k_keyframe.inc, whose body (k_keyframe_body.inc) it compiles a second time with KF_ROT 1; k_keyframe_step itself is the same text
// with KF_ROT 0.  Like it: one workgroup per stream, only that stream's rows and state, plain vector stores, no atomics, f64 in the
// order ofk.h states.  The eighteen extra sums of a walk go through k_lstsq.inc's block_sums, like the Acc beside them and in the same
// LDS rows; the 3 x 3 work (its sym3_from6, eig_inverse3, eig_solve3, all_finite_sum) is done by every thread, the covariances by
// thread 0 alone, which parks them in LDS until the record is written.

#define KR_SUMS 18                                               // M_Td 0-8 (row i of T, column k of delta), M_dd 9-14 (upper triangle), g_d 15-17

struct kr_cfg { int source, ax0, ax1, ax2, iters; double sg2, sb, var_att, dmax; };
struct kr_prior { double lam[3], sig[3]; bool held[3]; };

// the row's share of the joint sums: c_k the columns of B (a third component of zero), N = X^T X of p = (a, b, 1), q = (u0, u1, 0)
__device__ __forceinline__ void kr_point(double *J, double a, double b, double u0, double u1, double sA)
{
    const double pp = a * a + b * b + 1.0;
    const double n00 = pp - a * a, n01 = -a * b, n02 = -a, n11 = pp - b * b, n12 = -b;
    const double cx[3] = {-(a * b), 1.0 + a * a, -b}, cy[3] = {-(1.0 + b * b), a * b, a};
    double w0[3], w1[3], w2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w0[k] = n00 * cx[k] + n01 * cy[k]; w1[k] = n01 * cx[k] + n11 * cy[k]; w2[k] = n02 * cx[k] + n12 * cy[k];
        J[k] += sA * w0[k]; J[3 + k] += sA * w1[k]; J[6 + k] += sA * w2[k];
    }
    J[9] += cx[0] * w0[0] + cy[0] * w1[0]; J[10] += cx[0] * w0[1] + cy[0] * w1[1]; J[11] += cx[0] * w0[2] + cy[0] * w1[2];
    J[12] += cx[1] * w0[1] + cy[1] * w1[1]; J[13] += cx[1] * w0[2] + cy[1] * w1[2]; J[14] += cx[2] * w0[2] + cy[2] * w1[2];
    const double q0 = n00 * u0 + n01 * u1, q1 = n01 * u0 + n11 * u1;
#pragma unroll
    for (int k = 0; k < 3; ++k) J[15 + k] += cx[k] * q0 + cy[k] * q1;
}

// R = exp([o]x) R0 with rule 1's coefficients
__device__ __forceinline__ void kr_exp_mul(const double *o, const double *R0, double *R)
{
    const double th2 = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
    double A = 1.0, B = 0.5;
    if (!(th2 < 1e-16)) { const double th = sqrt(th2); A = sin(th) / th; B = (1.0 - cos(th)) / th2; }
    const double K[9] = {0.0, -o[2], o[1], o[2], 0.0, -o[0], -o[1], o[0], 0.0};
    double E[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double k2 = o[i] * o[j] - (i == j ? th2 : 0.0);
            E[3 * i + j] = ((i == j ? 1.0 : 0.0) + A * K[3 * i + j]) + B * k2;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (E[3 * i] * R0[j] + E[3 * i + 1] * R0[3 + j]) + E[3 * i + 2] * R0[6 + j];
}

// One walk over the member rows under the rotation R; gate: only the rows whose residual under (Rg, Tg) is inside g2.  The sums come
// back reduced, in every thread.
__device__ __forceinline__ void kr_walk(const ofk_kf_rows &t, const ofk_kf_in &in, size_t base, int n, const kf_frame &f0, const double *R,
                                        bool gate, const double *Rg, const double *Tg, double g2, Acc &a, double *J, double (*part)[KR_SUMS])
{
    kf_frame f = f0, fg = f0;
    for (int k = 0; k < 9; ++k) { f.R[k] = R[k]; fg.R[k] = Rg[k]; }
    acc_zero(a);
    for (int k = 0; k < KR_SUMS; ++k) J[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const size_t r = base + i;
        if (in.status[r] == 0 || t.member[r] == 0) continue;
        double x, y, u0, u1, sA;
        if (gate && !(kf_row(t, in.next_pts, r, fg, x, y, u0, u1, sA) && kf_res2(x, y, u0, u1, sA, Tg) <= g2)) continue;
        if (kf_row(t, in.next_pts, r, f, x, y, u0, u1, sA)) { acc_point(a, x, y, u0, u1, 0.0, sA, 1.0); kr_point(J, x, y, u0, u1, sA); }
    }
    double v[11];
    acc_pack(a, v); block_sums<11, KR_SUMS>(v, part); acc_unpack(a, v);
    block_sums<KR_SUMS, KR_SUMS>(J, part);
}

// One Gauss-Newton step from the reduced sums: the Schur complement on the T block.  dl: the correction so far (the prior is on
// dl + step).  false: M_TT or the reduced system is not positive or not finite.  cov (thread 0, LDS): C_delta 0-5, C_T 6-11, the
// reduced system's eigenvalues 12-14.
__device__ bool kr_solve(const Acc &a, const double *J, const kr_prior &pr, const double *dl, double sf2, double *ds, double *T, double *cov)
{
    const double EPS = 2.220446049250313e-16;
    double A[3][3], lam[3], V[3][3]; sym3_from6(a, A);
    const double g[3] = {a.g0, a.g1, a.g2};
    jacobi3(A, lam, V);
    const double rows = 3.0 * a.cnt, cut = EPS * (rows > 3.0 ? rows : 3.0);   // times lam[0] below: not rank_cut's order
    if (!(all_finite_sum(lam, 3) && all_finite_sum(J, KR_SUMS) && all_finite_sum(g, 3)) || !(lam[2] > lam[0] * cut) || !(lam[2] > 0.0)) return false;
    double Mi[3][3], Y[3][3], t0[3];
    eig_inverse3(lam, V, Mi);
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) Y[i][k] = (Mi[i][0] * J[k] + Mi[i][1] * J[3 + k]) + Mi[i][2] * J[6 + k];
        t0[i] = (Mi[i][0] * g[0] + Mi[i][1] * g[1]) + Mi[i][2] * g[2];
    }
    double dd[3][3], S[3][3], h[3]; sym3_from6(J + 9, dd);
    for (int k = 0; k < 3; ++k) {
        for (int l = k; l < 3; ++l) {
            double v = (dd[k][l] + (k == l ? pr.lam[k] : 0.0)) - ((J[k] * Y[0][l] + J[3 + k] * Y[1][l]) + J[6 + k] * Y[2][l]);
            if (pr.held[k] || pr.held[l]) v = k == l ? 1.0 : 0.0;
            S[k][l] = v; S[l][k] = v;
        }
        h[k] = pr.held[k] ? 0.0 : (J[15 + k] - pr.lam[k] * dl[k]) - ((J[k] * t0[0] + J[3 + k] * t0[1]) + J[6 + k] * t0[2]);
    }
    double ls[3], U[3][3];
    jacobi3(S, ls, U);
    if (!(all_finite_sum(ls, 3) && all_finite_sum(h, 3)) || !(ls[2] > ls[0] * cut) || !(ls[2] > 0.0)) return false;
    eig_solve3(ls, U, h, nullptr, ds);
    for (int k = 0; k < 3; ++k) if (pr.held[k]) ds[k] = 0.0;
    for (int i = 0; i < 3; ++i) T[i] = t0[i] - ((Y[i][0] * ds[0] + Y[i][1] * ds[1]) + Y[i][2] * ds[2]);
    if (threadIdx.x == 0) {
        double Si[3][3], Z[3][3];
        eig_inverse3(ls, U, Si);
        for (int k = 0; k < 3; ++k)
            for (int l = 0; l < 3; ++l)
                if (pr.held[k] || pr.held[l]) Si[k][l] = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) Z[i][k] = (Y[i][0] * Si[0][k] + Y[i][1] * Si[1][k]) + Y[i][2] * Si[2][k];
        int s = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j) {
                cov[s] = sf2 * Si[i][j];
                cov[6 + s] = sf2 * (Mi[i][j] + ((Z[i][0] * Y[j][0] + Z[i][1] * Y[j][1]) + Z[i][2] * Y[j][2]));
                ++s;
            }
        cov[12] = ls[0]; cov[13] = ls[1]; cov[14] = ls[2];
    }
    return true;
}

struct kr_res { double T[3], dl[3], rms, rows2, rows; int gated, flag; };

// Rule 2 of ofk_set_keyframe_rotation behind a plain first solve that stands (a1, J1: its walk's sums under R_acc).  f.R: R_acc in,
// R^ out where the joint solve stands (true); false: the plain result stands and o.flag says why.  Uniform over the workgroup.
__device__ bool kr_joint(const ofk_kf_rows &t, const ofk_kf_in &in, size_t base, int n, kf_frame &f, const Acc &a1, const double *J1,
                         const kr_prior &pr, const kf_cfg &cfg, const kr_cfg &rc, double g2, double sf2, double (*part)[KR_SUMS], double *s_red,
                         double (*s_cov)[15], kr_res &o)
{
    double Racc[9], R1[9], dl[3] = {0.0, 0.0, 0.0}, ds[3], Tj[3], J[KR_SUMS];
    for (int k = 0; k < 9; ++k) { Racc[k] = f.R[k]; R1[k] = f.R[k]; }
    for (int k = 0; k < KR_SUMS; ++k) J[k] = J1[k];
    Acc a = a1;
    o.flag = OFK_KEYROT_SINGULAR; o.gated = 0; o.rows2 = 0.0; o.rms = 0.0;
    for (int k = 0; k < 3; ++k) { o.T[k] = 0.0; o.dl[k] = 0.0; }
#pragma unroll 1
    for (int it = 1;; ++it) {
        if (a.cnt < (double)cfg.min_rows || !kr_solve(a, J, pr, dl, sf2, ds, Tj, s_cov[0])) return false;
        for (int k = 0; k < 3; ++k) dl[k] += ds[k];
        kr_exp_mul(dl, Racc, R1);
        if (it >= rc.iters) break;
        kr_walk(t, in, base, n, f, R1, false, R1, Tj, g2, a, J, part);
    }
    o.rows = a.cnt;
    double Rg[9], Tg[3];
    for (int k = 0; k < 9; ++k) Rg[k] = R1[k];
    for (int k = 0; k < 3; ++k) Tg[k] = Tj[k];
    if (cfg.gate > 0.0) {
        double R2[9], d2[3] = {dl[0], dl[1], dl[2]}, T2[3];
        for (int k = 0; k < 9; ++k) R2[k] = R1[k];
        bool ok = true;
        double rows = 0.0;
#pragma unroll 1
        for (int it = 1; it <= rc.iters; ++it) {
            kr_walk(t, in, base, n, f, R2, true, Rg, Tg, g2, a, J, part);
            if (it == 1) o.rows2 = a.cnt;
            rows = a.cnt;
            if (a.cnt < (double)cfg.min_rows || !kr_solve(a, J, pr, d2, sf2, ds, T2, s_cov[1])) { ok = false; break; }
            for (int k = 0; k < 3; ++k) d2[k] += ds[k];
            kr_exp_mul(d2, Racc, R2);
        }
        if (ok) {
            o.gated = 1; o.rows = rows;
            for (int k = 0; k < 9; ++k) R1[k] = R2[k];
            for (int k = 0; k < 3; ++k) { dl[k] = d2[k]; Tj[k] = T2[k]; }
        }
    }
    const double nd = sqrt((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]);
    for (int k = 0; k < 3; ++k) o.dl[k] = dl[k];
    if (!(nd <= rc.dmax)) { o.flag = isfinite(nd) ? OFK_KEYROT_LARGE : OFK_KEYROT_SINGULAR; o.gated = 0; o.rows2 = 0.0; return false; }
    // the residual of the rows of the solve that stands, under its R^ and T
    kf_frame fr = f, fg = f;
    for (int k = 0; k < 9; ++k) { fr.R[k] = R1[k]; fg.R[k] = Rg[k]; }
    double ss = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const size_t r = base + i;
        if (in.status[r] == 0 || t.member[r] == 0) continue;
        double x, y, u0, u1, sA;
        if (o.gated && !(kf_row(t, in.next_pts, r, fg, x, y, u0, u1, sA) && kf_res2(x, y, u0, u1, sA, Tg) <= g2)) continue;
        if (kf_row(t, in.next_pts, r, fr, x, y, u0, u1, sA)) { ss += kf_res2(x, y, u0, u1, sA, Tj); cnt += 1.0; }
    }
    ss = block_sum(ss, s_red);
    cnt = block_sum(cnt, s_red);
    o.rms = cnt > 0.0 ? sqrt(ss / cnt) / f.sc : 0.0;
    for (int k = 0; k < 9; ++k) f.R[k] = R1[k];
    for (int k = 0; k < 3; ++k) o.T[k] = Tj[k];
    o.flag = OFK_KEYROT_OK;
    return true;
}

// rst [B][OFK_KEYROT_STATE]: R_world at the keyframe 0-8, 9 1 = valid, 10 the key_step it belongs to; rrec [B][OFK_KEYROT_DOUBLES]
__global__ __launch_bounds__(256) void k_keyframe_step_rot(ofk_kf_rows t, ofk_kf_in in, kf_cfg cfg, kr_cfg rc, double *__restrict__ rst_all,
                                                           double *__restrict__ rrec_all)
{
#define KF_ROT 1
#define KF_MAP 0
#include "k_keyframe_body.inc"
#undef KF_MAP
#undef KF_ROT
}

// the rotation state beside k_keyframe_begin (limit NULL, every stream), k_keyframe_replace (the streams with a budget) and
// k_keyframe_reset (one stream, b0): no R_world(key), an empty record with `flag`.  rst NULL (a step with every axis held): the record alone.
__global__ __launch_bounds__(64) void k_keyrot_clear(double *__restrict__ rst, double *__restrict__ rrec, const int *__restrict__ limit, int b0,
                                                     int flag)
{
    const int b = b0 + blockIdx.x, tid = threadIdx.x;
    if (!rows_stream_on(b, b0, gridDim.x, limit)) return;
    if (rst && tid < OFK_KEYROT_STATE) rst[(size_t)b * OFK_KEYROT_STATE + tid] = 0.0;
    if (tid < OFK_KEYROT_DOUBLES) rrec[(size_t)b * OFK_KEYROT_DOUBLES + tid] = tid == 3 ? (double)flag : 0.0;
}

static kr_cfg kr_make_cfg(const ofk_keyframe_rotation *r)
{
    kr_cfg c;
    c.source = r->source; c.ax0 = r->axes[0]; c.ax1 = r->axes[1]; c.ax2 = r->axes[2]; c.iters = r->iters;
    c.sg2 = r->sigma_gyro * r->sigma_gyro; c.sb = r->sigma_bias; c.var_att = 2.0 * (r->sigma_att * r->sigma_att); c.dmax = r->delta_max;
    return c;
}

void ofk_launch_keyframe_step_rot(hipStream_t s, const ofk_kf_rows &t, const ofk_kf_in &in, const ofk_keyframe *k, const ofk_keyframe_rotation *r,
                                  double *rst, double *rrec, int batch)
{
    hipLaunchKernelGGL(k_keyframe_step_rot, dim3(batch), dim3(256), 0, s, t, in, kf_make_cfg(k), kr_make_cfg(r), rst, rrec);
}

void ofk_launch_keyrot_clear(hipStream_t s, double *rst, double *rrec, const int *limit, int b0, int flag, int batch)
{
    hipLaunchKernelGGL(k_keyrot_clear, dim3(batch), dim3(64), 0, s, rst, rrec, limit, b0, flag);
}
