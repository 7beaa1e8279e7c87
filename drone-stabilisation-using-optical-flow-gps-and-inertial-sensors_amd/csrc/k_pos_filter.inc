// k_pos_filter.inc — the position filter of a video stream (ofk.h: ofk_set_pos_filter): a twelve-state Kalman filter per stream that
// carries the position at the keyframe beside the current one (a cloned state), so that the keyframe's displacement D, the step's
// velocity and an absolute position fix are fused without taking the key pixels' noise for white.  Included by k_tracks.hip behind
// k_keyframe_rot.inc.
// One wave per stream.  P (12 x 12 f64, 1152 B) lives in LDS beside a second buffer of its size and the 12 x 3 strips of an update;
// lane l owns entries l, l + 64 and l + 128 of P.  The 3 x 3 Cholesky, the innovation and the gate are computed by every lane from LDS,
// so that every decision is uniform over the wave without a broadcast.  The state of one stream is only ever touched by its own
// wave, with plain vector stores and no atomics: a second launch on the same inputs gives the same bits.  All arithmetic is f64 in
// the order ofk.h states (the build has no FMA contraction).  One latency-bound launch per step.

struct pf_cfg { double dt, sigma_v, floor, infl, share, q_p, q_v, q_b, p0_p, p0_v, p0_b, nis_max; };
// where a launch finds the step's inputs: the step's records, the keyframe's records, R_world (row-major, `rw_stride` doubles apart)
struct pf_in { const double *v; int plain; const double *key_rec; const double *rw; int rw_stride; };

#define PF_N OFK_POSF_STATES
#define PF_NN (PF_N * PF_N)
#define PF_TINY 0x1p-48                                          // 16 ulp of 1: a pivot's floor against the entries it came from

struct pf_lds { double P[PF_NN], B[PF_NN], PHt[PF_N * 3], HP[3 * PF_N], K[PF_N * 3], KR[PF_N * 3], BHt[PF_N * 3], x[PF_N]; };

// H = [.. I .. -I ..]: +I at columns ia .. ia + 2, -I at ic .. ic + 2 (ic < 0: none).  Rule 6 of ofk.h.
// Returns the outcome; nis and y are written whenever S could be factored.
__device__ __forceinline__ int pf_update(pf_lds &s, int lane, int ia, int ic, const double *z, const double *R, double nis_max, double &nis,
                                         double *y)
{
    // the strips P H^T (columns) and H P (rows)
    if (lane < 36) {
        const int i = lane / 3, n = lane % 3;
        s.PHt[lane] = ic < 0 ? s.P[i * PF_N + ia + n] : s.P[i * PF_N + ia + n] - s.P[i * PF_N + ic + n];
        const int m = lane / PF_N, j = lane % PF_N;
        s.HP[lane] = ic < 0 ? s.P[(ia + m) * PF_N + j] : s.P[(ia + m) * PF_N + j] - s.P[(ic + m) * PF_N + j];
    }
    __syncthreads();
    double S[3][3];
    for (int m = 0; m < 3; ++m)
        for (int n = 0; n < 3; ++n) {
            const double h = ic < 0 ? s.P[(ia + m) * PF_N + ia + n]
                                    : ((s.P[(ia + m) * PF_N + ia + n] - s.P[(ia + m) * PF_N + ic + n]) - s.P[(ic + m) * PF_N + ia + n]) +
                                          s.P[(ic + m) * PF_N + ic + n];
            S[m][n] = h + R[3 * m + n];
        }
    for (int m = 0; m < 3; ++m) y[m] = ic < 0 ? z[m] - s.x[ia + m] : z[m] - (s.x[ia + m] - s.x[ic + m]);
    nis = 0.0;
    // a pivot must stand above the rounding of the entries it was formed from: with a wide prior the blocks of p and c are equal
    // numbers of 1e12 and more, and their difference is noise that must not be taken for information
    double tiny[3];
    for (int m = 0; m < 3; ++m) {
        const double a = fabs(s.P[(ia + m) * PF_N + ia + m]);
        tiny[m] = PF_TINY * (ic < 0 ? a : ((a + fabs(s.P[(ia + m) * PF_N + ic + m])) + fabs(s.P[(ic + m) * PF_N + ia + m])) +
                                              fabs(s.P[(ic + m) * PF_N + ic + m]));
    }
    // 3 x 3 Cholesky of the lower triangle; a pivot that is not finite or not above its floor refuses
    const double d0 = S[0][0];
    if (!(isfinite(d0) && d0 > tiny[0])) return OFK_POSF_REFUSED;
    const double l00 = sqrt(d0), l10 = S[1][0] / l00, l20 = S[2][0] / l00;
    const double d1 = S[1][1] - l10 * l10;
    if (!(isfinite(d1) && d1 > tiny[1])) return OFK_POSF_REFUSED;
    const double l11 = sqrt(d1), l21 = (S[2][1] - l20 * l10) / l11;
    const double d2 = (S[2][2] - l20 * l20) - l21 * l21;
    if (!(isfinite(d2) && d2 > tiny[2])) return OFK_POSF_REFUSED;
    const double l22 = sqrt(d2);
    {
        const double w0 = y[0] / l00, w1 = (y[1] - l10 * w0) / l11, w2 = ((y[2] - l20 * w0) - l21 * w1) / l22;
        nis = (w0 * w0 + w1 * w1) + w2 * w2;
    }
    if (!isfinite(nis)) return OFK_POSF_REFUSED;
    if (nis_max > 0.0 && nis > nis_max) return OFK_POSF_GATED;
    // K = P H^T S^-1, a row per lane: S k = (P H^T)_i through the factor
    if (lane < PF_N) {
        const double a0 = s.PHt[3 * lane], a1 = s.PHt[3 * lane + 1], a2 = s.PHt[3 * lane + 2];
        const double t0 = a0 / l00, t1 = (a1 - l10 * t0) / l11, t2 = ((a2 - l20 * t0) - l21 * t1) / l22;
        const double k2 = t2 / l22, k1 = (t1 - l21 * k2) / l11, k0 = ((t0 - l10 * k1) - l20 * k2) / l00;
        s.K[3 * lane] = k0; s.K[3 * lane + 1] = k1; s.K[3 * lane + 2] = k2;
    }
    __syncthreads();                                             // every lane has read x for its y
    if (lane < 36) {
        const int i = lane / 3, n = lane % 3;
        s.KR[lane] = (s.K[3 * i] * R[n] + s.K[3 * i + 1] * R[3 + n]) + s.K[3 * i + 2] * R[6 + n];
    }
    if (lane < PF_N) s.x[lane] = s.x[lane] + ((s.K[3 * lane] * y[0] + s.K[3 * lane + 1] * y[1]) + s.K[3 * lane + 2] * y[2]);
    // Joseph form: B = (I - K H) P, then P = B (I - K H)^T + K R K^T
    for (int e = lane; e < PF_NN; e += 64) {
        const int i = e / PF_N, j = e % PF_N;
        s.B[e] = s.P[e] - ((s.K[3 * i] * s.HP[j] + s.K[3 * i + 1] * s.HP[PF_N + j]) + s.K[3 * i + 2] * s.HP[2 * PF_N + j]);
    }
    __syncthreads();
    if (lane < 36) {
        const int i = lane / 3, n = lane % 3;
        s.BHt[lane] = ic < 0 ? s.B[i * PF_N + ia + n] : s.B[i * PF_N + ia + n] - s.B[i * PF_N + ic + n];
    }
    __syncthreads();
    for (int e = lane; e < PF_NN; e += 64) {
        const int i = e / PF_N, j = e % PF_N;
        const double bk = (s.BHt[3 * i] * s.K[3 * j] + s.BHt[3 * i + 1] * s.K[3 * j + 1]) + s.BHt[3 * i + 2] * s.K[3 * j + 2];
        const double kk = (s.KR[3 * i] * s.K[3 * j] + s.KR[3 * i + 1] * s.K[3 * j + 1]) + s.KR[3 * i + 2] * s.K[3 * j + 2];
        s.P[e] = (s.B[e] - bk) + kk;
    }
    __syncthreads();
    double sym[3];
    for (int e = lane, q = 0; e < PF_NN; e += 64, ++q) sym[q] = (s.P[e] + s.P[(e % PF_N) * PF_N + e / PF_N]) / 2.0;
    __syncthreads();
    for (int e = lane, q = 0; e < PF_NN; e += 64, ++q) s.P[e] = sym[q];
    __syncthreads();
    return OFK_POSF_APPLIED;
}

// Rules 1-8 of ofk.h for the streams b0 + blockIdx.x.  x [B][12], P [B][144], ist [B][OFK_POSF_INTS], rec [B][OFK_POSF_DOUBLES],
// input [B][OFK_POSF_INPUT] (read, then zeroed).
__global__ __launch_bounds__(64) void k_pos_filter_step(double *__restrict__ x_all, double *__restrict__ P_all, int *__restrict__ ist_all,
                                                        double *__restrict__ rec_all, double *__restrict__ in_all, pf_in in, pf_cfg cfg)
{
    __shared__ pf_lds s;
    const int b = blockIdx.x, lane = threadIdx.x;
    double *xg = x_all + (size_t)b * PF_N, *Pg = P_all + (size_t)b * PF_NN, *o = rec_all + (size_t)b * OFK_POSF_DOUBLES;
    double *ui = in_all + (size_t)b * OFK_POSF_INPUT;
    int *is = ist_all + (size_t)b * OFK_POSF_INTS;
    const double *vr = in.v + (size_t)b * OFK_RECORD_DOUBLES, *kr = in.key_rec + (size_t)b * OFK_KEY_DOUBLES;
    const double *rw = in.rw + (size_t)b * in.rw_stride;
    int cnt[OFK_POSF_INTS];
    for (int k = 0; k < OFK_POSF_INTS; ++k) cnt[k] = is[k];
    double u[OFK_POSF_INPUT];
    for (int k = 0; k < OFK_POSF_INPUT; ++k) u[k] = ui[k];
    const double du_l = lane >= 3 && lane < 6 ? ui[lane - 3] : 0.0;   // this lane's component of du
    const bool start = cnt[3] == 0;

    // 1. start
    if (start) {
        const double pp = cfg.p0_p * cfg.p0_p, pv = cfg.p0_v * cfg.p0_v, pb = cfg.p0_b * cfg.p0_b;
        for (int e = lane; e < PF_NN; e += 64) {
            const int i = e / PF_N, j = e % PF_N, bi = i / 3, bj = j / 3;
            double v = 0.0;
            if (i % 3 == j % 3) {
                if ((bi == 0 || bi == 3) && (bj == 0 || bj == 3)) v = pp;
                else if (bi == 1 && bj == 1) v = pv;
                else if (bi == 2 && bj == 2) v = pb;
            }
            s.P[e] = v;
        }
        if (lane < PF_N) s.x[lane] = lane < 3 ? xg[lane] : lane >= 9 ? xg[lane - 9] : 0.0;
        cnt[1] = 1; cnt[3] = 1;
    } else {
        for (int e = lane; e < PF_NN; e += 64) s.P[e] = Pg[e];
        if (lane < PF_N) s.x[lane] = xg[lane];
    }
    __syncthreads();

    // 2. predict: F's blocks are I and +-dt I, so P'_ij = (P_ij + f_i P_i+3,j) + f_j (P_i,j+3 + f_i P_i+3,j+3), f = dt, -dt, none
    {
        double pn[3];
        for (int e = lane, q = 0; e < PF_NN; e += 64, ++q) {
            const int i = e / PF_N, j = e % PF_N;
            const bool ri = i < 6, cj = j < 6;
            const double fi = i < 3 ? cfg.dt : -cfg.dt, fj = j < 3 ? cfg.dt : -cfg.dt;
            double g = ri ? s.P[e] + fi * s.P[e + 3 * PF_N] : s.P[e];
            if (cj) {
                const double g3 = ri ? s.P[e + 3] + fi * s.P[e + 3 * PF_N + 3] : s.P[e + 3];
                g = g + fj * g3;
            }
            if (i == j) { const double q0 = i < 3 ? cfg.q_p : i < 6 ? cfg.q_v : i < 9 ? cfg.q_b : 0.0; g = g + q0 * q0; }
            pn[q] = g;
        }
        double xn = 0.0;
        if (lane < 3) xn = s.x[lane] + cfg.dt * s.x[lane + 3];
        else if (lane < 6) { const double du = isfinite(du_l) ? du_l : 0.0; xn = (s.x[lane] + du) - cfg.dt * s.x[lane + 3]; }
        else if (lane < PF_N) xn = s.x[lane];
        __syncthreads();
        for (int e = lane, q = 0; e < PF_NN; e += 64, ++q) s.P[e] = pn[q];
        if (lane < PF_N) s.x[lane] = xn;
        __syncthreads();
    }

    int out[3] = {OFK_POSF_NOT, OFK_POSF_NOT, OFK_POSF_NOT};
    double nis[3] = {0.0, 0.0, 0.0}, yv[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};

    // 3. the velocity
    const bool solved = (in.plain ? vr[4] >= 3.0 : vr[15] != 0.0) && isfinite(vr[8]) && isfinite(vr[9]) && isfinite(vr[10]);
    if (cfg.sigma_v > 0.0 && solved) {
        const double r = cfg.sigma_v * cfg.sigma_v, z[3] = {vr[8], vr[9], vr[10]}, R[9] = {r, 0.0, 0.0, 0.0, r, 0.0, 0.0, 0.0, r};
        out[0] = pf_update(s, lane, 3, -1, z, R, cfg.nis_max, nis[0], yv[0]);
    }

    // 4. the displacement against the keyframe
    {
        bool ok = kr[3] == (double)OFK_KEY_SOLVED;
        for (int k = 0; k < 3; ++k) ok = ok && isfinite(kr[10 + k]);
        for (int k = 0; k < 6; ++k) ok = ok && isfinite(kr[20 + k]);
        for (int k = 0; k < 9; ++k) ok = ok && isfinite(rw[k]);
        if (ok) {
            const double ct[9] = {kr[20], kr[21], kr[22], kr[21], kr[23], kr[24], kr[22], kr[24], kr[25]};
            double M[9], Cm[9];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) M[3 * i + j] = (rw[3 * i] * ct[j] + rw[3 * i + 1] * ct[3 + j]) + rw[3 * i + 2] * ct[6 + j];
            const double i2 = cfg.infl * cfg.infl, f2 = cfg.floor * cfg.floor;
            for (int i = 0; i < 3; ++i)
                for (int j = i; j < 3; ++j) {
                    const double w = (M[3 * i] * rw[3 * j] + M[3 * i + 1] * rw[3 * j + 1]) + M[3 * i + 2] * rw[3 * j + 2];
                    Cm[3 * i + j] = Cm[3 * j + i] = i == j ? i2 * w + f2 : i2 * w;
                }
            if (cnt[1] != 0) {                                   // the key pixels' share: part of where the key is, once per keyframe
                __syncthreads();
                double cl = 0.0;
                for (int k = 0; k < 9; ++k) cl = lane == k ? Cm[k] : cl;
                if (lane < 9) { const int e = (9 + lane / 3) * PF_N + 9 + lane % 3; s.P[e] = s.P[e] + cfg.share * cl; }
                __syncthreads();
                cnt[1] = 0;
            }
            double R[9];
            for (int k = 0; k < 9; ++k) R[k] = (1.0 - cfg.share) * Cm[k];
            const double z[3] = {kr[10], kr[11], kr[12]};
            out[1] = pf_update(s, lane, 0, 9, z, R, cfg.nis_max, nis[1], yv[1]);
        }
    }

    // 5. the fix
    if (u[3] != 0.0 && isfinite(u[4]) && isfinite(u[5]) && isfinite(u[6]) && isfinite(u[7]) && isfinite(u[8]) && isfinite(u[9]) && u[7] > 0.0 &&
        u[8] > 0.0 && u[9] > 0.0) {
        const double z[3] = {u[4], u[5], u[6]}, R[9] = {u[7] * u[7], 0.0, 0.0, 0.0, u[8] * u[8], 0.0, 0.0, 0.0, u[9] * u[9]};
        out[2] = pf_update(s, lane, 0, -1, z, R, cfg.nis_max, nis[2], yv[2]);
    }

    // 7. the clone
    const bool clone = kr[9] != 0.0;
    if (clone) {
        double pn[3];
        __syncthreads();
        for (int e = lane, q = 0; e < PF_NN; e += 64, ++q) {
            const int i = e / PF_N, j = e % PF_N;
            pn[q] = s.P[(i >= 9 ? i - 9 : i) * PF_N + (j >= 9 ? j - 9 : j)];
        }
        const double xc = lane < 3 ? s.x[lane] : 0.0;
        __syncthreads();
        for (int e = lane, q = 0; e < PF_NN; e += 64, ++q) s.P[e] = pn[q];
        if (lane < 3) s.x[9 + lane] = xc;
        cnt[1] = 1; cnt[2] += 1;
    }
    __syncthreads();

    // 8. state and record
    cnt[0] += 1;
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) cnt[4 + 3 * k + j] += out[k] == j + 1 ? 1 : 0;
    for (int e = lane; e < PF_NN; e += 64) Pg[e] = s.P[e];
    if (lane < PF_N) { xg[lane] = s.x[lane]; o[lane] = s.x[lane]; ui[lane] = 0.0; }
    if (lane < OFK_POSF_INTS) is[lane] = cnt[lane];
    if (lane == 0) {
        int q = 12;
        for (int blk = 0; blk < 2; ++blk)
            for (int i = 0; i < 3; ++i)
                for (int j = i; j < 3; ++j) o[q++] = s.P[(3 * blk + i) * PF_N + 3 * blk + j];
        o[24] = (s.P[6 * PF_N + 6] + s.P[7 * PF_N + 7]) + s.P[8 * PF_N + 8];
        for (int k = 0; k < 3; ++k) {
            o[25 + 5 * k] = (double)out[k]; o[26 + 5 * k] = nis[k];
            for (int m = 0; m < 3; ++m) o[27 + 5 * k + m] = yv[k][m];
        }
        o[40] = clone ? 1.0 : 0.0; o[41] = (double)cnt[1]; o[42] = (double)cnt[0]; o[43] = (double)cnt[2];
        o[44] = (double)((cnt[4] + cnt[7]) + cnt[10]); o[45] = (double)((cnt[5] + cnt[8]) + cnt[11]); o[46] = (double)((cnt[6] + cnt[9]) + cnt[12]);
        o[47] = start ? 1.0 : 0.0;
    }
}

// beside ofk_stream_begin and the first step with the setting on (every stream, the position at zero), and ofk_pos_filter_reset (one
// stream b0 at the position p): not started, so that the next step applies rule 1 with the priors of its setting.  input NULL: the
// input rows are left alone.
__global__ __launch_bounds__(64) void k_pos_filter_clear(double *__restrict__ x_all, double *__restrict__ P_all, int *__restrict__ ist_all,
                                                         double *__restrict__ rec_all, double *__restrict__ in_all, int b0, double p0, double p1,
                                                         double p2)
{
    const int b = b0 + blockIdx.x, lane = threadIdx.x;
    if (!rows_stream_on(b, b0, gridDim.x, nullptr)) return;
    const int ax = lane < 3 ? lane : lane - 9;                  // the axis of a position slot
    const double pa = ax == 0 ? p0 : ax == 1 ? p1 : p2;
    for (int e = lane; e < PF_NN; e += 64) P_all[(size_t)b * PF_NN + e] = 0.0;
    if (lane < OFK_POSF_DOUBLES) rec_all[(size_t)b * OFK_POSF_DOUBLES + lane] = lane < 3 || (lane >= 9 && lane < 12) ? pa : lane == 41 ? 1.0 : 0.0;
    if (lane < PF_N) x_all[(size_t)b * PF_N + lane] = lane < 3 || lane >= 9 ? pa : 0.0;
    if (lane < OFK_POSF_INTS) ist_all[(size_t)b * OFK_POSF_INTS + lane] = lane == 1 ? 1 : 0;
    if (in_all && lane < OFK_POSF_INPUT) in_all[(size_t)b * OFK_POSF_INPUT + lane] = 0.0;
}

void ofk_launch_pos_filter_step(hipStream_t s, const ofk_pos_filter *f, double *x, double *P, int *ist, double *rec, double *input, const double *v,
                                int plain, const double *key_rec, const double *rw, int rw_stride, int batch)
{
    pf_cfg c;
    c.dt = f->dt; c.sigma_v = f->sigma_v; c.floor = f->floor; c.infl = f->infl; c.share = f->share; c.q_p = f->q_p; c.q_v = f->q_v; c.q_b = f->q_b;
    c.p0_p = f->p0_p; c.p0_v = f->p0_v; c.p0_b = f->p0_b; c.nis_max = f->nis_max;
    pf_in in;
    in.v = v; in.plain = plain; in.key_rec = key_rec; in.rw = rw; in.rw_stride = rw_stride;
    hipLaunchKernelGGL(k_pos_filter_step, dim3(batch), dim3(64), 0, s, x, P, ist, rec, input, in, c);
}

void ofk_launch_pos_filter_clear(hipStream_t s, double *x, double *P, int *ist, double *rec, double *input, int b0, const double *p, int batch)
{
    hipLaunchKernelGGL(k_pos_filter_clear, dim3(batch), dim3(64), 0, s, x, P, ist, rec, input, b0, p[0], p[1], p[2]);
}
