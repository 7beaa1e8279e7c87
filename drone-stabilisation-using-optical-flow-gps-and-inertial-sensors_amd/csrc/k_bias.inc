// k_bias.inc — the gyro bias of a stream (ofk.h: ofk_set_gyro_bias): filtered from the flow, taken out of omega in front of every step.
// Included by k_estimate.hip behind k_joint.inc, whose core (joint_core), k_lstsq.inc's joint_inverse and k_second.inc's shells it shares.
// DESIGN.md, "gyro bias", has the model.
//
// k_gyro_bias_apply  one thread per stream, directly behind the sensors' upload: raw omega into the bias record, omega - b^ into the
//                    device copy of the sensor rows (and the IMU state's slots 18-20); restore != 0: the IMU state's raw bits back.
// k_stream_bias      one 256-thread workgroup per stream behind the solve kernel: joint_core without its second walk over the joint
//                    solve's point set, then thread 0's filter step.  k_bias_solve is the same over a stage entry's arrays.
// The kernels write the bias record and nothing else of a step's outputs.  No atomics, vector stores only.
struct bias_cfg { double sf, sg2, q, nis_max; int est[3]; };

static bias_cfg bias_make_cfg(const ofk_gyro_bias *g)
{
    bias_cfg bc;
    bc.sf = g->sigma_flow; bc.sg2 = g->sigma_gyro * g->sigma_gyro; bc.q = g->q; bc.nis_max = g->nis_max;
    for (int k = 0; k < 3; ++k) bc.est[k] = g->p0[k] > 0.0 ? 1 : 0;
    return bc;
}

// omega: the first stream's three values, `stride` doubles between streams (sensor rows: slot 4, OFK_SENSOR_DOUBLES; a stage entry: 3)
__global__ void k_gyro_bias_apply(double *__restrict__ omega, int stride, double *__restrict__ imu_state, double *__restrict__ bias, int batch,
                                  int restore)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double *r = bias + (size_t)b * OFK_BIAS_DOUBLES, *ist = imu_state ? imu_state + (size_t)b * OFK_IMU_STATE + 18 : nullptr;
    if (restore) {
        if (ist) for (int k = 0; k < 3; ++k) ist[k] = r[9 + k];
        return;
    }
    double *om = omega + (size_t)b * stride;
    for (int k = 0; k < 3; ++k) {
        const double raw = ist ? ist[k] : om[k], used = raw - r[k];
        r[9 + k] = raw; r[12 + k] = used;
        if (ist) ist[k] = used;
        om[k] = om[k] - r[k];
        r[15 + k] = 0.0;
    }
    r[18] = 4.0; r[19] = 0.0; r[21] = r[21] + 1.0;
    for (int k = 22; k < OFK_BIAS_DOUBLES; ++k) r[k] = 0.0;
}

void ofk_launch_gyro_bias_apply(hipStream_t s, double *omega, int stride, double *imu_state, double *bias, int batch, int restore)
{
    hipLaunchKernelGGL(k_gyro_bias_apply, dim3((batch + 63) / 64), dim3(64), 0, s, omega, stride, imu_state, bias, batch, restore);
}

// Thread 0, behind joint_core: the filter step of ofk.h on the core's record jr.  r: the stream's bias record, state in slots 0-8.
__device__ void bias_filter(const bias_cfg &c, const double *jr, double *r)
{
    double bh[3] = {r[0], r[1], r[2]};
    double P[3][3]; sym3_from6(r + 3, P);
    int ne = 0;
    for (int k = 0; k < 3; ++k)
        if (c.est[k]) { P[k][k] += c.q; ++ne; }
    r[3] = P[0][0]; r[6] = P[1][1]; r[8] = P[2][2];                                          // the prediction stands whatever follows
    r[28] = jr[11];
    const int core = (int)jr[10];
    if (core != 0) { r[18] = (double)core; return; }
    double z[3], S[3][3], Rm[3][3], Cw[3][3]; sym3_from6(jr + 15, Cw);
    bool fin = true;
    for (int i = 0; i < 3; ++i) {
        z[i] = c.est[i] ? -jr[3 + i] : 0.0;
        for (int j = 0; j < 3; ++j) {
            const bool in = c.est[i] && c.est[j];
            Rm[i][j] = in ? Cw[i][j] + (i == j ? c.sg2 : 0.0) : 0.0;
            S[i][j] = in ? P[i][j] + Rm[i][j] : 0.0;
            fin = fin && isfinite(S[i][j]);
        }
    }
    if (!fin) { r[18] = 2.0; return; }
    double Sc[3][3], ls[3], W[3][3], Si[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Sc[i][j] = S[i][j];
    jacobi3(Sc, ls, W);
    for (int k = 0; k < ne; ++k)
        if (!(ls[k] > 0.0)) { r[18] = 2.0; return; }
    joint_inverse(ls, W, ne, Si);
    double t[3], nis = 0.0;
    for (int i = 0; i < 3; ++i) t[i] = Si[i][0] * z[0] + Si[i][1] * z[1] + Si[i][2] * z[2];
    for (int i = 0; i < 3; ++i) nis += z[i] * t[i];
    if (!isfinite(nis)) { r[18] = 2.0; return; }
    r[19] = nis;
    r[22] = Rm[0][0]; r[23] = Rm[0][1]; r[24] = Rm[0][2]; r[25] = Rm[1][1]; r[26] = Rm[1][2]; r[27] = Rm[2][2];
    if (c.nis_max > 0.0 && !(nis <= c.nis_max)) { r[18] = 3.0; return; }
    double K[3][3], T[3][3], Pn[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) K[i][j] = P[i][0] * Si[0][j] + P[i][1] * Si[1][j] + P[i][2] * Si[2][j];
    // P - P S^-1 P = R S^-1 P: a product, where the difference cancels once P is large against R.  T = S^-1 P; rows and columns of
    // held axes keep P's own values
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T[i][j] = Si[i][0] * P[0][j] + Si[i][1] * P[1][j] + Si[i][2] * P[2][j];
    for (int i = 0; i < 3; ++i) {
        bh[i] += K[i][0] * z[0] + K[i][1] * z[1] + K[i][2] * z[2];
        for (int j = 0; j < 3; ++j)
            Pn[i][j] = c.est[i] && c.est[j] ? Rm[i][0] * T[0][j] + Rm[i][1] * T[1][j] + Rm[i][2] * T[2][j] : P[i][j];
    }
    for (int k = 0; k < 3; ++k) { r[k] = bh[k]; r[15 + k] = jr[3 + k]; }
    r[3] = Pn[0][0]; r[4] = (Pn[0][1] + Pn[1][0]) / 2.0; r[5] = (Pn[0][2] + Pn[2][0]) / 2.0;
    r[6] = Pn[1][1]; r[7] = (Pn[1][2] + Pn[2][1]) / 2.0; r[8] = Pn[2][2];
    r[18] = 0.0; r[20] = r[20] + 1.0;
}

// the prior variances the core takes: free where the axis is estimated, held elsewhere
__device__ __forceinline__ void bias_variances(const bias_cfg &c, double *ovar)
{
    for (int k = 0; k < 3; ++k) ovar[k] = c.est[k] ? INFINITY : 0.0;
}

// fused: a fused step's kernel ran (the status holds the keep flags, the record its solved flag, under use_imu the IMU state's normal
// and omega); else the plain step's k_pairs_solve / k_pairs_robust (status and the feasibility rule of g.use_feas / g.feas_T).
__global__ __launch_bounds__(256) void k_stream_bias(fuse_args g, int fused, const double *__restrict__ weights, bias_cfg c,
                                                     double *__restrict__ bias)
{
    __shared__ double part[4][JOINT_SUMS];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    resident_problem q;
    if (fused) stream_unpack(q, b, g, weights);
    else resident_unpack(q, b, g.prev_pts, g.next_pts, g.status, g.counts, g.pts_stride, g.sensors, nullptr, false, g.use_feas, g.feas_T, weights,
                         g.records);
    double ovar[3], v[3], omh[3], rss, jr[OFK_JOINT_DOUBLES];
    bias_variances(c, ovar);
    const double dsf = q.d * c.sf * q.scaling;
    joint_core<4, false>(part, bc, q.n, g.variant, q.nrm, q.om, q.d, q.rec03, q.rec03, q.solved && q.rank >= 3.0 && q.scaling != 0.0 && q.d != 0.0,
                         dsf * dsf, ovar, jr, v, omh, rss, q.pts);
    if (threadIdx.x == 0) bias_filter(c, jr, bias + (size_t)b * OFK_BIAS_DOUBLES);
}

void ofk_launch_stream_bias(hipStream_t s, const ofk_stream_in &in, int fused, int use_feas, double feas_T, const double *weights,
                            const ofk_gyro_bias *g, double *bias)
{
    hipLaunchKernelGGL(k_stream_bias, dim3(in.batch), dim3(256), 0, s, make_fuse_args(in, nullptr, use_feas, feas_T), fused, weights,
                       bias_make_cfg(g), bias);
}

__global__ __launch_bounds__(256) void k_bias_solve(int variant, const double *__restrict__ x, const double *__restrict__ u,
                                                    const uint8_t *__restrict__ valid, int n, const double *__restrict__ d,
                                                    const double *__restrict__ nrm, const double *__restrict__ omega,
                                                    const double *__restrict__ weights, bias_cfg c, const double *__restrict__ out,
                                                    double *__restrict__ bias)
{
    __shared__ double part[4][JOINT_SUMS];
    __shared__ double bc[8];
    const int b = blockIdx.x;
    stage_problem q;
    stage_unpack(q, b, x, u, valid, n, d, nrm, omega, nullptr, weights, out);
    double ovar[3], v[3], omh[3], rss, jr[OFK_JOINT_DOUBLES];
    bias_variances(c, ovar);
    joint_core<4, false>(part, bc, n, variant, q.nrm, q.om, q.d, q.vs, q.rec03, q.rank >= 3.0 && q.d != 0.0, (q.d * c.sf) * (q.d * c.sf), ovar, jr,
                         v, omh, rss, q.pts);
    if (threadIdx.x == 0) bias_filter(c, jr, bias + (size_t)b * OFK_BIAS_DOUBLES);
}

void ofk_launch_bias_solve(hipStream_t s, const ofk_stage_in &in, const double *weights, const ofk_gyro_bias *g, const double *out, double *bias)
{
    hipLaunchKernelGGL(k_bias_solve, dim3(in.batch), dim3(256), 0, s, in.variant, in.x, in.u, in.valid, in.n, in.d, in.nrm, in.omega, weights,
                       bias_make_cfg(g), out, bias);
}
