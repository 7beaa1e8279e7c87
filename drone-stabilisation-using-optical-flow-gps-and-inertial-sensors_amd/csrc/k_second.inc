// k_second.inc — what the second-stage solves (k_cov.inc, k_joint.inc, k_plane.inc, k_epi.inc) share: everything around their cores.
// Included by k_estimate.hip ahead of the four.  Each solve runs in three launch forms behind whichever velocity solve ran, plain or
// robust, one team per problem:
//   stage entry   host arrays x, u, valid (k_solve / k_solve_robust ran); `out` holds the solve's eight doubles
//   pairs         resident points of a slice (k_pairs_solve[_wg] / k_pairs_robust ran); a single wave or a 256-thread workgroup
//   stream        a fused step (k_stream_fuse / k_stream_fuse_robust ran and, with fuse_args.defer, left the filter at its prediction)
// A form is: unpack the problem, hand the core a point source, write back.  The cores keep their own sums and finish functions.

// ---------------------------------------------------------------------------------------------------- the team's sums
// Four "virtual waves" take the points vw * 64 + lane + 256 k, each is reduced by the shuffle butterfly and the partial sums are added
// as (p0 + p1) + (p2 + p3), the solve kernels' own order: the records are the same bit for bit whether one wave (NW = 1) or four walk.
template <int NW> __device__ __forceinline__ void team_barrier()
{
    if (NW == 1) __builtin_amdgcn_wave_barrier(); else __syncthreads();
}

// virtual wave vw's K partial sums into its row (lane 0 stores)
template <int K> __device__ __forceinline__ void team_put(double *row, const double *s)
{
#pragma unroll
    for (int k = 0; k < K; ++k) { const double t = wave_sum(s[k]); if ((threadIdx.x & 63) == 0) row[k] = t; }
}

// behind team_put of every virtual wave: the K totals (thread 0 calls this behind the barrier)
template <int K, int S> __device__ __forceinline__ void team_sums(double (*part)[S], double *t)
{
    for (int k = 0; k < K; ++k) t[k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
}

// ---------------------------------------------------------------------------------------------------- point sources
// source(i, x, y, ux, uy, w) -> point i enters (the set the solve used), with its terms and its final robust weight (or 1).
struct stage_points {
    const double *x, *u, *w; const uint8_t *valid;
    __device__ __forceinline__ bool operator()(int i, double &px, double &py, double &ux, double &uy, double &wt) const
    {
        if (valid && !valid[i]) return false;
        wt = w ? w[i] : 1.0;
        if (!(wt > 0.0)) return false;
        px = x[2 * i]; py = x[2 * i + 1]; ux = u[2 * i]; uy = u[2 * i + 1];
        return true;
    }
};

// Resident points.  A stream step's `status` holds the keep flags by now: it passes use_feas 0 (fuse_terms' x, y, u of OFK_FLOW_LK).
struct resident_points {
    const float *pp, *np_; const uint8_t *st; const double *w;
    double nrm[3], vp[3], cx, cy, scaling, feas_T, d; int use_feas;
    __device__ __forceinline__ bool operator()(int i, double &x, double &y, double &ux, double &uy, double &wt) const
    {
        if (!st[i]) return false;
        wt = w ? w[i] : 1.0;
        if (!(wt > 0.0)) return false;
        return pair_point(pp, np_, i, cx, cy, scaling, use_feas, feas_T, nrm, vp, d, x, y, ux, uy);
    }
};

// ---------------------------------------------------------------------------------------------------- the problems
// Problem b of a stage entry.  vs: the solve's v (the record holds v - omega x t when t is given).  pts points into the struct.
struct stage_problem {
    int n; double d, nrm[3], om[3], rec03[4], rank, vs[3];
    const double *t;                                             // its lever arm, or NULL
    stage_points pts;
};

__device__ __forceinline__ void stage_unpack(stage_problem &q, int b, const double *x, const double *u, const uint8_t *valid, int n,
                                             const double *d, const double *nrm, const double *omega, const double *t, const double *weights,
                                             const double *out)
{
    q.n = n; q.d = d[b]; q.t = t ? t + 3 * b : nullptr;
    q.pts.x = x + (size_t)b * n * 2; q.pts.u = u + (size_t)b * n * 2;
    q.pts.valid = valid ? valid + (size_t)b * n : nullptr;
    q.pts.w = weights ? weights + (size_t)b * n : nullptr;
    const double *o = out + (size_t)b * OFK_SOLVE_DOUBLES;
    for (int k = 0; k < 3; ++k) { q.nrm[k] = nrm[3 * b + k]; q.om[k] = omega[3 * b + k]; }
    for (int k = 0; k < 4; ++k) q.rec03[k] = o[k];
    q.rank = o[4];
    q.vs[0] = q.rec03[0]; q.vs[1] = q.rec03[1]; q.vs[2] = q.rec03[2];
    if (t) {
        const double *tb = q.t, *ob = q.om;
        q.vs[0] += ob[1] * tb[2] - ob[2] * tb[1]; q.vs[1] += ob[2] * tb[0] - ob[0] * tb[2]; q.vs[2] += ob[0] * tb[1] - ob[1] * tb[0];
    }
}

// the stage entry's write-back: the solve's slots of `out`, v less omega x t where t is given
__device__ __forceinline__ void stage_write(const stage_problem &q, bool rw, const double *v, const double *om, double rss, double *o)
{
    if (!rw || threadIdx.x != 0) return;
    if (q.t) sub_cross(v, om, q.t, o);
    else { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }
    o[3] = rss;
}

// Problem b of the resident forms.  ist: the stream's IMU state where the step uses it (then normal, omega and R are its own).
// solved: record[15] of a stream step, true for pairs.
struct resident_problem {
    const double *sn, *R; double *ist;
    int n; double d, scaling, nrm[3], om[3], rec03[4], rank; bool solved;
    resident_points pts;
};

__device__ __forceinline__ void resident_unpack(resident_problem &q, int b, const float *prev_pts, const float *next_pts, const uint8_t *status,
                                                const int *counts, int pts_stride, const double *sensors, double *ist, bool stream,
                                                int use_feas, double feas_T, const double *weights, const double *records)
{
    const double *sn = sensors + (size_t)b * OFK_SENSOR_DOUBLES, *r = records + (size_t)b * OFK_RECORD_DOUBLES;
    q.sn = sn; q.ist = ist; q.R = ist ? ist + 6 : sn + 7;
    q.d = sn[0]; q.scaling = sn[19];
    for (int k = 0; k < 3; ++k) { q.nrm[k] = ist ? ist[15 + k] : sn[1 + k]; q.om[k] = ist ? ist[18 + k] : sn[4 + k]; }
    for (int k = 0; k < 4; ++k) q.rec03[k] = r[k];
    q.rank = r[4]; q.solved = stream ? r[15] != 0.0 : true;
    for (int k = 0; k < 3; ++k) { q.pts.nrm[k] = q.nrm[k]; q.pts.vp[k] = stream ? q.rec03[k] : sn[22 + k]; }
    q.n = min(max(counts[b], 0), pts_stride);
    q.pts.pp = prev_pts + (size_t)b * pts_stride * 2; q.pts.np_ = next_pts + (size_t)b * pts_stride * 2;
    q.pts.st = status + (size_t)b * pts_stride;
    q.pts.w = weights ? weights + (size_t)b * pts_stride : nullptr;
    q.pts.cx = sn[20]; q.pts.cy = sn[21]; q.pts.scaling = q.scaling; q.pts.d = q.d;
    q.pts.use_feas = use_feas; q.pts.feas_T = feas_T;
}

// The gyro's variances of a setting that has sigma_omega and omega_from_imu: the IMU state's where the setting asks for them and the
// step has one (ist), else the setting's own.
template <class Cfg> __device__ __forceinline__ void gyro_variances(const Cfg &cfg, const double *ist, double *ovar)
{
    for (int k = 0; k < 3; ++k) ovar[k] = cfg.omega_from_imu && ist ? ist[21 + k] : cfg.so[k] * cfg.so[k];
}

__device__ __forceinline__ void stream_unpack(resident_problem &q, int b, const fuse_args &g, const double *weights)
{
    resident_unpack(q, b, g.prev_pts, g.next_pts, g.status, g.counts, g.pts_stride, g.sensors,
                    g.f.use_imu && g.imu_state ? g.imu_state + (size_t)b * OFK_IMU_STATE : nullptr, true, 0, 0.0, weights, g.records);
}

// ---------------------------------------------------------------------------------------------------- write-backs (thread 0)
// the record's slots a second-stage solve rewrites: v, rss and v_uav (vu) from v and the omega the solve ended with
__device__ __forceinline__ void record_write(const resident_problem &q, const double *v, const double *om, double rss, double *r, double *vu)
{
    lever_rotate(v, om, q.sn + 16, q.R, vu);
    r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = rss; r[8] = vu[0]; r[9] = vu[1]; r[10] = vu[2];
}

__device__ __forceinline__ void pairs_write(const resident_problem &q, bool rw, const double *v, const double *om, double rss, double *r)
{
    double vu[3];
    if (rw && threadIdx.x == 0) record_write(q, v, om, rss, r, vu);
}

// The filter's correct that the fused kernel deferred, around the caller's own correct (which runs where q.solved).  First the state
// and the measurement, read from the record as it stands now ...
__device__ __forceinline__ void deferred_load(const fuse_args &g, const resident_problem &q, int b, const double *r, double *kx,
                                              double (*kP)[KF_MAX], double *z)
{
    kf_load(g.ns, b, g.kf_x, g.kf_P, kx, kP);
    for (int k = 0; k < KF_MAX; ++k) z[k] = 0.0;
    if (!q.solved) return;
    for (int k = 0; k < 3; ++k) z[k] = g.f.z_sign * r[(g.f.z_source ? 8 : 0) + k];
    for (int k = 3; k < g.nm; ++k) z[k] = q.sn[22 + (k - 3)];
}

// ... then the state back where the step solved, and fused[0..7] rewritten.
__device__ __forceinline__ void deferred_store(const fuse_args &g, const resident_problem &q, int b, const double *kx, const double (*kP)[KF_MAX])
{
    if (q.solved) kf_store(g.ns, b, kx, kP, g.kf_x, g.kf_P);
    double *fu = g.fused + (size_t)b * 8, tr = 0.0;
    for (int i = 0; i < g.ns; ++i) tr += kP[i][i];
    for (int k = 0; k < 6; ++k) fu[k] = k < g.ns ? kx[k] : 0.0;
    fu[6] = tr; fu[7] = q.solved ? 1.0 : 0.0;
}

// The stream step's tail behind a solve that rewrites the record: the correct runs here with the refined v / v_uav (the solve's own
// where the record was left alone), and vel_overwrite is repeated with the refined v_uav.
__device__ __forceinline__ void stream_tail(const fuse_args &g, const resident_problem &q, int b, bool rw, const double *v, const double *om,
                                            double rss)
{
    if (threadIdx.x != 0) return;
    double *r = g.records + (size_t)b * OFK_RECORD_DOUBLES, *ist = q.ist;
    double vu[3] = {r[8], r[9], r[10]};
    if (rw) record_write(q, v, om, rss, r, vu);
    if (g.f.filter && g.defer) {
        double kx[KF_MAX], kP[KF_MAX][KF_MAX], z[KF_MAX];
        deferred_load(g, q, b, r, kx, kP, z);
        if (q.solved) kf_correct_dev(g.ns, g.nm, g.H, g.Rm, z, kx, kP);
        deferred_store(g, q, b, kx, kP);
    } else if (!g.f.filter && rw) {
        double *fu = g.fused + (size_t)b * 8;
        fu[0] = vu[0]; fu[1] = vu[1]; fu[2] = vu[2];
    }
    if (g.f.vel_overwrite && q.solved && ist && rw) { ist[0] = vu[0]; ist[1] = vu[1]; ist[2] = vu[2]; }   // node:261
}

// ---------------------------------------------------------------------------------------------------- launches
// ofk_launch_pairs_solve's rule and reason: a single wave finds room beside the other slice's kernels, a small batch has the chip to itself
template <class K, class... A> static void launch_pairs_form(hipStream_t s, int batch, K wave_form, K workgroup_form, A... args)
{
    if (batch >= 128) hipLaunchKernelGGL(wave_form, dim3(batch), dim3(64), 0, s, args...);
    else hipLaunchKernelGGL(workgroup_form, dim3(batch), dim3(256), 0, s, args...);
}
