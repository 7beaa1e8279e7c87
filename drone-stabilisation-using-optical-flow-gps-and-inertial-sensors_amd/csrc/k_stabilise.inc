// k_stabilise.inc — the stabilised view of a video stream (ofk.h: ofk_set_stabilise): k_stab_pose turns the rigid motion the keyframe
// holds (R, T, the ground plane) into the pixel homography M that k_warp_u8 (k_warp.inc) resamples the step's new frame with, and keeps
// the view Bv continuous across re-keys.  Included by k_tracks.hip behind k_keyframe.inc (rule 1's kf_rotate is the keyframe's own).
// One thread per stream, all f64 in the order ofk.h states (the build has no FMA contraction); a stream's state is only touched by its
// own thread with plain vector stores, so a second launch on the same inputs gives the same bits.  One small launch per step.

struct stab_args {
    const double *R; int R_stride;                               // the rotation used (st_copy NULL): doubles between streams
    const double *st_copy;                                       // [B][OFK_KEY_STATE] in front of the keyframe's launch: R = rule 1's product
    const double *omega; int omega_stride;                       // ... with the omega the keyframe read
    const double *key_rec;                                       // [B][OFK_KEY_DOUBLES] behind the keyframe's launch
    const double *sensors;                                       // [B][OFK_SENSOR_DOUBLES]: d, scaling, cx, cy
    const double *normal; int normal_stride;                     // where the keyframe read n
    const int *cov;                                              // [B] covered pixels of the stream's previous warp (read where ist[3] != 0)
    double *Bv; int *ist; double *rec, *M;                       // [B][9], [B][OFK_STAB_INTS], [B][OFK_STAB_DOUBLES], [B][9]
    int mode, chain; double min_cover, hw;                       // hw = h w in f64
    int batch;
};

__device__ __forceinline__ void stab_mul3(const double *A, const double *B, double *C)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// M = K A K^-1, K = [[1/sc, 0, cx], [0, 1/sc, cy], [0, 0, 1]]; true where every entry is finite
__device__ __forceinline__ bool stab_pixels(const double *A, double sc, double cx, double cy, double *M)
{
    const double f = 1.0 / sc, kx = cx * sc, ky = cy * sc;
    double P[9];
    for (int j = 0; j < 3; ++j) { P[j] = f * A[j] + cx * A[6 + j]; P[3 + j] = f * A[3 + j] + cy * A[6 + j]; P[6 + j] = A[6 + j]; }
    bool fin = true;
    for (int i = 0; i < 3; ++i) {
        M[3 * i] = P[3 * i] * sc; M[3 * i + 1] = P[3 * i + 1] * sc; M[3 * i + 2] = P[3 * i + 2] - (P[3 * i] * kx + P[3 * i + 1] * ky);
        fin = fin && isfinite(M[3 * i]) && isfinite(M[3 * i + 1]) && isfinite(M[3 * i + 2]);
    }
    return fin;
}

__global__ __launch_bounds__(64) void k_stab_pose(stab_args a)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.batch) return;
    const double *kr = a.key_rec + (size_t)b * OFK_KEY_DOUBLES, *sn = a.sensors + (size_t)b * OFK_SENSOR_DOUBLES;
    const double *nn = a.normal + (size_t)b * a.normal_stride;
    double *Bv = a.Bv + (size_t)b * 9, *o = a.rec + (size_t)b * OFK_STAB_DOUBLES, *Mo = a.M + (size_t)b * 9;
    int *is = a.ist + (size_t)b * OFK_STAB_INTS;
    const double I3[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    // 1. the inputs
    double R[9], T[3];
    if (a.st_copy) {
        const double *om = a.omega + (size_t)b * a.omega_stride;
        kf_rotate(om[0], om[1], om[2], a.st_copy + (size_t)b * OFK_KEY_STATE, R);
    } else
        for (int k = 0; k < 9; ++k) R[k] = a.R[(size_t)b * a.R_stride + k];
    for (int k = 0; k < 3; ++k) T[k] = kr[k];
    const int kflag = (int)kr[3];
    const bool rekey = kr[9] != 0.0;
    // 2. the normalised homography, key to current
    const double n0 = nn[0], n1 = nn[1], n2 = nn[2], d = sn[0];
    const double den = d - ((n0 * T[0] + n1 * T[1]) + n2 * T[2]);
    bool fin = isfinite(den) && isfinite(n0) && isfinite(n1) && isfinite(n2) && isfinite(T[0]) && isfinite(T[1]) && isfinite(T[2]);
    for (int k = 0; k < 9; ++k) fin = fin && isfinite(R[k]);
    int flag = OFK_STAB_ROTATION_ONLY;
    if (kflag == OFK_KEY_NONE) flag = OFK_STAB_NONE;
    else if (a.mode == OFK_STAB_PLANE && kflag == OFK_KEY_SOLVED && fabs(den) >= 1e-12 && fin) flag = OFK_STAB_FULL;
    double G[9];
    if (flag == OFK_STAB_FULL) {
        const double nv[3] = {n0, n1, n2};
        double C[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) C[3 * i + j] = (i == j ? 1.0 : 0.0) + (T[i] * nv[j]) / den;
        stab_mul3(C, R, G);
    } else
        for (int k = 0; k < 9; ++k) G[k] = flag == OFK_STAB_NONE ? I3[k] : R[k];
    // 4. re-base, in front of rule 3
    const int prev = is[3] != 0 ? a.cov[b] : -1;
    int reason = 0;
    if (a.min_cover > 0.0 && prev >= 0 && (double)prev < a.min_cover * a.hw) reason = OFK_STAB_RB_COVER;
    double B0[9], A[9], M[9];
    for (int k = 0; k < 9; ++k) B0[k] = reason ? I3[k] : Bv[k];
    // 3. the view
    stab_mul3(G, B0, A);
    if (!stab_pixels(A, sn[19], sn[20], sn[21], M) && reason == 0) {
        reason = OFK_STAB_RB_FINITE;
        for (int k = 0; k < 9; ++k) B0[k] = I3[k];
        stab_mul3(G, B0, A);
        stab_pixels(A, sn[19], sn[20], sn[21], M);
    }
    int since = is[0], rebases = is[1], approx = is[2];
    if (reason) { since = 0; rebases += 1; } else since += 1;
    if (rekey && flag != OFK_STAB_FULL) approx += 1;
    for (int k = 0; k < 9; ++k) { Bv[k] = rekey ? (a.chain ? A[k] : I3[k]) : B0[k]; Mo[k] = M[k]; }
    is[0] = since; is[1] = rebases; is[2] = approx; is[3] = 1;
    for (int k = 0; k < 9; ++k) { o[k] = M[k]; o[9 + k] = Bv[k]; o[18 + k] = R[k]; }
    for (int k = 0; k < 3; ++k) o[27 + k] = T[k];
    o[30] = (double)flag; o[31] = (double)reason; o[32] = (double)since; o[33] = (double)rebases; o[34] = (double)approx;
    o[35] = rekey ? 1.0 : 0.0; o[36] = (double)prev;
    for (int k = 37; k < OFK_STAB_DOUBLES; ++k) o[k] = 0.0;
}

// the view of `batch` streams from b0 on back to the identity, counts zero, no previous warp (limit != NULL: only where limit[b] > 0,
// the counts staying); the record zero but for M = Bv = I
__global__ __launch_bounds__(64) void k_stab_clear(double *Bv, int *ist, double *rec, const int *__restrict__ limit, int b0, int batch)
{
    const int b = b0 + blockIdx.x * 64 + threadIdx.x;
    if (!rows_stream_on(b, b0, batch, limit)) return;
    for (int k = 0; k < 9; ++k) Bv[(size_t)b * 9 + k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    if (!limit) {
        for (int k = 0; k < OFK_STAB_INTS; ++k) ist[(size_t)b * OFK_STAB_INTS + k] = 0;
        double *o = rec + (size_t)b * OFK_STAB_DOUBLES;
        for (int k = 0; k < OFK_STAB_DOUBLES; ++k) o[k] = 0.0;
        o[0] = o[4] = o[8] = o[9] = o[13] = o[17] = 1.0; o[36] = -1.0;
    }
}

void ofk_launch_stab_pose(hipStream_t s, const ofk_stab_in &in, const ofk_stabilise *st, int h, int w, int batch)
{
    stab_args a;
    a.R = in.R; a.R_stride = in.R_stride; a.st_copy = in.st_copy; a.omega = in.omega; a.omega_stride = in.omega_stride;
    a.key_rec = in.key_rec; a.sensors = in.sensors; a.normal = in.normal; a.normal_stride = in.normal_stride; a.cov = in.cov;
    a.Bv = in.Bv; a.ist = in.ist; a.rec = in.rec; a.M = in.M;
    a.mode = st->mode; a.chain = st->chain; a.min_cover = st->min_cover; a.hw = (double)h * (double)w; a.batch = batch;
    hipLaunchKernelGGL(k_stab_pose, dim3((batch + 63) / 64), dim3(64), 0, s, a);
}

void ofk_launch_stab_clear(hipStream_t s, double *Bv, int *ist, double *rec, const int *limit, int b0, int batch)
{
    hipLaunchKernelGGL(k_stab_clear, dim3((batch + 63) / 64), dim3(64), 0, s, Bv, ist, rec, limit, b0, batch);
}
