// k_keyframe.inc — the keyframe of a video stream (ofk.h: ofk_set_keyframe): per row of the track table the row's ideal pixel in a frame
// that is held fixed, per stream the rotation accumulated since, and every step the translation against that frame from finite
// motion's exact relation, solved through the solve's own sums, Jacobi and rank rule.  Included by k_tracks.hip behind k_lstsq.inc.
// The rows and the state of one stream are only ever touched by that stream's workgroup, with plain vector stores and no atomics, so
// a second launch on the same inputs gives the same bits.  All arithmetic is f64 in the order ofk.h states (the build has no FMA
// contraction).  One latency-bound launch per step over a few hundred rows: it is not tuned beyond the launch count.

struct kf_cfg { double sf, gate, min_share, rot_max; int min_rows, max_age; };

__device__ __forceinline__ void kf_clear_state(const ofk_kf_rows &t, int b, int tid, bool pos_too)
{
    double *st = t.st + (size_t)b * OFK_KEY_STATE;
    int *is = t.ist + (size_t)b * OFK_KEY_INTS;
    if (pos_too) {
        if (tid < OFK_KEY_STATE) st[tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.0 : 0.0;
        if (tid < OFK_KEY_INTS) is[tid] = 0;
        if (tid < OFK_KEY_DOUBLES) t.rec[(size_t)b * OFK_KEY_DOUBLES + tid] = tid == 3 ? (double)OFK_KEY_NONE : 0.0;
    } else if (tid == 0)
        is[1] = 0;
}

// the rows of freshly detected tracks (beside k_track_table_begin): no members, no keyframe, the position at zero
__global__ __launch_bounds__(256) void k_keyframe_begin(ofk_kf_rows t, const int *__restrict__ counts, int stride)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[b], 0), stride);
    const size_t base = (size_t)b * stride;
    for (int i = tid; i < n; i += 256) { t.key_xy[2 * (base + i)] = 0.f; t.key_xy[2 * (base + i) + 1] = 0.f; t.member[base + i] = 0; }
    kf_clear_state(t, b, tid, true);
}

// behind k_replace_tracks (beside k_track_table_replace): the streams with a budget lose their keyframe and keep their position
__global__ __launch_bounds__(256) void k_keyframe_replace(ofk_kf_rows t, const int *__restrict__ limit, const int *__restrict__ new_counts,
                                                          int stride)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    if (limit[b] <= 0) return;
    const int n = min(max(new_counts[b], 0), stride);
    const size_t base = (size_t)b * stride;
    for (int i = tid; i < n; i += 256) { t.key_xy[2 * (base + i)] = 0.f; t.key_xy[2 * (base + i) + 1] = 0.f; t.member[base + i] = 0; }
    kf_clear_state(t, b, tid, false);
}

// ofk_keyframe_reset: stream b starts over at the position p
__global__ __launch_bounds__(256) void k_keyframe_reset(ofk_kf_rows t, int b, int stride, double p0, double p1, double p2)
{
    const int tid = threadIdx.x;
    const size_t base = (size_t)b * stride;
    for (int i = tid; i < stride; i += 256) t.member[base + i] = 0;
    double *st = t.st + (size_t)b * OFK_KEY_STATE, *o = t.rec + (size_t)b * OFK_KEY_DOUBLES;
    int *is = t.ist + (size_t)b * OFK_KEY_INTS;
    if (tid < 9) st[tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.0 : 0.0;
    if (tid == 0) {                                              // the record of a stream without a keyframe: nothing of the last step stays
        const double p[3] = {p0, p1, p2};
        for (int k = 0; k < OFK_KEY_DOUBLES; ++k) o[k] = 0.0;
        for (int k = 0; k < 3; ++k) { st[9 + k] = p[k]; st[12 + k] = p[k]; o[13 + k] = p[k]; o[16 + k] = p[k]; }
        is[1] = 0;
        o[3] = (double)OFK_KEY_NONE; o[8] = (double)is[0]; o[26] = (double)is[2]; o[27] = (double)is[3];
    }
}

// what rule 2 needs of one stream, the same in every thread
struct kf_frame { double R[9], n0, n1, n2, d, cx, cy, sc; };

// Rule 2's terms of row r; false: the row is left out
__device__ __forceinline__ bool kf_row(const ofk_kf_rows &t, const float *__restrict__ next, size_t r, const kf_frame &f, double &a, double &b,
                                       double &u0, double &u1, double &sA)
{
    const double kx = ((double)t.key_xy[2 * r] - f.cx) * f.sc, ky = ((double)t.key_xy[2 * r + 1] - f.cy) * f.sc;
    const double px = ((double)next[2 * r] - f.cx) * f.sc, py = ((double)next[2 * r + 1] - f.cy) * f.sc;
    const double X = (f.R[0] * kx + f.R[1] * ky) + f.R[2], Y = (f.R[3] * kx + f.R[4] * ky) + f.R[5], Z = (f.R[6] * kx + f.R[7] * ky) + f.R[8];
    const double den = (f.n0 * px + f.n1 * py) + f.n2;
    if (!(Z >= OFK_KEY_MIN_DEPTH) || !(fabs(den) >= 1e-12)) return false;
    a = X / Z; b = Y / Z;
    const double nq = (f.n0 * a + f.n1 * b) + f.n2, s = nq / den;
    if (!(s > 0.0)) return false;
    u0 = s * (px - a); u1 = s * (py - b); sA = nq / f.d;
    return true;
}

__device__ __forceinline__ double kf_res2(double a, double b, double u0, double u1, double sA, const double *T)
{
    const double r0 = u0 - sA * (T[0] - T[2] * a), r1 = u1 - sA * (T[1] - T[2] * b);
    return r0 * r0 + r1 * r1;
}

// Rules 1-5 of ofk.h.  One workgroup per stream; every thread holds the stream's sums behind acc_block_sum and solves the 3 x 3 itself,
// so that the gate and the residual need no broadcast.  The compaction is the table's: a chunk of 256 rows is read completely before
// any of its rows is written, and a row only moves to a position <= its own.  Thread 0 writes the state and the record at the end;
// nothing reads them behind the first barrier.
__global__ __launch_bounds__(256) void k_keyframe_step(ofk_kf_rows t, ofk_kf_in in, kf_cfg cfg)
{
    __shared__ int s_wave[4];
    __shared__ int s_base;
    __shared__ double s_red[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(in.counts[b], 0), in.stride);
    const size_t base = (size_t)b * in.stride;
    const double *sn = in.sensors + (size_t)b * OFK_SENSOR_DOUBLES;
    const double *ist = in.imu ? in.imu + (size_t)b * OFK_IMU_STATE : nullptr;
    const double *rw = ist ? ist + 6 : sn + 7, *vr = in.v + (size_t)b * OFK_RECORD_DOUBLES;
    double *st = t.st + (size_t)b * OFK_KEY_STATE;
    int *is = t.ist + (size_t)b * OFK_KEY_INTS;
    const int key_step = is[0], mk = is[1], nkey = is[2], ndead = is[3], step = in.step[(size_t)b * in.step_stride];
    const double o0 = ist ? ist[18] : sn[4], o1 = ist ? ist[19] : sn[5], o2 = ist ? ist[20] : sn[6];
    double R0[9], anchor[3], pos[3];
    for (int k = 0; k < 9; ++k) R0[k] = st[k];
    for (int k = 0; k < 3; ++k) { anchor[k] = st[9 + k]; pos[k] = st[12 + k]; }
    kf_frame f;
    f.n0 = ist ? ist[15] : sn[1]; f.n1 = ist ? ist[16] : sn[2]; f.n2 = ist ? ist[17] : sn[3];
    f.d = sn[0]; f.sc = sn[19]; f.cx = sn[20]; f.cy = sn[21];

    // 1. rotate
    {
        const double th2 = (o0 * o0 + o1 * o1) + o2 * o2;
        double A = 1.0, B = 0.5;
        if (!(th2 < 1e-16)) { const double th = sqrt(th2); A = sin(th) / th; B = (1.0 - cos(th)) / th2; }
        const double om[3] = {o0, o1, o2};
        const double K[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
        double E[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double k2 = om[i] * om[j] - (i == j ? th2 : 0.0);
                E[3 * i + j] = ((i == j ? 1.0 : 0.0) + A * K[3 * i + j]) + B * k2;
            }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) f.R[3 * i + j] = (E[3 * i] * R0[j] + E[3 * i + 1] * R0[3 + j]) + E[3 * i + 2] * R0[6 + j];
    }
    const double cs = (((f.R[0] + f.R[4]) + f.R[8]) - 1.0) / 2.0;
    const double angle = acos(fmin(1.0, fmax(-1.0, cs)));

    // 2. the key solve
    Acc a1; acc_zero(a1);
    double live_d = 0.0;
    for (int i = tid; i < n; i += 256) {
        const size_t r = base + i;
        if (in.status[r] != 0 && t.member[r] != 0) {
            live_d += 1.0;
            double a, bb, u0, u1, sA;
            if (mk != 0 && kf_row(t, in.next_pts, r, f, a, bb, u0, u1, sA)) acc_point(a1, a, bb, u0, u1, 0.0, sA, 1.0);
        }
    }
    const int live = (int)block_sum(live_d, s_red);
    acc_block_sum(a1);
    double T[3] = {0.0, 0.0, 0.0}, s3[3];
    bool fin = true;
    int flag = mk == 0 ? OFK_KEY_NONE : OFK_KEY_UNSOLVED;
    if (mk != 0 && a1.cnt >= (double)cfg.min_rows && solve_from_acc(a1, T, s3, fin) == 3 && fin) flag = OFK_KEY_SOLVED;
    Acc as = a1;                                                 // the sums of the solve that stands
    const double T1[3] = {T[0], T[1], T[2]};                     // the gate is the first solve's, whichever stands
    double rows2 = 0.0;
    bool gated = false;
    const double sf = cfg.sf * f.sc, gs = cfg.gate * f.sc, g2 = gs * gs;
    if (flag == OFK_KEY_SOLVED && cfg.gate > 0.0) {              // uniform over the workgroup
        Acc a2; acc_zero(a2);
        for (int i = tid; i < n; i += 256) {
            const size_t r = base + i;
            double a, bb, u0, u1, sA;
            if (in.status[r] != 0 && t.member[r] != 0 && kf_row(t, in.next_pts, r, f, a, bb, u0, u1, sA) && kf_res2(a, bb, u0, u1, sA, T) <= g2)
                acc_point(a2, a, bb, u0, u1, 0.0, sA, 1.0);
        }
        acc_block_sum(a2);
        rows2 = a2.cnt;
        double T2[3], s32[3];
        bool fin2 = true;
        if (a2.cnt >= (double)cfg.min_rows && solve_from_acc(a2, T2, s32, fin2) == 3 && fin2) {
            gated = true; as = a2; T[0] = T2[0]; T[1] = T2[1]; T[2] = T2[2];
        }
    }
    double rms = 0.0;
    if (flag == OFK_KEY_SOLVED) {
        double ss = 0.0;
        for (int i = tid; i < n; i += 256) {
            const size_t r = base + i;
            double a, bb, u0, u1, sA;
            if (in.status[r] != 0 && t.member[r] != 0 && kf_row(t, in.next_pts, r, f, a, bb, u0, u1, sA) &&
                (!gated || kf_res2(a, bb, u0, u1, sA, T1) <= g2))
                ss += kf_res2(a, bb, u0, u1, sA, T);
        }
        ss = block_sum(ss, s_red);
        rms = sqrt(ss / as.cnt) / f.sc;
    } else
        T[0] = T[1] = T[2] = 0.0;

    // 3. the position
    const bool solved = (in.plain ? vr[4] >= 3.0 : vr[15] != 0.0) && isfinite(vr[8]) && isfinite(vr[9]) && isfinite(vr[10]);
    double D[3];
    if (flag == OFK_KEY_SOLVED) {
        const double *off = sn + 16;
        double w[3];
        for (int i = 0; i < 3; ++i) w[i] = T[i] + (off[i] - ((f.R[3 * i] * off[0] + f.R[3 * i + 1] * off[1]) + f.R[3 * i + 2] * off[2]));
        for (int i = 0; i < 3; ++i) D[i] = (rw[3 * i] * w[0] + rw[3 * i + 1] * w[1]) + rw[3 * i + 2] * w[2];
        if (isfinite(D[0]) && isfinite(D[1]) && isfinite(D[2]))
            for (int i = 0; i < 3; ++i) pos[i] = anchor[i] + D[i];
        else {                                                   // a lever arm or an R_world that is no number: the solve does not stand
            flag = OFK_KEY_UNSOLVED; gated = false; rms = 0.0; T[0] = T[1] = T[2] = 0.0;
        }
    }
    if (flag != OFK_KEY_SOLVED)
        for (int i = 0; i < 3; ++i) { if (solved) pos[i] = pos[i] + vr[8 + i]; D[i] = pos[i] - anchor[i]; }

    // 4. the re-key decision
    int bits = 0;
    if (flag != OFK_KEY_SOLVED) bits |= 1;
    if (live < cfg.min_rows) bits |= 2;
    if ((double)live < cfg.min_share * (double)mk) bits |= 4;
    if (angle > cfg.rot_max) bits |= 8;
    if (cfg.max_age > 0 && (step + 1) - key_step > cfg.max_age) bits |= 16;
    const bool rekey = bits != 0;
    const int reason = bits ? __ffs(bits) : 0;

    // 5. compaction
    if (tid == 0) s_base = 0;
    __syncthreads();                                            // also: every thread has read the state
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool inside = i < n;
        const size_t r = base + (inside ? i : 0);
        const bool keep = inside && in.status[r] != 0;
        float kx = t.key_xy[2 * r], ky = t.key_xy[2 * r + 1];
        uint8_t m = t.member[r];
        if (rekey) { kx = in.next_pts[2 * r]; ky = in.next_pts[2 * r + 1]; m = 1; }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int q = 0; q < wave; ++q) off += s_wave[q];
        const int p = off + __popcll(bal & ((1ull << lane) - 1));
        __syncthreads();                                        // every thread has read the rows of this chunk: safe to overwrite
        if (keep) { const size_t w = base + p; t.key_xy[2 * w] = kx; t.key_xy[2 * w + 1] = ky; t.member[w] = m; }
        if (tid == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    const int kept = s_base;
    const int extra = in.new_counts ? max(0, min(min(in.new_counts[b], in.max_total - kept), in.stride - kept)) : 0;
    for (int i = tid; i < extra; i += 256) { const size_t w = base + kept + i; t.key_xy[2 * w] = 0.f; t.key_xy[2 * w + 1] = 0.f; t.member[w] = 0; }
    if (tid == 0) {
        double *o = t.rec + (size_t)b * OFK_KEY_DOUBLES;
        for (int k = 0; k < OFK_KEY_DOUBLES; ++k) o[k] = 0.0;
        if (flag == OFK_KEY_SOLVED) {
            double A[3][3] = {{as.m00, as.m01, as.m02}, {as.m01, as.m11, as.m12}, {as.m02, as.m12, as.m22}}, lam[3], V[3][3];
            jacobi3(A, lam, V);
            const double sf2 = sf * sf;
            int s = 20;
            for (int i = 0; i < 3; ++i)
                for (int j = i; j < 3; ++j)
                    o[s++] = sf2 * ((V[i][0] * V[j][0] / lam[0] + V[i][1] * V[j][1] / lam[1]) + V[i][2] * V[j][2] / lam[2]);
        }
        const int mk_out = rekey ? kept : mk, ks_out = rekey ? step + 1 : key_step, nkey_out = nkey + (rekey ? 1 : 0);
        const int ndead_out = ndead + (flag != OFK_KEY_SOLVED ? 1 : 0);
        if (rekey) for (int k = 0; k < 3; ++k) anchor[k] = pos[k];
        for (int k = 0; k < 9; ++k) st[k] = rekey ? ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0) : f.R[k];
        for (int k = 0; k < 3; ++k) { st[9 + k] = anchor[k]; st[12 + k] = pos[k]; }
        is[0] = ks_out; is[1] = mk_out; is[2] = nkey_out; is[3] = ndead_out;
        o[0] = T[0]; o[1] = T[1]; o[2] = T[2]; o[3] = (double)flag; o[4] = a1.cnt; o[5] = rows2; o[6] = rms;
        o[7] = (double)mk_out; o[8] = (double)ks_out; o[9] = (double)reason;
        for (int k = 0; k < 3; ++k) { o[10 + k] = D[k]; o[13 + k] = pos[k]; o[16 + k] = anchor[k]; }
        o[19] = angle; o[26] = (double)nkey_out; o[27] = (double)ndead_out; o[28] = (double)live; o[29] = gated ? 1.0 : 0.0;
        o[30] = (double)bits;
    }
}

static kf_cfg kf_make_cfg(const ofk_keyframe *k)
{
    kf_cfg c;
    c.sf = k->sigma_flow; c.gate = k->gate; c.min_share = k->min_share; c.rot_max = k->rot_max; c.min_rows = k->min_rows; c.max_age = k->max_age;
    return c;
}

void ofk_launch_keyframe_begin(hipStream_t s, const ofk_kf_rows &t, const int *counts, int stride, int batch)
{
    hipLaunchKernelGGL(k_keyframe_begin, dim3(batch), dim3(256), 0, s, t, counts, stride);
}

void ofk_launch_keyframe_replace(hipStream_t s, const ofk_kf_rows &t, const int *limit, const int *new_counts, int stride, int batch)
{
    hipLaunchKernelGGL(k_keyframe_replace, dim3(batch), dim3(256), 0, s, t, limit, new_counts, stride);
}

void ofk_launch_keyframe_reset(hipStream_t s, const ofk_kf_rows &t, int b, int stride, const double *p)
{
    hipLaunchKernelGGL(k_keyframe_reset, dim3(1), dim3(256), 0, s, t, b, stride, p[0], p[1], p[2]);
}

void ofk_launch_keyframe_step(hipStream_t s, const ofk_kf_rows &t, const ofk_kf_in &in, const ofk_keyframe *k, int batch)
{
    hipLaunchKernelGGL(k_keyframe_step, dim3(batch), dim3(256), 0, s, t, in, kf_make_cfg(k));
}
