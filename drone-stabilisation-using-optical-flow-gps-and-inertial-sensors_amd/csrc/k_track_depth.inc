// k_track_depth.inc — an inverse depth per track of a video stream (ofk.h: ofk_set_track_depth): rho, its variance and the number of
// measurements per row of the track table, filtered over the frames, and the velocity solved from the depths of the earlier frames.
// Included by k_tracks.hip behind k_lstsq.inc, whose sums, reduction, solve and eig_inverse3 the map solve shares.  The rows of one
// stream are only ever touched by that stream's workgroup, with plain vector stores and no atomics, so a second launch on the same
// inputs gives the same bits.  All arithmetic is f64 in the order ofk.h states (the build has no FMA contraction).

struct td_cfg { double sf, b_min, gate, q, rel_max; int min_obs, min_rows, update; };

__device__ __forceinline__ void td_fresh_row(const ofk_td_rows &t, size_t w) { t.rho[w] = 0.0; t.var[w] = 0.0; t.nobs[w] = 0; }   // no depth yet

// the rows of freshly detected tracks (beside k_track_table_begin): no depth yet, and an empty record.  One workgroup per stream.
__global__ __launch_bounds__(256) void k_track_depth_begin(ofk_td_rows t, const int *__restrict__ counts, int stride)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[b], 0), stride);
    const size_t base = (size_t)b * stride;
    for (int i = tid; i < n; i += 256) td_fresh_row(t, base + i);
    if (tid < OFK_TD_DOUBLES) t.rec[(size_t)b * OFK_TD_DOUBLES + tid] = 0.0;
}

// behind k_replace_tracks (beside k_track_table_replace): the streams with a budget start over
__global__ __launch_bounds__(256) void k_track_depth_replace(ofk_td_rows t, const int *__restrict__ limit, const int *__restrict__ new_counts,
                                                             int stride)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!rows_stream_on(b, 0, gridDim.x, limit)) return;
    const int n = min(max(new_counts[b], 0), stride);
    const size_t base = (size_t)b * stride;
    for (int i = tid; i < n; i += 256) td_fresh_row(t, base + i);
}

// Point r's terms: the stage entry's x and u as they are, the resident points as pair_point forms them (k_estimate.hip).
__device__ __forceinline__ void td_point(const ofk_td_in &in, size_t r, double cx, double cy, double scaling, double &x, double &y, double &ux,
                                         double &uy)
{
    if (in.x) { x = in.x[2 * r]; y = in.x[2 * r + 1]; ux = in.u[2 * r]; uy = in.u[2 * r + 1]; return; }
    const double X = (double)in.next_pts[2 * r], Y = (double)in.next_pts[2 * r + 1];
    x = (X - cx) * scaling; y = (Y - cy) * scaling;
    ux = (X - (double)in.prev_pts[2 * r]) * scaling; uy = (Y - (double)in.prev_pts[2 * r + 1]) * scaling;
}

// Rules 1-4 of ofk.h, in front of k_track_table_update and with its walk (k_rows.inc).  One workgroup per stream.
//   1. the map solve over the mature rows of the state as the previous step left it: the ten sums of acc_point with (sA, sB) =
//      (rho_i, 1), acc_block_sum, solve_from_acc; it reads nothing of this step's record
//   2.-4. per chunk of 256 rows: measurement, prediction, and the kept rows move up in order, in place.
// The counts are ballots summed per wave and across the waves through LDS.  Thread 0 solves the 3 x 3 behind the walk and writes the
// record.
__global__ __launch_bounds__(256) void k_track_depth_step(ofk_td_rows t, ofk_td_in in, td_cfg cfg)
{
    __shared__ row_walk s_rows;
    __shared__ int s_cnt[4][6];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(in.counts[b], 0), in.stride);
    const size_t base = (size_t)b * in.stride;
    const double *sn = in.sensors ? in.sensors + (size_t)b * OFK_SENSOR_DOUBLES : nullptr;
    const double scaling = sn ? sn[19] : 1.0, cx = sn ? sn[20] : 0.0, cy = sn ? sn[21] : 0.0;
    const double *ob = in.omega + (size_t)b * in.omega_stride, *vr = in.v + (size_t)b * OFK_RECORD_DOUBLES;
    const double om[3] = {ob[0], ob[1], ob[2]}, v[3] = {vr[0], vr[1], vr[2]};
    const bool solved = in.plain ? vr[4] >= 3.0 : vr[15] != 0.0;  // the plain step's record has no solved flag: its rank
    const bool meas = solved && isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]);
    const double sf = cfg.sf * scaling, bmin = cfg.b_min * scaling, sf2 = sf * sf, g2 = cfg.gate * cfg.gate, gs = g2 * sf2;

    // 1. the map solve, from the prior state
    Acc a; acc_zero(a);
    for (int i = tid; i < n; i += 256) {
        const size_t r = base + i;
        const double rho = t.rho[r], lim = cfg.rel_max * rho;
        if (in.status[r] != 0 && t.nobs[r] >= cfg.min_obs && rho > 0.0 && t.var[r] <= lim * lim) {
            double x, y, ux, uy, c0, c1, c2;
            td_point(in, r, cx, cy, scaling, x, y, ux, uy);
            cross_p(x, y, om[0], om[1], om[2], c0, c1, c2);       // [p]x omega
            acc_point(a, x, y, ux + c0, uy + c1, c2, rho, 1.0);
        }
    }
    acc_block_sum(a);                                            // its barriers: every thread has read the prior state

    // 2.-4.
    int c_upd = 0, c_ini = 0, c_b = 0, c_r = 0, c_nu = 0, c_rst = 0;    // wave-uniform
    rows_begin(s_rows);
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool inside = i < n;
        const size_t r = base + (inside ? i : 0);
        const bool keep = inside && in.status[r] != 0;
        double rho = t.rho[r], var = t.var[r];
        int nobs = t.nobs[r];
        bool upd = false, ini = false, skb = false, skr = false, sknu = false, rst = false;
        if (keep) {
            double x, y, ux, uy;
            td_point(in, r, cx, cy, scaling, x, y, ux, uy);
            if (meas) {
                double c0, c1, c2;
                cross_p(x, y, om[0], om[1], om[2], c0, c1, c2);
                const double q0 = ux + c0, q1 = uy + c1, q2 = c2;
                const double a0 = q0 - q2 * x, a1 = q1 - q2 * y, b0 = v[0] - v[2] * x, b1 = v[1] - v[2] * y;
                const double bb = b0 * b0 + b1 * b1, ab = a0 * b0 + a1 * b1, nb = sqrt(bb);
                const double cr = a0 * b1 - a1 * b0, kap = ab / bb, rr = cr / nb;
                skb = nb < bmin;
                skr = !skb && cfg.gate > 0.0 && rr * rr > gs;
                if (!skb && !skr && !isfinite(kap)) skb = true;  // counted with the short |b|: it is |b| = 0 or a point that is no number
                if (!skb && !skr) {
                    const double R = sf2 / bb;
                    if (nobs == 0) {
                        if (kap > 0.0) { rho = kap; var = R; nobs = 1; ini = true; }
                    } else if (cfg.update) {
                        const double nu = kap - rho, S = var + R;
                        if (cfg.gate > 0.0 && nu * nu > g2 * S) sknu = true;
                        else { const double K = var / S; rho = rho + K * nu; var = var * R / S; nobs += 1; upd = true; }
                    }
                }
            }
            if (nobs >= 1) {
                if (solved) {
                    const double w = om[0] * y - om[1] * x, g = (1.0 + rho * v[2]) + w;
                    if (isfinite(g) && g >= 0.1) { const double J = (1.0 + w) / (g * g); rho = rho / g; var = var * J * J + cfg.q; }
                    else { rho = 0.0; var = 0.0; nobs = 0; rst = true; }
                } else
                    var = var + cfg.q;
            }
        }
        c_upd += __popcll(__ballot(upd)); c_ini += __popcll(__ballot(ini)); c_b += __popcll(__ballot(skb));
        c_r += __popcll(__ballot(skr)); c_nu += __popcll(__ballot(sknu)); c_rst += __popcll(__ballot(rst));
        const int pos = rows_place(s_rows, keep);
        if (keep) { const size_t w = base + pos; t.rho[w] = rho; t.var[w] = var; t.nobs[w] = nobs; }
        rows_next(s_rows);
    }
    const int kept = s_rows.base;
    const int extra = rows_extra(in.new_counts, b, in.max_total, in.stride, kept);
    for (int i = tid; i < extra; i += 256) td_fresh_row(t, base + kept + i);
    if (lane == 0) { int *s = s_cnt[wave]; s[0] = c_upd; s[1] = c_ini; s[2] = c_b; s[3] = c_r; s[4] = c_nu; s[5] = c_rst; }
    __syncthreads();
    if (tid == 0) {
        double *o = t.rec + (size_t)b * OFK_TD_DOUBLES;
        for (int k = 0; k < OFK_TD_DOUBLES; ++k) o[k] = 0.0;
        double vm[3] = {0.0, 0.0, 0.0}, s3[3], lam[3], V[3][3];
        bool fin = true;
        const int rank = a.cnt >= (double)cfg.min_rows ? solve_from_acc(a, vm, s3, fin, lam, V) : 0;
        const bool ok = rank == 3 && fin;
        if (ok) {                                                // C_map = sigma_flow^2 M^-1 from the solve's own decomposition
            double Mi[3][3];
            eig_inverse3(lam, V, Mi);
            int s = 10;
            for (int i = 0; i < 3; ++i)
                for (int j = i; j < 3; ++j) o[s++] = sf2 * Mi[i][j];
            o[0] = vm[0]; o[1] = vm[1]; o[2] = vm[2];
        }
        o[3] = ok ? 0.0 : 1.0; o[4] = a.cnt;
        for (int k = 0; k < 5; ++k) o[5 + k] = (double)(s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k]);
        o[16] = v[0]; o[17] = v[1]; o[18] = v[2]; o[19] = solved ? 1.0 : 0.0;
        o[20] = (double)(s_cnt[0][5] + s_cnt[1][5] + s_cnt[2][5] + s_cnt[3][5]);
    }
}

static td_cfg td_make_cfg(const ofk_track_depth *d)
{
    td_cfg c;
    c.sf = d->sigma_flow; c.b_min = d->b_min; c.gate = d->gate; c.q = d->q; c.rel_max = d->rel_max;
    c.min_obs = d->min_obs; c.min_rows = d->min_rows; c.update = d->update;
    return c;
}

void ofk_launch_track_depth_begin(hipStream_t s, const ofk_td_rows &t, const int *counts, int stride, int batch)
{
    hipLaunchKernelGGL(k_track_depth_begin, dim3(batch), dim3(256), 0, s, t, counts, stride);
}

void ofk_launch_track_depth_replace(hipStream_t s, const ofk_td_rows &t, const int *limit, const int *new_counts, int stride, int batch)
{
    hipLaunchKernelGGL(k_track_depth_replace, dim3(batch), dim3(256), 0, s, t, limit, new_counts, stride);
}

void ofk_launch_track_depth_step(hipStream_t s, const ofk_td_rows &t, const ofk_td_in &in, const ofk_track_depth *d, int batch)
{
    hipLaunchKernelGGL(k_track_depth_step, dim3(batch), dim3(256), 0, s, t, in, td_make_cfg(d));
}
