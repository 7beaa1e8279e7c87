// k_keyframe_map.inc — the keyframe's map (ofk.h: ofk_set_keyframe_map): the depth filter's rho and var per track row frozen at the
// keyframe, and the key translation solved against them in the ground plane's place.  Included by k_tracks.hip behind
// k_keyframe_rot.inc; it compiles k_keyframe_body.inc a third time with KF_MAP 1 (rules M1-M5 around rules 1-5), k_keyframe_step and
// k_keyframe_step_rot being the same text with KF_MAP 0.  Like them: one workgroup per stream, only that stream's rows and state,
// plain vector stores, no atomics, f64 in the order ofk.h states.  Every walk takes the rows i = tid + 256 k, so a thread only ever
// reads the key depths it captured itself in front of the compaction's barriers.

struct km_cfg { int min_obs, min_rows, weights; double rel_max, ready_share; };
typedef ofk_km_rows km_rows;                                     // ofk_internal.h

__device__ __forceinline__ void km_fresh_row(const km_rows &m, size_t w) { m.key_rho[w] = 0.0; m.key_var[w] = 0.0; }   // no key depth

// acc_point_w's arithmetic (k_robust.inc) with the row always counted: rows are rows, not weight sums
__device__ __forceinline__ void km_point(Acc &a, double x, double y, double q0, double q1, double sA, double w)
{
    double c0, c1, c2, t0, t1, t2;
    cross_p(x, y, q0, q1, 0.0, c0, c1, c2);
    cross_p(x, y, c0, c1, c2, t0, t1, t2);
    const double pp = x * x + y * y + 1.0, sa2 = sA * sA * w, sab = sA * 1.0 * w;
    a.m00 += sa2 * (pp - x * x); a.m01 += sa2 * (-x * y); a.m02 += sa2 * (-x);
    a.m11 += sa2 * (pp - y * y); a.m12 += sa2 * (-y);     a.m22 += sa2 * (pp - 1.0);
    a.g0 -= sab * t0; a.g1 -= sab * t1; a.g2 -= sab * t2;
    a.cnt += 1.0;
}

// Rule M3's terms of the live map row r; false: the row is left out
__device__ __forceinline__ bool km_row(const ofk_kf_rows &t, const km_rows &m, const float *__restrict__ next, size_t r, const kf_frame &f,
                                       int weights, double sf2, double &x, double &y, double &u0, double &u1, double &sA, double &w)
{
    const double kx = ((double)t.key_xy[2 * r] - f.cx) * f.sc, ky = ((double)t.key_xy[2 * r + 1] - f.cy) * f.sc;
    x = ((double)next[2 * r] - f.cx) * f.sc; y = ((double)next[2 * r + 1] - f.cy) * f.sc;
    const double X = (f.R[0] * kx + f.R[1] * ky) + f.R[2], Y = (f.R[3] * kx + f.R[4] * ky) + f.R[5], Z = (f.R[6] * kx + f.R[7] * ky) + f.R[8];
    if (!(Z >= OFK_KEY_MIN_DEPTH)) return false;
    const double a = X / Z, b = Y / Z, kr = m.key_rho[r];
    u0 = x - a; u1 = y - b; sA = kr / Z;
    w = weights ? sf2 / (sf2 + ((u0 * u0 + u1 * u1) * m.key_var[r]) / (kr * kr)) : 1.0;
    return true;
}

struct km_res { Acc as; double T[3], rows1, rows2, rms, sumw, spread; bool gated; };

// Rule M3 over the live map rows.  true: the map solve stands (o.as the sums of the solve that stands).  Uniform over the workgroup.
__device__ bool km_solve(const ofk_kf_rows &t, const ofk_kf_in &in, const km_rows &m, size_t base, int n, const kf_frame &f, const kf_cfg &cfg,
                         const km_cfg &mc, double sf2, double g2, double *s_red, km_res &o)
{
    Acc a1; acc_zero(a1);
    for (int i = threadIdx.x; i < n; i += 256) {
        const size_t r = base + i;
        double x, y, u0, u1, sA, w;
        if (in.status[r] != 0 && t.member[r] != 0 && m.key_rho[r] > 0.0 && km_row(t, m, in.next_pts, r, f, mc.weights, sf2, x, y, u0, u1, sA, w))
            km_point(a1, x, y, u0, u1, sA, w);
    }
    acc_block_sum(a1);
    o.as = a1; o.rows1 = a1.cnt; o.rows2 = 0.0; o.rms = o.sumw = o.spread = 0.0; o.gated = false;
    double s3[3];
    bool fin = true;
    o.T[0] = o.T[1] = o.T[2] = 0.0;
    if (!(a1.cnt >= (double)mc.min_rows && solve_from_acc(a1, o.T, s3, fin) == 3 && fin)) { o.T[0] = o.T[1] = o.T[2] = 0.0; return false; }
    const double T1[3] = {o.T[0], o.T[1], o.T[2]};
    if (cfg.gate > 0.0) {
        Acc a2; acc_zero(a2);
        for (int i = threadIdx.x; i < n; i += 256) {
            const size_t r = base + i;
            double x, y, u0, u1, sA, w;
            if (in.status[r] != 0 && t.member[r] != 0 && m.key_rho[r] > 0.0 && km_row(t, m, in.next_pts, r, f, mc.weights, sf2, x, y, u0, u1, sA, w) &&
                w * kf_res2(x, y, u0, u1, sA, T1) <= g2)
                km_point(a2, x, y, u0, u1, sA, w);
        }
        acc_block_sum(a2);
        o.rows2 = a2.cnt;
        double T2[3], s32[3];
        bool fin2 = true;
        if (a2.cnt >= (double)cfg.min_rows && solve_from_acc(a2, T2, s32, fin2) == 3 && fin2) {
            o.gated = true; o.as = a2; o.T[0] = T2[0]; o.T[1] = T2[1]; o.T[2] = T2[2];
        }
    }
    double ss = 0.0, sw = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const size_t r = base + i;
        double x, y, u0, u1, sA, w;
        if (in.status[r] != 0 && t.member[r] != 0 && m.key_rho[r] > 0.0 && km_row(t, m, in.next_pts, r, f, mc.weights, sf2, x, y, u0, u1, sA, w) &&
            (!o.gated || w * kf_res2(x, y, u0, u1, sA, T1) <= g2)) {
            ss += w * kf_res2(x, y, u0, u1, sA, o.T); sw += w;
        }
    }
    ss = block_sum(ss, s_red);
    sw = block_sum(sw, s_red);
    o.rms = sqrt(ss / o.as.cnt) / f.sc; o.sumw = sw; o.spread = sqrt(ss / sw) / f.sc;
    return true;
}

__global__ __launch_bounds__(256) void k_keyframe_step_map(ofk_kf_rows t, ofk_kf_in in, kf_cfg cfg, km_cfg mc, km_rows km)
{
#define KF_ROT 0
#define KF_MAP 1
#include "k_keyframe_body.inc"
#undef KF_MAP
#undef KF_ROT
}

// the map beside k_keyframe_begin (limit NULL, counts: the rows in use), k_keyframe_replace (the streams with a budget, counts: the
// new rows) and k_keyframe_reset (one stream b0, counts NULL: all `stride` rows), behind them on the stream: no key depths, and
// captured_for = the keyframe's key_step (key_ist: its istate), so that nothing is captured before the next re-key - the depth state
// of this moment is not the keyframe's; keep_rec 0: an empty record with flag OFK_KEYMAP_NONE
__global__ __launch_bounds__(256) void k_keymap_clear(km_rows m, const int *__restrict__ key_ist, const int *__restrict__ limit,
                                                      const int *__restrict__ counts, int stride, int b0, int keep_rec)
{
    const int b = b0 + blockIdx.x, tid = threadIdx.x;
    if (!rows_stream_on(b, b0, gridDim.x, limit)) return;
    const int n = counts ? min(max(counts[b], 0), stride) : stride;
    const size_t base = (size_t)b * stride;
    for (int i = tid; i < n; i += 256) km_fresh_row(m, base + i);
    if (tid == 0) { m.mstate[(size_t)b * 2] = key_ist[(size_t)b * OFK_KEY_INTS]; m.mstate[(size_t)b * 2 + 1] = 0; }
    if (!keep_rec && tid < OFK_KEYMAP_DOUBLES) m.mrec[(size_t)b * OFK_KEYMAP_DOUBLES + tid] = tid == 0 ? (double)OFK_KEYMAP_NONE : 0.0;
}

static km_cfg km_make_cfg(const ofk_keyframe_map *k)
{
    km_cfg c;
    c.min_obs = k->min_obs; c.min_rows = k->min_rows; c.weights = k->weights; c.rel_max = k->rel_max; c.ready_share = k->ready_share;
    return c;
}

void ofk_launch_keyframe_step_map(hipStream_t s, const ofk_kf_rows &t, const ofk_kf_in &in, const ofk_keyframe *k, const ofk_keyframe_map *m,
                                  const ofk_km_rows &r, int batch)
{
    hipLaunchKernelGGL(k_keyframe_step_map, dim3(batch), dim3(256), 0, s, t, in, kf_make_cfg(k), km_make_cfg(m), r);
}

void ofk_launch_keymap_clear(hipStream_t s, const ofk_km_rows &r, const int *key_ist, const int *limit, const int *counts, int stride, int b0,
                             int keep_rec, int batch)
{
    hipLaunchKernelGGL(k_keymap_clear, dim3(batch), dim3(256), 0, s, r, key_ist, limit, counts, stride, b0, keep_rec);
}
