// k_robust.inc — the robust velocity solve (ofk.h: ofk_set_robust): a least-median-of-squares start sampled from two-point hypotheses,
// then iteratively reweighted least squares (Huber / Tukey) with the scale taken from the median residual.  Included by k_estimate.hip,
// whose helpers (acc_point's sums, solve_from_acc, resid_point, point_terms, pair_point, fuse_terms, ofk_philox4x32_10) it shares.
//
// One team per problem: a single wave (k_pairs_robust<1>, beside the response kernel / LK of large batches) or a 256-thread workgroup
// (<4>: small batches, the stage entry, the stream steps).  Both forms compute the same bits:
//   * every sum over the points is formed as the plain solve forms it - four "virtual waves" take the chunks c = vw, vw + 4, ... of 64
//     points, each is reduced by the shuffle butterfly, the four partial sums are added as (s0 + s1) + (s2 + s3);
//   * the order statistic is exact (a radix select on the f64 bit patterns: non-negative doubles order as their u64 images), so it does
//     not depend on who counts;
//   * everything else (two-point solves, 3x3 eigen-solves, weights) is per-point or per-problem arithmetic.
// Work split: the per-point terms (x, y, q, sA, sB) are computed once and parked in a global workspace row (7 doubles per point, read
// back through L1/L2: max_pts goes up to 4096, far beyond what registers or one wave's share of LDS hold); a lane keeps rho^2 of its
// first ROB_CACHE chunks (512 points per team) in registers across the ~63 counting passes of a selection and recomputes the rest.
// A selection is wave-local (ballot + popcount per pass, high word first, stops as soon as one candidate is left), so in the
// workgroup form the four waves score different hypotheses at the same time.  The K two-point solves run one per LANE.
// LDS: 9.7 KB per team (8 KB of it the rank -> point index list the sampling needs).  No atomics, no MFMA, vector stores only.
#define ROB_CACHE 8
#define ROB_MAX_PTS 4096

struct rob_cfg { int loss; double c; int iters, hyps; unsigned k0, k1; int drop; };
struct rob_result { double v[3], r, rank, s3[3], cnt, kept, tracked; bool fin; };   // cnt: points with w > 0; kept: points that entered; fin: the plain sums are finite

struct rob_lds {
    unsigned long long keep[ROB_MAX_PTS / 64];                   // bit `lane` of keep[c]: point c * 64 + lane enters the solve
    unsigned short idx[ROB_MAX_PTS];                             // kept point number -> point index
    double part[4][14];                                          // wave-reduced sums of the four virtual waves
    double best[4][5];                                           // per wave: score, hypothesis, its velocity (kept here, not in registers)
    double plain[4][8];                                          // per wave: the plain start 0-2, then singular values 3-5 and rank 6 of the current system
    double sums[4][4];                                           // per wave: bb, kept count, tracked count of the plain sums, whether they are finite
};

__device__ __forceinline__ void acc_point_w(Acc &a, double x, double y, double q0, double q1, double q2, double sA, double sB, double w)
{
    double c0, c1, c2, t0, t1, t2;
    cross_p(x, y, q0, q1, q2, c0, c1, c2);
    cross_p(x, y, c0, c1, c2, t0, t1, t2);
    const double pp = x * x + y * y + 1.0, sa2 = sA * sA * w, sab = sA * sB * w;
    a.m00 += sa2 * (pp - x * x); a.m01 += sa2 * (-x * y); a.m02 += sa2 * (-x);
    a.m11 += sa2 * (pp - y * y); a.m12 += sa2 * (-y);     a.m22 += sa2 * (pp - 1.0);
    a.g0 -= sab * t0; a.g1 -= sab * t1; a.g2 -= sab * t2;
    a.cnt += w > 0.0 ? 1.0 : 0.0;
}

__device__ __forceinline__ double rob_weight(int loss, double rho2, double cs)
{
    const double t = sqrt(rho2) / cs;
    if (loss == OFK_ROBUST_HUBER) return t <= 1.0 ? 1.0 : 1.0 / t;
    const double u = 1.0 - t * t;
    return t < 1.0 ? u * u : 0.0;
}

// The element of index k (ascending) among the team's kept rho^2 values: r2[j] holds chunk j's value of this lane (valid where bit j of
// vm is set), tail(c, valid) recomputes chunk c >= ROB_CACHE.  Wave-local; the result is the same in every lane.
template <class Tail>
__device__ __forceinline__ double rob_select(const double (&r2)[ROB_CACHE], unsigned vm, int nchunks, int m, int k, Tail tail)
{
    unsigned phi = 0, plo = 0;
    int cand = m, bit = 62;
    for (; bit >= 0 && cand > 1; --bit) {
        const bool high = bit >= 32;
        const int sh = high ? bit - 32 : bit;
        // candidates whose bit `bit` is 0: they agree with the prefix on every bit above it, and the prefix's own bit is still 0
        auto zero_here = [&](double val) {
            const unsigned long long key = (unsigned long long)__double_as_longlong(val);
            const unsigned hi = (unsigned)(key >> 32), lo = (unsigned)key;
            return high ? ((hi ^ phi) >> sh) == 0u : (hi == phi && ((lo ^ plo) >> sh) == 0u);
        };
        int cnt0 = 0;
#pragma unroll
        for (int j = 0; j < ROB_CACHE; ++j) cnt0 += __popcll(__ballot(((vm >> j) & 1u) && zero_here(r2[j])));
        for (int c = ROB_CACHE; c < nchunks; ++c) {
            bool valid;
            const double val = tail(c, valid);
            cnt0 += __popcll(__ballot(valid && zero_here(val)));
        }
        if (k < cnt0) cand = cnt0;
        else { k -= cnt0; cand -= cnt0; if (high) phi |= 1u << sh; else plo |= 1u << sh; }
    }
    // what is left agrees with the prefix above `bit`: one element, or several equal ones (then the loop ran out of bits)
    const unsigned long long prefix = ((unsigned long long)phi << 32) | plo;
    const int sh = bit + 1;
    unsigned long long found = 0;
    auto take = [&](double val) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(val);
        if (((key ^ prefix) >> sh) == 0ull && key > found) found = key;
    };
#pragma unroll
    for (int j = 0; j < ROB_CACHE; ++j) if ((vm >> j) & 1u) take(r2[j]);
    for (int c = ROB_CACHE; c < nchunks; ++c) {
        bool valid;
        const double val = tail(c, valid);
        if (valid) take(val);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(found, o); found = u > found ? u : found; }
    return __longlong_as_double((long long)found);
}

// terms(i, x, y, q0, q1, q2, sA, sB, tracked) -> point i enters the solve; called exactly once per point i < n.
// T: this problem's workspace [7][stride]; wa: its weight row (output, [stride]); wb: a scratch row; stats: OFK_ROBUST_DOUBLES.
// min_cnt: the plain solve's guard (solved when more than min_cnt points entered).  The result is valid in every thread.
template <int NW, class Terms>
__device__ __forceinline__ void robust_core(rob_lds &L, const rob_cfg &rc, int n, int stride, unsigned problem, double min_cnt,
                                            double *T, double *wa, double *wb, double *stats, Terms terms, rob_result &R)
{
    const int lane = threadIdx.x & 63, wave = NW == 1 ? 0 : (int)(threadIdx.x >> 6);
    const int nchunks = (n + 63) >> 6;
    const size_t S = (size_t)stride;
    // ---- per-point terms, keep masks and the plain sums
    for (int vw = wave; vw < 4; vw += NW) {
        Acc a; acc_zero(a);
        double tracked = 0.0;
        for (int c = vw; c < nchunks; c += 4) {
            const int i = c * 64 + lane;
            double x = 0, y = 0, q0 = 0, q1 = 0, q2 = 0, sA = 0, sB = 0;
            const bool kept = i < n && terms(i, x, y, q0, q1, q2, sA, sB, tracked);
            if (kept) {
                T[i] = x; T[S + i] = y; T[2 * S + i] = q0; T[3 * S + i] = q1; T[4 * S + i] = q2; T[5 * S + i] = sA; T[6 * S + i] = sB;
                acc_point(a, x, y, q0, q1, q2, sA, sB);
            }
            const unsigned long long mk = __ballot(kept);
            if (lane == 0) L.keep[c] = mk;
        }
        const double v[12] = {a.m00, a.m01, a.m02, a.m11, a.m12, a.m22, a.g0, a.g1, a.g2, a.bb, a.cnt, tracked};
#pragma unroll
        for (int k = 0; k < 12; ++k) { const double w_ = wave_sum(v[k]); if (lane == 0) L.part[vw][k] = w_; }
    }
    __syncthreads();                                             // also publishes the workspace rows to the whole team
    Acc a0;
    {
        double t[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) t[k] = (L.part[0][k] + L.part[1][k]) + (L.part[2][k] + L.part[3][k]);
        a0.m00 = t[0]; a0.m01 = t[1]; a0.m02 = t[2]; a0.m11 = t[3]; a0.m12 = t[4]; a0.m22 = t[5]; a0.g0 = t[6]; a0.g1 = t[7]; a0.g2 = t[8];
        a0.bb = t[9]; a0.cnt = t[10];
        // what only the end (and the exact-fit test) needs waits in LDS, not in registers: every lane stores the same value and reads
        // back its own store, so no barrier is involved
        L.sums[wave][0] = t[9]; L.sums[wave][1] = t[10]; L.sums[wave][2] = t[11];
    }
    bool solvable = a0.cnt > min_cnt;
    double v[3] = {0, 0, 0};
    double *plain = L.plain[wave];
    {
        double s3[3] = {0, 0, 0};
        bool fin = true;
        const int rank = solvable ? solve_from_acc(a0, v, s3, fin) : 0;   // today's plain result; every thread solves the same system
        solvable = solvable && fin;                              // non-finite sums: not solved - flag 1, weights 1, residual 0
        L.sums[wave][3] = fin ? 1.0 : 0.0;
        plain[0] = v[0]; plain[1] = v[1]; plain[2] = v[2]; plain[3] = s3[0]; plain[4] = s3[1]; plain[5] = s3[2]; plain[6] = (double)rank;
    }
    // kept point number -> index: an exclusive scan of the chunks' populations, then each kept point's place inside its chunk
    const int pc = lane < nchunks ? __popcll(L.keep[lane]) : 0;
    int incl = pc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
    const int m = __shfl(incl, 63), base = incl - pc;
    for (int c = wave; c < nchunks; c += NW) {
        const unsigned long long mk = L.keep[c];
        const int bc = __shfl(base, c);
        if ((mk >> lane) & 1ull) L.idx[bc + __popcll(mk & ((1ull << lane) - 1ull))] = (unsigned short)(c * 64 + lane);
    }
    unsigned vm = 0;
#pragma unroll
    for (int j = 0; j < ROB_CACHE; ++j) if (j < nchunks) vm |= (unsigned)((L.keep[j] >> lane) & 1ull) << j;
    __syncthreads();

    auto rho2_at = [&](int i, const double *vv) {
        return resid_point(T[i], T[S + i], T[2 * S + i], T[3 * S + i], T[4 * S + i], T[5 * S + i], T[6 * S + i], vv);
    };
    double r2[ROB_CACHE];
    auto eval = [&](const double *vv) {
#pragma unroll
        for (int j = 0; j < ROB_CACHE; ++j) r2[j] = ((vm >> j) & 1u) ? rho2_at(j * 64 + lane, vv) : 0.0;
    };
    auto select = [&](const double *vv) {
        return rob_select(r2, vm, nchunks, m, m / 2, [&](int c, bool &valid) {
            valid = (L.keep[c] >> lane) & 1ull;
            return valid ? rho2_at(c * 64 + lane, vv) : 0.0;
        });
    };

    double s = 0.0, score = 0.0;
    int hyp = -1, done = 0, flag = 0;
    bool ones = true;                                            // the current weights are all 1 (nothing stored yet)
    double *wcur = wa;
    if (m < OFK_ROBUST_MIN_POINTS || !solvable) flag = 1;
    else {
        // ---- sampled start: K two-point hypotheses, one solve per lane, scored by the median squared residual over all kept points
        // the best hypothesis' velocity waits in LDS (written by lane 0, read behind the barrier), the plain start in `plain`: the
        // scoring loop needs the registers.  The best score itself stays in a register: every lane computes the same one.
        double *mine = L.best[wave];
        double bscore = INFINITY;
        int bh = -1;
        for (int h0 = 0; h0 < rc.hyps; h0 += 64) {
            double hv[3] = {0, 0, 0};
            int hrank = 0;
            if (h0 + lane < rc.hyps) {
                unsigned xr[4];
                ofk_philox4x32_10((unsigned)(h0 + lane), problem, 0u, 0u, rc.k0, rc.k1, xr);
                const int i = (int)(xr[0] % (unsigned)m);
                int j = (int)(xr[1] % (unsigned)(m - 1));
                j += j >= i ? 1 : 0;
                const int pi = L.idx[i], pj = L.idx[j];
                Acc a; acc_zero(a);
                acc_point(a, T[pi], T[S + pi], T[2 * S + pi], T[3 * S + pi], T[4 * S + pi], T[5 * S + pi], T[6 * S + pi]);
                acc_point(a, T[pj], T[S + pj], T[2 * S + pj], T[3 * S + pj], T[4 * S + pj], T[5 * S + pj], T[6 * S + pj]);
                double hs[3];
                bool hfin;
                hrank = solve_from_acc(a, hv, hs, hfin);
            }
            const int nh = rc.hyps - h0 < 64 ? rc.hyps - h0 : 64;
            for (int hl = wave; hl < nh; hl += NW) {
                if (__shfl(hrank, hl) < 3) continue;                 // void
                const double vv[3] = {__shfl(hv[0], hl), __shfl(hv[1], hl), __shfl(hv[2], hl)};
                eval(vv);
                const double sc = select(vv);
                if (sc < bscore) {
                    bscore = sc; bh = h0 + hl;
                    if (lane == 0) { mine[2] = vv[0]; mine[3] = vv[1]; mine[4] = vv[2]; }
                }
            }
        }
        if (lane == 0) { mine[0] = bscore; mine[1] = (double)bh; }
        __syncthreads();
        v[0] = plain[0]; v[1] = plain[1]; v[2] = plain[2];
        for (int w_ = 0; w_ < NW; ++w_) {                        // the best of the waves' bests, ties to the smaller hypothesis
            const double sc = L.best[w_][0];
            const int h = (int)L.best[w_][1];
            if (h >= 0 && (hyp < 0 || sc < score || (sc == score && h < hyp))) { score = sc; hyp = h; v[0] = L.best[w_][2]; v[1] = L.best[w_][3]; v[2] = L.best[w_][4]; }
        }
        // ---- IRLS: exactly rc.iters rounds unless the data fit exactly (flag 2) or a weighted system loses rank (flag 3)
        for (int it = 0; it < rc.iters; ++it) {
            eval(v);
            s = 1.4826 * sqrt(select(v));
            if (!(s * s > 1e-24 * L.sums[wave][0] / (double)m)) { flag = 2; break; }
            const double cs = rc.c * s;
            double *wn = (ones || wcur == wb) ? wa : wb;
            __syncthreads();                                     // every wave has read the previous sums
            // rho^2 is recomputed here (five rounds against K scorings): the loops stay rolled and the cache's registers are free
#pragma unroll 1
            for (int vw = wave; vw < 4; vw += NW) {
                Acc a; acc_zero(a);
#pragma unroll 1
                for (int c = vw; c < nchunks; c += 4)
                    if ((L.keep[c] >> lane) & 1ull) {
                        const int i = c * 64 + lane;
                        const double w_ = rob_weight(rc.loss, rho2_at(i, v), cs);
                        wn[i] = w_;
                        acc_point_w(a, T[i], T[S + i], T[2 * S + i], T[3 * S + i], T[4 * S + i], T[5 * S + i], T[6 * S + i], w_);
                    }
                const double t[10] = {a.m00, a.m01, a.m02, a.m11, a.m12, a.m22, a.g0, a.g1, a.g2, a.cnt};
#pragma unroll
                for (int k = 0; k < 10; ++k) { const double w_ = wave_sum(t[k]); if (lane == 0) L.part[vw][k] = w_; }
            }
            __syncthreads();
            Acc aw; acc_zero(aw);
            {
                double t[10];
#pragma unroll
                for (int k = 0; k < 10; ++k) t[k] = (L.part[0][k] + L.part[1][k]) + (L.part[2][k] + L.part[3][k]);
                aw.m00 = t[0]; aw.m01 = t[1]; aw.m02 = t[2]; aw.m11 = t[3]; aw.m12 = t[4]; aw.m22 = t[5]; aw.g0 = t[6]; aw.g1 = t[7]; aw.g2 = t[8]; aw.cnt = t[9];
            }
            double v2[3], s2[3];
            bool wfin;
            const int rk = solve_from_acc(aw, v2, s2, wfin);
            if (rk < 3) { flag = 3; break; }
            v[0] = v2[0]; v[1] = v2[1]; v[2] = v2[2]; plain[3] = s2[0]; plain[4] = s2[1]; plain[5] = s2[2]; plain[6] = (double)rk;
            wcur = wn; ones = false; ++done;
        }
    }
    // ---- outputs: the weighted residual sum of the final v under the final weights, the weights themselves
    const bool resid = solvable;
    __syncthreads();
#pragma unroll 1
    for (int vw = wave; vw < 4; vw += NW) {
        double r = 0.0, sw = 0.0, cnt = 0.0;
        auto point = [&](int i, double rho2) {
            const double w_ = ones ? 1.0 : wcur[i];
            wa[i] = w_;
            if (resid) r += w_ * rho2;
            sw += w_; cnt += w_ > 0.0 ? 1.0 : 0.0;
        };
#pragma unroll 1
        for (int c = vw; c < nchunks; c += 4) if ((L.keep[c] >> lane) & 1ull) point(c * 64 + lane, rho2_at(c * 64 + lane, v));
        r = wave_sum(r); sw = wave_sum(sw); cnt = wave_sum(cnt);
        if (lane == 0) { L.part[vw][0] = r; L.part[vw][1] = sw; L.part[vw][2] = cnt; }
    }
    for (int i = threadIdx.x; i < stride; i += 64 * NW)
        if (i >= n || !((L.keep[i >> 6] >> (i & 63)) & 1ull)) wa[i] = 0.0;
    __syncthreads();
    R.r = (L.part[0][0] + L.part[1][0]) + (L.part[2][0] + L.part[3][0]);
    const double sw = (L.part[0][1] + L.part[1][1]) + (L.part[2][1] + L.part[3][1]);
    R.cnt = (L.part[0][2] + L.part[1][2]) + (L.part[2][2] + L.part[3][2]);
    R.v[0] = v[0]; R.v[1] = v[1]; R.v[2] = v[2]; R.rank = plain[6]; R.s3[0] = plain[3]; R.s3[1] = plain[4]; R.s3[2] = plain[5];
    R.kept = L.sums[wave][1]; R.tracked = L.sums[wave][2]; R.fin = L.sums[wave][3] != 0.0;
    if (threadIdx.x == 0) {
        stats[0] = s; stats[1] = sw; stats[2] = R.cnt; stats[3] = (double)m; stats[4] = (double)hyp; stats[5] = score;
        stats[6] = (double)done; stats[7] = (double)flag;
    }
}

// ------------------------------------------------------------------------------------------------ stage entry (host buffers)
__global__ __launch_bounds__(256) void k_solve_robust(int variant, const double *__restrict__ x, const double *__restrict__ u,
                                                      const uint8_t *__restrict__ valid, int n, const double *__restrict__ d,
                                                      const double *__restrict__ nrm, const double *__restrict__ omega,
                                                      const double *__restrict__ t, const double *__restrict__ wgt, rob_cfg rc,
                                                      double *work, double *weights, double *wtmp, double *__restrict__ stats,
                                                      double *__restrict__ out)
{
    __shared__ rob_lds L;
    const int b = blockIdx.x;
    const double *xb = x + (size_t)b * n * 2, *ub = u + (size_t)b * n * 2;
    const uint8_t *vb = valid ? valid + (size_t)b * n : nullptr;
    const double *wb = wgt ? wgt + (size_t)b * n : nullptr;
    const double nb[3] = {nrm[3 * b], nrm[3 * b + 1], nrm[3 * b + 2]};
    double ob[3] = {0, 0, 0};
    if (omega) { ob[0] = omega[3 * b]; ob[1] = omega[3 * b + 1]; ob[2] = omega[3 * b + 2]; }
    const double db = d ? d[b] : 1.0;
    rob_result R;
    robust_core<4>(L, rc, n, n, (unsigned)b, 0.0, work + (size_t)b * 7 * n, weights + (size_t)b * n, wtmp + (size_t)b * n,
                   stats + (size_t)b * OFK_ROBUST_DOUBLES,
                   [&](int i, double &px, double &py, double &q0, double &q1, double &q2, double &sA, double &sB, double &) {
                       if (vb && !vb[i]) return false;
                       px = xb[2 * i]; py = xb[2 * i + 1];
                       point_terms(variant, px, py, ub[2 * i], ub[2 * i + 1], nb, ob, db, wb ? wb[i] : 1.0, q0, q1, q2, sA, sB);
                       return true;
                   }, R);
    if (threadIdx.x == 0) {
        double *o = out + (size_t)b * OFK_SOLVE_DOUBLES;
        if (t && R.fin) sub_cross(R.v, ob, t + 3 * b, o);
        else { o[0] = R.v[0]; o[1] = R.v[1]; o[2] = R.v[2]; }
        o[3] = R.r; o[4] = R.rank; o[5] = R.s3[0]; o[6] = R.s3[1]; o[7] = R.s3[2];
    }
}

void ofk_launch_solve_robust(hipStream_t s, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                             const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                             const ofk_robust *r, double *work, double *weights, double *wtmp, double *stats, double *out)
{
    const rob_cfg rc = {r->loss, r->c, r->iters, r->hypotheses, (unsigned)r->seed, (unsigned)(r->seed >> 32), 0};
    hipLaunchKernelGGL(k_solve_robust, dim3(batch), dim3(256), 0, s, variant, x, u, valid, n, d, nrm, omega, t, wgt, rc, work, weights, wtmp,
                       stats, out);
}

// ------------------------------------------------------------------------------------------------ frame pairs / plain stream step
// k_pairs_solve's inputs and record; problem0: the index of the slice's first pair in the whole batch (the sampling's counter).
// drop_status (stream steps with drop): the keep flag of every kept point whose final weight is 0 is cleared.
template <int NW>
__global__ __launch_bounds__(64 * NW, 4) void k_pairs_robust(const float *__restrict__ prev_pts, const float *__restrict__ next_pts,
                                                          const uint8_t *status, const int *__restrict__ counts, int pts_stride,
                                                          const double *__restrict__ sensors, int variant, int use_feas, double feas_T,
                                                          const int *__restrict__ cand_count, rob_cfg rc, int problem0, double *work,
                                                          double *weights, double *wtmp, double *__restrict__ stats,
                                                          uint8_t *drop_status, double *__restrict__ records)
{
    __shared__ rob_lds L;
    const int b = blockIdx.x;
    const double *sn = sensors + (size_t)b * OFK_SENSOR_DOUBLES;
    const double d = sn[0], nrm[3] = {sn[1], sn[2], sn[3]}, om[3] = {sn[4], sn[5], sn[6]};
    const double scaling = sn[19], cx = sn[20], cy = sn[21], vp[3] = {sn[22], sn[23], sn[24]};
    const int n = min(max(counts[b], 0), pts_stride);
    const float *pp = prev_pts + (size_t)b * pts_stride * 2, *np_ = next_pts + (size_t)b * pts_stride * 2;
    const uint8_t *st = status + (size_t)b * pts_stride;
    double *wrow = weights + (size_t)b * pts_stride;
    rob_result R;
    robust_core<NW>(L, rc, n, pts_stride, (unsigned)(problem0 + b), 0.0, work + (size_t)b * 7 * pts_stride, wrow,
                    wtmp + (size_t)b * pts_stride, stats + (size_t)b * OFK_ROBUST_DOUBLES,
                    [&](int i, double &x, double &y, double &q0, double &q1, double &q2, double &sA, double &sB, double &tracked) {
                        if (!st[i]) return false;
                        tracked += 1.0;
                        double ux, uy;
                        if (!pair_point(pp, np_, i, cx, cy, scaling, use_feas, feas_T, nrm, vp, d, x, y, ux, uy)) return false;
                        point_terms(variant, x, y, ux, uy, nrm, om, d, 1.0, q0, q1, q2, sA, sB);
                        return true;
                    }, R);
    if (drop_status) {
        uint8_t *ds = drop_status + (size_t)b * pts_stride;
        for (int i = threadIdx.x; i < n; i += 64 * NW)
            if (((L.keep[i >> 6] >> (i & 63)) & 1ull) && wrow[i] == 0.0) ds[i] = 0;
    }
    if (threadIdx.x == 0) {
        double *o = records + (size_t)b * OFK_RECORD_DOUBLES, vu[3];
        write_record(o, R.v, R.r, R.rank, R.s3, om, sn + 16, sn + 7, R.cnt, n, R.tracked, vu);
        o[14] = cand_count ? (double)cand_count[b * OFK_CNT_STRIDE] : 0.0; o[15] = 0.0;
    }
}

void ofk_launch_pairs_robust(hipStream_t s, const float *prev_pts, const float *next_pts, const uint8_t *status, const int *counts,
                             int pts_stride, const double *sensors, int variant, int use_feas, double feas_T, const int *cand_count,
                             const ofk_robust *r, int problem0, double *work, double *weights, double *wtmp, double *stats,
                             uint8_t *drop_status, double *records, int batch)
{
    const rob_cfg rc = {r->loss, r->c, r->iters, r->hypotheses, (unsigned)r->seed, (unsigned)(r->seed >> 32), r->drop};
    // ofk_launch_pairs_solve's rule and reason: a single wave finds room beside the other slice's kernels, a small batch has the chip to itself
    if (batch >= 128)
        hipLaunchKernelGGL(k_pairs_robust<1>, dim3(batch), dim3(64), 0, s, prev_pts, next_pts, status, counts, pts_stride, sensors, variant,
                           use_feas, feas_T, cand_count, rc, problem0, work, weights, wtmp, stats, drop_status, records);
    else
        hipLaunchKernelGGL(k_pairs_robust<4>, dim3(batch), dim3(256), 0, s, prev_pts, next_pts, status, counts, pts_stride, sensors, variant,
                           use_feas, feas_T, cand_count, rc, problem0, work, weights, wtmp, stats, drop_status, records);
}

// ------------------------------------------------------------------------------------------------ fused stream step
// k_stream_fuse with the robust solve in the place of the plain one: the same prologue (filter predict, keep flags), the same epilogue
// with the robust v / v_uav going into the filter's correct; `solved` keeps its meaning (kept points against min_solve), the record's
// count field is the number of points with w > 0.  A twin and not a template of k_stream_fuse: that kernel keeps its code as it is.
struct rob_fuse_args { rob_cfg rc; double *work, *weights, *wtmp, *stats; };

__global__ __launch_bounds__(256) void k_stream_fuse_robust(fuse_args g, rob_fuse_args ra)
{
    __shared__ rob_lds L;
    __shared__ double s_pre[12];                                // nrm 0-2, omega 3-5, prior velocity 6-8
    const int b = blockIdx.x, tid = threadIdx.x;
    const double *sn = g.sensors + (size_t)b * OFK_SENSOR_DOUBLES;
    const double d = sn[0], scaling = sn[19], cx = sn[20], cy = sn[21];
    double *ist = g.f.use_imu && g.imu_state ? g.imu_state + (size_t)b * OFK_IMU_STATE : nullptr;
    double kx[KF_MAX], kP[KF_MAX][KF_MAX];                      // thread 0 only
    if (tid == 0) {
        for (int k = 0; k < 3; ++k) { s_pre[k] = ist ? ist[15 + k] : sn[1 + k]; s_pre[3 + k] = ist ? ist[18 + k] : sn[4 + k]; s_pre[6 + k] = ist ? ist[k] : sn[22 + k]; }
        if (g.f.filter) {
            kf_load(g.ns, b, g.kf_x, g.kf_P, kx, kP);
            double u[KF_MAX] = {0, 0, 0, 0, 0, 0};
            if (g.f.control == OFK_CONTROL_IMU && g.imu_dv) for (int k = 0; k < 3; ++k) u[k] = g.imu_dv[3 * (size_t)b + k];
            else for (int k = 0; k < 3; ++k) u[k] = sn[25 + k];
            kf_predict_dev(g.ns, g.nc, g.F, g.nc ? g.Bm : nullptr, g.Q, g.nc ? u : nullptr, kx, kP);
            if (g.f.keep == OFK_KEEP_LEGACY) for (int k = 0; k < 3; ++k) s_pre[6 + k] = kx[k];
        }
        if (g.imu_dv) for (int k = 0; k < 3; ++k) g.imu_dv[3 * (size_t)b + k] = 0.0;
    }
    __syncthreads();
    const double nrm[3] = {s_pre[0], s_pre[1], s_pre[2]}, om[3] = {s_pre[3], s_pre[4], s_pre[5]}, vp[3] = {s_pre[6], s_pre[7], s_pre[8]};
    const int n = min(max(g.counts[b], 0), g.pts_stride);
    const float *pp = g.prev_pts + (size_t)b * g.pts_stride * 2, *np_ = g.next_pts + (size_t)b * g.pts_stride * 2;
    uint8_t *st = g.status + (size_t)b * g.pts_stride;
    double *wrow = ra.weights + (size_t)b * g.pts_stride;
    rob_result R;
    robust_core<4>(L, ra.rc, n, g.pts_stride, (unsigned)b, (double)g.f.min_solve, ra.work + (size_t)b * 7 * g.pts_stride, wrow,
                   ra.wtmp + (size_t)b * g.pts_stride, ra.stats + (size_t)b * OFK_ROBUST_DOUBLES,
                   [&](int i, double &x, double &y, double &q0, double &q1, double &q2, double &sA, double &sB, double &tracked) {
                       const int s0 = st[i];
                       tracked += s0 ? 1.0 : 0.0;
                       double ux, uy, wgt, rl;
                       fuse_terms(g, i, pp, np_, cx, cy, scaling, nrm, om, vp, x, y, ux, uy, wgt, rl);
                       const bool keep = fuse_keep(g, s0, x, y, ux, uy, rl, nrm, vp, d);
                       st[i] = keep ? 1 : 0;
                       if (!keep) return false;
                       point_terms(g.variant, x, y, ux, uy, nrm, om, d, wgt, q0, q1, q2, sA, sB);
                       return true;
                   }, R);
    if (ra.rc.drop)
        for (int i = tid; i < n; i += 256)
            if (((L.keep[i >> 6] >> (i & 63)) & 1ull) && wrow[i] == 0.0) st[i] = 0;
    const bool solved = R.kept > (double)g.f.min_solve && R.fin;
    if (tid == 0) {
        double *o = g.records + (size_t)b * OFK_RECORD_DOUBLES, vu[3];
        write_record(o, R.v, R.r, R.rank, R.s3, om, sn + 16, ist ? ist + 6 : sn + 7, R.cnt, n, R.tracked, vu);
        o[14] = 0.0; o[15] = solved ? 1.0 : 0.0;
        double *fu = g.fused + (size_t)b * 8;
        if (g.f.filter) {
            if (solved && !g.defer) {
                double z[KF_MAX] = {0, 0, 0, 0, 0, 0};
                for (int k = 0; k < 3; ++k) z[k] = g.f.z_sign * (g.f.z_source ? vu[k] : R.v[k]);
                for (int k = 3; k < g.nm; ++k) z[k] = sn[22 + (k - 3)];
                kf_correct_dev(g.ns, g.nm, g.H, g.Rm, z, kx, kP);
            }
            kf_store(g.ns, b, kx, kP, g.kf_x, g.kf_P);
            double tr = 0.0;
            for (int i = 0; i < g.ns; ++i) tr += kP[i][i];
            for (int k = 0; k < 6; ++k) fu[k] = k < g.ns ? kx[k] : 0.0;
            fu[6] = tr; fu[7] = solved ? 1.0 : 0.0;
        } else {
            for (int k = 0; k < 3; ++k) fu[k] = solved ? vu[k] : (ist ? ist[k] : 0.0);
            fu[3] = fu[4] = fu[5] = fu[6] = 0.0; fu[7] = solved ? 1.0 : 0.0;
        }
        if (g.f.vel_overwrite && solved && ist) { ist[0] = vu[0]; ist[1] = vu[1]; ist[2] = vu[2]; }   // node:261
    }
}

void ofk_launch_stream_fuse_robust(hipStream_t s, const ofk_stream_in &in, double *imu_dv, int use_feas, double feas_T, const ofk_robust *r,
                                   double *work, double *weights, double *wtmp, double *stats)
{
    const rob_fuse_args ra = {{r->loss, r->c, r->iters, r->hypotheses, (unsigned)r->seed, (unsigned)(r->seed >> 32), r->drop}, work, weights, wtmp, stats};
    hipLaunchKernelGGL(k_stream_fuse_robust, dim3(in.batch), dim3(256), 0, s, make_fuse_args(in, imu_dv, use_feas, feas_T), ra);
}
