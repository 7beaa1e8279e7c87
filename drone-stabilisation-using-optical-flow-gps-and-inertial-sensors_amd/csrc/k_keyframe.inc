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

__device__ __forceinline__ void kf_fresh_row(const ofk_kf_rows &t, size_t w) { t.key_xy[2 * w] = 0.f; t.key_xy[2 * w + 1] = 0.f; t.member[w] = 0; }   // no member

// the rows of freshly detected tracks (beside k_track_table_begin): no members, no keyframe, the position at zero
__global__ __launch_bounds__(256) void k_keyframe_begin(ofk_kf_rows t, const int *__restrict__ counts, int stride)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[b], 0), stride);
    const size_t base = (size_t)b * stride;
    for (int i = tid; i < n; i += 256) kf_fresh_row(t, base + i);
    kf_clear_state(t, b, tid, true);
}

// behind k_replace_tracks (beside k_track_table_replace): the streams with a budget lose their keyframe and keep their position
__global__ __launch_bounds__(256) void k_keyframe_replace(ofk_kf_rows t, const int *__restrict__ limit, const int *__restrict__ new_counts,
                                                          int stride)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!rows_stream_on(b, 0, gridDim.x, limit)) return;
    const int n = min(max(new_counts[b], 0), stride);
    const size_t base = (size_t)b * stride;
    for (int i = tid; i < n; i += 256) kf_fresh_row(t, base + i);
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

// Rule 1: R = exp([omega]x) R0, entry by entry as ofk.h writes it (k_stab_pose forms the same product from a copy of the state)
__device__ __forceinline__ void kf_rotate(double o0, double o1, double o2, const double *R0, double *R)
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
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (E[3 * i] * R0[j] + E[3 * i + 1] * R0[3 + j]) + E[3 * i + 2] * R0[6 + j];
}

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
// so that the gate and the residual need no broadcast.  The compaction is the table's, k_rows.inc's walk.  Thread 0 writes the state
// and the record at the end; nothing reads them behind the first barrier.
// The body is k_keyframe_body.inc, which k_keyframe_rot.inc compiles a second time with the joint rule 2 (KF_ROT 1).
__global__ __launch_bounds__(256) void k_keyframe_step(ofk_kf_rows t, ofk_kf_in in, kf_cfg cfg)
{
#define KF_ROT 0
#define KF_MAP 0
#include "k_keyframe_body.inc"
#undef KF_MAP
#undef KF_ROT
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
