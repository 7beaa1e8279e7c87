// k_track_table.inc — the track table of a video stream (ofk.h: ofk_set_track_table): an id, an age, a birth step, a birth position
// and the last flow per track row, kept in step with k_update_tracks / k_replace_tracks, and LK's start positions from the last
// flow.  Included by k_tracks.hip.  The rows of one stream are only ever touched by that stream's workgroup, with plain vector
// stores and no atomics, so a second launch on the same inputs gives the same bits.

// A fresh row at index w: the track `id`, born in `step` at (x, y), not tracked yet.
__device__ __forceinline__ void tt_fresh_row(const ofk_tt_rows &t, size_t w, unsigned id, int step, float x, float y)
{
    t.ids[w] = id; t.age[w] = 0; t.birth_step[w] = step; t.birth_xy[2 * w] = x; t.birth_xy[2 * w + 1] = y; t.flow_xy[2 * w] = 0.f; t.flow_xy[2 * w + 1] = 0.f;
}

// rule 1: the table of tracks that have just been detected.  One workgroup per stream.
__global__ __launch_bounds__(256) void k_track_table_begin(ofk_tt_rows t, const float *__restrict__ pts, const int *__restrict__ counts,
                                                           int stride)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[b], 0), stride);
    const size_t base = (size_t)b * stride;
    for (int i = tid; i < n; i += 256) tt_fresh_row(t, base + i, (unsigned)i, 0, pts[2 * (base + i)], pts[2 * (base + i) + 1]);
    if (tid == 0) {
        t.head[2 * b] = 0; t.head[2 * b + 1] = n;
        int *s = t.stats + (size_t)b * OFK_TT_STATS;
        s[0] = n; s[1] = 0; s[2] = 0; s[3] = n; s[4] = 0; s[5] = 0; s[6] = n; s[7] = 0;
    }
}

// rule 2, behind k_replace_tracks: the streams with a budget start over with fresh ids.  One workgroup per stream.
__global__ __launch_bounds__(256) void k_track_table_replace(ofk_tt_rows t, const int *__restrict__ limit, const float *__restrict__ new_pts,
                                                             const int *__restrict__ new_counts, int stride)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!rows_stream_on(b, 0, gridDim.x, limit)) return;
    const int n = min(max(new_counts[b], 0), stride);
    const int step = t.head[2 * b];
    const unsigned nid = (unsigned)t.head[2 * b + 1];
    const int before = t.stats[(size_t)b * OFK_TT_STATS];
    const size_t base = (size_t)b * stride;
    __syncthreads();                                            // every thread holds the head before one of them rewrites it
    for (int i = tid; i < n; i += 256) tt_fresh_row(t, base + i, nid + (unsigned)i, step, new_pts[2 * (base + i)], new_pts[2 * (base + i) + 1]);
    if (tid == 0) {
        t.head[2 * b + 1] = (int)(nid + (unsigned)n);
        int *s = t.stats + (size_t)b * OFK_TT_STATS;
        s[0] = n; s[1] = 0; s[2] = before; s[3] = n; s[4] = 0; s[5] = step; s[6] = (int)(nid + (unsigned)n); s[7] = 0;
    }
}

// rules 3 and 6, in front of k_update_tracks and with its walk (k_rows.inc): the rows of the kept points move up in order, in place,
// the re-detected corners are appended.  One workgroup per stream.  The seeded count is a ballot summed per wave and across the waves
// through LDS; the oldest age is an LDS maximum.
__global__ __launch_bounds__(256) void k_track_table_update(ofk_tt_rows t, const float *__restrict__ prev_pts, const float *__restrict__ next_pts,
                                                            const uint8_t *__restrict__ status, const int *__restrict__ counts_in, int stride,
                                                            const float *__restrict__ new_pts, const int *__restrict__ new_counts,
                                                            int max_total, int seed_on, float gain)
{
    __shared__ row_walk s_rows;
    __shared__ int s_seed[4], s_age[256];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(counts_in[b], 0), stride);
    const int step = t.head[2 * b];
    const unsigned nid = (unsigned)t.head[2 * b + 1];
    const size_t base = (size_t)b * stride;
    int c_seed = 0, oldest = 0;                                  // wave-uniform / per thread
    rows_begin(s_rows);
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool in = i < n;
        const size_t r = base + (in ? i : 0);
        const bool keep = in && status[r] != 0;
        const unsigned id = t.ids[r];
        const int age = t.age[r], bs = t.birth_step[r];
        const float bx = t.birth_xy[2 * r], by = t.birth_xy[2 * r + 1], fx = t.flow_xy[2 * r], fy = t.flow_xy[2 * r + 1];
        const float px = prev_pts[2 * r], py = prev_pts[2 * r + 1], nx = next_pts[2 * r], ny = next_pts[2 * r + 1];
        if (in) t.step_ids[r] = id;
        const float tx = gain * fx, ty = gain * fy;
        const float sx = px + tx, sy = py + ty;
        const bool seeded = in && seed_on && age >= 1 && fabsf(sx) <= 1e6f && fabsf(sy) <= 1e6f;
        c_seed += __popcll(__ballot(seeded));
        const int pos = rows_place(s_rows, keep);
        if (keep) {
            const size_t w = base + pos;
            t.ids[w] = id; t.age[w] = age + 1; t.birth_step[w] = bs;
            t.birth_xy[2 * w] = bx; t.birth_xy[2 * w + 1] = by;
            t.flow_xy[2 * w] = nx - px; t.flow_xy[2 * w + 1] = ny - py;
            oldest = max(oldest, age + 1);
        }
        rows_next(s_rows);
    }
    const int kept = s_rows.base;
    const int extra = rows_extra(new_counts, b, max_total, stride, kept);
    for (int i = tid; i < extra; i += 256) tt_fresh_row(t, base + kept + i, nid + (unsigned)i, step + 1, new_pts[2 * (base + i)], new_pts[2 * (base + i) + 1]);
    s_age[tid] = oldest;
    if (lane == 0) s_seed[wave] = c_seed;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) s_age[tid] = max(s_age[tid], s_age[tid + h]);
        __syncthreads();
    }
    if (tid == 0) {
        const int next_id = (int)(nid + (unsigned)extra);
        t.head[2 * b] = step + 1; t.head[2 * b + 1] = next_id;
        int *s = t.stats + (size_t)b * OFK_TT_STATS;
        s[0] = kept + extra; s[1] = kept; s[2] = n - kept; s[3] = extra; s[4] = s_age[0]; s[5] = step + 1; s[6] = next_id;
        s[7] = s_seed[0] + s_seed[1] + s_seed[2] + s_seed[3];
    }
}

// rule 5: LK's start positions from the tracks' last flow, written where LK reads them.  One thread per point.  The build has no FMA
// contraction, so the product and the sum round separately, as ofk.h states.
__global__ __launch_bounds__(256) void k_track_seed(const float *__restrict__ pts, const int *__restrict__ counts, int stride,
                                                    const int *__restrict__ age, const float *__restrict__ flow_xy, float gain, int keep_age0,
                                                    float *__restrict__ seed)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= stride || p >= counts[b]) return;
    const size_t pi = (size_t)b * stride + p;
    const float x = pts[2 * pi], y = pts[2 * pi + 1];
    if (age[pi] >= 1) {
        const float tx = gain * flow_xy[2 * pi], ty = gain * flow_xy[2 * pi + 1];
        const float sx = x + tx, sy = y + ty;
        const bool ok = fabsf(sx) <= 1e6f && fabsf(sy) <= 1e6f;  // false for NaN and infinity too
        seed[2 * pi] = ok ? sx : x; seed[2 * pi + 1] = ok ? sy : y;
    } else if (!keep_age0) {
        seed[2 * pi] = x; seed[2 * pi + 1] = y;
    }
}

void ofk_launch_track_table_begin(hipStream_t s, const ofk_tt_rows &t, const float *pts, const int *counts, int stride, int batch)
{
    hipLaunchKernelGGL(k_track_table_begin, dim3(batch), dim3(256), 0, s, t, pts, counts, stride);
}

void ofk_launch_track_table_replace(hipStream_t s, const ofk_tt_rows &t, const int *limit, const float *new_pts, const int *new_counts,
                                    int stride, int batch)
{
    hipLaunchKernelGGL(k_track_table_replace, dim3(batch), dim3(256), 0, s, t, limit, new_pts, new_counts, stride);
}

void ofk_launch_track_table_update(hipStream_t s, const ofk_tt_rows &t, const float *prev_pts, const float *next_pts, const uint8_t *status,
                                   const int *counts_in, int stride, const float *new_pts, const int *new_counts, int max_total, int seed_on,
                                   float gain, int batch)
{
    hipLaunchKernelGGL(k_track_table_update, dim3(batch), dim3(256), 0, s, t, prev_pts, next_pts, status, counts_in, stride, new_pts,
                       new_counts, max_total, seed_on, gain);
}

void ofk_launch_track_seed(hipStream_t s, const float *pts, const int *counts, int stride, const int *age, const float *flow_xy, float gain,
                           int keep_age0, float *seed, int batch)
{
    hipLaunchKernelGGL(k_track_seed, dim3((stride + 255) / 256, batch), dim3(256), 0, s, pts, counts, stride, age, flow_xy, gain, keep_age0,
                       seed);
}
