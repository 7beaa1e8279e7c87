// k_zones.inc — exclusion zones of a video stream (ofk.h: ofk_set_zones, rules 1-7), included by k_tracks.hip.  gfx950.
// Table of one stream: tab [OFK_ZONE_MAX][OFK_ZONE_INTS] = ttl, vertices, members, the vertices; mot [OFK_ZONE_MAX][4] = off, flow.

__device__ inline int zone_pos(float v) { return (int)fminf(fmaxf(v, -32768.f), 32767.f); }                       // rule 1; a NaN gives -32768
__device__ inline int zone_shift(float o) { return (int)fminf(fmaxf(rintf(o), -1048576.f), 1048576.f); }          // rule 5; rintf rounds half to even

// Rule 5 for the pixel (px, py) against n shifted vertices.  Every difference fits 32 bits (|p| < 2^15, |v| < 2^20 + 2^15), every
// product is formed in 64.  cross^2 is only formed where |cross| <= 2^25, to stay inside 64 bits when a zone has drifted far from p;
// that changes nothing: a hull's vertices lie within -32768..32767 per axis (rule 1), so L <= 2^33, r^2 L < 2^49 (r <= 255), and
// beyond the bound cross^2 > 2^50.
__device__ inline bool zone_inside(int px, int py, const int *vx, const int *vy, int n, int radius)
{
    if (n <= 0) return false;
    const long long r2 = (long long)radius * radius;
    bool conv = n >= 3, hit = false;
    const int ne = n <= 2 ? 1 : n;
    for (int i = 0; i < ne; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        const int ex = vx[j] - vx[i], ey = vy[j] - vy[i], qx = px - vx[i], qy = py - vy[i], sx = px - vx[j], sy = py - vy[j];
        const long long cr = (long long)ex * qy - (long long)ey * qx, t = (long long)qx * ex + (long long)qy * ey;
        const long long L = (long long)ex * ex + (long long)ey * ey, ac = cr < 0 ? -cr : cr;
        conv = conv && cr >= 0;
        hit = hit || (long long)qx * qx + (long long)qy * qy <= r2 || (long long)sx * sx + (long long)sy * sy <= r2 ||
              (t > 0 && t < L && ac <= (1ll << 25) && cr * cr <= r2 * L);
    }
    return hit || conv;
}

// Rule 7 for zone `z` of a table, by one lane per zone; returns whether the zone is still live.
__device__ inline bool zone_age(int *tab, float *mot, int z)
{
    int *t = tab + z * OFK_ZONE_INTS;
    float *m = mot + z * OFK_ZONE_FLOATS;
    const int ttl = t[0];
    if (ttl <= 0) return false;
    if (ttl == 1) {
        for (int k = 0; k < OFK_ZONE_INTS; ++k) t[k] = 0;
        m[0] = m[1] = m[2] = m[3] = 0.f;
        return false;
    }
    m[0] = m[0] + m[2]; m[1] = m[1] + m[3];
    t[0] = ttl - 1;
    return true;
}

__device__ inline long long zone_cross(unsigned o, unsigned a, unsigned p)      // keys: (x + 32768) << 16 | (y + 32768)
{
    const int ox = (int)(o >> 16), oy = (int)(o & 0xffff), ax = (int)(a >> 16), ay = (int)(a & 0xffff), qx = (int)(p >> 16), qy = (int)(p & 0xffff);
    return (long long)(ax - ox) * (qy - oy) - (long long)(ay - oy) * (qx - ox);
}

// Rules 1-4 (and 7 with do_age) for one stream per 256-thread workgroup.  Dynamic LDS, 12 bytes per point of pts_stride: positions and
// a hook / count / sort array (int each), labels and point indices (u16 each: a context holds at most 4096 points per image).
//   A  the rejects are compacted in index order; one that lies in a live zone marks the zone and stays out (rule 2)
//   B  labels: every point takes the smallest label among its linked neighbours and hooks its ROOT under it (ds_min on the hook
//      array, read and written in separate phases: the result of a sweep does not depend on the order of the lanes), then full
//      pointer jumping; the trees halve per sweep on a chain, whatever its index order, where plain relaxation walks its length
//   C  one lane deals the components out to the slots in ascending id; a slot's last owner is the one whose zone is built
//   D  per owned slot: rank sort of the members' positions by the workgroup, Andrew's chain by lane 0 with its two stacks in `work`
//      ([2 * pts_stride] ints per stream), the f64 flow sum in index order by lane 64
__global__ __launch_bounds__(256) void k_zones_update(const float *__restrict__ old_pts, const float *__restrict__ new_pts,
                                                      const uint8_t *__restrict__ st_pre, const uint8_t *__restrict__ keep,
                                                      const int *__restrict__ counts, int pts_stride, ofk_zones set, int *__restrict__ tab_all,
                                                      float *__restrict__ mot_all, int *__restrict__ stats_all, int *__restrict__ work_all,
                                                      int do_age)
{
    extern __shared__ int s_dyn[];
    int *s_xy = s_dyn, *s_hook = s_dyn + pts_stride;
    unsigned short *s_lab = (unsigned short *)(s_dyn + 2 * (size_t)pts_stride), *s_idx = s_lab + pts_stride;
    __shared__ int s_vx[OFK_ZONE_MAX][OFK_ZONE_VERTS], s_vy[OFK_ZONE_MAX][OFK_ZONE_VERTS];
    __shared__ int s_nv[OFK_ZONE_MAX], s_ttl[OFK_ZONE_MAX], s_ref[OFK_ZONE_MAX], s_owner[OFK_ZONE_MAX], s_ocnt[OFK_ZONE_MAX];
    __shared__ row_walk s_rows;
    __shared__ int s_cnt[4][2], s_flag, s_ins, s_evi;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = max(0, min(counts[b], pts_stride));
    const size_t base = (size_t)b * pts_stride;
    int *tab = tab_all + (size_t)b * OFK_ZONE_MAX * OFK_ZONE_INTS;
    float *mot = mot_all + (size_t)b * OFK_ZONE_MAX * OFK_ZONE_FLOATS;
    int *stats = stats_all + (size_t)b * OFK_ZONE_STATS;
    int *work = work_all + (size_t)b * 2 * pts_stride;

    for (int e = tid; e < OFK_ZONE_MAX * OFK_ZONE_VERTS; e += 256) {
        const int z = e / OFK_ZONE_VERTS, k = e - z * OFK_ZONE_VERTS;
        s_vx[z][k] = tab[z * OFK_ZONE_INTS + 3 + 2 * k] + zone_shift(mot[z * OFK_ZONE_FLOATS]);
        s_vy[z][k] = tab[z * OFK_ZONE_INTS + 4 + 2 * k] + zone_shift(mot[z * OFK_ZONE_FLOATS + 1]);
    }
    if (tid < OFK_ZONE_MAX) {
        const int ttl = tab[tid * OFK_ZONE_INTS];
        s_ttl[tid] = ttl; s_nv[tid] = ttl > 0 ? min(tab[tid * OFK_ZONE_INTS + 1], OFK_ZONE_VERTS) : 0; s_ref[tid] = 0; s_owner[tid] = -1; s_ocnt[tid] = 0;
    }
    rows_begin(s_rows);                                          // its barrier also: the zones are in LDS

    // A: k_rows.inc's walk, into LDS
    int c_rej = 0, c_abs = 0;                                    // wave-uniform
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool rej = i < n && st_pre[base + i] == 1 && keep[base + i] == 0;
        bool absorbed = false;
        int px = 0, py = 0;
        if (rej) {
            px = zone_pos(old_pts[2 * (base + i)]); py = zone_pos(old_pts[2 * (base + i) + 1]);
            for (int z = 0; z < OFK_ZONE_MAX; ++z)
                if (s_nv[z] > 0 && zone_inside(px, py, s_vx[z], s_vy[z], s_nv[z], set.radius)) { s_ref[z] = 1; absorbed = true; }
        }
        const bool in = rej && !absorbed;
        c_rej += __popcll(__ballot(rej)); c_abs += __popcll(__ballot(absorbed));
        const int pos = rows_place(s_rows, in);
        if (in) { s_xy[pos] = (int)((unsigned)(px & 0xffff) | ((unsigned)py << 16)); s_idx[pos] = (unsigned short)i; s_lab[pos] = (unsigned short)pos; }
        rows_next(s_rows);
    }
    if (lane == 0) { s_cnt[wave][0] = c_rej; s_cnt[wave][1] = c_abs; }
    __syncthreads();
    const int m = s_rows.base;
    if (tid < OFK_ZONE_MAX && s_ref[tid]) { s_ttl[tid] = set.ttl; tab[tid * OFK_ZONE_INTS] = set.ttl; }

    // B
    int sweeps = 0;
    while (m > 0) {
        ++sweeps;
        for (int j = tid; j < m; j += 256) s_hook[j] = j;
        if (tid == 0) s_flag = 0;
        __syncthreads();
        for (int j = tid; j < m; j += 256) {
            const int xy = s_xy[j], x = (short)(xy & 0xffff), y = xy >> 16;
            int mn = s_lab[j];
            for (int k = 0; k < m; ++k) {
                const int o = s_xy[k], dx = x - (short)(o & 0xffff), dy = y - (o >> 16);
                if (abs(dx) < set.link && abs(dy) < set.link) mn = min(mn, (int)s_lab[k]);
            }
            atomicMin(&s_hook[s_lab[j]], mn);
        }
        __syncthreads();
        for (int j = tid; j < m; j += 256)
            if (s_lab[j] == j && s_hook[j] < j) { s_lab[j] = (unsigned short)s_hook[j]; s_flag = 1; }
        __syncthreads();
        const int hooked = s_flag;
        __syncthreads();
        if (!hooked) break;
        while (true) {                                           // pointer jumping: a label read late is an ancestor all the same
            if (tid == 0) s_flag = 0;
            __syncthreads();
            for (int j = tid; j < m; j += 256) {
                const int l = s_lab[j], ll = s_lab[l];
                if (ll != l) { s_lab[j] = (unsigned short)ll; s_flag = 1; }
            }
            __syncthreads();
            const int moved = s_flag;
            __syncthreads();
            if (!moved) break;
        }
    }

    // C
    for (int j = tid; j < m; j += 256) s_hook[j] = 0;
    __syncthreads();
    for (int j = tid; j < m; j += 256) atomicAdd(&s_hook[s_lab[j]], 1);
    __syncthreads();
    if (tid == 0) {
        int ins = 0, evi = 0;
        for (int r = 0; r < m; ++r) {
            if (s_lab[r] != r || s_hook[r] < set.min_members) continue;
            int slot = 0;
            for (int z = 1; z < set.max_zones; ++z)
                if (s_ttl[z] < s_ttl[slot]) slot = z;
            if (s_ttl[slot] > 0) ++evi;
            s_ttl[slot] = set.ttl; s_owner[slot] = r; s_ocnt[slot] = s_hook[r];
            ++ins;
        }
        s_ins = ins; s_evi = evi;
    }
    __syncthreads();

    // D
    for (int z = 0; z < OFK_ZONE_MAX; ++z) {
        const int root = s_owner[z], cnt = s_ocnt[z];            // workgroup-uniform
        if (root < 0) continue;
        for (int j = tid; j < m; j += 256) {
            if (s_lab[j] != root) continue;
            const int xy = s_xy[j];
            const unsigned key = ((unsigned)((short)(xy & 0xffff) + 32768) << 16) | (unsigned)((xy >> 16) + 32768);
            int rank = 0;
            for (int k = 0; k < m; ++k) {
                if (s_lab[k] != root) continue;
                const int o = s_xy[k];
                const unsigned ko = ((unsigned)((short)(o & 0xffff) + 32768) << 16) | (unsigned)((o >> 16) + 32768);
                rank += ko < key || (ko == key && k < j);
            }
            s_hook[rank] = (int)key;
        }
        __syncthreads();
        int *t = tab + z * OFK_ZONE_INTS;
        if (tid == 0) {
            unsigned *srt = (unsigned *)s_hook;
            int u = 0;
            for (int i = 0; i < cnt; ++i)
                if (u == 0 || srt[i] != srt[u - 1]) srt[u++] = srt[i];
            int nv = 0;
            auto put = [&](unsigned key) { t[3 + 2 * nv] = (int)(key >> 16) - 32768; t[4 + 2 * nv] = (int)(key & 0xffff) - 32768; ++nv; };
            if (u <= 2) {
                for (int i = 0; i < u; ++i) put(srt[i]);
            } else {
                unsigned *lo = (unsigned *)work, *up = lo + pts_stride;
                int nlo = 0, nup = 0;
                for (int i = 0; i < u; ++i) {
                    while (nlo >= 2 && zone_cross(lo[nlo - 2], lo[nlo - 1], srt[i]) <= 0) --nlo;
                    lo[nlo++] = srt[i];
                }
                for (int i = u - 1; i >= 0; --i) {
                    while (nup >= 2 && zone_cross(up[nup - 2], up[nup - 1], srt[i]) <= 0) --nup;
                    up[nup++] = srt[i];
                }
                if (nlo - 1 + nup - 1 > OFK_ZONE_VERTS) {        // the bounding box; x is the sort's major key
                    unsigned y0 = 0xffff, y1 = 0;
                    for (int i = 0; i < u; ++i) { y0 = min(y0, srt[i] & 0xffff); y1 = max(y1, srt[i] & 0xffff); }
                    const unsigned x0 = srt[0] & 0xffff0000u, x1 = srt[u - 1] & 0xffff0000u;
                    put(x0 | y0); put(x1 | y0); put(x1 | y1); put(x0 | y1);
                } else {
                    for (int i = 0; i + 1 < nlo; ++i) put(lo[i]);
                    for (int i = 0; i + 1 < nup; ++i) put(up[i]);
                }
            }
            for (int k = nv; k < OFK_ZONE_VERTS; ++k) t[3 + 2 * k] = t[4 + 2 * k] = 0;
            t[0] = set.ttl; t[1] = nv; t[2] = cnt;
            mot[z * OFK_ZONE_FLOATS] = 0.f; mot[z * OFK_ZONE_FLOATS + 1] = 0.f;
        } else if (tid == 64) {
            double fx = 0.0, fy = 0.0;
            for (int j = 0; j < m; ++j) {
                if (s_lab[j] != root) continue;
                const size_t pi = base + s_idx[j];
                fx += (double)new_pts[2 * pi] - (double)old_pts[2 * pi]; fy += (double)new_pts[2 * pi + 1] - (double)old_pts[2 * pi + 1];
            }
            mot[z * OFK_ZONE_FLOATS + 2] = (float)(fx / (double)cnt); mot[z * OFK_ZONE_FLOATS + 3] = (float)(fy / (double)cnt);
        }
        __syncthreads();
    }

    if (tid == 0) {
        int ref = 0;
        for (int z = 0; z < OFK_ZONE_MAX; ++z) ref += s_ref[z];
        stats[1] = s_ins; stats[2] = ref; stats[3] = s_evi;
        stats[4] = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0]; stats[5] = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
        stats[6] = sweeps; stats[7] = 0;                      // the eighth slot is reserved
    }
    if (do_age && wave == 0) {                                   // behind the barrier that ended D: the table is the workgroup's own
        const bool live = lane < OFK_ZONE_MAX && zone_age(tab, mot, lane);
        const int nlive = __popcll(__ballot(live));
        if (lane == 0) stats[0] = nlive;
    }
}

// Rule 7 alone, for the steps whose mask is drawn between the update and the ageing.  One wave per stream.
__global__ __launch_bounds__(64) void k_zones_age(int *__restrict__ tab_all, float *__restrict__ mot_all, int *__restrict__ stats_all)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const bool live = lane < OFK_ZONE_MAX && zone_age(tab_all + (size_t)b * OFK_ZONE_MAX * OFK_ZONE_INTS, mot_all + (size_t)b * OFK_ZONE_MAX * OFK_ZONE_FLOATS, lane);
    const int nlive = __popcll(__ballot(live));
    if (lane == 0) stats_all[(size_t)b * OFK_ZONE_STATS] = nlive;
}

// Rule 6: zero the pixels of every live zone.  grid (tile, zone, stream), 256 threads; a workgroup walks the 64 x 16 tiles of its
// zone's bounding box (grown by the radius, clamped to the image) in steps of the grid; the edge list sits in LDS.  Writes zero bytes
// only, like k_disc_mask.  limit != NULL: streams whose limit is <= 0 (no re-detection this step) are skipped.
__global__ __launch_bounds__(256) void k_zone_mask(uint8_t *__restrict__ mask, size_t mask_stride, int h, int w, const int *__restrict__ tab_all,
                                                   const float *__restrict__ mot_all, int radius, const int *__restrict__ limit)
{
    __shared__ int s_vx[OFK_ZONE_VERTS], s_vy[OFK_ZONE_VERTS];
    const int z = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    if (limit && limit[b] <= 0) return;
    const int *t = tab_all + ((size_t)b * OFK_ZONE_MAX + z) * OFK_ZONE_INTS;
    const float *mo = mot_all + ((size_t)b * OFK_ZONE_MAX + z) * OFK_ZONE_FLOATS;
    const int nv = min(t[1], OFK_ZONE_VERTS);
    if (t[0] <= 0 || nv <= 0) return;                            // workgroup-uniform, as the return above
    if (tid < nv) { s_vx[tid] = t[3 + 2 * tid] + zone_shift(mo[0]); s_vy[tid] = t[4 + 2 * tid] + zone_shift(mo[1]); }
    __syncthreads();
    int x0 = s_vx[0], x1 = s_vx[0], y0 = s_vy[0], y1 = s_vy[0];
    for (int k = 1; k < nv; ++k) { x0 = min(x0, s_vx[k]); x1 = max(x1, s_vx[k]); y0 = min(y0, s_vy[k]); y1 = max(y1, s_vy[k]); }
    x0 = max(0, x0 - radius); x1 = min(w - 1, x1 + radius); y0 = max(0, y0 - radius); y1 = min(h - 1, y1 + radius);
    if (x0 > x1 || y0 > y1) return;                              // the zone has left the image
    const int tw = (x1 - x0) / 64 + 1, th = (y1 - y0) / 16 + 1;
    uint8_t *m = mask + (size_t)b * mask_stride;
    for (int tile = blockIdx.x; tile < tw * th; tile += gridDim.x) {
        const int ty = tile / tw, tx = tile - ty * tw;
        const int x = x0 + tx * 64 + (tid & 63);
        for (int k = 0; k < 4; ++k) {
            const int y = y0 + ty * 16 + (tid >> 6) + 4 * k;
            if (x <= x1 && y <= y1 && zone_inside(x, y, s_vx, s_vy, nv, radius)) m[(size_t)y * w + x] = 0;
        }
    }
}

void ofk_launch_zones_update(hipStream_t s, const float *old_pts, const float *new_pts, const uint8_t *st_pre, const uint8_t *keep, const int *counts,
                             int pts_stride, const ofk_zones *set, int *tab, float *mot, int *stats, int *work, int do_age, int batch)
{
    hipLaunchKernelGGL(k_zones_update, dim3(batch), dim3(256), (size_t)pts_stride * 12, s, old_pts, new_pts, st_pre, keep, counts, pts_stride, *set,
                       tab, mot, stats, work, do_age);
}

void ofk_launch_zones_age(hipStream_t s, int *tab, float *mot, int *stats, int batch)
{
    hipLaunchKernelGGL(k_zones_age, dim3(batch), dim3(64), 0, s, tab, mot, stats);
}

void ofk_launch_zone_mask(hipStream_t s, uint8_t *mask, size_t mask_stride, int h, int w, const int *tab, const float *mot, int radius,
                          const int *limit, int batch)
{
    const int tiles = ((w + 63) / 64) * ((h + 15) / 16);
    hipLaunchKernelGGL(k_zone_mask, dim3(tiles < 32 ? tiles : 32, OFK_ZONE_MAX, batch), dim3(256), 0, s, mask, mask_stride, h, w, tab, mot, radius, limit);
}
