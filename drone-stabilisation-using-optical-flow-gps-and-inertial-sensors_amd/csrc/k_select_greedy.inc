// Body of k_select_greedy<NT> (SEL_GRID 0: the text the kernel had before the corner grid existed, hence the same code, registers
// and LDS) and of k_select_greedy_grid<NT> (SEL_GRID 1: ofk.h's per-cell cap - the counts of OFK_GRID_MAX_CELLS cells in LDS, a
// same-cell matrix beside the conflict matrix of every 64-candidate round, a running rank over the chunks for max_rank and the
// statistics).  Included by k_corners.hip inside the two kernels' braces.
    constexpr int NW = NT / 64;
    constexpr int NB = NT > SEL_NB ? NT : SEL_NB;               // histogram bins per refinement level of the generic path (>= one per thread)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#if SEL_GRID
    if (tid == 0) { gstats[2 * b] = 0; gstats[2 * b + 1] = 0; }  // {accepted, examined} of an image that returns early; plain stores, one thread
#endif
    const int max_corners = limit ? min(max_corners_all, limit[b]) : max_corners_all;
    if (max_corners <= 0) { if (tid == 0) counts[b] = 0; return; }
    unsigned long long *s_key = reinterpret_cast<unsigned long long *>(sel_smem);
    unsigned *s_idx = reinterpret_cast<unsigned *>(sel_smem);
    unsigned *s_hist = reinterpret_cast<unsigned *>(sel_smem);
    volatile unsigned short *s_grid = reinterpret_cast<volatile unsigned short *>(sel_smem + 4 * (size_t)tgtA);
    int *s_acc = reinterpret_cast<int *>(sel_smem + 6 * (size_t)tgtA);
    volatile unsigned short *s_next = reinterpret_cast<volatile unsigned short *>(sel_smem + 6 * (size_t)tgtA + 4 * (size_t)max_corners_all);
    __shared__ unsigned long long s_conf[128];                  // conflict matrices of the current and the next greedy round
    __shared__ unsigned s_w[NW];
    __shared__ int s_n, s_nacc, s_D, s_cum;
#if SEL_GRID
    __shared__ unsigned s_occ[OFK_GRID_MAX_CELLS / 2];          // corners per cell, two u16 counts per dword (<= 2 max_pts <= 8192 each)
    __shared__ unsigned long long s_same[128];                  // same-cell matrices of the current and the next greedy round
    __shared__ int s_nfull, s_exam;                             // cells with occ >= cap; rank of the last decided candidate + 1
    __shared__ int s_stop[2];                                   // [round & 1]: the pass ended before this round (budget met or every cell full)
#endif

    const unsigned long long *cand = cand_all + (size_t)b * cand_cap;
    const unsigned mb = maxbits[b * OFK_MAX_STRIDE];
    if (tid == 0) { s_nacc = 0; s_n = 0; counts[b] = 0; }
#if SEL_GRID
    if (tid == 0) { s_nfull = 0; s_exam = 0; }
#endif
    if (mb == 0) return;
    const float thr = (float)((double)__uint_as_float(mb) * quality);
    // keys of interest: [a, kend);  v > thr  <=>  key < (~bits(thr)) << 32
    const unsigned long long kend = (unsigned long long)(~__float_as_uint(thr)) << 32;
    unsigned long long a = (unsigned long long)(~mb) << 32;     // smallest possible key (value == max)
    const float md2 = min_distance * min_distance;
    const bool use_dist = min_distance >= 1.f;
    const int total_keys = cand_count[b * OFK_CNT_STRIDE];
    if (total_keys > cand_cap) {                                // flat list overflow (uniform): the host reports OFK_E_CAPACITY
        if (tid == 0) counts[b] = -1;
        return;
    }
    const int C = total_keys;
    if (C <= 0 || !(thr < __uint_as_float(mb))) return;         // nothing is strictly above the threshold
    const int tgt = sel_tgt(max_corners);
    const int gw = (w + cs - 1) / cs, gh = (h + cs - 1) / cs;
    const int nsel = min(cand_count[b * OFK_CNT_STRIDE + SEL_CNT_PICK], min(tgt, sel_stride));
    const int Dbins = cand_count[b * OFK_CNT_STRIDE + SEL_CNT_BINS];
    bool fast = Dbins > 0;                                      // k_select_pick made the first cut
    bool grid_ready = false;
#if SEL_GRID
    // ---- initial occupancy: the listed points whose truncated position lies in the image, counted into their cells by all threads
    const int ncells = ggw * ((h + gcell - 1) / gcell);         // <= OFK_GRID_MAX_CELLS (the host refuses more)
    for (int i = tid; i < OFK_GRID_MAX_CELLS / 2; i += NT) s_occ[i] = 0;           // 1024 / NT trips
    __syncthreads();
    if (occ_pts) {
        const int no = min(occ_counts[b], occ_stride);
        for (int i = tid; i < no; i += NT) {                    // at most occ_stride / NT + 1 trips
            const float px = occ_pts[((size_t)b * occ_stride + i) * 2], py = occ_pts[((size_t)b * occ_stride + i) * 2 + 1];
            if (px > -1.f && px < (float)w && py > -1.f && py < (float)h) {         // (int)px in [0, w), (int)py in [0, h); a NaN fails
                const int c = ((int)py / gcell) * ggw + (int)px / gcell;
                atomicAdd(&s_occ[c >> 1], 1u << ((c & 1) * 16));
            }
        }
    }
    __syncthreads();
    for (int c = tid; c < ncells; c += NT)                      // at most OFK_GRID_MAX_CELLS / NT trips
        if ((int)((s_occ[c >> 1] >> ((c & 1) * 16)) & 0xffffu) >= gcap) atomicAdd(&s_nfull, 1);
    __syncthreads();
    if (s_nfull >= ncells) return;                              // the list closes every cell (uniform): nothing is examined, {0, 0} stands
    int rank_base = 0;                                          // rank of the current chunk's first candidate
#endif
    __syncthreads();
    while (true) {
        unsigned long long T = kend;
        int n = 0;
        if (fast) {
            const unsigned a_hi = ~mb, width = (unsigned)(kend >> 32) - a_hi;
            const int hshift = width <= SEL_HB ? 0 : 32 - __clz((int)(width - 1)) - 10;
            const unsigned long long cut = ((unsigned long long)a_hi + ((unsigned long long)Dbins << hshift)) << 32;
            T = cut < kend ? cut : kend;
            n = nsel;
            const unsigned long long *src = sel_keys + (size_t)b * sel_stride;
            for (int i = tid; i < n; i += NT) s_key[i] = src[i];
        } else {
            if (!(a < kend)) break;
            // ---- choose T in (a, kend] so that 1 <= #{a <= key < T} <= cap (or detect that none is left)
            const int cap = tgtA / 2;                           // later rounds sort inside the index region: the grid and the accepted set live behind it
            unsigned long long curA = a, curB = kend;
            int taken = 0;
            bool have_cut = false;
            for (int level = 0; level < 9; ++level) {
                const unsigned long long width = curB - curA;
                const int shift = width <= NB ? 0 : 64 - __clzll((long long)(width - 1)) - (NB == 512 ? 9 : 10);
                const int nb = (int)((width - 1) >> shift) + 1;
                for (int i = tid; i < NB; i += NT) s_hist[i] = 0;
                if (tid == 0) { s_D = 0; s_cum = 0; }
                __syncthreads();
                for (int i0 = tid; i0 < C; i0 += 4 * NT) {
                    unsigned long long key[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { const int i = i0 + q * NT; key[q] = i < C ? cand[i] : ~0ull; }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (key[q] >= curA && key[q] < curB) atomicAdd(&s_hist[(unsigned)((key[q] - curA) >> shift)], 1u);
                }
                __syncthreads();
                // inclusive prefix over the bins (NB / NT per thread); D = #bins whose inclusive prefix fits the budget
                constexpr int BPT = NB / NT;
                unsigned hv[BPT], loc = 0;
#pragma unroll
                for (int q = 0; q < BPT; ++q) { hv[q] = s_hist[BPT * tid + q]; loc += hv[q]; }
                unsigned incl = loc;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const unsigned n_ = __shfl_up(incl, o); if (lane >= o) incl += n_; }
                if (lane == 63) s_w[wave] = incl;
                __syncthreads();
                unsigned woff = 0, total = 0;
#pragma unroll
                for (int q = 0; q < NW; ++q) { const unsigned ws = s_w[q]; if (q < wave) woff += ws; total += ws; }
                const int budget = cap - taken;
                unsigned pre = woff + incl - loc;               // exclusive prefix of this thread's first bin
                int fit = 0;
#pragma unroll
                for (int q = 0; q < BPT; ++q) { pre += hv[q]; fit += (int)pre <= budget; }
                if (fit) atomicAdd(&s_D, fit);
                __syncthreads();
                const int D = min(s_D, nb);
                // the thread that owns bin D - 1 knows the keys below the cut (prefixes are non-decreasing: the fitting bins are a leading run)
                if (D > 0 && (D - 1) / BPT == tid) {
                    unsigned p2 = woff + incl - loc;
#pragma unroll
                    for (int q = 0; q < BPT; ++q) { p2 += hv[q]; if (BPT * tid + q == D - 1) s_cum = (int)p2; }
                }
                __syncthreads();
                taken += s_cum;
                if (level == 0 && total == 0) break;            // no key left in [a, kend)
                if (D >= nb) { T = curB; have_cut = true; break; }             // everything in [curA, curB) fits
                const unsigned long long newA = curA + ((unsigned long long)D << shift);
                if (taken >= cap / 4) { T = newA; have_cut = true; break; }
                curA = newA;                                    // descend into the first bin that did not fit
                const unsigned long long bin_end = newA + (1ull << shift);
                if (bin_end < curB) curB = bin_end;
                __syncthreads();                                // s_D / s_cum are reset at the top of the next level
            }
            if (!have_cut) break;                               // (nine levels of nine bits always reach single keys: a cut exists unless nothing is left)
            // ---- gather keys in [a, T)
            __syncthreads();
            if (tid == 0) s_n = 0;
            __syncthreads();
            for (int i0 = tid; i0 < C; i0 += 4 * NT) {
                unsigned long long key[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { const int i = i0 + q * NT; key[q] = i < C ? cand[i] : ~0ull; }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (key[q] >= a && key[q] < T) { const int slot = atomicAdd(&s_n, 1); if (slot < cap) s_key[slot] = key[q]; }
            }
            __syncthreads();
            n = min(s_n, cap);
        }
        fast = false;
        int npad = 64;
        while (npad < n) npad <<= 1;
        for (int i = n + tid; i < npad; i += NT) s_key[i] = ~0ull;
        __syncthreads();
        // ---- bitonic sort ascending.  Element i is handled by thread i % NT: for j >= NT both partners of a compare-exchange
        // belong to the same thread, for j < 64 to the same wave (LDS executes a wave's accesses in order) — only the steps with
        // 64 <= j < NT exchange between waves and need the workgroup barrier, before and after.
        for (int kk = 2; kk <= npad; kk <<= 1)
            for (int j = kk >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < npad; i += NT) {
                    const int p = i ^ j;
                    if (p > i) {
                        const unsigned long long x0 = s_key[i], x1 = s_key[p];
                        const bool up = (i & kk) == 0;
                        if ((x0 > x1) == up) { s_key[i] = x1; s_key[p] = x0; }
                    }
                }
                const int nj = j > 1 ? (j >> 1) : kk;           // the step that follows (first step of the next stage: j = kk)
                if ((j >= 64 && j < NT) || (nj >= 64 && nj < NT)) __syncthreads();
                else __builtin_amdgcn_wave_barrier();
            }
        __syncthreads();
        // ---- sorted keys -> sorted pixel positions x | y << 16, in place (the key holds ~index: equal responses sort by DESCENDING
        //      index); the two divisions per candidate happen here, once, spread over the whole workgroup
        {
            unsigned idxv[OFK_CHUNK / NT];
#pragma unroll
            for (int q = 0; q < OFK_CHUNK / NT; ++q) {
                const int i = tid + q * NT;
                const unsigned idx = i < n ? ~(unsigned)(s_key[i] & 0xffffffffu) : 0u;
                const unsigned y = idx / (unsigned)w;
                idxv[q] = (idx - y * (unsigned)w) | (y << 16);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < OFK_CHUNK / NT; ++q) { const int i = tid + q * NT; if (i < n) s_idx[i] = idxv[q]; }
        }
#if SEL_GRID
        const int chunk_n = n;
        if (max_rank > 0) n = min(n, max_rank - rank_base);     // only the first max_rank candidates are ever examined (rank_base < max_rank here)
#endif
        if (!grid_ready) {                                      // the first sort may have run over the grid's place
            unsigned *g32 = reinterpret_cast<unsigned *>(sel_smem + 4 * (size_t)tgtA);
            for (int i = tid; i < tgtA / 2; i += NT) g32[i] = 0xffffffffu;
            grid_ready = true;
        }
        __syncthreads();
        // ---- greedy over the sorted chunk, 64 candidates per round, software-pipelined over the waves: while wave 0 resolves round r
        //      (accepted-set test through the grid, acceptance sweeps, stores), the other waves build the 64 x 64 conflict matrix of
        //      round r + 1 into the other half of s_conf - one workgroup barrier per round, the matrix off wave 0's path
        auto conflict_rows = [&](int base_, unsigned long long *conf) {
            // rows of the matrix of the round starting at base_, shared by the waves 1 .. NW-1 (all of it by wave 0 when alone)
            const int ci_ = base_ + lane;
            const unsigned xy_ = ci_ < n ? s_idx[ci_] : 0u;
            const int x_ = (int)(xy_ & 0xffffu), y_ = (int)(xy_ >> 16);
#if SEL_GRID
            const int c_ = (y_ / gcell) * ggw + x_ / gcell;
            unsigned long long *same = s_same + (conf - s_conf);
#endif
            const int w0 = NW > 1 ? wave - 1 : 0, nw = NW > 1 ? NW - 1 : 1;
            for (int j = __builtin_amdgcn_readfirstlane(w0); j < 64; j += nw) {
                const int jx = __builtin_amdgcn_readlane(x_, j), jy = __builtin_amdgcn_readlane(y_, j);
                const int dx = x_ - jx, dy = y_ - jy;
                const unsigned long long bj = __ballot((float)(dx * dx + dy * dy) < md2);
                if (lane == 0) conf[j] = bj;
#if SEL_GRID
                const unsigned long long sj = __ballot(c_ == __builtin_amdgcn_readlane(c_, j));
                if (lane == 0) same[j] = sj;
#endif
            }
        };
#if SEL_GRID
        if (n > 0 && (NW == 1 || wave > 0)) conflict_rows(0, s_conf);            // the same-cell rows are needed without a minDistance too
        if (tid == 0) s_stop[0] = 0;                            // a chunk is only begun while the pass goes on
#else
        if (use_dist && n > 0 && (NW == 1 || wave > 0)) conflict_rows(0, s_conf);
#endif
        __syncthreads();
        const float inv_cs = 1.f / (float)cs;                   // floor((c + 0.5) / cs) exactly: |error| <= 2.4e-7 * 16384 / cs < 0.5 / cs
        int round = 0;
        for (int base = 0; base < n; base += 64, ++round) {
#if SEL_GRID
            // Uniform exit: wave 0 wrote this round's flag before the barrier that ended the previous round and writes the OTHER slot in
            // this round, so every wave reads the same value whenever it gets here (s_nacc and s_nfull are rewritten by wave 0 in the
            // round itself and are read here by wave 0 alone).
            if (s_stop[round & 1]) break;
            const int nacc = s_nacc;
#else
            const int nacc = s_nacc;
            if (nacc >= max_corners) break;
#endif
            if (wave > 0 || NW == 1) {
#if SEL_GRID
                if (base + 64 < n) conflict_rows(base + 64, s_conf + 64 * ((round + 1) & 1));
#else
                if (use_dist && base + 64 < n) conflict_rows(base + 64, s_conf + 64 * ((round + 1) & 1));
#endif
            }
            if (wave == 0) {
                const int ci = base + lane;
                const bool live = ci < n;
                const unsigned xy = live ? s_idx[ci] : 0u;
                const int cx = (int)(xy & 0xffffu), cy = (int)(xy >> 16);
                // the accepted set through the grid: corners closer than minDistance sit in the 3 x 3 cells around the candidate's
                const int gx = (int)(((float)cx + 0.5f) * inv_cs), gy = (int)(((float)cy + 0.5f) * inv_cs);
                bool rej = false;
                if (use_dist && live) {
                    unsigned head[9];                           // the nine cell heads first (independent LDS reads), then the short chains
#pragma unroll
                    for (int q = 0; q < 9; ++q) {
                        const int yy = gy + q / 3 - 1, xx = gx + q % 3 - 1;
                        const bool in = yy >= 0 && yy < gh && xx >= 0 && xx < gw;
                        head[q] = in ? (unsigned)s_grid[in ? yy * gw + xx : 0] : 0xffffu;
                    }
#pragma unroll
                    for (int q = 0; q < 9; ++q) {
                        unsigned j = head[q];
                        while (j != 0xffffu) {
                            const int aj = s_acc[j];
                            const int dx = cx - (aj & 0xffff), dy = cy - (aj >> 16);
                            rej = rej || (float)(dx * dx + dy * dy) < md2;
                            j = s_next[j];
                        }
                    }
                }
                const unsigned long long alive = __ballot(live && !rej);   // survivors of the accepted-set test, best first
                const unsigned long long myconf = use_dist ? s_conf[64 * (round & 1) + lane] : 0ull;   // lanes clashing with candidate `lane`
                // Greedy acceptance in rank order, a few parallel sweeps instead of one scalar step per candidate: U = candidates not
                // decided yet, with everything that clashes with an accepted one already removed.  A lane whose earlier clashing
                // lanes are all decided is accepted in this sweep (the lowest undecided lane always is); the accepted lanes and
                // whatever clashes with them (the matrix is symmetric and has its diagonal set) leave U.  Decisions only depend on
                // earlier lanes, so the result is that of the sequential pass, and its first `room` members are what the sequential
                // pass would have accepted before running out of room.
                const unsigned long long lower = (1ull << lane) - 1ull;
#if SEL_GRID
                // The cap: a lane is ready once its earlier clashing lanes AND its earlier lanes of the same cell are decided; a ready
                // lane is accepted iff its cell still has room after the accepted earlier lanes of that cell, else it leaves U without
                // joining A.  The lowest lane of U has no earlier lane in U, so it is ready and leaves U: at most 64 trips.
                const int mycell = (cy / gcell) * ggw + cx / gcell;
                const int occ0 = (int)((reinterpret_cast<volatile unsigned *>(s_occ)[mycell >> 1] >> ((mycell & 1) * 16)) & 0xffffu);
                const unsigned long long mysame = s_same[64 * (round & 1) + lane];
                unsigned long long U = alive & ~__ballot(occ0 >= gcap), A = 0;
                while (U) {
                    const bool ready = ((U >> lane) & 1ull) && ((myconf | mysame) & U & lower) == 0ull;
                    const bool join = ready && occ0 + __popcll(A & mysame & lower) < gcap;
                    const unsigned long long J = __ballot(join);
                    A |= J;
                    U &= ~(__ballot((myconf & J) != 0ull) | J | __ballot(ready && !join));
                }
#else
                unsigned long long U = alive, A = 0;
                while (U) {
                    const bool join = ((U >> lane) & 1ull) && (myconf & U & lower) == 0ull;
                    const unsigned long long J = __ballot(join);
                    A |= J;
                    U &= ~(__ballot((myconf & J) != 0ull) | J);
                }
#endif
                const int room = max_corners - nacc;
                const unsigned long long acc = __ballot(((A >> lane) & 1ull) && __popcll(A & lower) < room);
                const bool mine = (acc >> lane) & 1ull;
                const int pos = nacc + __popcll(acc & lower);   // accepted candidates store in parallel, in rank order
                if (mine) {
                    s_acc[pos] = cx | (cy << 16);
                    pts[((size_t)b * pts_stride + pos) * 2] = (float)cx;
                    pts[((size_t)b * pts_stride + pos) * 2 + 1] = (float)cy;
                }
                if (use_dist) {
                    // link the new corners into their cells: all lanes store their index as the cell's head, the lane that reads its
                    // own index back won and chains to the old head; the others of that cell go again (order inside a cell is free)
                    bool pend = mine;
                    const int cell = gy * gw + gx;
                    while (__ballot(pend)) {
                        unsigned old = 0xffffu;
                        if (pend) old = s_grid[cell];
                        __builtin_amdgcn_wave_barrier();
                        if (pend) s_grid[cell] = (unsigned short)pos;
                        __builtin_amdgcn_wave_barrier();
                        if (pend && s_grid[cell] == (unsigned short)pos) { s_next[pos] = (unsigned short)old; pend = false; }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
                if (lane == 0) s_nacc = nacc + __popcll(acc);
#if SEL_GRID
                if (mine) atomicAdd(&s_occ[mycell >> 1], 1u << ((mycell & 1) * 16));
                const unsigned long long filled = __ballot(mine && occ0 + __popcll(acc & mysame & lower) + 1 == gcap);
                if (lane == 0) {
                    const int nf = s_nfull + __popcll(filled);
                    s_nfull = nf;
                    // the pass stops behind the acceptance that fills the budget or the last open cell; otherwise the round is decided
                    const bool stop = nacc + __popcll(acc) >= max_corners || nf >= ncells;
                    s_stop[(round + 1) & 1] = stop;
                    // (a stop follows an acceptance.  __builtin_clzll behind the zero test, not __clzll: one more call site of that shared
                    //  device function widens the value range the compiler infers for it and changes the code of the PLAIN kernels.)
                    s_exam = rank_base + (stop && acc ? base + 64 - __builtin_clzll(acc) : min(base + 64, n));
                }
#endif
            }
            __syncthreads();
        }
        if (s_nacc >= max_corners) break;
#if SEL_GRID
        if (s_nfull >= ncells) break;
        rank_base += chunk_n;
        if (max_rank > 0 && rank_base >= max_rank) break;
#endif
        a = T;
        __syncthreads();
    }
    if (tid == 0) counts[b] = s_nacc;
#if SEL_GRID
    if (tid == 0) { gstats[2 * b] = s_nacc; gstats[2 * b + 1] = s_exam; }
#endif
