// k_keyframe_body.inc — rules 1-5 of ofk_set_keyframe, the body of k_keyframe_step (KF_ROT 0) and of k_keyframe_step_rot (KF_ROT 1,
// k_keyframe_rot.inc: rule 2 widened by ofk_set_keyframe_rotation).  With KF_ROT 0 the text is k_keyframe_step's as it always was.
// KF_MAP 1 (k_keyframe_map.inc, with KF_ROT 0): rules M1-M5 of ofk_set_keyframe_map around them, the body of k_keyframe_step_map;
// with KF_MAP 0 nothing of it is compiled.
    __shared__ row_walk s_rows;
    __shared__ double s_red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
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
    kf_rotate(o0, o1, o2, R0, f.R);
#if KF_ROT
    // 1'. the source's rotation and the prior of this step (ofk_set_keyframe_rotation)
    __shared__ double s_jp[4][KR_SUMS];
    __shared__ double s_cov[2][15];
    double *rst = rst_all + (size_t)b * OFK_KEYROT_STATE;
    const bool att = rc.source == OFK_KEYROT_ATTITUDE && mk != 0 && rst[9] == 1.0 && rst[10] == (double)key_step;
    if (att)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) f.R[3 * i + j] = (rw[i] * rst[j] + rw[3 + i] * rst[3 + j]) + rw[6 + i] * rst[6 + j];
    double Racc[9];
    for (int k = 0; k < 9; ++k) Racc[k] = f.R[k];
    kr_prior pr;
    const double age = (double)((step + 1) - key_step);
    {
        const double sfp = cfg.sf * f.sc, var = att ? rc.var_att : age * rc.sg2 + (age * rc.sb) * (age * rc.sb);
        const int ax[3] = {rc.ax0, rc.ax1, rc.ax2};
        for (int k = 0; k < 3; ++k) {
            pr.held[k] = ax[k] == 0 || !(var > 0.0);
            pr.lam[k] = pr.held[k] ? 0.0 : (sfp * sfp) / var;
            pr.sig[k] = pr.held[k] ? 0.0 : sqrt(var);
        }
    }
    double J1[KR_SUMS];
    for (int k = 0; k < KR_SUMS; ++k) J1[k] = 0.0;
#endif
    const double cs = (((f.R[0] + f.R[4]) + f.R[8]) - 1.0) / 2.0;
#if KF_ROT
    double angle = acos(fmin(1.0, fmax(-1.0, cs)));                  // of R_acc; of R^ behind a joint solve that stands
#else
    const double angle = acos(fmin(1.0, fmax(-1.0, cs)));
#endif

#if KF_MAP
    // M1. capture; M2's live map rows and M4's mature rows in the same walk
    int *ms = km.mstate + (size_t)b * 2;
    const int cap_for = ms[0];
    const bool capture = mk != 0 && cap_for != key_step;
    double mcnt[3] = {0.0, 0.0, 0.0};                            // captured, live map rows, mature among the live rows
    for (int i = tid; i < n; i += 256) {
        const size_t r = base + i;
        bool mature = false;
        if (km.rho) { const double rho = km.rho[r], lim = mc.rel_max * rho; mature = km.nobs[r] >= mc.min_obs && rho > 0.0 && km.var[r] <= lim * lim; }
        const bool mem = t.member[r] != 0;
        if (capture && mem) {
            km.key_rho[r] = mature ? km.rho[r] : 0.0; km.key_var[r] = mature ? km.var[r] : 0.0;
            if (mature) mcnt[0] += 1.0;
        }
        if (in.status[r] != 0 && mem) {
            if (km.key_rho[r] > 0.0) mcnt[1] += 1.0;
            if (mature) mcnt[2] += 1.0;
        }
    }
    __shared__ double s_mc[4][3];
    block_sums<3, 3>(mcnt, s_mc);
    const int map_rows = capture ? (int)mcnt[0] : ms[1], live_map = (int)mcnt[1], ready = (int)mcnt[2];
    const bool use_map = map_rows >= mc.min_rows && live_map >= mc.min_rows;   // uniform over the workgroup
#endif

    // 2. the key solve
    Acc a1; acc_zero(a1);
    double live_d = 0.0;
    for (int i = tid; i < n; i += 256) {
        const size_t r = base + i;
        if (in.status[r] != 0 && t.member[r] != 0) {
            live_d += 1.0;
            double a, bb, u0, u1, sA;
#if KF_ROT
            if (mk != 0 && kf_row(t, in.next_pts, r, f, a, bb, u0, u1, sA)) { acc_point(a1, a, bb, u0, u1, 0.0, sA, 1.0); kr_point(J1, a, bb, u0, u1, sA); }
#else
            if (mk != 0 && kf_row(t, in.next_pts, r, f, a, bb, u0, u1, sA)) acc_point(a1, a, bb, u0, u1, 0.0, sA, 1.0);
#endif
        }
    }
    const int live = (int)block_sum(live_d, s_red);
    acc_block_sum(a1);
#if KF_ROT
    block_sums<KR_SUMS, KR_SUMS>(J1, s_jp);
#endif
    double T[3] = {0.0, 0.0, 0.0}, s3[3];
    bool fin = true;
    int flag = mk == 0 ? OFK_KEY_NONE : OFK_KEY_UNSOLVED;
    if (mk != 0 && a1.cnt >= (double)cfg.min_rows && solve_from_acc(a1, T, s3, fin) == 3 && fin) flag = OFK_KEY_SOLVED;
    Acc as = a1;                                                 // the sums of the solve that stands
    const double T1[3] = {T[0], T[1], T[2]};                     // the gate is the first solve's, whichever stands
    double rows2 = 0.0;
    bool gated = false;
    const double sf = cfg.sf * f.sc, gs = cfg.gate * f.sc, g2 = gs * gs;
#if KF_ROT
    // 2'. the joint solve; where it does not stand, the plain rule 2 goes on below as it always did
    kr_res jo;
    jo.flag = OFK_KEYROT_NONE; jo.gated = 0; jo.rms = jo.rows2 = jo.rows = 0.0;
    for (int k = 0; k < 3; ++k) { jo.T[k] = 0.0; jo.dl[k] = 0.0; }
    bool jok = false;
    if (flag == OFK_KEY_SOLVED) {
        if (pr.held[0] && pr.held[1] && pr.held[2]) jo.flag = OFK_KEYROT_HELD;
        else jok = kr_joint(t, in, base, n, f, a1, J1, pr, cfg, rc, g2, sf * sf, s_jp, s_red, s_cov, jo);
    }
    if (jok) {                                                   // rule 3's displacement under R^ and the joint T: one that is no number withdraws
        const double *off = sn + 16;                             // the joint solve here, in front of the plain rule 2, which then runs untouched
        double w[3], Dj[3];
        for (int i = 0; i < 3; ++i) w[i] = jo.T[i] + (off[i] - ((f.R[3 * i] * off[0] + f.R[3 * i + 1] * off[1]) + f.R[3 * i + 2] * off[2]));
        for (int i = 0; i < 3; ++i) Dj[i] = (rw[3 * i] * w[0] + rw[3 * i + 1] * w[1]) + rw[3 * i + 2] * w[2];
        if (!(isfinite(Dj[0]) && isfinite(Dj[1]) && isfinite(Dj[2]))) {
            jok = false; jo.flag = OFK_KEYROT_NONE;
            for (int k = 0; k < 9; ++k) f.R[k] = Racc[k];
        }
    }
    if (jok) {
        T[0] = jo.T[0]; T[1] = jo.T[1]; T[2] = jo.T[2]; rows2 = jo.rows2; gated = jo.gated != 0;
        angle = acos(fmin(1.0, fmax(-1.0, (((f.R[0] + f.R[4]) + f.R[8]) - 1.0) / 2.0)));
    }
    if (!jok)
#endif
#if KF_MAP
    // M3. the map solve in rule 2's place; where it does not stand the plain rule 2 goes on below as it always did
    km_res mo;
    const bool plain_ok = flag == OFK_KEY_SOLVED;
    const bool mok = use_map && km_solve(t, in, km, base, n, f, cfg, mc, sf * sf, g2, s_red, mo);
    if (mok) {
        flag = OFK_KEY_SOLVED; T[0] = mo.T[0]; T[1] = mo.T[1]; T[2] = mo.T[2]; rows2 = mo.rows2; gated = mo.gated; as = mo.as; a1.cnt = mo.rows1;
    }
    if (!mok)
#endif
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
#if KF_ROT
    if (jok) rms = jo.rms;
    else
#endif
#if KF_MAP
    if (mok) rms = mo.rms;
    else
#endif
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
#if KF_MAP
    // M4. a keyframe without a map, and depths that would give it one
    if (mc.ready_share > 0.0 && map_rows < mc.min_rows && ready >= mc.min_rows && (double)ready >= mc.ready_share * (double)live) bits |= 32;
#endif
    const bool rekey = bits != 0;
    const int reason = bits ? __ffs(bits) : 0;

    // 5. compaction: the table's walk (k_rows.inc)
    rows_begin(s_rows);                                         // its barrier also: every thread has read the state
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool inside = i < n;
        const size_t r = base + (inside ? i : 0);
        const bool keep = inside && in.status[r] != 0;
        float kx = t.key_xy[2 * r], ky = t.key_xy[2 * r + 1];
        uint8_t m = t.member[r];
        if (rekey) { kx = in.next_pts[2 * r]; ky = in.next_pts[2 * r + 1]; m = 1; }
#if KF_MAP
        double krho = km.key_rho[r], kvar = km.key_var[r];          // M5: they move with key_xy; a re-key empties them until M1 fills them
        if (rekey) { krho = 0.0; kvar = 0.0; }
#endif
        const int p = rows_place(s_rows, keep);
        if (keep) { const size_t w = base + p; t.key_xy[2 * w] = kx; t.key_xy[2 * w + 1] = ky; t.member[w] = m; }
#if KF_MAP
        if (keep) { const size_t w = base + p; km.key_rho[w] = krho; km.key_var[w] = kvar; }
#endif
        rows_next(s_rows);
    }
    const int kept = s_rows.base;
    const int extra = rows_extra(in.new_counts, b, in.max_total, in.stride, kept);
    for (int i = tid; i < extra; i += 256) kf_fresh_row(t, base + kept + i);
#if KF_MAP
    for (int i = tid; i < extra; i += 256) km_fresh_row(km, base + kept + i);
#endif
    if (tid == 0) {
        double *o = t.rec + (size_t)b * OFK_KEY_DOUBLES;
        for (int k = 0; k < OFK_KEY_DOUBLES; ++k) o[k] = 0.0;
#if KF_ROT
        if (jok) for (int k = 0; k < 6; ++k) o[20 + k] = s_cov[gated ? 1 : 0][6 + k];
        else
#endif
        if (flag == OFK_KEY_SOLVED) {
            double A[3][3], lam[3], V[3][3], Mi[3][3]; sym3_from6(as, A);
            jacobi3(A, lam, V);
            eig_inverse3(lam, V, Mi);
            const double sf2 = sf * sf;
            int s = 20;
            for (int i = 0; i < 3; ++i)
                for (int j = i; j < 3; ++j) o[s++] = sf2 * Mi[i][j];
        }
        const int mk_out = rekey ? kept : mk, ks_out = rekey ? step + 1 : key_step, nkey_out = nkey + (rekey ? 1 : 0);
        const int ndead_out = ndead + (flag != OFK_KEY_SOLVED ? 1 : 0);
        if (rekey) for (int k = 0; k < 3; ++k) anchor[k] = pos[k];
#if KF_ROT
        for (int k = 0; k < 9; ++k) st[k] = rekey ? ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0) : Racc[k];   // the source's, not R^
#else
        for (int k = 0; k < 9; ++k) st[k] = rekey ? ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0) : f.R[k];
#endif
        for (int k = 0; k < 3; ++k) { st[9 + k] = anchor[k]; st[12 + k] = pos[k]; }
        is[0] = ks_out; is[1] = mk_out; is[2] = nkey_out; is[3] = ndead_out;
        o[0] = T[0]; o[1] = T[1]; o[2] = T[2]; o[3] = (double)flag; o[4] = a1.cnt; o[5] = rows2; o[6] = rms;
        o[7] = (double)mk_out; o[8] = (double)ks_out; o[9] = (double)reason;
        for (int k = 0; k < 3; ++k) { o[10 + k] = D[k]; o[13 + k] = pos[k]; o[16 + k] = anchor[k]; }
        o[19] = angle; o[26] = (double)nkey_out; o[27] = (double)ndead_out; o[28] = (double)live; o[29] = gated ? 1.0 : 0.0;
        o[30] = (double)bits;
#if KF_MAP
        const int cap_out = capture ? key_step : cap_for;
        ms[0] = cap_out; ms[1] = rekey ? 0 : map_rows;
        double *q = km.mrec + (size_t)b * OFK_KEYMAP_DOUBLES;
        for (int k = 0; k < OFK_KEYMAP_DOUBLES; ++k) q[k] = 0.0;
        q[0] = (double)(mok ? OFK_KEYMAP_USED : use_map ? OFK_KEYMAP_FELL_BACK : map_rows < mc.min_rows ? OFK_KEYMAP_NONE : OFK_KEYMAP_FEW);
        q[1] = (double)map_rows; q[2] = (double)live_map;
        if (use_map) { q[3] = mo.rows1; q[4] = mo.rows2; q[5] = mo.sumw; q[6] = mo.spread; }
        if (use_map && plain_ok) for (int k = 0; k < 3; ++k) q[7 + k] = T1[k];
        q[10] = capture ? mcnt[0] : 0.0; q[11] = (double)cap_out;
#endif
#if KF_ROT
        if (rekey) { for (int k = 0; k < 9; ++k) rst[k] = rw[k]; rst[9] = 1.0; rst[10] = (double)ks_out; }
        double *q = rrec_all + (size_t)b * OFK_KEYROT_DOUBLES;
        for (int k = 0; k < OFK_KEYROT_DOUBLES; ++k) q[k] = 0.0;
        if (jo.flag == OFK_KEYROT_OK || jo.flag == OFK_KEYROT_LARGE) for (int k = 0; k < 3; ++k) q[k] = jo.dl[k];
        q[3] = (double)jo.flag;
        for (int k = 0; k < 9; ++k) q[4 + k] = f.R[k];
        if (jok) {
            for (int k = 0; k < 6; ++k) q[13 + k] = s_cov[gated ? 1 : 0][k];
            for (int k = 0; k < 3; ++k) q[25 + k] = s_cov[gated ? 1 : 0][12 + k];
            q[31] = (double)rc.iters; q[37] = jo.rows;
        }
        for (int k = 0; k < 6; ++k) q[19 + k] = o[20 + k];
        for (int k = 0; k < 3; ++k) { q[28 + k] = pr.sig[k]; q[32 + k] = jo.flag != OFK_KEYROT_NONE ? T1[k] : 0.0; }
        q[35] = att ? 1.0 : 0.0; q[36] = age;
#endif
    }
