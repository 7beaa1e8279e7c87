// ofk_api.hip — the C ABI of libofk.so (include/ofk.h): context lifecycle, host<->HBM plumbing, stage entry
// points and the resident frame-pair pipeline.  No CPU fallback anywhere: every entry point launches HIP
// kernels on the context's stream or returns an error.
#include "ofk_internal.h"
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static char g_create_err[512] = "";

int ofk_fail(ofk_ctx *ctx, int code, const char *fmt, ...)
{
    char *dst = ctx ? ctx->errmsg : g_create_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
    return code;
}

#define TRY(expr) do { int rc_ = (expr); if (rc_ != OFK_OK) return rc_; } while (0)
static size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

ofk_levels ofk_make_levels(int h, int w, int win, int max_level)
{
    ofk_levels lv;
    memset(&lv, 0, sizeof lv);
    lv.h[0] = h; lv.w[0] = w; lv.off[0] = 0;
    size_t off = up((size_t)h * w, 256);
    int l = 0;
    while (l < max_level && l < OFK_MAX_LEVELS - 1) {
        const int nh = (lv.h[l] + 1) / 2, nw = (lv.w[l] + 1) / 2;
        if (win > 0 && (nw <= win || nh <= win)) break;
        ++l;
        lv.h[l] = nh; lv.w[l] = nw; lv.off[l] = off;
        off += up((size_t)nh * nw, 256);
    }
    lv.n = l;
    return lv;
}

static size_t levels_bytes(int h, int w, int max_level)
{
    const ofk_levels lv = ofk_make_levels(h, w, 0, max_level);
    return lv.off[lv.n] + up((size_t)lv.h[lv.n] * lv.w[lv.n], 256);
}

// Hardware queues: the free-running slices keep four HIP streams busy (six to eight with RCCL's) and the runtime multiplexes
// streams onto GPU_MAX_HW_QUEUES hardware queues, 4 by default; two streams of one queue run in order (-10 % measured).  The
// variable is read when the HIP runtime initialises, so it is the HOST's to set before its first HIP call (the Python binding and
// bench.py do; INTEGRATION.md tells C callers): a library that edits its host's environment from a load-time constructor races with
// getenv on other threads and changes every other HIP user of the process (rounds 1-2 did that).  ofk_set_streams warns when the
// value in effect is too small.

ofk_tuning g_ofk_tuning = {0, 0, 0, 0, 0, 0, 0};

static int *tuning_slot(const char *knob, int *lo, int *hi)
{
    struct { const char *name; int *slot; int lo, hi; } tab[] = {
        {"eig_rows", &g_ofk_tuning.eig_rows, 8, 4096},        // rows per strip of the streaming response kernels
        {"no_pair", &g_ofk_tuning.no_pair, 0, 1},             // 1: one column per lane everywhere (k_mineig_stream instead of k_mineig_pair)
        {"no_pyr3", &g_ofk_tuning.no_pyr3, 0, 1},             // 1: pyramid level by level instead of the three-level pass
        {"pyr3_chunks", &g_ofk_tuning.pyr3_chunks, 1, 4096},  // row chunks per strip of k_pyr3_stream
        {"pyr_rows", &g_ofk_tuning.pyr_rows, 1, 4096},        // rows per strip of k_pyr_down_stream
        {"jpeg_chunk", &g_ofk_tuning.jpeg_chunk, 64, 1024},   // bytes of entropy data per decoder thread (a power of two)
        {"jpeg_sub", &g_ofk_tuning.jpeg_sub, 1, 13},          // second-level Huffman look-up tables per image + 1 (1: none - every long code takes the canonical search)
        {"gray_px", &g_ofk_tuning.gray_px, 16, 64},           // experiment: one-wave workgroups of 16 / 32 / 64 pixels per thread in the BGR -> gray conversion
    };
    for (auto &t : tab)
        if (knob && strcmp(knob, t.name) == 0) { *lo = t.lo; *hi = t.hi; return t.slot; }
    return nullptr;
}

extern "C" int ofk_set_tuning(const char *knob, int value)
{
    int lo, hi;
    int *slot = tuning_slot(knob, &lo, &hi);
    if (!slot) return ofk_fail(nullptr, OFK_E_INVALID, "ofk_set_tuning: unknown knob '%s'", knob ? knob : "(null)");
    const bool jpeg_ok = slot != &g_ofk_tuning.jpeg_chunk || (value & (value - 1)) == 0;
    if (value != 0 && (value < lo || value > hi || !jpeg_ok)) return ofk_fail(nullptr, OFK_E_INVALID, "ofk_set_tuning: %s takes 0 (default) or %d..%d", knob, lo, hi);
    *slot = value;
    return OFK_OK;
}

extern "C" int ofk_get_tuning(const char *knob, int *value)
{
    int lo, hi;
    int *slot = tuning_slot(knob, &lo, &hi);
    if (!slot || !value) return ofk_fail(nullptr, OFK_E_INVALID, "ofk_get_tuning: unknown knob '%s'", knob ? knob : "(null)");
    *value = *slot;
    return OFK_OK;
}

extern "C" int ofk_version(void) { return OFK_VERSION; }

extern "C" const char *ofk_last_error(const ofk_ctx *ctx) { return ctx ? ctx->errmsg : g_create_err; }

extern "C" int ofk_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int ofk_device_sync(void) { return hipDeviceSynchronize() == hipSuccess ? OFK_OK : OFK_E_HIP; }

#define ALLOC(ptr, bytes)                                                                                     \
    do {                                                                                                      \
        hipError_t e_ = hipMalloc((void **)&(ptr), (bytes));                                                  \
        if (e_ != hipSuccess) {                                                                               \
            ofk_fail(nullptr, OFK_E_HIP, "hipMalloc(%zu bytes) for %s: %s", (size_t)(bytes), #ptr, hipGetErrorString(e_)); \
            ofk_destroy(c);                                                                                   \
            return OFK_E_HIP;                                                                                 \
        }                                                                                                     \
    } while (0)

extern "C" int ofk_create(int device, int max_w, int max_h, int max_batch, int max_pts, int max_level, ofk_ctx **out)
{
    if (!out) return ofk_fail(nullptr, OFK_E_INVALID, "out is NULL");
    *out = nullptr;
    if (max_w < 16 || max_h < 16 || max_w > 16384 || max_h > 16384 || max_batch < 1 || max_pts < 1 || max_pts > 4096 ||
        max_level < 0 || max_level > 8)
        return ofk_fail(nullptr, OFK_E_INVALID, "ofk_create: bad limits (w %d h %d batch %d pts %d level %d)", max_w, max_h,
                        max_batch, max_pts, max_level);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ofk_fail(nullptr, OFK_E_NOGPU, "no HIP device visible");
    if (device < 0 || device >= ndev) return ofk_fail(nullptr, OFK_E_INVALID, "device %d out of range (%d visible)", device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ofk_fail(nullptr, OFK_E_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ofk_fail(nullptr, OFK_E_NOGPU, "device %d is %s; libofk.so is built for gfx950 only", device, prop.gcnArchName);
    if (hipSetDevice(device) != hipSuccess) return ofk_fail(nullptr, OFK_E_HIP, "hipSetDevice(%d) failed", device);

    ofk_ctx *c = (ofk_ctx *)calloc(1, sizeof(ofk_ctx));
    if (!c) return ofk_fail(nullptr, OFK_E_INVALID, "out of host memory");
    c->device = device; c->max_w = max_w; c->max_h = max_h; c->max_batch = max_batch; c->max_pts = max_pts; c->max_level = max_level;
    c->P = (size_t)max_w * max_h;
    c->bgr_stride = up(c->P * 3, 256);
    c->pyr_stride = levels_bytes(max_h, max_w, max_level);
    c->img_stride = up(c->P, 64);
    c->cand_cap = (int)(c->P / 4 < 4096 ? 4096 : c->P / 4);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { free(c); return ofk_fail(nullptr, OFK_E_HIP, "hipStreamCreate failed"); }
    c->nstreams = 1;
    c->streams[0] = c->stream;
    c->overlap = 1;
    c->gray_direct_set = -1;
    c->lk_seed_mode = OFK_SEED_OFF; c->lk_seed_gain = 1.0;
    c->light = ofk_lk_light{OFK_LIGHT_OFF, 4.0};
    c->robust = ofk_robust{OFK_ROBUST_OFF, 4.685, 5, 64, 0ull, 0};
    c->gate = ofk_track_gate{OFK_FB_OFF, 0.5, -1, 0.0};
    c->cov = ofk_cov{OFK_COV_OFF, 0.0, 0.0, 0.0, {0.0, 0.0, 0.0}, 0.0, 0.0, 0, 0, 0.0, 0.0};
    c->joint = ofk_joint{OFK_JOINT_OFF, 0.2, {INFINITY, INFINITY, INFINITY}, 0};
    c->bias = ofk_gyro_bias{OFK_BIAS_OFF, 0.2, 0.0, 0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, 1};
    c->plane = ofk_plane{OFK_PLANE_OFF, 0.2, INFINITY, 0.1, {0.0, 0.0, 1.0}, 6};
    c->epi = ofk_epipolar{OFK_EPI_OFF, INFINITY, 5, 0.008, {0.0, 0.0, 1.0}, OFK_EPI_W_ONE};
    c->zones = ofk_zones{OFK_ZONES_OFF, 48, 3, 20, 30, OFK_ZONE_MAX};
    c->camera = ofk_camera{OFK_CAMERA_OFF, 20, 1.0, 1.0, 0.0, 0.0, {0, 0, 0, 0, 0, 0, 0, 0}, 1.0, 1.0, 0.0, 0.0};
    c->rs = ofk_rshutter{OFK_RS_OFF, 0, 0.0, 0.5, 1.0};
    c->fm = ofk_finite_motion{OFK_FM_OFF, 0.1};
    c->tt = ofk_track_table{OFK_TT_OFF, OFK_TT_SEED_OFF, 1.0};
    c->td = ofk_track_depth{OFK_TD_OFF, 0.2, 0.5, 3.0, 0.0, 3, 0.25, 8, 1};
    c->tpl = ofk_track_template{OFK_TPL_OFF, 15, 0.8, 3, 2.0, OFK_TPL_KEEP, 6, 2.0, 1.5};
    c->key = ofk_keyframe{OFK_KEY_OFF, 0.2, 2.0, 8, 0.5, 0.5, 0};
    c->krot = ofk_keyframe_rotation{OFK_KEYROT_OFF, OFK_KEYROT_GYRO, {1, 1, 1}, 0.0, 1e-4, 1e-3, 2, 0.1};
    c->kmap = ofk_keyframe_map{OFK_KEYMAP_OFF, 3, 0.02, 8, 0.5, 1};
    c->posf = ofk_pos_filter{OFK_POSF_OFF, 1.0, 1e-3, 0.0, 1.0, 0.5, 0.0, 1e-3, 0.0, 0.0, 1.0, 0.0, 0.0};
    c->stab = ofk_stabilise{OFK_STAB_OFF, OFK_BORDER_CONSTANT, 0, 0.5, 1};
    c->rect = ofk_rectify{OFK_RECTIFY_OFF, 0.0};
    // Slice and auxiliary streams are created when a call first needs them (need_streams): the runtime multiplexes HIP streams
    // onto a few hardware queues (4 by default), and two streams of one queue run in order - an idle stream would cost a real one
    // its concurrency.
    bool ok = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_x, hipEventDisableTiming) == hipSuccess;
    for (int k = 0; k < OFK_MAX_STREAMS && ok; ++k)
        ok = hipEventCreateWithFlags(&c->ev_g0[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->ev_aux[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->ev_lkdone[0][k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->ev_lkdone[1][k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->ev_end[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->ev_stagger[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        ofk_fail(nullptr, OFK_E_HIP, "hipEventCreate failed");
        ofk_destroy(c);
        return OFK_E_HIP;
    }
    const size_t B = (size_t)max_batch;
    for (int k = 0; k < 2; ++k) { ALLOC(c->bgr[k], B * c->bgr_stride); ALLOC(c->pyr[k], B * c->pyr_stride); }
    ALLOC(c->eig, B * c->img_stride * sizeof(float));
    ALLOC(c->cand, B * (size_t)c->cand_cap * 8);
    c->seg_keys = (size_t)(c->P / 4) + (size_t)(c->P / 4) / 2 + 64 * OFK_SEG_MAX;   // segment rounding slack
    ALLOC(c->cand_seg, B * c->seg_keys * 8);
    ALLOC(c->seg_count, B * OFK_SEG_MAX * 4);
    ALLOC(c->cand_count, B * OFK_CNT_STRIDE * 4); ALLOC(c->maxbits, B * OFK_MAX_STRIDE * 4);
    ALLOC(c->sel_hist, B * 1024 * 4);
    ALLOC(c->sel_keys, B * OFK_CHUNK * 8);
    ALLOC(c->pts_prev, B * max_pts * 8); ALLOC(c->pts_next, B * max_pts * 8);
    ALLOC(c->status, B * max_pts); ALLOC(c->err, B * max_pts * 4); ALLOC(c->counts, B * 4);
    ALLOC(c->sensors, B * OFK_SENSOR_DOUBLES * 8); ALLOC(c->records, B * OFK_RECORD_DOUBLES * 8);
    ALLOC(c->dev_flags, 16);
    hipMemsetAsync(c->dev_flags, 0, 16, c->stream);
    hipMemsetAsync(c->counts, 0, B * 4, c->stream);
    hipMemsetAsync(c->sensors, 0, B * OFK_SENSOR_DOUBLES * 8, c->stream);
    c->ev_cap = 32768;                                           // stage timers between two ofk_profile_read calls (28 per step with two slices);
                                                                 // the events themselves are created on first use
    c->ev = (hipEvent_t *)calloc(c->ev_cap, sizeof(hipEvent_t));
    c->ev_stage = (int *)calloc(c->ev_cap / 2, sizeof(int));
    hipStreamSynchronize(c->stream);
    *out = c;
    return OFK_OK;
}

static void track_free(ofk_ctx *c);                             // the per-track states' allocations (TRACK[], below)

extern "C" int ofk_destroy(ofk_ctx *c)
{
    if (!c) return OFK_OK;
    hipSetDevice(c->device);
    if (c->stream) hipDeviceSynchronize();
    ofk_comm_destroy(c);
    for (int k = 0; k < 2; ++k) { if (c->bgr[k]) hipFree(c->bgr[k]); if (c->pyr[k]) hipFree(c->pyr[k]); }
    void *ptrs[] = {c->eig, c->mask, c->deriv, c->cand, c->cand_seg, c->seg_count, c->cand_count, c->sel_hist, c->sel_keys, c->maxbits, c->pts_prev, c->pts_next, c->status, c->err,
                    c->counts, c->sensors, c->records, c->dev_flags, c->scratch, c->pts_new, c->new_counts, c->limit,
                    c->imu_state, c->imu_dv, c->kf_mats, c->kf_x, c->kf_P, c->fused, c->imu_msgs, c->imu_counts, c->rob_work, c->pts_back, c->grid_stats, c->cov_rec, c->joint_rec, c->bias_rec, c->plane_rec, c->epi_rec,
                    c->zone_tab, c->pts_prev_u};
    for (void *p : ptrs) if (p) hipFree(p);
    track_free(c);
    if (c->sb_frames) hipFree(c->sb_frames);
    if (c->hstage) hipHostFree(c->hstage);
    ofk_jpeg_release(c);
    if (c->ev) { for (int i = 0; i < c->ev_cap; ++i) if (c->ev[i]) hipEventDestroy(c->ev[i]); free(c->ev); }
    free(c->ev_stage);
    free(c->h_counts);
    for (int k = 1; k < OFK_MAX_STREAMS; ++k) if (c->streams[k]) hipStreamDestroy(c->streams[k]);
    for (int k = 0; k < OFK_MAX_STREAMS; ++k) {
        if (c->aux[k]) hipStreamDestroy(c->aux[k]);
        if (c->ev_g0[k]) hipEventDestroy(c->ev_g0[k]);
        if (c->ev_aux[k]) hipEventDestroy(c->ev_aux[k]);
        for (int s = 0; s < 2; ++s) if (c->ev_lkdone[s][k]) hipEventDestroy(c->ev_lkdone[s][k]);
    }
    for (int k = 0; k < 2; ++k) if (c->pyr_alt[k]) hipFree(c->pyr_alt[k]);
    for (int k = 0; k < 8; ++k) if (c->marks[k]) hipEventDestroy(c->marks[k]);
    for (int k = 0; k < OFK_MAX_STREAMS; ++k) {
        if (c->ev_end[k]) hipEventDestroy(c->ev_end[k]);
        if (c->ev_stagger[k]) hipEventDestroy(c->ev_stagger[k]);
    }
    if (c->ev_x) hipEventDestroy(c->ev_x);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->stream) hipStreamDestroy(c->stream);
    free(c);
    return OFK_OK;
}

// Slice streams free-run across consecutive ofk_pairs_run calls.  Every other entry point works on the context's stream and
// on buffers the slices use, so it first makes that stream wait for whatever the slices (and the export stream) still hold.
static int need_streams(ofk_ctx *c, int slices, bool overlap)
{
    for (int k = 1; k < slices; ++k)
        if (!c->streams[k]) OFK_HIP(c, hipStreamCreateWithFlags(&c->streams[k], hipStreamNonBlocking));
    for (int k = 0; k < slices && overlap; ++k)
        if (!c->aux[k]) OFK_HIP(c, hipStreamCreateWithFlags(&c->aux[k], hipStreamNonBlocking));
    return OFK_OK;
}

// The last slice's stream once every other slice of the latest call has finished: where record export and marks are queued while
// the slices are open.  The slices are offset in time and the last one finishes last, so the waits cost it nothing; a stream of
// their own would have to share a hardware queue with one of the slices.
static int tail_stream(ofk_ctx *c, hipStream_t *out)
{
    *out = c->stream;
    if (!c->slices_open) return OFK_OK;
    hipStream_t s = c->streams[c->open_slices - 1];
    for (int k = 0; k + 1 < c->open_slices; ++k) OFK_HIP(c, hipStreamWaitEvent(s, c->ev_end[k], 0));
    *out = s;
    return OFK_OK;
}

static int join_slices(ofk_ctx *c)
{
    if (c->slices_open) {
        for (int k = 1; k < c->open_slices; ++k) OFK_HIP(c, hipStreamWaitEvent(c->stream, c->ev_end[k], 0));
        c->slices_open = 0;
    }
    if (c->x_pending) {
        OFK_HIP(c, hipStreamWaitEvent(c->stream, c->ev_x, 0));
        c->x_pending = 0;
    }
    return OFK_OK;
}

// Preamble of the entry points.  Those that leave the slices running (ofk_pairs_run and what is queued behind it) take use_device alone.
static int use_device(ofk_ctx *c) { return hipSetDevice(c->device) == hipSuccess ? OFK_OK : ofk_fail(c, OFK_E_HIP, "hipSetDevice failed"); }
static int enter(ofk_ctx *c)
{
    TRY(use_device(c));
    return join_slices(c);
}

int ofk_join_slices(ofk_ctx *c) { return join_slices(c); }
int ofk_prepare_streams(ofk_ctx *c) { return need_streams(c, c->nstreams < 1 ? 1 : c->nstreams, c->overlap != 0); }

extern "C" int ofk_sync(ofk_ctx *c)
{
    if (!c) return OFK_E_INVALID;
    TRY(join_slices(c));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

// every stream of the context idle (slice, auxiliary and context stream)
static int drain_all(ofk_ctx *c)
{
    TRY(enter(c));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < OFK_MAX_STREAMS; ++k) {
        if (k && c->streams[k]) OFK_HIP(c, hipStreamSynchronize(c->streams[k]));
        if (c->aux[k]) OFK_HIP(c, hipStreamSynchronize(c->aux[k]));
    }
    return OFK_OK;
}

int ofk_resident_pyramid(ofk_ctx *c, int frame_set, int image, uint8_t *out, size_t bytes)
{
    if (!c || !out || frame_set < 0 || frame_set > 1 || image < 0 || image >= c->max_batch || bytes > c->pyr_stride)
        return ofk_fail(c, OFK_E_INVALID, "resident pyramid: frame set 0/1, image < max_batch, at most one slab (%zu bytes)", c ? c->pyr_stride : (size_t)0);
    TRY(drain_all(c));
    const uint8_t *base = (c->pyr_last && c->pyr_alt[frame_set]) ? c->pyr_alt[frame_set] : c->pyr[frame_set];
    OFK_HIP(c, hipMemcpy(out, base + (size_t)image * c->pyr_stride, bytes, hipMemcpyDeviceToHost));
    return OFK_OK;
}

int ofk_need_scratch(ofk_ctx *c, size_t bytes)
{
    if (bytes <= c->scratch_bytes) return OFK_OK;
    if (c->scratch) { hipStreamSynchronize(c->stream); hipFree(c->scratch); c->scratch = nullptr; c->scratch_bytes = 0; }
    bytes = up(bytes, 1 << 20);
    OFK_HIP(c, hipMalloc(&c->scratch, bytes));
    c->scratch_bytes = bytes;
    return OFK_OK;
}

static int check_geom(ofk_ctx *c, int batch, int h, int w, const char *who)
{
    if (!c) return OFK_E_INVALID;
    if (batch < 1 || batch > c->max_batch || h < 1 || w < 1 || (size_t)h * w > c->P || h > 16384 || w > 16384)
        return ofk_fail(c, OFK_E_INVALID, "%s: batch %d / %dx%d exceeds the context (batch %d, %zu px)", who, batch, w, h, c->max_batch, c->P);
    return enter(c);
}

// host [batch][bytes_per] (tight) <-> device base + b*stride
static int h2d(ofk_ctx *c, void *dev, size_t stride, const void *host, size_t bytes_per, int batch)
{
    OFK_HIP(c, hipMemcpy2DAsync(dev, stride, host, bytes_per, bytes_per, batch, hipMemcpyHostToDevice, c->stream));
    return OFK_OK;
}
static int d2h(ofk_ctx *c, void *host, const void *dev, size_t stride, size_t bytes_per, int batch)
{
    OFK_HIP(c, hipMemcpy2DAsync(host, bytes_per, dev, stride, bytes_per, batch, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}
static int check_launch(ofk_ctx *c, const char *who)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ofk_fail(c, OFK_E_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return OFK_OK;
}
// what the stage entries over [batch][stride] point arrays ask of their counts
static int check_counts(ofk_ctx *c, const char *who, const int *counts, int batch, int stride)
{
    for (int b = 0; b < batch; ++b)
        if (counts[b] < 0 || counts[b] > stride) return ofk_fail(c, OFK_E_INVALID, "%s: counts[%d]=%d outside 0..%d", who, b, counts[b], stride);
    return OFK_OK;
}

// What every ofk_set_* / ofk_get_* pair of a struct setting does.  v == NULL: off(the context's copy) and nothing else; otherwise
// check(v), the setter's rules (its check_* function, which composes the refusal), and the struct is copied whole.  A setter that
// reads a struct whose mode is OFF like NULL hands NULL in for it.
template <class T, class Off, class Check>
static int setting_set(ofk_ctx *c, T ofk_ctx::*member, const T *v, Off off, Check check)
{
    if (!c) return OFK_E_INVALID;
    if (!v) { off(c->*member); return OFK_OK; }
    TRY(check(v));
    c->*member = *v;
    return OFK_OK;
}
template <class T>
static int setting_get(const ofk_ctx *c, T ofk_ctx::*member, T *out)
{
    if (!c || !out) return OFK_E_INVALID;
    *out = c->*member;
    return OFK_OK;
}

static int lazy_mask(ofk_ctx *c)
{
    if (!c->mask) OFK_HIP(c, hipMalloc((void **)&c->mask, (size_t)c->max_batch * c->img_stride));
    return OFK_OK;
}

// ------------------------------------------------------------------------------------------------ stage entry points
extern "C" int ofk_gray_bgr8(ofk_ctx *c, const uint8_t *bgr, int batch, int h, int w, uint8_t *gray)
{
    TRY(check_geom(c, batch, h, w, "ofk_gray_bgr8"));
    if (!bgr || !gray) return ofk_fail(c, OFK_E_INVALID, "ofk_gray_bgr8: NULL buffer");
    const size_t px = (size_t)h * w;
    TRY(h2d(c, c->bgr[0], c->bgr_stride, bgr, px * 3, batch));
    ofk_launch_gray(c->stream, c->bgr[0], c->bgr_stride, c->pyr[0], c->pyr_stride, batch, h, w);
    TRY(check_launch(c, "k_gray_bgr8"));
    return d2h(c, gray, c->pyr[0], c->pyr_stride, px, batch);
}

extern "C" int ofk_pyr_down_u8(ofk_ctx *c, const uint8_t *src, int batch, int h, int w, uint8_t *dst)
{
    TRY(check_geom(c, batch, h, w, "ofk_pyr_down_u8"));
    if (!src || !dst) return ofk_fail(c, OFK_E_INVALID, "ofk_pyr_down_u8: NULL buffer");
    if (h < 2 || w < 2) return ofk_fail(c, OFK_E_INVALID, "ofk_pyr_down_u8: image smaller than 2x2");
    const size_t px = (size_t)h * w, dpx = (size_t)((h + 1) / 2) * ((w + 1) / 2);
    TRY(h2d(c, c->pyr[0], c->pyr_stride, src, px, batch));
    ofk_launch_pyr_down(c->stream, c->pyr[0], c->pyr_stride, h, w, c->pyr[1], c->pyr_stride, batch);
    TRY(check_launch(c, "k_pyr_down"));
    return d2h(c, dst, c->pyr[1], c->pyr_stride, dpx, batch);
}

extern "C" int ofk_scharr_s16(ofk_ctx *c, const uint8_t *gray, int batch, int h, int w, int16_t *dxdy)
{
    TRY(check_geom(c, batch, h, w, "ofk_scharr_s16"));
    if (!gray || !dxdy) return ofk_fail(c, OFK_E_INVALID, "ofk_scharr_s16: NULL buffer");
    if (h < 2 || w < 2) return ofk_fail(c, OFK_E_INVALID, "ofk_scharr_s16: image smaller than 2x2");
    if (!c->deriv) OFK_HIP(c, hipMalloc((void **)&c->deriv, (size_t)c->max_batch * c->img_stride * 4));
    const size_t px = (size_t)h * w;
    TRY(h2d(c, c->pyr[0], c->pyr_stride, gray, px, batch));
    ofk_launch_scharr(c->stream, c->pyr[0], c->pyr_stride, h, w, c->deriv, c->img_stride, batch);
    TRY(check_launch(c, "k_scharr"));
    return d2h(c, dxdy, c->deriv, c->img_stride * 4, px * 4, batch);
}

extern "C" int ofk_warp_perspective(ofk_ctx *c, const uint8_t *src, int sh, int sw, int channels, const double *M, uint8_t *dst, int dh,
                                    int dw, int border, int border_value, int batch, int *covered)
{
    TRY(check_geom(c, batch, sh, sw, "ofk_warp_perspective (source)"));
    TRY(check_geom(c, batch, dh, dw, "ofk_warp_perspective (destination)"));
    if (!src || !M || !dst) return ofk_fail(c, OFK_E_INVALID, "ofk_warp_perspective: NULL buffer");
    if (channels != 1 && channels != 3) return ofk_fail(c, OFK_E_INVALID, "ofk_warp_perspective: %d channels (1 or 3)", channels);
    if (border != OFK_BORDER_CONSTANT && border != OFK_BORDER_REPLICATE) return ofk_fail(c, OFK_E_INVALID, "ofk_warp_perspective: unknown border %d", border);
    if (border_value < 0 || border_value > 255) return ofk_fail(c, OFK_E_INVALID, "ofk_warp_perspective: border_value %d outside 0..255", border_value);
    const size_t m_bytes = up((size_t)batch * 9 * sizeof(double), 256);
    TRY(ofk_need_scratch(c, m_bytes + (size_t)batch * sizeof(int)));
    double *d_M = (double *)c->scratch;
    int *d_cov = covered ? (int *)((char *)c->scratch + m_bytes) : nullptr;
    TRY(h2d(c, c->bgr[0], c->bgr_stride, src, (size_t)sh * sw * channels, batch));
    OFK_HIP(c, hipMemcpyAsync(d_M, M, (size_t)batch * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ofk_launch_warp(c->stream, c->bgr[0], c->bgr_stride, sh, sw, channels, d_M, c->bgr[1], c->bgr_stride, dh, dw, border, border_value, d_cov, batch);
    TRY(check_launch(c, "k_warp_u8"));
    if (covered) OFK_HIP(c, hipMemcpyAsync(covered, d_cov, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    return d2h(c, dst, c->bgr[1], c->bgr_stride, (size_t)dh * dw * channels, batch);
}

static int check_block(ofk_ctx *c, int h, int w, int block)
{
    if (block < 1 || block > 45) return ofk_fail(c, OFK_E_INVALID, "block_size %d outside 1..45", block);
    if (h < block + 4 || w < block + 4) return ofk_fail(c, OFK_E_INVALID, "image %dx%d too small for block_size %d", w, h, block);
    return OFK_OK;
}

extern "C" int ofk_mineig_response(ofk_ctx *c, const uint8_t *gray, int batch, int h, int w, int block, float *eig)
{
    TRY(check_geom(c, batch, h, w, "ofk_mineig_response"));
    if (!gray || !eig) return ofk_fail(c, OFK_E_INVALID, "ofk_mineig_response: NULL buffer");
    TRY(check_block(c, h, w, block));
    const size_t px = (size_t)h * w;
    TRY(h2d(c, c->pyr[0], c->pyr_stride, gray, px, batch));
    if (ofk_launch_mineig(c->stream, c->pyr[0], c->pyr_stride, h, w, block, c->eig, c->img_stride, nullptr, nullptr, 0, batch))
        return ofk_fail(c, OFK_E_INVALID, "k_mineig: LDS tile too large for block_size %d", block);
    TRY(check_launch(c, "k_mineig"));
    return d2h(c, eig, c->eig, c->img_stride * 4, px * 4, batch);
}

static int check_select(ofk_ctx *c, int max_corners, double quality, double min_distance)
{
    if (max_corners < 1 || max_corners > c->max_pts) return ofk_fail(c, OFK_E_INVALID, "max_corners %d outside 1..%d", max_corners, c->max_pts);
    if (!(quality > 0.0) || !(min_distance >= 0.0)) return ofk_fail(c, OFK_E_INVALID, "quality must be > 0 and min_distance >= 0");
    return OFK_OK;
}

static uint8_t *const *pyr_set(ofk_ctx *c, int set) { return set ? c->pyr_alt : c->pyr; }   // set 1: the overlapped schedule's second one

// ------------------------------------------------------------------------------------------------ the point corrections
// One row per setting that rewrites the tracked points in front of the solve stage, in the order of their launches in track().  With
// any of them on, the solve stage reads pts_prev_u / pts_next_u instead of pts_prev / pts_next; everything in the image keeps the raw ones.
struct point_setting {
    const char *set;                                            // the setter's name
    bool (*on)(const ofk_ctx *);
    int ofk_ctx::*batch;                                        // images of the latest run / step with it on (its download), 0 = none
};
static bool camera_on(const ofk_ctx *c) { return c->camera.model != OFK_CAMERA_OFF; }
static bool rs_on(const ofk_ctx *c) { return c->rs.mode != OFK_RS_OFF; }
static bool fm_on(const ofk_ctx *c) { return c->fm.mode != OFK_FM_OFF; }
enum { POINTS_CAMERA, POINTS_RS, POINTS_FM };
static const point_setting POINTS[3] = {
    {"ofk_set_camera", camera_on, &ofk_ctx::cam_batch},
    {"ofk_set_rolling_shutter", rs_on, &ofk_ctx::rs_batch},
    {"ofk_set_finite_motion", fm_on, &ofk_ctx::fm_batch},
};
static bool solve_points_on(const ofk_ctx *c)
{
    for (const point_setting &s : POINTS) if (s.on(c)) return true;
    return false;
}

// The context's per-image buffers from image b0 on, for nb images: the one place that knows their strides.  A slice of ofk_pairs_run
// builds one per stream; every other entry point works on the whole batch (b0 = 0, pyramid set 0).
struct View {
    int nb;
    uint8_t *bgr[2], *pyr[2];
    unsigned int *maxbits; int *cand_count; unsigned long long *cand, *cand_seg; int *seg_count;
    int nseg, segcap;                                            // key segments the latest detect_response filled (0: the flat list)
    unsigned *sel_hist; unsigned long long *sel_keys;
    float *pts_prev, *pts_next; uint8_t *status; float *err; int *counts;
    double *sensors, *records;
    float *pts_back, *err_back, *fb2; uint8_t *status_back; int *gate_stats;   // NULL until a run with a track gate on (gate_alloc)
    int *grid_stats;                                             // NULL until a selection with a corner grid on (grid_alloc)
    float *pts_prev_u, *pts_next_u;                              // NULL until a run with a point correction on (solve_points_prepare)
    const float *solve_prev, *solve_next;                        // what the solve stage reads: those two with a point correction on, else pts_prev / pts_next
};
static View view_of(ofk_ctx *c, int b0, int nb, int set)
{
    const size_t b = (size_t)b0;
    uint8_t *const *pyr = pyr_set(c, set);
    View v;
    v.nb = nb;
    for (int k = 0; k < 2; ++k) { v.bgr[k] = c->bgr[k] + b * c->bgr_stride; v.pyr[k] = pyr[k] + b * c->pyr_stride; }
    v.maxbits = c->maxbits + b * OFK_MAX_STRIDE; v.cand_count = c->cand_count + b * OFK_CNT_STRIDE;
    v.cand = c->cand + b * c->cand_cap; v.cand_seg = c->cand_seg + b * c->seg_keys; v.seg_count = c->seg_count + b * OFK_SEG_MAX;
    v.nseg = v.segcap = 0;
    v.sel_hist = c->sel_hist + b * 1024; v.sel_keys = c->sel_keys + b * OFK_CHUNK;
    v.pts_prev = c->pts_prev + b * c->max_pts * 2; v.pts_next = c->pts_next + b * c->max_pts * 2;
    v.status = c->status + b * c->max_pts; v.err = c->err + b * c->max_pts; v.counts = c->counts + b;
    v.sensors = c->sensors + b * OFK_SENSOR_DOUBLES; v.records = c->records + b * OFK_RECORD_DOUBLES;
    v.pts_back = v.err_back = v.fb2 = nullptr; v.status_back = nullptr; v.gate_stats = nullptr;
    if (c->pts_back) {
        v.pts_back = c->pts_back + b * c->max_pts * 2; v.err_back = c->err_back + b * c->max_pts; v.fb2 = c->fb2 + b * c->max_pts;
        v.status_back = c->status_back + b * c->max_pts; v.gate_stats = c->gate_stats + b * 4;
    }
    v.grid_stats = c->grid_stats ? c->grid_stats + b * 2 : nullptr;
    v.pts_prev_u = c->pts_prev_u ? c->pts_prev_u + b * c->max_pts * 2 : nullptr;
    v.pts_next_u = c->pts_next_u ? c->pts_next_u + b * c->max_pts * 2 : nullptr;
    const bool u = solve_points_on(c);
    v.solve_prev = u ? v.pts_prev_u : v.pts_prev; v.solve_next = u ? v.pts_next_u : v.pts_next;
    return v;
}

// Detection, first half: the detection state zeroed in one launch (histogram of the selection included), then response + 3x3 NMS +
// candidate keys of level 0 of v.pyr[0], no map in HBM.  dmask (optional) belongs to image 0 of the view.
static int detect_response(ofk_ctx *c, hipStream_t s, View &v, const uint8_t *dmask, int h, int w, int block, double quality)
{
    ofk_launch_zero_detect_state(s, v.maxbits, v.cand_count, v.sel_hist, v.nb);
    if (ofk_launch_mineig_cand(s, v.pyr[0], c->pyr_stride, h, w, block, v.maxbits, dmask, dmask ? c->img_stride : 0, quality, v.cand, c->cand_cap,
                               v.cand_count, v.cand_seg, c->seg_keys, v.seg_count, OFK_SEG_MAX, c->dev_flags, v.nb, &v.nseg, &v.segcap))
        return ofk_fail(c, OFK_E_INVALID, "corner response: block_size %d does not fit (LDS tile / key segments)", block);
    return OFK_OK;
}
// Second half: the candidates of the view -> at most max_corners (limit[b], where given) corners per image in dst / dst_counts
// g (cell > 0: the corner grid, checked by check_grid; the view's grid_stats exist then) with the occupancy list of the view's images
static void detect_select(ofk_ctx *c, hipStream_t s, const View &v, int h, int w, int max_corners, double quality, double min_distance,
                          float *dst, int *dst_counts, const int *limit, const ofk_corner_grid &g, const float *occ_pts = nullptr,
                          const int *occ_counts = nullptr, int occ_stride = 0)
{
    const ofk_sel_grid sg = {g.cell, g.cap, g.max_rank, occ_pts, occ_counts, occ_stride, v.grid_stats};
    ofk_launch_select(s, v.cand, c->cand_cap, v.cand_count, v.cand_seg, v.segcap, v.seg_count, v.nseg, v.maxbits, quality, h, w, max_corners,
                      (float)min_distance, dst, c->max_pts, dst_counts, limit, v.nb, v.sel_hist, v.sel_keys, g.cell > 0 ? &sg : nullptr);
}

// ------------------------------------------------------------------------------------------------ corner grid setting
// h == 0: the frame is not known yet (ofk_set_corner_grid); the cell count is checked by the call that selects
static int check_grid(ofk_ctx *c, const ofk_corner_grid *g, int h, int w, const char *who)
{
    if (g->cell < 0) return ofk_fail(c, OFK_E_INVALID, "%s: corner grid cell %d is negative", who, g->cell);
    if (g->cell == 0) return OFK_OK;
    if (g->cap < 1) return ofk_fail(c, OFK_E_INVALID, "%s: corner grid cap %d must be at least 1", who, g->cap);
    if (g->max_rank < 0) return ofk_fail(c, OFK_E_INVALID, "%s: corner grid max_rank %d is negative (0 = unlimited)", who, g->max_rank);
    if (h > 0) {
        const long long cells = (long long)((w + g->cell - 1) / g->cell) * ((h + g->cell - 1) / g->cell);
        if (cells > OFK_GRID_MAX_CELLS)
            return ofk_fail(c, OFK_E_INVALID, "%s: corner grid cell %d makes %lld cells of a %dx%d frame, more than OFK_GRID_MAX_CELLS = %d", who,
                            g->cell, cells, w, h, OFK_GRID_MAX_CELLS);
    }
    return OFK_OK;
}

extern "C" int ofk_set_corner_grid(ofk_ctx *c, const ofk_corner_grid *g)
{
    return setting_set(c, &ofk_ctx::grid, g, [](ofk_corner_grid &s) { s.cell = 0; },
                       [c](const ofk_corner_grid *v) { return check_grid(c, v, 0, 0, "ofk_set_corner_grid"); });
}
extern "C" int ofk_get_corner_grid(const ofk_ctx *c, ofk_corner_grid *g) { return setting_get(c, &ofk_ctx::grid, g); }

// the grid's resident buffers (statistics, the stage entries' occupancy list), allocated when a selection first needs them
static int grid_alloc(ofk_ctx *c)
{
    if (c->grid_stats) return OFK_OK;                            // one allocation, carved into the three buffers
    const size_t B = (size_t)c->max_batch, o_cnt = B * 8, o_pts = up(o_cnt + B * 4, 256);
    uint8_t *base = nullptr;
    OFK_HIP(c, hipMalloc((void **)&base, o_pts + B * c->max_pts * 8));
    c->grid_stats = (int *)base; c->grid_occ_counts = (int *)(base + o_cnt); c->grid_occ = (float *)(base + o_pts);
    return OFK_OK;
}
// what every entry point that selects does before its first launch: the setting against the frame, the buffers, the batch on record
static int grid_prepare(ofk_ctx *c, const ofk_corner_grid &g, int batch, int h, int w, const char *who)
{
    TRY(check_grid(c, &g, h, w, who));
    if (g.cell == 0) return OFK_OK;
    TRY(grid_alloc(c));
    c->grid_batch = batch;
    return OFK_OK;
}

extern "C" int ofk_corner_grid_download(ofk_ctx *c, int *stats)
{
    if (!c) return OFK_E_INVALID;
    if (!stats) return ofk_fail(c, OFK_E_INVALID, "ofk_corner_grid_download: stats is NULL");
    if (c->grid_batch < 1 || !c->grid_stats) return ofk_fail(c, OFK_E_INVALID, "ofk_corner_grid_download: no selection with a corner grid on yet");
    TRY(enter(c));
    OFK_HIP(c, hipMemcpyAsync(stats, c->grid_stats, (size_t)c->grid_batch * 8, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

// device-side: eig (+mask) resident in ctx -> corners in pts_prev / counts
static int run_select(ofk_ctx *c, const uint8_t *dmask, int batch, int h, int w, int max_corners, double quality, double min_distance,
                      const ofk_corner_grid &g, const float *occ_pts, const int *occ_counts, int occ_stride)
{
    const View v = view_of(c, 0, batch, 0);                      // nseg = 0: k_nms fills the flat list
    ofk_launch_zero_detect_state(c->stream, v.maxbits, v.cand_count, v.sel_hist, batch);
    ofk_launch_maxbits(c->stream, c->eig, c->img_stride, dmask, c->img_stride, h, w, v.maxbits, batch);
    ofk_launch_nms(c->stream, c->eig, c->img_stride, dmask, c->img_stride, h, w, v.maxbits, quality, v.cand, c->cand_cap, v.cand_count,
                   c->dev_flags, batch);
    detect_select(c, c->stream, v, h, w, max_corners, quality, min_distance, v.pts_prev, v.counts, nullptr, g, occ_pts, occ_counts, occ_stride);
    return check_launch(c, "corner selection");
}

// flags = the host's copy of dev_flags.  A negative count or flag bit 0 is a candidate overflow: the counts (where the caller asked for
// them) read 0 for those images and the device flags are cleared for the next call.
static int check_capacity(ofk_ctx *c, const int *flags, int *counts, int batch)
{
    bool over = (flags[0] & 1) != 0;
    for (int b = 0; counts && b < batch; ++b) if (counts[b] < 0) { over = true; counts[b] = 0; }
    if (!over) return OFK_OK;
    hipMemsetAsync(c->dev_flags, 0, 16, c->stream);
    return ofk_fail(c, OFK_E_CAPACITY, "corner candidates exceeded the per-image capacity (%d)", c->cand_cap);
}

static int fetch_corners(ofk_ctx *c, int batch, int max_corners, float *pts, int *counts)
{
    int flags[4];
    OFK_HIP(c, hipMemcpyAsync(flags, c->dev_flags, 16, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipMemcpyAsync(counts, c->counts, (size_t)batch * 4, hipMemcpyDeviceToHost, c->stream));
    TRY(d2h(c, pts, c->pts_prev, (size_t)c->max_pts * 8, (size_t)max_corners * 8, batch));
    return check_capacity(c, flags, counts, batch);
}

// The occupancy list of a stage entry (host, nullable) -> the context's buffer; *dev / *dev_counts NULL without a list or a grid
static int grid_occupancy(ofk_ctx *c, const ofk_corner_grid &g, const float *occ_pts, const int *occ_counts, int occ_stride, int batch,
                          const float **dev, const int **dev_counts, const char *who)
{
    *dev = nullptr; *dev_counts = nullptr;
    if (g.cell == 0 || !occ_pts) return OFK_OK;
    if (!occ_counts || occ_stride < 1 || occ_stride > c->max_pts)
        return ofk_fail(c, OFK_E_INVALID, "%s: an occupancy list needs its counts and occ_stride in 1..%d (%d)", who, c->max_pts, occ_stride);
    OFK_HIP(c, hipMemcpyAsync(c->grid_occ, occ_pts, (size_t)batch * occ_stride * 8, hipMemcpyHostToDevice, c->stream));
    OFK_HIP(c, hipMemcpyAsync(c->grid_occ_counts, occ_counts, (size_t)batch * 4, hipMemcpyHostToDevice, c->stream));
    *dev = c->grid_occ; *dev_counts = c->grid_occ_counts;
    return OFK_OK;
}

static int select_corners_impl(ofk_ctx *c, const char *who, const float *eig, const uint8_t *mask, int batch, int h, int w, int max_corners,
                               double quality, double min_distance, float *pts, int *counts, const ofk_corner_grid &g, const float *occ_pts,
                               const int *occ_counts, int occ_stride)
{
    TRY(check_geom(c, batch, h, w, who));
    if (!eig || !pts || !counts) return ofk_fail(c, OFK_E_INVALID, "%s: NULL buffer", who);
    if (h < 3 || w < 3) return ofk_fail(c, OFK_E_INVALID, "%s: image smaller than 3x3", who);
    TRY(check_select(c, max_corners, quality, min_distance));
    TRY(grid_prepare(c, g, batch, h, w, who));
    const float *docc; const int *dcnt;
    TRY(grid_occupancy(c, g, occ_pts, occ_counts, occ_stride, batch, &docc, &dcnt, who));
    const size_t px = (size_t)h * w;
    TRY(h2d(c, c->eig, c->img_stride * 4, eig, px * 4, batch));
    const uint8_t *dmask = nullptr;
    if (mask) { TRY(lazy_mask(c)); TRY(h2d(c, c->mask, c->img_stride, mask, px, batch)); dmask = c->mask; }
    TRY(run_select(c, dmask, batch, h, w, max_corners, quality, min_distance, g, docc, dcnt, occ_stride));
    return fetch_corners(c, batch, max_corners, pts, counts);
}

static int good_features_impl(ofk_ctx *c, const char *who, const uint8_t *gray, const uint8_t *mask, int batch, int h, int w, int max_corners,
                              double quality, double min_distance, int block, float *pts, int *counts, const ofk_corner_grid &g,
                              const float *occ_pts, const int *occ_counts, int occ_stride)
{
    TRY(check_geom(c, batch, h, w, who));
    if (!gray || !pts || !counts) return ofk_fail(c, OFK_E_INVALID, "%s: NULL buffer", who);
    TRY(check_block(c, h, w, block));
    TRY(check_select(c, max_corners, quality, min_distance));
    TRY(grid_prepare(c, g, batch, h, w, who));
    const float *docc; const int *dcnt;
    TRY(grid_occupancy(c, g, occ_pts, occ_counts, occ_stride, batch, &docc, &dcnt, who));
    const size_t px = (size_t)h * w;
    TRY(h2d(c, c->pyr[0], c->pyr_stride, gray, px, batch));
    const uint8_t *dmask = nullptr;
    if (mask) { TRY(lazy_mask(c)); TRY(h2d(c, c->mask, c->img_stride, mask, px, batch)); dmask = c->mask; }
    View v = view_of(c, 0, batch, 0);
    TRY(detect_response(c, c->stream, v, dmask, h, w, block, quality));
    detect_select(c, c->stream, v, h, w, max_corners, quality, min_distance, v.pts_prev, v.counts, nullptr, g, docc, dcnt, occ_stride);
    TRY(check_launch(c, "corner detection"));
    return fetch_corners(c, batch, max_corners, pts, counts);
}

static const ofk_corner_grid k_grid_off = {0, 0, 0};

extern "C" int ofk_select_corners(ofk_ctx *c, const float *eig, const uint8_t *mask, int batch, int h, int w, int max_corners,
                                  double quality, double min_distance, float *pts, int *counts)
{
    if (!c) return OFK_E_INVALID;
    return select_corners_impl(c, "ofk_select_corners", eig, mask, batch, h, w, max_corners, quality, min_distance, pts, counts, c->grid, nullptr,
                               nullptr, 0);
}

extern "C" int ofk_select_corners_grid(ofk_ctx *c, const float *eig, const uint8_t *mask, int batch, int h, int w, int max_corners,
                                       double quality, double min_distance, float *pts, int *counts, const ofk_corner_grid *g,
                                       const float *occ_pts, const int *occ_counts, int occ_stride)
{
    if (!c) return OFK_E_INVALID;
    return select_corners_impl(c, "ofk_select_corners_grid", eig, mask, batch, h, w, max_corners, quality, min_distance, pts, counts,
                               g ? *g : k_grid_off, occ_pts, occ_counts, occ_stride);
}

extern "C" int ofk_good_features(ofk_ctx *c, const uint8_t *gray, const uint8_t *mask, int batch, int h, int w, int max_corners,
                                 double quality, double min_distance, int block, float *pts, int *counts)
{
    if (!c) return OFK_E_INVALID;
    return good_features_impl(c, "ofk_good_features", gray, mask, batch, h, w, max_corners, quality, min_distance, block, pts, counts, c->grid,
                              nullptr, nullptr, 0);
}

extern "C" int ofk_good_features_grid(ofk_ctx *c, const uint8_t *gray, const uint8_t *mask, int batch, int h, int w, int max_corners,
                                      double quality, double min_distance, int block, float *pts, int *counts, const ofk_corner_grid *g,
                                      const float *occ_pts, const int *occ_counts, int occ_stride)
{
    if (!c) return OFK_E_INVALID;
    return good_features_impl(c, "ofk_good_features_grid", gray, mask, batch, h, w, max_corners, quality, min_distance, block, pts, counts,
                              g ? *g : k_grid_off, occ_pts, occ_counts, occ_stride);
}

static int check_lk(ofk_ctx *c, int h, int w, int win, int max_level)
{
    if (win < 3 || win > 31 || (win & 1) == 0) return ofk_fail(c, OFK_E_INVALID, "win %d must be odd and in 3..31", win);
    if (max_level < 0 || max_level > c->max_level) return ofk_fail(c, OFK_E_INVALID, "max_level %d outside 0..%d", max_level, c->max_level);
    if (h <= win || w <= win) return ofk_fail(c, OFK_E_INVALID, "image %dx%d not larger than the LK window %d", w, h, win);
    return OFK_OK;
}

// Levels 1..lv.n of nb resident pyramids (pyr1 == NULL) or of nb pairs of them: levels 1..3 in one pass where the geometry allows it,
// then level by level
static void build_pyramids(ofk_ctx *c, hipStream_t s, uint8_t *pyr0, uint8_t *pyr1, const ofk_levels &lv, int nb)
{
    for (int l = ofk_launch_pyr3(s, pyr0, pyr1, c->pyr_stride, lv, nb, pyr1 ? 2 * nb : nb) ? 4 : 1; l <= lv.n; ++l) {
        if (pyr1)
            ofk_launch_pyr_down2(s, pyr0 + lv.off[l - 1], pyr1 + lv.off[l - 1], c->pyr_stride, lv.h[l - 1], lv.w[l - 1], pyr0 + lv.off[l],
                                 pyr1 + lv.off[l], c->pyr_stride, nb);
        else
            ofk_launch_pyr_down(s, pyr0 + lv.off[l - 1], c->pyr_stride, lv.h[l - 1], lv.w[l - 1], pyr0 + lv.off[l], c->pyr_stride, nb);
    }
}

static bool gate_on(const ofk_track_gate &g) { return g.fb_mode != OFK_FB_OFF || g.err_max != 0.0; }

// ------------------------------------------------------------------------------------------------ camera setting
// one_focal: ofk_set_camera's extra rule (the solve has one scaling)
static int check_camera(ofk_ctx *c, const ofk_camera *m, bool one_focal, const char *who)
{
    if (m->model != OFK_CAMERA_BROWN && m->model != OFK_CAMERA_FISHEYE)
        return ofk_fail(c, OFK_E_INVALID, "%s: model %d is neither OFK_CAMERA_BROWN nor OFK_CAMERA_FISHEYE", who, m->model);
    if (m->iters < 1 || m->iters > 50) return ofk_fail(c, OFK_E_INVALID, "%s: iters %d outside 1..50", who, m->iters);
    const double vals[8] = {m->fx, m->fy, m->cx, m->cy, m->fo_x, m->fo_y, m->co_x, m->co_y};
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(vals[k]) || !std::isfinite(m->k[k])) return ofk_fail(c, OFK_E_INVALID, "%s: a field is not finite", who);
    if (m->fx == 0.0 || m->fy == 0.0 || m->fo_x == 0.0 || m->fo_y == 0.0) return ofk_fail(c, OFK_E_INVALID, "%s: fx, fy, fo_x and fo_y must not be 0", who);
    if (m->model == OFK_CAMERA_FISHEYE && (m->k[4] != 0.0 || m->k[5] != 0.0 || m->k[6] != 0.0 || m->k[7] != 0.0))
        return ofk_fail(c, OFK_E_INVALID, "%s: the fisheye model has four coefficients: k[4..7] must be 0", who);
    if (one_focal && m->fo_x != m->fo_y)
        return ofk_fail(c, OFK_E_INVALID, "%s: fo_x = %g and fo_y = %g differ: the solve has one scaling (sensors[19] = 1 / fo_x)", who, m->fo_x, m->fo_y);
    return OFK_OK;
}

extern "C" int ofk_set_camera(ofk_ctx *c, const ofk_camera *m)
{
    return setting_set(c, &ofk_ctx::camera, m && m->model == OFK_CAMERA_OFF ? nullptr : m, [](ofk_camera &s) { s.model = OFK_CAMERA_OFF; },
                       [c](const ofk_camera *v) { return check_camera(c, v, true, "ofk_set_camera"); });
}
extern "C" int ofk_get_camera(const ofk_ctx *c, ofk_camera *m) { return setting_get(c, &ofk_ctx::camera, m); }

// ------------------------------------------------------------------------------------------------ rolling-shutter setting
// stage: ofk_rs_correct_points' extra rule (no run to take the frame height from)
static int check_rs(ofk_ctx *c, const ofk_rshutter *r, bool stage, const char *who)
{
    if (r->mode != OFK_RS_FLOW && r->mode != OFK_RS_GYRO)
        return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_RS_FLOW nor OFK_RS_GYRO", who, r->mode);
    if (!std::isfinite(r->readout) || !std::isfinite(r->anchor) || !std::isfinite(r->omega_gain))
        return ofk_fail(c, OFK_E_INVALID, "%s: a field is not finite", who);
    if (fabs(r->readout) > 1.0) return ofk_fail(c, OFK_E_INVALID, "%s: readout %g outside -1..1 frame intervals", who, r->readout);
    if (r->anchor < 0.0 || r->anchor > 1.0) return ofk_fail(c, OFK_E_INVALID, "%s: anchor %g outside 0..1", who, r->anchor);
    if (r->rows < 0 || r->rows > 65536) return ofk_fail(c, OFK_E_INVALID, "%s: rows %d outside 0..65536", who, r->rows);
    if (stage && r->rows == 0) return ofk_fail(c, OFK_E_INVALID, "%s: rows 0 means the frame height of a run: the stage entry needs rows > 0", who);
    if (r->omega_gain == 0.0) return ofk_fail(c, OFK_E_INVALID, "%s: omega_gain must not be 0", who);
    return OFK_OK;
}

extern "C" int ofk_set_rolling_shutter(ofk_ctx *c, const ofk_rshutter *r)
{
    return setting_set(c, &ofk_ctx::rs, r && r->mode == OFK_RS_OFF ? nullptr : r, [](ofk_rshutter &s) { s.mode = OFK_RS_OFF; },
                       [c](const ofk_rshutter *v) { return check_rs(c, v, false, "ofk_set_rolling_shutter"); });
}
extern "C" int ofk_get_rolling_shutter(const ofk_ctx *c, ofk_rshutter *r) { return setting_get(c, &ofk_ctx::rs, r); }

// ------------------------------------------------------------------------------------------------ finite-motion setting
static int check_fm(ofk_ctx *c, const ofk_finite_motion *f, const char *who)
{
    if (f->mode != OFK_FM_EXACT) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is not OFK_FM_EXACT", who, f->mode);
    if (!std::isfinite(f->min_depth) || !(f->min_depth > 0.0) || f->min_depth > 1.0)
        return ofk_fail(c, OFK_E_INVALID, "%s: min_depth %g outside (0, 1]", who, f->min_depth);
    return OFK_OK;
}

extern "C" int ofk_set_finite_motion(ofk_ctx *c, const ofk_finite_motion *f)
{
    return setting_set(c, &ofk_ctx::fm, f && f->mode == OFK_FM_OFF ? nullptr : f, [](ofk_finite_motion &s) { s.mode = OFK_FM_OFF; },
                       [c](const ofk_finite_motion *v) { return check_fm(c, v, "ofk_set_finite_motion"); });
}
extern "C" int ofk_get_finite_motion(const ofk_ctx *c, ofk_finite_motion *f) { return setting_get(c, &ofk_ctx::fm, f); }

// What a fused step may not have beside a setting that rewrites the sensor model's rows (ofk.h), and the refusal that names them.
enum { NO_OFMODULE = 1, NO_ROTATIONAL = 2, NO_LEGACY = 4 };
static int refuse_not_sensor_model(ofk_ctx *c, const char *who, int refused, const char *what, const char *set)
{
    static const char *const names[3] = {"OFK_SOLVE_OFMODULE", "OFK_FLOW_ROTATIONAL", "OFK_KEEP_LEGACY"};
    char list[64] = "";
    for (int k = 0; k < 3; ++k)
        if (refused >> k & 1) { if (list[0]) strcat(list, " / "); strcat(list, names[k]); }
    return ofk_fail(c, OFK_E_INVALID, "%s: %s are not the sensor model: no %s (%s is on)", who, list, what, set);
}

// The fused steps' own refusals with the finite motion on (ofk.h): the rewrite is of the sensor model's rows.
static int fm_check_step(ofk_ctx *c, int variant, const ofk_fusion *fu, const char *who)
{
    if (!fm_on(c)) return OFK_OK;
    if (variant == OFK_SOLVE_OFMODULE || (fu && (fu->flow == OFK_FLOW_ROTATIONAL || fu->keep == OFK_KEEP_LEGACY)))
        return refuse_not_sensor_model(c, who, NO_OFMODULE | NO_ROTATIONAL | NO_LEGACY, "finite motion", POINTS[POINTS_FM].set);
    return OFK_OK;
}

// the solve stage's own points (the camera's ideal pixels, the rolling shutter's corrected ones, the finite motion's rewritten ones, or
// any of them in turn): their resident buffers, allocated when a run first needs them; `batch`: the run's images, on record for the
// download of every row that is on
static int solve_points_prepare(ofk_ctx *c, int batch)
{
    if (!solve_points_on(c)) return OFK_OK;
    if (!c->pts_prev_u) {                                        // one allocation, carved into the two buffers
        const size_t np = (size_t)c->max_batch * c->max_pts;
        float *base = nullptr;
        OFK_HIP(c, hipMalloc((void **)&base, np * 16));
        OFK_HIP(c, hipMemsetAsync(base, 0, np * 16, c->stream));
        OFK_HIP(c, hipStreamSynchronize(c->stream));
        c->pts_prev_u = base; c->pts_next_u = base + np * 2;
    }
    for (const point_setting &s : POINTS) if (s.on(c)) c->*s.batch = batch;
    return OFK_OK;
}

// The points the solve stage of the latest run or step with the row's setting on saw: the first min(stride, max_pts) of each image.
static int points_download(ofk_ctx *c, const point_setting &s, const char *who, float *prev, float *next, int stride)
{
    if (!c) return OFK_E_INVALID;
    if (c->*s.batch < 1 || !c->pts_prev_u) return ofk_fail(c, OFK_E_INVALID, "%s: no run or step with %s on yet", who, s.set);
    if (stride < 1) return ofk_fail(c, OFK_E_INVALID, "%s: stride %d", who, stride);
    TRY(enter(c));
    const size_t n = (size_t)(stride < c->max_pts ? stride : c->max_pts), mp = (size_t)c->max_pts;
    if (prev) OFK_HIP(c, hipMemcpy2DAsync(prev, (size_t)stride * 8, c->pts_prev_u, mp * 8, n * 8, c->*s.batch, hipMemcpyDeviceToHost, c->stream));
    if (next) OFK_HIP(c, hipMemcpy2DAsync(next, (size_t)stride * 8, c->pts_next_u, mp * 8, n * 8, c->*s.batch, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

// ------------------------------------------------------------------------------------------------ lighting-insensitive LK setting
static int check_light(ofk_ctx *c, const ofk_lk_light *l, const char *who)
{
    if (l->mode != OFK_LIGHT_OFF && l->mode != OFK_LIGHT_BIAS && l->mode != OFK_LIGHT_GAIN)
        return ofk_fail(c, OFK_E_INVALID, "%s: light mode %d is none of OFK_LIGHT_OFF, _BIAS, _GAIN", who, l->mode);
    if (!(std::isfinite(l->gain_max) && l->gain_max > 1.0))
        return ofk_fail(c, OFK_E_INVALID, "%s: gain_max = %g must be finite and above 1", who, l->gain_max);
    return OFK_OK;
}

extern "C" int ofk_set_lk_light(ofk_ctx *c, const ofk_lk_light *l)
{
    return setting_set(c, &ofk_ctx::light, l && l->mode == OFK_LIGHT_OFF ? nullptr : l, [](ofk_lk_light &s) { s.mode = OFK_LIGHT_OFF; },
                       [c](const ofk_lk_light *v) { return check_light(c, v, "ofk_set_lk_light"); });
}
extern "C" int ofk_get_lk_light(const ofk_ctx *c, ofk_lk_light *l) { return setting_get(c, &ofk_ctx::light, l); }

// The one place LK is launched from: the setting off is ofk_launch_lk, the kernels and the launch of before the setting existed.
static void launch_lk(hipStream_t s, const uint8_t *prev, const uint8_t *next, size_t pyr_stride, const ofk_levels &lv, const float *prev_pts,
                      const int *counts, int pts_stride, int win, int max_count, double eps, double min_eig_thr, float *next_pts,
                      uint8_t *status, float *err, int batch, int flags, const ofk_lk_light &light)
{
    if (light.mode == OFK_LIGHT_OFF)
        ofk_launch_lk(s, prev, next, pyr_stride, lv, prev_pts, counts, pts_stride, win, max_count, eps, min_eig_thr, next_pts, status, err, batch, flags);
    else
        ofk_launch_lk_light(s, prev, next, pyr_stride, lv, prev_pts, counts, pts_stride, win, max_count, eps, min_eig_thr, next_pts, status, err, batch,
                            flags, light);
}

// Rules 2-5 of the track gates (ofk.h) behind a forward LK of the view on stream s: the backward LK, which is the forward launch with
// the two pyramids swapped and a level table of the gate's depth, then k_track_gate.  The view's gate buffers exist (gate_alloc).
// light: the forward pass's ofk_lk_light; the backward pass tracks under the same mode.
static int gate_tracks(ofk_ctx *c, hipStream_t s, const View &v, const ofk_levels &lv, int win, int max_level, int max_count, double eps,
                       double min_eig_thr, const ofk_track_gate &g, const ofk_lk_light &light)
{
    const bool fb = g.fb_mode != OFK_FB_OFF;
    if (fb) {
        const int depth = g.fb_level < 0 || g.fb_level > max_level ? max_level : g.fb_level;
        const ofk_levels lb = ofk_make_levels(lv.h[0], lv.w[0], win, depth);
        const bool seeded = g.fb_mode == OFK_FB_SEEDED;            // LK's next_pts is in/out: the search starts at the original points
        if (seeded) OFK_HIP(c, hipMemcpyAsync(v.pts_back, v.pts_prev, (size_t)v.nb * c->max_pts * 8, hipMemcpyDeviceToDevice, s));
        launch_lk(s, v.pyr[1], v.pyr[0], c->pyr_stride, lb, v.pts_next, v.counts, c->max_pts, win, max_count, eps, min_eig_thr, v.pts_back,
                  v.status_back, v.err_back, v.nb, seeded ? OFK_LK_USE_INITIAL_FLOW : 0, light);
    }
    ofk_launch_track_gate(s, v.pts_prev, fb ? v.pts_back : nullptr, fb ? v.status_back : nullptr, v.err, v.counts, c->max_pts, fb ? 1 : 0,
                          (float)(g.fb_thr * g.fb_thr), g.err_max != 0.0 ? 1 : 0, (float)g.err_max, v.status, fb ? v.fb2 : nullptr, v.gate_stats,
                          v.nb);
    return OFK_OK;
}

// The track step of the resident chains: with ofk_set_lk_seed on, the start positions are written where LK reads them (imu_state: the
// source k_stream_fuse uses under use_imu, NULL = the sensors only) and LK starts there;
// with ofk_set_lk_light on, both LK passes are the lighting-insensitive kernels;
// with ofk_set_track_gate on, the gates follow on the same stream.  With ofk_set_camera on (the view's ideal buffers exist:
// solve_points_prepare) the sensors speak of the ideal image, so the predictor runs on the ideal points and its seeds are brought back into
// the image; behind the gates the ideal points of both sets are written for the solve stage - one launch, unless the seed needed
// the previous points' earlier.  With ofk_set_rolling_shutter on, one k_rs_correct launch follows: it reads the raw rows and the
// ideal points (the camera's, corrected in place, or the raw points themselves) and writes what the solve stage reads.  With
// ofk_set_finite_motion on, one k_finite_correct launch follows that: in place on those buffers, or from the raw points into them.
// tt != NULL (a stream step with ofk_set_track_table's seed on; the view is the whole batch): the k_track_seed launch of rule 5 behind
// the model seeds, and LK starts at what both have written.
// tp != NULL (a stream step with ofk_set_track_template on; the view is the whole batch, age the table's): rules 1-5 of the templates
// directly behind the gates, on the raw points and the status everything below reads.
// key_copy != NULL (a stream step with ofk_set_keyframe on): where the finite-motion rewrite is in place, the ideal next points in
// front of it are kept there.
static int track(ofk_ctx *c, hipStream_t s, const View &v, const ofk_levels &lv, const ofk_params *p, const double *imu_state,
                 const ofk_tt_rows *tt = nullptr, const ofk_tp_rows *tp = nullptr, const int *age = nullptr, float *key_copy = nullptr)
{
    const bool seeded = c->lk_seed_mode != OFK_SEED_OFF, cam = camera_on(c);
    if (seeded && cam) {
        ofk_launch_camera(s, &c->camera, 0, v.pts_prev, v.pts_prev_u, nullptr, nullptr, v.counts, c->max_pts, v.nb);
        ofk_launch_seed_points(s, v.pts_prev_u, v.counts, c->max_pts, v.sensors, imu_state, c->lk_seed_mode, c->lk_seed_gain, v.pts_next, v.nb);
        ofk_launch_camera(s, &c->camera, 1, v.pts_next, v.pts_next, nullptr, nullptr, v.counts, c->max_pts, v.nb);
    } else if (seeded)
        ofk_launch_seed_points(s, v.pts_prev, v.counts, c->max_pts, v.sensors, imu_state, c->lk_seed_mode, c->lk_seed_gain, v.pts_next, v.nb);
    if (tt) ofk_launch_track_seed(s, v.pts_prev, v.counts, c->max_pts, tt->age, tt->flow_xy, (float)c->tt.gain, seeded ? 1 : 0, v.pts_next, v.nb);
    launch_lk(s, v.pyr[0], v.pyr[1], c->pyr_stride, lv, v.pts_prev, v.counts, c->max_pts, p->win, p->max_count, p->eps, p->min_eig_thr,
              v.pts_next, v.status, v.err, v.nb, seeded || tt ? OFK_LK_USE_INITIAL_FLOW : 0, c->light);
    if (gate_on(c->gate)) TRY(gate_tracks(c, s, v, lv, p->win, p->max_level, p->max_count, p->eps, p->min_eig_thr, c->gate, c->light));
    if (tp) {
        ofk_launch_track_affine(s, v.pts_prev, v.pts_next, v.status, v.counts, c->max_pts, lv.h[0], lv.w[0], &c->tpl, tp->L, tp->rec, v.nb);
        ofk_launch_track_template(s, *tp, v.pyr[0] + lv.off[0], v.pyr[1] + lv.off[0], c->pyr_stride, lv.h[0], lv.w[0], v.pts_prev, v.pts_next, v.status,
                                  age, v.counts, c->max_pts, &c->tpl, v.nb);
    }
    if (cam && seeded) ofk_launch_camera(s, &c->camera, 0, v.pts_next, v.pts_next_u, nullptr, nullptr, v.counts, c->max_pts, v.nb);
    else if (cam) ofk_launch_camera(s, &c->camera, 0, v.pts_prev, v.pts_prev_u, v.pts_next, v.pts_next_u, v.counts, c->max_pts, v.nb);
    if (rs_on(c)) {
        ofk_rshutter r = c->rs;
        if (r.rows == 0) r.rows = lv.h[0];                       // the frame height of the run
        ofk_launch_rs_correct(s, &r, v.pts_prev, v.pts_next, cam ? v.pts_prev_u : nullptr, cam ? v.pts_next_u : nullptr, v.pts_prev_u, v.pts_next_u,
                              v.counts, c->max_pts, v.sensors, imu_state, v.nb);
    }
    if (fm_on(c)) {
        const bool id = cam || rs_on(c);
        if (id && key_copy) OFK_HIP(c, hipMemcpyAsync(key_copy, v.pts_next_u, (size_t)v.nb * c->max_pts * 8, hipMemcpyDeviceToDevice, s));
        ofk_launch_finite_correct(s, &c->fm, id ? v.pts_prev_u : v.pts_prev, id ? v.pts_next_u : v.pts_next, v.pts_prev_u, v.pts_next_u, v.counts,
                                  c->max_pts, v.sensors, imu_state, v.nb);
    }
    return OFK_OK;
}

// ------------------------------------------------------------------------------------------------ track gate setting
static int check_gate(ofk_ctx *c, const ofk_track_gate *g, const char *who)
{
    if (g->fb_mode != OFK_FB_OFF && g->fb_mode != OFK_FB_PLAIN && g->fb_mode != OFK_FB_SEEDED)
        return ofk_fail(c, OFK_E_INVALID, "%s: fb_mode %d is none of OFK_FB_OFF, _PLAIN, _SEEDED", who, g->fb_mode);
    if (g->fb_mode != OFK_FB_OFF && !(std::isfinite(g->fb_thr) && g->fb_thr > 0.0))
        return ofk_fail(c, OFK_E_INVALID, "%s: fb_thr = %g must be finite and positive", who, g->fb_thr);
    if (g->fb_level < -1 || g->fb_level > c->max_level)
        return ofk_fail(c, OFK_E_INVALID, "%s: fb_level %d outside -1..%d", who, g->fb_level, c->max_level);
    if (!(std::isfinite(g->err_max) && g->err_max >= 0.0))
        return ofk_fail(c, OFK_E_INVALID, "%s: err_max = %g must be finite and not negative (0 = off)", who, g->err_max);
    return OFK_OK;
}

extern "C" int ofk_set_track_gate(ofk_ctx *c, const ofk_track_gate *g)
{
    return setting_set(c, &ofk_ctx::gate, g, [](ofk_track_gate &s) { s.fb_mode = OFK_FB_OFF; s.err_max = 0.0; },       // both gates
                       [c](const ofk_track_gate *v) { return check_gate(c, v, "ofk_set_track_gate"); });
}
extern "C" int ofk_get_track_gate(const ofk_ctx *c, ofk_track_gate *g) { return setting_get(c, &ofk_ctx::gate, g); }

// the resident buffers of the gates, allocated when a run first needs them
static int gate_alloc(ofk_ctx *c)
{
    if (c->pts_back) return OFK_OK;                              // one allocation, carved into the five buffers: all of them or none
    const size_t B = (size_t)c->max_batch, np = B * c->max_pts;
    const size_t o_err = np * 8, o_fb2 = o_err + np * 4, o_stats = o_fb2 + np * 4, o_st = o_stats + B * 16;
    uint8_t *base = nullptr;
    OFK_HIP(c, hipMalloc((void **)&base, o_st + np));
    c->pts_back = (float *)base; c->err_back = (float *)(base + o_err); c->fb2 = (float *)(base + o_fb2);
    c->gate_stats = (int *)(base + o_stats); c->status_back = base + o_st;
    return OFK_OK;
}

extern "C" int ofk_track_gate_download(ofk_ctx *c, float *fb2, float *back_pts, uint8_t *back_status, int stride, int *stats)
{
    if (!c) return OFK_E_INVALID;
    if (c->gate_batch < 1 || !c->pts_back) return ofk_fail(c, OFK_E_INVALID, "ofk_track_gate_download: no run or step with ofk_set_track_gate on yet");
    if ((fb2 || back_pts || back_status) && stride < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_track_gate_download: stride %d", stride);
    TRY(enter(c));
    const int B = c->gate_batch;
    const size_t n = (size_t)(stride < c->max_pts ? stride : c->max_pts), mp = (size_t)c->max_pts;
    if (c->gate_fb) {
        if (fb2) OFK_HIP(c, hipMemcpy2DAsync(fb2, (size_t)stride * 4, c->fb2, mp * 4, n * 4, B, hipMemcpyDeviceToHost, c->stream));
        if (back_pts) OFK_HIP(c, hipMemcpy2DAsync(back_pts, (size_t)stride * 8, c->pts_back, mp * 8, n * 8, B, hipMemcpyDeviceToHost, c->stream));
        if (back_status) OFK_HIP(c, hipMemcpy2DAsync(back_status, stride, c->status_back, mp, n, B, hipMemcpyDeviceToHost, c->stream));
    } else {
        for (int b = 0; b < B; ++b) {                            // the err cap alone: there was no backward pass
            if (fb2) memset(fb2 + (size_t)b * stride, 0, n * 4);
            if (back_pts) memset(back_pts + (size_t)b * stride * 2, 0, n * 8);
            if (back_status) memset(back_status + (size_t)b * stride, 0, n);
        }
    }
    if (stats) OFK_HIP(c, hipMemcpyAsync(stats, c->gate_stats, (size_t)B * 16, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

static int lk_pyr_impl(ofk_ctx *c, const char *who, const uint8_t *prev, const uint8_t *next, int batch, int h, int w, const float *prev_pts,
                       const int *counts, int pts_stride, int win, int max_level, int max_count, double eps, double min_eig_thr,
                       const float *init_pts, int flags, float *next_pts, uint8_t *status, float *err, const ofk_track_gate *g = nullptr,
                       float *back_pts = nullptr, uint8_t *back_status = nullptr, float *fb2 = nullptr, const ofk_lk_light *light = nullptr)
{
    TRY(check_geom(c, batch, h, w, who));
    if (!prev || !next || !prev_pts || !counts || !next_pts || !status || !err) return ofk_fail(c, OFK_E_INVALID, "%s: NULL buffer", who);
    TRY(check_lk(c, h, w, win, max_level));
    if (pts_stride < 1 || pts_stride > c->max_pts) return ofk_fail(c, OFK_E_INVALID, "pts_stride %d outside 1..%d", pts_stride, c->max_pts);
    for (int b = 0; b < batch; ++b)
        if (counts[b] < 0 || counts[b] > pts_stride) return ofk_fail(c, OFK_E_INVALID, "counts[%d]=%d outside 0..%d", b, counts[b], pts_stride);
    if (flags & ~(OFK_LK_USE_INITIAL_FLOW | OFK_LK_GET_MIN_EIGENVALS)) return ofk_fail(c, OFK_E_INVALID, "%s: unknown flag bits 0x%x", who, flags);
    if (g) {                                                     // the setting's rules hold for a structure that switches nothing on, too
        TRY(check_gate(c, g, who));
        if ((flags & OFK_LK_GET_MIN_EIGENVALS) && g->err_max != 0.0)
            return ofk_fail(c, OFK_E_INVALID, "%s: err_max with OFK_LK_GET_MIN_EIGENVALS: err is no residual then", who);
    }
    const bool lit = light && light->mode != OFK_LIGHT_OFF;
    if (lit) TRY(check_light(c, light, who));
    const ofk_lk_light lt = lit ? *light : ofk_lk_light{OFK_LIGHT_OFF, 4.0};
    const bool gated = g && gate_on(*g);
    const bool seeded = (flags & OFK_LK_USE_INITIAL_FLOW) != 0;
    if (seeded) {
        if (!init_pts) return ofk_fail(c, OFK_E_INVALID, "%s: OFK_LK_USE_INITIAL_FLOW needs init_pts", who);
        for (int b = 0; b < batch; ++b)
            for (int i = 0; i < 2 * counts[b]; ++i) {
                const float v = init_pts[(size_t)b * pts_stride * 2 + i];
                if (!(fabsf(v) <= 1e6f)) return ofk_fail(c, OFK_E_INVALID, "%s: init_pts[%d][%d] = %g is not a finite coordinate within 1e6", who, b, i / 2, (double)v);
            }
    }
    if (gated) TRY(gate_alloc(c));                               // behind every refusal
    const size_t px = (size_t)h * w;
    const ofk_levels lv = ofk_make_levels(h, w, win, max_level);
    TRY(h2d(c, c->pyr[0], c->pyr_stride, prev, px, batch));
    TRY(h2d(c, c->pyr[1], c->pyr_stride, next, px, batch));
    TRY(h2d(c, c->pts_prev, (size_t)c->max_pts * 8, prev_pts, (size_t)pts_stride * 8, batch));
    if (seeded) TRY(h2d(c, c->pts_next, (size_t)c->max_pts * 8, init_pts, (size_t)pts_stride * 8, batch));   // in/out, as cv2's nextPts
    OFK_HIP(c, hipMemcpyAsync(c->counts, counts, (size_t)batch * 4, hipMemcpyHostToDevice, c->stream));
    build_pyramids(c, c->stream, c->pyr[0], c->pyr[1], lv, batch);
    launch_lk(c->stream, c->pyr[0], c->pyr[1], c->pyr_stride, lv, c->pts_prev, c->counts, c->max_pts, win, max_count, eps,
              min_eig_thr, c->pts_next, c->status, c->err, batch, flags, lt);
    if (gated) {
        TRY(gate_tracks(c, c->stream, view_of(c, 0, batch, 0), lv, win, max_level, max_count, eps, min_eig_thr, *g, lt));
        c->gate_batch = batch; c->gate_fb = g->fb_mode != OFK_FB_OFF;
    }
    TRY(check_launch(c, "k_lk"));
    if (gated && g->fb_mode != OFK_FB_OFF) {
        if (back_pts) OFK_HIP(c, hipMemcpy2DAsync(back_pts, (size_t)pts_stride * 8, c->pts_back, (size_t)c->max_pts * 8, (size_t)pts_stride * 8, batch,
                                                  hipMemcpyDeviceToHost, c->stream));
        if (back_status) OFK_HIP(c, hipMemcpy2DAsync(back_status, pts_stride, c->status_back, c->max_pts, pts_stride, batch, hipMemcpyDeviceToHost, c->stream));
        if (fb2) OFK_HIP(c, hipMemcpy2DAsync(fb2, (size_t)pts_stride * 4, c->fb2, (size_t)c->max_pts * 4, (size_t)pts_stride * 4, batch,
                                             hipMemcpyDeviceToHost, c->stream));
    }
    OFK_HIP(c, hipMemcpy2DAsync(next_pts, (size_t)pts_stride * 8, c->pts_next, (size_t)c->max_pts * 8, (size_t)pts_stride * 8, batch,
                                hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipMemcpy2DAsync(status, pts_stride, c->status, c->max_pts, pts_stride, batch, hipMemcpyDeviceToHost, c->stream));
    return d2h(c, err, c->err, (size_t)c->max_pts * 4, (size_t)pts_stride * 4, batch);
}

extern "C" int ofk_lk_pyr(ofk_ctx *c, const uint8_t *prev, const uint8_t *next, int batch, int h, int w, const float *prev_pts,
                          const int *counts, int pts_stride, int win, int max_level, int max_count, double eps, double min_eig_thr,
                          float *next_pts, uint8_t *status, float *err)
{
    return lk_pyr_impl(c, "ofk_lk_pyr", prev, next, batch, h, w, prev_pts, counts, pts_stride, win, max_level, max_count, eps, min_eig_thr,
                       nullptr, 0, next_pts, status, err);
}

extern "C" int ofk_lk_pyr_ex(ofk_ctx *c, const uint8_t *prev, const uint8_t *next, int batch, int h, int w, const float *prev_pts,
                             const int *counts, int pts_stride, int win, int max_level, int max_count, double eps, double min_eig_thr,
                             const float *init_pts, int flags, float *next_pts, uint8_t *status, float *err)
{
    return lk_pyr_impl(c, "ofk_lk_pyr_ex", prev, next, batch, h, w, prev_pts, counts, pts_stride, win, max_level, max_count, eps, min_eig_thr,
                       init_pts, flags, next_pts, status, err);
}

extern "C" int ofk_lk_pyr_fb(ofk_ctx *c, const uint8_t *prev, const uint8_t *next, int batch, int h, int w, const float *prev_pts,
                             const int *counts, int pts_stride, int win, int max_level, int max_count, double eps, double min_eig_thr,
                             const float *init_pts, int flags, float *next_pts, uint8_t *status, float *err, const ofk_track_gate *g,
                             float *back_pts, uint8_t *back_status, float *fb2)
{
    return lk_pyr_impl(c, "ofk_lk_pyr_fb", prev, next, batch, h, w, prev_pts, counts, pts_stride, win, max_level, max_count, eps, min_eig_thr,
                       init_pts, flags, next_pts, status, err, g, back_pts, back_status, fb2);
}

extern "C" int ofk_lk_pyr_light(ofk_ctx *c, const uint8_t *prev, const uint8_t *next, int batch, int h, int w, const float *prev_pts,
                                const int *counts, int pts_stride, int win, int max_level, int max_count, double eps, double min_eig_thr,
                                const float *init_pts, int flags, float *next_pts, uint8_t *status, float *err, const ofk_track_gate *g,
                                float *back_pts, uint8_t *back_status, float *fb2, const ofk_lk_light *light)
{
    return lk_pyr_impl(c, "ofk_lk_pyr_light", prev, next, batch, h, w, prev_pts, counts, pts_stride, win, max_level, max_count, eps, min_eig_thr,
                       init_pts, flags, next_pts, status, err, g, back_pts, back_status, fb2, light);
}

static bool seed_mode_ok(int mode) { return mode == OFK_SEED_OFF || mode == OFK_SEED_MODEL || mode == OFK_SEED_ROTATION; }

extern "C" int ofk_set_lk_seed(ofk_ctx *c, int mode, double gain)
{
    if (!c) return OFK_E_INVALID;
    if (!seed_mode_ok(mode)) return ofk_fail(c, OFK_E_INVALID, "ofk_set_lk_seed: mode %d is none of OFK_SEED_OFF, _MODEL, _ROTATION", mode);
    if (!(fabs(gain) <= 1e12)) return ofk_fail(c, OFK_E_INVALID, "ofk_set_lk_seed: gain %g is not finite", gain);
    c->lk_seed_mode = mode; c->lk_seed_gain = gain;
    return OFK_OK;
}

extern "C" int ofk_get_lk_seed(const ofk_ctx *c, int *mode, double *gain)
{
    if (!c) return OFK_E_INVALID;
    if (mode) *mode = c->lk_seed_mode;
    if (gain) *gain = c->lk_seed_gain;
    return OFK_OK;
}

// ------------------------------------------------------------------------------------------------ robust solve setting
static int check_robust(ofk_ctx *c, const ofk_robust *r, const char *who)
{
    if (r->loss != OFK_ROBUST_HUBER && r->loss != OFK_ROBUST_TUKEY) return ofk_fail(c, OFK_E_INVALID, "%s: loss %d is neither OFK_ROBUST_HUBER nor _TUKEY", who, r->loss);
    if (!(std::isfinite(r->c) && r->c > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: c = %g must be finite and positive", who, r->c);
    if (r->iters < 0 || r->iters > 32) return ofk_fail(c, OFK_E_INVALID, "%s: iters %d outside 0..32", who, r->iters);
    if (r->hypotheses < 0 || r->hypotheses > 256) return ofk_fail(c, OFK_E_INVALID, "%s: hypotheses %d outside 0..256", who, r->hypotheses);
    if (r->drop != 0 && r->drop != 1) return ofk_fail(c, OFK_E_INVALID, "%s: drop %d is neither 0 nor 1", who, r->drop);
    return OFK_OK;
}

extern "C" int ofk_set_robust(ofk_ctx *c, const ofk_robust *r)
{
    return setting_set(c, &ofk_ctx::robust, r && r->loss == OFK_ROBUST_OFF ? nullptr : r, [](ofk_robust &s) { s.loss = OFK_ROBUST_OFF; },
                       [c](const ofk_robust *v) { return check_robust(c, v, "ofk_set_robust"); });
}
extern "C" int ofk_get_robust(const ofk_ctx *c, ofk_robust *r) { return setting_get(c, &ofk_ctx::robust, r); }

// the resident buffers of the robust solve, allocated when a run first needs them
static int robust_alloc(ofk_ctx *c)
{
    if (c->rob_work) return OFK_OK;                              // one allocation, carved into the four buffers: all of them or none
    const size_t B = (size_t)c->max_batch, np = B * c->max_pts;
    double *base = nullptr;
    OFK_HIP(c, hipMalloc((void **)&base, (np * 9 + B * OFK_ROBUST_DOUBLES) * 8));
    c->rob_work = base; c->rob_w = base + np * 7; c->rob_wtmp = base + np * 8; c->rob_stats = base + np * 9;
    return OFK_OK;
}

// ------------------------------------------------------------------------------------------------ velocity covariance setting
static int check_cov(ofk_ctx *c, const ofk_cov *v, const char *who)
{
    if (v->mode != OFK_COV_OFF && v->mode != OFK_COV_PROPAGATE && v->mode != OFK_COV_RESIDUAL)
        return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is none of OFK_COV_OFF, _PROPAGATE, _RESIDUAL", who, v->mode);
    const double vals[10] = {v->sigma_flow, v->sigma_pos, v->sigma_d, v->sigma_omega[0], v->sigma_omega[1], v->sigma_omega[2], v->sigma_normal,
                             v->sigma_offset, v->r_floor, v->nis_max};
    for (int k = 0; k < 10; ++k)
        if (!(std::isfinite(vals[k]) && vals[k] >= 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: a sigma, r_floor or nis_max is negative or not finite (%g)", who, vals[k]);
    if ((v->omega_from_imu != 0 && v->omega_from_imu != 1) || (v->filter_r != 0 && v->filter_r != 1))
        return ofk_fail(c, OFK_E_INVALID, "%s: omega_from_imu and filter_r are 0 or 1", who);
    if (v->filter_r && v->mode == OFK_COV_OFF) return ofk_fail(c, OFK_E_INVALID, "%s: filter_r needs a covariance: mode is OFK_COV_OFF", who);
    return OFK_OK;
}

extern "C" int ofk_set_cov(ofk_ctx *c, const ofk_cov *v)
{
    return setting_set(c, &ofk_ctx::cov, v, [](ofk_cov &s) { s.mode = OFK_COV_OFF; s.filter_r = 0; },      // filter_r needs a covariance
                       [c](const ofk_cov *x) { return check_cov(c, x, "ofk_set_cov"); });
}
extern "C" int ofk_get_cov(const ofk_ctx *c, ofk_cov *v) { return setting_get(c, &ofk_ctx::cov, v); }

// ------------------------------------------------------------------------------------------------ joint velocity and rotation setting
static int check_joint(ofk_ctx *c, const ofk_joint *v, const char *who)
{
    if (v->mode != OFK_JOINT_OFF && v->mode != OFK_JOINT_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_JOINT_OFF nor OFK_JOINT_ON", who, v->mode);
    if (!(std::isfinite(v->sigma_flow) && v->sigma_flow > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_flow %g is not finite or not positive", who, v->sigma_flow);
    for (int k = 0; k < 3; ++k)
        if (!(v->sigma_omega[k] >= 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_omega[%d] is negative or NaN (%g)", who, k, v->sigma_omega[k]);
    if (v->omega_from_imu != 0 && v->omega_from_imu != 1) return ofk_fail(c, OFK_E_INVALID, "%s: omega_from_imu is 0 or 1", who);
    return OFK_OK;
}

extern "C" int ofk_set_joint(ofk_ctx *c, const ofk_joint *v)
{
    return setting_set(c, &ofk_ctx::joint, v, [](ofk_joint &s) { s.mode = OFK_JOINT_OFF; }, [c](const ofk_joint *x) { return check_joint(c, x, "ofk_set_joint"); });
}
extern "C" int ofk_get_joint(const ofk_ctx *c, ofk_joint *v) { return setting_get(c, &ofk_ctx::joint, v); }

// ------------------------------------------------------------------------------------------------ plane setting
static int check_plane(ofk_ctx *c, const ofk_plane *v, const char *who)
{
    if (v->mode != OFK_PLANE_OFF && v->mode != OFK_PLANE_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_PLANE_OFF nor OFK_PLANE_ON", who, v->mode);
    if (!(std::isfinite(v->sigma_flow) && v->sigma_flow > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_flow %g is not finite or not positive", who, v->sigma_flow);
    if (!(v->sigma_normal >= 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_normal is negative or NaN (%g)", who, v->sigma_normal);
    if (!(v->sigma_max > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_max is not positive or NaN (%g)", who, v->sigma_max);
    const double bb = v->beam[0] * v->beam[0] + v->beam[1] * v->beam[1] + v->beam[2] * v->beam[2];
    if (!(std::isfinite(v->beam[0]) && std::isfinite(v->beam[1]) && std::isfinite(v->beam[2]) && std::isfinite(bb) && bb > 0.0))
        return ofk_fail(c, OFK_E_INVALID, "%s: the beam (%g, %g, %g) has no length or is not finite", who, v->beam[0], v->beam[1], v->beam[2]);
    if (v->iters < 1 || v->iters > 16) return ofk_fail(c, OFK_E_INVALID, "%s: iters %d is outside 1..16", who, v->iters);
    return OFK_OK;
}

extern "C" int ofk_set_plane(ofk_ctx *c, const ofk_plane *v)
{
    return setting_set(c, &ofk_ctx::plane, v, [](ofk_plane &s) { s.mode = OFK_PLANE_OFF; }, [c](const ofk_plane *x) { return check_plane(c, x, "ofk_set_plane"); });
}
extern "C" int ofk_get_plane(const ofk_ctx *c, ofk_plane *v) { return setting_get(c, &ofk_ctx::plane, v); }

// ------------------------------------------------------------------------------------------------ epipolar setting
static int check_epipolar(ofk_ctx *c, const ofk_epipolar *v, const char *who)
{
    if (v->mode != OFK_EPI_OFF && v->mode != OFK_EPI_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_EPI_OFF nor OFK_EPI_ON", who, v->mode);
    if (v->weights != OFK_EPI_W_ONE && v->weights != OFK_EPI_W_ROBUST)
        return ofk_fail(c, OFK_E_INVALID, "%s: weights %d is neither OFK_EPI_W_ONE nor OFK_EPI_W_ROBUST", who, v->weights);
    if (!(v->anchor > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: anchor is not positive or NaN (%g)", who, v->anchor);
    if (v->anchor_min < 1) return ofk_fail(c, OFK_E_INVALID, "%s: anchor_min %d is below 1", who, v->anchor_min);
    if (!(v->sigma_max > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_max is not positive or NaN (%g)", who, v->sigma_max);
    const double bb = v->beam[0] * v->beam[0] + v->beam[1] * v->beam[1] + v->beam[2] * v->beam[2];
    if (!(std::isfinite(v->beam[0]) && std::isfinite(v->beam[1]) && std::isfinite(v->beam[2]) && std::isfinite(bb) && bb > 0.0))
        return ofk_fail(c, OFK_E_INVALID, "%s: the beam (%g, %g, %g) has no length or is not finite", who, v->beam[0], v->beam[1], v->beam[2]);
    return OFK_OK;
}

extern "C" int ofk_set_epipolar(ofk_ctx *c, const ofk_epipolar *v)
{
    return setting_set(c, &ofk_ctx::epi, v, [](ofk_epipolar &s) { s.mode = OFK_EPI_OFF; }, [c](const ofk_epipolar *x) { return check_epipolar(c, x, "ofk_set_epipolar"); });
}
extern "C" int ofk_get_epipolar(const ofk_ctx *c, ofk_epipolar *v) { return setting_get(c, &ofk_ctx::epi, v); }

// ------------------------------------------------------------------------------------------------ gyro bias setting
static int check_bias(ofk_ctx *c, const ofk_gyro_bias *v, const char *who)
{
    if (v->mode != OFK_BIAS_OFF && v->mode != OFK_BIAS_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_BIAS_OFF nor OFK_BIAS_ON", who, v->mode);
    if (!(std::isfinite(v->sigma_flow) && v->sigma_flow > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_flow %g is not finite or not positive", who, v->sigma_flow);
    if (!(std::isfinite(v->sigma_gyro) && v->sigma_gyro >= 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_gyro %g is not finite or negative", who, v->sigma_gyro);
    if (!(std::isfinite(v->q) && v->q >= 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: q %g is not finite or negative", who, v->q);
    if (!(std::isfinite(v->nis_max) && v->nis_max >= 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: nis_max %g is not finite or negative", who, v->nis_max);
    for (int k = 0; k < 3; ++k) {
        if (!(std::isfinite(v->p0[k]) && v->p0[k] >= 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: p0[%d] is not finite or negative (%g)", who, k, v->p0[k]);
        if (!std::isfinite(v->p0[k] * v->p0[k])) return ofk_fail(c, OFK_E_INVALID, "%s: the square of p0[%d] is not finite (%g)", who, k, v->p0[k]);
        if (!std::isfinite(v->b0[k])) return ofk_fail(c, OFK_E_INVALID, "%s: b0[%d] is not finite (%g)", who, k, v->b0[k]);
    }
    if (v->update != 0 && v->update != 1) return ofk_fail(c, OFK_E_INVALID, "%s: update is 0 or 1", who);
    return OFK_OK;
}

static bool bias_on(const ofk_ctx *c) { return c->bias.mode != OFK_BIAS_OFF; }
static bool bias_estimates(const ofk_gyro_bias &g) { return g.update && (g.p0[0] > 0.0 || g.p0[1] > 0.0 || g.p0[2] > 0.0); }

extern "C" int ofk_set_gyro_bias(ofk_ctx *c, const ofk_gyro_bias *v)
{
    TRY(setting_set(c, &ofk_ctx::bias, v && v->mode == OFK_BIAS_OFF ? nullptr : v, [](ofk_gyro_bias &s) { s.mode = OFK_BIAS_OFF; },
                    [c](const ofk_gyro_bias *x) { return check_bias(c, x, "ofk_set_gyro_bias"); }));
    c->bias_fresh = 1; c->bias_batch = 0;                        // the state is (b0, diag(p0^2)) again, set when a step or a reset first needs it
    return OFK_OK;
}
extern "C" int ofk_get_gyro_bias(const ofk_ctx *c, ofk_gyro_bias *v) { return setting_get(c, &ofk_ctx::bias, v); }

// one stream's state from a setting: b0, diag(p0^2), everything else 0
static void bias_state_of(const ofk_gyro_bias &g, double *r)
{
    for (int k = 0; k < OFK_BIAS_DOUBLES; ++k) r[k] = 0.0;
    for (int k = 0; k < 3; ++k) r[k] = g.b0[k];
    r[3] = g.p0[0] * g.p0[0]; r[6] = g.p0[1] * g.p0[1]; r[8] = g.p0[2] * g.p0[2];
}

// the streams' rows, allocated on first use, and the state of the setting where it is still to be set
static int bias_prepare(ofk_ctx *c)
{
    if (!c->bias_rec) { OFK_HIP(c, hipMalloc((void **)&c->bias_rec, (size_t)c->max_batch * OFK_BIAS_DOUBLES * 8)); c->bias_fresh = 1; }
    if (!c->bias_fresh) return OFK_OK;
    double row[OFK_BIAS_DOUBLES];
    bias_state_of(c->bias, row);
    for (int b = 0; b < c->max_batch; ++b)
        OFK_HIP(c, hipMemcpyAsync(c->bias_rec + (size_t)b * OFK_BIAS_DOUBLES, row, sizeof row, hipMemcpyHostToDevice, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    c->bias_fresh = 0;
    return OFK_OK;
}

extern "C" int ofk_gyro_bias_reset(ofk_ctx *c, const double *state, int batch)
{
    if (!c || !state || batch < 1 || batch > c->max_batch) return ofk_fail(c, OFK_E_INVALID, "ofk_gyro_bias_reset: bad argument");
    if (!bias_on(c)) return ofk_fail(c, OFK_E_INVALID, "ofk_gyro_bias_reset: ofk_set_gyro_bias is off");
    for (size_t k = 0; k < (size_t)batch * 9; ++k)
        if (!std::isfinite(state[k])) return ofk_fail(c, OFK_E_INVALID, "ofk_gyro_bias_reset: a state value is not finite");
    TRY(enter(c));
    TRY(bias_prepare(c));
    double *rows = (double *)calloc((size_t)batch * OFK_BIAS_DOUBLES, 8);
    if (!rows) return ofk_fail(c, OFK_E_INVALID, "out of host memory");
    for (int b = 0; b < batch; ++b) memcpy(rows + (size_t)b * OFK_BIAS_DOUBLES, state + (size_t)b * 9, 9 * 8);
    const hipError_t e = hipMemcpy(c->bias_rec, rows, (size_t)batch * OFK_BIAS_DOUBLES * 8, hipMemcpyHostToDevice);
    free(rows);
    OFK_HIP(c, e);
    return OFK_OK;
}

extern "C" int ofk_gyro_bias_download(ofk_ctx *c, double *rec)
{
    if (!c) return OFK_E_INVALID;
    if (c->bias_batch < 1 || !c->bias_rec) return ofk_fail(c, OFK_E_INVALID, "ofk_gyro_bias_download: no step with ofk_set_gyro_bias on yet");
    if (!rec) return ofk_fail(c, OFK_E_INVALID, "ofk_gyro_bias_download: NULL buffer");
    TRY(enter(c));
    OFK_HIP(c, hipMemcpyAsync(rec, c->bias_rec, (size_t)c->bias_batch * OFK_BIAS_DOUBLES * 8, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

// The steps' own refusals with the setting on and updating (ofk.h), then the rows; fu: a fused step's.
static int bias_check_step(ofk_ctx *c, int B, int variant, const ofk_fusion *fu, const char *who)
{
    if (!bias_on(c)) return OFK_OK;
    if (c->bias.update && (variant == OFK_SOLVE_OFMODULE || (fu && (fu->flow == OFK_FLOW_ROTATIONAL || fu->keep == OFK_KEEP_LEGACY))))
        return refuse_not_sensor_model(c, who, NO_OFMODULE | NO_ROTATIONAL | NO_LEGACY, "gyro bias update", "ofk_set_gyro_bias");
    TRY(bias_prepare(c));
    c->bias_batch = B;
    return OFK_OK;
}

// ------------------------------------------------------------------------------------------------ the second-stage settings
// One row per setting whose kernel runs behind the velocity solve, in the order of their checks and launches.  No two run together:
// a row refuses every earlier row that is on.
struct second_setting {
    const char *set, *what;                                     // the setter's name, what the kernel adds
    int (*mode)(const ofk_ctx *);                               // 0: off
    double *ofk_ctx::*rec; int doubles; int ofk_ctx::*batch;    // the records' rows (allocated on first use), problems of the latest run / step
    double *ofk_ctx::*pts;                                      // [max_pts][4] per problem behind the rows, or NULL
    const char *beside;                                         // the refusal beside an earlier row: who, that row's setter
    int fused_refuse;                                           // what a fused step may not have: not the sensor model
    bool ofmodule_late;                                         // OFK_SOLVE_OFMODULE is refused behind `beside`, in words of its own
    void (*pairs)(ofk_ctx *, hipStream_t, const ofk_pairs_in &, const double *weights, int b0);
    void (*stream)(ofk_ctx *, const ofk_stream_in &, const double *weights);
};
enum { SECOND_COV, SECOND_JOINT, SECOND_PLANE, SECOND_EPI };
static const second_setting SECOND[4] = {
    {"ofk_set_cov", "covariance", [](const ofk_ctx *c) { return c->cov.mode; }, &ofk_ctx::cov_rec, OFK_COV_DOUBLES, &ofk_ctx::cov_batch, nullptr,
     nullptr, NO_OFMODULE | NO_ROTATIONAL, false,
     [](ofk_ctx *c, hipStream_t st, const ofk_pairs_in &in, const double *w, int b0) {
         ofk_launch_pairs_cov(st, in, w, &c->cov, c->cov_rec + (size_t)b0 * OFK_COV_DOUBLES); },
     [](ofk_ctx *c, const ofk_stream_in &in, const double *w) { ofk_launch_stream_cov(c->stream, in, w, &c->cov, c->cov_rec); }},
    {"ofk_set_joint", "joint solve", [](const ofk_ctx *c) { return c->joint.mode; }, &ofk_ctx::joint_rec, OFK_JOINT_DOUBLES, &ofk_ctx::joint_batch,
     nullptr, "%s: ofk_set_joint and %s are both on: the covariance takes omega as an input, not an estimate",
     NO_OFMODULE | NO_ROTATIONAL | NO_LEGACY, false,
     [](ofk_ctx *c, hipStream_t st, const ofk_pairs_in &in, const double *w, int b0) {
         ofk_launch_pairs_joint(st, in, w, &c->joint, c->joint_rec + (size_t)b0 * OFK_JOINT_DOUBLES); },
     [](ofk_ctx *c, const ofk_stream_in &in, const double *w) { ofk_launch_stream_joint(c->stream, in, w, &c->joint, c->joint_rec); }},
    {"ofk_set_plane", "plane solve", [](const ofk_ctx *c) { return c->plane.mode; }, &ofk_ctx::plane_rec, OFK_PLANE_DOUBLES, &ofk_ctx::plane_batch,
     nullptr, "%s: ofk_set_plane is on beside %s: both take the normal as an input, not an estimate", NO_ROTATIONAL | NO_LEGACY, true,
     [](ofk_ctx *c, hipStream_t st, const ofk_pairs_in &in, const double *w, int b0) {
         ofk_launch_pairs_plane(st, in, w, &c->plane, c->plane_rec + (size_t)b0 * OFK_PLANE_DOUBLES); },
     [](ofk_ctx *c, const ofk_stream_in &in, const double *w) { ofk_launch_stream_plane(c->stream, in, w, &c->plane, c->plane_rec); }},
    {"ofk_set_epipolar", "epipolar solve", [](const ofk_ctx *c) { return c->epi.mode; }, &ofk_ctx::epi_rec, OFK_EPI_DOUBLES, &ofk_ctx::epi_batch,
     &ofk_ctx::epi_pts, "%s: ofk_set_epipolar is on beside %s: that setting rests on the plane this one replaces", NO_ROTATIONAL | NO_LEGACY, true,
     [](ofk_ctx *c, hipStream_t st, const ofk_pairs_in &in, const double *w, int b0) {
         ofk_launch_pairs_epi(st, in, w, &c->epi, c->epi_rec + (size_t)b0 * OFK_EPI_DOUBLES, c->epi_pts + (size_t)b0 * c->max_pts * 4); },
     [](ofk_ctx *c, const ofk_stream_in &in, const double *w) { ofk_launch_stream_epi(c->stream, in, w, &c->epi, c->epi_rec, c->epi_pts); }},
};

static bool second_on(const ofk_ctx *c)
{
    for (const second_setting &s : SECOND) if (s.mode(c)) return true;
    return false;
}

// The runs' and steps' own refusals with a setting on (ofk.h), row by row; allocates the rows on first use.  fu: a fused step's.
static int second_prepare(ofk_ctx *c, int B, int variant, const ofk_fusion *fu, const char *who)
{
    const int has = !fu ? 0 : (variant == OFK_SOLVE_OFMODULE ? NO_OFMODULE : 0) | (fu->flow == OFK_FLOW_ROTATIONAL ? NO_ROTATIONAL : 0) |
                                  (fu->keep == OFK_KEEP_LEGACY ? NO_LEGACY : 0);
    const second_setting *first = nullptr;                      // the row that is on already
    for (const second_setting &s : SECOND) {
        if (!s.mode(c)) continue;
        if (has & s.fused_refuse) return refuse_not_sensor_model(c, who, s.fused_refuse, s.what, s.set);
        if (first) return ofk_fail(c, OFK_E_INVALID, s.beside, who, first->set);
        if (s.ofmodule_late && variant == OFK_SOLVE_OFMODULE)
            return ofk_fail(c, OFK_E_INVALID, "%s: OFK_SOLVE_OFMODULE is not the sensor model: no %s (%s is on)", who, s.what, s.set);
        if (!(c->*s.rec)) {
            const size_t rows = (size_t)c->max_batch * s.doubles;
            OFK_HIP(c, hipMalloc((void **)&(c->*s.rec), rows * 8 + (s.pts ? (size_t)c->max_batch * c->max_pts * 32 : 0)));
            if (s.pts) c->*s.pts = c->*s.rec + rows;
        }
        c->*s.batch = B;
        first = &s;
    }
    return OFK_OK;
}

// A setting's rows of the latest run or step (points: its per-point rows) to the host.
static int second_download(ofk_ctx *c, const second_setting &s, const char *who, double *dst, bool points = false)
{
    if (!c) return OFK_E_INVALID;
    if (c->*s.batch < 1 || !(c->*s.rec)) return ofk_fail(c, OFK_E_INVALID, "%s: no run or step with %s on yet", who, s.set);
    if (!dst) return ofk_fail(c, OFK_E_INVALID, "%s: NULL buffer", who);
    TRY(enter(c));
    const size_t per = points ? (size_t)c->max_pts * 32 : (size_t)s.doubles * 8;
    OFK_HIP(c, hipMemcpyAsync(dst, points ? c->*s.pts : c->*s.rec, (size_t)(c->*s.batch) * per, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

extern "C" int ofk_cov_download(ofk_ctx *c, double *cov) { return second_download(c, SECOND[SECOND_COV], "ofk_cov_download", cov); }
extern "C" int ofk_joint_download(ofk_ctx *c, double *joint) { return second_download(c, SECOND[SECOND_JOINT], "ofk_joint_download", joint); }
extern "C" int ofk_plane_download(ofk_ctx *c, double *plane) { return second_download(c, SECOND[SECOND_PLANE], "ofk_plane_download", plane); }
extern "C" int ofk_epipolar_download(ofk_ctx *c, double *epi) { return second_download(c, SECOND[SECOND_EPI], "ofk_epipolar_download", epi); }
extern "C" int ofk_epipolar_points_download(ofk_ctx *c, double *points)
{
    return second_download(c, SECOND[SECOND_EPI], "ofk_epipolar_points_download", points, true);
}

// The solve of nb pairs from pair b0 on (their views' pointers): the plain kernels, or with ofk_set_robust on the robust ones, and
// behind either the kernel of the second-stage setting that is on.
// drop_status: the stream steps' keep flags (cleared for zero-weight points when the setting asks for it), NULL for frame pairs.
static void solve_pairs(ofk_ctx *c, hipStream_t st, const float *pts_prev, const float *pts_next, uint8_t *status, const int *counts,
                        const double *sensors, const ofk_params *p, const int *cand_count, double *records, int b0, int nb, bool stream)
{
    const size_t o = (size_t)b0 * c->max_pts;
    const bool rob = c->robust.loss != OFK_ROBUST_OFF;
    if (rob)
        ofk_launch_pairs_robust(st, pts_prev, pts_next, status, counts, c->max_pts, sensors, p->solve_variant, p->use_feasibility, p->feas_T,
                                cand_count, &c->robust, b0, c->rob_work + o * 7, c->rob_w + o, c->rob_wtmp + o,
                                c->rob_stats + (size_t)b0 * OFK_ROBUST_DOUBLES, stream && c->robust.drop ? status : nullptr, records, nb);
    else
        ofk_launch_pairs_solve(st, pts_prev, pts_next, status, counts, c->max_pts, sensors, p->solve_variant, p->use_feasibility, p->feas_T,
                               cand_count, records, nb);
    if (stream && bias_on(c) && bias_estimates(c->bias)) {       // the gyro bias's filter step: the record still holds the solve's own v
        static const ofk_fusion none = {};
        const ofk_stream_in bin = {pts_prev, pts_next, status, counts, c->max_pts, sensors, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, &none,
                                   p->solve_variant, records, nullptr, nb, 0};
        ofk_launch_stream_bias(st, bin, 0, p->use_feasibility, p->feas_T, rob ? c->rob_w + o : nullptr, &c->bias,
                               c->bias_rec + (size_t)b0 * OFK_BIAS_DOUBLES);
    }
    const ofk_pairs_in in = {pts_prev, pts_next, status, counts, c->max_pts, sensors, p->solve_variant, p->use_feasibility, p->feas_T, records, nb};
    for (const second_setting &s : SECOND) if (s.mode(c)) s.pairs(c, st, in, rob ? c->rob_w + o : nullptr, b0);
}

extern "C" int ofk_robust_download(ofk_ctx *c, double *weights, int stride, double *stats)
{
    if (!c) return OFK_E_INVALID;
    if (c->rob_batch < 1 || !c->rob_work) return ofk_fail(c, OFK_E_INVALID, "ofk_robust_download: no run or step with ofk_set_robust on yet");
    if (weights && stride < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_robust_download: stride %d", stride);
    TRY(enter(c));
    const int B = c->rob_batch;
    if (weights) {
        const size_t wb = (size_t)(stride < c->max_pts ? stride : c->max_pts) * 8;
        OFK_HIP(c, hipMemcpy2DAsync(weights, (size_t)stride * 8, c->rob_w, (size_t)c->max_pts * 8, wb, B, hipMemcpyDeviceToHost, c->stream));
    }
    if (stats) OFK_HIP(c, hipMemcpyAsync(stats, c->rob_stats, (size_t)B * OFK_ROBUST_DOUBLES * 8, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

static void philox4x32_10_host(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4])
{
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// host only: the two kept-point numbers of every hypothesis, as the kernels draw them (k_robust.inc)
extern "C" int ofk_robust_pairs(unsigned long long seed, unsigned problem, int hypotheses, int m, int *i, int *j)
{
    if (hypotheses < 0 || hypotheses > 256 || m < 2 || (hypotheses > 0 && (!i || !j))) return OFK_E_INVALID;
    for (int h = 0; h < hypotheses; ++h) {
        unsigned x[4];
        philox4x32_10_host((unsigned)h, problem, 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32), x);
        i[h] = (int)(x[0] % (unsigned)m);
        j[h] = (int)(x[1] % (unsigned)(m - 1));
        j[h] += j[h] >= i[h] ? 1 : 0;
    }
    return OFK_OK;
}

// the predictor on host buffers; device scratch only, so resident points, sensors and filter states are not touched
extern "C" int ofk_predict_points(ofk_ctx *c, const float *pts, const int *counts, int batch, int stride, const double *sensors, int mode,
                                  double gain, float *seed_out)
{
    if (!c || !pts || !counts || !sensors || !seed_out || batch < 1 || stride < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_predict_points: bad argument");
    if (mode != OFK_SEED_MODEL && mode != OFK_SEED_ROTATION) return ofk_fail(c, OFK_E_INVALID, "ofk_predict_points: mode must be OFK_SEED_MODEL or OFK_SEED_ROTATION");
    for (int b = 0; b < batch; ++b)
        if (counts[b] < 0 || counts[b] > stride) return ofk_fail(c, OFK_E_INVALID, "counts[%d]=%d outside 0..%d", b, counts[b], stride);
    TRY(enter(c));
    const size_t pb = up((size_t)batch * stride * 8, 256), cb = up((size_t)batch * 4, 256), sb = up((size_t)batch * OFK_SENSOR_DOUBLES * 8, 256);
    TRY(ofk_need_scratch(c, 2 * pb + cb + sb));
    char *base = (char *)c->scratch;
    float *dp = (float *)base, *ds = (float *)(base + pb);
    int *dc = (int *)(base + 2 * pb);
    double *dsn = (double *)(base + 2 * pb + cb);
    OFK_HIP(c, hipMemcpyAsync(dp, pts, (size_t)batch * stride * 8, hipMemcpyHostToDevice, c->stream));
    OFK_HIP(c, hipMemcpyAsync(ds, pts, (size_t)batch * stride * 8, hipMemcpyHostToDevice, c->stream));     // entries beyond counts[b]: the points
    OFK_HIP(c, hipMemcpyAsync(dc, counts, (size_t)batch * 4, hipMemcpyHostToDevice, c->stream));
    OFK_HIP(c, hipMemcpyAsync(dsn, sensors, (size_t)batch * OFK_SENSOR_DOUBLES * 8, hipMemcpyHostToDevice, c->stream));
    ofk_launch_seed_points(c->stream, dp, dc, stride, dsn, nullptr, mode, gain, ds, batch);
    TRY(check_launch(c, "k_seed_points"));
    OFK_HIP(c, hipMemcpyAsync(seed_out, ds, (size_t)batch * stride * 8, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

// levels 1..L of a batch of gray images, built exactly as ofk_lk_pyr / ofk_pairs_run build them (three levels per pass where the
// geometry allows it); out = per image the levels 1..L back to back, tightly packed
extern "C" int ofk_pyramid_u8(ofk_ctx *c, const uint8_t *gray, int batch, int h, int w, int max_level, uint8_t *out, int *levels_built)
{
    TRY(check_geom(c, batch, h, w, "ofk_pyramid_u8"));
    if (!gray || !out) return ofk_fail(c, OFK_E_INVALID, "ofk_pyramid_u8: NULL buffer");
    if (max_level < 0 || max_level > c->max_level) return ofk_fail(c, OFK_E_INVALID, "max_level %d outside 0..%d", max_level, c->max_level);
    const ofk_levels lv = ofk_make_levels(h, w, 0, max_level);
    TRY(h2d(c, c->pyr[0], c->pyr_stride, gray, (size_t)h * w, batch));
    build_pyramids(c, c->stream, c->pyr[0], nullptr, lv, batch);
    TRY(check_launch(c, "pyramid"));
    size_t total = 0, o = 0;
    for (int l = 1; l <= lv.n; ++l) total += (size_t)lv.h[l] * lv.w[l];
    for (int l = 1; l <= lv.n; ++l) {
        const size_t px = (size_t)lv.h[l] * lv.w[l];
        OFK_HIP(c, hipMemcpy2DAsync(out + o, total, c->pyr[0] + lv.off[l], c->pyr_stride, px, batch, hipMemcpyDeviceToHost, c->stream));
        o += px;
    }
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    if (levels_built) *levels_built = lv.n;
    return OFK_OK;
}

// ------------------------------------------------------------------------------------------------ estimation entry points
struct Bump {                                               // carves device scratch and uploads host arrays
    ofk_ctx *c; char *base; size_t off; int rc;
    double *put(const void *host, size_t bytes)
    {
        if (!host) return nullptr;
        char *p = base + off;
        off += up(bytes, 256);
        if (rc == OFK_OK && hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = OFK_E_HIP;
        return (double *)p;
    }
    double *take(size_t bytes) { char *p = base + off; off += up(bytes, 256); return (double *)p; }
};
static int get(ofk_ctx *c, void *host, const void *dev, size_t bytes)
{
    OFK_HIP(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}
static bool all_finite(const double *a, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}
static int est_begin(ofk_ctx *c, size_t bytes, Bump &bp)
{
    if (!c) return OFK_E_INVALID;
    TRY(enter(c));
    TRY(ofk_need_scratch(c, bytes + 64 * 256));
    bp.c = c; bp.base = (char *)c->scratch; bp.off = 0; bp.rc = OFK_OK;
    return OFK_OK;
}

extern "C" int ofk_flow_model(ofk_ctx *c, const double *x, int batch, int n, const double *v, const double *omega, const double *d,
                              const double *nrm, const double *t, double *flow)
{
    if (!c || !x || !v || !omega || !d || !nrm || !flow || batch < 1 || n < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_flow_model: bad argument");
    const size_t pb = (size_t)batch * n * 16;
    Bump bp;
    TRY(est_begin(c, 2 * pb + (size_t)batch * 256 * 5, bp));
    double *dx = bp.put(x, pb), *dv = bp.put(v, batch * 24), *dom = bp.put(omega, batch * 24), *dd = bp.put(d, batch * 8),
           *dn = bp.put(nrm, batch * 24), *dt = bp.put(t, batch * 24), *df = bp.take(pb);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_flow_model: upload failed");
    ofk_launch_flow_model(c->stream, dx, batch, n, dv, dom, dd, dn, dt, df);
    TRY(check_launch(c, "k_flow_model"));
    return get(c, flow, df, pb);
}

extern "C" int ofk_feasibility(ofk_ctx *c, int variant, const double *x, const double *u, int batch, int n, const double *nrm,
                               const double *v, const double *dist, const double *omega, const double *t, double *r, double *dd)
{
    if (!c || !x || !u || !nrm || !v || !r || !dd || batch < 1 || n < 1 || variant < 0 || variant > 2)
        return ofk_fail(c, OFK_E_INVALID, "ofk_feasibility: bad argument");
    if (variant == OFK_FEAS_RTILDE && !dist) return ofk_fail(c, OFK_E_INVALID, "ofk_feasibility: dist required");
    if (variant == OFK_FEAS_SIM && (!omega || !t)) return ofk_fail(c, OFK_E_INVALID, "ofk_feasibility: omega and t required");
    const size_t pb = (size_t)batch * n * 16, rb = (size_t)batch * n * 8;
    Bump bp;
    TRY(est_begin(c, 2 * pb + 2 * rb + (size_t)batch * 256 * 5, bp));
    double *dx = bp.put(x, pb), *du = bp.put(u, pb), *dn = bp.put(nrm, batch * 24), *dv = bp.put(v, batch * 24),
           *ddist = bp.put(dist, batch * 8), *dom = bp.put(omega, batch * 24), *dt = bp.put(t, batch * 24), *dr = bp.take(rb),
           *ddd = bp.take(rb);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_feasibility: upload failed");
    ofk_launch_feasibility(c->stream, variant, dx, du, batch, n, dn, dv, ddist, dom, dt, dr, ddd);
    TRY(check_launch(c, "k_feasibility"));
    TRY(get(c, r, dr, rb));
    return get(c, dd, ddd, rb);
}

extern "C" int ofk_velocity_solve(ofk_ctx *c, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                                  const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                                  double *out)
{
    if (!c || !x || !u || !nrm || !out || batch < 1 || n < 1 || variant < 0 || variant > 2)
        return ofk_fail(c, OFK_E_INVALID, "ofk_velocity_solve: bad argument");
    if (variant == OFK_SOLVE_OFMODULE ? !wgt : (!d || !omega)) return ofk_fail(c, OFK_E_INVALID, "ofk_velocity_solve: missing input for variant %d", variant);
    const size_t pb = (size_t)batch * n * 16;
    Bump bp;
    TRY(est_begin(c, 2 * pb + (size_t)batch * n * 9 + (size_t)batch * 256 * 6, bp));
    double *dx = bp.put(x, pb), *du = bp.put(u, pb);
    uint8_t *dval = (uint8_t *)bp.put(valid, (size_t)batch * n);
    double *dd = bp.put(d, batch * 8), *dn = bp.put(nrm, batch * 24), *dom = bp.put(omega, batch * 24), *dt = bp.put(t, batch * 24),
           *dw = bp.put(wgt, (size_t)batch * n * 8), *dout = bp.take((size_t)batch * OFK_SOLVE_DOUBLES * 8);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_velocity_solve: upload failed");
    ofk_launch_solve(c->stream, variant, dx, du, dval, batch, n, dd, dn, dom, dt, dw, dout);
    TRY(check_launch(c, "k_solve"));
    return get(c, out, dout, (size_t)batch * OFK_SOLVE_DOUBLES * 8);
}

extern "C" int ofk_velocity_solve_robust(ofk_ctx *c, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                                         const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                                         const ofk_robust *r, double *out, double *weights, double *stats)
{
    if (!c || !x || !u || !nrm || !out || !r || batch < 1 || n < 1 || n > 4096 || variant < 0 || variant > 2)
        return ofk_fail(c, OFK_E_INVALID, "ofk_velocity_solve_robust: bad argument");
    if (variant == OFK_SOLVE_OFMODULE ? !wgt : (!d || !omega)) return ofk_fail(c, OFK_E_INVALID, "ofk_velocity_solve_robust: missing input for variant %d", variant);
    TRY(check_robust(c, r, "ofk_velocity_solve_robust"));
    const size_t pb = (size_t)batch * n * 16, wb = (size_t)batch * n * 8;
    Bump bp;
    TRY(est_begin(c, 2 * pb + (size_t)batch * n * 9 + 9 * wb + (size_t)batch * 256 * 8, bp));
    double *dx = bp.put(x, pb), *du = bp.put(u, pb);
    uint8_t *dval = (uint8_t *)bp.put(valid, (size_t)batch * n);
    double *dd = bp.put(d, batch * 8), *dn = bp.put(nrm, batch * 24), *dom = bp.put(omega, batch * 24), *dt = bp.put(t, batch * 24),
           *dw = bp.put(wgt, wb), *dout = bp.take((size_t)batch * OFK_SOLVE_DOUBLES * 8), *dwork = bp.take(7 * wb), *dwts = bp.take(wb),
           *dtmp = bp.take(wb), *dst = bp.take((size_t)batch * OFK_ROBUST_DOUBLES * 8);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_velocity_solve_robust: upload failed");
    ofk_launch_solve_robust(c->stream, variant, dx, du, dval, batch, n, dd, dn, dom, dt, dw, r, dwork, dwts, dtmp, dst, dout);
    TRY(check_launch(c, "k_solve_robust"));
    if (weights) TRY(get(c, weights, dwts, wb));
    if (stats) TRY(get(c, stats, dst, (size_t)batch * OFK_ROBUST_DOUBLES * 8));
    return get(c, out, dout, (size_t)batch * OFK_SOLVE_DOUBLES * 8);
}

// The four second-stage stage entries: the plain or robust solve, the setting's kernel behind it.  what: what the kernel adds; have:
// the entry's own pointers are there; wgt: refused unless NULL (the entries that ignore theirs pass NULL); check: the setting's own
// check, the mode it needs included; points: the epipolar [batch][n][4], or NULL; launch(in, weights, out, rec, points) on the device.
// rec_in: the record's rows are uploaded from it (the gyro bias's state), NULL: they are the kernel's to write; before(omega, rec) on
// the device arrays in front of the solve.
template <class Check, class Before, class Launch>
static int solve_second_chain(ofk_ctx *c, const char *who, const char *what, bool have, int variant, const double *x, const double *u,
                              const uint8_t *valid, int batch, int n, const double *d, const double *nrm, const double *omega, const double *t,
                              const double *wgt, const ofk_robust *r, Check check, const double *rec_in, Before before, const char *kernel,
                              Launch launch, double *out, double *rec, int rec_doubles, double *points)
{
    if (!c || !x || !u || !nrm || !out || !have || batch < 1 || n < 1 || n > 4096 || variant < 0 || variant > 2)
        return ofk_fail(c, OFK_E_INVALID, "%s: bad argument", who);
    if (variant == OFK_SOLVE_OFMODULE) return ofk_fail(c, OFK_E_INVALID, "%s: OFK_SOLVE_OFMODULE is not the sensor model: no %s", who, what);
    if (!d || !omega) return ofk_fail(c, OFK_E_INVALID, "%s: missing input for variant %d", who, variant);
    if (wgt) return ofk_fail(c, OFK_E_INVALID, "%s: wgt must be NULL (the argument is there for the solve entries' signature; the weights are the robust setting's)", who);
    TRY(check());
    const bool rob = r && r->loss != OFK_ROBUST_OFF;
    if (rob) TRY(check_robust(c, r, who));
    const size_t pb = (size_t)batch * n * 16, wb = (size_t)batch * n * 8, ob = (size_t)batch * OFK_SOLVE_DOUBLES * 8, rb = (size_t)batch * rec_doubles * 8;
    Bump bp;
    TRY(est_begin(c, 2 * pb + (size_t)batch * n * 9 + 9 * wb + 4 * wb + (size_t)batch * 256 * 12, bp));
    double *dx = bp.put(x, pb), *du = bp.put(u, pb);
    uint8_t *dval = (uint8_t *)bp.put(valid, (size_t)batch * n);
    double *dd = bp.put(d, batch * 8), *dn = bp.put(nrm, batch * 24), *dom = bp.put(omega, batch * 24), *dt = bp.put(t, batch * 24),
           *dout = bp.take(ob), *drec = rec_in ? bp.put(rec_in, rb) : bp.take(rb), *dpt = points ? bp.take(4 * wb) : nullptr, *dwts = nullptr;
    if (rob) {
        double *dwork = bp.take(7 * wb);
        dwts = bp.take(wb);
        double *dtmp = bp.take(wb), *dst = bp.take((size_t)batch * OFK_ROBUST_DOUBLES * 8);
        if (bp.rc) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
        before(dom, drec);
        ofk_launch_solve_robust(c->stream, variant, dx, du, dval, batch, n, dd, dn, dom, dt, nullptr, r, dwork, dwts, dtmp, dst, dout);
    } else {
        if (bp.rc) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
        before(dom, drec);
        ofk_launch_solve(c->stream, variant, dx, du, dval, batch, n, dd, dn, dom, dt, nullptr, dout);
    }
    launch(ofk_stage_in{variant, dx, du, dval, batch, n, dd, dn, dom, dt}, dwts, dout, drec, dpt);
    TRY(check_launch(c, kernel));
    TRY(get(c, rec, drec, rb));
    if (points) TRY(get(c, points, dpt, 4 * wb));
    return get(c, out, dout, ob);
}

template <class Check, class Launch>
static int solve_second_impl(ofk_ctx *c, const char *who, const char *what, bool have, int variant, const double *x, const double *u,
                             const uint8_t *valid, int batch, int n, const double *d, const double *nrm, const double *omega, const double *t,
                             const double *wgt, const ofk_robust *r, Check check, const char *kernel, Launch launch, double *out, double *rec,
                             int rec_doubles, double *points)
{
    return solve_second_chain(c, who, what, have, variant, x, u, valid, batch, n, d, nrm, omega, t, wgt, r, check, nullptr, [](double *, double *) {},
                              kernel, launch, out, rec, rec_doubles, points);
}

extern "C" int ofk_velocity_solve_cov(ofk_ctx *c, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                                      const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                                      const ofk_robust *r, const ofk_cov *cv, double *out, double *cov)
{
    const char *who = "ofk_velocity_solve_cov";
    (void)wgt;
    return solve_second_impl(c, who, "covariance", cv && cov, variant, x, u, valid, batch, n, d, nrm, omega, t, nullptr, r, [&] {
        TRY(check_cov(c, cv, who));
        if (cv->mode == OFK_COV_OFF || cv->filter_r) return ofk_fail(c, OFK_E_INVALID, "%s: mode must be PROPAGATE or RESIDUAL, filter_r 0", who);
        return (int)OFK_OK;
    }, "k_cov_solve", [&](const ofk_stage_in &in, const double *w, double *dout, double *drec, double *) {
        ofk_launch_cov_solve(c->stream, in, w, cv, dout, drec);
    }, out, cov, OFK_COV_DOUBLES, nullptr);
}

extern "C" int ofk_velocity_solve_joint(ofk_ctx *c, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                                        const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                                        const ofk_robust *r, const ofk_joint *jv, double *out, double *joint)
{
    const char *who = "ofk_velocity_solve_joint";
    (void)wgt;
    return solve_second_impl(c, who, "joint solve", jv && joint, variant, x, u, valid, batch, n, d, nrm, omega, t, nullptr, r, [&] {
        TRY(check_joint(c, jv, who));
        if (jv->mode != OFK_JOINT_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode must be OFK_JOINT_ON", who);
        return (int)OFK_OK;
    }, "k_joint_solve", [&](const ofk_stage_in &in, const double *w, double *dout, double *drec, double *) {
        ofk_launch_joint_solve(c->stream, in, w, jv, dout, drec);
    }, out, joint, OFK_JOINT_DOUBLES, nullptr);
}

// One step of the gyro bias without images: the shared chain with the apply kernel in front of the solve and the state uploaded where
// the other entries take their record's rows.
extern "C" int ofk_gyro_bias_step(ofk_ctx *c, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                                  const double *d, const double *nrm, const double *omega_raw, const double *wgt, const ofk_robust *r,
                                  const ofk_gyro_bias *g, double *state, double *out)
{
    const char *who = "ofk_gyro_bias_step";
    return solve_second_chain(c, who, "gyro bias", g && state, variant, x, u, valid, batch, n, d, nrm, omega_raw, nullptr, wgt, r, [&] {
        TRY(check_bias(c, g, who));
        if (g->mode != OFK_BIAS_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode must be OFK_BIAS_ON", who);
        return (int)OFK_OK;
    }, state, [&](double *dom, double *drec) {
        ofk_launch_gyro_bias_apply(c->stream, dom, 3, nullptr, drec, batch, 0);
    }, "k_bias_solve", [&](const ofk_stage_in &in, const double *w, double *dout, double *drec, double *) {
        if (bias_estimates(*g)) ofk_launch_bias_solve(c->stream, in, w, g, dout, drec);
    }, out, state, OFK_BIAS_DOUBLES, nullptr);
}

extern "C" int ofk_velocity_solve_plane(ofk_ctx *c, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                                        const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                                        const ofk_robust *r, const ofk_plane *jv, double *out, double *plane)
{
    const char *who = "ofk_velocity_solve_plane";
    return solve_second_impl(c, who, "plane solve", jv && plane, variant, x, u, valid, batch, n, d, nrm, omega, t, wgt, r, [&] {
        TRY(check_plane(c, jv, who));
        if (jv->mode != OFK_PLANE_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode must be OFK_PLANE_ON", who);
        return (int)OFK_OK;
    }, "k_plane_solve", [&](const ofk_stage_in &in, const double *w, double *dout, double *drec, double *) {
        ofk_launch_plane_solve(c->stream, in, w, jv, dout, drec);
    }, out, plane, OFK_PLANE_DOUBLES, nullptr);
}

extern "C" int ofk_velocity_solve_epipolar(ofk_ctx *c, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                                           const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                                           const ofk_robust *r, const ofk_epipolar *ev, double *out, double *epi, double *points)
{
    const char *who = "ofk_velocity_solve_epipolar";
    return solve_second_impl(c, who, "epipolar solve", ev && epi && points, variant, x, u, valid, batch, n, d, nrm, omega, t, wgt, r, [&] {
        TRY(check_epipolar(c, ev, who));
        if (ev->mode != OFK_EPI_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode must be OFK_EPI_ON", who);
        return (int)OFK_OK;
    }, "k_epi_solve", [&](const ofk_stage_in &in, const double *w, double *dout, double *drec, double *dpt) {
        ofk_launch_epi_solve(c->stream, in, w, ev, dout, drec, dpt);
    }, out, epi, OFK_EPI_DOUBLES, points);
}

extern "C" int ofk_imu_propagate(ofk_ctx *c, double *state, const double *msg, int batch)
{
    if (!c || !state || !msg || batch < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_imu_propagate: bad argument");
    Bump bp;
    TRY(est_begin(c, (size_t)batch * (OFK_IMU_STATE + OFK_IMU_MSG) * 8, bp));
    double *ds = bp.put(state, (size_t)batch * OFK_IMU_STATE * 8), *dm = bp.put(msg, (size_t)batch * OFK_IMU_MSG * 8);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_imu_propagate: upload failed");
    ofk_launch_imu(c->stream, ds, dm, batch);
    TRY(check_launch(c, "k_imu"));
    return get(c, state, ds, (size_t)batch * OFK_IMU_STATE * 8);
}

extern "C" int ofk_post_solve(ofk_ctx *c, const double *v_obs, const double *rotation, const double *ang, const double *offset,
                              int batch, double *v_uav)
{
    if (!c || !v_obs || !rotation || !ang || !offset || !v_uav || batch < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_post_solve: bad argument");
    Bump bp;
    TRY(est_begin(c, (size_t)batch * 24 * 8, bp));
    double *dv = bp.put(v_obs, batch * 24), *dr = bp.put(rotation, batch * 72), *da = bp.put(ang, batch * 24),
           *dof = bp.put(offset, batch * 24), *dout = bp.take(batch * 24);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_post_solve: upload failed");
    ofk_launch_post_solve(c->stream, dv, dr, da, dof, batch, dout);
    TRY(check_launch(c, "k_post_solve"));
    return get(c, v_uav, dout, batch * 24);
}

extern "C" int ofk_associate_sensors(ofk_ctx *c, const double *t_img, int n_img, const double *imu_t, const double *imu_quat,
                                     const double *imu_omega, int n_imu, const double *hgt_t, const double *hgt_range, int n_hgt,
                                     double *sensors, int *imu_index, int *hgt_index)
{
    if (!c || !t_img || !imu_t || !imu_quat || !imu_omega || !hgt_t || !hgt_range || !sensors || n_img < 1 || n_imu < 1 || n_hgt < 1)
        return ofk_fail(c, OFK_E_INVALID, "ofk_associate_sensors: bad argument (every log needs at least one sample)");
    // np.argmin over distances that are all inf or NaN names no nearest sample: refused before anything is uploaded
    if (!all_finite(t_img, n_img) || !all_finite(imu_t, n_imu) || !all_finite(hgt_t, n_hgt) || !all_finite(hgt_range, n_hgt))
        return ofk_fail(c, OFK_E_INVALID, "ofk_associate_sensors: non-finite image time, sample time or range");
    Bump bp;
    TRY(est_begin(c, ((size_t)n_img * (1 + OFK_SENSOR_DOUBLES + 1) + (size_t)n_imu * 8 + (size_t)n_hgt * 2) * 8, bp));
    double *dt = bp.put(t_img, (size_t)n_img * 8), *dit = bp.put(imu_t, (size_t)n_imu * 8), *diq = bp.put(imu_quat, (size_t)n_imu * 32),
           *diw = bp.put(imu_omega, (size_t)n_imu * 24), *dht = bp.put(hgt_t, (size_t)n_hgt * 8), *dhr = bp.put(hgt_range, (size_t)n_hgt * 8),
           *ds = bp.put(sensors, (size_t)n_img * OFK_SENSOR_DOUBLES * 8);
    int *dii = (int *)bp.take((size_t)n_img * 4), *dhi = (int *)bp.take((size_t)n_img * 4);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_associate_sensors: upload failed");
    ofk_launch_associate(c->stream, dt, n_img, n_imu, dit, diq, diw, n_hgt, dht, dhr, ds, dii, dhi);
    TRY(check_launch(c, "k_associate"));
    if (imu_index) TRY(get(c, imu_index, dii, (size_t)n_img * 4));
    if (hgt_index) TRY(get(c, hgt_index, dhi, (size_t)n_img * 4));
    return get(c, sensors, ds, (size_t)n_img * OFK_SENSOR_DOUBLES * 8);
}

extern "C" int ofk_d_split(ofk_ctx *c, const double *d, const int *counts, int batch, int stride, double d_exp_err, double *sorted,
                           double *diff, int *nsplit)
{
    if (!c || !d || !counts || !sorted || !diff || !nsplit || batch < 1 || stride < 1 || stride > 4096)
        return ofk_fail(c, OFK_E_INVALID, "ofk_d_split: bad argument (stride 1..4096)");
    const size_t n = (size_t)batch * stride;
    Bump bp;
    TRY(est_begin(c, n * 24 + (size_t)batch * 8 + 1024, bp));
    double *dd = bp.put(d, n * 8);
    int *dcn = (int *)bp.put(counts, (size_t)batch * 4);
    double *ds = bp.take(n * 8), *dg = bp.take(n * 8);
    int *dn = (int *)bp.take((size_t)batch * 4);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_d_split: upload failed");
    OFK_HIP(c, hipMemsetAsync(ds, 0, n * 8, c->stream)); OFK_HIP(c, hipMemsetAsync(dg, 0, n * 8, c->stream));
    ofk_launch_d_split(c->stream, dd, dcn, batch, stride, d_exp_err, ds, dg, dn);
    TRY(check_launch(c, "k_d_split"));
    TRY(get(c, sorted, ds, n * 8)); TRY(get(c, diff, dg, n * 8));
    return get(c, nsplit, dn, (size_t)batch * 4);
}

extern "C" int ofk_feature_eval(ofk_ctx *c, const double *pos, const double *pos_err, const double *oldpos, const double *oldpos_err,
                                const int *counts, int batch, int stride, const double *vel, const double *vel_err, double focal_len,
                                double dummy_value, int img_w, int img_h, const double *weight, double *height, double *height_err,
                                uint8_t *immobile, double *score, int *order, int *bad_height)
{
    if (!c || !pos || !pos_err || !oldpos || !oldpos_err || !counts || !vel || !vel_err || !weight || !height || !height_err || !immobile ||
        !score || !order || batch < 1 || stride < 1)
        return ofk_fail(c, OFK_E_INVALID, "ofk_feature_eval: bad argument");
    const size_t n = (size_t)batch * stride;
    Bump bp;
    TRY(est_begin(c, n * (2 + 1 + 2 + 1 + 1 + 1 + 1 + 1) * 8 + (size_t)batch * 64 + 1024, bp));
    double *dp = bp.put(pos, n * 16), *dpe = bp.put(pos_err, n * 8), *dop = bp.put(oldpos, n * 16), *doe = bp.put(oldpos_err, n * 8);
    int *dcn = (int *)bp.put(counts, (size_t)batch * 4);
    double *dv = bp.put(vel, (size_t)batch * 24), *dve = bp.put(vel_err, (size_t)batch * 24), *dw = bp.put(weight, 32);
    double *dh = bp.take(n * 8), *dhe = bp.take(n * 8), *dsc = bp.take(n * 8);
    uint8_t *dim = (uint8_t *)bp.take(n);
    int *dord = (int *)bp.take(n * 4), *dfl = (int *)bp.take(16);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_feature_eval: upload failed");
    OFK_HIP(c, hipMemsetAsync(dfl, 0, 16, c->stream));
    OFK_HIP(c, hipMemsetAsync(dim, 0, n, c->stream));
    OFK_HIP(c, hipMemsetAsync(dh, 0, n * 8, c->stream)); OFK_HIP(c, hipMemsetAsync(dhe, 0, n * 8, c->stream));
    OFK_HIP(c, hipMemsetAsync(dsc, 0, n * 8, c->stream));
    OFK_HIP(c, hipMemsetAsync(dord, 0xff, n * 4, c->stream));                   // slots past a set's count read -1
    // of.pix_trans (of_library.py:31-43): d/2 if even else (d+1)/2
    const double tx = (img_w % 2 == 0) ? img_w / 2.0 : (img_w + 1) / 2.0, ty = (img_h % 2 == 0) ? img_h / 2.0 : (img_h + 1) / 2.0;
    ofk_launch_feature_eval(c->stream, dp, dpe, dop, doe, dcn, batch, stride, dv, dve, focal_len, dummy_value, tx, ty, dw, dh, dhe, dim, dsc,
                            dord, dfl);
    TRY(check_launch(c, "k_feature_eval"));
    int fl[4] = {0, 0, 0, 0};
    TRY(get(c, fl, dfl, 16));
    if (bad_height) *bad_height = fl[1];
    TRY(get(c, height, dh, n * 8)); TRY(get(c, height_err, dhe, n * 8)); TRY(get(c, score, dsc, n * 8));
    TRY(get(c, immobile, dim, n));
    return get(c, order, dord, n * 4);
}

extern "C" int ofk_kf_predict_update(ofk_ctx *c, int ns, int nm, int nc, const double *F, const double *Bm, const double *H,
                                     const double *Q, const double *Rm, double *x, double *P, const double *u, const double *z,
                                     int batch, int do_predict)
{
    if (!c || ns < 1 || ns > 6 || nm < 1 || nm > 6 || nc < 0 || nc > 6 || !F || !H || !Q || !Rm || !x || !P || batch < 1)
        return ofk_fail(c, OFK_E_INVALID, "ofk_kf_predict_update: bad argument");
    Bump bp;
    TRY(est_begin(c, (size_t)batch * (ns + ns * ns + nc + nm) * 8 + 8 * 256 * 8, bp));
    double *dF = bp.put(F, ns * ns * 8), *dB = (Bm && nc) ? bp.put(Bm, ns * nc * 8) : nullptr, *dH = bp.put(H, nm * ns * 8),
           *dQ = bp.put(Q, ns * ns * 8), *dR = bp.put(Rm, nm * nm * 8), *dx = bp.put(x, (size_t)batch * ns * 8),
           *dP = bp.put(P, (size_t)batch * ns * ns * 8), *du = (u && nc) ? bp.put(u, (size_t)batch * nc * 8) : nullptr,
           *dz = bp.put(z, (size_t)batch * nm * 8);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_kf_predict_update: upload failed");
    ofk_launch_kf(c->stream, ns, nm, nc, dF, dB, dH, dQ, dR, dx, dP, du, dz, batch, do_predict);
    TRY(check_launch(c, "k_kf"));
    TRY(get(c, x, dx, (size_t)batch * ns * 8));
    return get(c, P, dP, (size_t)batch * ns * ns * 8);
}

extern "C" int ofk_of_simulation(ofk_ctx *c, const double *truth, const double *sig, const double *pos, const double *true_flow,
                                 int n, const double *z, int trials, double *v_obs, double *bound)
{
    if (!c || !truth || !sig || !pos || !true_flow || !z || !v_obs || !bound || n < 1 || trials < 1)
        return ofk_fail(c, OFK_E_INVALID, "ofk_of_simulation: bad argument");
    const size_t zb = (size_t)trials * (10 + 4 * (size_t)n) * 8;
    Bump bp;
    TRY(est_begin(c, zb + (size_t)n * 32 + (size_t)trials * 32 + 8 * 256, bp));
    double *dt = bp.put(truth, 13 * 8), *ds = bp.put(sig, 6 * 8), *dp = bp.put(pos, (size_t)n * 16), *df = bp.put(true_flow, (size_t)n * 16),
           *dz = bp.put(z, zb), *dv = bp.take((size_t)trials * 24), *db = bp.take((size_t)trials * 8);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_of_simulation: upload failed");
    ofk_launch_of_simulation(c->stream, dt, ds, dp, df, n, dz, trials, dv, db);
    TRY(check_launch(c, "k_of_simulation"));
    TRY(get(c, v_obs, dv, (size_t)trials * 24));
    return get(c, bound, db, (size_t)trials * 8);
}

// of_simulation with the normals drawn on the device (counter-based: k_estimate.hip ofk_noise_normal); nothing but 13 + 6 + 4 n doubles
// goes up and 4 doubles per trial come back
extern "C" int ofk_of_simulation_rng(ofk_ctx *c, const double *truth, const double *sig, const double *pos, const double *true_flow, int n,
                                     unsigned long long seed, unsigned step, unsigned trial0, int trials, double *v_obs, double *bound)
{
    if (!c || !truth || !sig || !pos || !true_flow || !v_obs || !bound || n < 1 || trials < 1 || (unsigned long long)n * 4 + 10 > 0x7fffffffull)
        return ofk_fail(c, OFK_E_INVALID, "ofk_of_simulation_rng: bad argument");
    Bump bp;
    TRY(est_begin(c, (size_t)n * 32 + (size_t)trials * 32 + 8 * 256, bp));
    double *dt = bp.put(truth, 13 * 8), *ds = bp.put(sig, 6 * 8), *dp = bp.put(pos, (size_t)n * 16), *df = bp.put(true_flow, (size_t)n * 16),
           *dv = bp.take((size_t)trials * 24), *db = bp.take((size_t)trials * 8);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_of_simulation_rng: upload failed");
    ofk_launch_of_simulation_rng(c->stream, dt, ds, dp, df, n, seed, step, trial0, trials, dv, db);
    TRY(check_launch(c, "k_of_simulation<rng>"));
    TRY(get(c, v_obs, dv, (size_t)trials * 24));
    return get(c, bound, db, (size_t)trials * 8);
}

// elements 0 .. count - 1 of the noise row of (seed, step, trial): the generator itself, for tests and for callers that want the draws
extern "C" int ofk_noise_normals(ofk_ctx *c, unsigned long long seed, unsigned step, unsigned trial, int count, double *out)
{
    if (!c || !out || count < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_noise_normals: bad argument");
    Bump bp;
    TRY(est_begin(c, (size_t)count * 8 + 256, bp));
    double *d = bp.take((size_t)count * 8);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_noise_normals: scratch");
    ofk_launch_noise_normals(c->stream, (unsigned)seed, (unsigned)(seed >> 32), step, trial, count, d);
    TRY(check_launch(c, "k_noise_normals"));
    return get(c, out, d, (size_t)count * 8);
}

extern "C" int ofk_feas_simulation(ofk_ctx *c, const double *truth, const double *sig, const double *pos, const double *true_flow,
                                   int n, const double *z, int trials, double *mean, double *per_trial, double *v_obs)
{
    if (!c || !truth || !sig || !pos || !true_flow || !z || !mean || n < 1 || trials < 1)
        return ofk_fail(c, OFK_E_INVALID, "ofk_feas_simulation: bad argument");
    const size_t zb = (size_t)trials * (12 + 4 * (size_t)n) * 8, pb = (size_t)trials * 6 * n * 8;
    Bump bp;
    TRY(est_begin(c, zb + pb + (size_t)n * 32 + (size_t)n * 48 + (size_t)trials * 24 + 8 * 256, bp));
    double *dt = bp.put(truth, OFK_FEAS_SIM_TRUTH * 8), *ds = bp.put(sig, OFK_FEAS_SIM_SIG * 8), *dp = bp.put(pos, (size_t)n * 16),
           *df = bp.put(true_flow, (size_t)n * 16), *dz = bp.put(z, zb), *dper = bp.take(pb), *dmean = bp.take((size_t)n * 48),
           *dv = bp.take((size_t)trials * 24);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_feas_simulation: upload failed");
    ofk_launch_feas_simulation(c->stream, dt, ds, dp, df, n, dz, trials, dper, dmean, dv);
    TRY(check_launch(c, "k_feas_simulation"));
    if (per_trial) TRY(get(c, per_trial, dper, pb));
    if (v_obs) TRY(get(c, v_obs, dv, (size_t)trials * 24));
    return get(c, mean, dmean, (size_t)n * 48);
}

extern "C" int ofk_hist_overlap(ofk_ctx *c, const double *data1, int n1, const double *data2, int n2, int bins, int *overlap)
{
    if (!c || !data1 || !data2 || !overlap || n1 < 1 || n2 < 1 || bins < 1 || bins > 1024)
        return ofk_fail(c, OFK_E_INVALID, "ofk_hist_overlap: bad argument (bins 1..1024, both samples non-empty)");
    if (!all_finite(data1, n1) || !all_finite(data2, n2))        // np.histogram raises ValueError on a non-finite range
        return ofk_fail(c, OFK_E_INVALID, "ofk_hist_overlap: non-finite sample");
    Bump bp;
    TRY(est_begin(c, ((size_t)n1 + n2) * 8 + 1024, bp));
    double *d1 = bp.put(data1, (size_t)n1 * 8), *d2 = bp.put(data2, (size_t)n2 * 8);
    int *dout = (int *)bp.take(16);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_hist_overlap: upload failed");
    ofk_launch_hist_overlap(c->stream, d1, n1, d2, n2, bins, dout);
    TRY(check_launch(c, "k_hist_overlap"));
    return get(c, overlap, dout, 4);
}

// ------------------------------------------------------------------------------------------------ resident pipeline
// The second pyramid set of the overlapped schedule, allocated on first use: true when the schedule is on and the set exists.  Where it
// does not fit, the context falls back to the one-set schedule for good.
static bool need_pyr_alt(ofk_ctx *c)
{
    if (!c->overlap) return false;
    for (int k = 0; k < 2; ++k)
        if (!c->pyr_alt[k] && hipMalloc((void **)&c->pyr_alt[k], (size_t)c->max_batch * c->pyr_stride) != hipSuccess) c->overlap = 0;
    if (c->overlap) return true;
    (void)hipGetLastError();
    for (int k = 0; k < 2; ++k) if (c->pyr_alt[k]) { hipFree(c->pyr_alt[k]); c->pyr_alt[k] = nullptr; }
    return false;
}

extern "C" int ofk_pairs_upload(ofk_ctx *c, const uint8_t *prev_bgr, const uint8_t *next_bgr, int batch, int h, int w)
{
    TRY(check_geom(c, batch, h, w, "ofk_pairs_upload"));
    if (!prev_bgr || !next_bgr) return ofk_fail(c, OFK_E_INVALID, "ofk_pairs_upload: NULL buffer");
    const size_t px = (size_t)h * w;
    TRY(h2d(c, c->bgr[0], c->bgr_stride, prev_bgr, px * 3, batch));
    TRY(h2d(c, c->bgr[1], c->bgr_stride, next_bgr, px * 3, batch));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    c->cur_batch = batch; c->cur_h = h; c->cur_w = w;
    c->gray_direct_set = -1;
    return OFK_OK;
}

// Compressed ingest: the frames arrive as baseline JPEG streams (sensor_msgs/CompressedImage payloads) and are decoded on the
// device straight into the resident BGR buffers (k_jpeg.hip) - 15-20x fewer bytes over PCIe than ofk_pairs_upload.
extern "C" int ofk_pairs_upload_jpeg(ofk_ctx *c, const uint8_t *const *prev_jpeg, const size_t *prev_bytes, const uint8_t *const *next_jpeg,
                                     const size_t *next_bytes, int batch)
{
    if (!c) return OFK_E_INVALID;
    if (!prev_jpeg || !prev_bytes || !next_jpeg || !next_bytes) return ofk_fail(c, OFK_E_INVALID, "ofk_pairs_upload_jpeg: NULL argument");
    if (batch < 1 || batch > c->max_batch) return ofk_fail(c, OFK_E_INVALID, "ofk_pairs_upload_jpeg: batch %d exceeds the context (%d)", batch, c->max_batch);
    // both frames of every pair in ONE decoder batch (previous frames first): half the launches and host round trips of two batches
    const uint8_t **all = (const uint8_t **)malloc(sizeof(void *) * 2 * (size_t)batch);
    size_t *len = (size_t *)malloc(sizeof(size_t) * 2 * (size_t)batch);
    if (!all || !len) { free(all); free(len); return ofk_fail(c, OFK_E_INVALID, "out of host memory"); }
    for (int b = 0; b < batch; ++b) { all[b] = prev_jpeg[b]; len[b] = prev_bytes[b]; all[batch + b] = next_jpeg[b]; len[batch + b] = next_bytes[b]; }
    int rc = ofk_jpeg_stage(c, 0, all, len, 2 * batch);
    free(all); free(len);
    if (rc != OFK_OK) return ofk_fail(c, rc, "%s", ofk_jpeg_slot_error(c, 0));      // synchronous caller = the owner thread: its message
    return ofk_pairs_upload_staged(c, 0);
}

// Phase 1 of the compressed ingest, callable from a second thread while the context's owner decodes the other slot (include/ofk.h).
extern "C" int ofk_jpeg_stage(ofk_ctx *c, int slot, const uint8_t *const *jpeg, const size_t *nbytes, int count)
{
    if (!c) return OFK_E_INVALID;
    if (hipSetDevice(c->device) != hipSuccess) return OFK_E_HIP;
    return ofk_jpeg_stage_streams(c, slot, jpeg, nbytes, count);
}

// Message of the slot's last ofk_jpeg_stage ("" after a success).  ofk_jpeg_stage does not touch ofk_last_error: it may run on a helper
// thread while the owner thread is inside another entry point.
extern "C" const char *ofk_jpeg_stage_error(const ofk_ctx *c, int slot) { return ofk_jpeg_slot_error(c, slot); }

// Phase 2: the 2 B streams staged in `slot` (B previous frames, then B next frames) decoded into the resident frame-pair buffers.
extern "C" int ofk_pairs_upload_staged(ofk_ctx *c, int slot)
{
    if (!c) return OFK_E_INVALID;
    TRY(use_device(c));
    // With one slice and the double-buffered pyramid sets of the overlapped schedule the decoder's colour kernel writes GRAY straight
    // into level 0 of the set the next ofk_pairs_run will take (the one the run in flight is NOT reading), on the ingest stream: the
    // decoder passes of batch k + 1 go on beside the run of batch k, and that run's first stage is already done (gray_direct_set).  The
    // set was last read by the LK of the run before the latest one (ev_lkdone).  With several slices, or without the second set, the
    // old way: BGR into bgr[] on the context's stream, behind everything.
    const bool direct = c->nstreams <= 1 && need_pyr_alt(c);
    int h = 0, w = 0, batch = 0;
    c->cur_batch = 0;
    c->gray_direct_set = -1;
    if (direct) {
        const int set = c->pyr_set;
        uint8_t *const *pyr = pyr_set(c, set);
        TRY(ofk_jpeg_decode_staged_pairs(c, slot, pyr[0], pyr[1], c->pyr_stride, c->P, &batch, &h, &w, c->ev_lkdone[set], OFK_MAX_STREAMS, 1));
        c->gray_direct_set = set;
    } else {
        TRY(join_slices(c));
        TRY(ofk_jpeg_decode_staged_pairs(c, slot, c->bgr[0], c->bgr[1], c->bgr_stride, c->P, &batch, &h, &w, nullptr, 0, 0));
    }
    if (batch > c->max_batch) return ofk_fail(c, OFK_E_INVALID, "ofk_pairs_upload_staged: %d pairs exceed the context (%d)", batch, c->max_batch);
    c->cur_batch = batch; c->cur_h = h; c->cur_w = w;
    return OFK_OK;
}

extern "C" int ofk_jpeg_decode_bgr8(ofk_ctx *c, const uint8_t *const *jpeg, const size_t *nbytes, int batch, uint8_t *bgr)
{
    if (!c) return OFK_E_INVALID;
    if (!bgr) return ofk_fail(c, OFK_E_INVALID, "ofk_jpeg_decode_bgr8: NULL output");
    TRY(enter(c));
    int h = 0, w = 0;
    uint8_t *dev = nullptr;
    size_t stride = 0;
    TRY(ofk_jpeg_decode_device(c, jpeg, nbytes, batch, nullptr, 0, 0, &h, &w, &dev, &stride));
    return d2h(c, bgr, dev, stride, (size_t)h * w * 3, batch);
}

extern "C" int ofk_pairs_set_sensors(ofk_ctx *c, const double *sensors, int batch)
{
    if (!c || !sensors || batch < 1 || batch > c->max_batch) return ofk_fail(c, OFK_E_INVALID, "ofk_pairs_set_sensors: bad argument");
    TRY(enter(c));
    OFK_HIP(c, hipMemcpyAsync(c->sensors, sensors, (size_t)batch * OFK_SENSOR_DOUBLES * 8, hipMemcpyHostToDevice, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

struct StageTimer {
    ofk_ctx *c; int stage; bool on; hipStream_t st; int slot;
    StageTimer(ofk_ctx *c_, int stg, hipStream_t s) : c(c_), stage(stg), on(((c_->prof_mask >> stg) & 1) && c_->ev_n + 2 <= c_->ev_cap), st(s), slot(c_->ev_n)
    {
        if (!on) return;
        c->ev_n += 2;
        if (!c->ev[slot]) hipEventCreate(&c->ev[slot]);
        if (!c->ev[slot + 1]) hipEventCreate(&c->ev[slot + 1]);
        hipEventRecord(c->ev[slot], st);
    }
    ~StageTimer()
    {
        if (!on) return;
        hipEventRecord(c->ev[slot + 1], st);
        c->ev_stage[slot / 2] = stage;
    }
};

extern "C" int ofk_pairs_run(ofk_ctx *c, const ofk_params *p)
{
    if (!c || !p) return OFK_E_INVALID;
    if (c->cur_batch < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_pairs_run: no resident frame pairs (call ofk_pairs_upload)");
    TRY(use_device(c));
    const int B = c->cur_batch, h = c->cur_h, w = c->cur_w;
    TRY(check_block(c, h, w, p->block_size));
    TRY(check_select(c, p->max_corners, p->quality, p->min_distance));
    TRY(check_lk(c, h, w, p->win, p->max_level));
    if (p->solve_variant != OFK_SOLVE_NODE && p->solve_variant != OFK_SOLVE_SIM) return ofk_fail(c, OFK_E_INVALID, "solve_variant must be NODE or SIM");
    TRY(grid_prepare(c, c->grid, B, h, w, "ofk_pairs_run"));
    const ofk_levels lv = ofk_make_levels(h, w, p->win, p->max_level);
    // The batch is cut into `nstreams` contiguous slices, each running the whole stage chain on its own stream: the
    // latency-bound stages of one slice (corner selection: one workgroup per image; the per-pair solve) overlap with the
    // streaming stages of the others.  Pairs are independent, so slices share nothing.
    const int S = c->nstreams < 1 ? 1 : (c->nstreams > B ? B : c->nstreams);
    // Inside a slice the chain forks once more: the response kernel and LK are VALU-bound, the gray conversions and the
    // pyramids HBM-bound, so the two kinds run beside each other.  The gray conversions and the pyramids (HBM-bound) run on an auxiliary stream and may even run AHEAD of the context's
    // stream: they write one of two pyramid buffer sets, alternating per call, so the next call's conversions overlap this
    // call's LK.  The only hazard is the set itself, still read by the LK of the call that used it last (ev_lkdone).
    const bool overlap = need_pyr_alt(c);
    int set = 0;
    if (overlap) { set = c->pyr_set; c->pyr_set ^= 1; }
    const bool have_gray = c->gray_direct_set >= 0;               // compressed ingest: the frames came in as gray level 0 of that set (and only there)
    if (have_gray) { set = c->gray_direct_set; c->pyr_set = set ^ 1; }
    c->pyr_last = set;
    // Slices are forked off the context's stream once and then free-run over consecutive calls: nothing joins them until an
    // entry point needs the context's stream to see their results (join_slices).  On the fork the response kernels are chained
    // slice after slice, which offsets the slices by one response kernel for as long as they run.
    const bool fork = S > 1 && !c->slices_open;
    if (c->robust.loss != OFK_ROBUST_OFF) { TRY(robust_alloc(c)); c->rob_batch = B; }
    if (gate_on(c->gate)) { TRY(gate_alloc(c)); c->gate_batch = B; c->gate_fb = c->gate.fb_mode != OFK_FB_OFF; }
    TRY(second_prepare(c, B, p->solve_variant, nullptr, "ofk_pairs_run"));
    TRY(solve_points_prepare(c, B));
    TRY(need_streams(c, S, overlap));
    if (fork) {
        OFK_HIP(c, hipEventRecord(c->ev_fork, c->stream));
        for (int k = 1; k < S; ++k) OFK_HIP(c, hipStreamWaitEvent(c->streams[k], c->ev_fork, 0));
    }
    int rc_track = OFK_OK;                                       // a failed gate copy is reported behind the loop: the slices' events and
                                                                 // the bookkeeping below stay whole, so the next call joins what this one forked
    for (int k = 0; k < S; ++k) {
        const int b0 = (int)((long long)B * k / S), nb = (int)((long long)B * (k + 1) / S) - b0;
        if (nb <= 0) continue;
        hipStream_t st = k == 0 ? c->stream : c->streams[k];
        hipStream_t sa = overlap ? c->aux[k] : st;
        if (overlap) OFK_HIP(c, hipStreamWaitEvent(sa, c->ev_lkdone[set][k], 0));
        View v = view_of(c, b0, nb, set);
        if (!have_gray) {
            StageTimer t(c, OFK_STAGE_GRAY, sa);
            ofk_launch_gray(sa, v.bgr[0], c->bgr_stride, v.pyr[0], c->pyr_stride, nb, h, w);
        }
        if (overlap) OFK_HIP(c, hipEventRecord(c->ev_g0[k], sa));
        if (!have_gray) {
            StageTimer t(c, OFK_STAGE_GRAY, sa);
            ofk_launch_gray(sa, v.bgr[1], c->bgr_stride, v.pyr[1], c->pyr_stride, nb, h, w);
        }
        {
            StageTimer t(c, OFK_STAGE_PYR, sa);
            build_pyramids(c, sa, v.pyr[0], v.pyr[1], lv, nb);
        }
        if (overlap) {
            OFK_HIP(c, hipEventRecord(c->ev_aux[k], sa));
            OFK_HIP(c, hipStreamWaitEvent(st, c->ev_g0[k], 0));              // the response kernel needs the previous frame's gray level
        }
        if (fork && k > 0) OFK_HIP(c, hipStreamWaitEvent(st, c->ev_stagger[k - 1], 0));
        {
            StageTimer t(c, OFK_STAGE_EIG, st);
            TRY(detect_response(c, st, v, nullptr, h, w, p->block_size, p->quality));
        }
        if (fork) OFK_HIP(c, hipEventRecord(c->ev_stagger[k], st));
        {
            StageTimer t(c, OFK_STAGE_SELECT, st);
            detect_select(c, st, v, h, w, p->max_corners, p->quality, p->min_distance, v.pts_prev, v.counts, nullptr, c->grid);
        }
        if (overlap) OFK_HIP(c, hipStreamWaitEvent(st, c->ev_aux[k], 0));    // LK needs both pyramids
        {
            StageTimer t(c, OFK_STAGE_LK, st);
            const int rc = track(c, st, v, lv, p, nullptr);      // a seed comes from the pair's sensors
            if (rc != OFK_OK && rc_track == OFK_OK) rc_track = rc;
        }
        if (overlap) OFK_HIP(c, hipEventRecord(c->ev_lkdone[set][k], st));   // behind the set's last reader (the gate's backward pass, when on): it may be rewritten from here on
        if (c->x_pending) OFK_HIP(c, hipStreamWaitEvent(st, c->ev_x, 0));    // the previous call's records are still being exported
        {
            StageTimer t(c, OFK_STAGE_SOLVE, st);
            solve_pairs(c, st, v.solve_prev, v.solve_next, v.status, v.counts, v.sensors, p, v.cand_count, v.records, b0, nb, false);
        }
        if (S > 1) OFK_HIP(c, hipEventRecord(c->ev_end[k], st));             // joined lazily (join_slices), not here
    }
    if (S > 1) { c->slices_open = 1; c->open_slices = S; }
    if (rc_track != OFK_OK) return rc_track;
    return check_launch(c, "ofk_pairs_run");
}

extern "C" int ofk_pairs_download(ofk_ctx *c, double *records, float *prev_pts, float *next_pts, uint8_t *status, float *err,
                                  int *counts)
{
    if (!c || c->cur_batch < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_pairs_download: nothing resident");
    TRY(enter(c));
    const int B = c->cur_batch;
    const size_t np = (size_t)B * c->max_pts;
    int flags[4];
    OFK_HIP(c, hipMemcpyAsync(flags, c->dev_flags, 16, hipMemcpyDeviceToHost, c->stream));
    if (records) OFK_HIP(c, hipMemcpyAsync(records, c->records, (size_t)B * OFK_RECORD_DOUBLES * 8, hipMemcpyDeviceToHost, c->stream));
    if (prev_pts) OFK_HIP(c, hipMemcpyAsync(prev_pts, c->pts_prev, np * 8, hipMemcpyDeviceToHost, c->stream));
    if (next_pts) OFK_HIP(c, hipMemcpyAsync(next_pts, c->pts_next, np * 8, hipMemcpyDeviceToHost, c->stream));
    if (status) OFK_HIP(c, hipMemcpyAsync(status, c->status, np, hipMemcpyDeviceToHost, c->stream));
    if (err) OFK_HIP(c, hipMemcpyAsync(err, c->err, np * 4, hipMemcpyDeviceToHost, c->stream));
    if (counts) OFK_HIP(c, hipMemcpyAsync(counts, c->counts, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return check_capacity(c, flags, counts, B);
}

// What was just queued on the tail stream reads the records: while the slices are open, their next solve must not overtake it
static int tail_done(ofk_ctx *c, hipStream_t s)
{
    if (c->slices_open) {
        OFK_HIP(c, hipEventRecord(c->ev_x, s));
        c->x_pending = 1;
    }
    return OFK_OK;
}

// k_records_f32 of the latest ofk_pairs_run on the stream that ends the step (the last slice's, behind the other slices' end
// events); *stream_out lets a caller queue more work behind it (the RCCL gather of ofk_comm.hip)
int ofk_export_records_stream(ofk_ctx *c, float *device_dst, int batch, hipStream_t *stream_out)
{
    hipStream_t s;
    TRY(tail_stream(c, &s));
    ofk_launch_records_f32(s, c->records, device_dst, batch);
    TRY(tail_done(c, s));
    if (stream_out) *stream_out = s;
    return check_launch(c, "k_records_f32");
}

extern "C" int ofk_pairs_export_records_f32(ofk_ctx *c, void *device_dst, int batch)
{
    if (!c || !device_dst || batch < 1 || batch > c->cur_batch) return ofk_fail(c, OFK_E_INVALID, "ofk_pairs_export_records_f32: bad argument");
    return ofk_export_records_stream(c, (float *)device_dst, batch, nullptr);
}

// ------------------------------------------------------------------------------------------------ camera stage entries
// device scratch only, so resident points and settings are not touched; `out` goes up first: entries beyond counts[b] keep its contents
static int camera_points(ofk_ctx *c, const char *who, int distort, const ofk_camera *m, const float *pts, const int *counts, int batch, int stride,
                         float *out)
{
    if (!c) return OFK_E_INVALID;
    if (!m || !pts || !counts || !out || batch < 1 || stride < 1) return ofk_fail(c, OFK_E_INVALID, "%s: bad argument", who);
    TRY(check_camera(c, m, false, who));
    TRY(check_counts(c, who, counts, batch, stride));
    const size_t pb = (size_t)batch * stride * 8;
    Bump bp;
    TRY(est_begin(c, 2 * pb + (size_t)batch * 4, bp));
    const float *dp = (const float *)bp.put(pts, pb);
    float *dout = (float *)bp.put(out, pb);
    const int *dc = (const int *)bp.put(counts, (size_t)batch * 4);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
    ofk_launch_camera(c->stream, m, distort, dp, dout, nullptr, nullptr, dc, stride, batch);
    TRY(check_launch(c, who));
    return get(c, out, dout, pb);
}

extern "C" int ofk_undistort_points(ofk_ctx *c, const ofk_camera *m, const float *pts, const int *counts, int batch, int stride, float *out)
{
    return camera_points(c, "ofk_undistort_points", 0, m, pts, counts, batch, stride, out);
}

extern "C" int ofk_distort_points(ofk_ctx *c, const ofk_camera *m, const float *pts, const int *counts, int batch, int stride, float *out)
{
    return camera_points(c, "ofk_distort_points", 1, m, pts, counts, batch, stride, out);
}

extern "C" int ofk_camera_download(ofk_ctx *c, float *prev_ideal, float *next_ideal, int stride)
{
    return points_download(c, POINTS[POINTS_CAMERA], "ofk_camera_download", prev_ideal, next_ideal, stride);
}

// the warp through a lens: ofk_warp_perspective's buffers and checks, ofk_undistort_points' camera checks
extern "C" int ofk_warp_lens(ofk_ctx *c, const ofk_camera *m, const uint8_t *src, int sh, int sw, int channels, const double *M, uint8_t *dst, int dh,
                             int dw, int border, int border_value, double r_max, int batch, int *covered)
{
    const char *who = "ofk_warp_lens";
    if (!c) return OFK_E_INVALID;
    TRY(check_geom(c, batch, sh, sw, "ofk_warp_lens (source)"));
    TRY(check_geom(c, batch, dh, dw, "ofk_warp_lens (destination)"));
    if (!m || !src || !dst) return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
    if (channels != 1 && channels != 3) return ofk_fail(c, OFK_E_INVALID, "%s: %d channels (1 or 3)", who, channels);
    if (border != OFK_BORDER_CONSTANT && border != OFK_BORDER_REPLICATE) return ofk_fail(c, OFK_E_INVALID, "%s: unknown border %d", who, border);
    if (border_value < 0 || border_value > 255) return ofk_fail(c, OFK_E_INVALID, "%s: border_value %d outside 0..255", who, border_value);
    if (!std::isfinite(r_max) || r_max < 0.0) return ofk_fail(c, OFK_E_INVALID, "%s: r_max = %g is negative or not finite", who, r_max);
    TRY(check_camera(c, m, false, who));
    const size_t m_bytes = up((size_t)batch * 9 * sizeof(double), 256);
    TRY(ofk_need_scratch(c, m_bytes + (size_t)batch * sizeof(int)));
    double *d_M = M ? (double *)c->scratch : nullptr;
    int *d_cov = covered ? (int *)((char *)c->scratch + m_bytes) : nullptr;
    TRY(h2d(c, c->bgr[0], c->bgr_stride, src, (size_t)sh * sw * channels, batch));
    if (M) OFK_HIP(c, hipMemcpyAsync(d_M, M, (size_t)batch * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ofk_launch_warp_lens(c->stream, m, r_max, c->bgr[0], c->bgr_stride, sh, sw, channels, d_M, c->bgr[1], c->bgr_stride, dh, dw, border, border_value, d_cov, batch);
    TRY(check_launch(c, "k_warp_lens_u8"));
    if (covered) OFK_HIP(c, hipMemcpyAsync(covered, d_cov, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    return d2h(c, dst, c->bgr[1], c->bgr_stride, (size_t)dh * dw * channels, batch);
}

// ------------------------------------------------------------------------------------------------ rectify setting
static int check_rectify(ofk_ctx *c, const ofk_rectify *r, const char *who)
{
    if (r->mode != OFK_RECTIFY_OFF && r->mode != OFK_RECTIFY_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_RECTIFY_OFF nor OFK_RECTIFY_ON", who, r->mode);
    if (!std::isfinite(r->r_max) || r->r_max < 0.0) return ofk_fail(c, OFK_E_INVALID, "%s: r_max = %g is negative or not finite", who, r->r_max);
    return OFK_OK;
}
extern "C" int ofk_set_rectify(ofk_ctx *c, const ofk_rectify *r)
{
    return setting_set(c, &ofk_ctx::rect, r && r->mode == OFK_RECTIFY_OFF ? nullptr : r, [](ofk_rectify &s) { s.mode = OFK_RECTIFY_OFF; },
                       [c](const ofk_rectify *v) { return check_rectify(c, v, "ofk_set_rectify"); });
}
extern "C" int ofk_get_rectify(const ofk_ctx *c, ofk_rectify *r) { return setting_get(c, &ofk_ctx::rect, r); }

// ------------------------------------------------------------------------------------------------ rolling-shutter and finite-motion stage entries
// Both ends of every point through one launch.  Device scratch only, so resident points and settings are not touched; the outputs go
// up first: entries beyond counts[b] keep their contents.  have: the setting's struct is there; id0 / id1: optional, both or neither;
// rules(): the setting's check and its rule on the sensors; launch(in0, in1, id0, id1, out0, out1, counts, sensors) on device arrays.
template <class Rules, class Launch>
static int correct_points(ofk_ctx *c, const char *who, bool have, const float *in0, const float *in1, const float *id0, const float *id1,
                          const int *counts, int batch, int stride, const double *sensors, float *out0, float *out1, Rules rules, Launch launch)
{
    if (!c) return OFK_E_INVALID;
    if (!have || !in0 || !in1 || !counts || !out0 || !out1 || batch < 1 || stride < 1 || !id0 != !id1) return ofk_fail(c, OFK_E_INVALID, "%s: bad argument", who);
    TRY(rules());
    TRY(check_counts(c, who, counts, batch, stride));
    const size_t pb = (size_t)batch * stride * 8, sb = (size_t)batch * OFK_SENSOR_DOUBLES * 8;
    Bump bp;
    TRY(est_begin(c, (id0 ? 6 : 4) * pb + sb + (size_t)batch * 4, bp));
    const float *d0 = (const float *)bp.put(in0, pb), *d1 = (const float *)bp.put(in1, pb);
    const float *di0 = (const float *)bp.put(id0, pb), *di1 = (const float *)bp.put(id1, pb);                    // NULL stays NULL
    float *do0 = (float *)bp.put(out0, pb), *do1 = (float *)bp.put(out1, pb);
    const double *dsn = bp.put(sensors, sb);
    const int *dc = (const int *)bp.put(counts, (size_t)batch * 4);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
    launch(d0, d1, di0, di1, do0, do1, dc, dsn);
    TRY(check_launch(c, who));
    OFK_HIP(c, hipMemcpyAsync(out0, do0, pb, hipMemcpyDeviceToHost, c->stream));
    return get(c, out1, do1, pb);
}

extern "C" int ofk_rs_correct_points(ofk_ctx *c, const ofk_rshutter *r, const float *raw_prev, const float *raw_next, const float *ideal_prev,
                                     const float *ideal_next, const int *counts, int batch, int stride, const double *sensors, float *out_prev,
                                     float *out_next)
{
    const char *who = "ofk_rs_correct_points";
    return correct_points(c, who, r != nullptr, raw_prev, raw_next, ideal_prev, ideal_next, counts, batch, stride, sensors, out_prev, out_next,
        [&] {
            TRY(check_rs(c, r, true, who));
            return r->mode == OFK_RS_GYRO && !sensors ? ofk_fail(c, OFK_E_INVALID, "%s: OFK_RS_GYRO needs the sensors", who) : OFK_OK;
        },
        [&](const float *d0, const float *d1, const float *di0, const float *di1, float *do0, float *do1, const int *dc, const double *dsn) {
            ofk_launch_rs_correct(c->stream, r, d0, d1, di0, di1, do0, do1, dc, stride, dsn, nullptr, batch);
        });
}

extern "C" int ofk_rs_download(ofk_ctx *c, float *prev, float *next, int stride)
{
    return points_download(c, POINTS[POINTS_RS], "ofk_rs_download", prev, next, stride);
}

extern "C" int ofk_finite_correct_points(ofk_ctx *c, const ofk_finite_motion *f, const float *prev, const float *next, const int *counts, int batch,
                                         int stride, const double *sensors, float *out_prev, float *out_next)
{
    const char *who = "ofk_finite_correct_points";
    return correct_points(c, who, f != nullptr, prev, next, nullptr, nullptr, counts, batch, stride, sensors, out_prev, out_next,
        [&] {
            TRY(check_fm(c, f, who));
            return !sensors ? ofk_fail(c, OFK_E_INVALID, "%s: the rewrite needs the sensors", who) : OFK_OK;
        },
        [&](const float *d0, const float *d1, const float *, const float *, float *do0, float *do1, const int *dc, const double *dsn) {
            ofk_launch_finite_correct(c->stream, f, d0, d1, do0, do1, dc, stride, dsn, nullptr, batch);
        });
}

extern "C" int ofk_finite_download(ofk_ctx *c, float *prev, float *next, int stride)
{
    return points_download(c, POINTS[POINTS_FM], "ofk_finite_download", prev, next, stride);
}

// ------------------------------------------------------------------------------------------------ exclusion zones
static int check_zones(ofk_ctx *c, const ofk_zones *z, const char *who)
{
    if (z->mode != OFK_ZONES_OFF && z->mode != OFK_ZONES_HULL) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_ZONES_OFF nor OFK_ZONES_HULL", who, z->mode);
    if (z->mode == OFK_ZONES_OFF) return OFK_OK;
    if (z->link < 1 || z->link > 4096) return ofk_fail(c, OFK_E_INVALID, "%s: link %d outside 1..4096", who, z->link);
    if (z->min_members < 1 || z->min_members > c->max_pts) return ofk_fail(c, OFK_E_INVALID, "%s: min_members %d outside 1..%d", who, z->min_members, c->max_pts);
    if (z->radius < 0 || z->radius > 255) return ofk_fail(c, OFK_E_INVALID, "%s: radius %d outside 0..255", who, z->radius);
    if (z->ttl < 1 || z->ttl > 65535) return ofk_fail(c, OFK_E_INVALID, "%s: ttl %d outside 1..65535", who, z->ttl);
    if (z->max_zones < 1 || z->max_zones > OFK_ZONE_MAX) return ofk_fail(c, OFK_E_INVALID, "%s: max_zones %d outside 1..%d", who, z->max_zones, OFK_ZONE_MAX);
    return OFK_OK;
}

extern "C" int ofk_set_zones(ofk_ctx *c, const ofk_zones *z)
{
    return setting_set(c, &ofk_ctx::zones, z && z->mode == OFK_ZONES_OFF ? nullptr : z, [](ofk_zones &s) { s.mode = OFK_ZONES_OFF; },
                       [c](const ofk_zones *v) { return check_zones(c, v, "ofk_set_zones"); });
}
extern "C" int ofk_get_zones(const ofk_ctx *c, ofk_zones *z) { return setting_get(c, &ofk_ctx::zones, z); }

// bytes of the tables, the motion rows and the statistics of `batch` streams (each kind lies back to back)
static size_t zones_tab_bytes(int batch) { return (size_t)batch * OFK_ZONE_MAX * OFK_ZONE_INTS * 4; }
static size_t zones_mot_bytes(int batch) { return (size_t)batch * OFK_ZONE_MAX * OFK_ZONE_FLOATS * 4; }
static size_t zones_stat_bytes(int batch) { return (size_t)batch * OFK_ZONE_STATS * 4; }
static int zones_clear(ofk_ctx *c, int batch)
{
    OFK_HIP(c, hipMemsetAsync(c->zone_tab, 0, zones_tab_bytes(batch), c->stream));
    OFK_HIP(c, hipMemsetAsync(c->zone_mot, 0, zones_mot_bytes(batch), c->stream));
    OFK_HIP(c, hipMemsetAsync(c->zone_stats, 0, zones_stat_bytes(batch), c->stream));
    return OFK_OK;
}
// the zones' resident buffers, allocated (and cleared) when a step or an entry first needs them
static int zones_alloc(ofk_ctx *c)
{
    if (c->zone_tab) return OFK_OK;                              // one allocation, carved into the five buffers
    const size_t B = (size_t)c->max_batch, o_mot = up(zones_tab_bytes(c->max_batch), 256), o_st = o_mot + up(zones_mot_bytes(c->max_batch), 256),
                 o_wk = o_st + up(zones_stat_bytes(c->max_batch), 256), o_ss = o_wk + up(B * 2 * c->max_pts * 4, 256);
    uint8_t *base = nullptr;
    OFK_HIP(c, hipMalloc((void **)&base, o_ss + B * c->max_pts));
    c->zone_tab = (int *)base; c->zone_mot = (float *)(base + o_mot); c->zone_stats = (int *)(base + o_st); c->zone_work = (int *)(base + o_wk);
    c->zone_status = base + o_ss;
    return zones_clear(c, c->max_batch);
}

extern "C" int ofk_zones_reset(ofk_ctx *c, int batch)
{
    if (!c) return OFK_E_INVALID;
    if (batch < 1 || batch > c->max_batch) return ofk_fail(c, OFK_E_INVALID, "ofk_zones_reset: batch %d outside 1..%d", batch, c->max_batch);
    TRY(enter(c));
    TRY(zones_alloc(c));
    TRY(zones_clear(c, batch));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

extern "C" int ofk_zones_download(ofk_ctx *c, int *zones, float *motion, int *stats)
{
    if (!c) return OFK_E_INVALID;
    TRY(enter(c));
    TRY(zones_alloc(c));
    if (zones) OFK_HIP(c, hipMemcpyAsync(zones, c->zone_tab, zones_tab_bytes(c->max_batch), hipMemcpyDeviceToHost, c->stream));
    if (motion) OFK_HIP(c, hipMemcpyAsync(motion, c->zone_mot, zones_mot_bytes(c->max_batch), hipMemcpyDeviceToHost, c->stream));
    if (stats) OFK_HIP(c, hipMemcpyAsync(stats, c->zone_stats, zones_stat_bytes(c->max_batch), hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

extern "C" int ofk_zones_step(ofk_ctx *c, const float *old_pts, const float *new_pts, const uint8_t *status, const uint8_t *keep, const int *counts,
                              int batch, int stride, int h, int w, const uint8_t *mask_in, uint8_t *mask_out)
{
    TRY(check_geom(c, batch, h, w, "ofk_zones_step"));
    if (!old_pts || !new_pts || !status || !keep || !counts || !mask_out) return ofk_fail(c, OFK_E_INVALID, "ofk_zones_step: NULL argument");
    if (stride < 1 || stride > c->max_pts) return ofk_fail(c, OFK_E_INVALID, "ofk_zones_step: stride %d outside 1..%d", stride, c->max_pts);
    if (c->zones.mode == OFK_ZONES_OFF) return ofk_fail(c, OFK_E_INVALID, "ofk_zones_step: ofk_set_zones is off");
    TRY(zones_alloc(c));
    TRY(lazy_mask(c));
    const size_t np = (size_t)batch * stride;
    Bump bp;
    TRY(est_begin(c, np * 18 + (size_t)batch * 4, bp));
    const float *d_old = (const float *)bp.put(old_pts, np * 8), *d_new = (const float *)bp.put(new_pts, np * 8);
    const uint8_t *d_st = (const uint8_t *)bp.put(status, np), *d_keep = (const uint8_t *)bp.put(keep, np);
    const int *d_cnt = (const int *)bp.put(counts, (size_t)batch * 4);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "ofk_zones_step: upload failed");
    ofk_launch_zones_update(c->stream, d_old, d_new, d_st, d_keep, d_cnt, stride, &c->zones, c->zone_tab, c->zone_mot, c->zone_stats, c->zone_work, 0, batch);
    if (mask_in) TRY(h2d(c, c->mask, c->img_stride, mask_in, (size_t)h * w, batch));
    else OFK_HIP(c, hipMemsetAsync(c->mask, 1, (size_t)batch * c->img_stride, c->stream));
    ofk_launch_zone_mask(c->stream, c->mask, c->img_stride, h, w, c->zone_tab, c->zone_mot, c->zones.radius, nullptr, batch);
    ofk_launch_zones_age(c->stream, c->zone_tab, c->zone_mot, c->zone_stats, batch);
    TRY(check_launch(c, "ofk_zones_step"));
    return d2h(c, mask_out, c->mask, c->img_stride, (size_t)h * w, batch);
}

// ------------------------------------------------------------------------------------------------ the per-track states of a stream
// One row per state that a stream keeps per track, in the order in which a step begins them (the keyframe in front of its rotation: a
// keyframe that begins afresh takes the rotation state with it).  Each state lives in ONE lazy allocation, cleared when it is made and
// carved into the arrays of its list; the first array owns it.
struct track_array { size_t at, row, stream; };                  // where ofk_ctx holds the pointer; its bytes per row of the table, per stream
#define TRACK_ARRAY(member, row, stream) {offsetof(ofk_ctx, member), (size_t)(row), (size_t)(stream)}
#define TRACK_LIST(a) a, (int)(sizeof(a) / sizeof(a[0]))
static int tp_stride_of(int win) { return (int)up((size_t)(win + 2) * (win + 2), 4); }
static const track_array TT_ARRAYS[] = {TRACK_ARRAY(ttr.ids, 4, 0), TRACK_ARRAY(ttr.age, 4, 0), TRACK_ARRAY(ttr.birth_step, 4, 0), TRACK_ARRAY(ttr.birth_xy, 8, 0),
    TRACK_ARRAY(ttr.flow_xy, 8, 0), TRACK_ARRAY(ttr.step_ids, 4, 0), TRACK_ARRAY(ttr.head, 0, 8), TRACK_ARRAY(ttr.stats, 0, OFK_TT_STATS * 4)};
static const track_array TD_ARRAYS[] = {TRACK_ARRAY(tdr.rho, 8, 0), TRACK_ARRAY(tdr.var, 8, 0), TRACK_ARRAY(tdr.nobs, 4, 0), TRACK_ARRAY(tdr.rec, 0, OFK_TD_DOUBLES * 8)};
static const track_array TP_ARRAYS[] = {                         // the templates of the widest window
    TRACK_ARRAY(tpr.tmpl[0], tp_stride_of(31), 0), TRACK_ARRAY(tpr.tmpl[1], tp_stride_of(31), 0), TRACK_ARRAY(tpr.A, 16, 0), TRACK_ARRAY(tpr.A_new, 16, 0),
    TRACK_ARRAY(tpr.ncc, 4, 0), TRACK_ARRAY(tpr.ncc_new, 4, 0), TRACK_ARRAY(tpr.move, 4, 0), TRACK_ARRAY(tpr.flag, 1, 0), TRACK_ARRAY(tpr.flag_new, 1, 0),
    TRACK_ARRAY(tpr.tstate, 1, 0), TRACK_ARRAY(tpr.L, 0, 16), TRACK_ARRAY(tpr.rec, 0, OFK_TPL_DOUBLES * 8)};
static const track_array KF_ARRAYS[] = {TRACK_ARRAY(kfr.key_xy, 8, 0), TRACK_ARRAY(kfr.member, 1, 0), TRACK_ARRAY(kfr.st, 0, OFK_KEY_STATE * 8),
    TRACK_ARRAY(kfr.ist, 0, OFK_KEY_INTS * 4), TRACK_ARRAY(kfr.rec, 0, OFK_KEY_DOUBLES * 8), TRACK_ARRAY(kfr.next_copy, 8, 0)};
static const track_array KR_ARRAYS[] = {TRACK_ARRAY(kr_st, 0, OFK_KEYROT_STATE * 8), TRACK_ARRAY(kr_rec, 0, OFK_KEYROT_DOUBLES * 8)};
static const track_array KM_ARRAYS[] = {TRACK_ARRAY(kmr.key_rho, 8, 0), TRACK_ARRAY(kmr.key_var, 8, 0), TRACK_ARRAY(kmr.mstate, 0, 8),
    TRACK_ARRAY(kmr.mrec, 0, OFK_KEYMAP_DOUBLES * 8)};
static const track_array PF_ARRAYS[] = {TRACK_ARRAY(pf_x, 0, OFK_POSF_STATES * 8), TRACK_ARRAY(pf_P, 0, OFK_POSF_STATES * OFK_POSF_STATES * 8),
    TRACK_ARRAY(pf_rec, 0, OFK_POSF_DOUBLES * 8), TRACK_ARRAY(pf_in, 0, OFK_POSF_INPUT * 8), TRACK_ARRAY(pf_ist, 0, OFK_POSF_INTS * 4)};
static const track_array SB_ARRAYS[] = {TRACK_ARRAY(sb_Bv, 0, 72), TRACK_ARRAY(sb_rec, 0, OFK_STAB_DOUBLES * 8), TRACK_ARRAY(sb_M, 0, 72),
    TRACK_ARRAY(sb_st, 0, OFK_KEY_STATE * 8), TRACK_ARRAY(sb_ist, 0, OFK_STAB_INTS * 4), TRACK_ARRAY(sb_cov, 0, 4)};

enum { TS_TABLE, TS_DEPTH, TS_TEMPLATE, TS_KEY, TS_KEYROT, TS_KEYMAP, TS_POSF, TS_STAB };
struct track_state {
    const char *set, *download, *began;                          // the setter's and the download's names, "run" / "stepped": for messages
    bool (*on)(const ofk_ctx *);
    int ofk_ctx::*batch, ofk_ctx::*live;                         // streams of the latest begin / step with it on; streams whose rows match their tracks
    const track_array *arrays; int narrays;
    int (*begin)(ofk_ctx *, int B);                              // what a state that is not live queues to begin afresh
    void (*replace)(ofk_ctx *, int B);                           // beside k_replace_tracks; NULL: nothing
    int needs; const char *why;                                  // the state it is refused without (-1: none), and the refusal's last clause
    const char *model;                                           // not NULL: the sensor model only; what the refusal calls it
};
static const track_state TRACK[] = {
    {"ofk_set_track_table", "ofk_track_table_download", "run", [](const ofk_ctx *c) { return c->tt.mode != OFK_TT_OFF; },
     &ofk_ctx::tt_batch, &ofk_ctx::tt_live, TRACK_LIST(TT_ARRAYS),
     [](ofk_ctx *c, int B) -> int { ofk_launch_track_table_begin(c->stream, c->ttr, c->pts_prev, c->counts, c->max_pts, B); return OFK_OK; },
     [](ofk_ctx *c, int B) { ofk_launch_track_table_replace(c->stream, c->ttr, c->limit, c->pts_new, c->new_counts, c->max_pts, B); }, -1, nullptr, nullptr},
    {"ofk_set_track_depth", "ofk_track_depth_download", "stepped", [](const ofk_ctx *c) { return c->td.mode != OFK_TD_OFF; },
     &ofk_ctx::td_batch, &ofk_ctx::td_live, TRACK_LIST(TD_ARRAYS),
     [](ofk_ctx *c, int B) -> int { ofk_launch_track_depth_begin(c->stream, c->tdr, c->counts, c->max_pts, B); return OFK_OK; },
     [](ofk_ctx *c, int B) { ofk_launch_track_depth_replace(c->stream, c->tdr, c->limit, c->new_counts, c->max_pts, B); },
     TS_TABLE, "the depths are kept per row of the table", "depth per track"},
    {"ofk_set_track_template", "ofk_track_template_download", "stepped", [](const ofk_ctx *c) { return c->tpl.mode != OFK_TPL_OFF; },
     &ofk_ctx::tp_batch, &ofk_ctx::tp_live, TRACK_LIST(TP_ARRAYS),
     [](ofk_ctx *c, int) -> int {                                // none (tstate 0); rows of age 0 are captured anew whatever replaced them
         OFK_HIP(c, hipMemsetAsync(c->tpr.tstate, 0, (size_t)c->max_batch * c->max_pts, c->stream));
         OFK_HIP(c, hipMemsetAsync(c->tpr.rec, 0, (size_t)c->max_batch * OFK_TPL_DOUBLES * 8, c->stream));
         c->tpr.cur = 0; c->tpr.tstride = tp_stride_of(c->tpl.win);
         return OFK_OK;
     },
     nullptr, TS_TABLE, "the templates are kept per row of the table", nullptr},
    {"ofk_set_keyframe", "ofk_keyframe_download", "stepped", [](const ofk_ctx *c) { return c->key.mode != OFK_KEY_OFF; },
     &ofk_ctx::kf_batch, &ofk_ctx::kf_live, TRACK_LIST(KF_ARRAYS),
     [](ofk_ctx *c, int B) -> int { ofk_launch_keyframe_begin(c->stream, c->kfr, c->counts, c->max_pts, B); c->kr_live = c->km_live = 0; return OFK_OK; },
     [](ofk_ctx *c, int B) { ofk_launch_keyframe_replace(c->stream, c->kfr, c->limit, c->new_counts, c->max_pts, B); },
     TS_TABLE, "the keyframe is kept per row of the table", "keyframe"},
    {"ofk_set_keyframe_rotation", "ofk_keyframe_rotation_download", "stepped", [](const ofk_ctx *c) { return c->krot.mode != OFK_KEYROT_OFF; },
     &ofk_ctx::kr_batch, &ofk_ctx::kr_live, TRACK_LIST(KR_ARRAYS),     // in step with the keyframe's: cleared where that began afresh
     [](ofk_ctx *c, int B) -> int { ofk_launch_keyrot_clear(c->stream, c->kr_st, c->kr_rec, nullptr, 0, OFK_KEYROT_NONE, B); return OFK_OK; },
     [](ofk_ctx *c, int B) { ofk_launch_keyrot_clear(c->stream, c->kr_st, c->kr_rec, c->limit, 0, OFK_KEYROT_NONE, B); },
     TS_KEY, "it refines the keyframe's rotation", nullptr},
    {"ofk_set_keyframe_map", "ofk_keyframe_map_download", "stepped", [](const ofk_ctx *c) { return c->kmap.mode != OFK_KEYMAP_OFF; },
     &ofk_ctx::km_batch, &ofk_ctx::km_live, TRACK_LIST(KM_ARRAYS),     // in step with the keyframe's: cleared where that began afresh
     [](ofk_ctx *c, int B) -> int { ofk_launch_keymap_clear(c->stream, c->kmr, c->kfr.ist, nullptr, c->counts, c->max_pts, 0, 0, B); return OFK_OK; },
     [](ofk_ctx *c, int B) { ofk_launch_keymap_clear(c->stream, c->kmr, c->kfr.ist, c->limit, c->new_counts, c->max_pts, 0, 1, B); },
     TS_KEY, "it solves the keyframe's translation", nullptr},
    {"ofk_set_pos_filter", "ofk_pos_filter_download", "stepped", [](const ofk_ctx *c) { return c->posf.mode != OFK_POSF_OFF; },
     &ofk_ctx::pf_batch, &ofk_ctx::pf_live, TRACK_LIST(PF_ARRAYS),     // per stream, not per track: a replacement of the tracks re-keys, the filter runs on
     [](ofk_ctx *c, int B) -> int {                              // not started, at zero; an input handed in before the first step stays
         const double zero[3] = {0.0, 0.0, 0.0};
         ofk_launch_pos_filter_clear(c->stream, c->pf_x, c->pf_P, c->pf_ist, c->pf_rec, nullptr, 0, zero, B);
         return OFK_OK;
     },
     nullptr, TS_KEY, "it fuses the keyframe's displacement", nullptr},
    {"ofk_set_stabilise", "ofk_stab_download", "stepped", [](const ofk_ctx *c) { return c->stab.mode != OFK_STAB_OFF; },
     &ofk_ctx::sb_batch, &ofk_ctx::sb_live, TRACK_LIST(SB_ARRAYS),     // per stream, not per track: the view is the identity where the keyframe begins afresh
     [](ofk_ctx *c, int B) -> int { ofk_launch_stab_clear(c->stream, c->sb_Bv, c->sb_ist, c->sb_rec, nullptr, 0, B); c->sb_h = c->sb_w = 0; return OFK_OK; },
     [](ofk_ctx *c, int B) { ofk_launch_stab_clear(c->stream, c->sb_Bv, c->sb_ist, c->sb_rec, c->limit, 0, B); },
     TS_KEY, "it warps into the keyframe's view", nullptr},
};

static void *&track_slot(ofk_ctx *c, const track_array &a) { return *(void **)((char *)c + a.at); }
static void track_free(ofk_ctx *c)
{
    for (const track_state &s : TRACK) if (track_slot(c, s.arrays[0])) hipFree(track_slot(c, s.arrays[0]));
}
// the state's arrays over max_batch streams of max_pts rows, allocated (and cleared) by the first begin or step with the setting on
static int track_alloc(ofk_ctx *c, const track_state &s)
{
    if (track_slot(c, s.arrays[0])) return OFK_OK;
    const size_t np = (size_t)c->max_batch * c->max_pts;
    auto bytes_of = [&](const track_array &a) { return up(np * a.row + c->max_batch * a.stream, 256); };
    size_t bytes = 0;
    for (int i = 0; i < s.narrays; ++i) bytes += bytes_of(s.arrays[i]);
    uint8_t *base = nullptr;
    OFK_HIP(c, hipMalloc((void **)&base, bytes));
    for (int i = 0; i < s.narrays; ++i) { track_slot(c, s.arrays[i]) = base; base += bytes_of(s.arrays[i]); }   // the context owns it from here on
    OFK_HIP(c, hipMemsetAsync(track_slot(c, s.arrays[0]), 0, bytes, c->stream));
    return OFK_OK;
}
// the state for the current tracks of the first B streams: begun afresh unless it is live already
static int track_begin(ofk_ctx *c, const track_state &s, int B)
{
    TRY(track_alloc(c, s));
    if (c->*s.live != B) TRY(s.begin(c, B));
    c->*s.batch = c->*s.live = B;
    return OFK_OK;
}
// The steps' own refusals with a state on (ofk.h), in their precedence; fu: a fused step's.
static int track_check_step(ofk_ctx *c, int variant, const ofk_fusion *fu, const char *who)
{
    static const int order[] = {TS_DEPTH, TS_TEMPLATE, TS_KEYROT, TS_KEYMAP, TS_POSF, TS_STAB, TS_KEY};
    for (int k : order) {
        const track_state &s = TRACK[k];
        if (!s.on(c)) continue;
        if (!TRACK[s.needs].on(c)) return ofk_fail(c, OFK_E_INVALID, "%s: %s is on without %s: %s", who, s.set, TRACK[s.needs].set, s.why);
        if (k == TS_KEYMAP) {                                    // the map is the depths', frozen; the joint solve is not in it
            if (!TRACK[TS_DEPTH].on(c)) return ofk_fail(c, OFK_E_INVALID, "%s: %s is on without %s: the map is the depth state at the keyframe", who, s.set, TRACK[TS_DEPTH].set);
            if (TRACK[TS_KEYROT].on(c)) return ofk_fail(c, OFK_E_INVALID, "%s: %s is on beside %s: the joint solve over map rows is not built", who, s.set, TRACK[TS_KEYROT].set);
        }
        // the homography holds between ideal global-shutter images; ofk_set_rectify puts the lens's map behind it, nothing undoes the shutter
        if (k == TS_STAB && ((camera_on(c) && c->rect.mode == OFK_RECTIFY_OFF) || rs_on(c)))
            return ofk_fail(c, OFK_E_INVALID, "%s: %s is on beside %s: a raw frame needs a remap in front of the warp, which is not built", who, s.set,
                            camera_on(c) && c->rect.mode == OFK_RECTIFY_OFF ? "ofk_set_camera" : "ofk_set_rolling_shutter");
        if (s.model && (variant == OFK_SOLVE_OFMODULE || (fu && (fu->flow == OFK_FLOW_ROTATIONAL || fu->keep == OFK_KEEP_LEGACY))))
            return refuse_not_sensor_model(c, who, NO_OFMODULE | NO_ROTATIONAL | NO_LEGACY, s.model, s.set);
    }
    return OFK_OK;
}
// What a download of a state begins with: refused before any begin or step with the setting on, and for rows without a stride.
static int track_download_begin(ofk_ctx *c, const track_state &s, bool rows, int stride)
{
    if (c->*s.batch < 1 || !track_slot(c, s.arrays[0])) return ofk_fail(c, OFK_E_INVALID, "%s: no stream has %s with %s on yet", s.download, s.began, s.set);
    if (rows && stride < 1) return ofk_fail(c, OFK_E_INVALID, "%s: stride %d", s.download, stride);
    return enter(c);
}
// ... and ends with: per row {dst (NULL: skipped), src, bytes per element}, the first min(stride, max_pts) rows of B streams into a host
// pitch of `stride` elements; pitch != 0: one element per stream out of a device pitch of that many bytes (a record, or its head)
struct download_row { void *dst; const void *src; size_t el, pitch; };
static int rows_download(ofk_ctx *c, int B, int stride, const download_row *rows, int n)
{
    const size_t k = (size_t)(stride < c->max_pts ? stride : c->max_pts), mp = (size_t)c->max_pts;
    for (int i = 0; i < n; ++i) {
        const download_row &r = rows[i];
        if (!r.dst) continue;
        if (!r.pitch) OFK_HIP(c, hipMemcpy2DAsync(r.dst, (size_t)stride * r.el, r.src, mp * r.el, k * r.el, B, hipMemcpyDeviceToHost, c->stream));
        else if (r.pitch == r.el) OFK_HIP(c, hipMemcpyAsync(r.dst, r.src, (size_t)B * r.el, hipMemcpyDeviceToHost, c->stream));
        else OFK_HIP(c, hipMemcpy2DAsync(r.dst, r.el, r.src, r.pitch, r.el, B, hipMemcpyDeviceToHost, c->stream));
    }
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}
// What the stage entries stage on the host and fetch back.  host_buf frees a temporary where its entry returns.
struct host_buf { void *p; ~host_buf() { free(p); } };
// the step's records as the kernels read them: v in slots v0 .. v0 + 2, solved in 15; NULL: out of host memory
static double *stage_step_records(const double *v, const int *solved, size_t B, int v0)
{
    double *h = (double *)calloc(B * OFK_RECORD_DOUBLES, 8);
    for (size_t b = 0; h && b < B; ++b) {
        for (int k = 0; k < 3; ++k) h[b * OFK_RECORD_DOUBLES + v0 + k] = v[3 * b + k];
        h[b * OFK_RECORD_DOUBLES + 15] = solved[b] ? 1.0 : 0.0;
    }
    return h;
}
struct back_row { void *dst; const void *src; size_t bytes; };   // dst NULL: skipped
static int fetch_back(ofk_ctx *c, const char *who, const back_row *rows, int n)
{
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i)
        if (rows[i].dst) e = hipMemcpyAsync(rows[i].dst, rows[i].src, rows[i].bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? OFK_OK : ofk_fail(c, OFK_E_HIP, "%s: download failed: %s", who, hipGetErrorString(e));
}

// ------------------------------------------------------------------------------------------------ track table
static int check_tt(ofk_ctx *c, const ofk_track_table *t, const char *who)
{
    if (t->mode != OFK_TT_OFF && t->mode != OFK_TT_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_TT_OFF nor OFK_TT_ON", who, t->mode);
    if (t->mode == OFK_TT_OFF) return OFK_OK;
    if (t->seed != OFK_TT_SEED_OFF && t->seed != OFK_TT_SEED_FLOW)
        return ofk_fail(c, OFK_E_INVALID, "%s: seed %d is neither OFK_TT_SEED_OFF nor OFK_TT_SEED_FLOW", who, t->seed);
    if (!std::isfinite(t->gain)) return ofk_fail(c, OFK_E_INVALID, "%s: gain = %g must be finite", who, t->gain);
    return OFK_OK;
}

extern "C" int ofk_set_track_table(ofk_ctx *c, const ofk_track_table *t)
{
    return setting_set(c, &ofk_ctx::tt, t && t->mode == OFK_TT_OFF ? nullptr : t, [](ofk_track_table &s) { s.mode = OFK_TT_OFF; },
                       [c](const ofk_track_table *v) { return check_tt(c, v, "ofk_set_track_table"); });
}
extern "C" int ofk_get_track_table(const ofk_ctx *c, ofk_track_table *t) { return setting_get(c, &ofk_ctx::tt, t); }

extern "C" int ofk_track_table_download(ofk_ctx *c, uint32_t *ids, int *age, int *birth_step, float *birth_xy, float *flow_xy, uint32_t *step_ids,
                                        int stride, int *stats)
{
    if (!c) return OFK_E_INVALID;
    TRY(track_download_begin(c, TRACK[TS_TABLE], ids || age || birth_step || birth_xy || flow_xy || step_ids, stride));
    const ofk_tt_rows &t = c->ttr;
    const download_row rows[] = {{ids, t.ids, 4, 0}, {age, t.age, 4, 0}, {birth_step, t.birth_step, 4, 0}, {birth_xy, t.birth_xy, 8, 0},
                                 {flow_xy, t.flow_xy, 8, 0}, {step_ids, t.step_ids, 4, 0}, {stats, t.stats, OFK_TT_STATS * 4, OFK_TT_STATS * 4}};
    return rows_download(c, c->tt_batch, stride, rows, 7);
}

// rules 3 and 6 on host buffers: device scratch only
extern "C" int ofk_track_table_step(ofk_ctx *c, const ofk_track_table *set, uint32_t *ids, int *age, int *birth_step, float *birth_xy, float *flow_xy,
                                    int *head, const float *prev_pts, const float *next_pts, const uint8_t *status, int *counts,
                                    const float *new_pts, const int *new_counts, int max_total, int batch, int stride, uint32_t *step_ids, int *stats)
{
    const char *who = "ofk_track_table_step";
    if (!c) return OFK_E_INVALID;
    if (!ids || !age || !birth_step || !birth_xy || !flow_xy || !head || !prev_pts || !next_pts || !status || !counts)
        return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
    if (batch < 1 || stride < 1) return ofk_fail(c, OFK_E_INVALID, "%s: batch %d / stride %d", who, batch, stride);
    if ((new_pts == nullptr) != (new_counts == nullptr)) return ofk_fail(c, OFK_E_INVALID, "%s: new_pts and new_counts come together", who);
    if (max_total < 0 || max_total > stride) return ofk_fail(c, OFK_E_INVALID, "%s: max_total %d outside 0..%d", who, max_total, stride);
    TRY(check_counts(c, who, counts, batch, stride));
    if (set) TRY(check_tt(c, set, who));
    const size_t np = (size_t)batch * stride;
    Bump bp;
    TRY(est_begin(c, np * 64 + (size_t)batch * 64 + 24 * 256, bp));
    ofk_tt_rows t;
    t.ids = (unsigned *)bp.put(ids, np * 4); t.age = (int *)bp.put(age, np * 4); t.birth_step = (int *)bp.put(birth_step, np * 4);
    t.birth_xy = (float *)bp.put(birth_xy, np * 8); t.flow_xy = (float *)bp.put(flow_xy, np * 8);
    t.step_ids = (unsigned *)bp.take(np * 4); t.head = (int *)bp.put(head, (size_t)batch * 8); t.stats = (int *)bp.take((size_t)batch * OFK_TT_STATS * 4);
    const float *d_prev = (const float *)bp.put(prev_pts, np * 8), *d_next = (const float *)bp.put(next_pts, np * 8);
    const uint8_t *d_st = (const uint8_t *)bp.put(status, np);
    const int *d_cnt = (const int *)bp.put(counts, (size_t)batch * 4);
    const float *d_new = (const float *)bp.put(new_pts, np * 8);
    const int *d_nc = (const int *)bp.put(new_counts, (size_t)batch * 4);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
    OFK_HIP(c, hipMemsetAsync(t.step_ids, 0, np * 4, c->stream));
    const bool seed = set && set->mode != OFK_TT_OFF && set->seed == OFK_TT_SEED_FLOW;
    ofk_launch_track_table_update(c->stream, t, d_prev, d_next, d_st, d_cnt, stride, d_new, d_nc, max_total, seed ? 1 : 0, seed ? (float)set->gain : 0.f, batch);
    TRY(check_launch(c, "k_track_table_update"));
    const host_buf h = {malloc((size_t)batch * OFK_TT_STATS * 4)};
    const int *h_stats = (const int *)h.p;
    if (!h_stats) return ofk_fail(c, OFK_E_INVALID, "%s: out of host memory", who);
    const back_row back[] = {{ids, t.ids, np * 4}, {age, t.age, np * 4}, {birth_step, t.birth_step, np * 4}, {birth_xy, t.birth_xy, np * 8},
        {flow_xy, t.flow_xy, np * 8}, {step_ids, t.step_ids, np * 4}, {head, t.head, (size_t)batch * 8}, {h.p, t.stats, (size_t)batch * OFK_TT_STATS * 4}};
    TRY(fetch_back(c, who, back, 8));
    for (int b = 0; b < batch; ++b) counts[b] = h_stats[(size_t)b * OFK_TT_STATS];
    if (stats) memcpy(stats, h_stats, (size_t)batch * OFK_TT_STATS * 4);
    return OFK_OK;
}

// rule 5 on host buffers: device scratch only
extern "C" int ofk_track_seed_points(ofk_ctx *c, const float *pts, const int *counts, int batch, int stride, const int *age, const float *flow_xy,
                                     double gain, int keep_age0, float *seed_io)
{
    const char *who = "ofk_track_seed_points";
    if (!c) return OFK_E_INVALID;
    if (!pts || !counts || !age || !flow_xy || !seed_io || batch < 1 || stride < 1) return ofk_fail(c, OFK_E_INVALID, "%s: bad argument", who);
    if (!std::isfinite(gain)) return ofk_fail(c, OFK_E_INVALID, "%s: gain = %g must be finite", who, gain);
    TRY(check_counts(c, who, counts, batch, stride));
    const size_t np = (size_t)batch * stride;
    Bump bp;
    TRY(est_begin(c, np * 28 + (size_t)batch * 4 + 8 * 256, bp));
    const float *d_pts = (const float *)bp.put(pts, np * 8), *d_flow = (const float *)bp.put(flow_xy, np * 8);
    float *d_seed = (float *)bp.put(seed_io, np * 8);
    const int *d_age = (const int *)bp.put(age, np * 4), *d_cnt = (const int *)bp.put(counts, (size_t)batch * 4);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
    ofk_launch_track_seed(c->stream, d_pts, d_cnt, stride, d_age, d_flow, (float)gain, keep_age0 ? 1 : 0, d_seed, batch);
    TRY(check_launch(c, "k_track_seed"));
    return get(c, seed_io, d_seed, np * 8);
}

// ------------------------------------------------------------------------------------------------ depth per track
static int check_td(ofk_ctx *c, const ofk_track_depth *t, const char *who)
{
    if (t->mode != OFK_TD_OFF && t->mode != OFK_TD_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_TD_OFF nor OFK_TD_ON", who, t->mode);
    if (t->mode == OFK_TD_OFF) return OFK_OK;
    if (!std::isfinite(t->sigma_flow) || !std::isfinite(t->b_min) || !std::isfinite(t->gate) || !std::isfinite(t->q) || !std::isfinite(t->rel_max))
        return ofk_fail(c, OFK_E_INVALID, "%s: sigma_flow, b_min, gate, q and rel_max must be finite", who);
    if (!(t->sigma_flow > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_flow = %g must be positive", who, t->sigma_flow);
    if (t->b_min < 0.0 || t->gate < 0.0 || t->q < 0.0)
        return ofk_fail(c, OFK_E_INVALID, "%s: b_min = %g, gate = %g and q = %g must not be negative", who, t->b_min, t->gate, t->q);
    if (t->min_obs < 1) return ofk_fail(c, OFK_E_INVALID, "%s: min_obs = %d must be at least 1", who, t->min_obs);
    if (!(t->rel_max > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: rel_max = %g must be positive", who, t->rel_max);
    if (t->min_rows < 3) return ofk_fail(c, OFK_E_INVALID, "%s: min_rows = %d must be at least 3", who, t->min_rows);
    return OFK_OK;
}

extern "C" int ofk_set_track_depth(ofk_ctx *c, const ofk_track_depth *t)
{
    return setting_set(c, &ofk_ctx::td, t && t->mode == OFK_TD_OFF ? nullptr : t, [](ofk_track_depth &s) { s.mode = OFK_TD_OFF; },
                       [c](const ofk_track_depth *v) { return check_td(c, v, "ofk_set_track_depth"); });
}
extern "C" int ofk_get_track_depth(const ofk_ctx *c, ofk_track_depth *t) { return setting_get(c, &ofk_ctx::td, t); }

extern "C" int ofk_track_depth_download(ofk_ctx *c, double *rho, double *var, int *nobs, int stride, double *rec)
{
    if (!c) return OFK_E_INVALID;
    TRY(track_download_begin(c, TRACK[TS_DEPTH], rho || var || nobs, stride));
    const ofk_td_rows &t = c->tdr;
    const download_row rows[] = {{rho, t.rho, 8, 0}, {var, t.var, 8, 0}, {nobs, t.nobs, 4, 0}, {rec, t.rec, OFK_TD_DOUBLES * 8, OFK_TD_DOUBLES * 8}};
    return rows_download(c, c->td_batch, stride, rows, 4);
}

extern "C" int ofk_track_depth_reset(ofk_ctx *c, int b, const double *rho, const double *var, const int *nobs, int n)
{
    const char *who = "ofk_track_depth_reset";
    if (!c) return OFK_E_INVALID;
    if (!rho || !var || !nobs) return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
    if (c->stream_batch < 1 || b < 0 || b >= c->stream_batch) return ofk_fail(c, OFK_E_INVALID, "%s: stream %d is none of the %d active streams", who, b, c->stream_batch);
    if (n < 0 || n > c->max_pts) return ofk_fail(c, OFK_E_INVALID, "%s: n %d outside 0..%d", who, n, c->max_pts);
    for (int i = 0; i < n; ++i)
        if (nobs[i] < 0) return ofk_fail(c, OFK_E_INVALID, "%s: nobs[%d] = %d is negative", who, i, nobs[i]);
    TRY(enter(c));
    TRY(track_begin(c, TRACK[TS_DEPTH], c->stream_batch));
    const size_t o = (size_t)b * c->max_pts;
    if (n) {
        OFK_HIP(c, hipMemcpyAsync(c->tdr.rho + o, rho, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        OFK_HIP(c, hipMemcpyAsync(c->tdr.var + o, var, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        OFK_HIP(c, hipMemcpyAsync(c->tdr.nobs + o, nobs, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    }
    TRY(check_launch(c, who));
    OFK_HIP(c, hipStreamSynchronize(c->stream));                  // the host buffers are the caller's again
    return OFK_OK;
}

// rules 1-4 on host buffers: device scratch only
extern "C" int ofk_track_depth_step(ofk_ctx *c, const ofk_track_depth *set, const double *x, const double *u, const uint8_t *status, const int *counts,
                                    const double *omega, const double *v, const int *solved, double *rho, double *var, int *nobs,
                                    const int *new_counts, int max_total, int batch, int stride, double *rec)
{
    const char *who = "ofk_track_depth_step";
    if (!c) return OFK_E_INVALID;
    if (!set || !x || !u || !status || !counts || !omega || !v || !solved || !rho || !var || !nobs) return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
    if (batch < 1 || stride < 1) return ofk_fail(c, OFK_E_INVALID, "%s: batch %d / stride %d", who, batch, stride);
    if (max_total < 0 || max_total > stride) return ofk_fail(c, OFK_E_INVALID, "%s: max_total %d outside 0..%d", who, max_total, stride);
    if (set->mode == OFK_TD_OFF) return ofk_fail(c, OFK_E_INVALID, "%s: the setting is off", who);
    TRY(check_td(c, set, who));
    TRY(check_counts(c, who, counts, batch, stride));
    const size_t np = (size_t)batch * stride, B = (size_t)batch;
    const host_buf h_rec = {stage_step_records(v, solved, B, 0)};
    if (!h_rec.p) return ofk_fail(c, OFK_E_INVALID, "%s: out of host memory", who);
    Bump bp;
    TRY(est_begin(c, np * 53 + B * (OFK_RECORD_DOUBLES * 8 + OFK_TD_DOUBLES * 8 + 32) + 16 * 256, bp));
    ofk_td_rows t;
    t.rho = bp.put(rho, np * 8); t.var = bp.put(var, np * 8); t.nobs = (int *)bp.put(nobs, np * 4); t.rec = bp.take(B * OFK_TD_DOUBLES * 8);
    ofk_td_in in = {};
    in.x = bp.put(x, np * 16); in.u = bp.put(u, np * 16); in.status = (const uint8_t *)bp.put(status, np);
    in.counts = (const int *)bp.put(counts, B * 4); in.stride = stride;
    in.new_counts = (const int *)bp.put(new_counts, B * 4); in.max_total = max_total;
    in.omega = bp.put(omega, B * 24); in.omega_stride = 3;
    in.v = bp.put(h_rec.p, B * OFK_RECORD_DOUBLES * 8); in.plain = 0;
    if (bp.rc != OFK_OK || hipStreamSynchronize(c->stream) != hipSuccess) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
    ofk_launch_track_depth_step(c->stream, t, in, set, batch);
    TRY(check_launch(c, "k_track_depth_step"));
    const back_row back[] = {{rho, t.rho, np * 8}, {var, t.var, np * 8}, {nobs, t.nobs, np * 4}, {rec, t.rec, B * OFK_TD_DOUBLES * 8}};
    return fetch_back(c, who, back, 4);
}

// ------------------------------------------------------------------------------------------------ track templates
static int check_tpl(ofk_ctx *c, const ofk_track_template *t, const char *who)
{
    if (t->mode != OFK_TPL_OFF && t->mode != OFK_TPL_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_TPL_OFF nor OFK_TPL_ON", who, t->mode);
    if (t->mode == OFK_TPL_OFF) return OFK_OK;
    if (!std::isfinite(t->ncc_min) || !std::isfinite(t->anchor_max) || !std::isfinite(t->fit_gate) || !std::isfinite(t->scale_max))
        return ofk_fail(c, OFK_E_INVALID, "%s: ncc_min, anchor_max, fit_gate and scale_max must be finite", who);
    if (t->win < 5 || t->win > 31 || t->win % 2 == 0) return ofk_fail(c, OFK_E_INVALID, "%s: win = %d must be odd and in 5..31", who, t->win);
    if (t->ncc_min < -1.0 || t->ncc_min > 1.0) return ofk_fail(c, OFK_E_INVALID, "%s: ncc_min = %g outside [-1, 1]", who, t->ncc_min);
    if (t->anchor_iters < 0 || t->anchor_iters > 8) return ofk_fail(c, OFK_E_INVALID, "%s: anchor_iters = %d outside 0..8", who, t->anchor_iters);
    if (!(t->anchor_max > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: anchor_max = %g must be positive", who, t->anchor_max);
    if (t->outside != OFK_TPL_KEEP && t->outside != OFK_TPL_DROP) return ofk_fail(c, OFK_E_INVALID, "%s: outside = %d is neither OFK_TPL_KEEP nor OFK_TPL_DROP", who, t->outside);
    if (t->fit_min < 3) return ofk_fail(c, OFK_E_INVALID, "%s: fit_min = %d must be at least 3", who, t->fit_min);
    if (t->fit_gate < 0.0) return ofk_fail(c, OFK_E_INVALID, "%s: fit_gate = %g must not be negative (0: a single fit)", who, t->fit_gate);
    if (t->scale_max != 0.0 && !(t->scale_max >= 1.0)) return ofk_fail(c, OFK_E_INVALID, "%s: scale_max = %g is neither 0 (never refresh) nor >= 1", who, t->scale_max);
    return OFK_OK;
}

extern "C" int ofk_set_track_template(ofk_ctx *c, const ofk_track_template *t)
{
    const int rc = setting_set(c, &ofk_ctx::tpl, t && t->mode == OFK_TPL_OFF ? nullptr : t, [](ofk_track_template &s) { s.mode = OFK_TPL_OFF; },
                               [c](const ofk_track_template *v) { return check_tpl(c, v, "ofk_set_track_template"); });
    if (c && rc == OFK_OK) c->tp_live = 0;                       // templates of another window are no templates: the next step starts over
    return rc;
}
extern "C" int ofk_get_track_template(const ofk_ctx *c, ofk_track_template *t) { return setting_get(c, &ofk_ctx::tpl, t); }

extern "C" int ofk_track_template_download(ofk_ctx *c, uint8_t *tmpl, float *A, float *ncc, uint8_t *flag, uint8_t *tstate, int stride, double *rec)
{
    if (!c) return OFK_E_INVALID;
    TRY(track_download_begin(c, TRACK[TS_TEMPLATE], tmpl || A || ncc || flag || tstate, stride));
    const ofk_tp_rows &t = c->tpr;
    if (tmpl && tp_stride_of(c->tpl.win) != t.tstride)
        return ofk_fail(c, OFK_E_INVALID, "ofk_track_template_download: the window was set to %d behind the latest step: its templates are gone", c->tpl.win);
    const download_row rows[] = {{tmpl, t.tmpl[t.cur], (size_t)t.tstride, 0}, {A, t.A, 16, 0}, {ncc, t.ncc, 4, 0}, {flag, t.flag, 1, 0}, {tstate, t.tstate, 1, 0},
                                 {rec, t.rec, OFK_TPL_DOUBLES * 8, OFK_TPL_DOUBLES * 8}};
    return rows_download(c, c->tp_batch, stride, rows, 6);
}

// rule 1 on host buffers: device scratch only
extern "C" int ofk_track_affine_fit(ofk_ctx *c, const ofk_track_template *set, const float *prev_pts, const float *next_pts, const uint8_t *status,
                                    const int *counts, int batch, int stride, int h, int w, double *rec, float *L)
{
    const char *who = "ofk_track_affine_fit";
    if (!c) return OFK_E_INVALID;
    if (!set || !prev_pts || !next_pts || !status || !counts || !rec) return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
    if (batch < 1 || stride < 1 || h < 1 || w < 1) return ofk_fail(c, OFK_E_INVALID, "%s: batch %d / stride %d / frame %d x %d", who, batch, stride, w, h);
    if (set->mode == OFK_TPL_OFF) return ofk_fail(c, OFK_E_INVALID, "%s: the setting is off", who);
    TRY(check_tpl(c, set, who));
    TRY(check_counts(c, who, counts, batch, stride));
    const size_t np = (size_t)batch * stride, B = (size_t)batch;
    Bump bp;
    TRY(est_begin(c, np * 17 + B * (4 + 16 + OFK_TPL_DOUBLES * 8) + 8 * 256, bp));
    const float *d_prev = (const float *)bp.put(prev_pts, np * 8), *d_next = (const float *)bp.put(next_pts, np * 8);
    const uint8_t *d_st = (const uint8_t *)bp.put(status, np);
    const int *d_cnt = (const int *)bp.put(counts, B * 4);
    float *d_L = (float *)bp.take(B * 16);
    double *d_rec = bp.take(B * OFK_TPL_DOUBLES * 8);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
    OFK_HIP(c, hipMemsetAsync(d_rec, 0, B * OFK_TPL_DOUBLES * 8, c->stream));
    ofk_launch_track_affine(c->stream, d_prev, d_next, d_st, d_cnt, stride, h, w, set, d_L, d_rec, batch);
    TRY(check_launch(c, "k_track_affine"));
    if (L) OFK_HIP(c, hipMemcpyAsync(L, d_L, B * 16, hipMemcpyDeviceToHost, c->stream));
    return get(c, rec, d_rec, B * OFK_TPL_DOUBLES * 8);
}

// rules 2-6 on host buffers: device scratch only
extern "C" int ofk_track_template_step(ofk_ctx *c, const ofk_track_template *set, const uint8_t *prev, const uint8_t *next, int h, int w,
                                       const float *prev_pts, float *next_pts, uint8_t *status, const int *age, const int *counts, const float *L,
                                       uint8_t *tmpl, float *A, float *ncc, uint8_t *flag, uint8_t *tstate, const int *new_counts, int max_total,
                                       int batch, int stride, double *rec)
{
    const char *who = "ofk_track_template_step";
    if (!c) return OFK_E_INVALID;
    if (!set || !prev || !next || !prev_pts || !next_pts || !status || !age || !counts || !L || !tmpl || !A || !ncc || !flag || !tstate)
        return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
    if (batch < 1 || stride < 1 || h < 2 || w < 2) return ofk_fail(c, OFK_E_INVALID, "%s: batch %d / stride %d / frame %d x %d", who, batch, stride, w, h);
    if (max_total < 0 || max_total > stride) return ofk_fail(c, OFK_E_INVALID, "%s: max_total %d outside 0..%d", who, max_total, stride);
    if (set->mode == OFK_TPL_OFF) return ofk_fail(c, OFK_E_INVALID, "%s: the setting is off", who);
    TRY(check_tpl(c, set, who));
    TRY(check_counts(c, who, counts, batch, stride));
    const size_t np = (size_t)batch * stride, B = (size_t)batch, px = (size_t)h * w, ts = (size_t)tp_stride_of(set->win);
    Bump bp;
    TRY(est_begin(c, 2 * up(B * px, 256) + np * (2 * ts + 2 * 16 + 3 * 4 + 3 + 2 * 8 + 1 + 4) + B * (4 + 4 + 16 + OFK_TPL_DOUBLES * 8) + 24 * 256, bp));
    const uint8_t *d_prev = (const uint8_t *)bp.put(prev, B * px), *d_next = (const uint8_t *)bp.put(next, B * px);
    ofk_tp_rows t = {};
    t.tmpl[0] = (uint8_t *)bp.put(tmpl, np * ts); t.tmpl[1] = (uint8_t *)bp.take(np * ts); t.cur = 0; t.tstride = (int)ts;
    t.A = (float *)bp.put(A, np * 16); t.A_new = (float *)bp.take(np * 16);
    t.ncc = (float *)bp.put(ncc, np * 4); t.ncc_new = (float *)bp.take(np * 4); t.move = (float *)bp.take(np * 4);
    t.flag = (uint8_t *)bp.put(flag, np); t.flag_new = (uint8_t *)bp.take(np); t.tstate = (uint8_t *)bp.put(tstate, np);
    t.L = (float *)bp.put(L, B * 16); t.rec = bp.take(B * OFK_TPL_DOUBLES * 8);
    const float *d_pp = (const float *)bp.put(prev_pts, np * 8);
    float *d_np = (float *)bp.put(next_pts, np * 8);
    uint8_t *d_st = (uint8_t *)bp.put(status, np);
    const int *d_age = (const int *)bp.put(age, np * 4), *d_cnt = (const int *)bp.put(counts, B * 4), *d_nc = (const int *)bp.put(new_counts, B * 4);
    if (bp.rc) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
    OFK_HIP(c, hipMemsetAsync(t.rec, 0, B * OFK_TPL_DOUBLES * 8, c->stream));
    OFK_HIP(c, hipMemcpyAsync(t.tmpl[1], t.tmpl[0], np * ts, hipMemcpyDeviceToDevice, c->stream));   // rows beyond the kept ones come back as they went in
    ofk_launch_track_template(c->stream, t, d_prev, d_next, px, h, w, d_pp, d_np, d_st, d_age, d_cnt, stride, set, batch);
    ofk_launch_track_template_update(c->stream, t, d_st, d_cnt, stride, d_nc, max_total, set, batch);
    TRY(check_launch(c, "k_track_template"));
    const back_row back[] = {{next_pts, d_np, np * 8}, {status, d_st, np}, {tmpl, t.tmpl[1], np * ts}, {A, t.A, np * 16}, {ncc, t.ncc, np * 4}, {flag, t.flag, np},
                             {tstate, t.tstate, np}, {rec, t.rec, B * OFK_TPL_DOUBLES * 8}};
    return fetch_back(c, who, back, 8);
}

// ------------------------------------------------------------------------------------------------ keyframe per stream
static int check_key(ofk_ctx *c, const ofk_keyframe *k, const char *who)
{
    if (k->mode != OFK_KEY_OFF && k->mode != OFK_KEY_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_KEY_OFF nor OFK_KEY_ON", who, k->mode);
    if (k->mode == OFK_KEY_OFF) return OFK_OK;
    if (!std::isfinite(k->sigma_flow) || !std::isfinite(k->gate) || !std::isfinite(k->min_share) || !std::isfinite(k->rot_max))
        return ofk_fail(c, OFK_E_INVALID, "%s: sigma_flow, gate, min_share and rot_max must be finite", who);
    if (!(k->sigma_flow > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_flow = %g must be positive", who, k->sigma_flow);
    if (k->gate < 0.0) return ofk_fail(c, OFK_E_INVALID, "%s: gate = %g must not be negative", who, k->gate);
    if (k->min_rows < 3) return ofk_fail(c, OFK_E_INVALID, "%s: min_rows = %d must be at least 3", who, k->min_rows);
    if (k->min_share < 0.0 || k->min_share > 1.0) return ofk_fail(c, OFK_E_INVALID, "%s: min_share = %g outside [0, 1]", who, k->min_share);
    if (!(k->rot_max > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: rot_max = %g must be positive", who, k->rot_max);
    if (k->max_age < 0) return ofk_fail(c, OFK_E_INVALID, "%s: max_age = %d must not be negative", who, k->max_age);
    return OFK_OK;
}

extern "C" int ofk_set_keyframe(ofk_ctx *c, const ofk_keyframe *k)
{
    return setting_set(c, &ofk_ctx::key, k && k->mode == OFK_KEY_OFF ? nullptr : k, [](ofk_keyframe &s) { s.mode = OFK_KEY_OFF; },
                       [c](const ofk_keyframe *v) { return check_key(c, v, "ofk_set_keyframe"); });
}
extern "C" int ofk_get_keyframe(const ofk_ctx *c, ofk_keyframe *k) { return setting_get(c, &ofk_ctx::key, k); }

// the keyframe's rotation (ofk.h: ofk_set_keyframe_rotation)
static int check_keyrot(ofk_ctx *c, const ofk_keyframe_rotation *r, const char *who)
{
    if (r->mode != OFK_KEYROT_OFF && r->mode != OFK_KEYROT_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_KEYROT_OFF nor OFK_KEYROT_ON", who, r->mode);
    if (r->mode == OFK_KEYROT_OFF) return OFK_OK;
    if (r->source != OFK_KEYROT_GYRO && r->source != OFK_KEYROT_ATTITUDE)
        return ofk_fail(c, OFK_E_INVALID, "%s: source %d is neither OFK_KEYROT_GYRO nor OFK_KEYROT_ATTITUDE", who, r->source);
    if (!(r->sigma_gyro >= 0.0) || !(r->sigma_bias >= 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_gyro and sigma_bias must not be negative or NaN", who);
    if (!(r->sigma_att >= 0.0) || !std::isfinite(r->sigma_att)) return ofk_fail(c, OFK_E_INVALID, "%s: sigma_att = %g must be finite and not negative", who, r->sigma_att);
    if (r->iters < 1 || r->iters > OFK_KEYROT_MAX_ITERS) return ofk_fail(c, OFK_E_INVALID, "%s: iters = %d outside 1..%d", who, r->iters, OFK_KEYROT_MAX_ITERS);
    if (!(r->delta_max > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: delta_max = %g must be positive", who, r->delta_max);
    return OFK_OK;
}

extern "C" int ofk_set_keyframe_rotation(ofk_ctx *c, const ofk_keyframe_rotation *r)
{
    return setting_set(c, &ofk_ctx::krot, r && r->mode == OFK_KEYROT_OFF ? nullptr : r, [](ofk_keyframe_rotation &s) { s.mode = OFK_KEYROT_OFF; },
                       [c](const ofk_keyframe_rotation *v) { return check_keyrot(c, v, "ofk_set_keyframe_rotation"); });
}
extern "C" int ofk_get_keyframe_rotation(const ofk_ctx *c, ofk_keyframe_rotation *r) { return setting_get(c, &ofk_ctx::krot, r); }

// every axis held by the setting alone: the plain kernel runs (ofk.h)
static bool kr_all_held(const ofk_keyframe_rotation *r)
{
    if (!r->axes[0] && !r->axes[1] && !r->axes[2]) return true;
    return r->source == OFK_KEYROT_ATTITUDE ? r->sigma_att == 0.0 : r->sigma_gyro == 0.0 && r->sigma_bias == 0.0;
}
// the keyframe's map (ofk.h: ofk_set_keyframe_map)
static int check_keymap(ofk_ctx *c, const ofk_keyframe_map *m, const char *who)
{
    if (m->mode != OFK_KEYMAP_OFF && m->mode != OFK_KEYMAP_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_KEYMAP_OFF nor OFK_KEYMAP_ON", who, m->mode);
    if (m->mode == OFK_KEYMAP_OFF) return OFK_OK;
    if (!std::isfinite(m->rel_max) || !std::isfinite(m->ready_share)) return ofk_fail(c, OFK_E_INVALID, "%s: rel_max and ready_share must be finite", who);
    if (m->min_obs < 1) return ofk_fail(c, OFK_E_INVALID, "%s: min_obs = %d must be at least 1", who, m->min_obs);
    if (!(m->rel_max > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: rel_max = %g must be positive", who, m->rel_max);
    if (m->min_rows < 3) return ofk_fail(c, OFK_E_INVALID, "%s: min_rows = %d must be at least 3", who, m->min_rows);
    if (m->ready_share < 0.0 || m->ready_share > 1.0) return ofk_fail(c, OFK_E_INVALID, "%s: ready_share = %g outside [0, 1]", who, m->ready_share);
    if (m->weights != 0 && m->weights != 1) return ofk_fail(c, OFK_E_INVALID, "%s: weights = %d is neither 0 nor 1", who, m->weights);
    return OFK_OK;
}

extern "C" int ofk_set_keyframe_map(ofk_ctx *c, const ofk_keyframe_map *m)
{
    return setting_set(c, &ofk_ctx::kmap, m && m->mode == OFK_KEYMAP_OFF ? nullptr : m, [](ofk_keyframe_map &s) { s.mode = OFK_KEYMAP_OFF; },
                       [c](const ofk_keyframe_map *v) { return check_keymap(c, v, "ofk_set_keyframe_map"); });
}
extern "C" int ofk_get_keyframe_map(const ofk_ctx *c, ofk_keyframe_map *m) { return setting_get(c, &ofk_ctx::kmap, m); }

// the launch of rules 1-5: k_keyframe_step, or with the rotation on (r, not all held) k_keyframe_step_rot in its place, or with the
// map on (m, mr; never beside r) k_keyframe_step_map
static void launch_key_step(ofk_ctx *c, const ofk_kf_rows &t, const ofk_kf_in &in, const ofk_keyframe *k, const ofk_keyframe_rotation *r,
                            double *rst, double *rrec, int batch, const ofk_keyframe_map *m = nullptr, const ofk_km_rows *mr = nullptr)
{
    if (m) { ofk_launch_keyframe_step_map(c->stream, t, in, k, m, *mr, batch); return; }
    if (!r) { ofk_launch_keyframe_step(c->stream, t, in, k, batch); return; }
    if (kr_all_held(r)) {
        ofk_launch_keyframe_step(c->stream, t, in, k, batch);
        ofk_launch_keyrot_clear(c->stream, nullptr, rrec, nullptr, 0, OFK_KEYROT_HELD, batch);
        return;
    }
    ofk_launch_keyframe_step_rot(c->stream, t, in, k, r, rst, rrec, batch);
}

extern "C" int ofk_keyframe_rotation_download(ofk_ctx *c, double *rec)
{
    if (!c) return OFK_E_INVALID;
    TRY(track_download_begin(c, TRACK[TS_KEYROT], false, 0));
    if (!rec) return ofk_fail(c, OFK_E_INVALID, "ofk_keyframe_rotation_download: NULL argument");
    const download_row row = {rec, c->kr_rec, OFK_KEYROT_DOUBLES * 8, OFK_KEYROT_DOUBLES * 8};
    return rows_download(c, c->kr_batch, 0, &row, 1);
}

extern "C" int ofk_keyframe_map_download(ofk_ctx *c, double *key_rho, double *key_var, int stride, double *rec)
{
    if (!c) return OFK_E_INVALID;
    TRY(track_download_begin(c, TRACK[TS_KEYMAP], key_rho || key_var, stride));
    const download_row rows[] = {{key_rho, c->kmr.key_rho, 8, 0}, {key_var, c->kmr.key_var, 8, 0},
                                 {rec, c->kmr.mrec, OFK_KEYMAP_DOUBLES * 8, OFK_KEYMAP_DOUBLES * 8}};
    return rows_download(c, c->km_batch, stride, rows, 3);
}

extern "C" int ofk_keyframe_download(ofk_ctx *c, float *key_xy, uint8_t *member, int stride, double *R_acc, double *rec)
{
    if (!c) return OFK_E_INVALID;
    TRY(track_download_begin(c, TRACK[TS_KEY], key_xy || member, stride));
    const ofk_kf_rows &t = c->kfr;
    const download_row rows[] = {{key_xy, t.key_xy, 8, 0}, {member, t.member, 1, 0}, {R_acc, t.st, 72, OFK_KEY_STATE * 8},
                                 {rec, t.rec, OFK_KEY_DOUBLES * 8, OFK_KEY_DOUBLES * 8}};
    return rows_download(c, c->kf_batch, stride, rows, 4);
}

extern "C" int ofk_keyframe_reset(ofk_ctx *c, int b, const double *anchor)
{
    const char *who = "ofk_keyframe_reset";
    if (!c) return OFK_E_INVALID;
    if (c->stream_batch < 1 || b < 0 || b >= c->stream_batch) return ofk_fail(c, OFK_E_INVALID, "%s: stream %d is none of the %d active streams", who, b, c->stream_batch);
    const double zero[3] = {0.0, 0.0, 0.0}, *p = anchor ? anchor : zero;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return ofk_fail(c, OFK_E_INVALID, "%s: the position must be finite", who);
    TRY(enter(c));
    TRY(track_begin(c, TRACK[TS_KEY], c->stream_batch));
    ofk_launch_keyframe_reset(c->stream, c->kfr, b, c->max_pts, p);
    if (c->kr_st && c->kr_live == c->stream_batch) ofk_launch_keyrot_clear(c->stream, c->kr_st, c->kr_rec, nullptr, b, OFK_KEYROT_NONE, 1);
    if (c->kmr.key_rho && c->km_live == c->stream_batch) ofk_launch_keymap_clear(c->stream, c->kmr, c->kfr.ist, nullptr, nullptr, c->max_pts, b, 0, 1);
    TRY(check_launch(c, who));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

// what ofk_keyframe_map_step adds to ofk_keyframe_step's arguments
struct host_map { const ofk_keyframe_map *set; const double *rho, *var; const int *nobs; double *key_rho, *key_var; int *mstate; double *mrec; };
// rules 1-5 on host buffers: device scratch only; rot != NULL: with the rotation's rule 2 (rstate in and out, rrec out); hm != NULL:
// with the map's rules M1-M5 (never beside rot)
static int keyframe_step_host(ofk_ctx *c, const char *who, const ofk_keyframe *set, const ofk_keyframe_rotation *rot, const float *next_pts,
                              const uint8_t *status, const int *counts, const double *sensors, const double *v_uav, const int *solved,
                              const int *step, float *key_xy, uint8_t *member, double *state, int *istate, const int *new_counts, int max_total,
                              int batch, int stride, double *rec, double *rstate, double *rrec, const host_map *hm = nullptr)
{
    if (!set || !next_pts || !status || !counts || !sensors || !v_uav || !solved || !step || !key_xy || !member || !state || !istate)
        return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
    if (batch < 1 || stride < 1) return ofk_fail(c, OFK_E_INVALID, "%s: batch %d / stride %d", who, batch, stride);
    if (max_total < 0 || max_total > stride) return ofk_fail(c, OFK_E_INVALID, "%s: max_total %d outside 0..%d", who, max_total, stride);
    if (set->mode == OFK_KEY_OFF) return ofk_fail(c, OFK_E_INVALID, "%s: the setting is off", who);
    TRY(check_key(c, set, who));
    if (rot) {
        if (!rstate) return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
        if (rot->mode == OFK_KEYROT_OFF) return ofk_fail(c, OFK_E_INVALID, "%s: the rotation setting is off", who);
        TRY(check_keyrot(c, rot, who));
    }
    if (hm) {
        if (!hm->set || !hm->key_rho || !hm->key_var || !hm->mstate) return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
        if ((hm->rho == nullptr) != (hm->var == nullptr) || (hm->rho == nullptr) != (hm->nobs == nullptr))
            return ofk_fail(c, OFK_E_INVALID, "%s: rho, var and nobs come together", who);
        if (hm->set->mode == OFK_KEYMAP_OFF) return ofk_fail(c, OFK_E_INVALID, "%s: the map setting is off", who);
        TRY(check_keymap(c, hm->set, who));
    }
    TRY(check_counts(c, who, counts, batch, stride));
    const size_t np = (size_t)batch * stride, B = (size_t)batch;
    const host_buf h_rec = {stage_step_records(v_uav, solved, B, 8)};
    if (!h_rec.p) return ofk_fail(c, OFK_E_INVALID, "%s: out of host memory", who);
    Bump bp;
    TRY(est_begin(c, np * (18 + (hm ? 36 : 0)) + B * ((OFK_RECORD_DOUBLES + OFK_KEY_DOUBLES + OFK_KEY_STATE + OFK_SENSOR_DOUBLES + OFK_KEYROT_STATE + OFK_KEYROT_DOUBLES + OFK_KEYMAP_DOUBLES) * 8 + OFK_KEY_INTS * 4 + 20) + 26 * 256, bp));
    ofk_kf_rows t = {};
    t.key_xy = (float *)bp.put(key_xy, np * 8); t.member = (uint8_t *)bp.put(member, np); t.st = bp.put(state, B * OFK_KEY_STATE * 8);
    t.ist = (int *)bp.put(istate, B * OFK_KEY_INTS * 4); t.rec = bp.take(B * OFK_KEY_DOUBLES * 8);
    ofk_kf_in in = {};
    in.next_pts = (const float *)bp.put(next_pts, np * 8); in.status = (const uint8_t *)bp.put(status, np);
    in.counts = (const int *)bp.put(counts, B * 4); in.stride = stride;
    in.new_counts = (const int *)bp.put(new_counts, B * 4); in.max_total = max_total;
    in.sensors = bp.put(sensors, B * OFK_SENSOR_DOUBLES * 8); in.imu = nullptr;
    in.v = bp.put(h_rec.p, B * OFK_RECORD_DOUBLES * 8); in.plain = 0;
    in.step = (const int *)bp.put(step, B * 4); in.step_stride = 1;
    double *d_rst = rot ? bp.put(rstate, B * OFK_KEYROT_STATE * 8) : nullptr, *d_rrec = rot ? bp.take(B * OFK_KEYROT_DOUBLES * 8) : nullptr;
    ofk_km_rows mr = {};
    if (hm) {
        mr.key_rho = bp.put(hm->key_rho, np * 8); mr.key_var = bp.put(hm->key_var, np * 8); mr.mstate = (int *)bp.put(hm->mstate, B * 8);
        mr.mrec = bp.take(B * OFK_KEYMAP_DOUBLES * 8);
        mr.rho = bp.put(hm->rho, np * 8); mr.var = bp.put(hm->var, np * 8); mr.nobs = (const int *)bp.put(hm->nobs, np * 4);
    }
    if (bp.rc != OFK_OK || hipStreamSynchronize(c->stream) != hipSuccess) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
    launch_key_step(c, t, in, set, rot, d_rst, d_rrec, batch, hm ? hm->set : nullptr, &mr);
    TRY(check_launch(c, hm ? "k_keyframe_step_map" : rot ? "k_keyframe_step_rot" : "k_keyframe_step"));
    const back_row back[] = {{hm ? hm->key_rho : nullptr, mr.key_rho, np * 8}, {hm ? hm->key_var : nullptr, mr.key_var, np * 8},
                             {hm ? hm->mstate : nullptr, mr.mstate, B * 8}, {hm ? hm->mrec : nullptr, mr.mrec, B * OFK_KEYMAP_DOUBLES * 8},
                             {rot ? rstate : nullptr, d_rst, B * OFK_KEYROT_STATE * 8}, {rot ? rrec : nullptr, d_rrec, B * OFK_KEYROT_DOUBLES * 8},
                             {key_xy, t.key_xy, np * 8}, {member, t.member, np}, {state, t.st, B * OFK_KEY_STATE * 8}, {istate, t.ist, B * OFK_KEY_INTS * 4},
                             {rec, t.rec, B * OFK_KEY_DOUBLES * 8}};
    return fetch_back(c, who, back, 11);
}

extern "C" int ofk_keyframe_step(ofk_ctx *c, const ofk_keyframe *set, const float *next_pts, const uint8_t *status, const int *counts,
                                 const double *sensors, const double *v_uav, const int *solved, const int *step, float *key_xy, uint8_t *member,
                                 double *state, int *istate, const int *new_counts, int max_total, int batch, int stride, double *rec)
{
    if (!c) return OFK_E_INVALID;
    return keyframe_step_host(c, "ofk_keyframe_step", set, nullptr, next_pts, status, counts, sensors, v_uav, solved, step, key_xy, member, state,
                              istate, new_counts, max_total, batch, stride, rec, nullptr, nullptr);
}

extern "C" int ofk_keyframe_rotation_step(ofk_ctx *c, const ofk_keyframe *set, const ofk_keyframe_rotation *rot, const float *next_pts,
                                          const uint8_t *status, const int *counts, const double *sensors, const double *v_uav,
                                          const int *solved, const int *step, float *key_xy, uint8_t *member, double *state, int *istate,
                                          const int *new_counts, int max_total, int batch, int stride, double *rec, double *rstate, double *rrec)
{
    if (!c) return OFK_E_INVALID;
    if (!rot) return ofk_fail(c, OFK_E_INVALID, "ofk_keyframe_rotation_step: NULL argument");
    return keyframe_step_host(c, "ofk_keyframe_rotation_step", set, rot, next_pts, status, counts, sensors, v_uav, solved, step, key_xy, member,
                              state, istate, new_counts, max_total, batch, stride, rec, rstate, rrec);
}

extern "C" int ofk_keyframe_map_step(ofk_ctx *c, const ofk_keyframe *set, const ofk_keyframe_map *map, const float *next_pts, const uint8_t *status,
                                     const int *counts, const double *sensors, const double *v_uav, const int *solved, const int *step,
                                     float *key_xy, uint8_t *member, double *state, int *istate, const int *new_counts, int max_total, int batch,
                                     int stride, double *rec, const double *rho, const double *var, const int *nobs, double *key_rho,
                                     double *key_var, int *mstate, double *mrec)
{
    if (!c) return OFK_E_INVALID;
    const host_map hm = {map, rho, var, nobs, key_rho, key_var, mstate, mrec};
    return keyframe_step_host(c, "ofk_keyframe_map_step", set, nullptr, next_pts, status, counts, sensors, v_uav, solved, step, key_xy, member,
                              state, istate, new_counts, max_total, batch, stride, rec, nullptr, nullptr, &hm);
}

// ------------------------------------------------------------------------------------------------ position filter
static int check_posf(ofk_ctx *c, const ofk_pos_filter *f, const char *who)
{
    if (f->mode != OFK_POSF_OFF && f->mode != OFK_POSF_ON) return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is neither OFK_POSF_OFF nor OFK_POSF_ON", who, f->mode);
    if (f->mode == OFK_POSF_OFF) return OFK_OK;
    const double all[] = {f->dt, f->sigma_v, f->floor, f->infl, f->share, f->q_p, f->q_v, f->q_b, f->p0_p, f->p0_v, f->p0_b, f->nis_max};
    if (!all_finite(all, sizeof all / 8)) return ofk_fail(c, OFK_E_INVALID, "%s: every field must be finite", who);
    if (!(f->dt > 0.0) || !(f->infl > 0.0)) return ofk_fail(c, OFK_E_INVALID, "%s: dt = %g and infl = %g must be positive", who, f->dt, f->infl);
    if (f->sigma_v < 0.0 || f->floor < 0.0 || f->q_p < 0.0 || f->q_v < 0.0 || f->q_b < 0.0 || f->p0_p < 0.0 || f->p0_v < 0.0 || f->p0_b < 0.0)
        return ofk_fail(c, OFK_E_INVALID, "%s: sigma_v, floor, q_* and p0_* must not be negative", who);
    if (f->share < 0.0 || f->share > 1.0) return ofk_fail(c, OFK_E_INVALID, "%s: share = %g outside [0, 1]", who, f->share);
    if (f->nis_max < 0.0) return ofk_fail(c, OFK_E_INVALID, "%s: nis_max = %g must not be negative", who, f->nis_max);
    return OFK_OK;
}

extern "C" int ofk_set_pos_filter(ofk_ctx *c, const ofk_pos_filter *f)
{
    return setting_set(c, &ofk_ctx::posf, f && f->mode == OFK_POSF_OFF ? nullptr : f, [](ofk_pos_filter &s) { s.mode = OFK_POSF_OFF; },
                       [c](const ofk_pos_filter *v) { return check_posf(c, v, "ofk_set_pos_filter"); });
}
extern "C" int ofk_get_pos_filter(const ofk_ctx *c, ofk_pos_filter *f) { return setting_get(c, &ofk_ctx::posf, f); }

extern "C" int ofk_pos_filter_input(ofk_ctx *c, const double *input)
{
    const char *who = "ofk_pos_filter_input";
    if (!c) return OFK_E_INVALID;
    if (c->stream_batch < 1) return ofk_fail(c, OFK_E_INVALID, "%s: no active streams", who);
    if (!input) return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
    TRY(enter(c));
    TRY(track_alloc(c, TRACK[TS_POSF]));
    OFK_HIP(c, hipMemcpyAsync(c->pf_in, input, (size_t)c->stream_batch * OFK_POSF_INPUT * 8, hipMemcpyHostToDevice, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

extern "C" int ofk_pos_filter_reset(ofk_ctx *c, int b, const double *pos)
{
    const char *who = "ofk_pos_filter_reset";
    if (!c) return OFK_E_INVALID;
    if (c->stream_batch < 1 || b < 0 || b >= c->stream_batch) return ofk_fail(c, OFK_E_INVALID, "%s: stream %d is none of the %d active streams", who, b, c->stream_batch);
    const double zero[3] = {0.0, 0.0, 0.0}, *p = pos ? pos : zero;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return ofk_fail(c, OFK_E_INVALID, "%s: the position must be finite", who);
    TRY(enter(c));
    TRY(track_begin(c, TRACK[TS_POSF], c->stream_batch));
    ofk_launch_pos_filter_clear(c->stream, c->pf_x, c->pf_P, c->pf_ist, c->pf_rec, c->pf_in, b, p, 1);
    TRY(check_launch(c, who));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

extern "C" int ofk_pos_filter_download(ofk_ctx *c, double *x, double *P, int *istate, double *rec)
{
    if (!c) return OFK_E_INVALID;
    TRY(track_download_begin(c, TRACK[TS_POSF], false, 0));
    const download_row rows[] = {{x, c->pf_x, OFK_POSF_STATES * 8, OFK_POSF_STATES * 8},
                                 {P, c->pf_P, OFK_POSF_STATES * OFK_POSF_STATES * 8, OFK_POSF_STATES * OFK_POSF_STATES * 8},
                                 {istate, c->pf_ist, OFK_POSF_INTS * 4, OFK_POSF_INTS * 4}, {rec, c->pf_rec, OFK_POSF_DOUBLES * 8, OFK_POSF_DOUBLES * 8}};
    return rows_download(c, c->pf_batch, 0, rows, 4);
}

// rules 1-8 on host buffers: device scratch only
extern "C" int ofk_pos_filter_step(ofk_ctx *c, const ofk_pos_filter *f, const double *v_uav, const int *solved, const double *key_rec,
                                   const double *R_world, const double *input, double *x, double *P, int *istate, int batch, double *rec)
{
    const char *who = "ofk_pos_filter_step";
    if (!c) return OFK_E_INVALID;
    if (!f || !v_uav || !solved || !key_rec || !R_world || !x || !P || !istate) return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
    if (batch < 1) return ofk_fail(c, OFK_E_INVALID, "%s: batch %d", who, batch);
    if (f->mode == OFK_POSF_OFF) return ofk_fail(c, OFK_E_INVALID, "%s: the setting is off", who);
    TRY(check_posf(c, f, who));
    const size_t B = (size_t)batch, NN = OFK_POSF_STATES * OFK_POSF_STATES;
    const host_buf h_rec = {stage_step_records(v_uav, solved, B, 8)};
    if (!h_rec.p) return ofk_fail(c, OFK_E_INVALID, "%s: out of host memory", who);
    Bump bp;
    TRY(est_begin(c, B * ((OFK_RECORD_DOUBLES + OFK_KEY_DOUBLES + 9 + OFK_POSF_INPUT + OFK_POSF_STATES + NN + OFK_POSF_DOUBLES) * 8 + OFK_POSF_INTS * 4) + 9 * 256, bp));
    const double *d_v = bp.put(h_rec.p, B * OFK_RECORD_DOUBLES * 8), *d_key = bp.put(key_rec, B * OFK_KEY_DOUBLES * 8), *d_rw = bp.put(R_world, B * 72);
    double *d_in = input ? bp.put(input, B * OFK_POSF_INPUT * 8) : bp.take(B * OFK_POSF_INPUT * 8);
    double *d_x = bp.put(x, B * OFK_POSF_STATES * 8), *d_P = bp.put(P, B * NN * 8), *d_rec = bp.take(B * OFK_POSF_DOUBLES * 8);
    int *d_ist = (int *)bp.put(istate, B * OFK_POSF_INTS * 4);
    if (!input && bp.rc == OFK_OK && hipMemsetAsync(d_in, 0, B * OFK_POSF_INPUT * 8, c->stream) != hipSuccess) bp.rc = OFK_E_HIP;
    if (bp.rc != OFK_OK || hipStreamSynchronize(c->stream) != hipSuccess) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
    ofk_launch_pos_filter_step(c->stream, f, d_x, d_P, d_ist, d_rec, d_in, d_v, 0, d_key, d_rw, 9, batch);
    TRY(check_launch(c, "k_pos_filter_step"));
    const back_row back[] = {{x, d_x, B * OFK_POSF_STATES * 8}, {P, d_P, B * NN * 8}, {istate, d_ist, B * OFK_POSF_INTS * 4}, {rec, d_rec, B * OFK_POSF_DOUBLES * 8}};
    return fetch_back(c, who, back, 4);
}

// ------------------------------------------------------------------------------------------------ stabilised view
static int check_stab(ofk_ctx *c, const ofk_stabilise *s, const char *who)
{
    if (s->mode != OFK_STAB_OFF && s->mode != OFK_STAB_ROTATION && s->mode != OFK_STAB_PLANE)
        return ofk_fail(c, OFK_E_INVALID, "%s: mode %d is none of OFK_STAB_OFF, OFK_STAB_ROTATION, OFK_STAB_PLANE", who, s->mode);
    if (s->mode == OFK_STAB_OFF) return OFK_OK;
    if (s->border != OFK_BORDER_CONSTANT && s->border != OFK_BORDER_REPLICATE) return ofk_fail(c, OFK_E_INVALID, "%s: unknown border %d", who, s->border);
    if (s->border_value < 0 || s->border_value > 255) return ofk_fail(c, OFK_E_INVALID, "%s: border_value %d outside 0..255", who, s->border_value);
    if (!std::isfinite(s->min_cover) || s->min_cover < 0.0 || !(s->min_cover < 1.0)) return ofk_fail(c, OFK_E_INVALID, "%s: min_cover = %g outside [0, 1)", who, s->min_cover);
    if (s->chain != 0 && s->chain != 1) return ofk_fail(c, OFK_E_INVALID, "%s: chain %d is neither 0 nor 1", who, s->chain);
    return OFK_OK;
}

extern "C" int ofk_set_stabilise(ofk_ctx *c, const ofk_stabilise *s)
{
    return setting_set(c, &ofk_ctx::stab, s && s->mode == OFK_STAB_OFF ? nullptr : s, [](ofk_stabilise &v) { v.mode = OFK_STAB_OFF; },
                       [c](const ofk_stabilise *v) { return check_stab(c, v, "ofk_set_stabilise"); });
}
extern "C" int ofk_get_stabilise(const ofk_ctx *c, ofk_stabilise *s) { return setting_get(c, &ofk_ctx::stab, s); }

// the frames' buffer, [max_batch] images of the context's largest frame, 256-B aligned each
static int stab_frames_alloc(ofk_ctx *c)
{
    if (c->sb_frames) return OFK_OK;
    c->sb_stride = up(c->P, 256);
    OFK_HIP(c, hipMalloc((void **)&c->sb_frames, (size_t)c->max_batch * c->sb_stride));
    return OFK_OK;
}

extern "C" int ofk_stab_download(ofk_ctx *c, uint8_t *frames, double *rec, int *covered)
{
    if (!c) return OFK_E_INVALID;
    TRY(track_download_begin(c, TRACK[TS_STAB], false, 0));
    if (frames && !(c->sb_frames && c->sb_h > 0)) return ofk_fail(c, OFK_E_INVALID, "ofk_stab_download: no step has warped a frame yet");
    if (frames)
        OFK_HIP(c, hipMemcpy2DAsync(frames, (size_t)c->sb_h * c->sb_w, c->sb_frames, c->sb_stride, (size_t)c->sb_h * c->sb_w, c->sb_batch, hipMemcpyDeviceToHost, c->stream));
    const download_row rows[] = {{rec, c->sb_rec, OFK_STAB_DOUBLES * 8, OFK_STAB_DOUBLES * 8}, {covered, c->sb_cov, 4, 4}};
    return rows_download(c, c->sb_batch, 0, rows, 2);
}

extern "C" int ofk_stab_frames(ofk_ctx *c, uint8_t **device_ptr, size_t *image_stride)
{
    if (!c) return OFK_E_INVALID;
    if (!device_ptr || !image_stride) return ofk_fail(c, OFK_E_INVALID, "ofk_stab_frames: NULL argument");
    TRY(track_download_begin(c, TRACK[TS_STAB], false, 0));
    if (!(c->sb_frames && c->sb_h > 0)) return ofk_fail(c, OFK_E_INVALID, "ofk_stab_frames: no step has warped a frame yet");
    *device_ptr = c->sb_frames; *image_stride = c->sb_stride;
    return OFK_OK;
}

extern "C" int ofk_stab_reset(ofk_ctx *c, int b)
{
    const char *who = "ofk_stab_reset";
    if (!c) return OFK_E_INVALID;
    if (c->stream_batch < 1 || b < 0 || b >= c->stream_batch) return ofk_fail(c, OFK_E_INVALID, "%s: stream %d is none of the %d active streams", who, b, c->stream_batch);
    TRY(enter(c));
    TRY(track_begin(c, TRACK[TS_STAB], c->stream_batch));
    ofk_launch_stab_clear(c->stream, c->sb_Bv, c->sb_ist, c->sb_rec, nullptr, b, 1);
    TRY(check_launch(c, who));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

// rules 1-4 on host buffers: device scratch only
extern "C" int ofk_stab_pose(ofk_ctx *c, const ofk_stabilise *s, const double *R, const double *key_rec, const double *sensors, const double *normal,
                             const int *prev_covered, int h, int w, double *Bv, int *ints, int batch, double *rec)
{
    const char *who = "ofk_stab_pose";
    if (!c) return OFK_E_INVALID;
    if (!s || !R || !key_rec || !sensors || !Bv || !ints) return ofk_fail(c, OFK_E_INVALID, "%s: NULL argument", who);
    if (batch < 1 || h < 1 || w < 1) return ofk_fail(c, OFK_E_INVALID, "%s: batch %d, frame %d x %d", who, batch, w, h);
    if (s->mode == OFK_STAB_OFF) return ofk_fail(c, OFK_E_INVALID, "%s: the setting is off", who);
    TRY(check_stab(c, s, who));
    const size_t B = (size_t)batch;
    Bump bp;
    TRY(est_begin(c, B * ((9 + OFK_KEY_DOUBLES + OFK_SENSOR_DOUBLES + 3 + 9 + OFK_STAB_DOUBLES + 9) * 8 + (1 + OFK_STAB_INTS) * 4) + 9 * 256, bp));
    ofk_stab_in in = {};
    in.R = bp.put(R, B * 72); in.R_stride = 9;
    in.key_rec = bp.put(key_rec, B * OFK_KEY_DOUBLES * 8); in.sensors = bp.put(sensors, B * OFK_SENSOR_DOUBLES * 8);
    in.normal = normal ? bp.put(normal, B * 24) : in.sensors + 1; in.normal_stride = normal ? 3 : OFK_SENSOR_DOUBLES;
    int *d_cov = prev_covered ? (int *)bp.put(prev_covered, B * 4) : (int *)bp.take(B * 4);
    in.cov = d_cov;
    in.Bv = bp.put(Bv, B * 72); in.ist = (int *)bp.put(ints, B * OFK_STAB_INTS * 4);
    in.rec = bp.take(B * OFK_STAB_DOUBLES * 8); in.M = bp.take(B * 72);
    if (!prev_covered && bp.rc == OFK_OK && hipMemsetAsync(d_cov, 0, B * 4, c->stream) != hipSuccess) bp.rc = OFK_E_HIP;
    if (bp.rc != OFK_OK || hipStreamSynchronize(c->stream) != hipSuccess) return ofk_fail(c, OFK_E_HIP, "%s: upload failed", who);
    ofk_launch_stab_pose(c->stream, in, s, h, w, batch);
    TRY(check_launch(c, "k_stab_pose"));
    const back_row back[] = {{Bv, in.Bv, B * 72}, {ints, in.ist, B * OFK_STAB_INTS * 4}, {rec, in.rec, B * OFK_STAB_DOUBLES * 8}};
    return fetch_back(c, who, back, 3);
}

// ------------------------------------------------------------------------------------------------ video streams
static int stream_alloc(ofk_ctx *c)
{
    if (!c->pts_new) {
        OFK_HIP(c, hipMalloc((void **)&c->pts_new, (size_t)c->max_batch * c->max_pts * 8));
        OFK_HIP(c, hipMalloc((void **)&c->new_counts, (size_t)c->max_batch * 4));
        OFK_HIP(c, hipMalloc((void **)&c->limit, (size_t)c->max_batch * 4));
    }
    return lazy_mask(c);
}

// gray + pyramid of a batch of BGR frames (host) into pyramid slot k
static int stream_ingest(ofk_ctx *c, int k, const uint8_t *bgr, int batch, int h, int w, const ofk_levels &lv)
{
    if (bgr) TRY(h2d(c, c->bgr[k], c->bgr_stride, bgr, (size_t)h * w * 3, batch));      // NULL: the frames are in bgr[k] already (JPEG ingest)
    c->pyr_last = 0;
    ofk_launch_gray(c->stream, c->bgr[k], c->bgr_stride, c->pyr[k], c->pyr_stride, batch, h, w);
    build_pyramids(c, c->stream, c->pyr[k], nullptr, lv, batch);
    return OFK_OK;
}

// corners of the previous frame (pyramid slot 0, level 0) -> dst/dst_counts, optional mask and per-stream budget
static int stream_detect(ofk_ctx *c, const uint8_t *dmask, const int *limit, int batch, int h, int w, const ofk_params *p, float *dst,
                         int *dst_counts, const float *occ_pts = nullptr, const int *occ_counts = nullptr)   // the corner grid's occupancy list, rows of max_pts
{
    View v = view_of(c, 0, batch, 0);
    TRY(detect_response(c, c->stream, v, dmask, h, w, p->block_size, p->quality));
    detect_select(c, c->stream, v, h, w, p->max_corners, p->quality, p->min_distance, dst, dst_counts, limit, c->grid, occ_pts, occ_counts, c->max_pts);
    return check_launch(c, "stream corner detection");
}

static int stream_fetch_tracks(ofk_ctx *c, int batch, int max_corners, float *tracks, int *counts)
{
    int flags[4];
    if (!c->h_counts) c->h_counts = (int *)calloc(c->max_batch, sizeof(int));
    OFK_HIP(c, hipMemcpyAsync(flags, c->dev_flags, 16, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipMemcpyAsync(c->h_counts, c->counts, (size_t)batch * 4, hipMemcpyDeviceToHost, c->stream));   // also tells the next step who re-detects
    if (tracks) OFK_HIP(c, hipMemcpy2DAsync(tracks, (size_t)max_corners * 8, c->pts_prev, (size_t)c->max_pts * 8, (size_t)max_corners * 8, batch,
                                            hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    const int rc = check_capacity(c, flags, c->h_counts, batch);
    if (counts) memcpy(counts, c->h_counts, (size_t)batch * 4);
    return rc;
}

// first_bgr == NULL: the first frames have been decoded into bgr[0] already (ofk_stream_begin_jpeg)
static int stream_begin_impl(ofk_ctx *c, const uint8_t *first_bgr, int batch, int h, int w, const ofk_params *p, float *tracks, int *counts)
{
    TRY(check_block(c, h, w, p->block_size));
    TRY(check_select(c, p->max_corners, p->quality, p->min_distance));
    TRY(check_lk(c, h, w, p->win, p->max_level));
    TRY(grid_prepare(c, c->grid, batch, h, w, "ofk_stream_begin"));
    TRY(stream_alloc(c));
    if (c->zone_tab) TRY(zones_clear(c, c->max_batch));          // new streams start without zones (a table that was never used is clear)
    c->bias_fresh = 1; c->bias_batch = 0;                        // ... and with the gyro bias of the setting
    const ofk_levels lv = ofk_make_levels(h, w, p->win, p->max_level);
    TRY(stream_ingest(c, 0, first_bgr, batch, h, w, lv));
    TRY(stream_detect(c, nullptr, nullptr, batch, h, w, p, c->pts_prev, c->counts));
    if (c->pf_in) OFK_HIP(c, hipMemsetAsync(c->pf_in, 0, (size_t)c->max_batch * OFK_POSF_INPUT * 8, c->stream));   // no position input waits for the new streams
    for (const track_state &s : TRACK) c->*s.batch = c->*s.live = 0;   // ... and without per-track state: the first step with a setting on starts its own,
    if (TRACK[TS_TABLE].on(c)) TRY(track_begin(c, TRACK[TS_TABLE], batch));   // but for the track table, which begins with the tracks
    c->stream_h = h; c->stream_w = w; c->stream_batch = batch;
    return stream_fetch_tracks(c, batch, p->max_corners, tracks, counts);
}

extern "C" int ofk_stream_begin(ofk_ctx *c, const uint8_t *first_bgr, int batch, int h, int w, const ofk_params *p, float *tracks,
                                int *counts)
{
    TRY(check_geom(c, batch, h, w, "ofk_stream_begin"));
    if (!first_bgr || !p) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_begin: NULL argument");
    return stream_begin_impl(c, first_bgr, batch, h, w, p, tracks, counts);
}

// The same with the frames arriving as baseline JPEG streams (CompressedImage payloads, node:112): decoded on the device straight
// into the stream's frame buffer, no decoded frame ever crosses PCIe.
extern "C" int ofk_stream_begin_jpeg(ofk_ctx *c, const uint8_t *const *jpeg, const size_t *nbytes, int batch, const ofk_params *p,
                                     float *tracks, int *counts)
{
    if (!c || !jpeg || !nbytes || !p || batch < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_begin_jpeg: bad argument");
    int h = 0, w = 0;
    if (ofk_jpeg_info(jpeg[0], nbytes[0], &h, &w, nullptr) != OFK_OK) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_begin_jpeg: stream 0 is not a supported JPEG stream");
    TRY(check_geom(c, batch, h, w, "ofk_stream_begin_jpeg"));
    c->stream_batch = 0;
    TRY(ofk_jpeg_decode_device(c, jpeg, nbytes, batch, c->bgr[0], c->bgr_stride, c->P, &h, &w, nullptr, nullptr));
    return stream_begin_impl(c, nullptr, batch, h, w, p, tracks, counts);
}

// the node's initial state (node:182-217): vel 0.1, first message pending, rotation I, normal e_z
static const double k_imu_init[OFK_IMU_STATE] = {0.1, 0.1, 0.1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0};

static int filters_alloc(ofk_ctx *c)
{
    const size_t B = (size_t)c->max_batch;
    if (!c->imu_state) {
        OFK_HIP(c, hipMalloc((void **)&c->imu_state, B * OFK_IMU_STATE * 8)); OFK_HIP(c, hipMalloc((void **)&c->imu_dv, B * 24));
        OFK_HIP(c, hipMalloc((void **)&c->kf_mats, 5 * 36 * 8)); OFK_HIP(c, hipMalloc((void **)&c->kf_x, B * 6 * 8));
        OFK_HIP(c, hipMalloc((void **)&c->kf_P, B * 36 * 8)); OFK_HIP(c, hipMalloc((void **)&c->fused, B * 8 * 8));
        OFK_HIP(c, hipMemsetAsync(c->imu_dv, 0, B * 24, c->stream)); OFK_HIP(c, hipMemsetAsync(c->fused, 0, B * 64, c->stream));
        OFK_HIP(c, hipMemsetAsync(c->kf_mats, 0, 5 * 36 * 8, c->stream));
        for (size_t b = 0; b < B; ++b)
            OFK_HIP(c, hipMemcpyAsync(c->imu_state + b * OFK_IMU_STATE, k_imu_init, sizeof k_imu_init, hipMemcpyHostToDevice, c->stream));
        OFK_HIP(c, hipStreamSynchronize(c->stream));
    }
    return OFK_OK;
}

extern "C" int ofk_imu_reset(ofk_ctx *c, const double *state0, int batch)
{
    if (!c || batch < 1 || batch > c->max_batch) return ofk_fail(c, OFK_E_INVALID, "ofk_imu_reset: bad argument");
    TRY(enter(c));
    TRY(filters_alloc(c));
    const double *src = state0 ? state0 : k_imu_init;
    for (int b = 0; b < batch; ++b)
        OFK_HIP(c, hipMemcpyAsync(c->imu_state + (size_t)b * OFK_IMU_STATE, src, sizeof k_imu_init, hipMemcpyHostToDevice, c->stream));
    OFK_HIP(c, hipMemsetAsync(c->imu_dv, 0, (size_t)batch * 24, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

extern "C" int ofk_imu_push(ofk_ctx *c, const double *msgs, const int *counts, int max_msgs, int batch)
{
    if (!c || !msgs || !counts || max_msgs < 1 || batch < 1 || batch > c->max_batch) return ofk_fail(c, OFK_E_INVALID, "ofk_imu_push: bad argument");
    TRY(enter(c));
    TRY(filters_alloc(c));
    const size_t mb = (size_t)batch * max_msgs * OFK_IMU_MSG * 8;
    if (mb > c->imu_msgs_bytes) {
        if (c->imu_msgs) { OFK_HIP(c, hipStreamSynchronize(c->stream)); hipFree(c->imu_msgs); c->imu_msgs = nullptr; c->imu_msgs_bytes = 0; }
        OFK_HIP(c, hipMalloc((void **)&c->imu_msgs, mb));
        c->imu_msgs_bytes = mb;
    }
    if (!c->imu_counts) OFK_HIP(c, hipMalloc((void **)&c->imu_counts, (size_t)c->max_batch * 4));
    OFK_HIP(c, hipMemcpyAsync(c->imu_msgs, msgs, mb, hipMemcpyHostToDevice, c->stream));
    OFK_HIP(c, hipMemcpyAsync(c->imu_counts, counts, (size_t)batch * 4, hipMemcpyHostToDevice, c->stream));
    ofk_launch_imu_seq(c->stream, c->imu_state, c->imu_dv, c->imu_msgs, c->imu_counts, max_msgs, batch);
    TRY(check_launch(c, "k_imu_seq"));
    OFK_HIP(c, hipStreamSynchronize(c->stream));                  // the host buffers are the caller's again
    return OFK_OK;
}

extern "C" int ofk_imu_state(ofk_ctx *c, double *state, double *dv, int batch)
{
    if (!c || !state || batch < 1 || batch > c->max_batch) return ofk_fail(c, OFK_E_INVALID, "ofk_imu_state: bad argument");
    TRY(enter(c));
    TRY(filters_alloc(c));
    if (dv) OFK_HIP(c, hipMemcpyAsync(dv, c->imu_dv, (size_t)batch * 24, hipMemcpyDeviceToHost, c->stream));
    return get(c, state, c->imu_state, (size_t)batch * OFK_IMU_STATE * 8);
}

extern "C" int ofk_filter_configure(ofk_ctx *c, int ns, int nm, int nc, const double *F, const double *Bm, const double *H, const double *Q,
                                    const double *Rm, const double *x0, const double *P0, int batch)
{
    if (!c || ns < 1 || ns > 6 || nm < 1 || nm > 6 || nc < 0 || nc > 6 || !F || !H || !Q || !Rm || !x0 || !P0 || (nc && !Bm) || batch < 1 ||
        batch > c->max_batch)
        return ofk_fail(c, OFK_E_INVALID, "ofk_filter_configure: bad argument");
    TRY(enter(c));
    TRY(filters_alloc(c));
    double mats[5 * 36] = {0};
    memcpy(mats, F, (size_t)ns * ns * 8); if (nc) memcpy(mats + 36, Bm, (size_t)ns * nc * 8);
    memcpy(mats + 72, H, (size_t)nm * ns * 8); memcpy(mats + 108, Q, (size_t)ns * ns * 8); memcpy(mats + 144, Rm, (size_t)nm * nm * 8);
    OFK_HIP(c, hipMemcpyAsync(c->kf_mats, mats, sizeof mats, hipMemcpyHostToDevice, c->stream));
    for (int b = 0; b < batch; ++b) {
        OFK_HIP(c, hipMemcpyAsync(c->kf_x + (size_t)b * ns, x0, (size_t)ns * 8, hipMemcpyHostToDevice, c->stream));
        OFK_HIP(c, hipMemcpyAsync(c->kf_P + (size_t)b * ns * ns, P0, (size_t)ns * ns * 8, hipMemcpyHostToDevice, c->stream));
    }
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    c->kf_ns = ns; c->kf_nm = nm; c->kf_nc = nc;
    return OFK_OK;
}

extern "C" int ofk_filter_state(ofk_ctx *c, double *x, double *P, int batch)
{
    if (!c || !x || !P || batch < 1 || batch > c->max_batch || c->kf_ns < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_filter_state: no filter configured / bad argument");
    TRY(enter(c));
    OFK_HIP(c, hipMemcpyAsync(x, c->kf_x, (size_t)batch * c->kf_ns * 8, hipMemcpyDeviceToHost, c->stream));
    return get(c, P, c->kf_P, (size_t)batch * c->kf_ns * c->kf_ns * 8);
}

// Per-pair filter update of the resident batch behind the latest ofk_pairs_run (asynchronous, on the stream that ends the step):
// predict + correct(z_sign * v) for every pair from its own record; the filter states (ofk_filter_configure) never leave the device.
extern "C" int ofk_pairs_filter_step(ofk_ctx *c, double z_sign, int z_source, int batch)
{
    if (!c || batch < 1 || batch > c->cur_batch || c->kf_ns < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_pairs_filter_step: no filter configured / bad batch");
    TRY(use_device(c));
    hipStream_t s;
    TRY(tail_stream(c, &s));
    if (c->cov.mode != OFK_COV_OFF && c->cov_rec && c->cov_batch >= batch)       // behind a run with the setting on: R_eff, NIS, the gate
        ofk_launch_kf_records_cov(s, c->kf_ns, c->kf_nm, c->kf_mats, c->kf_x, c->kf_P, c->records, c->cov_rec, &c->cov, z_sign, z_source, batch);
    else
        ofk_launch_kf_records(s, c->kf_ns, c->kf_nm, c->kf_mats, c->kf_x, c->kf_P, c->records, z_sign, z_source, batch);
    TRY(tail_done(c, s));
    return check_launch(c, "k_kf_records");
}

// fu == NULL: the plain step (status filter, node-style solve, no resident filters); next_bgr == NULL: the new frames are in bgr[1]
// already (stream_step_jpeg)
static int stream_step_impl(ofk_ctx *c, const uint8_t *next_bgr, const double *sensors, const ofk_params *p, const ofk_fusion *fu,
                            int min_features, int mask_radius, double *records, double *fused, float *tracks, int *counts)
{
    const int B = c->stream_batch, h = c->stream_h, w = c->stream_w;
    TRY(check_block(c, h, w, p->block_size));
    TRY(check_select(c, p->max_corners, p->quality, p->min_distance));
    TRY(check_lk(c, h, w, p->win, p->max_level));
    if (mask_radius < 0 || mask_radius > 255) return ofk_fail(c, OFK_E_INVALID, "mask_radius outside 0..255");
    if (fu) {
        if (p->solve_variant < OFK_SOLVE_NODE || p->solve_variant > OFK_SOLVE_OFMODULE) return ofk_fail(c, OFK_E_INVALID, "solve_variant must be NODE, SIM or OFMODULE");
        if (p->solve_variant == OFK_SOLVE_OFMODULE && fu->keep != OFK_KEEP_LEGACY)
            return ofk_fail(c, OFK_E_INVALID, "OFK_SOLVE_OFMODULE weights its rows with the legacy r_tilde distances: it needs keep = OFK_KEEP_LEGACY");
        if (fu->filter && c->kf_ns < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_step_fused: filter requested but ofk_filter_configure was not called");
        if (fu->flow < 0 || fu->flow > 1 || fu->keep < 0 || fu->keep > 1 || fu->control < 0 || fu->control > 1 || fu->min_solve < 0)
            return ofk_fail(c, OFK_E_INVALID, "ofk_stream_step_fused: bad ofk_fusion field");
        if (fu->hold_on_skip && B != 1) return ofk_fail(c, OFK_E_INVALID, "ofk_fusion.hold_on_skip needs a context with one stream (%d here): a batch shares one frame swap", B);
        TRY(filters_alloc(c));
    } else if (p->solve_variant != OFK_SOLVE_NODE && p->solve_variant != OFK_SOLVE_SIM) return ofk_fail(c, OFK_E_INVALID, "solve_variant must be NODE or SIM");
    TRY(check_grid(c, &c->grid, h, w, "ofk_stream_step"));
    TRY(fm_check_step(c, p->solve_variant, fu, fu ? "ofk_stream_step_fused" : "ofk_stream_step"));
    TRY(second_prepare(c, B, p->solve_variant, fu, fu ? "ofk_stream_step_fused" : "ofk_stream_step"));
    TRY(bias_check_step(c, B, p->solve_variant, fu, fu ? "ofk_stream_step_fused" : "ofk_stream_step"));
    TRY(track_check_step(c, p->solve_variant, fu, fu ? "ofk_stream_step_fused" : "ofk_stream_step"));
    const int defer = second_on(c) && fu && fu->filter ? 1 : 0;   // the second-stage kernel corrects
    const ofk_levels lv = ofk_make_levels(h, w, p->win, p->max_level);
    if (c->robust.loss != OFK_ROBUST_OFF) { TRY(robust_alloc(c)); c->rob_batch = B; }
    if (gate_on(c->gate)) { TRY(gate_alloc(c)); c->gate_batch = B; c->gate_fb = c->gate.fb_mode != OFK_FB_OFF; }
    const bool zones_on = c->zones.mode != OFK_ZONES_OFF;
    if (zones_on) { TRY(check_zones(c, &c->zones, "ofk_stream_step")); TRY(zones_alloc(c)); }
    TRY(solve_points_prepare(c, B));
    OFK_HIP(c, hipMemcpyAsync(c->sensors, sensors, (size_t)B * OFK_SENSOR_DOUBLES * 8, hipMemcpyHostToDevice, c->stream));
    // the step's omega, ground normal and R_world: the resident IMU state's (imu: for the kernels that choose themselves) or the sensor rows'
    struct step_source { const double *imu, *omega, *normal, *rw; int stride; };
    const step_source src = fu && fu->use_imu ? step_source{c->imu_state, c->imu_state + 18, c->imu_state + 15, c->imu_state + 6, OFK_IMU_STATE}
                                              : step_source{nullptr, c->sensors + 4, c->sensors + 1, c->sensors + 7, OFK_SENSOR_DOUBLES};
    double *const bias_ist = bias_on(c) && src.imu ? c->imu_state : nullptr;
    if (bias_on(c)) ofk_launch_gyro_bias_apply(c->stream, c->sensors + 4, OFK_SENSOR_DOUBLES, bias_ist, c->bias_rec, B, 0);   // everything below reads omega - b^
    struct bias_restore {                                        // a step that ends early still puts the IMU state's raw omega back
        ofk_ctx *c; double *ist; int B;
        void now() { if (ist) ofk_launch_gyro_bias_apply(c->stream, nullptr, 0, ist, c->bias_rec, B, 1); ist = nullptr; }
        ~bias_restore() { now(); }
    } restore = {c, bias_ist, B};
    bool on[sizeof(TRACK) / sizeof(TRACK[0])];                   // track_check_step: none is on without the state it needs
    for (const track_state &s : TRACK) {
        on[&s - TRACK] = s.on(c);
        if (s.on(c)) TRY(track_begin(c, s, B));                  // no state of these tracks yet: begun afresh
        else c->*s.live = 0;                                     // the tracks move on without it
    }
    const bool table = on[TS_TABLE], depth = on[TS_DEPTH], templ = on[TS_TEMPLATE], keyf = on[TS_KEY], krot = on[TS_KEYROT], kmap = on[TS_KEYMAP];
    const bool stab = on[TS_STAB];
    if (stab) TRY(stab_frames_alloc(c));
    const bool flow_seed = table && c->tt.seed == OFK_TT_SEED_FLOW;
    bool few = false;                                            // the host knows the track counts from the previous call
    for (int b = 0; b < B; ++b) few = few || (c->h_counts && c->h_counts[b] <= min_features);
    if (fu && fu->redetect_replace && few) {
        // of_module.py:83-86: before tracking, streams with few tracks replace them by fresh corners of the PREVIOUS frame (no mask)
        ofk_launch_redetect_limits(c->stream, c->counts, min_features, p->max_corners, c->limit, B);
        TRY(grid_prepare(c, c->grid, B, h, w, "ofk_stream_step_fused"));
        if (zones_on) {                                          // the zones alone, where they stand in the previous frame
            OFK_HIP(c, hipMemsetAsync(c->mask, 1, (size_t)B * c->img_stride, c->stream));
            ofk_launch_zone_mask(c->stream, c->mask, c->img_stride, h, w, c->zone_tab, c->zone_mot, c->zones.radius, c->limit, B);
        }
        TRY(stream_detect(c, zones_on ? c->mask : nullptr, c->limit, B, h, w, p, c->pts_new, c->new_counts));
        ofk_launch_replace_tracks(c->stream, c->limit, c->pts_new, c->new_counts, c->max_pts, c->pts_prev, c->counts, B);
        for (const track_state &s : TRACK) if (on[&s - TRACK] && s.replace) s.replace(c, B);
    }
    TRY(stream_ingest(c, 1, next_bgr, B, h, w, lv));
    // track (node:133), solve on the tracked points (node:229-258)
    const View v = view_of(c, 0, B, 0);                          // the solve stage reads v.solve_*; the tracks, the zones and the re-detection stay in the image
    TRY(track(c, c->stream, v, lv, p, src.imu, flow_seed ? &c->ttr : nullptr, templ ? &c->tpr : nullptr,
              c->ttr.age, keyf ? c->kfr.next_copy : nullptr));
    if (zones_on)                                                // the solve stage turns the status into its keep flags: rule 1 needs both
        OFK_HIP(c, hipMemcpyAsync(c->zone_status, c->status, (size_t)B * c->max_pts, hipMemcpyDeviceToDevice, c->stream));
    if (fu) {
        const bool rob = c->robust.loss != OFK_ROBUST_OFF;
        const ofk_stream_in in = {v.solve_prev, v.solve_next, c->status, c->counts, c->max_pts, c->sensors, c->imu_state, c->kf_ns, c->kf_nm, c->kf_nc, c->kf_mats,
                                  c->kf_x, c->kf_P, fu, p->solve_variant, c->records, c->fused, B, defer};
        if (rob)
            ofk_launch_stream_fuse_robust(c->stream, in, c->imu_dv, p->use_feasibility, p->feas_T, &c->robust, c->rob_work, c->rob_w, c->rob_wtmp,
                                          c->rob_stats);
        else
            ofk_launch_stream_fuse(c->stream, in, c->imu_dv, p->use_feasibility, p->feas_T);
        if (bias_on(c) && bias_estimates(c->bias)) ofk_launch_stream_bias(c->stream, in, 1, 0, 0.0, rob ? c->rob_w : nullptr, &c->bias, c->bias_rec);
        for (const second_setting &s : SECOND) if (s.mode(c)) s.stream(c, in, rob ? c->rob_w : nullptr);
    } else
        solve_pairs(c, c->stream, v.solve_prev, v.solve_next, c->status, c->counts, c->sensors, p, nullptr, c->records, 0, B, true);
    // re-detection for the streams that had few features (node:157-166): mask = discs around the OLD positions, image = OLD frame.
    // The host knows the track counts from the previous call, so the whole branch is skipped when no stream needs it.
    // of_module.py:138 `continue`: a step of the ONE stream that did not solve leaves old_gray / old_pos as they were.  The host has to
    // know before it queues the track update, hence one wait (hold_on_skip is opt-in).
    bool hold = false;
    if (fu && fu->hold_on_skip) {
        double solved = 1.0;
        OFK_HIP(c, hipMemcpyAsync(&solved, c->records + 15, 8, hipMemcpyDeviceToHost, c->stream));
        OFK_HIP(c, hipStreamSynchronize(c->stream));
        hold = solved == 0.0;
    }
    const bool any = few && !(fu && fu->redetect_replace) && !hold;
    if (zones_on && !hold)                                       // rules 1-4; rule 7 in the same launch unless the mask comes between them
        ofk_launch_zones_update(c->stream, c->pts_prev, c->pts_next, c->zone_status, c->status, c->counts, c->max_pts, &c->zones, c->zone_tab,
                                c->zone_mot, c->zone_stats, c->zone_work, any ? 0 : 1, B);
    if (any) {
        ofk_launch_redetect_limits(c->stream, c->counts, min_features, p->max_corners, c->limit, B);
        OFK_HIP(c, hipMemsetAsync(c->mask, 1, (size_t)B * c->img_stride, c->stream));
        ofk_launch_disc_mask(c->stream, c->mask, c->img_stride, h, w, c->pts_prev, c->counts, c->max_pts, mask_radius, c->limit, B);
        if (zones_on) {
            ofk_launch_zone_mask(c->stream, c->mask, c->img_stride, h, w, c->zone_tab, c->zone_mot, c->zones.radius, c->limit, B);
            ofk_launch_zones_age(c->stream, c->zone_tab, c->zone_mot, c->zone_stats, B);
        }
        // with a corner grid the old tracks are its occupancy list as well: the new corners go to the cells the tracks have left
        TRY(grid_prepare(c, c->grid, B, h, w, "ofk_stream_step"));
        TRY(stream_detect(c, c->mask, c->limit, B, h, w, p, c->pts_new, c->new_counts, c->pts_prev, c->counts));
    }
    // tracks := new[status == 1] ++ re-detected (node:134,166); the new frame becomes the previous one (node:175)
    if (!hold) {
        if (keyf) {                                              // in front of the depths', the templates' and the table's update
            ofk_kf_in in = {};                                   // the ideal next points in front of the finite-motion rewrite
            in.next_pts = !fm_on(c) ? v.solve_next : camera_on(c) || rs_on(c) ? c->kfr.next_copy : v.pts_next;
            in.status = c->status; in.counts = c->counts; in.stride = c->max_pts;
            in.new_counts = any ? c->new_counts : nullptr; in.max_total = p->max_corners; in.sensors = c->sensors;
            in.imu = src.imu; in.v = c->records; in.plain = fu ? 0 : 1;
            in.step = c->ttr.head; in.step_stride = 2;
            ofk_km_rows mr = c->kmr;                             // the depths as the previous step left them: their step is behind this launch
            mr.rho = c->tdr.rho; mr.var = c->tdr.var; mr.nobs = c->tdr.nobs;
            const bool stab_rot = stab && krot && !kr_all_held(&c->krot);      // the view's R: the rotation record's, else rule 1's product anew
            if (stab && !stab_rot) OFK_HIP(c, hipMemcpyAsync(c->sb_st, c->kfr.st, (size_t)B * OFK_KEY_STATE * 8, hipMemcpyDeviceToDevice, c->stream));
            launch_key_step(c, c->kfr, in, &c->key, krot ? &c->krot : nullptr, c->kr_st, c->kr_rec, B, kmap ? &c->kmap : nullptr, &mr);
            if (on[TS_POSF])                                     // directly behind it, on the record it has just written
                ofk_launch_pos_filter_step(c->stream, &c->posf, c->pf_x, c->pf_P, c->pf_ist, c->pf_rec, c->pf_in, c->records, fu ? 0 : 1, c->kfr.rec,
                                           src.rw, src.stride, B);
            if (stab) {                                          // behind both: the view's pose, then the new frame (pyramid slot 1, level 0) into it
                ofk_stab_in si = {};
                if (stab_rot) { si.R = c->kr_rec + 4; si.R_stride = OFK_KEYROT_DOUBLES; }
                else { si.st_copy = c->sb_st; si.omega = src.omega; si.omega_stride = src.stride; }
                si.key_rec = c->kfr.rec; si.sensors = c->sensors;
                si.normal = src.normal; si.normal_stride = src.stride;
                si.cov = c->sb_cov; si.Bv = c->sb_Bv; si.ist = c->sb_ist; si.rec = c->sb_rec; si.M = c->sb_M;
                ofk_launch_stab_pose(c->stream, si, &c->stab, h, w, B);
                if (camera_on(c))                                // accepted with ofk_set_rectify on only: the raw frame through the lens's map
                    ofk_launch_warp_lens(c->stream, &c->camera, c->rect.r_max, c->pyr[1], c->pyr_stride, h, w, 1, c->sb_M, c->sb_frames, c->sb_stride, h, w,
                                         c->stab.border, c->stab.border_value, c->sb_cov, B);
                else
                    ofk_launch_warp(c->stream, c->pyr[1], c->pyr_stride, h, w, 1, c->sb_M, c->sb_frames, c->sb_stride, h, w, c->stab.border, c->stab.border_value,
                                    c->sb_cov, B);
                c->sb_h = h; c->sb_w = w;
            }
        }
        if (depth) {                                             // in front of the table's update, on what k_update_tracks is about to read
            ofk_td_in in = {};
            in.prev_pts = v.solve_prev; in.next_pts = v.solve_next; in.status = c->status; in.counts = c->counts; in.stride = c->max_pts;
            in.new_counts = any ? c->new_counts : nullptr; in.max_total = p->max_corners; in.sensors = c->sensors;
            in.omega = src.omega; in.omega_stride = src.stride;
            in.v = c->records; in.plain = fu ? 0 : 1;
            ofk_launch_track_depth_step(c->stream, c->tdr, in, &c->td, B);
        }
        if (templ) {                                             // rule 6, with the keep rule of the two launches below; the templates change buffers
            ofk_launch_track_template_update(c->stream, c->tpr, c->status, c->counts, c->max_pts, any ? c->new_counts : nullptr, p->max_corners, &c->tpl, B);
            c->tpr.cur ^= 1;
        }
        if (table)                                               // in front of it: it overwrites pts_prev and counts
            ofk_launch_track_table_update(c->stream, c->ttr, c->pts_prev, c->pts_next, c->status, c->counts, c->max_pts, any ? c->pts_new : nullptr,
                                          any ? c->new_counts : nullptr, p->max_corners, flow_seed ? 1 : 0, flow_seed ? (float)c->tt.gain : 0.f, B);
        ofk_launch_update_tracks(c->stream, c->pts_next, c->status, c->counts, c->max_pts, any ? c->pts_new : nullptr, any ? c->new_counts : nullptr,
                                 c->pts_prev, c->counts, p->max_corners, B);
    }
    restore.now();                                               // the step's last launch: the IMU state's raw omega back, bit for bit
    TRY(check_launch(c, "ofk_stream_step"));
    if (records) OFK_HIP(c, hipMemcpyAsync(records, c->records, (size_t)B * OFK_RECORD_DOUBLES * 8, hipMemcpyDeviceToHost, c->stream));
    if (fu && fused) OFK_HIP(c, hipMemcpyAsync(fused, c->fused, (size_t)B * 64, hipMemcpyDeviceToHost, c->stream));
    // The tracks on the device already belong to the new frame (k_update_tracks), so the frame swap happens whatever the fetch
    // reports (OFK_E_CAPACITY from a re-detection, a failed copy): the next step must track against THIS frame's pyramid.
    const int rc = stream_fetch_tracks(c, B, p->max_corners, tracks, counts);
    if (hold) return rc;                                         // old frame and old tracks stay; the next frame overwrites slot 1
    uint8_t *t = c->pyr[0]; c->pyr[0] = c->pyr[1]; c->pyr[1] = t;
    t = c->bgr[0]; c->bgr[0] = c->bgr[1]; c->bgr[1] = t;
    return rc;
}

extern "C" int ofk_stream_step(ofk_ctx *c, const uint8_t *next_bgr, const double *sensors, const ofk_params *p, int min_features,
                               int mask_radius, double *records, float *tracks, int *counts)
{
    if (!c || !next_bgr || !sensors || !p) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_step: NULL argument");
    if (c->stream_batch < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_step: call ofk_stream_begin first");
    TRY(enter(c));
    return stream_step_impl(c, next_bgr, sensors, p, nullptr, min_features, mask_radius, records, nullptr, tracks, counts);
}

// the JPEG variants: the new frames decoded on the device into bgr[1], which must come out with the streams' geometry, then the step
static int stream_step_jpeg(ofk_ctx *c, const char *who, const uint8_t *const *jpeg, const size_t *nbytes, const double *sensors,
                            const ofk_params *p, const ofk_fusion *fu, int min_features, int mask_radius, double *records, double *fused,
                            float *tracks, int *counts)
{
    if (c->stream_batch < 1) return ofk_fail(c, OFK_E_INVALID, "%s: call ofk_stream_begin / ofk_stream_begin_jpeg first", who);
    TRY(enter(c));
    int h = 0, w = 0;
    TRY(ofk_jpeg_decode_device(c, jpeg, nbytes, c->stream_batch, c->bgr[1], c->bgr_stride, c->P, &h, &w, nullptr, nullptr));
    if (h != c->stream_h || w != c->stream_w)
        return ofk_fail(c, OFK_E_INVALID, "%s: frames are %dx%d, the streams were begun with %dx%d", who, w, h, c->stream_w, c->stream_h);
    return stream_step_impl(c, nullptr, sensors, p, fu, min_features, mask_radius, records, fused, tracks, counts);
}

extern "C" int ofk_stream_step_jpeg(ofk_ctx *c, const uint8_t *const *jpeg, const size_t *nbytes, const double *sensors, const ofk_params *p,
                                    int min_features, int mask_radius, double *records, float *tracks, int *counts)
{
    if (!c || !jpeg || !nbytes || !sensors || !p) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_step_jpeg: NULL argument");
    return stream_step_jpeg(c, "ofk_stream_step_jpeg", jpeg, nbytes, sensors, p, nullptr, min_features, mask_radius, records, nullptr, tracks,
                            counts);
}

// next positions and keep flags of the LATEST stream step (they stay in place until the next step): what a caller needs to form
// the flow of the kept points, new - old, against the tracks it received before the step (node:134-136)
extern "C" int ofk_stream_last_points(ofk_ctx *c, float *next_pts, uint8_t *keep, int stride)
{
    if (!c || !next_pts || !keep || stride < 1 || stride > c->max_pts) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_last_points: bad argument");
    if (c->stream_batch < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_last_points: no active streams");
    TRY(enter(c));
    OFK_HIP(c, hipMemcpy2DAsync(next_pts, (size_t)stride * 8, c->pts_next, (size_t)c->max_pts * 8, (size_t)stride * 8, c->stream_batch, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipMemcpy2DAsync(keep, stride, c->status, c->max_pts, stride, c->stream_batch, hipMemcpyDeviceToHost, c->stream));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    return OFK_OK;
}

extern "C" int ofk_stream_step_fused(ofk_ctx *c, const uint8_t *next_bgr, const double *sensors, const ofk_params *p, const ofk_fusion *f,
                                     int min_features, int mask_radius, double *records, double *fused, float *tracks, int *counts)
{
    if (!c || !next_bgr || !sensors || !p || !f) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_step_fused: NULL argument");
    if (c->stream_batch < 1) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_step_fused: call ofk_stream_begin first");
    TRY(enter(c));
    return stream_step_impl(c, next_bgr, sensors, p, f, min_features, mask_radius, records, fused, tracks, counts);
}

extern "C" int ofk_stream_step_fused_jpeg(ofk_ctx *c, const uint8_t *const *jpeg, const size_t *nbytes, const double *sensors, const ofk_params *p,
                                          const ofk_fusion *f, int min_features, int mask_radius, double *records, double *fused, float *tracks,
                                          int *counts)
{
    if (!c || !jpeg || !nbytes || !sensors || !p || !f) return ofk_fail(c, OFK_E_INVALID, "ofk_stream_step_fused_jpeg: NULL argument");
    return stream_step_jpeg(c, "ofk_stream_step_fused_jpeg", jpeg, nbytes, sensors, p, f, min_features, mask_radius, records, fused, tracks,
                            counts);
}

extern "C" int ofk_set_streams(ofk_ctx *c, int nstreams)
{
    if (!c || nstreams < 1 || nstreams > OFK_MAX_STREAMS) return ofk_fail(c, OFK_E_INVALID, "ofk_set_streams: 1..%d", OFK_MAX_STREAMS);
    // A different slice count moves the slice boundaries: a new slice's auxiliary stream would only wait for the LK of the OLD
    // slice with the same index (ev_lkdone[set][k]) while another old slice may still read the pyramid rows it is about to
    // rewrite.  Changing the schedule is rare (set-up time), so drain everything.
    TRY(drain_all(c));
    c->nstreams = nstreams;
    if (nstreams > 1) {
        const char *q = getenv("GPU_MAX_HW_QUEUES");
        static bool warned = false;
        if (!warned && q && atoi(q) > 0 && atoi(q) < 2 * nstreams) {
            fprintf(stderr, "libofk: GPU_MAX_HW_QUEUES=%s, but %d slices keep %d streams busy: streams that share a hardware queue run in order "
                            "(set GPU_MAX_HW_QUEUES >= %d before the first HIP call)\n", q, nstreams, 2 * nstreams, 2 * nstreams);
            warned = true;
        }
    }
    // Create the slice and auxiliary streams NOW: the runtime deals streams onto its hardware queues in creation order, and a
    // library that creates streams of its own later (RCCL does at ncclCommInitRank) must not get in between - with the
    // pipeline's streams created lazily behind RCCL's, two of them shared a queue and the rate fell by 10 % (99 k -> 87 k).
    return need_streams(c, nstreams, c->overlap != 0);
}

extern "C" int ofk_set_overlap(ofk_ctx *c, int on)
{
    if (!c) return OFK_E_INVALID;
    TRY(drain_all(c));                                           // same hazard as ofk_set_streams
    c->overlap = on ? 1 : 0;
    return OFK_OK;
}

extern "C" int ofk_mark(ofk_ctx *c, int slot)
{
    if (!c || slot < 0 || slot >= 8) return ofk_fail(c, OFK_E_INVALID, "ofk_mark: slot 0..7");
    TRY(use_device(c));
    if (!c->marks[slot]) OFK_HIP(c, hipEventCreateWithFlags(&c->marks[slot], hipEventDisableTiming));
    hipStream_t s;
    TRY(tail_stream(c, &s));                                     // "everything enqueued so far" includes every slice
    OFK_HIP(c, hipEventRecord(c->marks[slot], s));
    return OFK_OK;
}

extern "C" int ofk_mark_wait(ofk_ctx *c, int slot)
{
    if (!c || slot < 0 || slot >= 8) return ofk_fail(c, OFK_E_INVALID, "ofk_mark_wait: slot 0..7");
    if (!c->marks[slot]) return OFK_OK;
    OFK_HIP(c, hipEventSynchronize(c->marks[slot]));
    return OFK_OK;
}

extern "C" int ofk_profile_enable(ofk_ctx *c, int stage_mask)
{
    if (!c) return OFK_E_INVALID;
    c->prof_mask = stage_mask;
    return OFK_OK;
}

extern "C" int ofk_profile_read(ofk_ctx *c, double *ms_total, int *launches)
{
    if (!c || !ms_total || !launches) return OFK_E_INVALID;
    TRY(join_slices(c));
    OFK_HIP(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < OFK_N_STAGES; ++s) { ms_total[s] = 0.0; launches[s] = 0; }
    for (int i = 0; i + 1 < c->ev_n; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]) == hipSuccess) { ms_total[c->ev_stage[i / 2]] += ms; launches[c->ev_stage[i / 2]] += 1; }
    }
    c->ev_n = 0;
    return OFK_OK;
}
