// ofk_internal.h — context layout and kernel-launcher prototypes shared by the libofk.so sources.
// gfx950 only (wave64, 160 KiB LDS/CU, 256 CUs in 8 XCDs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "ofk.h"

#define OFK_MAX_LEVELS 9            // level 0 .. 8
#define OFK_MAX_STREAMS 8           // slices of a batch that run their stage chains concurrently
#define OFK_CHUNK 4096              // candidates sorted per selection round (LDS resident)
#define OFK_SEG_MAX 2048            // segments (strips) per image the selection kernel walks
#define OFK_MAX_STRIDE 128          // ints between per-image response maxima: one L2 channel each (a packed array was a hot spot)
#define OFK_CNT_STRIDE 32           // ints between per-image candidate counters (one 128-B line each: no atomic contention)

struct ofk_levels {
    int n;                          // deepest level index in use (0..8)
    int h[OFK_MAX_LEVELS], w[OFK_MAX_LEVELS];
    size_t off[OFK_MAX_LEVELS];     // byte offset of level l inside one image's pyramid slab (256-B aligned)
};

// the track table's arrays (ofk.h: ofk_set_track_table), rows `stride` apart per stream
struct ofk_tt_rows { unsigned *ids; int *age, *birth_step; float *birth_xy, *flow_xy; unsigned *step_ids; int *head, *stats; };

// the depth per track (ofk.h: ofk_set_track_depth): the state's arrays, rows `stride` apart per stream in the table's row order, and the
// records [B][OFK_TD_DOUBLES]; what one step reads
struct ofk_td_rows { double *rho, *var; int *nobs; double *rec; };
struct ofk_td_in {
    const float *prev_pts, *next_pts;                            // the solve's resident points, or
    const double *x, *u;                                         // the stage entry's [B][stride][2] (then prev_pts / next_pts / sensors are NULL)
    const uint8_t *status; const int *counts; int stride;        // what k_update_tracks reads
    const int *new_counts; int max_total;                        // NULL: no re-detection
    const double *sensors;                                       // scaling, cx, cy of the resident points
    const double *omega; int omega_stride;                       // the omega the solve read, doubles between streams
    const double *v; int plain;                                  // [B][OFK_RECORD_DOUBLES]: v in 0-2, solved in 15 (plain: rank 3 in slot 4)
};

// the track templates (ofk.h: ofk_set_track_template): the state's arrays, rows `stride` apart per stream in the table's row order;
// tmpl[cur] holds the templates, tmpl[cur ^ 1] takes them from the compaction; *_new, move: what the latest k_track_template found
struct ofk_tp_rows {
    uint8_t *tmpl[2]; int cur, tstride;
    float *A, *A_new, *ncc, *ncc_new, *move; uint8_t *flag, *flag_new, *tstate;
    float *L; double *rec;                                       // [B][4], [B][OFK_TPL_DOUBLES]
};

// the keyframe (ofk.h: ofk_set_keyframe): the state's arrays, rows `stride` apart per stream in the table's row order, the per-stream
// state [B][OFK_KEY_STATE] / [B][OFK_KEY_INTS] and the records [B][OFK_KEY_DOUBLES]; next_copy: the ideal next points in front of an
// in-place finite-motion rewrite; what one step reads
struct ofk_kf_rows { float *key_xy; uint8_t *member; double *st; int *ist; double *rec; float *next_copy; };
struct ofk_kf_in {
    const float *next_pts;                                       // the ideal next points, [B][stride][2]
    const uint8_t *status; const int *counts; int stride;        // what k_update_tracks reads
    const int *new_counts; int max_total;                        // NULL: no re-detection
    const double *sensors, *imu;                                 // [B][OFK_SENSOR_DOUBLES]; the IMU state under use_imu, else NULL
    const double *v; int plain;                                  // [B][OFK_RECORD_DOUBLES]: v_uav in 8-10, solved in 15 (plain: rank 3 in slot 4)
    const int *step; int step_stride;                            // the table's step per stream, ints between streams
};
// the keyframe's map (ofk.h: ofk_set_keyframe_map): key_rho, key_var [B][stride] in the table's row order; mstate [B][2] =
// (captured_for, map_rows); mrec [B][OFK_KEYMAP_DOUBLES]; rho, var, nobs: the depth state as the previous step left it, read only
// (NULL: the stream has none, no row is mature)
struct ofk_km_rows { double *key_rho, *key_var; int *mstate; double *mrec; const double *rho, *var; const int *nobs; };

// the stabilised view (ofk.h: ofk_set_stabilise): what one k_stab_pose launch reads and writes.  R with R_stride doubles between streams is
// the rotation used, unless st_copy (the keyframe's state in front of its launch) is given: then R is rule 1's product of it and omega
struct ofk_stab_in {
    const double *R; int R_stride; const double *st_copy, *omega; int omega_stride;
    const double *key_rec, *sensors, *normal; int normal_stride;  // the keyframe's records behind its launch; d, scaling, c; where the keyframe read n
    const int *cov;                                              // [B] covered pixels of the previous warp (read where ist[3] != 0)
    double *Bv; int *ist; double *rec, *M;                       // [B][9], [B][OFK_STAB_INTS], [B][OFK_STAB_DOUBLES], [B][9]
};

struct ofk_comm;
struct ofk_ctx {
    int device;
    ofk_comm *comm;                                       // RCCL communicator + gather buffers (ofk_comm.hip), NULL until ofk_comm_init
    hipStream_t stream;                           // the context's stream (slice 0); entry points synchronise on it
    hipStream_t streams[OFK_MAX_STREAMS]; int nstreams;   // extra slice streams (created on first use), joined back into `stream` by events
    hipEvent_t ev_fork;
    hipStream_t aux[OFK_MAX_STREAMS]; int overlap;        // per-slice auxiliary stream: next-frame gray + pyramids beside the response kernel
    hipEvent_t ev_g0[OFK_MAX_STREAMS], ev_aux[OFK_MAX_STREAMS];
    uint8_t *pyr_alt[2]; int pyr_set;                     // second pyramid set: the auxiliary stream runs one call ahead
    int pyr_last;                                         // the set the latest ofk_pairs_run built its pyramids in (ofk_resident_pyramid)
    hipEvent_t ev_lkdone[2][OFK_MAX_STREAMS];             // LK of the call that last read a set has finished
    hipEvent_t marks[8];                                  // ofk_mark / ofk_mark_wait
    // Slices free-run across consecutive ofk_pairs_run calls (no fork/join per call) and are offset by one response kernel, so
    // one slice's latency-bound stages (selection, solve) always run beside another slice's response kernel or LK.
    int slices_open, open_slices;                         // slice streams hold work the context's stream has not joined yet / how many
    hipEvent_t ev_end[OFK_MAX_STREAMS];                   // end of a slice's chain of the latest call (slice 0 included)
    hipEvent_t ev_stagger[OFK_MAX_STREAMS];               // response kernel of slice k launched (first call after a join)
    hipEvent_t ev_x; int x_pending;                       // record export queued behind the last slice, not yet seen by `stream`
    int max_w, max_h, max_batch, max_pts, max_level;
    size_t P;                       // max_w * max_h
    size_t bgr_stride;              // bytes between images in bgr[], 256-B aligned
    size_t pyr_stride;              // bytes between images in pyr[], 256-B aligned (all levels of one image)
    size_t img_stride;              // elements between images in eig/mask (P rounded up to 64)
    int cand_cap;                   // candidate keys per image

    uint8_t *bgr[2];                // [B][bgr_stride]            prev / next BGR frames
    int gray_direct_set;            // >= 0: the resident frame pairs exist as gray level 0 of this pyramid set only (compressed ingest,
                                    // ofk_pairs_upload_staged): ofk_pairs_run takes that set and skips its BGR -> gray conversions; -1: bgr[] holds them
    uint8_t *pyr[2];                // [B][pyr_stride]            gray pyramids (level 0 = gray frame)
    float *eig;                     // [B][img_stride]            Shi-Tomasi response
    uint8_t *mask;                  // [B][img_stride]            optional detection mask (lazily allocated)
    int16_t *deriv;                 // [B][img_stride][2]         only for ofk_scharr_s16 (lazily allocated)
    unsigned long long *cand;       // [B][cand_cap]              candidate keys (~value bits << 32 | linear index), flat list
    unsigned long long *cand_seg;   // [B][seg_keys]              per-strip key segments written by the streaming response kernel
    int *seg_count;                 // [B][OFK_SEG_MAX]           keys per segment
    size_t seg_keys;                // keys per image in cand_seg
    int *cand_count;                // [B][OFK_CNT_STRIDE]
    unsigned *sel_hist;             // [B][1024]                  key histogram of k_select_prep
    unsigned long long *sel_keys;   // [B][OFK_CHUNK]             keys below the first cut, picked by k_select_pick for k_select_greedy
    unsigned int *maxbits;          // [B][OFK_MAX_STRIDE]                       bit pattern of max positive response
    float *pts_prev, *pts_next;     // [B][max_pts][2]
    uint8_t *status;                // [B][max_pts]
    float *err;                     // [B][max_pts]
    int *counts;                    // [B]                        corners per image
    float *pts_new;                 // [B][max_pts][2]            re-detected corners of a stream step (lazily allocated)
    int *new_counts, *limit;        // [B]                        their counts / per-stream re-detection budget
    int stream_h, stream_w, stream_batch;         // geometry of the active video streams (ofk_stream_begin), 0 = none
    int *h_counts;                                // host copy of the streams' track counts after the last call
    double *sensors;                // [B][OFK_SENSOR_DOUBLES]
    double *records;                // [B][OFK_RECORD_DOUBLES]
    int *dev_flags;                 // [4]                        device-side error flags (bit 0: candidate overflow)
    void *scratch; size_t scratch_bytes;          // device scratch for the estimation entry points
    void *hstage; size_t hstage_bytes;            // pinned host staging
    void *jstage;                                 // JPEG staging slots + copy stream (k_jpeg.hip), NULL until the first compressed frame

    // per-stream filters resident on the device (ofk_imu_*, ofk_filter_*, ofk_stream_step_fused); lazily allocated
    double *imu_state, *imu_dv;     // [B][OFK_IMU_STATE], [B][3]
    double *kf_mats, *kf_x, *kf_P;  // 5 x 36 doubles (F, B, H, Q, R), [B][6], [B][36]
    double *fused;                  // [B][8]
    double *imu_msgs; int *imu_counts; size_t imu_msgs_bytes;     // upload staging for ofk_imu_push
    int kf_ns, kf_nm, kf_nc;
    int cur_batch, cur_h, cur_w;    // resident pair geometry (ofk_pairs_upload)
    int prof_mask;
    int lk_seed_mode; double lk_seed_gain;   // ofk_set_lk_seed: OFK_SEED_OFF unless set
    ofk_lk_light light;                      // ofk_set_lk_light: mode OFK_LIGHT_OFF (gain_max 4) unless set
    ofk_robust robust;                       // ofk_set_robust: loss OFK_ROBUST_OFF unless set
    double *rob_work, *rob_w, *rob_wtmp, *rob_stats;   // [B][7][max_pts] per-point terms, [B][max_pts] weights (+ a scratch copy), [B][OFK_ROBUST_DOUBLES]; one lazy allocation (rob_work owns it)
    int rob_batch;                           // problems of the latest robust run / step (ofk_robust_download), 0 = none
    ofk_track_gate gate;                     // ofk_set_track_gate: fb_mode OFK_FB_OFF and err_max 0 unless set
    float *pts_back, *err_back, *fb2;        // [B][max_pts][2] end points of the backward pass, [B][max_pts] its err (discarded) and the squared
    uint8_t *status_back; int *gate_stats;   // distances; [B][max_pts] its status, [B][4] the gate's counts; one lazy allocation (pts_back owns it)
    int gate_batch, gate_fb;                 // images of the latest gated run / step (ofk_track_gate_download), 0 = none / it ran a backward pass
    ofk_corner_grid grid;                    // ofk_set_corner_grid: cell 0 (off) unless set
    int *grid_stats; int *grid_occ_counts; float *grid_occ;   // [B][2] statistics, [B] / [B][max_pts][2] occupancy list of the stage entries; one lazy allocation (grid_stats owns it)
    int grid_batch;                          // images of the latest selection with a grid on (ofk_corner_grid_download), 0 = none
    ofk_cov cov;                             // ofk_set_cov: mode OFK_COV_OFF unless set
    double *cov_rec; int cov_batch;          // [B][OFK_COV_DOUBLES] (lazily allocated); problems of the latest run / step with it on, 0 = none
    ofk_joint joint;                         // ofk_set_joint: mode OFK_JOINT_OFF unless set
    double *joint_rec; int joint_batch;      // [B][OFK_JOINT_DOUBLES] (lazily allocated); problems of the latest run / step with it on, 0 = none
    ofk_gyro_bias bias;                      // ofk_set_gyro_bias: mode OFK_BIAS_OFF unless set
    double *bias_rec; int bias_batch, bias_fresh;   // [B][OFK_BIAS_DOUBLES] state and record (lazily allocated); streams of the latest step with it on, 0 = none; the state is still to be set from the setting
    ofk_plane plane;                         // ofk_set_plane: mode OFK_PLANE_OFF unless set
    double *plane_rec; int plane_batch;      // [B][OFK_PLANE_DOUBLES] (lazily allocated); problems of the latest run / step with it on, 0 = none
    ofk_epipolar epi;                        // ofk_set_epipolar: mode OFK_EPI_OFF unless set
    double *epi_rec, *epi_pts; int epi_batch;   // [B][OFK_EPI_DOUBLES] and [B][max_pts][4] (one lazy allocation, epi_rec owns it); problems of the latest run / step with it on, 0 = none
    ofk_zones zones;                         // ofk_set_zones: mode OFK_ZONES_OFF unless set
    int *zone_tab; float *zone_mot; int *zone_stats, *zone_work;   // [B][OFK_ZONE_MAX][OFK_ZONE_INTS], [B][OFK_ZONE_MAX][OFK_ZONE_FLOATS], [B][OFK_ZONE_STATS], [B][2][max_pts] hull stacks;
    uint8_t *zone_status;                    // [B][max_pts] status in front of the solve stage; one lazy allocation (zone_tab owns it)
    ofk_camera camera;                       // ofk_set_camera: model OFK_CAMERA_OFF unless set
    float *pts_prev_u, *pts_next_u;          // [B][max_pts][2] ideal pixels of pts_prev / pts_next, what the solve stage reads with the camera on; one lazy allocation (pts_prev_u owns it)
    int cam_batch;                           // images of the latest run / step with the camera on (ofk_camera_download), 0 = none
    ofk_rshutter rs;                         // ofk_set_rolling_shutter: mode OFK_RS_OFF unless set; with it on the solve stage reads pts_prev_u / pts_next_u too
    int rs_batch;                            // images of the latest run / step with the rolling shutter on (ofk_rs_download), 0 = none
    ofk_finite_motion fm;                    // ofk_set_finite_motion: mode OFK_FM_OFF unless set; with it on the solve stage reads pts_prev_u / pts_next_u too
    int fm_batch;                            // images of the latest run / step with the finite motion on (ofk_finite_download), 0 = none
    ofk_track_table tt;                      // ofk_set_track_table: mode OFK_TT_OFF (gain 1) unless set
    ofk_tt_rows ttr;                         // the table's device rows, [B][max_pts] each, head [B][2], stats [B][OFK_TT_STATS]; one lazy allocation (ttr.ids owns it)
    int tt_batch, tt_live;                   // streams of the latest begin / step with the table on (ofk_track_table_download), 0 = none; streams whose rows match their current tracks
    ofk_track_depth td;                      // ofk_set_track_depth: mode OFK_TD_OFF unless set
    ofk_td_rows tdr;                         // the depth state's device rows, [B][max_pts] each, and records; one lazy allocation (tdr.rho owns it)
    int td_batch, td_live;                   // streams of the latest step with the depths on (ofk_track_depth_download), 0 = none; streams whose rows match their current tracks
    ofk_track_template tpl;                  // ofk_set_track_template: mode OFK_TPL_OFF unless set
    ofk_tp_rows tpr;                         // the templates' device rows, [B][max_pts] each, and records; one lazy allocation (tpr.tmpl[0] owns it)
    int tp_batch, tp_live;                   // streams of the latest step with the templates on (ofk_track_template_download), 0 = none; streams whose rows match their current tracks
    ofk_keyframe key;                        // ofk_set_keyframe: mode OFK_KEY_OFF unless set
    ofk_kf_rows kfr;                         // the keyframe's device rows and per-stream state; one lazy allocation (kfr.key_xy owns it)
    ofk_keyframe_rotation krot;              // ofk_set_keyframe_rotation: mode OFK_KEYROT_OFF unless set
    double *kr_st, *kr_rec;                  // [max_batch][OFK_KEYROT_STATE], [max_batch][OFK_KEYROT_DOUBLES]; one lazy allocation (kr_st owns it)
    int kr_batch, kr_live;                   // (kr_live: streams whose rotation state is in step with their keyframe) streams of the latest step with the rotation on (ofk_keyframe_rotation_download), 0 = none
    ofk_keyframe_map kmap;                   // ofk_set_keyframe_map: mode OFK_KEYMAP_OFF unless set
    ofk_km_rows kmr;                         // the map's device rows and per-stream state (rho, var, nobs unused here); one lazy allocation (kmr.key_rho owns it)
    int km_batch, km_live;                   // streams of the latest step with the map on (ofk_keyframe_map_download), 0 = none; streams whose map is in step with their keyframe
    ofk_pos_filter posf;                     // ofk_set_pos_filter: mode OFK_POSF_OFF unless set
    double *pf_x, *pf_P, *pf_rec, *pf_in;    // [max_batch][12], [max_batch][144], [max_batch][OFK_POSF_DOUBLES], [max_batch][OFK_POSF_INPUT]; one lazy allocation (pf_x owns it)
    int *pf_ist;                             // [max_batch][OFK_POSF_INTS]
    int pf_batch, pf_live;                   // streams of the latest step with the position filter on (ofk_pos_filter_download), 0 = none; streams whose filter runs on
    ofk_stabilise stab;                      // ofk_set_stabilise: mode OFK_STAB_OFF unless set
    ofk_rectify rect;                        // ofk_set_rectify: mode OFK_RECTIFY_OFF unless set; with it and the camera on the view's warp is k_warp_lens_u8
    double *sb_Bv, *sb_rec, *sb_M, *sb_st;   // [max_batch][9], [max_batch][OFK_STAB_DOUBLES], [max_batch][9], [max_batch][OFK_KEY_STATE] (the keyframe's state in front of its launch); one lazy allocation (sb_Bv owns it)
    int *sb_ist, *sb_cov;                    // [max_batch][OFK_STAB_INTS], [max_batch] covered pixels of the latest warp
    uint8_t *sb_frames; size_t sb_stride;    // [max_batch][sb_stride] the stabilised frames, 256-B aligned per image (an allocation of its own, made by the first step with the setting on)
    int sb_batch, sb_live, sb_h, sb_w;       // streams of the latest step with the setting on (ofk_stab_download), 0 = none; streams whose view runs on; the frames' geometry
    int kf_batch, kf_live;                   // streams of the latest step with the keyframe on (ofk_keyframe_download), 0 = none; streams whose rows match their current tracks
    hipEvent_t *ev; int ev_cap, ev_n; int *ev_stage;   // pairs of events: start/stop
    char errmsg[512];
};

// Launch-geometry knobs of ofk_set_tuning (ofk.h): process-wide, 0 = the built-in choice.  Results never depend on them.
struct ofk_tuning { int eig_rows, no_pair, no_pyr3, pyr3_chunks, pyr_rows, jpeg_chunk, gray_px, jpeg_sub; };
extern ofk_tuning g_ofk_tuning;

// --- helpers (host)
int ofk_fail(ofk_ctx *ctx, int code, const char *fmt, ...);
#define OFK_HIP(ctx, call)                                                                       \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return ofk_fail(ctx, OFK_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)
ofk_levels ofk_make_levels(int h, int w, int win, int max_level);   // win <= 0: ignore the winSize stop rule
int ofk_need_scratch(ofk_ctx *ctx, size_t bytes);
int ofk_join_slices(ofk_ctx *ctx);
int ofk_prepare_streams(ofk_ctx *ctx);                                 // create the slice / auxiliary streams of the current schedule
int ofk_export_records_stream(ofk_ctx *c, float *device_dst, int batch, hipStream_t *stream_out);   // k_records_f32 on the stream that ends the step
                                   // before touching the context's stream / shared buffers
void ofk_jpeg_release(ofk_ctx *c);
int ofk_jpeg_stage_streams(ofk_ctx *c, int slot, const uint8_t *const *jpeg, const size_t *nbytes, int count);
const char *ofk_jpeg_slot_error(const ofk_ctx *c, int slot);       // the slot's own message: staging may run beside the owner thread
int ofk_jpeg_decode_staged_pairs(ofk_ctx *c, int slot, uint8_t *dst_prev, uint8_t *dst_next, size_t dst_stride, size_t dst_capacity_px, int *batch_out,
                                 int *h_out, int *w_out, const hipEvent_t *wait_before_writing, int nwait, int as_gray);
                                 // wait_before_writing != NULL: decode on the ingest stream, beside whatever runs on the context's, behind those events;
                                 // as_gray: dst_* are gray planes (rows of w bytes; what k_gray_bgr8 would make of the decoded BGR frame), no BGR is written
int ofk_jpeg_decode_device(ofk_ctx *c, const uint8_t *const *jpeg, const size_t *nbytes, int batch, uint8_t *dst, size_t dst_stride,
                           size_t dst_capacity_px, int *h_out, int *w_out, uint8_t **out, size_t *out_stride);   // k_jpeg.hip

// the corner grid of one selection launch (ofk.h: ofk_corner_grid): setting, occupancy list (occ_pts NULL = empty) and the
// [batch][2] statistics, all of the launch's first image on
struct ofk_sel_grid { int cell, cap, max_rank; const float *occ_pts; const int *occ_counts; int occ_stride; int *stats; };

// --- what the solve launchers of one form share: the stage entries' device arrays, a slice's resident pairs, a fused stream step
struct ofk_stage_in { int variant; const double *x, *u; const uint8_t *valid; int batch, n; const double *d, *nrm, *omega, *t; };
struct ofk_pairs_in {
    const float *prev_pts, *next_pts; const uint8_t *status; const int *counts; int pts_stride; const double *sensors;
    int variant, use_feas; double feas_T; double *records; int batch;
};
struct ofk_stream_in {
    const float *prev_pts, *next_pts; uint8_t *status; const int *counts; int pts_stride; const double *sensors; double *imu_state;
    int ns, nm, nc; const double *kf_mats; double *kf_x, *kf_P; const ofk_fusion *f; int variant; double *records, *fused; int batch;
    int defer;                                                   // see fuse_args.defer
};

// --- launchers (all asynchronous on `s`; pointers are device pointers)
void ofk_launch_gray(hipStream_t s, const uint8_t *bgr, size_t bgr_stride, uint8_t *gray, size_t gray_stride, int batch,
                     int h, int w);
void ofk_launch_pyr_down(hipStream_t s, const uint8_t *src, size_t src_stride, int h, int w, uint8_t *dst,
                         size_t dst_stride, int batch);
void ofk_launch_pyr_down2(hipStream_t s, const uint8_t *src0, const uint8_t *src1, size_t src_stride, int h, int w,
                          uint8_t *dst0, uint8_t *dst1, size_t dst_stride, int batch);
bool ofk_launch_pyr3(hipStream_t s, uint8_t *pyr0, uint8_t *pyr1, size_t stride, const ofk_levels &lv, int batch, int images);
void ofk_launch_scharr(hipStream_t s, const uint8_t *src, size_t src_stride, int h, int w, int16_t *dxdy,
                       size_t dst_stride_elems, int batch);
// the perspective warp (ofk.h: ofk_warp_perspective; k_warp.inc): ch 1 or 3; M [batch][9] f64 destination -> source; every dst image
// 4-byte aligned; covered [batch] i32 is zeroed and counted, NULL = not counted
void ofk_launch_warp(hipStream_t s, const uint8_t *src, size_t src_stride, int sh, int sw, int ch, const double *M, uint8_t *dst,
                     size_t dst_stride, int dh, int dw, int border, int bval, int *covered, int batch);
// the same warp through a lens (ofk.h: ofk_warp_lens; k_warp_lens.inc): M maps a destination pixel to an IDEAL pixel of `cam`, NULL = the
// identity; cam->model BROWN or FISHEYE; r_max 0 = no limit
void ofk_launch_warp_lens(hipStream_t s, const ofk_camera *cam, double r_max, const uint8_t *src, size_t src_stride, int sh, int sw, int ch,
                          const double *M, uint8_t *dst, size_t dst_stride, int dh, int dw, int border, int bval, int *covered, int batch);
int  ofk_launch_mineig(hipStream_t s, const uint8_t *gray, size_t gray_stride, int h, int w, int block, float *eig,
                       size_t eig_stride, unsigned int *maxbits, const uint8_t *mask, size_t mask_stride, int batch);
void ofk_launch_maxbits(hipStream_t s, const float *eig, size_t eig_stride, const uint8_t *mask, size_t mask_stride,
                        int h, int w, unsigned int *maxbits, int batch);
void ofk_launch_nms(hipStream_t s, const float *eig, size_t eig_stride, const uint8_t *mask, size_t mask_stride, int h,
                    int w, const unsigned int *maxbits, double quality, unsigned long long *cand, int cand_cap,
                    int *cand_count, int *flags, int batch);
int  ofk_launch_mineig_cand(hipStream_t s, const uint8_t *gray, size_t gray_stride, int h, int w, int block,
                            unsigned int *maxbits, const uint8_t *mask, size_t mask_stride, double quality,
                            unsigned long long *cand, int cand_cap, int *cand_count, unsigned long long *seg,
                            size_t seg_keys_per_image, int *seg_count, int seg_count_cap, int *flags, int batch, int *nseg_out,
                            int *segcap_out);
void ofk_stream_geometry(int h, int w, int block, int batch, int *rows, int *nseg, int *seg_cap);
void ofk_launch_select(hipStream_t s, unsigned long long *cand, int cand_cap, int *cand_count, const unsigned long long *seg,
                       int seg_cap, const int *seg_count, int nseg, const unsigned int *maxbits, double quality, int h, int w,
                       int max_corners, float min_distance, float *pts, int pts_stride, int *counts, const int *limit, int batch,
                       unsigned *sel_hist, unsigned long long *sel_keys, const ofk_sel_grid *g = nullptr);
                       // nseg == 0: the flat list holds the candidates already; g with cell > 0: k_select_greedy_grid
// what a detection starts from, zeroed in one launch: response maxima, candidate counters and sel_hist ([batch][1024], the selection's prefilter)
void ofk_launch_zero_detect_state(hipStream_t s, unsigned int *maxbits, int *cand_count, unsigned *sel_hist, int batch);
void ofk_launch_disc_mask(hipStream_t s, uint8_t *mask, size_t mask_stride, int h, int w, const float *pts, const int *counts,
                          int pts_stride, int radius, const int *limit, int batch);
void ofk_launch_redetect_limits(hipStream_t s, const int *counts, int min_feat, int max_feat, int *limit, int batch);
void ofk_launch_update_tracks(hipStream_t s, const float *next_pts, const uint8_t *status, const int *counts_in, int pts_stride,
                              const float *new_pts, const int *new_counts, float *tracks, int *counts_out, int max_total, int batch);
// exclusion zones (ofk.h: ofk_set_zones; k_zones.inc): rules 1-4 per stream (do_age: rule 7 behind them), rule 7 alone, rule 6
// (limit NULL = every stream)
void ofk_launch_zones_update(hipStream_t s, const float *old_pts, const float *new_pts, const uint8_t *st_pre, const uint8_t *keep, const int *counts,
                             int pts_stride, const ofk_zones *set, int *tab, float *mot, int *stats, int *work, int do_age, int batch);
void ofk_launch_zones_age(hipStream_t s, int *tab, float *mot, int *stats, int batch);
void ofk_launch_zone_mask(hipStream_t s, uint8_t *mask, size_t mask_stride, int h, int w, const int *tab, const float *mot, int radius,
                          const int *limit, int batch);
// the camera model (ofk.h: ofk_set_camera; k_camera.inc): src0 -> dst0 and, with src1 not NULL, src1 -> dst1 in the same launch;
// distort 0 = image pixels -> ideal pixels, 1 = the forward map; src may be dst
void ofk_launch_camera(hipStream_t s, const ofk_camera *cam, int distort, const float *src0, float *dst0, const float *src1, float *dst1,
                       const int *counts, int pts_stride, int batch);
// the rolling shutter (ofk.h: ofk_set_rolling_shutter; k_rshutter.inc): both ends of every point in ONE launch; id0 / id1 NULL = the raw
// points are the ideal ones; id may be out; rs->rows > 0; sensors may be NULL for OFK_RS_FLOW; imu_state != NULL: its omega
void ofk_launch_rs_correct(hipStream_t s, const ofk_rshutter *rs, const float *raw0, const float *raw1, const float *id0, const float *id1,
                           float *out0, float *out1, const int *counts, int pts_stride, const double *sensors, const double *imu_state, int batch);
// the finite motion (ofk.h: ofk_set_finite_motion; k_finite.inc): both ends of every point in ONE launch; out may be in;
// imu_state != NULL: its normal and omega
void ofk_launch_finite_correct(hipStream_t s, const ofk_finite_motion *fm, const float *in0, const float *in1, float *out0, float *out1,
                               const int *counts, int pts_stride, const double *sensors, const double *imu_state, int batch);
void ofk_launch_lk(hipStream_t s, const uint8_t *prev, const uint8_t *next, size_t pyr_stride, const ofk_levels &lv,
                   const float *prev_pts, const int *counts, int pts_stride, int win, int max_count, double eps,
                   double min_eig_thr, float *next_pts, uint8_t *status, float *err, int batch, int flags = 0);   // flags: OFK_LK_*
// the lighting-insensitive tracker (ofk.h: ofk_lk_light; k_lk_light.inc): ofk_launch_lk's arguments and a setting that is on
void ofk_launch_lk_light(hipStream_t s, const uint8_t *prev, const uint8_t *next, size_t pyr_stride, const ofk_levels &lv,
                         const float *prev_pts, const int *counts, int pts_stride, int win, int max_count, double eps,
                         double min_eig_thr, float *next_pts, uint8_t *status, float *err, int batch, int flags, const ofk_lk_light &light);
// start positions of a seeded LK (ofk.h: ofk_set_lk_seed): seed_out[b][p] for p < counts[b]; imu_state NULL = sensors only
void ofk_launch_seed_points(hipStream_t s, const float *pts, const int *counts, int pts_stride, const double *sensors,
                            const double *imu_state, int mode, double gain, float *seed_out, int batch);
// the track gates behind LK (ofk.h: ofk_set_track_gate): status := keep, fb2 (fb_on) and stats[b][4]; back / st_back / fb2 NULL without fb_on
void ofk_launch_track_gate(hipStream_t s, const float *prev_pts, const float *back_pts, const uint8_t *st_back, const float *err,
                           const int *counts, int pts_stride, int fb_on, float thr2, int err_on, float err_max, uint8_t *status, float *fb2,
                           int *stats, int batch);
// the track table (ofk.h: ofk_set_track_table; k_track_table.inc): rule 1 on freshly detected tracks, rule 2 behind k_replace_tracks,
// rules 3 and 6 in front of k_update_tracks (its arguments; new_counts NULL = no re-detection), rule 5 into LK's start positions
void ofk_launch_track_table_begin(hipStream_t s, const ofk_tt_rows &t, const float *pts, const int *counts, int stride, int batch);
void ofk_launch_track_table_replace(hipStream_t s, const ofk_tt_rows &t, const int *limit, const float *new_pts, const int *new_counts,
                                    int stride, int batch);
void ofk_launch_track_table_update(hipStream_t s, const ofk_tt_rows &t, const float *prev_pts, const float *next_pts, const uint8_t *status,
                                   const int *counts_in, int stride, const float *new_pts, const int *new_counts, int max_total, int seed_on,
                                   float gain, int batch);
void ofk_launch_track_seed(hipStream_t s, const float *pts, const int *counts, int stride, const int *age, const float *flow_xy, float gain,
                           int keep_age0, float *seed, int batch);
// the depth per track (ofk.h: ofk_set_track_depth; k_track_depth.inc): beside the table's begin and replace, rules 1-4 in front of its update
void ofk_launch_track_depth_begin(hipStream_t s, const ofk_td_rows &t, const int *counts, int stride, int batch);
void ofk_launch_track_depth_replace(hipStream_t s, const ofk_td_rows &t, const int *limit, const int *new_counts, int stride, int batch);
void ofk_launch_track_depth_step(hipStream_t s, const ofk_td_rows &t, const ofk_td_in &in, const ofk_track_depth *d, int batch);
// the keyframe (ofk.h: ofk_set_keyframe; k_keyframe.inc): beside the table's begin and replace, rules 1-5 in front of the depths' step
void ofk_launch_keyframe_begin(hipStream_t s, const ofk_kf_rows &t, const int *counts, int stride, int batch);
void ofk_launch_keyframe_replace(hipStream_t s, const ofk_kf_rows &t, const int *limit, const int *new_counts, int stride, int batch);
void ofk_launch_keyframe_reset(hipStream_t s, const ofk_kf_rows &t, int b, int stride, const double *p);
void ofk_launch_keyframe_step(hipStream_t s, const ofk_kf_rows &t, const ofk_kf_in &in, const ofk_keyframe *k, int batch);
// the keyframe's rotation (ofk.h: ofk_set_keyframe_rotation; k_keyframe_rot.inc): k_keyframe_step's launch with the joint rule 2, and the
// rotation state cleared beside the keyframe's begin (limit NULL), replace (limit) and reset (one stream b0)
void ofk_launch_keyframe_step_rot(hipStream_t s, const ofk_kf_rows &t, const ofk_kf_in &in, const ofk_keyframe *k, const ofk_keyframe_rotation *r,
                                  double *rst, double *rrec, int batch);
void ofk_launch_keyrot_clear(hipStream_t s, double *rst, double *rrec, const int *limit, int b0, int flag, int batch);
// the keyframe's map (ofk.h: ofk_set_keyframe_map; k_keyframe_map.inc): k_keyframe_step's launch with rules M1-M5 around it, and the
// map cleared beside the keyframe's begin (limit NULL, counts), replace (limit, the new counts, keep_rec) and reset (one stream b0,
// counts NULL: every row)
void ofk_launch_keyframe_step_map(hipStream_t s, const ofk_kf_rows &t, const ofk_kf_in &in, const ofk_keyframe *k, const ofk_keyframe_map *m,
                                  const ofk_km_rows &r, int batch);
void ofk_launch_keymap_clear(hipStream_t s, const ofk_km_rows &r, const int *key_ist, const int *limit, const int *counts, int stride, int b0,
                             int keep_rec, int batch);
// the position filter (ofk.h: ofk_set_pos_filter; k_pos_filter.inc): rules 1-8 in one launch behind the keyframe's step (v: the step's
// records, plain as ofk_kf_in's; key_rec: the keyframe's records; rw: R_world, rw_stride doubles apart), and the state of `batch`
// streams from b0 on set back to "not started" at the position p (input NULL: the input rows stay)
void ofk_launch_pos_filter_step(hipStream_t s, const ofk_pos_filter *f, double *x, double *P, int *ist, double *rec, double *input, const double *v,
                                int plain, const double *key_rec, const double *rw, int rw_stride, int batch);
void ofk_launch_pos_filter_clear(hipStream_t s, double *x, double *P, int *ist, double *rec, double *input, int b0, const double *p, int batch);
// the stabilised view (ofk.h: ofk_set_stabilise; k_stabilise.inc): rules 1-4 in one launch behind the keyframe's step and the position
// filter's, in front of k_warp_u8; and the view of `batch` streams from b0 on back to the identity (limit != NULL: where limit[b] > 0,
// the counts staying)
void ofk_launch_stab_pose(hipStream_t s, const ofk_stab_in &in, const ofk_stabilise *st, int h, int w, int batch);
void ofk_launch_stab_clear(hipStream_t s, double *Bv, int *ist, double *rec, const int *limit, int b0, int batch);
// the track templates (ofk.h: ofk_set_track_template; k_track_template.inc): rule 1, rules 2-5 behind the gates, rule 6 in front of the table's update
void ofk_launch_track_affine(hipStream_t s, const float *prev_pts, const float *next_pts, const uint8_t *status, const int *counts, int stride,
                             int h, int w, const ofk_track_template *d, float *L, double *rec, int batch);
void ofk_launch_track_template(hipStream_t s, const ofk_tp_rows &t, const uint8_t *prev_img, const uint8_t *next_img, size_t img_stride, int h,
                               int w, const float *prev_pts, float *next_pts, uint8_t *status, const int *age, const int *counts, int stride,
                               const ofk_track_template *d, int batch);
void ofk_launch_track_template_update(hipStream_t s, const ofk_tp_rows &t, const uint8_t *status, const int *counts, int stride,
                                      const int *new_counts, int max_total, const ofk_track_template *d, int batch);
void ofk_launch_pairs_solve(hipStream_t s, const float *prev_pts, const float *next_pts, const uint8_t *status,
                            const int *counts, int pts_stride, const double *sensors, int variant, int use_feas,
                            double feas_T, const int *cand_count, double *records, int batch);
// the robust forms (k_robust.inc); work / weights / wtmp / stats: the slice's rows of the context's rob_* buffers
void ofk_launch_pairs_robust(hipStream_t s, const float *prev_pts, const float *next_pts, const uint8_t *status, const int *counts,
                             int pts_stride, const double *sensors, int variant, int use_feas, double feas_T, const int *cand_count,
                             const ofk_robust *r, int problem0, double *work, double *weights, double *wtmp, double *stats,
                             uint8_t *drop_status, double *records, int batch);
void ofk_launch_solve_robust(hipStream_t s, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                             const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                             const ofk_robust *r, double *work, double *weights, double *wtmp, double *stats, double *out);
void ofk_launch_stream_fuse_robust(hipStream_t s, const ofk_stream_in &in, double *imu_dv, int use_feas, double feas_T, const ofk_robust *r,
                                   double *work, double *weights, double *wtmp, double *stats);
// The second-stage solves (k_second.inc and k_cov / k_joint / k_plane / k_epi.inc), behind the solve kernels, in the three launch forms.
// weights: the robust solve's rows, NULL = the plain solve ran.  The last pointers are the slice's rows of the setting's records (and
// of epi_pts).  Joint, plane and epipolar rewrite out / records in place; the covariance only reads them.
void ofk_launch_cov_solve(hipStream_t s, const ofk_stage_in &in, const double *weights, const ofk_cov *c, const double *out, double *cov);
void ofk_launch_joint_solve(hipStream_t s, const ofk_stage_in &in, const double *weights, const ofk_joint *j, double *out, double *joint);
void ofk_launch_plane_solve(hipStream_t s, const ofk_stage_in &in, const double *weights, const ofk_plane *p, double *out, double *plane);
void ofk_launch_epi_solve(hipStream_t s, const ofk_stage_in &in, const double *weights, const ofk_epipolar *e, double *out, double *epi,
                          double *pts);
void ofk_launch_pairs_cov(hipStream_t s, const ofk_pairs_in &in, const double *weights, const ofk_cov *c, double *cov);
void ofk_launch_pairs_joint(hipStream_t s, const ofk_pairs_in &in, const double *weights, const ofk_joint *j, double *joint);
void ofk_launch_pairs_plane(hipStream_t s, const ofk_pairs_in &in, const double *weights, const ofk_plane *p, double *plane);
void ofk_launch_pairs_epi(hipStream_t s, const ofk_pairs_in &in, const double *weights, const ofk_epipolar *e, double *epi, double *pts);
void ofk_launch_stream_cov(hipStream_t s, const ofk_stream_in &in, const double *weights, const ofk_cov *c, double *cov);
void ofk_launch_stream_joint(hipStream_t s, const ofk_stream_in &in, const double *weights, const ofk_joint *j, double *joint);
void ofk_launch_stream_plane(hipStream_t s, const ofk_stream_in &in, const double *weights, const ofk_plane *p, double *plane);
void ofk_launch_stream_epi(hipStream_t s, const ofk_stream_in &in, const double *weights, const ofk_epipolar *e, double *epi, double *pts);
// the gyro bias (ofk.h: ofk_set_gyro_bias; k_bias.inc): apply / restore on `batch` omegas `stride` doubles apart, the filter step behind a
// stream step's solve kernel (fused: k_stream_fuse[_robust] ran, else the plain step's) and behind a stage entry's
void ofk_launch_gyro_bias_apply(hipStream_t s, double *omega, int stride, double *imu_state, double *bias, int batch, int restore);
void ofk_launch_stream_bias(hipStream_t s, const ofk_stream_in &in, int fused, int use_feas, double feas_T, const double *weights,
                            const ofk_gyro_bias *g, double *bias);
void ofk_launch_bias_solve(hipStream_t s, const ofk_stage_in &in, const double *weights, const ofk_gyro_bias *g, const double *out, double *bias);
void ofk_launch_kf_records_cov(hipStream_t s, int ns, int nm, const double *mats, double *x, double *P, const double *records, double *cov,
                               const ofk_cov *c, double z_sign, int z_source, int batch);
void ofk_launch_records_f32(hipStream_t s, const double *records, float *dst, int batch);

void ofk_launch_flow_model(hipStream_t s, const double *x, int batch, int n, const double *v, const double *omega,
                           const double *d, const double *nrm, const double *t, double *flow);
void ofk_launch_feasibility(hipStream_t s, int variant, const double *x, const double *u, int batch, int n,
                            const double *nrm, const double *v, const double *dist, const double *omega,
                            const double *t, double *r, double *dd);
void ofk_launch_solve(hipStream_t s, int variant, const double *x, const double *u, const uint8_t *valid, int batch,
                      int n, const double *d, const double *nrm, const double *omega, const double *t,
                      const double *wgt, double *out);
void ofk_launch_imu(hipStream_t s, double *state, const double *msg, int batch);
void ofk_launch_kf_records(hipStream_t s, int ns, int nm, const double *mats, double *x, double *P, const double *records, double z_sign,
                           int z_source, int batch);
void ofk_launch_imu_seq(hipStream_t s, double *state, double *dv, const double *msgs, const int *counts, int max_msgs, int batch);
void ofk_launch_stream_fuse(hipStream_t s, const ofk_stream_in &in, double *imu_dv, int use_feas, double feas_T);
void ofk_launch_replace_tracks(hipStream_t s, const int *limit, const float *new_pts, const int *new_counts, int pts_stride, float *tracks,
                               int *counts, int batch);
void ofk_launch_post_solve(hipStream_t s, const double *v_obs, const double *rot, const double *ang,
                           const double *offset, int batch, double *v_uav);
void ofk_launch_kf(hipStream_t s, int ns, int nm, int nc, const double *F, const double *Bm, const double *H,
                   const double *Q, const double *Rm, double *x, double *P, const double *u, const double *z, int batch,
                   int do_predict);
void ofk_launch_of_simulation(hipStream_t s, const double *truth, const double *sig, const double *pos,
                              const double *true_flow, int n, const double *z, int trials, double *v_obs,
                              double *bound);
void ofk_launch_of_simulation_rng(hipStream_t s, const double *truth, const double *sig, const double *pos, const double *true_flow, int n,
                                  unsigned long long seed, unsigned step, unsigned trial0, int trials, double *v_obs, double *bound);
void ofk_launch_noise_normals(hipStream_t s, unsigned k0, unsigned k1, unsigned step, unsigned trial, int count, double *out);
void ofk_launch_feas_simulation(hipStream_t s, const double *truth, const double *sig, const double *pos, const double *true_flow,
                                int n, const double *z, int trials, double *per, double *mean, double *v_obs);
void ofk_launch_hist_overlap(hipStream_t s, const double *d1, int n1, const double *d2, int n2, int bins, int *out);
void ofk_launch_feature_eval(hipStream_t s, const double *pos, const double *pos_err, const double *oldpos, const double *oldpos_err,
                             const int *counts, int batch, int stride, const double *vel, const double *vel_err, double focal,
                             double dummy, double tx, double ty, const double *weight, double *height, double *height_err,
                             uint8_t *immobile, double *score, int *order, int *flags);
void ofk_launch_d_split(hipStream_t s, const double *d, const int *counts, int batch, int stride, double d_exp_err, double *sorted,
                        double *diff, int *nsplit);
void ofk_launch_associate(hipStream_t s, const double *t_img, int n_img, int n_imu, const double *imu_t, const double *imu_q,
                          const double *imu_w, int n_hgt, const double *hgt_t, const double *hgt_r, double *sensors, int *imu_idx,
                          int *hgt_idx);
