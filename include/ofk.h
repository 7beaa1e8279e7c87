/*
 * include/ofk.h — C ABI of libofk.so, the MI355X (gfx950) implementation of the
 * optical-flow -> ego-velocity hot path of
 * liquidcronos/Drone-stabilisation-using-Optical-Flow-Gps-and-Inertial-Sensors.
 *
 * The reference has no FFI for this path: it is Python calling cv2 / numpy.  The entry
 * points below are therefore what a ctypes binding in the reference's own files would
 * call in place of each cv2 / numpy call (file:line of the call being replaced is given
 * per function; paths relative to the reference root; "node" = velocity_measurment_node).
 * INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++ or torch types, no exceptions.
 *   - Every function returns 0 on success or a negative OFK_E_* code; the text of the
 *     last error is available from ofk_last_error().
 *   - Image buffers are C-contiguous: gray [batch][h][w] u8, BGR [batch][h][w][3] u8,
 *     points [batch][stride][2] f32 as (x = column, y = row) — the layout of OpenCV's
 *     (N,1,2) float32 arrays.
 *   - Unless a parameter is documented as a DEVICE pointer, buffers are caller-owned
 *     HOST memory; the library copies to/from device memory it owns inside the context.
 *   - One context = one device + one HIP stream.  Not thread-safe: the caller serialises
 *     calls on a context (the Python facade holds a lock).
 *   - There is no CPU fallback: every entry point runs HIP kernels or fails.
 */
#ifndef OFK_H
#define OFK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFK_VERSION 100          /* 0.1.0 */

#define OFK_OK            0
#define OFK_E_INVALID    -1      /* bad argument / exceeds what the context was created for */
#define OFK_E_HIP        -2      /* a HIP runtime call failed (see ofk_last_error) */
#define OFK_E_CAPACITY   -3      /* a device-side list overflowed its capacity */
#define OFK_E_NOGPU      -4      /* no usable gfx950 device */

typedef struct ofk_ctx ofk_ctx;

/* ---------------------------------------------------------------- lifecycle */
int         ofk_version(void);
const char *ofk_last_error(const ofk_ctx *ctx);      /* ctx may be NULL: error of the last failed ofk_create */
int         ofk_device_count(void);
/* max_w/max_h: largest frame; max_batch: frame pairs per call; max_pts: corners per frame;
 * max_level: deepest LK pyramid level (0..8). */
int         ofk_create(int device, int max_w, int max_h, int max_batch, int max_pts, int max_level, ofk_ctx **out);
int         ofk_destroy(ofk_ctx *ctx);
int         ofk_sync(ofk_ctx *ctx);                   /* hipStreamSynchronize on the context's stream */
int         ofk_device_sync(void);                    /* hipDeviceSynchronize */

/* ------------------------------------------------- stage entry points (host buffers, synchronous) */

/* cv2.cvtColor(img, cv2.COLOR_BGR2GRAY) — of_module.py:40,80; node:113; evaluate_exp.py:65,85; of_library.py:236,248.
 * Y = (3735 B + 19235 G + 9798 R + 16384) >> 15. */
int ofk_gray_bgr8(ofk_ctx *ctx, const uint8_t *bgr, int batch, int h, int w, uint8_t *gray);

/* One pyrDown step of the pyramid cv2.calcOpticalFlowPyrLK builds (of_module.py:88; node:133; evaluate_exp.py:98):
 * separable [1 4 6 4 1]/16, REFLECT_101, dst = ((h+1)/2, (w+1)/2). */
int ofk_pyr_down_u8(ofk_ctx *ctx, const uint8_t *src, int batch, int h, int w, uint8_t *dst);

/* Gaussian pyramid (cv2.buildOpticalFlowPyramid without the derivative planes; what calcOpticalFlowPyrLK builds internally,
 * of_module.py:88): levels 1..max_level of every image by repeated pyrDown, stopping early when a level would be empty.
 * out: per image the levels back to back, tightly packed ((h+1)/2 x (w+1)/2, ...); *levels_built = number of levels written. */
int ofk_pyramid_u8(ofk_ctx *ctx, const uint8_t *gray, int batch, int h, int w, int max_level, uint8_t *out, int *levels_built);

/* Scharr derivatives of one pyramid level as calcOpticalFlowPyrLK computes them (same call sites):
 * dxdy [batch][h][w][2] int16 = (dx, dy), REFLECT_101 at the image border. */
int ofk_scharr_s16(ofk_ctx *ctx, const uint8_t *gray, int batch, int h, int w, int16_t *dxdy);

/* cv2.warpPerspective(src, M, dsize, flags = INTER_LINEAR | WARP_INVERSE_MAP, borderMode, borderValue) — the warp of the reference's
 * homography experiment (homography_experiments/homography.py), for `batch` images in one launch.
 * src [batch][sh][sw][channels] u8 -> dst [batch][dh][dw][channels] u8, channels 1 or 3 (interleaved).  M [batch][9] f64, row-major
 * 3x3 per image, maps a DESTINATION pixel to a SOURCE pixel (the caller inverts a source -> destination matrix).
 * The rule, per destination pixel with integer (x, y); all f64, every product and sum rounded on its own (no contraction), in this order:
 *   1. X = (M0 x + M1 y) + M2,  Y = (M3 x + M4 y) + M5,  W = (M6 x + M7 y) + M8.
 *   2. iw = (W != 0) ? 32.0 / W : 0.0 — one IEEE divide; no test on the sign of W, as in cv2.  fx = X iw, fy = Y iw.
 *   3. ok = |fx| <= 2^30 && |fy| <= 2^30 (false for NaN).  A pixel that is not ok gets border_value in every channel, under either
 *      border mode, and is not covered.
 *   4. ix = rint(fx), iy = rint(fy), ties to even.  sx = ix >> 5, ax = ix & 31, sy = iy >> 5, ay = iy & 31 (arithmetic shift: floor):
 *      cv2's 5 fractional bits of INTER_LINEAR.
 *   5. The taps are (sx, sy), (sx+1, sy), (sx, sy+1), (sx+1, sy+1) = p00, p01, p10, p11.  A tap outside [0, sw) x [0, sh) reads
 *      border_value under OFK_BORDER_CONSTANT and the pixel at the clamped coordinates under OFK_BORDER_REPLICATE.
 *   6. Per channel: out = ((32-ax)(32-ay) p00 + ax (32-ay) p01 + (32-ax) ay p10 + ax ay p11 + 512) >> 10, in integers.  (cv2's
 *      fixed-point sum exactly: its 15-bit weights (a/32)(b/32) 2^15 are the integers 32 a b, which sum to 2^15 without a fix-up,
 *      and (32 s + 2^14) >> 15 = (s + 512) >> 10.)
 *   7. A pixel is COVERED when it is ok and all four taps are inside the source.  covered [batch] i32 (nullable): covered pixels per image.
 * This is cv2's interpolation arithmetic, not its evaluation of the coordinates (cv2 steps X, Y, W along a row block by block, which
 * may round a tie differently).
 * OFK_E_INVALID before any launch: channels other than 1 and 3; batch, sh x sw or dh x dw beyond the context's; a border other than
 * the two; border_value outside 0..255; a NULL src, M or dst. */
#define OFK_BORDER_CONSTANT   0
#define OFK_BORDER_REPLICATE  1
int ofk_warp_perspective(ofk_ctx *ctx, const uint8_t *src, int sh, int sw, int channels, const double *M, uint8_t *dst, int dh, int dw,
                         int border, int border_value, int batch, int *covered);

/* The same warp through a lens: image rectification (cv2.undistort, cv2.fisheye.undistortImage) and, with a matrix, the warp of a raw
 * frame into an ideal view - one kernel, k_warp_lens_u8: the perspective warp with the lens's forward map behind the homography.
 * src [batch][sh][sw][channels] u8, the RAW images of camera `cam` -> dst [batch][dh][dw][channels] u8; channels 1 or 3.  M [batch][9]
 * f64 maps a DESTINATION pixel to an IDEAL pixel of the source camera, i.e. a pixel of the output matrix (fo_x, fo_y, co_x, co_y) of
 * `cam`; M == NULL is the identity for every image: plain rectification into that matrix.  One camera per call.
 * The rule, per destination pixel with integer (x, y); all f64, every product and sum rounded on its own (no contraction), in this order:
 *   1. Normalised matrix, once per image: Mn[0..2] = (M[0..2] - co_x M[6..8]) / fo_x, Mn[3..5] = (M[3..5] - co_y M[6..8]) / fo_y,
 *      Mn[6..8] = M[6..8].
 *   2. X = (Mn0 x + Mn1 y) + Mn2, Y and W alike.  iw = (W != 0) ? 1.0 / W : 0.0 - no test on the sign of W, as in the plain warp.
 *      xn = X iw, yn = Y iw: the ideal normalised coordinates.
 *   3. (xd, yd) = the forward map of ofk_set_camera ("Distort") on (xn, yn), its expressions unchanged.  Where the Brown model's k4, k5
 *      and k6 (k[5..7]) are all 0 the divide by the denominator, which is exactly 1.0, is left out; no bit of the frame depends on it.
 *   4. fx = (xd cam.fx + cam.cx) 32, fy = (yd cam.fy + cam.cy) 32.
 *   5. A pixel is OUTSIDE unless |fx| <= 2^30 and |fy| <= 2^30 (false for NaN) and, where r_max > 0, xn xn + yn yn <= r_max r_max
 *      (false for NaN).  An outside pixel gets border_value in every channel, under either border mode, and is not covered.  r_max
 *      bounds the ideal radius: a Brown polynomial with k1 < 0 folds back far outside the field of view, and ideal points out there
 *      would sample the inside of the raw frame (cv2.undistort shows that artefact).  0: no bound.
 *   6. Steps 4-7 of ofk_warp_perspective on (fx, fy): rint to even, 5 fractional bits, four taps, (sum + 512) >> 10, the border per
 *      tap, covered = not outside and all four taps inside.  The same device code.
 * Parity with cv2 is not claimed (cv2 interpolates a block-wise fixed-point map); this rule defines the result.
 * OFK_E_INVALID before any launch: ofk_warp_perspective's refusals (M may be NULL here); a NULL cam or one ofk_undistort_points would
 * refuse (model OFK_CAMERA_OFF included; fo_x != fo_y is accepted); r_max negative or not finite.  It touches no resident state. */
struct ofk_camera;                                              /* defined with ofk_set_camera, below */
int ofk_warp_lens(ofk_ctx *ctx, const struct ofk_camera *cam, const uint8_t *src, int sh, int sw, int channels, const double *M, uint8_t *dst,
                  int dh, int dw, int border, int border_value, double r_max, int batch, int *covered);

/* Shi-Tomasi response inside cv2.goodFeaturesToTrack (of_module.py:44,86; node:120,163; evaluate_exp.py:66,106;
 * of_library.py:238): Sobel-3 -> structure tensor box(block_size) -> min eigenvalue, f32 map [batch][h][w].
 * block_size 1..45. */
int ofk_mineig_response(ofk_ctx *ctx, const uint8_t *gray, int batch, int h, int w, int block_size, float *eig);

/* Selection half of cv2.goodFeaturesToTrack: > quality*max, 3x3 local max, sort (value desc, linear index desc: OpenCV's greaterThanPtr),
 * greedy min-distance, top max_corners.  mask (nullable) [batch][h][w] u8, 0 = excluded.
 * pts [batch][max_corners][2] f32, counts [batch]. max_corners in 1..ctx max_pts. */
int ofk_select_corners(ofk_ctx *ctx, const float *eig, const uint8_t *mask, int batch, int h, int w, int max_corners,
                       double quality, double min_distance, float *pts, int *counts);

/* cv2.goodFeaturesToTrack(gray, mask=mask, maxCorners, qualityLevel, minDistance, blockSize) — same call sites. */
int ofk_good_features(ofk_ctx *ctx, const uint8_t *gray, const uint8_t *mask, int batch, int h, int w, int max_corners,
                      double quality, double min_distance, int block_size, float *pts, int *counts);

/* The corner grid: a per-cell cap inside the greedy selection (the bucketing the reference gestures at with its cluster and mask
 * helpers, of_library.py:116-226, and what the re-detection of velocity_measurment_node.py:157-166 lacks: it only masks discs around
 * the old tracks, nothing steers the new corners towards the parts of the frame that have none).  Off by default; with it off every
 * entry point launches the kernels and returns the bits it always did.
 * Candidates and their order are unchanged: a candidate passes the mask, is > f32(f64(max) * quality) and a 3x3 local maximum; order
 * is value descending, then linear index descending; a candidate's rank is its place in that order, from 0.
 * The acceptance test, applied to each candidate in rank order, with occ[] the corners per cell:
 *   1. Stop if max_corners corners are accepted, if every cell holds occ >= cap, or if the candidate's rank >= max_rank (max_rank != 0).
 *   2. c = (y / cell) * gw + x / cell, integer division, gw = ceil(w / cell).  If occ[c] >= cap, skip the candidate.
 *   3. The minDistance test against all accepted corners, as always.  If it fails, skip.
 *   4. Accept the candidate and increment occ[c].
 * (The stop on full cells cannot change the corners: no later candidate passes step 2.  It is part of the rule because it fixes the
 * statistics.)  occ starts at zero, or, with an occupancy list occ_pts [batch][occ_stride][2] f32 / occ_counts [batch], as the number
 * of listed points i < min(occ_counts[b], occ_stride) whose truncated position ((int)x, (int)y) lies in the cell; points whose
 * truncated position is outside the image (or not a number) are ignored.  Occupancy points take no part in the minDistance test (a
 * stream step keeps its disc mask for that).  A cap that can never bind (>= max_corners with an empty list, say) gives exactly the
 * plain result.
 * Statistics, 2 x int32 per image: corners accepted; candidates examined = rank of the last candidate steps 2-4 decided, plus one
 * (the rank of the acceptance that filled the budget or the last open cell, plus one, when the pass stopped there; 0 when nothing was
 * decided, an image without budget in a re-detection included).
 * Refused with OFK_E_INVALID before any launch, a setting staying as it was: cell < 0; cap < 1 with cell > 0; max_rank < 0;
 * ceil(w / cell) * ceil(h / cell) > OFK_GRID_MAX_CELLS for the frame at hand (checked by the call that selects, the frame being
 * unknown to ofk_set_corner_grid); occ_stride outside 1..ctx max_pts with an occupancy list.
 * ofk_set_corner_grid (NULL or cell 0: off) is a context setting read by ofk_good_features, ofk_select_corners, ofk_pairs_run (every
 * slice), ofk_stream_begin[_jpeg], the replace-mode re-detection of ofk_stream_step_fused[_jpeg] and the append-mode re-detection of
 * every stream step.  The append-mode re-detection passes the OLD tracks (the points and counts its disc mask is drawn from) as the
 * occupancy list, so it refills the cells the tracks have left; all others start from empty cells.
 * ofk_good_features_grid / ofk_select_corners_grid: the two stage entries with the grid (g NULL or cell 0: off) and the occupancy
 * list (occ_pts NULL: empty) as arguments; they ignore the context setting.
 * ofk_corner_grid_download: stats [batch][2] i32 of the latest selection that ran with a grid on (`batch` is that selection's own);
 * OFK_E_INVALID before such a selection. */
#define OFK_GRID_MAX_CELLS 2048
typedef struct ofk_corner_grid {
    int cell;      /* cell edge in pixels; 0 = off (every other field ignored) */
    int cap;       /* most corners a cell may hold, >= 1 */
    int max_rank;  /* 0 = unlimited; else only the first max_rank candidates in rank order are ever examined */
} ofk_corner_grid;
int ofk_set_corner_grid(ofk_ctx *ctx, const ofk_corner_grid *g);
int ofk_get_corner_grid(const ofk_ctx *ctx, ofk_corner_grid *g);
int ofk_corner_grid_download(ofk_ctx *ctx, int *stats);
int ofk_select_corners_grid(ofk_ctx *ctx, const float *eig, const uint8_t *mask, int batch, int h, int w, int max_corners,
                            double quality, double min_distance, float *pts, int *counts, const ofk_corner_grid *g,
                            const float *occ_pts, const int *occ_counts, int occ_stride);
int ofk_good_features_grid(ofk_ctx *ctx, const uint8_t *gray, const uint8_t *mask, int batch, int h, int w, int max_corners,
                           double quality, double min_distance, int block_size, float *pts, int *counts, const ofk_corner_grid *g,
                           const float *occ_pts, const int *occ_counts, int occ_stride);

/* Exclusion zones: the solve stage's verdict fed back into the re-detection.  The reference's earlier tracker looped "find cluster ->
 * mask -> re-detect" on the host (of_library.py:146-226: distancecluster, convexhull, circles); here a per-stream table of zones lives
 * on the device, is built from the points the solve stage rejected, moves along with the object and is zeroed in the re-detection mask
 * beside the track discs, so a re-detection does not put corners straight back on an independently moving object.  Off by default;
 * with it off every stream step launches the kernels and returns the bits it always did.  Streams only: ofk_pairs_run ignores the
 * setting.
 * Per stream and per step, in this order; all image arithmetic is integer (64-bit where products need it):
 *   1. Rejects: the points i < count whose status behind the track gates is 1 and whose keep flag behind the solve stage (the
 *      feasibility rule, the legacy keep, the robust drop) is 0; lost tracks never count.  A reject's position is ((int)x, (int)y) of
 *      its OLD position - k_disc_mask's convention and the frame the re-detection runs on - each axis first brought into
 *      -32768..32767 (not a number: -32768); its flow is (double)new - (double)old per axis.
 *   2. Refresh: a reject whose position lies inside the shape (rule 5) of a live zone sets that zone's ttl back to the setting's, for
 *      every such zone, and takes no part in rule 3.
 *   3. Cluster: the remaining rejects fall into connected components, two of them linked when |dx| < link && |dy| < link
 *      (of_library.distancecluster's rule); a component's id is its smallest point index; components are handled in ascending id.
 *   4. Insert: a component of at least min_members rejects becomes a zone.  Vertices: the convex hull of the members' positions,
 *      duplicates merged, collinear points removed, in the order of Andrew's chain (points sorted by x then y; lower chain, then upper);
 *      a hull of more than OFK_ZONE_VERTS vertices is replaced by the bounding box (x0,y0),(x1,y0),(x1,y1),(x0,y1).  flow = f32 of the
 *      members' f64 flow sum (ascending index) divided by their number; off = (0,0); ttl = the setting's.  The zone goes to the free
 *      slot of lowest index below max_zones; with none free it replaces the zone of smallest ttl among them, ties to the lowest slot.
 *   5. Shape: V = the vertices + rint(off) (half to even; each axis brought into +-2^20, not a number: -2^20).  A pixel p is in the
 *      zone when (a) there are at least 3 vertices and cross(b - a, p - a) >= 0 for every edge a -> b, or (b) for some edge, with
 *      t = (p - a).(b - a) and L = |b - a|^2: |p - a|^2 <= r^2, or |p - b|^2 <= r^2, or 0 < t < L and cross^2 <= r^2 L.  One vertex
 *      is a disc, two are a capsule.
 *   6. Mask: on a step that re-detects, every live zone's pixels are zeroed in the mask behind the track discs; the replace-mode
 *      re-detection of ofk_stream_step_fused (no mask without zones) runs behind a mask of the zones alone, which are in the previous
 *      frame's coordinates at that point.
 *   7. Advect and age, at the end of the step, the zones inserted in it included: off = off + flow in f32, ttl -= 1, a zone at 0 is
 *      freed (its slot reads all zero).
 * ofk_stream_begin[_jpeg] clears the table; a held step (ofk_fusion.hold_on_skip) leaves it untouched.
 * ofk_set_zones: NULL or mode OFK_ZONES_OFF switches the feature off.  OFK_E_INVALID, the setting staying as it was: a mode that is
 * neither, link outside 1..4096, min_members outside 1..ctx max_pts, radius outside 0..255, ttl outside 1..65535, max_zones outside
 * 1..OFK_ZONE_MAX.
 * ofk_zones_step, the stage entry: rules 1-7 on host arrays (old_pts / new_pts [batch][stride][2] f32, status / keep [batch][stride]
 * u8, counts [batch]) against the context's resident table with the context's setting (which must be on); mask_out [batch][h][w] u8 =
 * mask_in (NULL: all ones) with every stream's live zones zeroed (rule 6).  Positions beyond +-32767 are taken as rule 1 states.
 * ofk_zones_reset: clears the tables of the first `batch` streams.
 * ofk_zones_download, all of the context's max_batch streams (a NULL buffer is skipped):
 *   zones  [max_batch][OFK_ZONE_MAX][OFK_ZONE_INTS] i32: ttl (0 = free), vertices, members, then OFK_ZONE_VERTS x (x, y)
 *   motion [max_batch][OFK_ZONE_MAX][OFK_ZONE_FLOATS] f32: off x, y; flow x, y
 *   stats  [max_batch][OFK_ZONE_STATS] i32 of the latest step: live zones behind rule 7, zones inserted, zones refreshed, inserts that
 *          replaced a live zone, rejects seen, rejects absorbed by rule 2, sweeps of rule 3's labelling; the eighth slot is reserved and reads 0. */
#define OFK_ZONES_OFF  0
#define OFK_ZONES_HULL 1
#define OFK_ZONE_MAX   16
#define OFK_ZONE_VERTS 32
#define OFK_ZONE_INTS  67
#define OFK_ZONE_FLOATS 4
#define OFK_ZONE_STATS 8
typedef struct ofk_zones { int mode; int link; int min_members; int radius; int ttl; int max_zones; } ofk_zones;
int ofk_set_zones(ofk_ctx *ctx, const ofk_zones *z);
int ofk_get_zones(const ofk_ctx *ctx, ofk_zones *z);
int ofk_zones_step(ofk_ctx *ctx, const float *old_pts, const float *new_pts, const uint8_t *status, const uint8_t *keep, const int *counts,
                   int batch, int stride, int h, int w, const uint8_t *mask_in, uint8_t *mask_out);
int ofk_zones_reset(ofk_ctx *ctx, int batch);
int ofk_zones_download(ofk_ctx *ctx, int *zones, float *motion, int *stats);

/* cv2.calcOpticalFlowPyrLK(prev, next, prevPts, None, winSize=(win,win), maxLevel, criteria=(EPS|COUNT, max_count, eps))
 * — of_module.py:88; node:133; evaluate_exp.py:98; of_library.py:249.
 * prev_pts/next_pts [batch][pts_stride][2] f32, counts [batch] (points used per image, <= pts_stride),
 * status [batch][pts_stride] u8, err [batch][pts_stride] f32.  win odd, 3..31. */
int ofk_lk_pyr(ofk_ctx *ctx, const uint8_t *prev, const uint8_t *next, int batch, int h, int w, const float *prev_pts,
               const int *counts, int pts_stride, int win, int max_level, int max_count, double eps, double min_eig_thr,
               float *next_pts, uint8_t *status, float *err);

/* cv2's operation flags of calcOpticalFlowPyrLK (same values).  Semantics against oracle/image_oracle.c:orc_lk_pyr:
 *   OFK_LK_USE_INITIAL_FLOW   at the TOP pyramid level the search starts at init_pts * 2^-L instead of at the point; everything else
 *                             (per-level bounds tests, the carry through a skipped level, criteria clamps) is unchanged, so
 *                             init_pts == prev_pts gives the plain result bit for bit;
 *   OFK_LK_GET_MIN_EIGENVALS  next_pts and status as without the flag; err = the f32 minEig of the level-0 normal matrix (before the
 *                             threshold test, whatever the status becomes), 0 where level 0 was skipped.  No L1 residual is computed.
 * ofk_lk_pyr_ex = ofk_lk_pyr plus `flags` and the start positions init_pts [batch][pts_stride][2] (NULL unless USE_INITIAL_FLOW is
 * set; then required, every used coordinate finite with |c| <= 1e6, else OFK_E_INVALID before any launch). */
#define OFK_LK_USE_INITIAL_FLOW   4
#define OFK_LK_GET_MIN_EIGENVALS  8
int ofk_lk_pyr_ex(ofk_ctx *ctx, const uint8_t *prev, const uint8_t *next, int batch, int h, int w, const float *prev_pts,
                  const int *counts, int pts_stride, int win, int max_level, int max_count, double eps, double min_eig_thr,
                  const float *init_pts, int flags, float *next_pts, uint8_t *status, float *err);

/* Seeding LK from the sensor model: the flow the pair's sensors predict (ofk_flow_model's expression) is applied BEFORE tracking.
 * Per point, float64, in this order, no contraction:
 *   x = (px - cx) * scaling, y likewise; k = (n0 x + n1 y + n2) / d;
 *   w0 = om1 - om2 y, w1 = om2 x - om0, w2 = om0 y - om1 x;
 *   fx = k (v0 - v2 x) + (w0 - w2 x), fy = k (v1 - v2 y) + (w1 - w2 y);
 *   seed = (float)(px + gain * fx / scaling), y likewise.
 * OFK_SEED_MODEL: v = the prior velocity; OFK_SEED_ROTATION: v = 0 (gyro-aided tracking when height or velocity are not trusted);
 * OFK_SEED_OFF: no seeding (the default).  Sources: sensors[0] d, [1..3] normal, [4..6] omega, [19..21] scaling, cx, cy, [22..24] prior
 * velocity; with ofk_fusion.use_imu the normal, omega and velocity of the resident IMU state (state[15..17], [18..20], [0..2]).
 * scaling == 0, d == 0 or a seed coordinate that is not finite or exceeds 1e6 in magnitude: the seed is the point itself.
 * `gain` (default 1) reconciles units, e.g. omega per second against flow per frame.
 * ofk_set_lk_seed is a context setting read by ofk_pairs_run (every slice), ofk_stream_step[_jpeg] and ofk_stream_step_fused[_jpeg]:
 * a k_seed_points launch writes the start positions in front of LK, which then runs with OFK_LK_USE_INITIAL_FLOW.
 * ofk_predict_points is the predictor as a stage entry on host buffers (pts, seed_out [batch][stride][2] f32, counts [batch],
 * sensors [batch][OFK_SENSOR_DOUBLES]); it touches no resident state, so it returns the exact seeds a resident run used. */
#define OFK_SEED_OFF       0
#define OFK_SEED_MODEL     1
#define OFK_SEED_ROTATION  2
int ofk_set_lk_seed(ofk_ctx *ctx, int mode, double gain);
int ofk_get_lk_seed(const ofk_ctx *ctx, int *mode, double *gain);
int ofk_predict_points(ofk_ctx *ctx, const float *pts, const int *counts, int batch, int stride, const double *sensors, int mode,
                       double gain, float *seed_out);

/* Track table: an identity per track of a video stream, resident on the device, and LK seeded from each track's own last flow.
 * A stream hands back anonymous points; with ofk_set_track_table on, every row of the tracks a call returns has an id, an age, a
 * birth step, a birth position and the flow of the step it last survived.  Off by default; with it off every stream step launches
 * the kernels and returns the bits it always did.  Streams only: ofk_pairs_run ignores the setting.
 * State per stream: step (i32), next_id (u32; it wraps around after 2^32 births, which is not handled), per track row r < count:
 * id (u32), age (i32, steps survived), birth_step (i32), birth_xy (2 x f32), flow_xy (2 x f32); and step_ids [max_pts] u32.  Rows are
 * in the order of the `tracks` the same call returns.
 *   1. Begin (ofk_stream_begin[_jpeg]): step = 0; row r < n: id = r, age = 0, birth_step = 0, birth_xy = the position, flow_xy = 0;
 *      next_id = n.
 *   2. Replace (ofk_fusion.redetect_replace, the streams whose budget is positive, behind k_replace_tracks): rows r < n =
 *      max(new count, 0) get id = next_id + r, age = 0, birth_step = step, birth_xy = the new position, flow_xy = 0; next_id += n.
 *      Other streams are untouched.
 *   3. Update (in front of k_update_tracks, on the steps that launch it): step_ids[i] = id[i] for i < n_old, the ids of the rows
 *      ofk_stream_last_points and the records' points speak of.  The rows with status[i] != 0 are kept in order, status being what
 *      k_update_tracks reads: the keep flags behind the gates, the feasibility rule and the robust drop.  A kept row keeps id and
 *      birth_*, age + 1, flow = next[i] - prev[i] per coordinate, one f32 subtraction of the raw pixels.  Then
 *      extra = max(0, min(new count, max_total - kept, stride - kept)) rows (0 without a re-detection; max_total <= stride wherever
 *      this runs, so the last term is idle) are appended, as for every other state of the rows: id = next_id + j, age = 0,
 *      birth_step = step + 1, birth_xy = the position, flow = 0.  next_id += extra; step += 1.
 *   4. A held step (ofk_fusion.hold_on_skip, not solved) leaves table, step, next_id, step_ids and the statistics as they were (a
 *      replace in front of it has happened).
 *   5. Seed (seed = OFK_TT_SEED_FLOW), behind k_seed_points and, with a camera, behind the launch that brings the model seeds back
 *      into the image - the last flow lives in raw pixels.  A row with age >= 1: t = (float)gain * flow (one f32 multiply),
 *      s = pos + t (one f32 add), no contraction; the seed is s if |s.x| <= 1e6 and |s.y| <= 1e6 (false for a NaN), else the point
 *      itself.  A row with age == 0 keeps what ofk_set_lk_seed wrote if that setting is on, else it gets the point itself.  LK (the
 *      lighting-insensitive one if selected) then runs with OFK_LK_USE_INITIAL_FLOW; a seed equal to the point gives the plain
 *      result bit for bit.  The gate's backward pass is unchanged.  Newborn tracks have no flow: at a reduced pyramid depth they
 *      need ofk_set_lk_seed or slow motion.
 *   6. Statistics per stream, int[OFK_TT_STATS]: count, kept, lost = n_old - kept, born, oldest age, step, next_id, the rows
 *      i < n_old of this step that rule 5 seeded from their flow (0 with the seed off).  Begin: n, 0, 0, n, 0, 0, n, 0.  Replace:
 *      n, 0, the count before, n, 0, step, next_id, 0.
 * ofk_set_track_table: NULL or mode OFK_TT_OFF switches the feature off.  OFK_E_INVALID, the setting staying as it was: a mode
 * that is neither OFK_TT_OFF nor OFK_TT_ON, a seed that is neither OFK_TT_SEED_OFF nor OFK_TT_SEED_FLOW, a gain that is not finite.
 * The buffers (32 bytes per track and the per-stream words) are allocated when a stream first begins or steps with the setting on;
 * streams that step with the setting on without a table of their current tracks (the setting came on, or was off for a step, after
 * ofk_stream_begin) start one there by rule 1, in front of everything else in the step.
 * ofk_track_table_download, the streams of the latest begin or step with the setting on, the first min(stride, max_pts) rows of
 * each (every output may be NULL; OFK_E_INVALID before such a call): ids, age, birth_step, step_ids [batch][stride], birth_xy,
 * flow_xy [batch][stride][2], stats [batch][OFK_TT_STATS].
 * ofk_track_table_step, rule 3 and 6 on host buffers (it touches no resident state): the table rows in and out in place (ids, age,
 * birth_step [batch][stride], birth_xy, flow_xy [batch][stride][2]), head [batch][2] = step, next_id in and out, prev_pts / next_pts
 * [batch][stride][2], status [batch][stride], counts [batch] in (n_old) and out (the new count), new_pts / new_counts (NULL: none),
 * max_total <= stride, step_ids [batch][stride] and stats out (either may be NULL).  t: the setting whose seed and gain the eighth
 * statistic takes (NULL: seed off).
 * ofk_track_seed_points, rule 5 on host buffers: pts [batch][stride][2], counts, age [batch][stride], flow_xy, gain; seed_io holds
 * the model seeds on entry when keep_age0 != 0 (age-0 rows stay as they are), and the start positions on return. */
#define OFK_TT_OFF        0
#define OFK_TT_ON         1
#define OFK_TT_SEED_OFF   0
#define OFK_TT_SEED_FLOW  1
#define OFK_TT_STATS      8
typedef struct ofk_track_table { int mode; int seed; double gain; } ofk_track_table;
int ofk_set_track_table(ofk_ctx *ctx, const ofk_track_table *t);
int ofk_get_track_table(const ofk_ctx *ctx, ofk_track_table *t);
int ofk_track_table_download(ofk_ctx *ctx, uint32_t *ids, int *age, int *birth_step, float *birth_xy, float *flow_xy, uint32_t *step_ids,
                             int stride, int *stats);
int ofk_track_table_step(ofk_ctx *ctx, const ofk_track_table *t, uint32_t *ids, int *age, int *birth_step, float *birth_xy, float *flow_xy,
                         int *head, const float *prev_pts, const float *next_pts, const uint8_t *status, int *counts, const float *new_pts,
                         const int *new_counts, int max_total, int batch, int stride, uint32_t *step_ids, int *stats);
int ofk_track_seed_points(ofk_ctx *ctx, const float *pts, const int *counts, int batch, int stride, const int *age, const float *flow_xy,
                          double gain, int keep_age0, float *seed_io);

/* Depth per track: an inverse depth per row of the track table, filtered over the frames on the device, and the velocity solved from
 * the depths of the earlier frames (v_map), which needs neither the ground plane nor this frame's range reading.  Off by default;
 * with it off every stream step allocates, launches and returns what it always did.  Streams only: ofk_pairs_run ignores the setting.
 * It needs ofk_set_track_table on.  Nothing of the records, `fused`, the tracks or the table changes with it on: v_map is reported
 * in a record of its own.
 * State per track row, in the table's row order, in arrays of their own: rho (f64, the inverse depth at the row's current position),
 * var (f64), nobs (i32, measurements taken; 0 = no depth yet).  Per stream a record of OFK_TD_DOUBLES.
 * Points and units: the points are the solve's own (the ideal points behind the camera, rolling-shutter and finite-motion rewrites);
 * x = (next - c) * scaling, u = (next - prev) * scaling as the solve forms them, p = (x, y, 1), q = (u, 0) + p x omega, omega what the
 * step's solve read (the sensors' behind the gyro-bias apply, the IMU state's under use_imu); v = fields 0-2 of the step's record as
 * the chain left it; solved = record[15] != 0 (ofk_stream_step's record carries no such flag: there it is rank = record[4] >= 3).
 * sigma_flow and b_min are given in pixels and multiplied by the stream's `scaling` in the stream steps; ofk_track_depth_step takes
 * them in the units of its points.  All arithmetic is f64 without contraction in the order written; the sums are the solve's (four
 * waves over the rows i = tid + 256 k, the shuffle butterfly, (s0 + s1) + (s2 + s3)).
 * One launch, k_track_depth_step, directly in front of k_track_table_update on exactly the steps that launch it (a held step leaves
 * state and record alone), on the status and counts k_update_tracks reads.  n = min(max(counts, 0), stride).  In order:
 *   1. Map solve, from the state as the previous step left it.  Mature rows: status != 0, nobs >= min_obs, rho > 0 and
 *      var <= (rel_max * rho)^2.  Their rows rho_i X_i v = X_i q_i enter the solve's own least squares with (sA, sB) = (rho_i, 1):
 *      its ten sums, its Jacobi, its rank rule.  v_map = M^+ g, C_map = sigma_flow^2 M^-1; the depths' variances are NOT propagated
 *      into C_map, which is therefore a lower bound.  Map flag 1 (v_map and C_map read 0): fewer than min_rows mature rows,
 *      rank < 3, or a sum that is not finite.  Nothing of this step's record is read, so v_map does not depend on this frame's d.
 *   2. Measurement, where solved and v is finite, for the rows with status != 0: a = (q - q_z p)_xy, b = (v_x - v_z x, v_y - v_z y),
 *      bb = b.b, |b| = sqrt(bb), z = kappa = a.b / bb, r = (a x b) / |b|.  The row is skipped and counted if |b| < b_min (slot 7); else
 *      if gate > 0 and r r > (gate gate)(sigma_flow sigma_flow) (slot 8); else if z is not finite (slot 7).  R = sigma_flow^2 / bb.
 *      nobs == 0: (rho, var, nobs) = (z, R, 1) if z > 0 (slot 6), else the row stays.  Any other row, with update != 0: nu = z - rho,
 *      S = var + R; skipped and counted if gate > 0 and nu nu > (gate gate) S (slot 9); else K = var / S, rho = rho + K nu,
 *      var = var R / S (product form: it cannot go negative), nobs += 1 (slot 5).  update == 0 leaves rows with nobs >= 1 to rule 3.
 *   3. Prediction to the next frame (P' = v + omega x P gives Z+ = Z g), every kept row with nobs >= 1.  Solved:
 *      w = omega_x y - omega_y x, g = (1 + rho v_z) + w; g finite and >= 0.1: J = (1 + w) / (g g), rho = rho / g, var = var J J + q;
 *      otherwise the row is reset to (0, 0, 0) (slot 20).  Not solved: var = var + q.
 *   4. Compaction: the rows with status != 0 move up in order, extra = max(0, min(new count, max_total - kept, stride - kept)) rows
 *      (0 without a re-detection) are appended as (0, 0, 0).  Rows beyond are not defined.
 * Record: 0-2 v_map, 3 map flag, 4 mature rows used, 5 rows updated, 6 rows initialised, 7 skipped for |b| (or z not finite), 8 skipped
 * for the cross-flow, 9 skipped for the innovation, 10-15 C_map's upper triangle, 16-18 the v rule 2 read, 19 solved, 20 rows reset by
 * rule 3, the rest 0.
 * The rows are zeroed where the table's begin and replace rules run; streams that step with the setting on without depths of their
 * current tracks start there with zeroed rows.  The buffers (20 bytes per track, the records) are allocated by the first step with
 * the setting on.
 * ofk_set_track_depth: NULL or mode OFK_TD_OFF switches the feature off.  OFK_E_INVALID, the setting staying as it was: a mode that is
 * neither, sigma_flow <= 0, b_min < 0, gate < 0 (0: no gates), q < 0, min_obs < 1, rel_max <= 0, min_rows < 3, a value that is not
 * finite.  Defaults behind "off": 0.2, 0.5, 3, 0, 3, 0.25, 8, update 1.
 * OFK_E_INVALID before any launch from a stream step with the setting on: ofk_set_track_table off; OFK_SOLVE_OFMODULE,
 * OFK_FLOW_ROTATIONAL, OFK_KEEP_LEGACY (not the sensor model).
 * ofk_track_depth_download, the streams of the latest step with the setting on, the first min(stride, max_pts) rows of each (every
 * output may be NULL): rho, var [batch][stride] f64, nobs [batch][stride] i32, rec [batch][OFK_TD_DOUBLES].
 * ofk_track_depth_reset: rows 0..n-1 of active stream b are loaded from rho, var, nobs (n <= max_pts, nobs >= 0) - a depth hint from
 * outside, e.g. a row with nobs 1 and a wide var; the other rows stay (streams without depths of their tracks get zeroed rows first).
 * ofk_track_depth_step, rules 1-4 on host buffers (it touches no resident state): x, u [batch][stride][2] f64, status
 * [batch][stride], counts [batch], omega, v [batch][3], solved [batch] i32, the state rho, var, nobs [batch][stride] in and out in
 * place, new_counts [batch] (NULL: none), max_total <= stride, rec [batch][OFK_TD_DOUBLES] out (may be NULL). */
#define OFK_TD_OFF      0
#define OFK_TD_ON       1
#define OFK_TD_DOUBLES  32
typedef struct ofk_track_depth { int mode; double sigma_flow; double b_min; double gate; double q; int min_obs; double rel_max; int min_rows; int update; } ofk_track_depth;
int ofk_set_track_depth(ofk_ctx *ctx, const ofk_track_depth *t);
int ofk_get_track_depth(const ofk_ctx *ctx, ofk_track_depth *t);
int ofk_track_depth_download(ofk_ctx *ctx, double *rho, double *var, int *nobs, int stride, double *rec);
int ofk_track_depth_reset(ofk_ctx *ctx, int b, const double *rho, const double *var, const int *nobs, int n);
int ofk_track_depth_step(ofk_ctx *ctx, const ofk_track_depth *t, const double *x, const double *u, const uint8_t *status, const int *counts,
                         const double *omega, const double *v, const int *solved, double *rho, double *var, int *nobs, const int *new_counts,
                         int max_total, int batch, int stride, double *rec);

/* Track templates: the patch a track was born with, kept per row of the track table, the window of every later frame compared with
 * it through the accumulated image deformation, and the position pulled back onto it (the monitoring half of Shi and Tomasi's "Good
 * Features to Track").  LK tracks frame to frame, every step starts from the previous step's result, so its sub-pixel errors add up,
 * and the forward-backward gate and err_max see two neighbouring frames only.  Off by default; with it off every stream step
 * allocates, launches and returns what it always did.  Streams only: ofk_pairs_run ignores the setting.  It needs
 * ofk_set_track_table on.  Everything lives in raw pixels of pyramid level 0, like the table's flow_xy; the camera, rolling-shutter
 * and finite-motion rewrites run behind it and read the status and the next points it leaves, as do the solves, the zones' copy of
 * the status, the depths and the table's flow_xy.
 * State per track row, in the table's row order, in arrays of their own: tmpl ((win+2)^2 u8, row-major, the window plus a rim of one
 * pixel for the gradients; `tmpl_stride` = (win+2)^2 rounded up to a multiple of 4 bytes apart), A (4 f32, row-major: template offsets
 * to image offsets), ncc (f32, the latest score), flag (u8, the latest verdict, | OFK_TPL_CAPTURED on the step that captured the
 * row), tstate (u8: 0 no template, 1 has one).  Per stream a record of OFK_TPL_DOUBLES.
 * The sampler S(img, p, A, o), o = (ox, oy) integers: sx = (a00 ox + a01 oy) + p.x, sy = (a10 ox + a11 oy) + p.y in f32;
 * ix = floorf(sx), qx = rint((sx - ix) 32) with ties to even, likewise y; outside if sx or sy is not finite, ix < 0, iy < 0,
 * ix + 1 > w - 1 or iy + 1 > h - 1; otherwise the integer I00 (32-qx)(32-qy) + I01 qx (32-qy) + I10 (32-qx) qy + I11 qx qy, the value
 * at scale 1024.  Every sum below is over such integers and exact in int64, so it does not depend on the order of the additions.
 *   1. Step map (k_track_affine, one workgroup per stream, behind LK and the track gates).  n = min(max(counts, 0), stride); the
 *      rows i < n with status != 0; x = prev - c, y = next - c in f64, c = (w/2, h/2).  Minimise sum |M x + t - y|^2: the sums of
 *      z z^T, z y_0 and z y_1 with z = (x_0, x_1, 1) in the solve's order (i = tid + 256 k, the shuffle butterfly,
 *      (s0 + s1) + (s2 + s3)), k_lstsq.inc's Jacobi once and its rank rule with the row count for `rows`, both right-hand sides from the
 *      one decomposition.  fit_gate > 0: a second fit over the rows with |M x + t - y|^2 <= fit_gate^2 under the first; it replaces
 *      the first when at least fit_min rows remain and it has rank 3 and finite sums.  L = I with fit flag 1 when fewer than
 *      fit_min rows are present, the rank is below 3 or a sum is not finite.  L is M rounded to f32 once; the record carries f64.
 *   2. Capture (k_track_template, one wave per row, for every row i < n): a row with age == 0 or tstate == 0 takes
 *      (S(prev level 0, prev point, I, o) + 512) >> 10 for o in -h-1..h+1, h = (win-1)/2, as its template, A = I, tstate = 1.  If a
 *      sample is outside the row has no template: tstate = 0, and with status != 0 its flag is NO_TEMPLATE, the row kept as LK left it.
 *   3. Score, rows with status != 0 and a template.  A' = L A, each entry L_r0 a_0c + L_r1 a_1c in f32.  T(o) the template's inner
 *      window, g(o) = (T(o + e_x) - T(o - e_x), T(o + e_y) - T(o - e_y)), J(o) = S(next level 0, p, A', o), D = J - 1024 T, N = win^2,
 *      vT = N sum T^2 - (sum T)^2, vJ = N sum J^2 - (sum J)^2, cTJ = N sum T J - sum T sum J, rho = (double)cTJ /
 *      sqrt((double)vT (double)vJ), stored as f32.  At p = LK's next point: OUTSIDE if a sample is outside (the row is kept, or with
 *      outside = OFK_TPL_DROP status = 0, without a score); else FLAT if vT <= 0 or vJ <= 0 (kept without a verdict).
 *   4. Re-anchor, at most anchor_iters times from p = LK's next point.  Gc = N sum g g^T - (sum g)(sum g)^T, bc = N sum g D -
 *      (sum g)(sum D) (a bias between the frames drops out); det = Gc00 Gc11 - Gc01 Gc01 in f64, det <= 0: no anchor.
 *      delta = (Gc11 bc.x - Gc01 bc.y, Gc00 bc.y - Gc01 bc.x) / det / 512; s = A' delta in f64; q = (float)((double)p - s).  The anchor
 *      is abandoned (p = LK's point again, the score the one taken there, flag ABANDONED) if s is not finite, if |q - p_LK| exceeds
 *      (float)anchor_max in x or y (f32), or if a sample at q is outside.  Otherwise p = q, and the walk stops when s.s < 1e-4.
 *   5. Verdict at the final p: FLAT (next stays LK's) if vJ <= 0 there; rho < ncc_min (f64): status = 0, next stays LK's, FAIL;
 *      otherwise next = p, PASS (ABANDONED where rule 4 says so).  Rows with status == 0 on entry are not touched (NOT_TRACKED).
 *   6. Compaction (k_track_template_update, one workgroup per stream, directly in front of k_track_table_update on the steps that
 *      launch it, with its keep rule status != 0): the kept rows carry tmpl, A', ncc, flag and tstate up in order; a kept row with a
 *      template whose det A' (a00 a11 - a01 a10 in f32) exceeds (float)scale_max^2 or falls below (float)(1 / scale_max^2), or is no
 *      number, gets tstate = 0 (scale_max = 0: never) and is captured afresh by the next step at its position then; the
 *      extra = max(0, min(new count, max_total - kept, stride - kept)) appended rows get A = I, ncc = 0, flag 0, tstate = 0.  The
 *      templates move from one buffer into a second one, which the host swaps.  The counts of the record come from the flags by
 *      ballot and popcount.
 * A held step runs rules 1-5 and not rule 6: A, the scores, the flags, the counts and the templates of rows with tstate = 1 stay; rows
 * with tstate = 0 may be captured, as the next step would with the same bits.
 * Record: 0-3 M, 4-5 t, 6 fit flag, 7 / 8 rows in the first / second fit, 9 rms residual in px of the rows of the fit that stands,
 * 10 rows scored (PASS, FAIL, ABANDONED), 11 rows dropped (FAIL, and OUTSIDE under OFK_TPL_DROP), 12 rows moved, 13 abandoned, 14 outside, 15 flat, 16 captured, 17 without a
 * template, 18 marked for refresh, 19 largest move in px (x or y), 20-31 0.  Slots 10-19 are written by rule 6.
 * Streams that step with the setting on without templates of their current tracks (the setting switched on in mid-stream, or set
 * again) start with tstate = 0 everywhere.  The buffers are allocated by the first step with the setting on, once and for the widest
 * window, so that a later win needs no reallocation: two template buffers of 1092 bytes per row of max_batch x max_pts (about 70 MB at
 * 64 streams of 500 rows; the default window of 15 uses 27 % of it) and 47 bytes per row for the rest.
 * ofk_set_track_template: NULL or mode OFK_TPL_OFF switches the feature off.  OFK_E_INVALID, the setting staying as it was: a mode
 * that is neither, win even or outside 5..31, ncc_min outside [-1, 1], anchor_iters outside 0..8, anchor_max <= 0, outside neither
 * OFK_TPL_KEEP nor OFK_TPL_DROP, fit_min < 3, fit_gate < 0 (0: a single fit), scale_max neither 0 nor >= 1, a value that is not
 * finite.  Defaults behind "off": 15, 0.8, 3, 2.0, keep, 6, 2.0, 1.5.
 * OFK_E_INVALID before any launch from a stream step with the setting on: ofk_set_track_table off.
 * ofk_track_template_download, the streams of the latest step with the setting on, the first min(stride, max_pts) rows of each (every
 * output may be NULL): tmpl [batch][stride][tmpl_stride of the setting], A [batch][stride][4], ncc [batch][stride] f32, flag, tstate
 * [batch][stride] u8, rec [batch][OFK_TPL_DOUBLES].
 * ofk_track_affine_fit, rule 1 on host buffers: prev_pts, next_pts [batch][stride][2] f32, status [batch][stride], counts [batch], the
 * frame's h and w; rec [batch][OFK_TPL_DOUBLES] out (slots 0-9, the rest 0), L [batch][4] f32 out (may be NULL).
 * ofk_track_template_step, rules 2-6 on host buffers (it touches no resident state): prev, next [batch][h][w] gray; prev_pts
 * [batch][stride][2]; next_pts and status in and out in place, rows as tracked; age [batch][stride] i32; counts [batch]; L
 * [batch][4] f32; the state tmpl [batch][stride][tmpl_stride], A, ncc, flag, tstate in and out in place, compacted; new_counts
 * [batch] (NULL: none), max_total <= stride; rec [batch][OFK_TPL_DOUBLES] out (slots 10-19, the rest 0; may be NULL). */
#define OFK_TPL_OFF          0
#define OFK_TPL_ON           1
#define OFK_TPL_DOUBLES      32
#define OFK_TPL_KEEP         0
#define OFK_TPL_DROP         1
#define OFK_TPL_NOT_TRACKED  0
#define OFK_TPL_PASS         1
#define OFK_TPL_FAIL         2
#define OFK_TPL_ABANDONED    3
#define OFK_TPL_OUTSIDE      4
#define OFK_TPL_FLAT         5
#define OFK_TPL_NO_TEMPLATE  6
#define OFK_TPL_CAPTURED     16
typedef struct ofk_track_template { int mode; int win; double ncc_min; int anchor_iters; double anchor_max; int outside; int fit_min; double fit_gate; double scale_max; } ofk_track_template;
int ofk_set_track_template(ofk_ctx *ctx, const ofk_track_template *t);
int ofk_get_track_template(const ofk_ctx *ctx, ofk_track_template *t);
int ofk_track_template_download(ofk_ctx *ctx, uint8_t *tmpl, float *A, float *ncc, uint8_t *flag, uint8_t *tstate, int stride, double *rec);
int ofk_track_affine_fit(ofk_ctx *ctx, const ofk_track_template *t, const float *prev_pts, const float *next_pts, const uint8_t *status,
                         const int *counts, int batch, int stride, int h, int w, double *rec, float *L);
int ofk_track_template_step(ofk_ctx *ctx, const ofk_track_template *t, const uint8_t *prev, const uint8_t *next, int h, int w,
                            const float *prev_pts, float *next_pts, uint8_t *status, const int *age, const int *counts, const float *L,
                            uint8_t *tmpl, float *A, float *ncc, uint8_t *flag, uint8_t *tstate, const int *new_counts, int max_total,
                            int batch, int stride, double *rec);

/* Keyframe per stream: the displacement against a frame that is held fixed.  Every solve works on one frame pair, so a stream knows
 * its position only as a sum of per-frame velocities, whose error grows without bound.  With this setting on a stream keeps, per row
 * of the track table, the row's ideal pixel in a KEYFRAME and, per stream, the rotation accumulated since; every step solves the
 * translation T of P_c = R_acc P_K + T from finite motion's relation (n.p_c)/d [q~]x T = [q~]x (p_c - q~), q~ = R_acc p_K
 * renormalised, which is exact for a pair any distance apart and linear in T.  Off by default; with it off every stream step
 * allocates, launches and returns what it always did.  Streams only: ofk_pairs_run ignores the setting.  It needs ofk_set_track_table
 * on.  Nothing of the records, `fused`, the tracks, the table, the depths or the templates changes with it on: the position is
 * reported in a record of its own, not fed back.  It removes the drift of the flow, not of the gyro: R_acc is the product of the
 * steps' rotations, and a constant error in omega is ofk_set_gyro_bias's job.
 * State per track row, in the table's row order, in arrays of their own: key_xy (2 f32, the row's ideal pixel in the keyframe),
 * member (u8, 1 = the row was alive at the keyframe).  Per stream: state [OFK_KEY_STATE] f64 = R_acc (0-8, row-major), anchor (9-11),
 * pos (12-14), 15 unused; istate [OFK_KEY_INTS] i32 = key_step, members_at_key, keyframes so far, dead-reckoned steps; a record of
 * OFK_KEY_DOUBLES.
 * The points are the ideal NEXT points of the step: behind the camera model and the rolling shutter, in FRONT of the finite-motion
 * rewrite (which replaces the next point by q~ of the neighbouring pair).  With finite motion on beside a camera or a rolling shutter
 * that rewrite is in place, and the step keeps one device copy of the next points in front of it; otherwise the buffers the rewrite
 * read are intact behind the solve.
 * Per stream: sn = the sensor row; d = sn[0]; n = sn[1..3], omega = sn[4..6], R_world = sn[7..15] (under use_imu the IMU state's
 * normal, ang and rotation); offset = sn[16..18]; scaling, c = sn[19], sn[20..21].  omega is what the step's solve read (behind the
 * gyro-bias apply).  sigma_flow and gate are given in pixels and multiplied by `scaling`.  v_uav = fields 8-10 of the step's record as
 * the chain left it, solved = record[15] != 0 (ofk_stream_step: rank = record[4] >= 3), and v_uav finite.  step = the table's step.
 * All arithmetic is f64 without contraction in the order written; sums of three are (a + b) + c; the sums over rows are the solve's
 * (four waves over the rows i = tid + 256 k, the shuffle butterfly, (s0 + s1) + (s2 + s3)); Jacobi and rank rule are the solve's.
 * One launch, k_keyframe_step, one workgroup per stream, on exactly the steps that launch k_track_table_update (a held step leaves
 * state and record alone) and in front of the depths', the templates' and the table's update, on the status and counts
 * k_update_tracks reads.  n = min(max(counts, 0), stride).  In order:
 *   1. Rotate (every step, solved or not).  th2 = (o0 o0 + o1 o1) + o2 o2; A = 1, B = 0.5 if th2 < 1e-16, else th = sqrt(th2),
 *      A = sin(th) / th, B = (1 - cos(th)) / th2 (rs_rotate3's coefficients, for a rotation by +omega).  K = [omega]x,
 *      K2_ij = o_i o_j - (i == j ? th2 : 0); E_ij = ((i == j ? 1 : 0) + A K_ij) + B K2_ij; R_acc_ij = (E_i0 R_0j + E_i1 R_1j) + E_i2 R_2j.
 *      angle = acos(min(1, max(-1, (((R00 + R11) + R22) - 1) / 2))), fmin / fmax: a trace that is no number reads -1, the angle pi.
 *   2. Key solve over the rows i < n with status != 0 and member != 0 (their number is `live`).  k = (key_xy - c) scaling,
 *      p = (next - c) scaling; (X, Y, Z) = R_acc (k, 1), each (R_i0 kx + R_i1 ky) + R_i2.  The row is left out unless
 *      Z >= OFK_KEY_MIN_DEPTH, den = (n0 px + n1 py) + n2 has |den| >= 1e-12 and s = nq / den > 0, with a = X / Z, b = Y / Z,
 *      nq = (n0 a + n1 b) + n2 (each false for NaN).  x^ = (a, b), u^ = (s (px - a), s (py - b)), sA = nq / d: the row enters the
 *      solve's sums as acc_point(x^, (u^, 0), sA, 1).  T = M^+ g.  Flag 2: members_at_key == 0 (no keyframe; nothing is solved).
 *      Flag 1: fewer than min_rows rows, rank < 3 or a sum that is not finite.  Flag 0 otherwise.
 *      gate > 0 and flag 0: r = u^ - sA (T_xy - T_z x^); a second solve over the rows with r.r <= (gate scaling)^2; it replaces the
 *      first when it has at least min_rows rows, rank 3 and finite sums.  rms = sqrt(sum r.r / rows) / scaling over the rows and
 *      under the T of the solve that stands.  C_T = (sigma_flow scaling)^2 M^-1 of that solve from the same Jacobi, entry (i, j) =
 *      ((V_i0 V_j0 / l0 + V_i1 V_j1 / l1) + V_i2 V_j2 / l2); the points' correlation over frames is not in it: a lower bound.
 *   3. Position.  Flag 0: w_i = T_i + (offset_i - ((R_i0 offset_0 + R_i1 offset_1) + R_i2 offset_2)), D_i = (Rw_i0 w_0 + Rw_i1 w_1) +
 *      Rw_i2 w_2, pos = anchor + D; a D that is not finite (an offset or an R_world that is no number) makes the flag 1, T and rms
 *      0, and the step goes on as below.  This is v_uav's sign convention: to first order D is the sum of the records' fields 8-10 since
 *      the keyframe.  Any other flag: pos += v_uav where the step's record is solved, pos stays otherwise; D = pos - anchor; the
 *      dead-reckoned count goes up by one.
 *   4. Re-key, when any of these holds; the record carries the lowest number and the set as bits (1 << (number - 1)):
 *      1 flag != 0;  2 live < min_rows;  3 live < min_share members_at_key (in f64);  4 angle > rot_max;
 *      5 max_age > 0 and (step + 1) - key_step > max_age.
 *   5. Compaction: the rows with status != 0 move up in order with key_xy and member;
 *      extra = max(0, min(new count, max_total - kept, stride - kept)) rows (0 without a re-detection) are appended with member 0
 *      and key_xy 0: raw detections without an ideal position, they join at the next re-key.  On a re-key every kept row gets
 *      key_xy = its ideal next point and member = 1, anchor = pos, R_acc = I, members_at_key = kept, key_step = step + 1, and the
 *      keyframe count goes up by one.  Rows beyond are not defined.
 * Record: 0-2 T, 3 flag, 4 / 5 rows of the first / the gated solve (5: 0 when none ran), 6 rms in px, 7 members_at_key and 8 key_step
 * behind rule 5, 9 re-key reason (0: none), 10-12 D, 13-15 pos, 16-18 anchor behind rule 5, 19 angle of R_acc in front of rule 5,
 * 20-25 C_T's upper triangle, 26 keyframes so far, 27 dead-reckoned steps, 28 live, 29 1 where the gated solve stands, 30 the reasons
 * as bits, 31 0.  T, rms and C_T read 0 unless flag 0.
 * k_keyframe_begin / k_keyframe_replace run where the table's begin and replace rules run: both clear the members and
 * members_at_key; begin also zeroes anchor, pos and the counts, sets R_acc = I and the record to zero with flag 2.  The first step
 * behind them reports flag 2, dead-reckons once and keys on the rows it tracked.  Streams that step with the setting on without
 * such state (switched on in mid-stream) start the same way.  The buffers (17 bytes per track, the per-stream state) are allocated
 * by the first step with the setting on.
 * ofk_set_keyframe: NULL or mode OFK_KEY_OFF switches the feature off.  OFK_E_INVALID, the setting staying as it was: a mode that is
 * neither, sigma_flow <= 0, gate < 0 (0: a single solve), min_rows < 3, min_share outside [0, 1], rot_max <= 0, max_age < 0 (0: no
 * limit), a value that is not finite.  Defaults behind "off": 0.2, 2.0, 8, 0.5, 0.5, 0.
 * OFK_E_INVALID before any launch from a stream step with the setting on: ofk_set_track_table off; OFK_SOLVE_OFMODULE,
 * OFK_FLOW_ROTATIONAL, OFK_KEEP_LEGACY (not the sensor model).
 * ofk_keyframe_download, the streams of the latest step with the setting on, the first min(stride, max_pts) rows of each (every
 * output may be NULL): key_xy [batch][stride][2] f32, member [batch][stride] u8, R_acc [batch][9], rec [batch][OFK_KEY_DOUBLES].
 * ofk_keyframe_reset: anchor = pos = the given position (NULL: zero) for active stream b, R_acc = I, the members cleared, the record
 * zero but for flag 2, pos, anchor, key_step and the two counts: the next step reports flag 2, dead-reckons from there and keys (streams without state get it first).
 * ofk_keyframe_step, rules 1-5 on host buffers (it touches no resident state): next_pts [batch][stride][2] f32 ideal next points,
 * status [batch][stride], counts [batch], sensors [batch][OFK_SENSOR_DOUBLES], v_uav [batch][3], solved [batch] i32, step [batch]
 * i32, the state key_xy, member, state [batch][OFK_KEY_STATE], istate [batch][OFK_KEY_INTS] in and out in place, new_counts [batch]
 * (NULL: none), max_total <= stride, rec [batch][OFK_KEY_DOUBLES] out (may be NULL). */
#define OFK_KEY_OFF        0
#define OFK_KEY_ON         1
#define OFK_KEY_DOUBLES    32
#define OFK_KEY_STATE      16
#define OFK_KEY_INTS       4
#define OFK_KEY_MIN_DEPTH  0.1
#define OFK_KEY_SOLVED     0
#define OFK_KEY_UNSOLVED   1
#define OFK_KEY_NONE       2
#define OFK_KEY_RE_FLAG    1
#define OFK_KEY_RE_ROWS    2
#define OFK_KEY_RE_SHARE   3
#define OFK_KEY_RE_ANGLE   4
#define OFK_KEY_RE_AGE     5
typedef struct ofk_keyframe { int mode; double sigma_flow; double gate; int min_rows; double min_share; double rot_max; int max_age; } ofk_keyframe;
int ofk_set_keyframe(ofk_ctx *ctx, const ofk_keyframe *k);
int ofk_get_keyframe(const ofk_ctx *ctx, ofk_keyframe *k);
int ofk_keyframe_download(ofk_ctx *ctx, float *key_xy, uint8_t *member, int stride, double *R_acc, double *rec);
int ofk_keyframe_reset(ofk_ctx *ctx, int b, const double *anchor);
int ofk_keyframe_step(ofk_ctx *ctx, const ofk_keyframe *k, const float *next_pts, const uint8_t *status, const int *counts,
                      const double *sensors, const double *v_uav, const int *solved, const int *step, float *key_xy, uint8_t *member,
                      double *state, int *istate, const int *new_counts, int max_total, int batch, int stride, double *rec);

/* Keyframe rotation: the accumulated rotation refined from the flow.  The key solve of ofk_set_keyframe takes R_acc, the bare product
 * of the steps' rotations, as exact, and loses about 1.5 d |error of R_acc|: gyro noise, a scale-factor error or a time-stamp offset
 * all accumulate in it over a keyframe's life.  With this setting on beside ofk_set_keyframe, rule 2 of the keyframe solves the
 * translation T together with a small rotation delta, R^ = exp([delta]x) R_acc, under a Gaussian prior on delta; rules 1 and 3-5 run
 * unchanged on the T and R^ that stand, and the keyframe's record and state keep their layout.  Off by default; with it off every
 * step allocates, launches and returns what it always did.  k_keyframe_step_rot is launched in k_keyframe_step's place, on exactly
 * the same steps; when every axis is held by the setting alone (axes all 0, or the sigmas of the source all 0) k_keyframe_step itself
 * runs and state and record are those of the setting off (rotation record: flag OFK_KEYROT_HELD, otherwise zero).
 * R_acc in the state stays the SOURCE's rotation: every step estimates delta from it afresh, nothing of delta^ is carried forward.
 * (The key pixels' noise is common to all steps of one keyframe; a recursion over steps that ignores this is overconfident.)
 * State of the setting's own per stream, rstate [OFK_KEYROT_STATE] f64: R_world at the keyframe (0-8, row-major), 9: 1 = valid, 10:
 * the key_step it belongs to, 11 unused.  Rule 5 writes it on every re-key (R_world of the step: sn[7..15], under use_imu the IMU
 * state's rotation; valid = 1; key_step = step + 1); k_keyrot_clear zeroes it, and sets the rotation record to zero with flag
 * OFK_KEYROT_NONE, where k_keyframe_begin, k_keyframe_replace (the streams with a budget) and k_keyframe_reset run.  A held step
 * leaves it alone.
 * Arithmetic, sums over rows, Jacobi: as ofk_set_keyframe states them.  sf = sigma_flow scaling.  In order, in the rules' places:
 *   1'. Source.  OFK_KEYROT_GYRO: R_acc is rule 1's product.  OFK_KEYROT_ATTITUDE, where members_at_key != 0, rstate is valid and
 *       its key_step is the keyframe's: R_acc_ij = (Rw_0i K_0j + Rw_1i K_1j) + Rw_2i K_2j, K = R_world at the keyframe, in the
 *       product's place (it is what rule 5 stores); otherwise the step runs as source gyro, prior included (record 35 says which).
 *       Prior variance per axis, age = (step + 1) - key_step in f64: gyro age sigma_gyro^2 + (age sigma_bias)(age sigma_bias);
 *       attitude 2 (sigma_att sigma_att).  Axis k is HELD when axes[k] == 0 or the variance is not > 0; otherwise its prior
 *       precision in the rows' units is L_k = sf^2 / variance (an infinite variance: 0, the axis is free).
 *   2'. The first walk under R_acc is rule 2's; it gives the plain T, flag and row count.  Unless the plain flag is 0 the joint
 *       solve is not attempted (OFK_KEYROT_NONE); with all axes held it is not either (OFK_KEYROT_HELD).  Otherwise, with the row's
 *       x^ = (a, b), u^, sA under the current R^ = exp([delta]x) R_acc (rule 1's coefficients), to first order in a further rotation
 *       delta' composed on the left: u^ = sA (T_xy - T_z x^) + B delta', B = [[-ab, 1 + a^2, -b], [-(1 + b^2), ab, a]] (the
 *       derivative of x^; rotfield's sign for a rotation by +omega).  In the solve's own cross-product rows, p = (a, b, 1),
 *       N = [p]x^T [p]x = (p.p) I - p p^T, c_k = (B_0k, B_1k, 0), q = (u^, 0), a walk adds to the solve's eleven sums (M, g of
 *       acc_point) eighteen more: M_Td[i][k] += sA (N c_k)_i, M_dd[k][l] += c_k . (N c_l) (k <= l), g_d[k] += c_k . (N q); every
 *       product with N is (N_i0 x + N_i1 y).  One Gauss-Newton step from sums with at least min_rows rows: Jacobi of M (it must
 *       pass the solve's rank rule with rank 3, all sums finite), Mi = M^-1 from it as rule 2 writes C_T, Y = Mi M_Td, t0 = Mi g;
 *       S_kl = (M_dd_kl + (k == l ? L_k : 0)) - ((M_Td_0k Y_0l + M_Td_1k Y_1l) + M_Td_2k Y_2l), h_k = (g_d_k - L_k delta_k) -
 *       ((M_Td_0k t0_0 + M_Td_1k t0_1) + M_Td_2k t0_2); a held axis has its row and column of S zero, the diagonal 1 and h 0.
 *       Jacobi of S; it must be finite with every eigenvalue > 0 and > eps max(3 rows, 3) times the largest, else
 *       OFK_KEYROT_SINGULAR.  delta' = S^-1 h through the eigenvectors as the solve does; T = t0 - Y delta'; delta += delta'.  No
 *       6 x 6 is factorised.  `iters` such steps, the first on the first walk's sums, each further one on a walk under the new R^.
 *       gate > 0: the rows inside are those whose residual r = u^ - sA (T_xy - T_z x^) under the first joint solve's R^ and T has
 *       r.r <= (gate scaling)^2; over them `iters` further steps starting from the first solve's delta, each on a walk of its own;
 *       they replace the first solve when every walk had min_rows rows and every step stood.  |delta^| > delta_max:
 *       OFK_KEYROT_LARGE (not finite: _SINGULAR).  With any flag but OFK_KEYROT_OK the plain rule 2 runs on, gate and all, and gives
 *       the bits of the setting off.  rms: over the rows of the solve that stands, under its R^ and T, divided by their number.
 *       C_delta = sf^2 S^-1 (held axes 0); C_T = sf^2 (Mi + Y S^-1 Y^T), the marginal with the rotation's share in it; both of the
 *       last step of the solve that stands.  The prior is what keeps them honest within one step; like rule 2's C_T they ignore that
 *       the key pixels' noise is shared across the steps of a keyframe.
 *   3-5. As ofk_set_keyframe, with R^ in the lever-arm term and in the angle of rule 4 (record 19) where the joint solve stands.
 *       The state's R_acc is the source's.  Rule 3's D is first formed under R^ and the joint T; one that is not finite withdraws the
 *       joint solve in front of the plain rule 2 (the rotation's flag OFK_KEYROT_NONE, delta^ and slots 32-34 zero), which then runs
 *       as with the setting off and refuses the step itself.
 * The keyframe's record: T, rms, rows (5: the first gated walk's), gated and C_T are those of the solve that stands.
 * Rotation record, OFK_KEYROT_DOUBLES: 0-2 delta^ (also the refused one under _LARGE; else 0), 3 flag, 4-12 R^ (R_acc where the plain
 * solve stands), 13-18 C_delta's upper triangle, 19-24 C_T's (the keyframe record's 20-25), 25-27 the eigenvalues of S descending
 * (a held axis contributes its 1), 28-30 the prior's sigma per axis (0: held, inf: free), 31 Gauss-Newton steps of the solve that
 * stands (0: plain), 32-34 the plain first solve's T, 35 1 where R_acc came from the attitudes, 36 age, 37 rows of the standing joint
 * solve's last walk, 38-39 0.
 * ofk_set_keyframe_rotation: NULL or mode OFK_KEYROT_OFF switches it off.  OFK_E_INVALID, the setting staying as it was: an unknown
 * mode or source, a sigma that is negative or not finite (sigma_gyro and sigma_bias may be +inf: free), iters outside
 * 1..OFK_KEYROT_MAX_ITERS, delta_max <= 0 or NaN.  Defaults behind "off": gyro, axes 1 1 1, sigma_gyro 0, sigma_bias 1e-4, sigma_att
 * 1e-3, iters 2, delta_max 0.1.  OFK_E_INVALID before any launch from a stream step with the setting on and ofk_set_keyframe off.
 * ofk_keyframe_rotation_download: rec [batch][OFK_KEYROT_DOUBLES] of the streams of the latest step with the setting on.
 * ofk_keyframe_reset also clears the stream's rotation state.
 * ofk_keyframe_rotation_step: ofk_keyframe_step's arguments and meaning (it touches no resident state), plus the rotation setting r,
 * rstate [batch][OFK_KEYROT_STATE] in and out in place and rrec [batch][OFK_KEYROT_DOUBLES] out (may be NULL). */
#define OFK_KEYROT_OFF        0
#define OFK_KEYROT_ON         1
#define OFK_KEYROT_GYRO       0
#define OFK_KEYROT_ATTITUDE   1
#define OFK_KEYROT_DOUBLES    40
#define OFK_KEYROT_STATE      12
#define OFK_KEYROT_MAX_ITERS  8
#define OFK_KEYROT_OK         0
#define OFK_KEYROT_NONE       1
#define OFK_KEYROT_SINGULAR   2
#define OFK_KEYROT_LARGE      3
#define OFK_KEYROT_HELD       4
typedef struct ofk_keyframe_rotation { int mode; int source; int axes[3]; double sigma_gyro, sigma_bias, sigma_att; int iters; double delta_max; } ofk_keyframe_rotation;
int ofk_set_keyframe_rotation(ofk_ctx *ctx, const ofk_keyframe_rotation *r);
int ofk_get_keyframe_rotation(const ofk_ctx *ctx, ofk_keyframe_rotation *r);
int ofk_keyframe_rotation_download(ofk_ctx *ctx, double *rec);
int ofk_keyframe_rotation_step(ofk_ctx *ctx, const ofk_keyframe *k, const ofk_keyframe_rotation *r, const float *next_pts,
                               const uint8_t *status, const int *counts, const double *sensors, const double *v_uav, const int *solved,
                               const int *step, float *key_xy, uint8_t *member, double *state, int *istate, const int *new_counts,
                               int max_total, int batch, int stride, double *rec, double *rstate, double *rrec);

/* Keyframe map: the key solve from per-track depths, not the ground plane.  Rule 2 of ofk_set_keyframe gives every member the depth of
 * one plane, rho_c = (n.p_c)/d; over a roof, a canopy or a ramp that is wrong, and the range reading d enters every key solve.  With
 * this setting on beside ofk_set_keyframe and ofk_set_track_depth (both must be on) the depth filter's rho and var are frozen per
 * track row at the keyframe, and the key translation is solved against them: a translation-only PnP against fixed landmarks that reads
 * neither n nor d.  Off by default; with it off every step allocates, launches and returns what it always did.  k_keyframe_step_map is
 * launched in k_keyframe_step's place on exactly its steps; k_track_depth_step is not touched and still runs behind it.  Streams only.
 * The relation.  For a member, k its scaled key pixel, (X, Y, Z) = R_acc (k, 1), rho_K its inverse z-depth at the keyframe, p its
 * scaled ideal next point: P_c = (X, Y, Z) / rho_K + T and p = P_c,xy / P_c,z give exactly (rho_K / Z) (T_xy - T_z p) = p - (a, b),
 * a = X / Z, b = Y / Z: a row of the solve's own form with x^ = p, u^ = p - (a, b), sA = rho_K / Z, linear in T, exact at any distance,
 * its residual r = u^ - sA (T_xy - T_z x^) a pixel difference in the current frame.  On a plane it is rule 2's row times Z_c.
 * Where the key depth comes from.  A re-key at table step k keys on the step's ideal next points and sets key_step = k + 1;
 * k_track_depth_step, behind it in the same step, predicts every depth to that same frame and compacts by the same keep rule.  At the
 * NEXT launch the depth state therefore holds rho, var, nobs at the keyframe for exactly the member rows, in their order: rule M1
 * captures them then.
 * State per track row, in the table's row order: key_rho, key_var (f64; 0, 0 = no map depth).  Per stream: mstate [2] i32 =
 * (captured_for: the key_step the rows were captured for, map_rows: the mature rows captured; 0 behind a re-key) and a record of
 * OFK_KEYMAP_DOUBLES.  Arithmetic, sums over rows, Jacobi, rank rule, compaction: as ofk_set_keyframe states them.  A row of the depth
 * state is MATURE when nobs >= min_obs, rho > 0 and var <= (rel_max rho)(rel_max rho), each false for NaN (this setting's min_obs and
 * rel_max, not the depth setting's); a stream without depth state has no mature row.  In order, around rules 1-5:
 *   M1. Capture, in front of rule 2, when members_at_key != 0 and captured_for != key_step: every row i < n with member != 0 gets
 *       (key_rho, key_var) = (rho, var) where it is mature, else (0, 0); map_rows = the mature ones, captured_for = key_step.
 *   M2. A LIVE MAP ROW has status != 0, member != 0 and key_rho > 0 (false for NaN).  use_map = map_rows >= min_rows and live map rows
 *       >= min_rows (this setting's min_rows).  Rule 2's first walk and solve always run as they stand (they give `live`); with use_map
 *       false all of rule 2 runs, bit for bit: flag OFK_KEYMAP_NONE where map_rows < min_rows, else OFK_KEYMAP_FEW.
 *   M3. Map solve, over the live map rows.  k, p, (X, Y, Z) as rule 2; the row is left out unless Z >= OFK_KEY_MIN_DEPTH.  a = X / Z,
 *       b = Y / Z, x^ = p, u^ = (px - a, py - b), sA = key_rho / Z.  sf = sigma_flow scaling.  weights 1: w = sf^2 / (sf^2 +
 *       ((u0 u0 + u1 u1) key_var) / (key_rho key_rho)), the parallax times the relative depth error beside the pixel noise; weights 0:
 *       w = 1.  The row enters the sums as acc_point(x^, (u^, 0), sA, 1) with sa2 = sA sA w and sab = sA 1 w (acc_point_w's order) and
 *       counts as one row.  T = M^+ g; the solve stands with at least min_rows rows (this setting's), rank 3 and finite sums.  gate > 0:
 *       a second solve over the rows with w r.r <= (gate scaling)^2 under the first T; it replaces the first with at least the
 *       keyframe's min_rows rows, rank 3 and finite sums.  Over the rows of the solve that stands and under its T: rms = sqrt(sum w r.r
 *       / rows) / scaling, spread = sqrt(sum w r.r / sum w) / scaling.  C_T = sf^2 M^-1 of that solve as rule 2 writes it.  Where the
 *       map solve stands (OFK_KEYMAP_USED) flag, T, rows 4 / 5, rms, gated and C_T of the keyframe's record are its own, whatever the
 *       plain first solve gave, and the rest of rule 2 does not run.  Where it does not (OFK_KEYMAP_FELL_BACK) rule 2 runs on untouched.
 *       Rule 3 and the keyframe's record keep their layout; a D that is not finite refuses the step as rule 3 says: the keyframe's
 *       flag is then 1 and its T, rms and C_T 0, while the map record stays as M3 left it - OFK_KEYMAP_USED and slots 3-6 speak of
 *       M3 alone, the keyframe's flag says whether the step stood.
 *   M4. Re-key reason 6 (OFK_KEY_RE_MAP, bit 32) beside rule 4's: ready_share > 0, map_rows < min_rows, and among the live rows
 *       (status != 0, member != 0) `ready` rows of the depth state as it stands are mature with ready >= min_rows and ready >=
 *       ready_share live (in f64).  Without it a keyframe born before any depth matured would stay a plane keyframe for life.
 *   M5. Compaction: key_rho and key_var move with key_xy; appended rows and every row of a re-key get (0, 0), and M1 fills them at the
 *       next launch.
 * Map record, OFK_KEYMAP_DOUBLES: 0 flag, 1 map_rows behind M1, 2 live map rows, 3 / 4 rows of the first / the gated map solve, 5 sum of
 * weights, 6 spread (3-6: 0 unless use_map; 4-6: 0 unless the map solve stands), 7-9 the plain first solve's T where use_map and
 * that solve stood (else 0), 10 rows captured this step, 11 captured_for behind M1, the rest 0.
 * k_keymap_clear runs behind k_keyframe_begin (and where a stream steps with this setting on without map state: switched on in
 * mid-stream), k_keyframe_replace (the streams with a budget; the record stays) and k_keyframe_reset: rows (0, 0), map_rows 0,
 * captured_for = the keyframe's key_step - the depth state of that moment is not the keyframe's, so nothing is captured before the
 * next re-key, which M4 brings about - and the record zero with flag OFK_KEYMAP_NONE.  The buffers (16 bytes per track, the
 * per-stream state) are allocated by the first step with the setting on.
 * Not in it: the joint rotation over map rows (a stream step with ofk_set_keyframe_rotation on beside this setting is refused);
 * refining key_rho from later frames; the map's common error in the position filter's `share`; pairs.  Beside ofk_set_finite_motion
 * the depths are taken at the solve's rewritten points and the key solve at the ideal points in front of the rewrite, as each does
 * without the other; the combination runs (README, "Keyframe map", says what it was measured at).
 * ofk_set_keyframe_map: NULL or mode OFK_KEYMAP_OFF switches it off.  OFK_E_INVALID, the setting staying as it was: an unknown mode,
 * min_obs < 1, rel_max <= 0, min_rows < 3, ready_share outside [0, 1], weights not 0 or 1, a value that is not finite.  Defaults behind
 * "off": 3, 0.02, 8, 0.5, 1.  OFK_E_INVALID before any launch from a stream step with the setting on: ofk_set_keyframe or
 * ofk_set_track_depth off; ofk_set_keyframe_rotation on.
 * ofk_keyframe_map_download, the streams of the latest step with the setting on, the first min(stride, max_pts) rows of each (every
 * output may be NULL): key_rho, key_var [batch][stride] f64, rec [batch][OFK_KEYMAP_DOUBLES].
 * ofk_keyframe_reset also clears the stream's map.
 * ofk_keyframe_map_step: ofk_keyframe_step's arguments and meaning (it touches no resident state), plus the map setting m, the depth
 * state rho, var [batch][stride] f64 and nobs [batch][stride] i32 (read only; all NULL: no depth state), the map state key_rho, key_var
 * [batch][stride] f64 and mstate [batch][2] i32 in and out in place, and mrec [batch][OFK_KEYMAP_DOUBLES] out (may be NULL). */
#define OFK_KEYMAP_OFF        0
#define OFK_KEYMAP_ON         1
#define OFK_KEYMAP_DOUBLES    32
#define OFK_KEYMAP_USED       0
#define OFK_KEYMAP_NONE       1
#define OFK_KEYMAP_FEW        2
#define OFK_KEYMAP_FELL_BACK  3
#define OFK_KEY_RE_MAP        6
typedef struct ofk_keyframe_map { int mode; int min_obs; double rel_max; int min_rows; double ready_share; int weights; } ofk_keyframe_map;
int ofk_set_keyframe_map(ofk_ctx *ctx, const ofk_keyframe_map *m);
int ofk_get_keyframe_map(const ofk_ctx *ctx, ofk_keyframe_map *m);
int ofk_keyframe_map_download(ofk_ctx *ctx, double *key_rho, double *key_var, int stride, double *rec);
int ofk_keyframe_map_step(ofk_ctx *ctx, const ofk_keyframe *k, const ofk_keyframe_map *m, const float *next_pts, const uint8_t *status,
                          const int *counts, const double *sensors, const double *v_uav, const int *solved, const int *step, float *key_xy,
                          uint8_t *member, double *state, int *istate, const int *new_counts, int max_total, int batch, int stride,
                          double *rec, const double *rho, const double *var, const int *nobs, double *key_rho, double *key_var, int *mstate,
                          double *mrec);

/* Position filter per stream: keyframe, velocity and position fixes fused.  The keyframe's D is drift-free while the keyframe lives, but
 * its pos re-anchors at every re-key, so its error is a random walk over the re-keys; a fix (GPS, a marker) has no way into a stream;
 * and the key pixels' noise is common to all steps of one keyframe, so a filter that took D every step as an independent position
 * measurement would be overconfident.  With this setting on beside ofk_set_keyframe every stream keeps a Kalman filter with a CLONED
 * state on the device: the position at the keyframe is carried beside the current one, D measures their difference, and a re-key
 * copies the current position, with its covariance and cross-covariances, into the clone.  Off by default; with it off every step
 * allocates, launches and returns what it always did.  Reported, not fed back: nothing else reads p.  Streams only: ofk_pairs_run
 * ignores it.
 * State per stream: x [OFK_POSF_STATES = 12] f64 = (p 0-2: position, world frame, v_uav's convention; v 3-5: velocity per unit of dt,
 * in v_uav's units; b 6-8: accelerometer bias as in ekf6; c 9-11: the clone of p at the keyframe); P [12][12] f64 row-major; istate
 * [OFK_POSF_INTS = 16] i32: 0 steps, 1 fresh (1 = no D update since the last clone), 2 clones, 3 started, 4-6 the velocity updates
 * applied / gated / refused, 7-9 the displacement's, 10-12 the fix's, 13-15 unused.
 * Input row per stream, [OFK_POSF_INPUT = 12] f64, consumed and zeroed by the next step that runs the filter (not held, the setting
 * on): 0-2 du, the velocity increment over the step in the world frame (zeros: none; a component that is not finite is taken as 0;
 * under OFK_CONTROL_IMU the caller passes what ofk_imu_state returns as dv - the fuse kernel's own use of imu_dv is not touched), 3
 * fix valid (0 / not 0), 4-6 the fix's position, 7-9 its sigma per axis, 10-11 unused.
 * k_pos_filter_step runs on exactly the steps that launch the keyframe's step kernel, in one launch directly behind it; a held step
 * leaves state, record and input alone.  It reads the step's record (v_uav 8-10; "solved" as rule 3 of the keyframe defines it), the
 * keyframe's record of this step (flag 3, re-key reason 9, D 10-12, C_T 20-25) and R_world as the keyframe read it (sensor slots
 * 7-15, the IMU state's under use_imu).  All arithmetic is f64 in the order written, no fused multiply-add; a sum of three terms is
 * (t0 + t1) + t2.  In order:
 *   1. Start, where istate[3] == 0 (behind ofk_stream_begin, behind ofk_pos_filter_reset, on the first step with the setting on after
 *      one without it; on host buffers: whatever the caller hands in with istate[3] == 0): p = c = x[0..2] as it stands (the given
 *      position; zero by default), v = b = 0; P = 0 but for the diagonals of the blocks pp, pc, cp, cc = p0_p^2, vv = p0_v^2, bb =
 *      p0_b^2; fresh = 1, started = 1.
 *   2. Predict.  p_k = p_k + dt v_k (the old v); v_k = (v_k + du_k) - dt b_k.  P = F P F^T + Q entry by entry, with f_i = dt for
 *      i < 3, -dt for 3 <= i < 6 and no term for i >= 6 (likewise f_j): P'_ij = (P_ij + f_i P_i+3,j) + f_j (P_i,j+3 + f_i P_i+3,j+3),
 *      every P on the right the old one; then P'_ii += q^2 with q = q_p, q_v, q_b for the blocks p, v, b and nothing for c.
 *   3. Velocity update, when sigma_v > 0 and the step's record is solved with a finite v_uav: H = [0 I 0 0], z = v_uav,
 *      R = (sigma_v sigma_v) I.
 *   4. Displacement update, when the keyframe's flag is OFK_KEY_SOLVED at this step and D, C_T and R_world are finite:
 *      M = R_world C_T, W = M R_world^T (upper triangle, mirrored), C_ij = (infl infl) W_ij, + floor floor on the diagonal.  If fresh:
 *      P_cc += share C entry by entry, fresh = 0 - the key pixels' share of the noise is common to all steps of this keyframe, hence
 *      part of the uncertainty of where the key is, not white noise.  Then H = [I 0 0 -I], z = D, R = (1 - share) C.
 *   5. Fix update, when input slot 3 is set and the fix and its sigmas are finite and the sigmas > 0: H = [I 0 0 0], R = diag(sigma_k
 *      sigma_k).
 *   6. Every update, with a the block of +I and c the block of -I (none in rules 3 and 5, whose terms with c drop out):
 *      S_mn = (((P_am,an - P_am,cn) - P_cm,an) + P_cm,cn) + R_mn; y_m = z_m - (x_am - x_cm).  Cholesky of S's lower triangle: d0 =
 *      S_00, l00 = sqrt d0, l10 = S_10 / l00, l20 = S_20 / l00, d1 = S_11 - l10 l10, l11 = sqrt d1, l21 = (S_21 - l20 l10) / l11, d2
 *      = (S_22 - l20 l20) - l21 l21, l22 = sqrt d2.  A pivot d_m that is not finite or not > tiny_m = 2^-48 (((|P_am,am| + |P_am,cm|) +
 *      |P_cm,am|) + |P_cm,cm|), the rounding of the entries it was formed from (0 where they are 0): REFUSED, state untouched,
 *      counted (NIS 0).  With a prior on p of 1e6 and more the blocks pp, pc and cc are nearly equal numbers whose difference f64
 *      no longer holds; the floor keeps a displacement update from taking that noise for information until a fix has brought p
 *      down.  (The filter is a covariance filter in f64: a prior on v or b whose dt^2-fold exceeds about 1e15 times the variance
 *      of p it is added to erases that variance, and P_pp may come out of the first velocity update negative.  Keep p0_v and p0_b
 *      within 1e7 of p0_p, or start them together.)  w = L^-1 y forward (w2 = ((y2 - l20 w0) - l21 w1) / l22), NIS = (w0 w0 + w1 w1) + w2 w2; not finite: refused as well.
 *      nis_max > 0 and NIS > nis_max: GATED, state untouched, counted.  Otherwise (P H^T)_in = P_i,an - P_i,cn, (H P)_mj = P_am,j -
 *      P_cm,j; row i of K solves S k = (P H^T)_i: forward t as w, back k2 = t2 / l22, k1 = (t1 - l21 k2) / l11, k0 = ((t0 - l10 k1)
 *      - l20 k2) / l00.  x_i += (K_i0 y0 + K_i1 y1) + K_i2 y2.  Joseph form: B_ij = P_ij - ((K_i0 (HP)_0j + K_i1 (HP)_1j) + K_i2
 *      (HP)_2j); (B H^T)_in = B_i,an - B_i,cn; (K R)_in = (K_i0 R_0n + K_i1 R_1n) + K_i2 R_2n; P_ij = (B_ij - (three-term sum of
 *      (B H^T)_in K_jn)) + (three-term sum of (K R)_in K_jn); then P_ij = (P_ij + P_ji) / 2.  A block whose prior and process noise
 *      are both 0 (say p0_b = q_b = 0) stays exactly 0 through all of this: that is how a block is held.
 *   7. Clone, when the keyframe's record reports a re-key (field 9 != 0), whatever its flag: c = p; rows and columns 9-11 of P become
 *      rows and columns 0-2 (block cc becomes block pp); fresh = 1, clones + 1.  The keyframe's own anchor / pos are not used.
 *   8. steps + 1; the counts; the record, OFK_POSF_DOUBLES = 48: 0-11 x; 12-17 P_pp's upper triangle, 18-23 P_vv's, 24 the trace of
 *      P_bb; per update (velocity 25-29, displacement 30-34, fix 35-39) its outcome (OFK_POSF_NOT attempted, _APPLIED, _GATED,
 *      _REFUSED), NIS and innovation y; 40 cloned this step, 41 fresh, 42 steps, 43 clones, 44-46 updates applied / gated / refused
 *      over the three kinds, 47 rule 1 ran this step.  The input row is zeroed.
 * ofk_set_pos_filter: NULL or mode OFK_POSF_OFF switches it off.  OFK_E_INVALID, the setting staying as it was: an unknown mode, dt <=
 * 0, a negative sigma_v, floor, q or p0, infl <= 0, share outside [0, 1], nis_max < 0, anything not finite.  Defaults behind "off":
 * dt 1, sigma_v 1e-3, floor 0, infl 1, share 0.5, q_p 0, q_v 1e-3, q_b 0, p0_p 0, p0_v 1, p0_b 0 (the bias is held), nis_max 0 (no
 * gate).  OFK_E_INVALID before any launch from a stream step with the setting on and ofk_set_keyframe off; the keyframe's own
 * refusals then apply unchanged.  The state is allocated by the first step (or reset, or input) with need of it; ofk_stream_begin
 * resets it and clears the input rows.
 * ofk_pos_filter_input: input [batch of the active streams][OFK_POSF_INPUT], kept for the next step that is not held (a second call
 * replaces the rows).  ofk_pos_filter_reset: active stream b starts over at pos (NULL: zero) with its next step; its input row is
 * cleared.  ofk_pos_filter_download: x, P, istate, rec of the streams of the latest step with the setting on; any may be NULL.
 * ofk_pos_filter_step: rules 1-8 on host buffers, touching no resident state, through the same kernel: v_uav [batch][3], solved
 * [batch], key_rec [batch][OFK_KEY_DOUBLES], R_world [batch][9], input [batch][OFK_POSF_INPUT] (NULL: none; not modified); x, P,
 * istate in and out in place; rec out (may be NULL). */
#define OFK_POSF_OFF      0
#define OFK_POSF_ON       1
#define OFK_POSF_STATES   12
#define OFK_POSF_INPUT    12
#define OFK_POSF_INTS     16
#define OFK_POSF_DOUBLES  48
#define OFK_POSF_NOT      0
#define OFK_POSF_APPLIED  1
#define OFK_POSF_GATED    2
#define OFK_POSF_REFUSED  3
typedef struct ofk_pos_filter { int mode; double dt, sigma_v, floor, infl, share, q_p, q_v, q_b, p0_p, p0_v, p0_b, nis_max; } ofk_pos_filter;
int ofk_set_pos_filter(ofk_ctx *ctx, const ofk_pos_filter *f);
int ofk_get_pos_filter(const ofk_ctx *ctx, ofk_pos_filter *f);
int ofk_pos_filter_input(ofk_ctx *ctx, const double *input);
int ofk_pos_filter_reset(ofk_ctx *ctx, int b, const double *pos);
int ofk_pos_filter_download(ofk_ctx *ctx, double *x, double *P, int *istate, double *rec);
int ofk_pos_filter_step(ofk_ctx *ctx, const ofk_pos_filter *f, const double *v_uav, const int *solved, const double *key_rec,
                        const double *R_world, const double *input, double *x, double *P, int *istate, int batch, double *rec);

/* Stabilised view per stream: every step's new gray frame resampled into the view of the stream's keyframe.  A stream with
 * ofk_set_keyframe on knows the rigid motion P_c = R P_K + T that ties the current frame to the keyframe, and the ground plane (n, d) of
 * the sensor row; for ground on that plane the motion is one homography per frame, K (I + T n' / (d - n.T)) R K^-1 (what
 * synth.pixel_homography(motion = "finite") renders with).  With this setting on every stream step leaves on the device the step's new
 * gray frame warped through it (k_warp_u8, ofk_warp_perspective's rule) into a view that stays that of the FIRST keyframe across
 * re-keys.  Off by default; with it off every step allocates, launches and returns what it always did.  Nothing is fed back: records,
 * `fused`, tracks, the table, depths, templates, the keyframe's state and record and the position filter keep their bits.  Streams only:
 * ofk_pairs_run ignores the setting.
 * State per stream: Bv [9] f64, row-major 3 x 3, view -> keyframe in normalised coordinates; ints [OFK_STAB_INTS] = steps since the
 * last re-base, re-bases, approx, 1 where a previous warp's covered count exists; covered, one i32, of the latest warp; a record of
 * OFK_STAB_DOUBLES.  Bv = I, the ints zero: by the first step with the setting on behind ofk_stream_begin (or switched on in
 * mid-stream) and by ofk_stab_reset; Bv = I alone where the replace re-detection resets the keyframe (the streams with a budget).
 * Two launches, k_stab_pose (one thread per stream) and k_warp_u8, on exactly the steps that launch the keyframe's kernel, behind it and
 * behind the position filter's; a held step leaves state, record, count and frame alone.  All arithmetic f64 without contraction in the
 * order written; sums of three are (a + b) + c; 3 x 3 products are (A_i0 B_0j + A_i1 B_1j) + A_i2 B_2j.  In order:
 *   1. Inputs.  R and T are the ones the keyframe's rule 2 used at this step, in front of its rule 5.  With ofk_set_keyframe_rotation on
 *      (and not every axis held by the setting alone) R = slots 4-12 of the rotation record.  Otherwise the keyframe's state is copied
 *      device to device in front of the keyframe's launch and R is its rule 1's product of that copy's R_acc and the omega the keyframe
 *      read, by the same device code.  T = slots 0-2 of the keyframe's record, kflag = its slot 3, rekey = its slot 9 != 0.
 *      n = sn[1..3] (under use_imu the IMU state's normal), d = sn[0], as the keyframe read them.
 *   2. Normalised homography G, key -> current.  den = d - ((n0 T0 + n1 T1) + n2 T2).  kflag OFK_KEY_NONE (no keyframe): flag
 *      OFK_STAB_NONE, G = I.  Otherwise flag OFK_STAB_FULL when the mode is OFK_STAB_PLANE, kflag is OFK_KEY_SOLVED, |den| >= 1e-12 and
 *      R, T, n and den are finite: C_ij = (i == j ? 1 : 0) + (T_i n_j) / den, G = C R.  Otherwise (mode OFK_STAB_ROTATION, an unsolved
 *      key step, a plane through the camera, something that is no number) flag OFK_STAB_ROTATION_ONLY, G = R.
 *   3. View.  A = G B, B = Bv (I on a re-base, rule 4).  K = [[f, 0, cx], [0, f, cy], [0, 0, 1]], f = 1.0 / scaling, (scaling, cx, cy) =
 *      sn[19..21]: P = K A with P_0j = f A_0j + cx A_2j, P_1j = f A_1j + cy A_2j, P_2j = A_2j; M = P K^-1 with M_i0 = P_i0 scaling,
 *      M_i1 = P_i1 scaling, M_i2 = P_i2 - (P_i0 (cx scaling) + P_i1 (cy scaling)).  M maps a pixel of the view to a pixel of the new
 *      frame: the warp's destination -> source matrix.  Behind the warp: rekey and chain = 1: Bv = A (the view stays the first
 *      keyframe's); rekey and chain = 0: Bv = I (the view jumps to the new keyframe); no rekey: Bv = B.  A rekey under a flag other than
 *      OFK_STAB_FULL raises the approx count: the view has lost that step's translation.
 *   4. Re-base, decided in front of rule 3.  OFK_STAB_RB_COVER: min_cover > 0, a previous warp of the stream exists and its covered
 *      count, in f64, is below min_cover (h w).  OFK_STAB_RB_FINITE: no re-base by cover and an entry of M that is not finite; A and M
 *      are formed again with B = I.  A re-base sets the steps since the last one to zero and raises the re-base count; any other step
 *      raises the steps.  The view is then the current keyframe's.
 *   5. Warp.  k_warp_u8 over level 0 of the step's new frame (the bytes ofk_resident_pyramid returns for it behind the step, JPEG steps
 *      included), one channel, h x w -> h x w, the setting's border and border_value, into a resident [B][h][w] u8 buffer, 256-B
 *      aligned per image, allocated by the first step with the setting on; covered as ofk_warp_perspective counts it.
 * Record: 0-8 M, 9-17 Bv behind the step, 18-26 R, 27-29 T, 30 flag, 31 re-base reason (0: none), 32 steps since the last re-base,
 * 33 re-bases, 34 approx, 35 1 on a rekey, 36 the previous warp's covered count as rule 4 read it (-1: none), 37-47 0.
 * ofk_set_stabilise: NULL or mode OFK_STAB_OFF switches it off.  OFK_E_INVALID, the setting staying as it was: an unknown mode or border,
 * border_value outside 0..255, min_cover outside [0, 1) or not finite (0: no re-base by cover), chain neither 0 nor 1.  Defaults
 * behind "off": OFK_STAB_PLANE, OFK_BORDER_CONSTANT, 0, 0.5, 1.
 * OFK_E_INVALID before any launch from a stream step with the setting on: ofk_set_keyframe off; ofk_set_camera or
 * ofk_set_rolling_shutter on (the homography holds between ideal global-shutter images; a raw frame behind a lens needs a remap in
 * front of the warp, which is not built).  With ofk_set_rectify on the camera is accepted (below); the rolling shutter never is.
 * ofk_stab_download, the streams of the latest step with the setting on (every output may be NULL): frames [batch][h][w] u8, rec
 * [batch][OFK_STAB_DOUBLES], covered [batch] i32.  ofk_stab_frames: the DEVICE pointer of the frames and the bytes between images, for
 * consumers on the device (valid until the context is destroyed; written by every step).  ofk_stab_reset: active stream b starts over
 * (Bv = I, the ints and the record zero but for M = Bv = I).
 * ofk_stab_pose, rules 1-4 on host buffers (it touches no resident state): R [batch][9] the rotation used, key_rec
 * [batch][OFK_KEY_DOUBLES], sensors [batch][OFK_SENSOR_DOUBLES], normal [batch][3] (NULL: the sensor rows'), prev_covered [batch] (NULL:
 * zeros; read where ints[b][3] != 0), h, w the frame, Bv [batch][9] and ints [batch][OFK_STAB_INTS] in and out in place, rec
 * [batch][OFK_STAB_DOUBLES] out (may be NULL). */
#define OFK_STAB_OFF            0
#define OFK_STAB_ROTATION       1
#define OFK_STAB_PLANE          2
#define OFK_STAB_DOUBLES        48
#define OFK_STAB_INTS           4
#define OFK_STAB_NONE           0
#define OFK_STAB_ROTATION_ONLY  1
#define OFK_STAB_FULL           2
#define OFK_STAB_RB_COVER       1
#define OFK_STAB_RB_FINITE      2
typedef struct ofk_stabilise { int mode; int border; int border_value; double min_cover; int chain; } ofk_stabilise;
int ofk_set_stabilise(ofk_ctx *ctx, const ofk_stabilise *s);
int ofk_get_stabilise(const ofk_ctx *ctx, ofk_stabilise *s);
int ofk_stab_download(ofk_ctx *ctx, uint8_t *frames, double *rec, int *covered);
int ofk_stab_frames(ofk_ctx *ctx, uint8_t **device_ptr, size_t *image_stride);
int ofk_stab_reset(ofk_ctx *ctx, int b);
int ofk_stab_pose(ofk_ctx *ctx, const ofk_stabilise *s, const double *R, const double *key_rec, const double *sensors, const double *normal,
                  const int *prev_covered, int h, int w, double *Bv, int *ints, int batch, double *rec);

/* Camera model: the lens distortion undone on the device before the solve.  The solve stage reads a point as a sample of an ideal
 * pinhole image, x = (px - cx) * scaling (sensors[19..21]); the reference's camera is a wide-angle module whose lens moves a point by
 * tens of pixels at the border.  With ofk_set_camera on, the resident chains keep everything that lives in the image on the raw
 * pixels (LK, the track gates, the tracks, the disc mask, the zones, the corner grid, every download of points) and hand the solve
 * stage (plain, robust and covariance kernels, the fused stream kernels and the feasibility rule inside them) the IDEAL pixels of the
 * same points.  Off by default; with it off every chain launches the kernels and returns the bits it always did.
 * k in cv2's order.  OFK_CAMERA_BROWN: k1 k2 p1 p2 k3 k4 k5 k6 (cv2's pinhole model; the rational terms k4..k6 may be 0).
 * OFK_CAMERA_FISHEYE: cv2.fisheye's equidistant model, k1..k4 in k[0..3]; k[4..7] must be 0.
 * Per point, float64, in the order written, no contraction, ONE rounding to float32 at the end:
 *   Undistort (image pixel p -> ideal pixel): x0 = (px - cx) / fx, y0 = (py - cy) / fy.
 *     Brown: x = x0, y = y0, then `iters` times
 *       r2 = x*x + y*y
 *       icd = (1 + ((k6 r2 + k5) r2 + k4) r2) / (1 + ((k3 r2 + k2) r2 + k1) r2)
 *       dx = 2 p1 x y + p2 (r2 + 2 x x)          [((2 p1) x) y, 2 x x = (2 x) x]
 *       dy = p1 (r2 + 2 y y) + 2 p2 x y
 *       x = (x0 - dx) icd, y = (y0 - dy) icd
 *     Fisheye: td = sqrt(x0*x0 + y0*y0), t = td, then `iters` Newton steps
 *       t2 = t*t, t4 = t2*t2, t6 = t4*t2, t8 = t4*t4
 *       t = t - (t (1 + k1 t2 + k2 t4 + k3 t6 + k4 t8) - td) / (1 + 3 k1 t2 + 5 k2 t4 + 7 k3 t6 + 9 k4 t8)     [sums left to right]
 *       s = tan(t) / td, s = 1 where td < 1e-8; x = x0 s, y = y0 s
 *     out = ((float)(x fo_x + co_x), (float)(y fo_y + co_y)).
 *   Distort (ideal pixel q -> image pixel), the closed-form forward map: x = (qx - co_x) / fo_x, y likewise.
 *     Brown: r2 = x*x + y*y, cd = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2), dx, dy as above,
 *       xd = x cd + dx, yd = y cd + dy.
 *     Fisheye: r = sqrt(x*x + y*y), t = atan(r), td = t (1 + k1 t2 + k2 t4 + k3 t6 + k4 t8), s = td / r, s = 1 where r < 1e-8,
 *       xd = x s, yd = y s.
 *     out = ((float)(xd fx + cx), (float)(yd fy + cy)).
 *   Fallback: a point one of whose two results is not finite or exceeds 1e6 in magnitude takes, for both coordinates, the linear map
 *     of the input with no lens term ((float)(x0 fo_x + co_x) / (float)(x fx + cx)) - k_seed_points' rule for a seed LK could not use.
 *     Its status is not touched.
 * `iters` is a FIXED count (deterministic, no data-dependent exit).  cv2.undistortPoints' default of 5 leaves up to 0.47 px of
 * round-trip error at the corners of a strong wide-angle lens (k1 = -0.28): 8 -> 0.018, 10 -> 0.0021, 15 -> 1e-5 px; the fisheye's
 * Newton iteration is at 5e-13 px after 3.
 * Refused with OFK_E_INVALID before any launch, a setting staying as it was: model none of the three, iters outside 1..50, a field
 * that is not finite, fx, fy, fo_x or fo_y zero, k[4..7] != 0 for the fisheye.  ofk_set_camera also refuses fo_x != fo_y: the solve
 * has ONE scaling, and the caller keeps sensors[19..21] = 1 / fo_x, co_x, co_y.  NULL or model OFK_CAMERA_OFF switches it off.
 * Resident chains (ofk_pairs_run with every slice count and overlap on and off, ofk_stream_step[_jpeg], ofk_stream_step_fused[_jpeg]):
 * behind the track step (forward LK, backward pass and gates) ONE k_camera_undistort launch per call and slice writes the ideal points
 * of pts_prev and pts_next.  With ofk_set_lk_seed on: undistort pts_prev, k_seed_points on the ideal points as it is, k_camera_distort
 * in place on the seeds, LK, undistort pts_next - three camera launches.
 * ofk_undistort_points / ofk_distort_points, the stage entries on host buffers (pts, out [batch][stride][2] f32, counts [batch]):
 * entries of `out` beyond counts[b] keep what the caller put there; they accept fo_x != fo_y; a camera with model OFK_CAMERA_OFF is
 * refused.  They touch no resident state.
 * ofk_camera_download: the ideal points the solve stage of the latest run / step with the setting on saw, [batch][stride][2] f32 each
 * (either may be NULL; at most the context's max_pts points per row are written); OFK_E_INVALID before such a run. */
#define OFK_CAMERA_OFF 0
#define OFK_CAMERA_BROWN 1
#define OFK_CAMERA_FISHEYE 2
typedef struct ofk_camera {
    int model; int iters;
    double fx; double fy; double cx; double cy;
    double k[8];
    double fo_x; double fo_y; double co_x; double co_y;
} ofk_camera;
int ofk_set_camera(ofk_ctx *ctx, const ofk_camera *cam);
int ofk_get_camera(const ofk_ctx *ctx, ofk_camera *cam);
int ofk_undistort_points(ofk_ctx *ctx, const ofk_camera *cam, const float *pts, const int *counts, int batch, int stride, float *out);
int ofk_distort_points(ofk_ctx *ctx, const ofk_camera *cam, const float *pts, const int *counts, int batch, int stride, float *out);
int ofk_camera_download(ofk_ctx *ctx, float *prev_ideal, float *next_ideal, int stride);

/* Rectified view: the stabilised view of a stream behind a lens.  The view and the matrix M of ofk_set_stabilise live in IDEAL pixels
 * (with a camera set the caller keeps sensors[19..21] = 1 / fo, co_x, co_y), the step's new frame in raw ones.  With this setting on AND
 * ofk_set_camera on, a stream step with ofk_set_stabilise on is accepted and its rule 5 launches k_warp_lens_u8 (ofk_warp_lens's rule)
 * with the context's camera and this r_max in the place of k_warp_u8: the same M (the view's pose does not change), level 0 of the new
 * frame (JPEG steps included), the same buffer, border, border_value, covered count and min_cover re-base.  Without a camera the
 * setting is inert and the plain warp runs; without the stabilised view it launches nothing; with it off (the default) every step
 * does what it always did, the refusal of the view beside ofk_set_camera included.  The view beside ofk_set_rolling_shutter stays
 * refused either way.  ofk_pairs_run ignores the setting.
 * ofk_set_rectify: NULL or mode OFK_RECTIFY_OFF switches it off.  OFK_E_INVALID, the setting staying as it was: a mode other than the
 * two, r_max negative or not finite (0: no bound).  Defaults behind "off": r_max 0. */
#define OFK_RECTIFY_OFF 0
#define OFK_RECTIFY_ON  1
typedef struct ofk_rectify { int mode; double r_max; } ofk_rectify;
int ofk_set_rectify(ofk_ctx *ctx, const ofk_rectify *r);
int ofk_get_rectify(const ofk_ctx *ctx, ofk_rectify *r);

/* Rolling shutter: the per-row capture time undone on the device before the solve.  The reference's camera exposes its rows one after
 * the other: a point in row y of a frame of H rows is seen readout * (y / H - anchor) frame intervals away from the frame's time
 * stamp, so the measured flow of a point that changes row spans 1 + readout * dy / H frame intervals, and neither end sits where the
 * sensor record (omega, d, n at the time stamp) says the camera was.  With ofk_set_rolling_shutter on, the resident chains hand the
 * solve stage (plain, robust and covariance kernels, the fused stream kernels and the feasibility rule inside them) the positions a
 * global shutter would have seen at the two time stamps; everything that lives in the image (LK and its seeds, the track gates, the
 * tracks, the disc mask, the zones, the corner grid, every download of points) keeps the raw pixels.  Off by default; with it off
 * every chain launches the kernels and returns the bits it always did.
 *   readout: the time from the first to the last row in frame intervals; negative = read from the bottom row up.
 *   rows:    H, the RAW frame's row count; 0 = the frame height of the run (resident chains only; the stage entry needs rows > 0).
 *   anchor:  the row fraction in [0, 1] whose exposure the frame's time stamp, and so the sensor record, belongs to.
 *   omega_gain: turns the sensors' omega into radians per frame interval, as `gain` does for ofk_set_lk_seed.
 * Per point i < counts[b], float64, in the order written, no contraction, ONE rounding to float32 at the end.  The rows are the raw
 * image's (r0, r1 = the point in the previous / next frame); positions and flow are the ideal ones (q0, q1 = the camera's ideal pixels
 * of r0, r1, or r0, r1 themselves with no camera):
 *   t0 = readout * (r0.y / H - anchor), t1 = readout * (r1.y / H - anchor), span = 1 + (t1 - t0)
 *   OFK_RS_FLOW (constant image velocity; needs no sensor):
 *     f = (q1 - q0) / span;  out_prev = (float)(q0 - t0 f), out_next = (float)(q1 - t1 f)
 *   OFK_RS_GYRO (the rotation over the row time from omega, exactly; the rest of the flow held constant): scaling, cx, cy =
 *   sensors[19..21]; om = omega_gain * omega, omega = sensors[4..6] or, under ofk_fusion.use_imu, the resident IMU state's (what
 *   k_seed_points takes):
 *     x0 = (q0 - c) * scaling, x1 = (q1 - c) * scaling                                           [per coordinate]
 *     rot(x, y, t), the point (x, y) as the rotation alone had it t frame intervals earlier:
 *       p = (-t) om;  th2 = p0 p0 + p1 p1 + p2 p2
 *       A = sin(th) / th, B = (1 - cos(th)) / th2 with th = sqrt(th2);  A = 1, B = 0.5 where th2 < 1e-16
 *       c = p x (x, y, 1):  c0 = p1 - p2 y, c1 = p2 x - p0, c2 = p0 y - p1 x
 *       d = p x c:          d0 = p1 c2 - p2 c1, d1 = p2 c0 - p0 c2, d2 = p0 c1 - p1 c0
 *       X = x + A c0 + B d0, Y = y + A c1 + B d1, Z = 1 + A c2 + B d2                            [Rodrigues; sums left to right]
 *       rot = (X / Z, Y / Z)
 *     hs = span / 2;  r = rot(x0, -hs), m = rot(x1, hs): both observations carried to the middle of the span by the rotation alone
 *     ft = ((m.x - r.x) / span, (m.y - r.y) / span): the rest of the flow, held constant
 *     for each end k: e = rot(xk, tk)
 *       out = ((float)((e.x - tk ft.x) / scaling + cx), (float)((e.y - tk ft.y) / scaling + cy))
 *     The rest of the flow is taken against the EXACT rotation, symmetrically about the middle of the span, not against the seed
 *     formula's rotational part at the mid point ((x1 - x0) / span - frot((x0 + x1) / 2)): that is a mid-point rule, whose error of
 *     the third order in omega leaves a point under pure rotation 0.1 px from its place at a yaw of 0.15 rad per frame.  With the
 *     exact rotation such a point comes back to 1e-12, and on combined motions the two forms agree (tests/rs_reference.py).
 *     The sign is the project's: the seed's field is dP/dt = omega x P.
 *   Fallback: a point whose span is not finite or < 0.5, or one of whose four results is not finite or exceeds 1e6 in magnitude, or
 *     (GYRO) whose scaling is 0, takes q0 and q1 unchanged; its status is not touched - k_seed_points' and the camera's rule.  Points
 *     with status 0 carry garbage in `next` and come out finite or as they went in.
 * What the model assumes: the image velocity of a point is constant between its two exposures (FLOW: all of it; GYRO: what is left
 * of it once the rotation is taken out), and omega is constant over a frame.  The covariance (ofk_set_cov) takes the corrected
 * points as its inputs and does not propagate an error of readout.  Out of scope: exposure blur, per-row IMU samples, a readout
 * estimated from data, vibration within a frame.  A seeded LK predicts its seeds exactly as with the setting off: a seed is a start
 * position, and the row time's effect on it is of second order.
 * Refused with OFK_E_INVALID before any launch, a setting staying as it was: mode none of the three, a field that is not finite,
 * |readout| > 1, anchor outside [0, 1], rows < 0 or > 65536, omega_gain == 0; in the stage entry also rows == 0 and OFK_RS_GYRO with
 * sensors == NULL.  NULL or mode OFK_RS_OFF switches the setting off.
 * Resident chains (ofk_pairs_run with every slice count and overlap on and off, ofk_stream_step[_jpeg], ofk_stream_step_fused[_jpeg],
 * append and replace mode): behind the track step, and behind k_camera_undistort when a camera is set, ONE k_rs_correct launch per
 * call and slice writes the corrected ideal points of both sets into the buffers the solve stage reads.
 * ofk_rs_correct_points, the stage entry on host buffers (points [batch][stride][2] f32, counts [batch], sensors [batch][28] f64,
 * NULL allowed for FLOW): ideal_prev and ideal_next both NULL = the raw points; entries of out_prev / out_next beyond counts[b] keep
 * what the caller put there.  It touches no resident state.
 * ofk_rs_download: the points the solve stage of the latest run / step with the setting on saw, [batch][stride][2] f32 each (either
 * may be NULL; at most the context's max_pts points per row are written); OFK_E_INVALID before such a run.  With ofk_set_camera on as
 * well, ofk_camera_download returns the same arrays: both are "what the solve stage saw". */
#define OFK_RS_OFF 0
#define OFK_RS_FLOW 1    /* constant image velocity from the measured flow; needs no sensor */
#define OFK_RS_GYRO 2    /* rotation over the row time from omega (exact), the rest of the flow held constant */
typedef struct ofk_rshutter { int mode; int rows; double readout; double anchor; double omega_gain; } ofk_rshutter;
int ofk_set_rolling_shutter(ofk_ctx *ctx, const ofk_rshutter *rs);
int ofk_get_rolling_shutter(const ofk_ctx *ctx, ofk_rshutter *rs);
int ofk_rs_correct_points(ofk_ctx *ctx, const ofk_rshutter *rs, const float *raw_prev, const float *raw_next, const float *ideal_prev,
                          const float *ideal_next, const int *counts, int batch, int stride, const double *sensors, float *out_prev,
                          float *out_next);
int ofk_rs_download(ofk_ctx *ctx, float *prev, float *next, int stride);

/* Finite motion: exact rotation and plane displacement before the solve.  Every solve builds the instantaneous motion field
 * u = (n.p)/d (v - v_z p) + (omega x p - (omega x p)_z p); a frame pair is a finite motion P1 = R P0 + T, R = exp([omega]x), and the
 * difference is the largest model error left: 0.3 % of the velocity at a flow of 5 px (at a focal length of 800 px), 3 % at 39 px,
 * 10 % at 128 px, 18 % at 149 px, and a false velocity of 0.011 per frame under a pure rotation of 0.15 rad (tests/finite_reference.py).
 * For points on the plane n.P1 = d (n, d in the NEXT frame's camera axes, which is what the sensor record carries and where the solves
 * evaluate n.p):  R P0 = (I - T n^T / d) P1.  With q~ the previous point rotated by R and renormalised, and p1 the next point,
 *   (n.p1)/d [q~]x T = [q~]x (p1 - q~),
 * the NODE system with [.]x taken from q~.  The solves build their system from ONE position x^ and ONE flow u^ and subtract the
 * first-order rotational field of omega at x^ themselves, so with ofk_set_finite_motion on, the resident chains hand the solve stage
 *   x^ = q~,   u^ = s (p1 - q~) + rotfield(q~, omega),   s = (n.q~)/(n.p1),   rotfield(p, w) = w x p - (w x p)_z p,
 * for which the first-order system IS the finite relation ([q~]x q~ = 0 absorbs the third component; d does not enter the rewrite).
 * The solve then returns T, the displacement per frame interval in the next frame's camera axes; it equals v to first order.
 * WHAT THE RECORD MEANS WITH THE SETTING ON: fields 0-2 are T, and v_uav = R_world (T - omega x offset), fields 8-10, is the MEAN
 * world-frame velocity over the frame interval, not the instantaneous one at the next frame.
 * Everything that lives in the image (LK and its seeds, the track gates, the tracks, the masks, the zones, the corner grid, every
 * download of points) keeps the raw pixels.  Off by default; with it off every chain launches the kernels and returns the bits it
 * always did.
 * Per point i < counts[b], float64, in the order written, no contraction, ONE rounding to float32 at the end.  q0, q1 = the points the
 * solve would otherwise have read (raw, the camera's ideal ones, or the rolling shutter's corrected ones):
 *   sc, cx, cy = sensors[19..21];  n = sensors[1..3], om = sensors[4..6] or, under ofk_fusion.use_imu, the resident IMU state's
 *   [15..17], [18..20] (what k_stream_fuse takes); om is exactly the vector the solve subtracts: no gain
 *   x0 = (q0.x - cx) sc, y0 = (q0.y - cy) sc;  x1, y1 likewise from q1
 *   (X, Y, Z) = the rotation of (x0, y0, 1) by +om: the rolling shutter's rot() above with t = -1, before its projection
 *   a = X / Z, b = Y / Z
 *   den = n0 x1 + n1 y1 + n2;  s = (n0 a + n1 b + n2) / den
 *   c0 = om1 - om2 b, c1 = om2 a - om0, c2 = om0 b - om1 a
 *   ux = s (x1 - a) + (c0 - c2 a),  uy = s (y1 - b) + (c1 - c2 b)
 *   out_next = ((float)(a / sc + cx), (float)(b / sc + cy))
 *   out_prev = ((float)((a - ux) / sc + cx), (float)((b - uy) / sc + cy))
 *   Fallback: a point with sc == 0, !(Z >= min_depth), !(|den| >= 1e-12), !(s > 0), or one of whose four results is not finite or
 *   exceeds 1e6 in magnitude keeps q0 and q1 as they came; its status is not touched - the camera's and the rolling shutter's rule.
 * The rewrite takes omega and n as the record gives them: with ofk_set_joint or ofk_set_plane on, which refine one of them, an error
 * of second order (correction x flow) remains.  The covariance takes the rewritten points as its inputs.
 * Out of scope: a plane given at the previous frame (non-linear in T), exact seeds for LK, the rewrite's own Jacobian in the
 * covariance, re-running the rewrite at the joint solve's omega or the plane solve's normal, a body-constant velocity V(omega)^-1 T.
 * Refused with OFK_E_INVALID before any launch, a setting staying as it was: an unknown mode, min_depth not finite or outside (0, 1];
 * in the stage entry sensors == NULL; in the runs and steps with the setting on OFK_SOLVE_OFMODULE, OFK_FLOW_ROTATIONAL and
 * OFK_KEEP_LEGACY, which are not the sensor model.  NULL or mode OFK_FM_OFF switches the setting off.
 * Resident chains (ofk_pairs_run with every slice count and overlap on and off, ofk_stream_step[_jpeg], ofk_stream_step_fused[_jpeg],
 * append and replace mode): behind the track step, k_camera_undistort and k_rs_correct, ONE k_finite_correct launch per call and
 * slice rewrites both sets in the buffers the solve stage reads (in place, or from the raw points when neither of the two is on).
 * ofk_finite_correct_points, the stage entry on host buffers (points [batch][stride][2] f32, counts [batch], sensors [batch][28] f64):
 * entries of out_prev / out_next beyond counts[b] keep what the caller put there.  It touches no resident state.
 * ofk_finite_download: the points the solve stage of the latest run / step with the setting on saw, [batch][stride][2] f32 each
 * (either may be NULL; at most the context's max_pts points per row are written); OFK_E_INVALID before such a run.  With
 * ofk_set_camera or ofk_set_rolling_shutter on as well, their downloads return the same arrays: all are "what the solve stage saw". */
#define OFK_FM_OFF 0
#define OFK_FM_EXACT 1
typedef struct ofk_finite_motion { int mode; double min_depth; } ofk_finite_motion;
int ofk_set_finite_motion(ofk_ctx *ctx, const ofk_finite_motion *fm);   /* NULL or OFF: off */
int ofk_get_finite_motion(const ofk_ctx *ctx, ofk_finite_motion *fm);
int ofk_finite_correct_points(ofk_ctx *ctx, const ofk_finite_motion *fm, const float *prev, const float *next, const int *counts,
                              int batch, int stride, const double *sensors, float *out_prev, float *out_next);
int ofk_finite_download(ofk_ctx *ctx, float *prev, float *next, int stride);

/* ------------------------------------------------- estimation (float64, batched over `batch` independent problems) */

/* generate_test_data(x, v, omega, d, n[, t]) — node:25-29; simulation.py:7-12.
 * x [batch][n][2]; v, omega, nrm, t [batch][3] (t nullable = no lever arm); d [batch]; flow [batch][n][2]. */
int ofk_flow_model(ofk_ctx *ctx, const double *x, int batch, int n, const double *v, const double *omega, const double *d,
                   const double *nrm, const double *t, double *flow);

#define OFK_FEAS_RTILDE  0   /* of.r_tilde(x,u,n,v,dist)            of_library.py:365-386 (node:238) */
#define OFK_FEAS_LEGACY  1   /* 4-arg r_tilde, no guard, no /dist    sensor_precision_experiments/pixhawk_pure_IMU/of_library.py:365-380 (of_module.py:125) */
#define OFK_FEAS_SIM     2   /* feasibility(pos,v,flow,omega,t,n)    simulation.py:108-120 */
/* x,u [batch][n][2]; nrm,v [batch][3]; dist [batch] (RTILDE only); omega,t [batch][3] (SIM only, else nullable);
 * r,dd [batch][n]. */
int ofk_feasibility(ofk_ctx *ctx, int variant, const double *x, const double *u, int batch, int n, const double *nrm,
                    const double *v, const double *dist, const double *omega, const double *t, double *r, double *dd);

#define OFK_SOLVE_NODE      0   /* node:30-42 / evaluate_exp.py:18-31: A_i=[p]x,        b_i=[p]x(u+[p]x w)/(n.p) */
#define OFK_SOLVE_SIM       1   /* simulation.py:15-30:               A_i=[p]x (n.p),  b_i=[p]x(u+[p]x w)        */
#define OFK_SOLVE_OFMODULE  2   /* of_module.py:139-146:              A_i=[p]x/w_i,    b_i=A_i u_i/(n.p), no omega, no d */
#define OFK_SOLVE_DOUBLES   8   /* out per problem: v[3], residual SS, rank, s[3] (singular values, descending) */
/* x,u [batch][n][2]; valid (nullable) [batch][n] u8, 0 = skip the point; d [batch]; nrm, omega [batch][3];
 * t (nullable) [batch][3]: subtract omega x t from v (simulation.py:28, evaluate_exp.py:29);
 * wgt (OFMODULE only) [batch][n] per-point distance.  Fewer than 1 valid point -> rank 0, v = 0.
 * Non-finite sums.  Every solve of the library (this entry, the robust and covariance entries, the pair and stream kernels) forms
 * the 3 x 3 normal equations M v = g.  A problem whose sums - M, g, and the eigenvalues of M - are not all finite (a NaN or inf
 * range, gyro or point; a valid point with n.p == 0 in the NODE system) is not solved: rank 0, v = 0 (no omega x t taken off),
 * s = 0, residual 0, the point count as counted.  It counts as not solved everywhere: record[15] = 0 and fused[7] = 0, the filters
 * stay at their prediction (record[4] != 3), vel_overwrite does not fire, the covariance record is void, the robust stats carry
 * flag 1 with all kept weights 1.  Problems whose sums are finite are not touched by this, bit for bit.
 * Accuracy.  v comes from the normal equations, so a rank-3 result is accurate to about C kappa^2 eps relative, kappa = s[0] / s[2]
 * (record fields 5 and 7), C a few tens ("rank"); the rank cut only fires at kappa = 1 / sqrt(eps 3N).  A
 * consumer that needs a given accuracy gates on kappa, not on rank 3. */
int ofk_velocity_solve(ofk_ctx *ctx, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                       const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                       double *out);

/* The robust velocity solve: a sampled least-median-of-squares start, then iteratively reweighted least squares.  Off by default;
 * with it off every entry point launches the kernels and returns the bits it always did.
 * For one problem let the kept points be those that enter the plain solve (status / valid / feasibility / legacy keep), m of them,
 * numbered 0..m-1 in point-index order, with the plain solve's per-point terms q, sA, sB.  r_i(v) = sA [p]x v - sB [p]x q,
 * rho_i = |r_i|.  A weighted solve multiplies point i's contributions to the 3x3 normal equations by w_i, counts the points with
 * w_i > 0 as its rows and is otherwise the plain solve (rank rule included).  sel(a) = the element of index m / 2 of a sorted
 * ascending: an exact selection, never an interpolation.
 *   1. m < OFK_ROBUST_MIN_POINTS (or the plain solve's own point guard fails): the plain result, all kept weights 1, flag 1.
 *   2. Start: v = the plain solve, hyp = -1.  For h = 0..hypotheses-1: (x0, x1, ., .) = Philox4x32-10(counter (h, b, 0, 0),
 *      key (seed & 0xffffffff, seed >> 32)), b = the problem's index in the call's whole batch; i = x0 mod m, j = x1 mod (m - 1),
 *      j += (j >= i); v_h = the weighted solve with weight 1 on kept points i and j only (rank < 3: void);
 *      score_h = sel(rho^2(v_h)) over all kept points.  The start is the non-void hypothesis of smallest score (ties: smaller h).
 *   3. Exactly `iters` times: s = 1.4826 sel(rho(v)); if !(s^2 > 1e-24 bb / m), bb = sum sB^2 |[p]x q|^2: the data fit exactly,
 *      flag 2, stop with v and the previous weights.  t_i = rho_i / (c s); HUBER w_i = t_i <= 1 ? 1 : 1 / t_i;
 *      TUKEY w_i = t_i < 1 ? (1 - t_i^2)^2 : 0.  v' = the weighted solve; rank < 3: flag 3, keep v and the previous weights, stop.
 *   4. Record / out fields: 0-2 v; 3 sum w_i rho_i^2(v); 4 rank and 5-7 singular values of the system of the final weights;
 *      8-10 v_uav from the robust v; 11 points with w_i > 0; 12-15 as always.  weights: w_i per point, 0 for points not kept.
 *      stats, OFK_ROBUST_DOUBLES per problem: s of the last round, sum w, count w > 0, m, hyp, score (0 without a hypothesis),
 *      rounds completed, flag.
 * ofk_set_robust (NULL or loss OFK_ROBUST_OFF: off, the default) is a context setting read by ofk_pairs_run (every slice),
 * ofk_stream_step[_jpeg] and ofk_stream_step_fused[_jpeg]; in the fused step the filter's correct takes the robust v / v_uav.  With
 * drop = 1 the stream steps clear the keep flag of every point whose final weight is 0 before the tracks are updated, so such points
 * leave the tracks as infeasible ones do.  Invalid settings (unknown loss, c not finite or <= 0, iters outside 0..32, hypotheses
 * outside 0..256, drop not 0/1) return OFK_E_INVALID and leave the previous setting in place.  Records are bit-identical across
 * launch forms (one wave per pair from 128 pairs per slice on, a 256-thread workgroup below), slice counts and overlap settings.
 * ofk_robust_download: weights [batch][stride] (the first min(stride, max_pts) of every row are written) and stats
 * [batch][OFK_ROBUST_DOUBLES] of the latest run / step with the setting on; either may be NULL; OFK_E_INVALID before such a run.
 * ofk_velocity_solve_robust = ofk_velocity_solve's arguments (n <= 4096) plus the setting; weights [batch][n], stats nullable.
 * ofk_robust_pairs (host only; no context, no GPU): the sample of step 2 for h = 0..hypotheses-1; m >= 2. */
#define OFK_ROBUST_OFF 0
#define OFK_ROBUST_HUBER 1
#define OFK_ROBUST_TUKEY 2
#define OFK_ROBUST_MIN_POINTS 8
#define OFK_ROBUST_DOUBLES 8
typedef struct ofk_robust { int loss; double c; int iters; int hypotheses; unsigned long long seed; int drop; } ofk_robust;
int ofk_set_robust(ofk_ctx *ctx, const ofk_robust *r);
int ofk_get_robust(const ofk_ctx *ctx, ofk_robust *r);
int ofk_robust_download(ofk_ctx *ctx, double *weights, int stride, double *stats);
int ofk_velocity_solve_robust(ofk_ctx *ctx, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                              const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                              const ofk_robust *r, double *out, double *weights, double *stats);
int ofk_robust_pairs(unsigned long long seed, unsigned problem, int hypotheses, int m, int *i, int *j);

/* Track gates: the forward-backward check of KLT trackers and a cap on LK's err, applied on the device behind LK and in front of
 * everything that keys on status == 1.  Both are off by default; with them off every entry point launches the kernels and returns
 * the bits it always did.  Per used point i < counts[b]:
 *   1. Forward pass: the LK the entry point always ran (seeded or not by ofk_set_lk_seed / init_pts) -> next, st_f, err.
 *   2. Backward pass (fb_mode != OFK_FB_OFF): the same LK with the NEXT frame's pyramid as "prev" and the previous frame's as "next",
 *      from next[i] for EVERY used point whatever st_f is (no compaction).  Window, criteria and min_eig_thr are the forward pass's;
 *      maxLevel is fb_level, -1 = the forward pass's, else min(fb_level, forward maxLevel); the level table is that of a pyramid of
 *      this depth (level offsets do not depend on the depth, so it addresses the same resident pyramids).  OFK_FB_PLAIN runs without
 *      flags (the search starts at next[i]: cv2.calcOpticalFlowPyrLK called a second time); OFK_FB_SEEDED runs with
 *      OFK_LK_USE_INITIAL_FLOW and start positions equal to the ORIGINAL points -> back, st_b (its err is discarded).
 *   3. Distance, float32, no contraction, in this order: dx = back.x - prev.x; dy = back.y - prev.y; fb2 = dx*dx + dy*dy.  The
 *      stored fb2 is that value where st_f == 1 && st_b == 1 and +infinity otherwise.
 *   4. keep = st_f == 1 && (fb off || (st_b == 1 && fb2 <= (float)(fb_thr * fb_thr))) && (err_max == 0 || err <= (float)err_max);
 *      the square is formed in double and rounded once; a NaN fails every comparison.
 *   5. status := keep; next and err stay as the forward pass left them (cv2 leaves the position of a lost point too).
 *      stats, 4 x int32 per image: points with st_f == 1; of those st_b == 0; of the rest fb2 over the threshold; of the rest err
 *      over the cap.
 * ofk_set_track_gate (NULL, or fb_mode OFK_FB_OFF with err_max 0: off) is a context setting read by ofk_pairs_run (every slice),
 * ofk_stream_step[_jpeg] and ofk_stream_step_fused[_jpeg]: the solve, the feasibility and legacy keep rules, the robust solve and its
 * drop, record field 13, the track update and ofk_stream_last_points all see the gated status.  Invalid settings (unknown mode;
 * fb_thr not finite or <= 0 with a mode other than OFK_FB_OFF; fb_level < -1 or above the context's max_level; err_max negative or
 * not finite) return OFK_E_INVALID and leave the previous setting in place.
 * ofk_track_gate_download: fb2 [batch][stride] f32, back_pts [batch][stride][2] f32, back_status [batch][stride] u8 (the first
 * min(stride, max_pts) of every row; zeros when the latest run had the err cap alone) and stats [batch][4] i32 of the latest run /
 * step with a gate on; any may be NULL; OFK_E_INVALID before such a run.  `batch` here is that run's own (the resident pairs, the
 * streams, or the batch of the latest gated ofk_lk_pyr_fb): the call writes that many rows, so size the buffers for it, or for the
 * context's max_batch.
 * ofk_lk_pyr_fb = ofk_lk_pyr_ex plus the gates as a stage entry on host buffers: status is the gated one; back_pts, back_status and
 * fb2 ([batch][pts_stride]..., nullable) are written only when fb_mode != OFK_FB_OFF.  g == NULL: no gate (ofk_lk_pyr_ex); any other
 * g is held to ofk_set_track_gate's rules, one that switches nothing on included, before any launch or allocation.
 * OFK_LK_GET_MIN_EIGENVALS with err_max != 0 is refused: err is no residual then. */
#define OFK_FB_OFF     0
#define OFK_FB_PLAIN   1   /* backward search starts at the forward result (cv2 called twice) */
#define OFK_FB_SEEDED  2   /* backward search starts at the ORIGINAL point (OFK_LK_USE_INITIAL_FLOW) */
typedef struct ofk_track_gate {
    int    fb_mode;     /* OFK_FB_* */
    double fb_thr;      /* pixels, > 0 and finite when fb_mode != OFK_FB_OFF */
    int    fb_level;    /* maxLevel of the backward pass; -1 = the forward pass's; effective value min(fb_level, forward maxLevel) */
    double err_max;     /* 0 = off; else status also needs err <= (float)err_max */
} ofk_track_gate;
int ofk_set_track_gate(ofk_ctx *ctx, const ofk_track_gate *g);
int ofk_get_track_gate(const ofk_ctx *ctx, ofk_track_gate *g);
int ofk_track_gate_download(ofk_ctx *ctx, float *fb2, float *back_pts, uint8_t *back_status, int stride, int *stats);
int ofk_lk_pyr_fb(ofk_ctx *ctx, const uint8_t *prev, const uint8_t *next, int batch, int h, int w, const float *prev_pts,
                  const int *counts, int pts_stride, int win, int max_level, int max_count, double eps, double min_eig_thr,
                  const float *init_pts, int flags, float *next_pts, uint8_t *status, float *err, const ofk_track_gate *g,
                  float *back_pts, uint8_t *back_status, float *fb2);

/* Lighting-insensitive LK: a gain alpha and a bias beta per window and Newton step, so that the tracker matches alpha J + beta
 * against I instead of J against I (auto-exposure between the two frames, vignetting across them).  Off by default; with it off
 * every entry point launches the kernels and returns the bits it always did.  With it on the tracker is kernels of its own
 * (k_lk_light, one wave per point); pyramid, level walk, bounds tests, the fixed-point bilinear weights, Ip / Ixp / Iyp, A11 / A12 /
 * A22, minEig, the status rules, the 2x2 solve, both stopping rules, OFK_LK_USE_INITIAL_FLOW and OFK_LK_GET_MIN_EIGENVALS are those
 * of ofk_lk_pyr_ex.  What changes is the mismatch vector and the residual err.  N = win * win; every sum below is an exact 64-bit
 * integer over the window and does not depend on the order of summation; I is the descaled template sample Ip (<= 8160), J the
 * interpolated next-frame sample of the step.
 *   1. Template sums, once per level: SI = sum I, SII = sum I^2, SIx = sum Ix, SIy = sum Iy, SIIx = sum I Ix, SIIy = sum I Iy.
 *   2. Per Newton step: SJ = sum J, SJJ = sum J^2, SJx = sum J Ix, SJy = sum J Iy.
 *   3. vI = N SII - SI^2, vJ = N SJJ - SJ^2.
 *   4. alpha, in f64: 1 in mode OFK_LIGHT_BIAS or when vI <= 0 or vJ <= 0; otherwise sqrt((double)vI / (double)vJ) - one division,
 *      one square root, both IEEE-rounded - clamped to [lo, gain_max] with lo = 1.0 / gain_max formed once on the host.
 *   5. Mismatch vector, in f64 in exactly this order, no contraction: cJx = N SJx - SJ SIx, cIx = N SIIx - SI SIx,
 *      b1 = (float)(((alpha * (double)cJx - (double)cIx) / (double)N) * 2^-20); b2 likewise with y.  This is
 *      sum (alpha J + beta - I) Ix with beta = mean I - alpha mean J.
 *   6. err, without OFK_LK_GET_MIN_EIGENVALS: at the final position SJ, SJJ and alpha as above, a12 = (int64)llrint(alpha * 4096),
 *      r_k = a12 (N J_k - SJ) - 4096 (N I_k - SI), err = (float)((double)sum |r_k| / (4096.0 * N * 32 * N)): the mean absolute
 *      residual of the compensated window in the units of the plain err, so ofk_track_gate.err_max keeps its meaning.
 * ofk_set_lk_light (NULL or mode OFK_LIGHT_OFF: off) is a context setting read by the forward LK of ofk_pairs_run (every slice),
 * ofk_stream_step[_jpeg] and ofk_stream_step_fused[_jpeg] and by the backward pass of their forward-backward gate; everything
 * behind LK sees only different next / status / err.  An unknown mode, or a gain_max that is not finite or is <= 1, returns
 * OFK_E_INVALID and leaves the previous setting in place.  ofk_lk_pyr, ofk_lk_pyr_ex and ofk_lk_pyr_fb do not read the setting.
 * ofk_lk_pyr_light = ofk_lk_pyr_fb plus the setting as an argument (forward and backward pass): light == NULL or mode
 * OFK_LIGHT_OFF is ofk_lk_pyr_fb itself, the same launches and the same bits; any other light is held to the setter's rules before
 * any launch. */
#define OFK_LIGHT_OFF 0
#define OFK_LIGHT_BIAS 1   /* beta alone (alpha = 1) */
#define OFK_LIGHT_GAIN 2   /* alpha and beta */
typedef struct ofk_lk_light {
    int    mode;       /* OFK_LIGHT_* */
    double gain_max;   /* finite, > 1; default 4: alpha is clamped to [1 / gain_max, gain_max] */
} ofk_lk_light;
int ofk_set_lk_light(ofk_ctx *ctx, const ofk_lk_light *light);   /* NULL or OFF: off */
int ofk_get_lk_light(const ofk_ctx *ctx, ofk_lk_light *light);
int ofk_lk_pyr_light(ofk_ctx *ctx, const uint8_t *prev, const uint8_t *next, int batch, int h, int w, const float *prev_pts,
                     const int *counts, int pts_stride, int win, int max_level, int max_count, double eps, double min_eig_thr,
                     const float *init_pts, int flags, float *next_pts, uint8_t *status, float *err, const ofk_track_gate *g,
                     float *back_pts, uint8_t *back_status, float *fb2, const ofk_lk_light *light);

/* The velocity covariance: first-order error propagation through the velocity solve, and a filter correct that uses it in the place of
 * the constant R.  (The reference carries vel_err, feat_err, flow_err, ang_err, d_err, normal_err through every callback of its node
 * and never reads them; its simulation.py estimates the same dependence from 100 noisy re-solves per step.)  Off by default; with it
 * off every entry point launches the kernels and returns the bits it always did.
 * For one problem let the kept points be those the solve used (gated status / valid / feasibility keep / legacy keep, and with the
 * robust solve on those of final weight w > 0), with the solve's per-point terms q, sA, sB and M = sum w sA^2 X^T X,
 * g = sum w sA sB X^T X q.  The plain solve's v = M^+ g is a function of its inputs; C_v = J Sigma J^T with J its exact first
 * derivative and Sigma diagonal: all inputs independent and zero-mean (the noise model of simulation.py:40-45).  The robust weights
 * are held fixed (the usual IRLS sandwich) and v is the solve's own, read from its record.  A point the robust drop takes out of a
 * stream's tracks in the same step has w = 0 and a cleared keep flag by the time the covariance kernel runs behind the solve: it is no
 * kept point by either, and that step's record is the same with drop 0 and drop 1.
 *   source     inputs                                            variance each
 *   flow       u_i, 2 per kept point                             sigma_flow^2
 *   position   x_i, 2 per kept point, u_i held fixed             sigma_pos^2
 *   gyro       omega, 3                                          sigma_omega[k]^2; with omega_from_imu and ofk_fusion.use_imu the resident
 *                                                                IMU state's slots 21-23 (variances already)
 *   range      d                                                 sigma_d^2
 *   normal     n, 3 components, isotropic                        sigma_normal^2
 *   lever arm  t / offset, 3, isotropic; only through v - w x t  sigma_offset^2
 * C_uav is the same propagation through v_uav = R (v - omega x offset) (node:258; R taken as exact), in the stage entry through
 * v - omega x t (R = I; t == NULL: C_uav = C_v, no lever-arm term).  The gyro reaches C_uav by both routes: its Jacobian there is
 * dv/domega + [offset]x.
 * OFK_COV_PROPAGATE: all six terms.  OFK_COV_RESIDUAL: the flow and position terms are replaced by s^2 M^+, s^2 = RSS / (2 m - 3)
 * with RSS the record's field 3 (the weighted sum of a robust run) and m the kept points (each point's three rows have rank 2); the
 * common-mode terms (gyro, range, normal, lever arm) stay as given: no residual sees them.
 * Void - all zeros with flag 1 - when the solve's rank is below 3, in residual mode when 2 m <= 3, when an entry is not finite, and
 * for a pair with scaling == 0 or d == 0.
 * Cov record, OFK_COV_DOUBLES per problem: 0-5 C_v upper triangle (xx xy xz yy yz zz); 6-11 C_uav likewise; 12 s^2 (0 when
 * 2 m <= 3); 13 flag; 14 NIS of the filter's correct (0 where none ran); 15 gated; 16-21 the trace of each source's share of C_v:
 * flow, position, gyro, range, normal, lever arm (the last of C_uav before the rotation; in residual mode 16 holds the trace of
 * s^2 M^+ and 17 is 0); 22-23 reserved, 0.
 * Units: sigma_flow and sigma_pos are in the units of the points an entry takes - scaled units in ofk_velocity_solve_cov, pixels in
 * the resident paths, where the kernel multiplies them by the pair's `scaling` (sensor slot 19).
 * The filter: every correct of ofk_stream_step_fused[_jpeg] and ofk_pairs_filter_step that runs with a setting on reports its
 * normalised innovation squared NIS = nu^T S^-1 nu.  With filter_r = 1 it uses R_eff = the configured R with its top-left 3x3 block
 * replaced by z_sign^2 C + r_floor I, C = C_uav when z_source is 1, else C_v; rows 3.. of a 6-row measurement keep R; a void
 * covariance falls back to the whole of R.  With nis_max > 0 a correct whose NIS exceeds it is skipped: state and P stay at the
 * prediction and gated = 1.  (With a setting on the fuse kernel leaves the filter at its prediction and the covariance kernel behind
 * it corrects and rewrites fused[0..7].)
 * ofk_set_cov (NULL or mode OFK_COV_OFF: off) is a context setting read by ofk_pairs_run (every slice), ofk_pairs_filter_step,
 * ofk_stream_step[_jpeg] and ofk_stream_step_fused[_jpeg].  Refused with OFK_E_INVALID before any launch, the previous setting staying
 * in place: an unknown mode; a sigma, r_floor or nis_max that is negative or not finite; omega_from_imu or filter_r not 0/1; filter_r
 * with mode OFF.  OFK_SOLVE_OFMODULE (no omega, no d, a per-point weight that is itself a function of the flow) and OFK_FLOW_ROTATIONAL
 * (a flow that is no measurement) are not the sensor model: refused with OFK_E_INVALID wherever a setting is on.
 * Records are bit-identical across launch forms (one wave per pair from 128 pairs per slice on, a 256-thread workgroup below), slice
 * counts and overlap settings.
 * ofk_cov_download: cov [batch][OFK_COV_DOUBLES] of the latest run / step with the setting on (`batch` is that run's own);
 * OFK_E_INVALID before such a run.
 * ofk_velocity_solve_cov = ofk_velocity_solve's arguments (n <= 4096; NODE or SIM) plus the robust setting (NULL: the plain solve) and
 * the covariance setting (mode PROPAGATE or RESIDUAL; filter_r 0); out as ofk_velocity_solve, cov [batch][OFK_COV_DOUBLES]. */
#define OFK_COV_OFF 0
#define OFK_COV_PROPAGATE 1
#define OFK_COV_RESIDUAL 2
#define OFK_COV_DOUBLES 24
typedef struct ofk_cov { int mode; double sigma_flow, sigma_pos, sigma_d, sigma_omega[3], sigma_normal, sigma_offset;
                         int omega_from_imu; int filter_r; double r_floor; double nis_max; } ofk_cov;
int ofk_set_cov(ofk_ctx *ctx, const ofk_cov *c);
int ofk_get_cov(const ofk_ctx *ctx, ofk_cov *c);
int ofk_cov_download(ofk_ctx *ctx, double *cov);
int ofk_velocity_solve_cov(ofk_ctx *ctx, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                           const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                           const ofk_robust *r, const ofk_cov *c, double *out, double *cov);

/* The joint velocity and rotation solve: the gyro refined from the flow.  Every solve of the library takes the sensor record's omega as
 * exact when it forms q = u + p x omega; a gyro sample associated by nearest time stamp (evaluate_exp.py:68-80) lags by up to half an
 * IMU period, a common-mode error no per-point repair sees.  The flow is linear in (v, omega), so both come from one 6-unknown linear
 * least squares on sums of the solve's own kind.  Off by default; with it off every entry point launches the kernels and returns the
 * bits it always did, with no allocation and no launch.  All arithmetic is f64.
 * Point set: the kept points are exactly the solve's - gated status / valid / pair feasibility keep, and behind a robust run those of
 * final weight w > 0, w used as the weight and held fixed (the weights are not re-run at the refined omega).
 * Model: with omega0 the sensors' omega, p = (x, y, 1), X = [p]x, N = X^T X = |p|^2 I - p p^T and the solve's per-point terms at omega0,
 * q0 = (u, 0) + p x omega0, a = sA, b = sB, point i's rows for omega = omega0 + delta are  a X v + b N delta = b X q0  (X X = -N).
 * With the prior delta_k ~ N(0, sigma_omega[k]^2) the normal equations are [M, K; K^T, D + Lambda] (v, delta) = (g_v, g_delta):
 *   M = sum w a^2 N (the solve's own matrix)     K = -sum w a b |p|^2 X (three sums)     D = sum w b^2 |p|^2 N (six sums)
 *   Lambda = diag((d sigma_f / sigma_omega[k])^2)
 * sigma_f is sigma_flow in the units of the points: scaled units in ofk_velocity_solve_joint, pixels x `scaling` (sensor slot 19) in the
 * resident paths, as for the covariance.  Solution by the Schur complement, with v_s = M^+ g_v read from the solve's record:
 *   c = sum w b |p|^2 X (b q0 - a v_s)   (three sums; the reduced right-hand side g_delta - K^T v_s)
 *   S = D + Lambda - K^T M^-1 K,   delta = S^-1 c,   v = v_s - M^-1 K delta,   omega^ = omega0 + delta
 * M is accumulated again in the solve's own order; M^-1 and S^-1 both come from the eigen-decomposition (cyclic Jacobi) the solve uses;
 * all 19 sums are added over four virtual waves as (s0 + s1) + (s2 + s3), so records are bit-identical across launch forms (one wave
 * per pair from 128 pairs per slice on, a 256-thread workgroup below), slice counts and overlap settings.
 * Per-axis prior sigma_omega[k]: +inf = the axis is free (Lambda_k = 0); 0 = the axis is held: it is taken out of S and delta_k = 0;
 * anything else is the prior's standard deviation.  With omega_from_imu under ofk_fusion.use_imu the variances are the resident IMU
 * state's slots 21-23 (variances already; 0 holds, +inf frees).  With all three axes held every record is bit-identical to the
 * setting off (the joint record reports flag 0, delta = 0 and C_v = (d sigma_f)^2 M^-1).
 * Not attempted, flag 1 - the record is untouched, omega^ = omega0: the solve did not solve (rank < 3, non-finite sums, in the stream
 * steps record[15] == 0), `scaling` == 0 or d == 0, or any joint sum or result is not finite.
 * Unobservable, flag 2 - the record is untouched, omega^ = omega0: among the estimated axes an eigenvalue of S is not positive or falls
 * below sqrt(eps 3 m) times the largest, m the kept points.  Slots 12-14 report the eigenvalues.
 * On success, flag 0: record / out fields 0-2 become v (the stage entry takes omega^ x t off when t is given); field 3 the residual sum
 * of squares sum w |a X v - b X q(omega^)|^2, without the prior term, from a second walk over the points in the solve's order; record
 * fields 8-10 become R (v - omega^ x offset).  Fields 4-7 and 11-15 stay.
 * Joint record, OFK_JOINT_DOUBLES per problem: 0-2 omega^; 3-5 delta; 6-8 fields 0-2 of the solve's record before; 9 its residual
 * before; 10 flag; 11 kept points; 12-14 eigenvalues of S, descending, 0 for held axes (0 with flag 1); 15-20 C_omega =
 * (d sigma_f)^2 S^-1, upper triangle (xx xy xz yy yz zz; 0 in held rows); 21-26 C_v = (d sigma_f)^2 (M^-1 + G S^-1 G^T), G = M^-1 K;
 * 27-31 reserved, 0.  With a flag set 3-5 and 15-26 are 0.
 * ofk_set_joint (NULL or mode OFK_JOINT_OFF: off) is a context setting read by ofk_pairs_run (every slice), ofk_stream_step[_jpeg] and
 * ofk_stream_step_fused[_jpeg]; ofk_pairs_filter_step behind such a run reads the rewritten records.  In the fused step with a filter
 * the fuse kernel leaves the filter at its prediction and the joint kernel behind it corrects with the joint v / v_uav, rewrites
 * fused[0..7] and repeats vel_overwrite with the joint v_uav; under use_imu omega0, the normal and R are the IMU state's.
 * Refused with OFK_E_INVALID before any launch, the previous setting staying in place: an unknown mode; a sigma_omega that is negative
 * or NaN; sigma_flow not finite or <= 0; omega_from_imu not 0/1.  Refused with OFK_E_INVALID by the runs and steps where the setting is
 * on: OFK_SOLVE_OFMODULE, OFK_FLOW_ROTATIONAL and OFK_KEEP_LEGACY (not the sensor model, as for the covariance), and the covariance
 * setting together with this one (its propagation treats omega as an input, not an estimate; the joint record's C_v is the stopgap).
 * ofk_joint_download: joint [batch][OFK_JOINT_DOUBLES] of the latest run / step with the setting on (`batch` is that run's own);
 * OFK_E_INVALID before such a run.
 * ofk_velocity_solve_joint = ofk_velocity_solve's arguments (n <= 4096; NODE or SIM) plus the robust setting (NULL: the plain solve)
 * and the joint setting (mode OFK_JOINT_ON); out as ofk_velocity_solve after the rewrite, joint [batch][OFK_JOINT_DOUBLES]. */
#define OFK_JOINT_OFF 0
#define OFK_JOINT_ON 1
#define OFK_JOINT_DOUBLES 32
typedef struct ofk_joint { int mode; double sigma_flow; double sigma_omega[3]; int omega_from_imu; } ofk_joint;
int ofk_set_joint(ofk_ctx *ctx, const ofk_joint *j);
int ofk_get_joint(const ofk_ctx *ctx, ofk_joint *j);
int ofk_joint_download(ofk_ctx *ctx, double *joint);
int ofk_velocity_solve_joint(ofk_ctx *ctx, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                             const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                             const ofk_robust *r, const ofk_joint *j, double *out, double *joint);

/* The gyro bias of a stream: filtered from the flow, taken out of omega in front of every step.  The joint solve above repairs the gyro
 * one frame at a time, with six unknowns where the plain solve has three, and forgets what it found; a gyro bias is constant over
 * seconds, so a stream learns it once and subtracts it before anything reads omega.  Off by default; with it off there is no
 * allocation and no launch and every entry point returns the bits it always did.  All arithmetic is f64, in the order written here.
 * Model: omega_true = omega_gyro - b, b a random walk of variance q per step, the gyro's white noise sigma_gyro.  State per stream: b^ (3)
 * and P (3 x 3, symmetric), in rad per frame interval, the units of sensor slots 4-6.  An axis with p0[k] == 0 is held at b0[k] (the
 * joint solve's "0 holds"): it is never estimated and its rows of P stay as they are (0 from the setting).
 * Apply (k_gyro_bias_apply, directly behind the sensors' upload): the raw omega goes into the bias record and the device copy of the
 * sensor rows gets slots 4-6 := omega - b^, one subtraction per axis; under ofk_fusion.use_imu the IMU state's slots 18-20 likewise, and
 * then that omega is the record's raw one.  LK's seed, the rolling shutter's gyro mode, the finite-motion rewrite, the feasibility rule,
 * every solve and every second-stage kernel read the corrected omega; none of them changes.  Under use_imu the same kernel ends the step
 * by putting the IMU state's raw bits back, so a step with no ofk_imu_push in between does not subtract twice.  The caller's sensor array
 * is never written.
 * Filter step (k_stream_bias, directly behind the solve kernel, in front of any second-stage kernel; update != 0 and at least one axis
 * estimated): the joint solve's core over the joint solve's point set at omega0 = the corrected omega, prior variance +inf on the
 * estimated axes E and 0 on the held ones, d sigma_f as for the joint solve; nothing but the bias record is written.  Then
 *   predict    P_kk += q for k in E, on every step, whatever follows
 *   flag 1, 2  the core's own (not attempted / unobservable): reported, no update
 *   z = -delta_E,  R = C_omega,EE + sigma_gyro^2 I,  S = P_EE + R;  S^-1 from the solve's eigen-decomposition over the |E| largest
 *              eigenvalues; a value of S or NIS that is not finite or an eigenvalue that is not positive: flag 2, no update
 *   NIS = z^T (S^-1 z);  nis_max > 0 and not NIS <= nis_max: flag 3, no update
 *   K = P S^-1 (held columns of S^-1 are 0),  b^_i += K_i0 z_0 + K_i1 z_1 + K_i2 z_2,  P_EE := R (S^-1 P)_EE,  then P_ij := (P_ij + P_ji) / 2
 *              R S^-1 P is P - P S^-1 P written as a product: the difference cancels once P is large against R (a wide prior) and
 *              can leave P indefinite, the product cannot.  Rows and columns of held axes are not written.
 * Bias record, OFK_BIAS_DOUBLES per stream: 0-2 b^ after the step; 3-8 P, upper triangle (xx xy xz yy yz zz); 9-11 raw omega; 12-14 the
 * omega used; 15-17 delta (0 with a flag set); 18 flag (0 updated, 1 not attempted, 2 unobservable, 3 gated, 4 apply only: update == 0
 * or no axis estimated); 19 NIS (0 unless the flag is 0 or 3); 20 updates so far; 21 steps so far; 22-27 R, upper triangle (0 unless
 * the flag is 0 or 3); 28 kept points; 29-31 reserved, 0.
 * ofk_set_gyro_bias (NULL or mode OFK_BIAS_OFF: off) is a context setting read by ofk_stream_step[_jpeg] and
 * ofk_stream_step_fused[_jpeg]; ofk_pairs_run ignores it, as it ignores the zones: independent pairs carry no state.  The state is
 * (b0, diag(p0^2)) with both counters 0 when the setting is set and at every ofk_stream_begin[_jpeg].  update == 0 applies b^ and never
 * changes it (a calibrated gyro).  Refused with OFK_E_INVALID, the previous setting staying in place: an unknown mode; sigma_flow not
 * finite or <= 0; sigma_gyro, q, nis_max or a p0 negative or not finite; a p0 whose square is not finite (the start state diag(p0^2)
 * must be one ofk_gyro_bias_reset would take), by ofk_gyro_bias_step as well; a b0 not finite; update not 0/1.  With update on the steps
 * refuse OFK_SOLVE_OFMODULE, OFK_FLOW_ROTATIONAL and OFK_KEEP_LEGACY: not the sensor model, as for the joint solve.
 * ofk_gyro_bias_reset: state [batch][9] = b^ (3), P upper triangle (6), all finite, loaded into the first `batch` streams, their
 * counters 0 (a hot start); the setting must be on.  ofk_gyro_bias_download: rec [batch][OFK_BIAS_DOUBLES] of the latest step with the
 * setting on (`batch` is that step's own); OFK_E_INVALID before such a step.
 * ofk_gyro_bias_step is one step without images: apply on omega_raw [batch][3], ofk_velocity_solve[_robust] at the corrected omega
 * (n <= 4096; NODE or SIM; wgt must be NULL; r NULL: the plain solve), then the filter step over the same points.  state
 * [batch][OFK_BIAS_DOUBLES] goes in (slots 0-8, 20 and 21 are read) and comes out as the step's bias record; out as ofk_velocity_solve. */
#define OFK_BIAS_OFF 0
#define OFK_BIAS_ON 1
#define OFK_BIAS_DOUBLES 32
typedef struct ofk_gyro_bias { int mode; double sigma_flow; double sigma_gyro; double q; double p0[3]; double b0[3]; double nis_max; int update; } ofk_gyro_bias;
int ofk_set_gyro_bias(ofk_ctx *ctx, const ofk_gyro_bias *g);
int ofk_get_gyro_bias(const ofk_ctx *ctx, ofk_gyro_bias *g);
int ofk_gyro_bias_reset(ofk_ctx *ctx, const double *state, int batch);
int ofk_gyro_bias_download(ofk_ctx *ctx, double *rec);
int ofk_gyro_bias_step(ofk_ctx *ctx, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                       const double *d, const double *nrm, const double *omega_raw, const double *wgt, const ofk_robust *r,
                       const ofk_gyro_bias *g, double *state, double *out);

/* The plane solve: the ground normal refined from the flow.  Every solve of the library - plain, robust, joint, the covariance, the
 * feasibility rule - takes the plane's normal as exact: the IMU's R [0,0,1], under ofk_fusion.use_imu the resident IMU state's, so
 * level ground is assumed.  A normal that is off is a common-mode error no residual sees (ofk_cov's sigma_normal only books it); the
 * flow itself determines it.  Off by default; with it off every entry point launches the kernels and returns the bits it always did,
 * with no allocation and no launch.  All arithmetic is f64.
 * Point set: the kept points are exactly the solve's - gated status / valid / pair feasibility keep, and behind a robust run those of
 * final weight w > 0, w used as the weight and held fixed (the weights, the feasibility keep, the LK seed, the camera model and the
 * rolling-shutter correction go on reading the sensors' normal).
 * Model: with p = (x, y, 1), X = [p]x, N = X^T X, the solve's per-point terms q = (u, 0) + p x omega, sA, sB at the sensors' normal n0
 * and distance d0, and m = n / d the plane's inverse-distance vector, point i's three rows are
 *   r_i = sB_i [ (m.p_i) X_i v - X_i q_i ];
 * at m0 = n0 / d0 these are the solve's rows sA X v - sB X q, for NODE and for SIM.  The rows are bilinear in (v, m) and (s m, v / s)
 * is a gauge freedom, which the range sensor fixes: it measured a range along the body-fixed beam e (`beam`, normalised here; default
 * the optical axis), so m.e = (n0.e) / d0 is held and m = m0 + T tau, tau in R^2, T = [t1 t2], t1 = normalize(e x a) with a the
 * coordinate axis of smallest |e_k| (lowest index on a tie), t2 = e x t1.  The unknowns are (v, tau).  The prior on the tilt is
 * isotropic, tau ~ N(0, (sigma_normal / d0)^2 I), sigma_normal in radians, and enters as Lambda = (d0^2 sigma_f / sigma_normal)^2 I;
 * sigma_f is sigma_flow in the units of the points: scaled units in ofk_velocity_solve_plane, pixels x `scaling` (sensor slot 19) in
 * the resident paths.  sigma_normal = +inf leaves the tilt free; 0 holds it: nothing is estimated, every record is bit-identical to
 * the setting off (the plane record reports flag 0, tau = 0 and C_v = (d0 sigma_f)^2 M^-1).
 * Iteration: Gauss-Newton from the solve's v (read from the record) and tau = 0, iters + 1 walks over the kept points (iters 1..16).
 * Each walk sums at the current (v, tau), with c = m.p, a = sB c (first walk: a = sA, the solve's own rows), h = T^T p, y = X v:
 *   M = sum w a^2 N (6; the first walk's is the solve's own matrix in its order)   K = sum w sB a (X^T y) h^T (6)
 *   D = sum w sB^2 |y|^2 h h^T (3)   g_v = -sum w a X^T r (3)   g_tau = -sum w sB (y.r) h (2)   sum w |r|^2 and the count
 * 22 sums, added over four virtual waves as (s0 + s1) + (s2 + s3), so records are bit-identical across launch forms (one wave per
 * pair from 128 pairs per slice on, a 256-thread workgroup below), slice counts and overlap settings.  After walks 0 .. iters-1 the
 * step is taken by the Schur complement: S = D + Lambda - K^T M^-1 K (2 x 2), dtau = S^-1 (g_tau - Lambda tau - K^T M^-1 g_v),
 * dv = M^-1 (g_v - K dtau); M^-1 from the cyclic Jacobi the solve uses, S^-1 in closed form from its eigen-decomposition.  The last
 * walk does not step: it gives the residual at the solution and the Hessian there.
 * Flags (plane record slot 10); with a flag other than 0 the record / out is untouched and slots 0-3 report n0, d0:
 *   0 success.
 *   1 not attempted: the solve did not solve (rank < 3; in the stream steps record[15] == 0), `scaling` == 0, d0 == 0 or n0.e == 0, or
 *     any sum or result is not finite.
 *   2 unobservable: a walk's S has an eigenvalue that is not positive, or the predicted 1 sigma of the normal's angle,
 *     d0 sqrt(lambda_max((d0 sigma_f)^2 S^-1)) of the last walk, exceeds sigma_max (radians; +inf disables the gate).  This is what
 *     stops a hover: the information about tau scales with |v|^2, which is why the threshold is absolute.
 *   3 rejected: the final objective sum w |r|^2 + tau^T Lambda tau is larger than the first walk's.
 * On flag 0 with the tilt estimated: record / out fields 0-2 become v (the stage entry takes omega x t off when t is given); field 3
 * the last walk's sum w |r|^2, without the prior term; record fields 8-10 become R (v - omega x offset).  Everything else stays.
 * Plane record, OFK_PLANE_DOUBLES per problem: 0-2 n^ = m^ / |m^|; 3 d^ = 1 / |m^|; 4-5 tau; 6-8 fields 0-2 of the solve's record
 * before; 9 its residual before; 10 flag; 11 kept points; 12-13 eigenvalues of the last S formed, descending; 14 predicted 1 sigma
 * of the angle; 15 angle between n^ and n0; 16 |last step| = sqrt(|dv|^2 + d0^2 |dtau|^2) over |v|; 17-19 C_tau = (d0 sigma_f)^2 S^-1,
 * upper triangle; 20-25 C_v = (d0 sigma_f)^2 (M^-1 + G S^-1 G^T), G = M^-1 K, upper triangle (xx xy xz yy yz zz); 26 the first walk's
 * objective; 27 the final objective; 28-31 reserved, 0.  With a flag set 4-5 and 14-25 are 0.
 * ofk_set_plane (NULL or mode OFK_PLANE_OFF: off) is a context setting read by ofk_pairs_run (every slice), ofk_stream_step[_jpeg] and
 * ofk_stream_step_fused[_jpeg]; ofk_pairs_filter_step behind such a run reads the rewritten records.  In the fused step with a filter
 * the fuse kernel leaves the filter at its prediction and the plane kernel behind it corrects with the refined v / v_uav, rewrites
 * fused[0..7] and repeats vel_overwrite; under use_imu n0, omega and R are the IMU state's.  OFK_IMU_STATE carries the normal but no
 * variance of it (vel, times, rotation, normal, ang, ang_err), so there is no normal_from_imu field: the prior is sigma_normal.
 * Refused with OFK_E_INVALID before any launch, the previous setting staying in place: an unknown mode; sigma_flow not finite or <= 0;
 * sigma_normal negative or NaN; sigma_max <= 0 or NaN; a beam of zero length or not finite; iters outside 1..16.  Refused with
 * OFK_E_INVALID by the runs and steps where the setting is on: OFK_SOLVE_OFMODULE, OFK_FLOW_ROTATIONAL and OFK_KEEP_LEGACY (not the
 * sensor model), and ofk_set_joint or ofk_set_cov together with this one (both take the normal as an input).
 * ofk_plane_download: plane [batch][OFK_PLANE_DOUBLES] of the latest run / step with the setting on (`batch` is that run's own);
 * OFK_E_INVALID before such a run.
 * ofk_velocity_solve_plane = ofk_velocity_solve_joint's arguments with the plane setting (mode OFK_PLANE_ON) in the joint setting's
 * place; out as ofk_velocity_solve after the rewrite, plane [batch][OFK_PLANE_DOUBLES].  wgt is there for the solve entries' common
 * signature alone and must be NULL (OFK_E_INVALID otherwise): the only weights the plane solve takes are the robust setting's. */
#define OFK_PLANE_OFF 0
#define OFK_PLANE_ON 1
#define OFK_PLANE_DOUBLES 32
typedef struct ofk_plane { int mode; double sigma_flow; double sigma_normal; double sigma_max; double beam[3]; int iters; } ofk_plane;
int ofk_set_plane(ofk_ctx *ctx, const ofk_plane *p);
int ofk_get_plane(const ofk_ctx *ctx, ofk_plane *p);
int ofk_plane_download(ofk_ctx *ctx, double *plane);
int ofk_velocity_solve_plane(ofk_ctx *ctx, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                             const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                             const ofk_robust *r, const ofk_plane *p, double *out, double *plane);

/* The epipolar solve: velocity and per-point inverse depths over ground that is no plane.  Every other solve of the library - plain,
 * robust, joint, plane, the covariance, the feasibility rule - takes each point's depth from one plane, Z = d / (n.p).  Roofs, trees,
 * a ledge or a ramp are no plane, and the robust solve helps only while a single plane holds the majority of the points.  This solve
 * needs the gyro and the range sensor alone.  Off by default; with it off every entry point launches the kernels and returns the bits
 * it always did, with no allocation and no launch.  All arithmetic is f64.
 * Point set: the solve's own - gated status / valid / pair feasibility keep.  weights = OFK_EPI_W_ONE (default) ignores the robust
 * weights (they are the plane model's verdict, the thing being replaced): every kept point enters with w = 1.  OFK_EPI_W_ROBUST takes
 * them as the joint solve does: points of final weight w > 0, w used as the weight.
 * Flow equation: with p = (x, y, 1), X = [p]x and q = (u, 0) + p x omega (the solve's per-point term) the flow equation is
 * rho_i X v = X q_i, rho_i point i's inverse depth.  Eliminating rho_i leaves one row per point, c_i.v = 0 with c_i = p_i x q_i: no
 * plane appears, and only the direction of v is determined.
 * Direction: the minimiser of sum w (c_i.t)^2 is badly biased at low flow-to-noise ratios.  Flow noise delta enters c_i as
 * X_i (delta, 0), so E[sum w c c^T] = E0 + sigma^2 N0 with E = sum w c c^T (six sums) and N0 = sum w X_i D X_i^T, D = diag(1, 1, 0)
 * (six sums).  t^ is the generalised eigenvector of (E, N0) for the smallest eigenvalue lambda_1 (Kanatani's renormalisation), without
 * iteration: the cyclic Jacobi the solve uses gives W = N0^(-1/2), again the smallest eigenvector y of W E W, and t^ = W y / |W y|.
 * Flow noise: sigma^ = sqrt(lambda_1 m / (m - 2)), m the kept points, in the units of the points.  lambda_1 is taken as t^'s Rayleigh
 * quotient t^^T E t^ / t^^T N0 t^ = sum w (c_i.t^)^2 |W y|^2 with the numerator summed from the second walk's residuals: the value the
 * decomposition returns carries a rounding floor of eps lambda_max, this one has none and is never negative.
 * Per point (second walk): a_i = (q - q_z p)_xy, the derotated image flow; b_i = (t^_x - t^_z x, t^_y - t^_z y);
 * kappa_i = a_i.b_i / |b_i|^2, the flow along the epipolar direction, = s rho_i; r_i = (a_i x b_i) / |b_i|, the flow across it
 * (c_i.t^ = |b_i| r_i).
 * Sign: t^ is flipped so that sum w a_i.b_i >= 0 (positive depths in aggregate); a point with kappa_i <= 0 then gets point flag 2.
 * Scale: the range sensor measured along the body-fixed beam e (`beam`, normalised here; default the optical axis), whose foot in the
 * image is p_e = e / e_z.  The anchor set is the kept points with |p_xy - p_e| <= anchor; over it s = sum w kappa_i m_i / sum w m_i^2,
 * m_i = (n0.p_i) / d0: the ground is taken as the sensors' plane under the beam only.  anchor = +inf takes every kept point.  anchor is
 * in the units of the points in ofk_velocity_solve_epipolar and pixels x `scaling` (sensor slot 19) in the resident paths.  Then
 * v = s t^ and rho_i = kappa_i / s.
 * Uncertainty: H = sum w c_i c_i^T / |b_i|^2 (six sums of the second walk); C_t = sigma^^2 (P H P)^+, P = I - t^ t^^T, the pseudo-inverse
 * over the two largest eigenvalues; the predicted 1 sigma of the direction is sqrt(tr C_t), radians;
 * var(s) = sigma^^2 sum_anchor w m_i^2 / |b_i|^2 / (sum_anchor w m_i^2)^2; C_v = s^2 C_t + var(s) t^ t^^T.
 * All sums - 13 in the first walk (E, N0, the count), 15 in the second (H, sum w r^2, sum w a.b, the anchor set's three sums and
 * count, the counts of kappa <= 0 and kappa >= 0, sum w (c.t^)^2) - are added over four virtual waves as (s0 + s1) + (s2 + s3), so records and point
 * rows are bit-identical across launch forms (one wave per pair from 128 pairs per slice on, a 256-thread workgroup below), slice
 * counts and overlap settings.
 * Flags (epipolar record slot 10); with a flag other than 0 the record / out is untouched and every point row is 0:
 *   0 success.
 *   1 not attempted: fewer than 3 kept points; d0, `scaling` or n0.e is 0 or e_z == 0; N0 has an eigenvalue not above eps 3 m times
 *     its largest; a sum, an input or a result is not finite (a kept point on the epipole, |b_i| = 0, is such a case); in the stream
 *     steps the solve did not solve (record[15] == 0).
 *   2 unobservable: P H P has fewer than two positive eigenvalues, or the predicted 1 sigma of the direction exceeds sigma_max
 *     (radians; +inf disables the gate).  This is what stops a hover, where the direction is noise.
 *   3 no scale: fewer than anchor_min anchor points, or s is not finite or s <= 0.
 * On flag 0: record / out fields 0-2 become v (the stage entry takes omega x t off when t is given); field 3 becomes sum w r_i^2, the
 * squared flow across the epipolar lines - NOT the solve's residual sum w |sA X v - sB X q|^2, and not comparable with it; record
 * fields 8-10 become R (v - omega x offset).  Everything else stays.
 * Epipolar record, OFK_EPI_DOUBLES per problem: 0-2 t^; 3 s; 4 sigma^; 5 sum w r_i^2; 6-8 fields 0-2 of the solve's record before;
 * 9 its residual before; 10 flag; 11 kept points; 12 anchor points; 13 points with kappa <= 0; 14-16 the generalised eigenvalues of
 * (E, N0), descending (16 is lambda_1, the Rayleigh quotient above); 17 predicted 1 sigma of the direction; 18-23 C_t, upper triangle (xx xy xz yy yz zz); 24 var(s);
 * 25-30 C_v, upper triangle; 31 reserved, 0.  With flag 1 everything but 6-11 is 0; with flag 2 slots 3, 18-30 are 0
 * (17 is +inf where P H P is singular); with flag 3 slots 3 and 24-30 are 0.
 * Point rows, [max_pts][4] per problem (ofk_epipolar_points_download; [n][4] in the stage entry): rho_i, r_i, |b_i| and the point
 * flag - 0 used, 1 not kept (or past the pair's count), 2 used with kappa_i <= 0 (rho_i <= 0).  Rows of a problem whose record
 * carries a flag are 0 throughout.
 * ofk_set_epipolar (NULL or mode OFK_EPI_OFF: off) is a context setting read by ofk_pairs_run (every slice), ofk_stream_step[_jpeg] and
 * ofk_stream_step_fused[_jpeg]; ofk_pairs_filter_step behind such a run reads the rewritten records.  In the fused step with a filter
 * the fuse kernel leaves the filter at its prediction and the epipolar kernel behind it corrects with the rewritten v / v_uav,
 * rewrites fused[0..7] and repeats vel_overwrite; under use_imu n0, omega and R are the IMU state's.  The camera model, the rolling
 * shutter and finite motion hand their ideal points to this solve as to every other.
 * Refused with OFK_E_INVALID before any launch, the previous setting staying in place: an unknown mode or weights; anchor <= 0 or NaN;
 * anchor_min < 1; sigma_max <= 0 or NaN; a beam of zero length or not finite.  Refused with OFK_E_INVALID by the runs and steps where
 * the setting is on: OFK_SOLVE_OFMODULE, OFK_FLOW_ROTATIONAL and OFK_KEEP_LEGACY (not the sensor model), and ofk_set_joint,
 * ofk_set_plane or ofk_set_cov together with this one (all three rest on the plane).
 * ofk_epipolar_download: epi [batch][OFK_EPI_DOUBLES] of the latest run / step with the setting on (`batch` is that run's own);
 * ofk_epipolar_points_download: points [batch][max_pts][4] of the same run; both OFK_E_INVALID before such a run.
 * ofk_velocity_solve_epipolar = ofk_velocity_solve_joint's arguments with the epipolar setting (mode OFK_EPI_ON) in the joint
 * setting's place; out as ofk_velocity_solve after the rewrite, epi [batch][OFK_EPI_DOUBLES], points [batch][n][4].  wgt is there for
 * the solve entries' common signature alone and must be NULL. */
#define OFK_EPI_OFF 0
#define OFK_EPI_ON 1
#define OFK_EPI_W_ONE 0
#define OFK_EPI_W_ROBUST 1
#define OFK_EPI_DOUBLES 32
typedef struct ofk_epipolar { int mode; double anchor; int anchor_min; double sigma_max; double beam[3]; int weights; } ofk_epipolar;
int ofk_set_epipolar(ofk_ctx *ctx, const ofk_epipolar *e);
int ofk_get_epipolar(const ofk_ctx *ctx, ofk_epipolar *e);
int ofk_epipolar_download(ofk_ctx *ctx, double *epi);
int ofk_epipolar_points_download(ofk_ctx *ctx, double *points);
int ofk_velocity_solve_epipolar(ofk_ctx *ctx, int variant, const double *x, const double *u, const uint8_t *valid, int batch, int n,
                                const double *d, const double *nrm, const double *omega, const double *t, const double *wgt,
                                const ofk_robust *r, const ofk_epipolar *e, double *out, double *epi, double *points);

/* optical_fusion.call_imu — node:61-89, batched over independent IMU streams, one message each.
 * state [batch][OFK_IMU_STATE]: vel[3], old_time, time_zero, first(0/1), rotation[9], normal[3], ang[3], ang_err[3]
 * msg   [batch][OFK_IMU_MSG]  : secs, nsecs, qx,qy,qz,qw, wx,wy,wz, cov0,cov4,cov8, ax,ay,az */
#define OFK_IMU_STATE 24
#define OFK_IMU_MSG   15
int ofk_imu_propagate(ofk_ctx *ctx, double *state, const double *msg, int batch);

/* of_library.py:270-286 (calc_height), :53-75 + :100-114 (convert_to_of inside dynamic_immobile), :291-317 (eval_ft) — the
 * per-feature estimators around the path, for a batch of track sets.  Per set b with counts[b] features (arrays are
 * [batch][stride]...): observed flow = pos - oldpos; height and its variance from the pin-hole model with the set's velocity
 * vel[b] +- vel_err[b]; immobile[i] = (observed - expected flow)^2 < var(observed) + var(expected) on both axes and neither old
 * coordinate equals dummy_value; score = w0 (1 - height_n) + w1 height_err_n + w2 (1 - centre_dist_n) + w3 pos_err_n with the
 * min/max normalisations of eval_ft; order = feature indices by ascending score (ties by index, NaN last; -1 past the count).
 * NaN follows numpy: the ranges are np.amin / np.amax, so ONE NaN among a set's heights, height variances, centre distances or
 * position errors makes that term zero for every feature of the set (level flight, v_z = 0: a feature without flow on one
 * axis has height_err = 0/0; a stationary one whose two estimates are infinities of opposite sign has height = NaN), and the
 * feature's own score is NaN where its own term is.  counts[b] is clamped to 0..stride; past it the outputs read 0 (order -1).
 * *bad_height is set non-zero when a height is not positive (where the reference raises ValueError).  pos, oldpos
 * [batch][stride][2] in pixels; pos_err, oldpos_err [batch][stride]; vel, vel_err [batch][3]; weight [4]. */
int ofk_feature_eval(ofk_ctx *ctx, const double *pos, const double *pos_err, const double *oldpos, const double *oldpos_err,
                     const int *counts, int batch, int stride, const double *vel, const double *vel_err, double focal_len,
                     double dummy_value, int img_w, int img_h, const double *weight, double *height, double *height_err,
                     uint8_t *immobile, double *score, int *order, int *bad_height);

/* velocity_measurment_node:249-252 — statistics of the per-feature plane distances d_i that r_tilde returns (ofk_feasibility):
 * sorted[b] = np.sort(d[b][:counts[b]]), diff[b][i] = sorted[i+1] - sorted[i], nsplit[b] = number of gaps >= d_exp_err (the
 * split the node's commented line describes: several ground planes in view).  Arrays [batch][stride], stride <= 4096.
 * The order is np.sort's: -inf first, +inf after every finite value, NaN last; a gap next to a NaN, or inf - inf, is NaN
 * and is not counted.  counts[b] is clamped to 0..stride; sorted and diff read 0 past the count, diff[b][counts[b]-1] too. */
int ofk_d_split(ofk_ctx *ctx, const double *d, const int *counts, int batch, int stride, double d_exp_err, double *sorted,
                double *diff, int *nsplit);

/* evaluate_exp.py:68-95 — sensor association for replayed logs: for every image time t_img[k] (seconds, as the script forms
 * them: float(secs - secs0) + float(nsecs)/1e9) the nearest IMU and range samples (np.argmin(np.abs(values - t)): the first
 * minimum), then d = range, R from the IMU quaternion (x,y,z,w), normal = R e_z, omega = angular velocity.  Fills fields
 * 0-15 of sensors[k] (see OFK_SENSOR_DOUBLES below; the other fields keep their values) and, when not NULL, the chosen
 * indices.  imu_quat [n_imu][4], imu_omega [n_imu][3].  A non-finite image time, sample time or range is refused with
 * OFK_E_INVALID before anything is uploaded (no sample is nearest to it). */
int ofk_associate_sensors(ofk_ctx *ctx, const double *t_img, int n_img, const double *imu_t, const double *imu_quat,
                          const double *imu_omega, int n_imu, const double *hgt_t, const double *hgt_range, int n_hgt,
                          double *sensors, int *imu_index, int *hgt_index);

/* node:258 — v_uav = R (v_obs - [w]x offset).  v_obs, ang, offset [batch][3]; rotation [batch][9]; v_uav [batch][3]. */
int ofk_post_solve(ofk_ctx *ctx, const double *v_obs, const double *rotation, const double *ang, const double *offset,
                   int batch, double *v_uav);

/* cv2.KalmanFilter(ns, nm, nc).predict(control) then .correct(measurement) — of_module.py:63-76,122,152
 * (the reference uses ns=nm=nc=3 with F=B=H=I; ns<=6, nm<=6, nc<=6 supported, row-major matrices shared by the batch).
 * x [batch][ns], P [batch][ns][ns] are updated in place; B/u nullable (no control); z nullable (predict only);
 * do_predict = 0 skips the predict step. */
int ofk_kf_predict_update(ofk_ctx *ctx, int ns, int nm, int nc, const double *F, const double *Bm, const double *H,
                          const double *Q, const double *Rm, double *x, double *P, const double *u, const double *z,
                          int batch, int do_predict);

/* of_simulation(...) — simulation.py:36-66 with the np.random.normal draws supplied by the caller:
 * z [trials][10+4n] standard normals in the reference's draw order (omega 3, t 3, height 1, flow 2n, position 2n,
 * normal 3 — drawn and discarded, simulation.py:45-46).  truth = v[3], omega[3], height, normal[3], t[3] (13);
 * sig = ang_vel, translation, height, flow, position, normal (6).  pos, true_flow [n][2].
 * v_obs [trials][3], bound [trials] (analytic error bound, simulation.py:56-64). */
int ofk_of_simulation(ofk_ctx *ctx, const double *truth, const double *sig, const double *pos, const double *true_flow,
                      int n, const double *z, int trials, double *v_obs, double *bound);
/* The same with the normals drawn ON THE DEVICE by a counter-based generator, for the 4096-wide batches of the Monte-Carlo sweeps
 * (simulation.py:183-461 at BASELINE configs[4]'s size: 2000 points x 4096 trials = 262 MB of host noise per step otherwise):
 * element e of the row of trial t of sweep step `step` = output (e & 1) of the Box-Muller transform of
 * Philox4x32-10(counter (e >> 1, t, step, 0), key (seed & 0xffffffff, seed >> 32)); uniforms ((x0 >> 5) 2^26 + (x1 >> 6) + 0.5) 2^-53.
 * Trials trial0 .. trial0 + trials - 1 (GLOBAL indices: ranks that shard the trials produce the same rows as one rank would).
 * ofk_noise_normals returns elements 0 .. count - 1 of one row - the generator itself (oracle: estimation_oracle.noise_normals). */
int ofk_of_simulation_rng(ofk_ctx *ctx, const double *truth, const double *sig, const double *pos, const double *true_flow, int n,
                          unsigned long long seed, unsigned step, unsigned trial0, int trials, double *v_obs, double *bound);
int ofk_noise_normals(ofk_ctx *ctx, unsigned long long seed, unsigned step, unsigned trial, int count, double *out);

/* feas_simulation(...) - simulation.py:70-104 (driven by the live experiment simulation.py:753-812: three ground planes, the
 * second one with randomly rotated flow), with the np.random.normal draws supplied by the caller:
 * z [trials][12+4n] standard normals in the reference's draw order (omega 3, t 3, height 1, flow 2n, position 2n,
 * velocity 3, orient 1, orient2 1).  truth = v[3] (unused by the reference's function body), omega[3], height, normal[3],
 * t[3], true_vel[3] (16); sig = ang_vel, translation, height, flow, position, normal, velocity (7; the reference reads the
 * last two from module globals).  pos, true_flow [n][2].  Per trial: perturbed inputs -> solve_lgs -> feasibility with the
 * solved velocity ("backward") and with the noisy prior velocity ("forward") -> per-point residual norms of both.
 * mean [6][n] = np.mean over the trials in the reference's return order: backward_para, backward_dist, forward_para,
 * forward_dist, backward_res, forward_res; per_trial (nullable) [trials][6][n]; v_obs (nullable) [trials][3]. */
#define OFK_FEAS_SIM_TRUTH 16
#define OFK_FEAS_SIM_SIG    7
int ofk_feas_simulation(ofk_ctx *ctx, const double *truth, const double *sig, const double *pos, const double *true_flow, int n,
                        const double *z, int trials, double *mean, double *per_trial, double *v_obs);

/* overlap(data1, data2) - simulation.py:124-136: histogram both samples over the `bins` (reference: 100, at most 1024) equal
 * bins spanning their joint range (np.histogram's edges and bin rule) and sum the bin-wise minima.  A non-finite sample is
 * refused with OFK_E_INVALID (np.histogram raises ValueError on a non-finite range). */
int ofk_hist_overlap(ofk_ctx *ctx, const double *data1, int n1, const double *data2, int n2, int bins, int *overlap);

/* ------------------------------------------------- resident frame-pair pipeline (the benchmarked path) */

typedef struct ofk_params {
    int    max_corners;      /* goodFeaturesToTrack maxCorners (<= ctx max_pts) */
    double quality;          /* qualityLevel */
    double min_distance;     /* minDistance */
    int    block_size;       /* blockSize */
    int    win;              /* LK winSize (square) */
    int    max_level;        /* LK maxLevel */
    int    max_count;        /* LK criteria COUNT */
    double eps;              /* LK criteria EPS */
    double min_eig_thr;      /* LK minEigThreshold (1e-4) */
    int    solve_variant;    /* OFK_SOLVE_NODE / OFK_SOLVE_SIM (ofk_pairs_run, ofk_stream_step); also OFK_SOLVE_OFMODULE in ofk_stream_step_fused */
    int    use_feasibility;  /* 1: keep points with r_tilde <= feas_T (node:238-245) using sensors' prior velocity */
    double feas_T;
} ofk_params;

/* Per-pair sensor record, [batch][OFK_SENSOR_DOUBLES] doubles:
 * 0 d (plane distance)  1-3 normal  4-6 omega  7-15 rotation (row-major)  16-18 offset (lever arm, node:204)
 * 19 scaling (node:182)  20 cx  21 cy (of.pix_trans, node:229)  22-24 prior velocity (feasibility; second measurement of a
 * 6-row filter)  25-27 filter control input (ofk_stream_step_fused, OFK_CONTROL_SENSORS) */
#define OFK_SENSOR_DOUBLES 28
/* Per-pair result record, [batch][OFK_RECORD_DOUBLES] doubles:
 * 0-2 v_obs  3 residual SS  4 rank  5-7 singular values  8-10 v_uav (node:258)  11 points used in the solve
 * 12 corners detected  13 points tracked (status==1)  14 corner candidates (after threshold + NMS)  15 reserved */
#define OFK_RECORD_DOUBLES 16

/* Copies a batch of BGR frame pairs into the context's device buffers (host -> HBM). */
int ofk_pairs_upload(ofk_ctx *ctx, const uint8_t *prev_bgr, const uint8_t *next_bgr, int batch, int h, int w);
/* The same from compressed frames: jpeg[i] / nbytes[i] = one baseline JPEG stream per frame (the payload of a
 * sensor_msgs/CompressedImage; the reference decodes it with cv_bridge.compressed_imgmsg_to_cv2 = cv::imdecode,
 * velocity_measurment_node.py:112).  All frames of a call must share size and chroma sampling.  Decoded on the device; pixels
 * identical to libjpeg's default decompressor (see ofk_jpeg_decode_bgr8).  On the default schedule (one slice, overlap on) the
 * decoder's colour kernel applies the pipeline's BGR -> gray conversion (node:113 cv2.cvtColor) to every pixel itself and writes the
 * gray frame straight into the pyramid set the next ofk_pairs_run takes: the BGR frame is never stored and that run skips its
 * first stage - same bytes in the gray level as after ofk_pairs_upload of the decoded frames. */
int ofk_pairs_upload_jpeg(ofk_ctx *ctx, const uint8_t *const *prev_jpeg, const size_t *prev_bytes, const uint8_t *const *next_jpeg,
                          const size_t *next_bytes, int batch);
/* The same in two phases, so that a camera loop can hide the host's share of the ingest (marker parse, staging copy, PCIe) behind
 * the GPU's work on the batch before:
 *   ofk_jpeg_stage(ctx, slot, jpeg, nbytes, count)   host + copy engine: parses `count` streams, packs tables and the entropy segments
 *       (without their byte stuffing, see ofk_jpeg_destuff) into pinned staging slot 0 or 1 and queues their asynchronous H2D copies
 *       on the context's copy stream as its worker threads finish their shares; returns when the host part is done.  It touches nothing but its slot, so it may run on a SECOND THREAD while the context's owner is inside any
 *       other entry point - as long as that is not the decode of the same slot.
 *   ofk_pairs_upload_staged(ctx, slot)               device: decodes the 2 B streams staged in `slot` - the B previous frames
 *       first, then the B next frames - into the resident frame-pair buffers (what ofk_pairs_upload_jpeg does after staging
 *       slot 0 itself).  A slot is decoded once.  On the default schedule the decoder runs on a stream of its own and writes the
 *       pyramid set the ofk_pairs_run in flight is not using, so it overlaps that run.
 * Loop: stage(0, batch 0); for k: { stage(k+1 & 1, batch k+1) on the helper thread; upload_staged(k & 1); ofk_pairs_run; }.
 * pipeline.FlowPipeline.run_jpeg_batches does exactly that; bench.py reports its rate as ingest_inclusive.jpeg_double_buffered. */
int ofk_jpeg_stage(ofk_ctx *ctx, int slot, const uint8_t *const *jpeg, const size_t *nbytes, int count);
/* Message of the slot's last ofk_jpeg_stage ("" after a success).  ofk_jpeg_stage never writes ofk_last_error: it may run on a helper
 * thread while the owner thread is inside another entry point, and the context holds ONE message. */
const char *ofk_jpeg_stage_error(const ofk_ctx *ctx, int slot);
int ofk_pairs_upload_staged(ofk_ctx *ctx, int slot);
int ofk_pairs_set_sensors(ofk_ctx *ctx, const double *sensors, int batch);
/* Runs gray -> pyramids -> corners -> LK -> centre/scale -> (feasibility) -> solve -> post-solve for every resident
 * pair.  Asynchronous on the context's stream; call ofk_sync / ofk_pairs_download to wait. */
int ofk_pairs_run(ofk_ctx *ctx, const ofk_params *p);
/* Any output pointer may be NULL.  records [batch][16] f64; prev_pts/next_pts [batch][max_corners][2] f32;
 * status [batch][max_corners] u8; err [batch][max_corners] f32; counts [batch]. */
int ofk_pairs_download(ofk_ctx *ctx, double *records, float *prev_pts, float *next_pts, uint8_t *status, float *err,
                       int *counts);
/* Writes the batch's velocity records as float32 [batch][8] = {vx,vy,vz,residual,n_used,s_min,rank,corners} to a
 * DEVICE pointer owned by the caller (the buffer an RCCL all_gather sends), asynchronously behind the latest ofk_pairs_run
 * (wait with ofk_mark + ofk_mark_wait, or ofk_sync). */
int ofk_pairs_export_records_f32(ofk_ctx *ctx, void *device_dst, int batch);

/* ------------------------------------------------- video streams: persistent tracks on the device (feature lifecycle)
 * velocity_measurment_node:92-177 with its commented-out blocks restored (of_module.py:78-167 and evaluate_exp.py:77-121
 * follow the same loop): `batch` independent streams advance one frame per call.
 *   begin : gray + pyramid of the first frames, goodFeaturesToTrack -> tracks                       (node:117-128, :120)
 *   step  : gray + pyramid of the new frames; LK from the tracks (node:133); velocity solve on the tracked points with
 *           x = new position, u = new - old (node:134-136, :229-258); tracks := new[status == 1];
 *           streams that had <= min_features tracks re-detect on the PREVIOUS frame with discs of mask_radius around
 *           the old positions masked out, maxCorners = p->max_corners - (old count), and append (node:157-166);
 *           the new frame becomes the previous one (node:175).
 * sensors as in ofk_pairs_set_sensors.  records [batch][16] as in ofk_pairs_download (slot 12 = tracks before the step,
 * 13 = tracked), tracks [batch][p->max_corners][2] f32 and counts [batch] = the tracks AFTER the step; any may be NULL. */
int ofk_stream_begin(ofk_ctx *ctx, const uint8_t *first_bgr, int batch, int h, int w, const ofk_params *p, float *tracks,
                     int *counts);
int ofk_stream_step(ofk_ctx *ctx, const uint8_t *next_bgr, const double *sensors, const ofk_params *p, int min_features,
                    int mask_radius, double *records, float *tracks, int *counts);
/* The same with the frames as the node receives them (node:112, 215): one baseline JPEG stream per camera (the payload of a
 * sensor_msgs/CompressedImage), decoded on the device into the stream's frame buffer - no decoded frame crosses PCIe.  Frame size
 * comes from the streams (all of one size and sampling; later frames must match the first). */
int ofk_stream_begin_jpeg(ofk_ctx *ctx, const uint8_t *const *jpeg, const size_t *nbytes, int batch, const ofk_params *p, float *tracks,
                          int *counts);
int ofk_stream_step_jpeg(ofk_ctx *ctx, const uint8_t *const *jpeg, const size_t *nbytes, const double *sensors, const ofk_params *p,
                         int min_features, int mask_radius, double *records, float *tracks, int *counts);

/* ---- the per-stream filters, resident on the device ("the only cross-pair state is the per-stream filter,
 * which stays on the GPU that owns the stream")
 * IMU dead-reckoning state (velocity_measurment_node:61-89), layout OFK_IMU_STATE as in ofk_imu_propagate:
 *   ofk_imu_reset   state of `batch` streams := state0 [OFK_IMU_STATE] (NULL: the node's initial values, node:182-217:
 *                   vel = 0.1, rotation = I, normal = e_z, first message pending)
 *   ofk_imu_push    the messages each stream received since its last frame, applied in order (k_imu_seq): msgs
 *                   [batch][max_msgs][OFK_IMU_MSG], counts [batch]; also accumulates the velocity increments (the filter's control)
 *   ofk_imu_state   download: state [batch][OFK_IMU_STATE], dv (nullable) [batch][3] = increments not yet consumed by a step
 * Kalman filter (cv2.KalmanFilter of of_module.py:63-76; ns, nm <= 6, nc <= 6; row-major matrices shared by the streams):
 *   ofk_filter_configure  matrices + every stream's state := x0 [ns], P0 [ns][ns]
 *   ofk_filter_state      download x [batch][ns], P [batch][ns][ns] */
int ofk_imu_reset(ofk_ctx *ctx, const double *state0, int batch);
int ofk_imu_push(ofk_ctx *ctx, const double *msgs, const int *counts, int max_msgs, int batch);
int ofk_imu_state(ofk_ctx *ctx, double *state, double *dv, int batch);
int ofk_filter_configure(ofk_ctx *ctx, int ns, int nm, int nc, const double *F, const double *Bm, const double *H, const double *Q,
                         const double *Rm, const double *x0, const double *P0, int batch);
int ofk_filter_state(ofk_ctx *ctx, double *x, double *P, int batch);

/* Per-pair filter update of the resident batch, queued behind the latest ofk_pairs_run (asynchronous): every pair's filter
 * (state from ofk_filter_configure, resident) predicts and corrects with z = z_sign * (z_source ? v_uav : v_obs) of its own record
 * when the solve had full rank - BASELINE configs[2] "batch of 1024 independent frame pairs + per-frame EKF update". */
int ofk_pairs_filter_step(ofk_ctx *ctx, double z_sign, int z_source, int batch);

/* What happens between calcOpticalFlowPyrLK and the next frame (ofk_stream_step_fused). */
#define OFK_FLOW_LK          0   /* u = new - old (node:235; of_module.py:108) */
#define OFK_FLOW_ROTATIONAL  1   /* of_module.py:113-114: the flow is overwritten by the rotational field of the sensors' omega */
#define OFK_KEEP_STATUS      0   /* status == 1, and r_tilde <= feas_T when p->use_feasibility (node:238-245) */
#define OFK_KEEP_LEGACY      1   /* legacy 4-arg r_tilde with the filter's predicted velocity, keep r - (uint8)(status - 1) >= feas_T: tracked points with r >= feas_T, a lost point's status-1 wraps to 255 (of_module.py:93,125-131) */
#define OFK_CONTROL_SENSORS  0   /* filter control = sensors[25..27] (of_module.py:122 draws it at random) */
#define OFK_CONTROL_IMU      1   /* filter control = velocity increments accumulated by ofk_imu_push since the last step */
typedef struct ofk_fusion {
    int    use_imu;          /* 1: normal, omega, rotation and the prior velocity come from the resident IMU state, not from `sensors` */
    int    flow;             /* OFK_FLOW_* */
    int    keep;             /* OFK_KEEP_*; the kept points become the stream's tracks (of_module.py:166) */
    int    filter;           /* 1: resident Kalman filter: predict(control) before the feasibility test, correct() after the solve */
    int    control;          /* OFK_CONTROL_* */
    double z_sign;           /* measurement = z_sign * velocity (of_module.py:152 corrects with -v_obs) */
    int    z_source;         /* 0: v_obs, 1: v_uav (lever arm + rotation applied, node:258) */
    int    vel_overwrite;    /* 1: the IMU state's velocity := v_uav after a solve (node:261) */
    int    redetect_replace; /* 1: streams with <= min_features tracks REPLACE them by maxCorners - count fresh corners of the previous
                                frame, no mask, before tracking (of_module.py:83-86); 0: append with a disc mask after tracking (node:157-166) */
    int    min_solve;        /* solve only with MORE than this many kept points (of_module.py:138: 3; node:256: 2) */
    int    hold_on_skip;     /* 1 (one stream per context only): a step that does not solve leaves the previous frame and the tracks as they
                                were, like the `continue` of of_module.py:138 - the next frame is tracked from the OLD one; the filter keeps
                                its prediction.  Costs one host wait per step.  0: the frame always advances (a batch shares one frame swap) */
} ofk_fusion;
/* ofk_stream_step with the filters in the loop: (redetect_replace) -> gray + pyramid of the new frames -> LK -> k_stream_fuse
 * (centre/scale, flow, filter predict, feasibility, solve with p->solve_variant incl. OFK_SOLVE_OFMODULE, lever arm + rotation,
 * filter correct, velocity overwrite) -> tracks := kept points -> (masked re-detection) -> frame swap.  records as in
 * ofk_stream_step (slot 15: 1 if the system was solved); fused [batch][8] = filter state x[0..5] (zero padded), trace(P), solved —
 * without a filter: v_uav (or the dead-reckoned velocity when nothing was solved).  of_module.py:138 `continue`s on <= 3 feasible points
 * WITHOUT advancing the frame: f->hold_on_skip = 1 reproduces that for a context with ONE stream (what the script is); a batch of
 * streams shares one frame swap, so there the frame always advances, the filter keeps its prediction and the record reports rank 0. */
int ofk_stream_step_fused(ofk_ctx *ctx, const uint8_t *next_bgr, const double *sensors, const ofk_params *p, const ofk_fusion *f,
                          int min_features, int mask_radius, double *records, double *fused, float *tracks, int *counts);
/* Next positions [batch][stride][2] and keep flags [batch][stride] of the latest step (valid until the next one): with the tracks
 * the caller held before the step they give the flow of the kept points, new - old (node:134-136). */
int ofk_stream_last_points(ofk_ctx *ctx, float *next_pts, uint8_t *keep, int stride);
int ofk_stream_step_fused_jpeg(ofk_ctx *ctx, const uint8_t *const *jpeg, const size_t *nbytes, const double *sensors, const ofk_params *p,
                               const ofk_fusion *f, int min_features, int mask_radius, double *records, double *fused, float *tracks,
                               int *counts);

/* ---- compressed-image ingest (cv2.imdecode of the reference's CompressedImage callback, velocity_measurment_node.py:112) ----
 * ofk_jpeg_info: header fields of a JPEG stream (host only; no context, no GPU).  OFK_E_INVALID if the stream is not one the decoder
 * accepts: 8-bit baseline / extended-sequential Huffman, one interleaved scan, gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0, with or
 * without restart intervals.
 * ofk_jpeg_decode_bgr8: decodes `batch` streams of equal size and sampling on the device into bgr [batch][h][w][3] (host; gray
 * streams are replicated over the three channels like cv2.IMREAD_COLOR).  Bit-identical to libjpeg's default decompressor (ISLOW
 * IDCT, fancy upsampling - replication where a chroma plane is one or two samples wide, as libjpeg chooses) - what cv::imdecode returns.  Entropy decoding runs on the GPU too (self-synchronising chunked Huffman
 * decoders); truncated or corrupt entropy data is an error, not a partially grey picture. */
int ofk_jpeg_info(const uint8_t *jpeg, size_t nbytes, int *h, int *w, int *components);
/* ofk_jpeg_destuff (host only; no context, no GPU): the entropy-coded segment of the stream's scan as the device decoders read it -
 * byte stuffing removed (FF00 -> FF, what jdhuff.c's fill_bit_buffer does on the fly behind cv::imdecode), the RSTn markers of a
 * stream with a restart interval taken out and the offsets behind them written to rst[0 .. *nrst) (offsets into `out`), the data
 * ending at the first other marker.  *out_len = bytes written; OFK_E_INVALID if the stream is not decodable (ofk_jpeg_info), if
 * out_capacity is smaller than the stuffed segment or rst_capacity smaller than the number of markers.  The staging of the ingest
 * (ofk_jpeg_stage, ofk_pairs_upload_jpeg ...) runs the same routine; this entry exists so that it can be tested without a GPU. */
int ofk_jpeg_destuff(const uint8_t *jpeg, size_t nbytes, uint8_t *out, size_t out_capacity, size_t *out_len, uint32_t *rst, int rst_capacity, int *nrst);
int ofk_jpeg_decode_bgr8(ofk_ctx *ctx, const uint8_t *const *jpeg, const size_t *nbytes, int batch, uint8_t *bgr);
/* ofk_jpeg_last_iterations: how many synchronisation passes the context's latest decode (any entry that takes JPEG streams) queued
 * behind the first one, in which every chunk decoder starts from its guess.  The host queues them in bursts (seven, then four at a
 * time) and looks at the convergence flags in between, so this is the fixed point's pass number rounded up to the end of its burst.
 * 0 before any decode and for a batch whose streams are a single chunk each (nothing to synchronise).  Read-only: for tests and
 * measurements, it has no effect on any result.  Textured frames take 7 to 15; flat or periodic content one pass per chunk. */
int ofk_jpeg_last_iterations(const ofk_ctx *ctx);

/* ------------------------------------------------- multi-GPU exchange: RCCL over xGMI, no PyTorch
 * The reference has no distributed code; frame pairs (and Monte-Carlo trials) are independent, so each rank (one process per
 * GPU) owns its own pairs and the only exchange is an all-gather of the per-pair velocity records.  librccl.so is bound at run
 * time (dlopen) by the first ofk_comm_* call; a single-GPU program never needs it.
 *   ofk_comm_unique_id     rank 0: n_ids x ncclGetUniqueId -> n_ids x 128 bytes the caller hands to every rank (file, socket ...)
 *   ofk_comm_init          ncclCommInitRank of communicator 0 on the context's device + the gather buffers.  With n_ids > 1 (one
 *                          communicator per free-running slice of ofk_set_streams, so that every slice gathers its own records on its
 *                          own stream; one is enough for correctness) the ranks first agree on the smallest n_ids any of them passed
 *                          (an all-reduce over communicator 0) and then create exactly that many.  ncclCommInitRank is collective, so
 *                          a failure behind that agreement is an error return on the rank that sees it - fatal for the job, never a
 *                          per-rank fallback that would leave the peers waiting inside the call
 *   ofk_comm_add           one more communicator from a 128-byte id; collective (every rank, same order); what ofk_comm_init does
 *                          n_ids - 1 times, exported for callers that negotiate the count themselves (sharding.Comm)
 *   ofk_comm_gather_records  k_records_f32 of the latest ofk_pairs_run + ncclAllGather of [batch][8] f32 {vx,vy,vz,residual,
 *                          n_used,s_min,rank,corners} into the context's receive buffer `slot` (0/1), stream-ordered behind the step
 *                          on the library's own EXCHANGE stream (one slice; with free-running slices: on the slices' streams): no
 *                          host wait, and step k+1's kernels do not queue behind the collective - its solve only waits for the
 *                          export kernel that reads the records
 *   ofk_comm_fetch_records waits for the gather of `slot`, copies [world][batch][8] f32 (rank-major) to host_out
 *   ofk_comm_allreduce_f64 in-place all-reduce of n <= 64 doubles (op 0 sum, 1 max, 2 min), synchronous: barriers, max-over-ranks
 *                          timing, and the Monte-Carlo sweep's per-step (sum v, sum v^2, count) statistics */
int ofk_comm_unique_id(uint8_t *ids, int n_ids);
int ofk_comm_init(ofk_ctx *ctx, const uint8_t *ids, int n_ids, int rank, int world);
int ofk_comm_add(ofk_ctx *ctx, const uint8_t *id);
int ofk_comm_destroy(ofk_ctx *ctx);
int ofk_comm_rank(const ofk_ctx *ctx);
int ofk_comm_world(const ofk_ctx *ctx);
int ofk_comm_gather_records(ofk_ctx *ctx, int batch, int slot);
int ofk_comm_fetch_records(ofk_ctx *ctx, int slot, int batch, float *host_out);
int ofk_comm_allreduce_f64(ofk_ctx *ctx, double *inout, int n, int op);
/* Communicators this rank holds = what the ranks agreed on (1: the step's records travel in one gather behind the last slice). */
int ofk_comm_count(const ofk_ctx *ctx);
/* Non-blocking watchdog query: bit k set = the gather of slice k of `slot` has not completed (0 = done / nothing queued). */
int ofk_comm_pending(ofk_ctx *ctx, int slot);
/* Host-only helper (needs neither a device nor a communicator): receive-buffer order of a step gathered per slice
 * ([slice][world][pairs of the slice][8] f32) -> rank-major [world][batch][8]; what ofk_comm_fetch_records applies. */
int ofk_comm_reorder_records(const float *recv, int world, int batch, int slices, float *out);

/* Number of concurrent slices ofk_pairs_run cuts the batch into (1..8, default 1): each slice runs the whole stage chain on
 * its own HIP stream so that latency-bound stages overlap with streaming ones; results do not depend on it.  With more than
 * one slice, consecutive ofk_pairs_run calls do not join the slices: they free-run, offset by one response kernel, until any
 * other entry point (download, sync, upload, set_sensors ...) needs their results and joins them.  ofk_pairs_export_records_f32
 * and ofk_mark queue behind the slices without joining them.  (The schedule needs 2 x nstreams hardware queues; the HIP
 * runtime's default is 4 in total - GPU_MAX_HW_QUEUES.) */
int ofk_set_streams(ofk_ctx *ctx, int nstreams);
/* ofk_pairs_run scheduling (default on): the HBM-bound gray conversions and pyramids run on an auxiliary stream into one
 * of two pyramid buffer sets, alternating per call, so that they overlap the VALU-bound response kernel and LK — of this call
 * and, when calls are queued back to back, of the previous one.  Results identical. */
int ofk_set_overlap(ofk_ctx *ctx, int on);
/* Launch-geometry knobs for measurements (process-wide; value 0 restores the built-in choice).  Results are bit-identical for
 * every setting - the knobs move strip lengths and pick between kernels that compute the same thing (tests/test_gpu_image_parity.py
 * runs the parity cases under them).  Knobs: "eig_rows" 8..4096 rows per strip of the streaming response kernels; "no_pair" 1 = one
 * column per lane (k_mineig_stream) where k_mineig_pair would run; "no_pyr3" 1 = pyramid level by level; "pyr3_chunks" row chunks per
 * strip of the three-level pyramid pass; "pyr_rows" rows per strip of the one-level pass; "jpeg_chunk" 64/128/256/512/1024 bytes of entropy
 * data per decoder thread; "jpeg_sub" 1..13 = second-level Huffman look-up tables per image + 1 (1: every code longer than 9 bits takes
 * the canonical search - a test hook for that path); "gray_px" 16/32/64 = the BGR -> gray conversion as one-wave workgroups of that many pixels per thread (an
 * experiment of DESIGN.md section 8: slower in the pipeline).  (Rounds 1-2 read OFK_* environment variables in the launch code instead.) */
int ofk_set_tuning(const char *knob, int value);
int ofk_get_tuning(const char *knob, int *value);
/* Completion marks (slots 0..7): ofk_mark records one behind everything queued so far on every slice, ofk_mark_wait
 * blocks the host until it has been reached (returns at once for a slot never marked).  They let a caller hand step k's
 * records to another library (an RCCL gather) while step k+1 is already queued, without draining the stream. */
int ofk_mark(ofk_ctx *ctx, int slot);
int ofk_mark_wait(ofk_ctx *ctx, int slot);

/* Per-stage HIP-event timing on the context's stream. */
#define OFK_STAGE_GRAY    0
#define OFK_STAGE_PYR     1
#define OFK_STAGE_EIG     2
#define OFK_STAGE_NMS     3
#define OFK_STAGE_SELECT  4
#define OFK_STAGE_LK      5
#define OFK_STAGE_SOLVE   6
#define OFK_N_STAGES      7
int ofk_profile_enable(ofk_ctx *ctx, int stage_mask);   /* bit s set: bracket stage s with hipEvents in ofk_pairs_run */
/* Sums the events recorded since the last call (synchronises the stream). ms_total and launches have OFK_N_STAGES entries. */
int ofk_profile_read(ofk_ctx *ctx, double *ms_total, int *launches);

/* Inspection: the resident pyramid slab of one image — frame set 0 (previous frames) or 1 (next frames) of the latest
 * ofk_pairs_run / ofk_pairs_upload batch, or pyramid slot 0/1 of the stream loop — copied to the host: level 0 (the gray image
 * cvtColor would return, of_module.py:86) at offset 0, level l at the offset ofk_pyramid_u8 reports (256-byte aligned levels,
 * tight rows), `bytes` bytes from the start of the slab.  Synchronises every stream of the context. */
int ofk_resident_pyramid(ofk_ctx *ctx, int frame_set, int image, uint8_t *out, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* OFK_H */
