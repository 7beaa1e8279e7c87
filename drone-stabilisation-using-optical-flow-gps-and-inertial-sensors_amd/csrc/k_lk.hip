// k_lk.hip — pyramidal Lucas-Kanade (cv2.calcOpticalFlowPyrLK semantics).  gfx950.
//   k_lk15q   the pipeline's kernel: 15 x 15 window, FOUR points per wave (a 16-lane DPP row per point) — see its own header below;
//   k_lk15    windows <= 15 on levels too small or too oddly sized for k_lk15q: one wave per point, lane = (row, 4-pixel segment);
//   k_lk<W>   windows up to 21 / 31: one wave per point, generic.
//   k_lk_light<W>  the lighting-insensitive tracker of ofk_set_lk_light (at the end of this file): k_lk's structure at every window.
// Common to all three: a 64-thread workgroup (= one wave) tracks its point(s) through all pyramid levels, coarse to fine:
//   * the (win+3)^2 neighbourhood of the previous-frame level is staged into LDS, the Scharr derivatives of its
//     (win+1)^2 core are computed there (never materialised in HBM), and each lane keeps its <= NPL window
//     pixels (I, Ix, Iy as int16) in registers;
//   * a (win+1+2M)^2 region of the next-frame level is staged into LDS once per level and re-staged only when the
//     window walks out of it, so Newton iterations touch LDS only;
//   * the 2x2 normal matrix and the mismatch vector are exact integer sums reduced across the wave with
//     shuffles (order-independent), converted to f32 once; the 2x2 solve is f32 with a fixed operation order.
// Parity target: bit-identical to oracle/image_oracle.c:orc_lk_pyr; the flagged variants (seeded start, min-eigenvalue error) to
// that function with the two additions include/ofk.h states.  The kernel bodies are k_lk_generic.inc, k_lk15.inc, k_lk15q.inc.
#include "ofk_internal.h"
#include <float.h>

#define LK_M 8                                   // margin of the staged next-frame region (pixels each side)

__device__ __forceinline__ int reflect101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}
__device__ __forceinline__ int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// cvRound of a value in [0, 2^22): adding 1.5 * 2^23 leaves the integer, rounded half to even by the addition itself, in the low
// mantissa bits — one full-rate f32 add and one integer subtract instead of v_rndne_f32 + v_cvt_i32_f32 (4 clocks each).
__device__ __forceinline__ int rn_small(float x) { return __float_as_int(x + 12582912.f) - 0x4B400000; }

__device__ __forceinline__ void lk_weights(float a, float b, int &w00, int &w01, int &w10, int &w11)
{
    // fl(fl((1-a)(1-b)) * 2^14) = fl((1-a) * ((1-b) * 2^14)): scaling by a power of two commutes with rounding
    const float a1 = 1.f - a, b1 = (1.f - b) * 16384.f, b0 = b * 16384.f;
    w00 = rn_small(a1 * b1);
    w01 = rn_small(a * b1);
    w10 = rn_small(a1 * b0);
    w11 = 16384 - w00 - w01 - w10;
}

// Variants (ofk.h: OFK_LK_USE_INITIAL_FLOW, OFK_LK_GET_MIN_EIGENVALS).  Every kernel body lives in a file of its own (k_lk_generic.inc,
// k_lk15.inc, k_lk15q.inc) that reads a compile-time constant FLAGS and is included twice: by the plain __global__ symbol with
// FLAGS = 0 - the same translation unit text as before the flags existed, hence the same code, registers and LDS - and by a
// kernel template <int FLAGS> for the flagged variants (k_lk_f, k_lk15_f, k_lk15q_f).  A forced-inline device function template was
// tried first: it moved k_lk15q's instruction mix and made k_lk15 spill three registers at its 64-register budget.
// LK_SEED: the search starts, at the top level, at the position `next_pts` holds on entry (cv2's in/out nextPts) instead of at the
// point itself - a flagged kernel therefore reads the array it writes, and its next_pts is not __restrict__.  LK_EIG: err is the
// level-0 minEig (before the threshold test, whatever the status becomes; 0 when level 0 was skipped) and the L1 residual pass is
// not run; positions and status do not change.
#define LK_SEED OFK_LK_USE_INITIAL_FLOW
#define LK_EIG OFK_LK_GET_MIN_EIGENVALS


template <int WMAX>
__global__ __launch_bounds__(64) void k_lk(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ next,
                                           size_t pyr_stride, ofk_levels lv, const float *__restrict__ prev_pts,
                                           const int *__restrict__ counts, int pts_stride, int win, int max_count,
                                           double eps2, double min_eig_thr, float *__restrict__ next_pts,
                                           uint8_t *__restrict__ status, float *__restrict__ err)
{
    constexpr int FLAGS = 0;
#include "k_lk_generic.inc"
}
// flagged variants: k_lk_f<WMAX, FLAGS>
template <int WMAX, int FLAGS>
__global__ __launch_bounds__(64) void k_lk_f(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ next,
                                             size_t pyr_stride, ofk_levels lv, const float *__restrict__ prev_pts,
                                             const int *__restrict__ counts, int pts_stride, int win, int max_count,
                                             double eps2, double min_eig_thr, float *next_pts,
                                             uint8_t *__restrict__ status, float *__restrict__ err)
{
#include "k_lk_generic.inc"
}


// ================================================================================================
// Fast path, win <= 15: lane = (window row, 4-pixel segment).
//   * staging: all global loads of a level (prev neighbourhood + next region) are issued before the first wait;
//     interior regions come in as aligned dwords re-aligned with v_alignbyte and land in LDS with 16-byte stores;
//   * every tap read is a pair of aligned dwords (ds_read2_b32) + v_alignbyte: 2 LDS reads per lane per iteration;
//   * the Scharr derivatives of the lane's own 2x5 taps are computed from its 4x7 neighbourhood in registers;
//   * reductions: 4 DPP adds inside each 16-lane row (int32 is exact: 16 lanes x 4 px x 8160 x 4080 < 2^31),
//     4 v_readlane, int64 scalar adds — no LDS traffic, no ds_bpermute.
// compiler-level ordering of LDS accesses inside the single wave of a workgroup (see the staging code of k_lk15)
#define LDS_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#define LKF_IP 24                                  // pitch of the staged prev neighbourhood (18 x 18 used)
#define LKF_JW 32                                  // staged next region: 32 x 32 = win + 1 + 2*LK_M at win 15
#define LKF_JP 40                                  // its LDS pitch: 10 banks per row, so the 16 rows a wave reads together hit 16 different bank groups (pitch 32: 4-way conflicts)

__device__ __forceinline__ int row_sum16(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);      // quad_perm(1,0,3,2)
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);      // quad_perm(2,3,0,1)
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);     // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);     // row_mirror
    return v;
}
__device__ __forceinline__ long long wave_sum_rows(int v)
{
    v = row_sum16(v);
    return (long long)__builtin_amdgcn_readlane(v, 0) + (long long)__builtin_amdgcn_readlane(v, 16) +
           (long long)__builtin_amdgcn_readlane(v, 32) + (long long)__builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ float wave_sum_rows_scaled(int v)
{
    v = row_sum16(v);
    // the four row sums are added as 64-bit integers on the scalar unit (they sit in SGPRs after v_readlane); the int64 is
    // below 2^33, so its f64 image and the scaling are exact and one rounding to f32 remains — as in the oracle
    const long long S = ((long long)__builtin_amdgcn_readlane(v, 0) + (long long)__builtin_amdgcn_readlane(v, 16)) +
                        ((long long)__builtin_amdgcn_readlane(v, 32) + (long long)__builtin_amdgcn_readlane(v, 48));
    // Nearly every sum fits 32 bits (the mismatch sums always do in practice): v_cvt_f32_i32 rounds to nearest even exactly as
    // f64 -> f32 does, and the scaling is a power of two, so one conversion + one multiply replace ten half-rate f64
    // instructions.  S is wave-uniform: the test and the branch run on the scalar unit.
    const int lo = (int)S, hi = (int)(S >> 32);
    int sx;                                                      // sign extension of lo, hidden from the optimiser: it would otherwise
    asm("s_ashr_i32 %0, %1, 31" : "=s"(sx) : "s"(lo));           // fold the test back into a 64-bit range check on the VALU
    if (__builtin_expect(hi == sx, 1)) return (float)lo * 0x1p-20f;
    return (float)((double)S * 0x1p-20);
}

// 5 consecutive bytes starting at byte offset `off` of an LDS byte array (4-byte aligned base)
__device__ __forceinline__ void lds_read5(const uint8_t *base, int off, int t[5])
{
    const unsigned *p = reinterpret_cast<const unsigned *>(base + (off & ~3));
    const unsigned d0 = p[0], d1 = p[1];
    const unsigned sh = (unsigned)off & 3u;
    const unsigned v = __builtin_amdgcn_alignbyte(d1, d0, sh);                 // bytes off .. off+3
    t[0] = v & 255; t[1] = (v >> 8) & 255; t[2] = (v >> 16) & 255; t[3] = v >> 24; t[4] = (d1 >> (8 * sh)) & 255;
}
// 7 consecutive bytes starting at `off`
__device__ __forceinline__ void lds_read7(const uint8_t *base, int off, int t[7])
{
    const unsigned *p = reinterpret_cast<const unsigned *>(base + (off & ~3));
    const unsigned d0 = p[0], d1 = p[1], d2 = p[2];
    const unsigned sh = (unsigned)off & 3u;
    const unsigned lo = __builtin_amdgcn_alignbyte(d1, d0, sh), hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
    t[0] = lo & 255; t[1] = (lo >> 8) & 255; t[2] = (lo >> 16) & 255; t[3] = lo >> 24;
    t[4] = hi & 255; t[5] = (hi >> 8) & 255; t[6] = (hi >> 16) & 255;
}

// Packed 16-bit arithmetic of k_lk15.  Pixels, Scharr sums (<= 16 * 255) and the 14-bit interpolation weights all fit 16 bits,
// so two adjacent columns travel in one register: v_perm expands byte pairs (b_k, b_k+1) to u16 pairs, v_pk_* instructions run
// the separable Scharr on two columns at once, and ONE v_dot2_i32_i16 evaluates a row of the bilinear interpolation
// (a*w0 + b*w1 + acc) — every sum is an exact integer, so the results are those of the scalar formulation bit for bit.
typedef short lk_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ lk_s2 lk_as_s2(unsigned v) { return __builtin_bit_cast(lk_s2, v); }
__device__ __forceinline__ unsigned lk_as_u(lk_s2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ int lk_dot2(unsigned a, unsigned w, int acc) { return __builtin_amdgcn_sdot2(lk_as_s2(a), lk_as_s2(w), acc, false); }
#define LK_PAIR_SEL(k) ((unsigned)(k) | 0x0c00u | ((unsigned)((k) + 1) << 16) | 0x0c000000u)   /* v_perm selector: (byte k, 0, byte k+1, 0) */


__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_lk15(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ next,
                                             size_t pyr_stride, ofk_levels lv, const float *__restrict__ prev_pts,
                                             const int *__restrict__ counts, int pts_stride, int win, int max_count,
                                             double eps2, float eps2_lo, float eps2_hi, double min_eig_thr,
                                             float *__restrict__ next_pts, uint8_t *__restrict__ status, float *__restrict__ err)
{
    constexpr int FLAGS = 0;
#include "k_lk15.inc"
}
template <int FLAGS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_lk15_f(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ next,
                                             size_t pyr_stride, ofk_levels lv, const float *__restrict__ prev_pts,
                                             const int *__restrict__ counts, int pts_stride, int win, int max_count,
                                             double eps2, float eps2_lo, float eps2_hi, double min_eig_thr,
                                             float *next_pts, uint8_t *__restrict__ status, float *__restrict__ err)
{
#include "k_lk15.inc"
}

// ================================================================================================
// k_lk15q — win == 15, FOUR points per wave: lane = (point g = lane / 16, window row r = lane % 16).
//
// k_lk15 spends most of its issue slots on work that is the same for all 64 lanes of a point: interpolation weights, the 2x2
// solve, convergence tests, 12 cross-lane instructions per window sum.  Here a 16-lane DPP row owns a point and a lane owns one
// window row of 15 pixels, so that per-point work is shared by four points, a window sum is 4 DPP adds that leave the total in
// every lane of the row (no v_readlane, no scalar round trip), and the Scharr pass runs on full rows: vertical pass first on
// 9 packed column pairs, the horizontal pass is then one packed subtract (dx) or one v_alignbit + 3 packed ops (dy) per pair.
//   * staging: LDS keeps RAW aligned dwords of each staged row (prev: 18 rows x 6 dwords, next: 32 rows x 9 dwords per point);
//     the byte offset of a row's first pixel goes into the v_perm selectors that expand byte pairs, so nothing is re-aligned.
//     Columns outside the image: image widths are multiples of 4, so an aligned dword is wholly inside or wholly outside; an
//     outside dword is ONE v_perm of two inside dwords (reflect-101 reverses bytes), loaded from the mirrored address.
//   * a lane interpolates its derivative row with both weight rows; the half that belongs to the window row above travels there
//     inside the add (v_add_u32_dpp row_shl:1).
//   * the mismatch sums use b = sum(J * Ixy) - sum(I * Ixy): the second term is a per-lane constant of the level; (Ix, Iy) sit
//     packed in one register per pixel and feed v_mad_i32_i16 (op_sel picks the half).
//   * exactness: a lane's 15 products and a quad's 60 fit int32 always; a whole window may not (|sum| < 2^33).  With
//     A11, A22 < 3e8 Cauchy-Schwarz bounds every partial sum of diff * Ix below 2^31 and the plain 32-bit DPP tree is exact;
//     windows above that (full-contrast noise) reduce the 16-bit halves of the lane sums separately.  A11, A22 < 2^32 always
//     (225 * 4080^2) and reduce as unsigned; A12 fits int32 when max(A11, A22) < 2^31, else it takes the split path too.
// The four points of a wave iterate until the last one has converged; finished rows idle.  Results are those of k_lk15 bit for
// bit (integer sums are order-free, the float operations and their order are the same).
#define LKQ_IP 28                                  // LDS pitch of a staged prev row: 6 dwords + 1 (odd dword pitch: no bank conflicts between rows)
#define LKQ_JP 36                                  // LDS pitch of a staged next row: 9 dwords
#define LKQ_ISZ (18 * LKQ_IP)
#define LKQ_JSZ (32 * LKQ_JP)
#define LKQ_SAFE_LIM 300000000u                    // 8160 * sqrt(225 * A) < 2^31  <=>  A < 3.078e8

__device__ __forceinline__ int lkq_reflect(int i, int n)               // one reflection: -n < i < 2n - 1
{
    i = max(i, -i);
    return i >= n ? 2 * (n - 1) - i : i;
}
__device__ __forceinline__ int lkq_floor_i(float x)
{
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));               // floor + convert in one instruction
    return r;
}
// a.lo * w.lo + a.hi * w.hi + c with the rounding constant c in an SGPR: the VOP2 form the compiler picks (v_dot2c) accumulates in
// place and needs a v_mov of the constant first
__device__ __forceinline__ int lkq_dot2_k(unsigned a, unsigned w, int c)
{
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(w), "s"(c));
    return d;
}
__device__ __forceinline__ int lkq_mad_lo(int a, unsigned packed, int acc)     // acc + a.lo16 * packed.lo16
{
    int d;
    asm("v_mad_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(packed), "v"(acc));
    return d;
}
__device__ __forceinline__ int lkq_mad_hi(int a, unsigned packed, int acc)     // acc + a.lo16 * packed.hi16
{
    int d;
    asm("v_mad_i32_i16 %0, %1, %2, %3 op_sel:[0,1,0,0]" : "=v"(d) : "v"(a), "v"(packed), "v"(acc));
    return d;
}
// sum over the 16 lanes of a DPP row, total in every lane
__device__ __forceinline__ int lkq_row_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);      // quad_perm(1,0,3,2)
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);      // quad_perm(2,3,0,1)
    v += __builtin_amdgcn_update_dpp(0, v, 0x124, 0xF, 0xF, true);     // row_ror:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, true);     // row_ror:8
    return v;
}
// exact sum of 16 int32 lane values as f32(sum * 2^-20): halves reduced separately (|sum of halves| < 2^21)
__device__ __forceinline__ float lkq_row_sum_split(int v)
{
    const int lo = lkq_row_sum(v & 0xffff), hi = lkq_row_sum(v >> 16);
    return (float)((double)(((long long)hi << 16) + lo) * 0x1p-20);
}
// Staging of one image row into LDS as ND raw aligned dwords from column A (multiple of 4, any sign), reflect-101 columns.
// The loads always come from inside the row: the strip of ND dwords at Sb = clamp(A, 0, lw - 4 ND).  Interior rows (Sb == A)
// store dword j at slot j.  A row over a border stores dword j at slot j + (Sb - A) / 4 when that is inside the staged row, and
// fills the outside slots with mirrored dwords: the dword at virtual column X < 0 is bytes n[-X], n[-X-1], n[-X-2], n[-X-3] — one
// v_perm of strip dwords j = -X/4 and j-1 — and X >= lw likewise from the strip at the right edge.  Slot positions are per-lane LDS
// addresses, so no register is indexed by a lane-varying amount; writes that fall outside go to a dump slot.
template <int ND>
__device__ __forceinline__ void lkq_load_row(const uint8_t *rowp, int lw, int A, unsigned (&d)[ND])
{
    const unsigned *g = reinterpret_cast<const unsigned *>(rowp + min(max(A, 0), lw - 4 * ND));
#pragma unroll
    for (int i = 0; i < ND; ++i) d[i] = g[i];
}
template <int ND>
__device__ __forceinline__ void lkq_store_row(unsigned *o, unsigned *dump, int lw, int A, bool border, const unsigned (&d)[ND])
{
    if (!border) {                                                      // wave-uniform: no lane of the wave is over a border
#pragma unroll
        for (int i = 0; i < ND; ++i) o[i] = d[i];
        return;
    }
    const bool left = A < 0, right = A + 4 * ND > lw;
    const int dpos = min(max(A, 0), lw - 4 * ND) - A;                   // byte position of strip dword 0 in the staged row
    const unsigned msel = left ? 0x01020304u : 0x03040506u;
    const int mbase = left ? -A : right ? lw + 4 * (ND - 1) - A : -1;   // mirrored dword of strip pair (j, j-1) sits at mbase - 4 j
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        const int pos = dpos + 4 * j;
        *((unsigned)pos < 4u * ND ? o + (pos >> 2) : dump) = d[j];
        if (j > 0) {
            const int mpos = mbase - 4 * j;
            *((unsigned)mpos < 4u * ND ? o + (mpos >> 2) : dump) = __builtin_amdgcn_perm(d[j], d[j - 1], msel);
        }
    }
}

// 120 VGPRs (amdgpu_num_vgpr counts register PAIRS of the unified file: 60): four waves per SIMD leave 32 registers, i.e. room for one
// 32-register gray wave beside them - the compiler's own allocation after the pixel-pair packing is 124, which takes that room away
#define OFK_LKQ_ATTR __attribute__((amdgpu_num_vgpr(60)))

__global__ __launch_bounds__(64) OFK_LKQ_ATTR void k_lk15q(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ next, size_t pyr_stride,
                                              ofk_levels lv, const float *__restrict__ prev_pts, const int *__restrict__ counts,
                                              int pts_stride, int max_count, double eps2, float eps2_lo, float eps2_hi,
                                              double min_eig_thr, float *__restrict__ next_pts, uint8_t *__restrict__ status,
                                              float *__restrict__ err)
{
    constexpr int FLAGS = 0;
#include "k_lk15q.inc"
}
// The flagged variants: 128 VGPRs, which still is four waves per SIMD.  The seeded ones spill three registers when held to the plain
// kernel's 120 (that bound only buys room for a gray wave beside LK, see above); the compiler's own allocation fits.
template <int FLAGS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(64))) void k_lk15q_f(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ next, size_t pyr_stride,
                                              ofk_levels lv, const float *__restrict__ prev_pts, const int *__restrict__ counts,
                                              int pts_stride, int max_count, double eps2, float eps2_lo, float eps2_hi,
                                              double min_eig_thr, float *next_pts, uint8_t *__restrict__ status,
                                              float *__restrict__ err)
{
#include "k_lk15q.inc"
}


// The one routing ladder, by window and level geometry.  FLAGS == 0 launches the plain symbols, not *_f<0> instantiations (see "Variants"
// above: the plain kernels are translation-unit text of their own); __restrict__ is no part of a function's type, so a plain kernel
// and its flagged variants share one pointer type.
template <int FLAGS>
static void launch_lk_flagged(hipStream_t s, bool quad, const uint8_t *prev, const uint8_t *next, size_t pyr_stride, const ofk_levels &lv,
                              const float *prev_pts, const int *counts, int pts_stride, int win, int max_count, double eps2,
                              double min_eig_thr, float *next_pts, uint8_t *status, float *err, int batch)
{
    decltype(&k_lk15q) k15q;
    decltype(&k_lk15) k15;
    decltype(&k_lk<21>) k21, k31;
    if constexpr (FLAGS == 0) { k15q = k_lk15q; k15 = k_lk15; k21 = k_lk<21>; k31 = k_lk<31>; }
    else { k15q = k_lk15q_f<FLAGS>; k15 = k_lk15_f<FLAGS>; k21 = k_lk_f<21, FLAGS>; k31 = k_lk_f<31, FLAGS>; }
    const dim3 grid(pts_stride, batch);
    const float lo = (float)(eps2 * (1.0 - 1e-5)), hi = (float)(eps2 * (1.0 + 1e-5));
    if (quad)
        hipLaunchKernelGGL(k15q, dim3((pts_stride + 3) / 4, batch), dim3(64), 0, s, prev, next, pyr_stride, lv, prev_pts, counts, pts_stride,
                           max_count, eps2, lo, hi, min_eig_thr, next_pts, status, err);
    else if (win <= 15)
        hipLaunchKernelGGL(k15, grid, dim3(64), 0, s, prev, next, pyr_stride, lv, prev_pts, counts, pts_stride, win, max_count, eps2, lo, hi,
                           min_eig_thr, next_pts, status, err);
    else
        hipLaunchKernelGGL(win <= 21 ? k21 : k31, grid, dim3(64), 0, s, prev, next, pyr_stride, lv, prev_pts, counts, pts_stride, win, max_count,
                           eps2, min_eig_thr, next_pts, status, err);
}

// flags: OFK_LK_USE_INITIAL_FLOW (next_pts holds the start positions on entry) | OFK_LK_GET_MIN_EIGENVALS
void ofk_launch_lk(hipStream_t s, const uint8_t *prev, const uint8_t *next, size_t pyr_stride, const ofk_levels &lv,
                   const float *prev_pts, const int *counts, int pts_stride, int win, int max_count, double eps,
                   double min_eig_thr, float *next_pts, uint8_t *status, float *err, int batch, int flags)
{
    if (max_count < 0) max_count = 0;
    if (max_count > 100) max_count = 100;
    if (eps < 0) eps = 0;
    if (eps > 10) eps = 10;
    // four points per wave when the window is the reference's 15 x 15 and every level allows dword rows with ONE reflection
    // (staged columns reach 27 past a border, staged rows 23, and the 36-byte strip of a row has to fit: levels of at least 40 x 32)
    bool quad = win == 15 && (pyr_stride & 3) == 0;
    for (int l = 0; l <= lv.n; ++l) quad = quad && (lv.w[l] & 3) == 0 && lv.w[l] >= 40 && lv.h[l] >= 32 && (lv.off[l] & 3) == 0;
#define LK_ROUTE(F) \
    launch_lk_flagged<F>(s, quad, prev, next, pyr_stride, lv, prev_pts, counts, pts_stride, win, max_count, eps * eps, min_eig_thr, next_pts, status, err, batch)
    switch (flags & (LK_SEED | LK_EIG)) {
    case LK_SEED: return LK_ROUTE(LK_SEED);
    case LK_EIG: return LK_ROUTE(LK_EIG);
    case LK_SEED | LK_EIG: return LK_ROUTE(LK_SEED | LK_EIG);
    default: return LK_ROUTE(0);
    }
#undef LK_ROUTE
}

// ================================================================================================
// k_lk_light — the lighting-insensitive tracker (ofk.h: ofk_lk_light): per-window gain and bias taken out of the mismatch vector
// and of the residual.  One wave per point at every window (k_lk's structure); the body is k_lk_light.inc.  light_mode
// (OFK_LIGHT_BIAS / _GAIN) and the clamp [gain_lo, gain_hi] are wave-uniform kernel arguments.  The kernels above are not touched
// by it: ofk_launch_lk_light does its own routing and is only called with the setting on.
template <int WMAX, int FLAGS>
__global__ __launch_bounds__(64) void k_lk_light(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ next,
                                                 size_t pyr_stride, ofk_levels lv, const float *__restrict__ prev_pts,
                                                 const int *__restrict__ counts, int pts_stride, int win, int max_count,
                                                 double eps2, double min_eig_thr, int light_mode, double gain_lo, double gain_hi,
                                                 float *next_pts, uint8_t *__restrict__ status, float *__restrict__ err)
{
#include "k_lk_light.inc"
}

template <int FLAGS>
static void launch_lk_light_flagged(hipStream_t s, const uint8_t *prev, const uint8_t *next, size_t pyr_stride, const ofk_levels &lv,
                                    const float *prev_pts, const int *counts, int pts_stride, int win, int max_count, double eps2,
                                    double min_eig_thr, int mode, double gain_lo, double gain_hi, float *next_pts, uint8_t *status,
                                    float *err, int batch)
{
    auto k = win <= 15 ? k_lk_light<15, FLAGS> : win <= 21 ? k_lk_light<21, FLAGS> : k_lk_light<31, FLAGS>;
    hipLaunchKernelGGL(k, dim3(pts_stride, batch), dim3(64), 0, s, prev, next, pyr_stride, lv, prev_pts, counts, pts_stride, win, max_count,
                       eps2, min_eig_thr, mode, gain_lo, gain_hi, next_pts, status, err);
}

// ofk_launch_lk with the setting on (light.mode is OFK_LIGHT_BIAS or _GAIN and light.gain_max has passed the setter's check)
void ofk_launch_lk_light(hipStream_t s, const uint8_t *prev, const uint8_t *next, size_t pyr_stride, const ofk_levels &lv,
                         const float *prev_pts, const int *counts, int pts_stride, int win, int max_count, double eps,
                         double min_eig_thr, float *next_pts, uint8_t *status, float *err, int batch, int flags, const ofk_lk_light &light)
{
    if (max_count < 0) max_count = 0;
    if (max_count > 100) max_count = 100;
    if (eps < 0) eps = 0;
    if (eps > 10) eps = 10;
    const double gain_lo = 1.0 / light.gain_max;                 // formed once, here: the kernels and the reference clamp to the same two doubles
#define LK_ROUTE(F) \
    launch_lk_light_flagged<F>(s, prev, next, pyr_stride, lv, prev_pts, counts, pts_stride, win, max_count, eps * eps, min_eig_thr, light.mode, \
                               gain_lo, light.gain_max, next_pts, status, err, batch)
    switch (flags & (LK_SEED | LK_EIG)) {
    case LK_SEED: return LK_ROUTE(LK_SEED);
    case LK_EIG: return LK_ROUTE(LK_EIG);
    case LK_SEED | LK_EIG: return LK_ROUTE(LK_SEED | LK_EIG);
    default: return LK_ROUTE(0);
    }
#undef LK_ROUTE
}
