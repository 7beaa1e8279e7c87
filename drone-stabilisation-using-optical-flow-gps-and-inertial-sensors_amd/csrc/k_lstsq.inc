// k_lstsq.inc — the least-squares path the estimation kernels share: the eleven sums of the 3N x 3 problem per point, their block
// reduction in the order every record depends on (wave butterfly, then (s0 + s1) + (s2 + s3): block_sums, for any number of sums),
// the cyclic Jacobi on the 3 x 3 normal matrix, the symmetric-3x3 helpers behind it (sym3_from6, eig_inverse3, joint_inverse,
// eig_solve3, rank_cut, all_finite_sum) and the solve with lstsq's rank rule.  Included by k_estimate.hip and by k_tracks.hip.
#pragma once
struct Acc { double m00, m01, m02, m11, m12, m22, g0, g1, g2, bb, cnt; };

__device__ __forceinline__ void acc_zero(Acc &a) { a.m00 = a.m01 = a.m02 = a.m11 = a.m12 = a.m22 = a.g0 = a.g1 = a.g2 = a.bb = a.cnt = 0.0; }

// p = (x,y,1); c = p x q  (= [p]x q)
__device__ __forceinline__ void cross_p(double x, double y, double q0, double q1, double q2, double &c0, double &c1, double &c2)
{
    c0 = y * q2 - q1; c1 = q0 - x * q2; c2 = x * q1 - y * q0;
}

__device__ __forceinline__ void acc_point(Acc &a, double x, double y, double q0, double q1, double q2, double sA, double sB)
{
    double c0, c1, c2, t0, t1, t2;
    cross_p(x, y, q0, q1, q2, c0, c1, c2);            // X q
    cross_p(x, y, c0, c1, c2, t0, t1, t2);            // X X q = -X^T X q
    const double pp = x * x + y * y + 1.0, sa2 = sA * sA, sab = sA * sB;
    a.m00 += sa2 * (pp - x * x); a.m01 += sa2 * (-x * y); a.m02 += sa2 * (-x);
    a.m11 += sa2 * (pp - y * y); a.m12 += sa2 * (-y);     a.m22 += sa2 * (pp - 1.0);
    a.g0 -= sab * t0; a.g1 -= sab * t1; a.g2 -= sab * t2;
    a.bb += sB * sB * (c0 * c0 + c1 * c1 + c2 * c2);
    a.cnt += 1.0;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// K sums at once, the one exchange every record's bits depend on: the wave reductions are independent shuffle chains the scheduler
// interleaves, and ONE LDS round (two barriers) replaces K; each sum is added in block_sum's order, so its bits do not depend on how
// many travel with it.  v: K values in, their block sums out, in every thread.  part: four rows of the caller's LDS.
template <int K, int S>
__device__ __forceinline__ void block_sums(double *v, double (*part)[S])
{
    static_assert(S >= K, "a row of the partials holds the K sums");
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) part[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
}

// Sum `v` over the 256 threads of the block; result valid in every thread.  s_red: >= 4 doubles.
__device__ __forceinline__ double block_sum(double v, double *s_red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__device__ __forceinline__ double block_minmax(double v, bool want_max, double *s_red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o);
        v = want_max ? fmax(v, u) : fmin(v, u);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double a = want_max ? fmax(s_red[0], s_red[1]) : fmin(s_red[0], s_red[1]);
    const double b = want_max ? fmax(s_red[2], s_red[3]) : fmin(s_red[2], s_red[3]);
    return want_max ? fmax(a, b) : fmin(a, b);
}

__device__ __forceinline__ void acc_pack(const Acc &a, double *v)
{
    v[0] = a.m00; v[1] = a.m01; v[2] = a.m02; v[3] = a.m11; v[4] = a.m12; v[5] = a.m22; v[6] = a.g0; v[7] = a.g1; v[8] = a.g2; v[9] = a.bb; v[10] = a.cnt;
}
__device__ __forceinline__ void acc_unpack(Acc &a, const double *v)
{
    a.m00 = v[0]; a.m01 = v[1]; a.m02 = v[2]; a.m11 = v[3]; a.m12 = v[4]; a.m22 = v[5]; a.g0 = v[6]; a.g1 = v[7]; a.g2 = v[8]; a.bb = v[9]; a.cnt = v[10];
}

// All eleven sums of an Acc, through LDS of its own.
__device__ void acc_block_sum(Acc &a)
{
    __shared__ double s_part[4][11];
    double v[11];
    acc_pack(a, v); block_sums<11, 11>(v, s_part); acc_unpack(a, v);
}

// Cyclic Jacobi on a symmetric 3x3; eigenvalues descending in lam[], eigenvectors in columns of V.
__device__ void jacobi3(double A[3][3], double lam[3], double V[3][3])
{
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        // converged: the off-diagonal mass is below 1e-20 of the diagonal (its effect on the eigenvalues, off^2 / gap, is far below
        // one ulp); waiting for an exact zero costs sweeps that change nothing — sometimes all 32
        if (off <= 1e-20 * (fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]))) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
                for (int k = 0; k < 3; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
                for (int k = 0; k < 3; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
            }
    }
    int o[3] = {0, 1, 2};
    double d[3] = {A[0][0], A[1][1], A[2][2]};
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2 - i; ++j) if (d[o[j]] < d[o[j + 1]]) { const int t = o[j]; o[j] = o[j + 1]; o[j + 1] = t; }
    double Vs[3][3];
    for (int k = 0; k < 3; ++k) { lam[k] = d[o[k]]; for (int i = 0; i < 3; ++i) Vs[i][k] = V[i][o[k]]; }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = Vs[i][j];
}

// The symmetric 3 x 3 around jacobi3.  Each helper states its order of operations: the build contracts and reassociates nothing, so a
// site that wrote the same order by hand gets the same bits from the helper.
// The upper triangle of six sums (00 01 02 11 12 22) as a full matrix.
__device__ __forceinline__ void sym3_from6(const double *s, double A[3][3])
{
    A[0][0] = s[0]; A[0][1] = A[1][0] = s[1]; A[0][2] = A[2][0] = s[2]; A[1][1] = s[3]; A[1][2] = A[2][1] = s[4]; A[2][2] = s[5];
}
__device__ __forceinline__ void sym3_from6(const Acc &a, double A[3][3])
{
    const double s[6] = {a.m00, a.m01, a.m02, a.m11, a.m12, a.m22};
    sym3_from6(s, A);
}

// x - x is 0 for a finite x and NaN otherwise, and a NaN in a sum stays: one compare covers the n values
__device__ __forceinline__ bool all_finite_sum(const double *s, int n)
{
    double f = 0.0;
    for (int k = 0; k < n; ++k) f += s[k] - s[k];
    return f == 0.0;
}

// lstsq's cut is s_k <= eps*max(M,N)*s_max; on the squared spectrum the resolvable floor is eps*lambda_max, so singular-value ratios
// below sqrt(eps*rows) count as zero (DESIGN.md, "rank").  The product is formed left to right.
__device__ __forceinline__ double rank_cut(double lam0, double rows) { return lam0 * 2.220446049250313e-16 * (rows > 3.0 ? rows : 3.0); }

// V diag(1 / lam) V^T as (t0 + t1) + t2, t_k = V[i][k] V[j][k] / lam[k]: the full-rank inverse.
__device__ __forceinline__ void eig_inverse3(const double lam[3], const double V[3][3], double Ai[3][3])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Ai[i][j] = (V[i][0] * V[j][0] / lam[0] + V[i][1] * V[j][1] / lam[1]) + V[i][2] * V[j][2] / lam[2];
}

// The same over the first `take` eigenvalues as ((0.0 + t0) + t1) + ...  Not eig_inverse3 with a count: where every term is -0.0 this
// sum is +0.0 and eig_inverse3's is -0.0, and the joint and bias records carry the entries as they are.
__device__ __forceinline__ void joint_inverse(const double lam[3], const double V[3][3], int take, double Ai[3][3])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double t = 0.0;
            for (int k = 0; k < take; ++k) t += V[i][k] * V[j][k] / lam[k];
            Ai[i][j] = t;
        }
}

// x = sum_k V[:,k] ((V[0][k] g0 + V[1][k] g1 + V[2][k] g2) / lam[k]), from 0.0 and in the order of k, over the k that keep[] names
// (NULL: all three).
__device__ __forceinline__ void eig_solve3(const double lam[3], const double V[3][3], const double *g, const bool *keep, double *x)
{
    x[0] = x[1] = x[2] = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (keep && !keep[k]) continue;
        const double c = (V[0][k] * g[0] + V[1][k] * g[1] + V[2][k] * g[2]) / lam[k];
        x[0] += c * V[0][k]; x[1] += c * V[1][k]; x[2] += c * V[2][k];
    }
}

// Solve from accumulated sums.  out8 = v[3], (residual filled later), rank, s[3].  Returns rank.  lam, V: the decomposition of M, for
// the callers that go on to M^-1.
// fin: whether M, g and the eigenvalues are all finite; where they are not the problem is not solved (ofk.h, "non-finite sums"):
// rank 0, v = s = 0, and the caller leaves the residual at 0.  Finite sums take the path they always took.
__device__ int solve_from_acc(const Acc &a, double *v, double *s3, bool &fin, double lam[3], double V[3][3])
{
    double A[3][3]; sym3_from6(a, A);
    const double g[3] = {a.g0, a.g1, a.g2};
    fin = all_finite_sum(&A[0][0], 9) && all_finite_sum(g, 3);   // before jacobi3 rotates A
    jacobi3(A, lam, V);
    fin = fin && all_finite_sum(lam, 3);
    if (!fin) { v[0] = v[1] = v[2] = 0.0; s3[0] = s3[1] = s3[2] = 0.0; return 0; }
    const double tol = rank_cut(lam[0], 3.0 * a.cnt);
    bool keep[3];
    int rank = 0;
    for (int k = 0; k < 3; ++k) {
        s3[k] = lam[k] > 0.0 ? sqrt(lam[k]) : 0.0;
        keep[k] = lam[k] > tol && lam[k] > 0.0;
        rank += keep[k] ? 1 : 0;
    }
    eig_solve3(lam, V, g, keep, v);
    return rank;
}

__device__ int solve_from_acc(const Acc &a, double *v, double *s3, bool &fin)
{
    double lam[3], V[3][3];
    return solve_from_acc(a, v, s3, fin, lam, V);
}
