// k_lstsq.inc — the least-squares path the estimation kernels share: the eleven sums of the 3N x 3 problem per point, their block
// reduction in the order every record depends on (wave butterfly, then (s0 + s1) + (s2 + s3)), the cyclic Jacobi on the 3 x 3 normal
// matrix and the solve with lstsq's rank rule.  Included by k_estimate.hip and by k_tracks.hip (k_track_depth.inc's map solve).
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

// All eleven sums at once: the wave reductions are independent shuffle chains the scheduler interleaves, and ONE LDS exchange
// (two barriers) replaces eleven; the order of the additions is block_sum's, so the results are the same bit for bit.
__device__ void acc_block_sum(Acc &a)
{
    __shared__ double s_part[4][11];
    double v[11] = {a.m00, a.m01, a.m02, a.m11, a.m12, a.m22, a.g0, a.g1, a.g2, a.bb, a.cnt};
#pragma unroll
    for (int k = 0; k < 11; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 11; ++k) s_part[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 11; ++k) v[k] = (s_part[0][k] + s_part[1][k]) + (s_part[2][k] + s_part[3][k]);
    a.m00 = v[0]; a.m01 = v[1]; a.m02 = v[2]; a.m11 = v[3]; a.m12 = v[4]; a.m22 = v[5]; a.g0 = v[6]; a.g1 = v[7]; a.g2 = v[8]; a.bb = v[9]; a.cnt = v[10];
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

// Solve from accumulated sums.  out8 = v[3], (residual filled later), rank, s[3].  Returns rank.
// fin: whether M, g and the eigenvalues are all finite; where they are not the problem is not solved (ofk.h, "non-finite sums"):
// rank 0, v = s = 0, and the caller leaves the residual at 0.  Finite sums take the path they always took.
__device__ int solve_from_acc(const Acc &a, double *v, double *s3, bool &fin)
{
    double A[3][3] = {{a.m00, a.m01, a.m02}, {a.m01, a.m11, a.m12}, {a.m02, a.m12, a.m22}};
    double lam[3], V[3][3];
    jacobi3(A, lam, V);
    // x - x is 0 for a finite x and NaN otherwise, and a NaN in a sum stays: one compare covers the twelve values
    fin = (a.m00 - a.m00) + (a.m01 - a.m01) + (a.m02 - a.m02) + (a.m11 - a.m11) + (a.m12 - a.m12) + (a.m22 - a.m22) + (a.g0 - a.g0) +
          (a.g1 - a.g1) + (a.g2 - a.g2) + (lam[0] - lam[0]) + (lam[1] - lam[1]) + (lam[2] - lam[2]) == 0.0;
    if (!fin) { v[0] = v[1] = v[2] = 0.0; s3[0] = s3[1] = s3[2] = 0.0; return 0; }
    const double rows = 3.0 * a.cnt;
    // lstsq's cut is s_k <= eps*max(M,N)*s_max; on the squared spectrum the resolvable floor is eps*lambda_max,
    // so singular-value ratios below sqrt(eps*rows) count as zero (DESIGN.md, "rank").
    const double tol = lam[0] * 2.220446049250313e-16 * (rows > 3.0 ? rows : 3.0);
    int rank = 0;
    v[0] = v[1] = v[2] = 0.0;
    for (int k = 0; k < 3; ++k) {
        s3[k] = lam[k] > 0.0 ? sqrt(lam[k]) : 0.0;
        if (lam[k] > tol && lam[k] > 0.0) {
            const double c = (V[0][k] * a.g0 + V[1][k] * a.g1 + V[2][k] * a.g2) / lam[k];
            v[0] += c * V[0][k]; v[1] += c * V[1][k]; v[2] += c * V[2][k];
            ++rank;
        }
    }
    return rank;
}
