// ekf_match_iter.hip -- the iterated (Gauss-Newton) matched update (ekf_update_matched_iter): a round of ekf_match.hip relinearised
// until its step vanishes.  Entry state (x^, P); linearisation points xi_0 = x^, xi_1, ..., held for the pose and the round's
// landmarks alone -- nothing else enters H or d.  Iteration i:
//   H_i, h(xi_i) as k_match_factor's, at xi_i (cos and sin of xi_i[2] from the device library, once per iteration),
//   d_0 = h(x^) - z by k_match_factor's very expression;  i > 0: d_i = (h(xi_i) - z) + H_i (x^ - xi_i),
//   W_i = P H_i^T,   S_i = H_i W_i + blockdiag(R_k) = U_i^T U_i  (MATCH_PIVOT_TOL in every iteration),   y_i = U_i^-T d_i,
//   xi_i+1 = x^ - W_i S_i^-1 d_i on the touched components,   step_i = max |xi_i+1 - xi_i| over them,
// and the round stops behind iteration i when step_i <= tol or i + 1 == max_iter: fuse_publish of THAT factorisation, so that
// k_match_gather, k_fuse_apply, k_fuse_finish and the dense pass run unchanged and leave x = x^ - V_i y_i, P = P - V_i V_i^T.  A
// pivot refused in any iteration refuses the round (and, through fs.done, the later ones).  With max_iter = 1 every value that
// leaves the kernel is k_match_factor's, bit for bit: iteration 0 takes no correction term.
//
// Included by ekf_api.hip behind ekf_match.hip (MATCH_PIVOT_TOL, match_round_count; the machinery of ekf_fuse.hip).  One kernel, one
// workgroup per filter:
//   k_match_factor_iter  once per round: x^ of the touched components, the R rows at the round's landmarks and ALL m x m blocks
//                        (i_k, i_l) of P into LDS (fuse_block; 32 KB at 32 entries, beside A's 35 KB: they do not change over the
//                        iterations, and the landmark step needs the lower triangle too).  Per iteration: the table and
//                        A = [S | d | W_R^T] at xi_i from LDS, fuse_cholesky<true>; S^-1 d by one back substitution in wave 0
//                        (lane a keeps row a, the solved entry broadcast by a shuffle); the robot part of xi_i+1 from the extra
//                        columns as x^_R - V_R y -- k_fuse_finish's sum --, the landmark part from the rows L_ik of W_i, formed
//                        again from the LDS blocks, times S^-1 d; the step by thread 0.
// Behind the last iteration: fuse_publish; the table for k_match_gather (H and cos / sin at the LAST linearisation point); the
// factorisations and the last step of every measurement of the round (IterScratch); fuse_prefix_d2 on y_0, saved behind iteration
// 0 and put back into A's column M once fuse_publish has read y_i from it -- the prior's compatibility, ekf_joint_compat's bits.
// One writer per value, every sum in a fixed order, no atomics: the same bits on every call and in the batch form.

#include "ekf_map_scratch.h"  // IterScratch

#define ITER_TOUCHED (3 + FUSE_MAX_COLS)  // the pose, then the two coordinates of measurement k's landmark at 3 + 2 k

__global__ __launch_bounds__(256) void k_match_factor_iter(EkfDev dv, FuseScratch fs, MatchScratch ms, IterScratch is, int buf, int round, int rs, int max_iter, double tol,
                                                           int b_off) {
    __shared__ double A[FUSE_MAX_COLS][FUSE_LD];
    __shared__ double sPB[EKF_MAX_PENDING][EKF_MAX_PENDING][4];  // the block (i_k, i_l) of P
    __shared__ double sFloor[FUSE_MAX_COLS];
    __shared__ double sH[EKF_MAX_PENDING][6];   // H_R,k, element (f, r) at 3 f + r
    __shared__ double sPR[EKF_MAX_PENDING][6];  // P_R,ik, element (r, g) at 2 r + g
    __shared__ double sWR[EKF_MAX_PENDING][6];  // W's robot rows of column pair k, element (r, f) at 2 r + f
    __shared__ double sXh[ITER_TOUCHED];        // x^
    __shared__ double sXi[ITER_TOUCHED];        // xi_i
    __shared__ double sNx[ITER_TOUCHED];        // xi_i+1
    __shared__ double sQ[FUSE_MAX_COLS];        // S^-1 d
    __shared__ double sY0[FUSE_MAX_COLS];       // y_0
    __shared__ double sCS[2];
    __shared__ double sStep;
    __shared__ int sId[EKF_MAX_PENDING];
    const int b = b_off + blockIdx.x;
    const int tid = threadIdx.x;
    const bool stopped = fs.done[2 * b + 1];
    const int m = stopped ? 0 : match_round_count(ms, b, round, rs);
    const int M = 2 * m, NC = M + 4;
    const size_t z0 = (size_t)b * ms.zcap + (size_t)round * rs;
    int bad = 0, iters = 0;
    double step = __builtin_nan("");
    if (m > 0) {
        const double *x = filt_x(dv, b);
        double prr[9];  // P_RR, thread k's copy
        if (tid < m) {
            const int k = tid, i = ms.ids[z0 + k];
            sId[k] = i;
            sXh[3 + 2 * k] = sXi[3 + 2 * k] = x[3 + 2 * i], sXh[4 + 2 * k] = sXi[4 + 2 * k] = x[4 + 2 * i];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double *pr = filt_R(dv, b, r);
                sPR[k][2 * r] = pr[3 + 2 * i], sPR[k][2 * r + 1] = pr[4 + 2 * i];
                prr[3 * r] = pr[0], prr[3 * r + 1] = pr[1], prr[3 * r + 2] = pr[2];
            }
        }
        if (tid < 3) sXh[tid] = sXi[tid] = x[tid];
        __syncthreads();
        {
            const double *bm = filt_Bm(dv, buf, b);
            const double *Dx = filt_D(dv, b);
            for (int idx = tid; idx < m * m; idx += 256) {
                const int k = idx / m, l = idx - k * m;
                double pb[4];
                fuse_block(dv, bm, Dx, sId[k], sId[l], pb);
#pragma unroll
                for (int q = 0; q < 4; q++) sPB[k][l][q] = pb[q];
            }
        }
        for (int it = 0;; it++) {
            if (tid < m) {
                const int k = tid;
                const double c = cos(sXi[2]), s = sin(sXi[2]);
                const double dpx = sXi[3 + 2 * k] - sXi[0], dpy = sXi[4 + 2 * k] - sXi[1];
                double h[6];
                h[0] = -c, h[1] = -s, h[2] = c * dpy - s * dpx;
                h[3] = s, h[4] = -c, h[5] = -(s * dpy) - c * dpx;
                const double dv0 = (c * dpx + s * dpy) - ms.z[2 * (z0 + k)], dv1 = (c * dpy - s * dpx) - ms.z[2 * (z0 + k) + 1];
                const double Cm[4] = {c, -s, s, c};  // C, element (g, f) at 2 g + f
#pragma unroll
                for (int r = 0; r < 3; r++) {
#pragma unroll
                    for (int f = 0; f < 2; f++)
                        sWR[k][2 * r + f] = (((prr[3 * r] * h[3 * f] + prr[3 * r + 1] * h[3 * f + 1]) + prr[3 * r + 2] * h[3 * f + 2]) + sPR[k][2 * r] * Cm[f]) +
                                            sPR[k][2 * r + 1] * Cm[2 + f];
                }
#pragma unroll
                for (int q = 0; q < 6; q++) sH[k][q] = h[q];
                if (k == 0) sCS[0] = c, sCS[1] = s;
                A[2 * k][M] = dv0, A[2 * k + 1][M] = dv1;
            }
            __syncthreads();
            if (it > 0) {
                // d_i = (h(xi_i) - z) + H_i (x^ - xi_i), row f of measurement k: the robot's three columns, then the landmark's two.
                // A phase of its own, behind a barrier, on what the table left in LDS: the table above is k_match_factor's text with
                // k_match_factor's uses of every value, so that the compiler contracts it to the same multiply-adds and iteration 0
                // leaves k_match_factor's bits.
                if (tid < M) {
                    const int k = tid >> 1, f = tid & 1;
                    const double c = sCS[0], s = sCS[1];
                    const double e0 = sXh[0] - sXi[0], e1 = sXh[1] - sXi[1], e2 = sXh[2] - sXi[2];
                    const double g0 = sXh[3 + 2 * k] - sXi[3 + 2 * k], g1 = sXh[4 + 2 * k] - sXi[4 + 2 * k];
                    const double c0 = f ? -s : c, c1 = f ? c : s;  // column f of C
                    A[tid][M] = A[tid][M] + ((((sH[k][3 * f] * e0 + sH[k][3 * f + 1] * e1) + sH[k][3 * f + 2] * e2) + c0 * g0) + c1 * g1);
                }
                __syncthreads();
            }
            {
                const double c = sCS[0], s = sCS[1];
                const double Cm[4] = {c, -s, s, c};
                for (int idx = tid; idx < m * m; idx += 256) {
                    const int k = idx / m, l = idx - k * m;
                    if (k > l) continue;  // (the upper triangle is all the factorisation reads)
                    const double *pb = sPB[k][l];
                    // T = rows (L_ik) of column pair l of W;  S block = H_R,k W_R,l + C^T T  (+ R_k on the diagonal)
                    double T[4];
#pragma unroll
                    for (int g = 0; g < 2; g++)
#pragma unroll
                        for (int f = 0; f < 2; f++)
                            T[2 * g + f] = (((sPR[k][g] * sH[l][3 * f] + sPR[k][2 + g] * sH[l][3 * f + 1]) + sPR[k][4 + g] * sH[l][3 * f + 2]) + pb[2 * g] * Cm[f]) +
                                           pb[2 * g + 1] * Cm[2 + f];
                    const double *Rk = ms.Rm + 4 * (z0 + k);
#pragma unroll
                    for (int e = 0; e < 2; e++)
#pragma unroll
                        for (int f = 0; f < 2; f++) {
                            double v = (((sH[k][3 * e] * sWR[l][f] + sH[k][3 * e + 1] * sWR[l][2 + f]) + sH[k][3 * e + 2] * sWR[l][4 + f]) + Cm[e] * T[f]) + Cm[2 + e] * T[2 + f];
                            if (k == l) v += Rk[2 * f + e];
                            A[2 * k + e][2 * l + f] = v;
                        }
                }
                for (int idx = tid; idx < 3 * M; idx += 256) {
                    const int r = idx / M, a = idx - r * M;
                    A[a][M + 1 + r] = sWR[a >> 1][2 * r + (a & 1)];
                }
            }
            __syncthreads();
            if (tid < M) sFloor[tid] = MATCH_PIVOT_TOL * A[tid][tid];
            __syncthreads();
            bad = fuse_cholesky<true>(A, M, NC, tid, sFloor);
            iters = it + 1;
            if (bad) break;
            // (fuse_cholesky's last step ends in a barrier: U, y and V_R^T are in A for every thread)
            if (it == 0 && tid < M) sY0[tid] = A[tid][M];
            if (tid < 64) {  // S^-1 d = U^-1 y: lane a keeps y_a less U[a][c] q_c of the entries c > a solved so far
                double yv = tid < M ? A[tid][M] : 0.0;
                for (int k = M - 1; k >= 0; k--) {
                    const double qk = __shfl(yv, k) / A[k][k];
                    if (tid == k) yv = qk;
                    else if (tid < k) yv = yv - A[tid][k] * qk;
                }
                if (tid < M) sQ[tid] = yv;
            }
            __syncthreads();
            if (tid < M) {  // row g of landmark i_k:  x^ - sum over l of the row of T(k, l) times (S^-1 d)_l, l ascending
                const int k = tid >> 1, g = tid & 1;
                const double c = sCS[0], s = sCS[1];
                const double Cm[4] = {c, -s, s, c};
                double acc = sXh[3 + tid];
                for (int l = 0; l < m; l++) {
                    const double *pb = sPB[k][l];
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        const double T = (((sPR[k][g] * sH[l][3 * f] + sPR[k][2 + g] * sH[l][3 * f + 1]) + sPR[k][4 + g] * sH[l][3 * f + 2]) + pb[2 * g] * Cm[f]) +
                                         pb[2 * g + 1] * Cm[2 + f];
                        acc = acc - T * sQ[2 * l + f];
                    }
                }
                sNx[3 + tid] = acc;
            } else if (tid < M + 3) {  // the pose: x^_R - V_R y, as k_fuse_finish sums it
                const int r = tid - M;
                double acc = sXh[r];
                for (int a = 0; a < M; a++) acc = acc - A[a][M + 1 + r] * A[a][M];
                sNx[r] = acc;
            }
            __syncthreads();
            if (tid == 0) {
                double big = 0.0;
                for (int q = 0; q < M + 3; q++) {
                    const double v = fabs(sNx[q] - sXi[q]);
                    big = v > big || v != v ? v : big;  // (a NaN stays)
                }
                sStep = big;
            }
            __syncthreads();
            step = sStep;
            if (step <= tol || it + 1 == max_iter) break;
            if (tid < M + 3) sXi[tid] = sNx[tid];
            __syncthreads();
        }
        if (tid < m) {
            const size_t at = (size_t)b * is.zcap + (size_t)round * rs + tid;
            is.iters[at] = iters, is.step[at] = step;
            double *t = ms.tab + ((size_t)b * EKF_MAX_PENDING + tid) * MATCH_TAB;
#pragma unroll
            for (int q = 0; q < 6; q++) t[q] = sH[tid][q];
            t[6] = sCS[0], t[7] = sCS[1];
        }
    }
    fuse_publish(dv, fs, A, b, m, bad, tid);
    if (m == 0) return;
    if (iters > 1) {  // column M holds y_i (or what a refused iteration i left of it): y_0 back, once fuse_publish has read it
        __syncthreads();
        if (tid < M) A[tid][M] = sY0[tid];
        __syncthreads();
    }
    if (tid == 0) fuse_prefix_d2(ms.d2 + z0, A, m, iters > 1 ? 0 : bad);
}
