// ekf_match.hip -- a scan with caller-given correspondences as one joint update (ekf_update_matched) and the read-only score of such
// a hypothesis (ekf_joint_compat).  The second client of the fusion machinery of ekf_fuse.hip: measurement k of a round observes
// landmark i_k,
//   dp_k = L_ik - p,   H_R,k = [-C^T | -C^T J dp_k],   H_L = C^T,   d_k = C^T dp_k - z_k      (C = Rot(phi), J = [[0, -1], [1, 0]]),
//   column pair k of W = P[:, 0:3] H_R,k^T + P[:, L_ik] C,   S = H W + blockdiag(R_k) = U^T U,   V = W U^-1,   y = U^-T d,
//   x -= V y,   P -= V V^T,
// every measurement of the round linearised at the round's entry state, cos phi and sin phi taken once per round ON THE DEVICE
// (cos() and sin() of the device library on x[2], in k_match_factor).  d is minus the reference's residual (Update.cpp:110), so
// x - V y is the reference's x + K res and k_fuse_apply / k_fuse_finish / the dense pass over set 0 run unchanged.
//
// Not on the hot path: once per call and round on a settled handle, all streams idle.  Included by ekf_api.hip behind ekf_fuse.hip,
// whose header says what the machinery takes from a client and what it gives back (fuse_cholesky, fuse_prefix_d2, fuse_publish,
// fuse_store_w; blocks of P through fuse_block).  This client's own, per round of at most dv.maxp measurements of every filter:
//   k_match_factor  the round's table (H_R,k, C, d_k, W's robot rows) from x, the R rows and P_RR; S from the blocks (i_k, i_l)
//                   directly, m (m + 1) / 2 fuse_block reads -- not from gathered rows, so that the score needs no gather and
//                   writes nothing to the filter; apply != 0: the table for the gather as well
//   k_match_gather  W's landmark rows, one thread per (landmark, measurement) of the filters that take part
// The factor runs BEFORE the gather: a filter whose S is refused gathers nothing.  ekf_joint_compat is k_match_factor alone with
// apply = 0 and a round of up to EKF_MAX_PENDING: the same code, so the same bits of d2 for a hypothesis that fits one round.
//
// A pivot counts as positive when it exceeds MATCH_PIVOT_TOL times its own diagonal entry of S: what is left of an exactly singular
// S after the elimination (the same landmark measured twice with R = 0) is rounding noise of either sign, a few 2^-52 of that entry.

#define MATCH_PIVOT_TOL 0x1p-44
#include "ekf_map_scratch.h"  // MatchScratch, MATCH_TAB

// measurements of filter b in round `round` of rounds of rs
__device__ __forceinline__ int match_round_count(const MatchScratch &ms, int b, int round, int rs) {
    const int m = ms.cnt[b] - round * rs;
    return m < 0 ? 0 : m > rs ? rs : m;
}

// One workgroup per filter.  A = [S | d | W_R^T] as in k_fuse_factor.
__global__ __launch_bounds__(256) void k_match_factor(EkfDev dv, FuseScratch fs, MatchScratch ms, int buf, int round, int rs, int apply, int b_off) {
    __shared__ double A[FUSE_MAX_COLS][FUSE_LD];
    __shared__ double sFloor[FUSE_MAX_COLS];
    __shared__ double sH[EKF_MAX_PENDING][6];   // H_R,k, element (f, r) at 3 f + r
    __shared__ double sPR[EKF_MAX_PENDING][6];  // P_R,ik, element (r, g) at 2 r + g
    __shared__ double sWR[EKF_MAX_PENDING][6];  // W's robot rows of column pair k, element (r, f) at 2 r + f
    __shared__ double sCS[2];
    __shared__ int sId[EKF_MAX_PENDING];
    const int b = b_off + blockIdx.x;
    const int tid = threadIdx.x;
    const bool stopped = apply && fs.done[2 * b + 1];
    const int m = stopped ? 0 : match_round_count(ms, b, round, rs);
    const int M = 2 * m, NC = M + 4;
    const size_t z0 = (size_t)b * ms.zcap + (size_t)round * rs;
    int bad = 0;
    if (m > 0) {
        const double *x = filt_x(dv, b);
        if (tid < m) {
            const int k = tid, i = ms.ids[z0 + k];
            const double c = cos(x[2]), s = sin(x[2]);
            const double dpx = x[3 + 2 * i] - x[0], dpy = x[4 + 2 * i] - x[1];
            double h[6];
            h[0] = -c, h[1] = -s, h[2] = c * dpy - s * dpx;
            h[3] = s, h[4] = -c, h[5] = -(s * dpy) - c * dpx;
            const double dv0 = (c * dpx + s * dpy) - ms.z[2 * (z0 + k)], dv1 = (c * dpy - s * dpx) - ms.z[2 * (z0 + k) + 1];
            double pr[6];
#pragma unroll
            for (int r = 0; r < 3; r++) pr[2 * r] = filt_R(dv, b, r)[3 + 2 * i], pr[2 * r + 1] = filt_R(dv, b, r)[4 + 2 * i];
            const double Cm[4] = {c, -s, s, c};  // C, element (g, f) at 2 g + f
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double *prr = filt_R(dv, b, r);  // P_RR row r in [0..2]
#pragma unroll
                for (int f = 0; f < 2; f++)
                    sWR[k][2 * r + f] = (((prr[0] * h[3 * f] + prr[1] * h[3 * f + 1]) + prr[2] * h[3 * f + 2]) + pr[2 * r] * Cm[f]) + pr[2 * r + 1] * Cm[2 + f];
            }
#pragma unroll
            for (int q = 0; q < 6; q++) sH[k][q] = h[q], sPR[k][q] = pr[q];
            sId[k] = i;
            if (k == 0) sCS[0] = c, sCS[1] = s;
            A[2 * k][M] = dv0, A[2 * k + 1][M] = dv1;
            if (apply) {
                double *t = ms.tab + ((size_t)b * EKF_MAX_PENDING + k) * MATCH_TAB;
#pragma unroll
                for (int q = 0; q < 6; q++) t[q] = h[q];
                t[6] = c, t[7] = s;
            }
        }
        __syncthreads();
        {
            const double *bm = filt_Bm(dv, buf, b);
            const double *Dx = filt_D(dv, b);
            const double c = sCS[0], s = sCS[1];
            const double Cm[4] = {c, -s, s, c};
            for (int idx = tid; idx < m * m; idx += 256) {
                const int k = idx / m, l = idx - k * m;
                if (k > l) continue;  // (the upper triangle is all the factorisation reads)
                double pb[4];
                fuse_block(dv, bm, Dx, sId[k], sId[l], pb);
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
    }
    if (tid == 0 && m > 0) fuse_prefix_d2(ms.d2 + z0, A, m, bad);
    if (!apply) return;
    fuse_publish(dv, fs, A, b, m, bad, tid);
}

// grid (landmarks / 256, measurements of the round, filters); behind k_match_factor, which has accepted fs.m_round[b] measurements.
// Thread (l, k): the rows of landmark l in column pair k of W, from P_lR (the R rows, coalesced over l), the block (l, i_k) from its
// one home (fuse_block: 32-byte pieces with one half used, as in k_fuse_gather) and the table.
__global__ __launch_bounds__(256) void k_match_gather(EkfDev dv, FuseScratch fs, MatchScratch ms, int buf, int round, int b_off) {
    const int b = b_off + blockIdx.z;
    const int k = blockIdx.y;
    if (k >= fs.m_round[b]) return;
    const int n = dv.n_lm[b];
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n) return;
    const int i = ms.ids[(size_t)b * ms.zcap + (size_t)round * dv.maxp + k];
    const double *t = ms.tab + ((size_t)b * EKF_MAX_PENDING + k) * MATCH_TAB;
    const double c = t[6], s = t[7];
    const double Cm[4] = {c, -s, s, c};
    double pb[4];
    fuse_block(dv, filt_Bm(dv, buf, b), filt_D(dv, b), l, i, pb);
    double w[4];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const double p0 = filt_R(dv, b, 0)[3 + 2 * l + e], p1 = filt_R(dv, b, 1)[3 + 2 * l + e], p2 = filt_R(dv, b, 2)[3 + 2 * l + e];
#pragma unroll
        for (int f = 0; f < 2; f++) w[2 * e + f] = (((p0 * t[3 * f] + p1 * t[3 * f + 1]) + p2 * t[3 * f + 2]) + pb[2 * e] * Cm[f]) + pb[2 * e + 1] * Cm[2 + f];
    }
    fuse_store_w(dv, b, l, k, w);
}
