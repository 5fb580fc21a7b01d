// ekf_polar.hip -- landmark measurements in polar form as joint updates (ekf_update_polar) and the read-only score of such a list
// (ekf_polar_compat): range only (UWB, radio or acoustic beacons), bearing only (a camera), or both with the noise in polar
// coordinates (laser, radar).  The fifth client of the fusion machinery of ekf_fuse.hip.  Entry k of a round observes landmark i_k:
//   dx = L_ik.x - x_R,  dy = L_ik.y - y_R,  q = dx^2 + dy^2,  r = sqrt(q),
//   range row:    h = r,                     H_R = [-dx / r, -dy / r,  0],   d = r - z
//   bearing row:  h = atan2(dy, dx) - phi,   H_R = [ dy / q, -dx / q, -1],   d = wrap(h - z)     (wrap: ekf_fix.hip's expression)
//   H_L = -H_R[0:2] for either row, so the round's table is the two H_R rows of a slot alone (6 of MATCH_TAB = 8 doubles);
//   column pair k of W = P[:, 0:3] H_R,k^T + P[:, L_ik] H_L,k^T,   S = H W + blockdiag(R_k) = U^T U,   V = W U^-1,   y = U^-T d,
//   x -= V y,   P -= V V^T,
// every entry of the round linearised at the round's entry state; sqrt() and atan2() are the device library's, taken once per entry
// and round (k_polar_factor).  An entry is one slot, two columns of W, by its kind (MatchScratch::ids carries it above the landmark:
// POLAR_KIND_SHIFT, ekf_device.h; the host's table has the live component of a one-component entry in row 0 of its z and R):
//   EKF_POLAR_BOTH     row 0 range, row 1 bearing
//   EKF_POLAR_RANGE    row 0 range, row 1 inert
//   EKF_POLAR_BEARING  row 0 bearing, row 1 inert
// The inert row is that of a heading entry in ekf_fix.hip: its row and column of S are 0, its diagonal entry exactly 1, its d 0 and
// its column of W 0 -- written as constants, not computed --, so its pivot is 1, its y and its column of V exact zeros, and
// k_fuse_apply, k_fuse_finish and the dense pass over set 0 run unchanged.
// A landmark exactly at the robot's position (q == 0) has no H: 0 / 0 makes its live rows of H NaN, so is its diagonal entry of S,
// and fuse_cholesky<true> refuses a NaN pivot (`!(piv > floor)`) as it refuses a non-positive one -- the rows in front of it are
// final and finite, fuse_publish accepts nothing of the round (fs.m_round = 0: no gather, no apply, no finish), and nothing but the
// scratch has seen the NaN.  A q so small that H overflows gives an infinite pivot against an infinite floor: refused alike.
//
// Not on the hot path: once per call and round on a settled handle, all streams idle.  Included by ekf_api.hip behind ekf_fix.hip.
//   k_polar_factor  the round's table (the H_R rows, d, W's robot rows) from x, the R rows and P_RR; S from the blocks (i_k, i_l)
//                   directly, m (m + 1) / 2 fuse_block reads, as k_match_factor -- the score needs no gather and writes nothing
//   k_polar_gather  W's landmark rows, one thread per (landmark, entry) of the filters that take part
// The factor runs BEFORE the gather, and ekf_polar_compat is k_polar_factor alone with apply = 0, as in ekf_match.hip.

// One workgroup per filter.  A = [S | d | W_R^T] as in k_fuse_factor.
__global__ __launch_bounds__(256) void k_polar_factor(EkfDev dv, FuseScratch fs, MatchScratch ms, int buf, int round, int rs, int apply, int b_off) {
    __shared__ double A[FUSE_MAX_COLS][FUSE_LD];
    __shared__ double sFloor[FUSE_MAX_COLS];
    __shared__ double sH[EKF_MAX_PENDING][6];   // H_R,k, element (f, r) at 3 f + r; an inert row: zeros
    __shared__ double sPR[EKF_MAX_PENDING][6];  // P_R,ik, element (r, g) at 2 r + g
    __shared__ double sWR[EKF_MAX_PENDING][6];  // W's robot rows of column pair k, element (r, f) at 2 r + f
    __shared__ int sId[EKF_MAX_PENDING];
    __shared__ int sBoth[EKF_MAX_PENDING];      // row 1 of the slot is live
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
            const int k = tid, packed = ms.ids[z0 + k];
            const int i = packed & POLAR_ID_MASK, kind = packed >> POLAR_KIND_SHIFT;
            const bool both = kind == EKF_POLAR_BOTH, range0 = (kind & EKF_POLAR_RANGE) != 0;
            const double dx = x[3 + 2 * i] - x[0], dy = x[4 + 2 * i] - x[1];
            const double q = dx * dx + dy * dy, r = sqrt(q);
            const double hr[3] = {-dx / r, -dy / r, 0.0};
            const double hb[3] = {dy / q, -dx / q, -1.0};
            const double bear = atan2(dy, dx) - x[2];
            double h[6];
#pragma unroll
            for (int c = 0; c < 3; c++) h[c] = range0 ? hr[c] : hb[c], h[3 + c] = both ? hb[c] : 0.0;
            double e0 = bear - ms.z[2 * (z0 + k)], e1 = bear - ms.z[2 * (z0 + k) + 1];
            e0 -= 6.283185307179586 * floor((e0 + 3.141592653589793) / 6.283185307179586);  // (k_fix_factor's wrap)
            e1 -= 6.283185307179586 * floor((e1 + 3.141592653589793) / 6.283185307179586);
            const double dv0 = range0 ? r - ms.z[2 * (z0 + k)] : e0, dv1 = both ? e1 : 0.0;
            double pr[6];
#pragma unroll
            for (int rr = 0; rr < 3; rr++) pr[2 * rr] = filt_R(dv, b, rr)[3 + 2 * i], pr[2 * rr + 1] = filt_R(dv, b, rr)[4 + 2 * i];
#pragma unroll
            for (int rr = 0; rr < 3; rr++) {
                const double *prr = filt_R(dv, b, rr);  // P_RR row rr in [0..2]
#pragma unroll
                for (int f = 0; f < 2; f++) {
                    const double w = (((prr[0] * h[3 * f] + prr[1] * h[3 * f + 1]) + prr[2] * h[3 * f + 2]) - pr[2 * rr] * h[3 * f]) - pr[2 * rr + 1] * h[3 * f + 1];
                    sWR[k][2 * rr + f] = f == 0 || both ? w : 0.0;
                }
            }
#pragma unroll
            for (int c = 0; c < 6; c++) sH[k][c] = h[c], sPR[k][c] = pr[c];
            sId[k] = i, sBoth[k] = both;
            A[2 * k][M] = dv0, A[2 * k + 1][M] = dv1;
            if (apply) {
                double *t = ms.tab + ((size_t)b * EKF_MAX_PENDING + k) * MATCH_TAB;
#pragma unroll
                for (int c = 0; c < 6; c++) t[c] = h[c];
            }
        }
        __syncthreads();
        {
            const double *bm = filt_Bm(dv, buf, b);
            const double *Dx = filt_D(dv, b);
            for (int idx = tid; idx < m * m; idx += 256) {
                const int k = idx / m, l = idx - k * m;
                if (k > l) continue;  // (the upper triangle is all the factorisation reads)
                double pb[4];
                fuse_block(dv, bm, Dx, sId[k], sId[l], pb);
                // T = rows (L_ik) of column pair l of W;  S block = H_R,k W_R,l + H_L,k T  (+ R_k on the diagonal)
                double T[4];
#pragma unroll
                for (int g = 0; g < 2; g++)
#pragma unroll
                    for (int f = 0; f < 2; f++)
                        T[2 * g + f] = (((sPR[k][g] * sH[l][3 * f] + sPR[k][2 + g] * sH[l][3 * f + 1]) + sPR[k][4 + g] * sH[l][3 * f + 2]) - pb[2 * g] * sH[l][3 * f]) -
                                       pb[2 * g + 1] * sH[l][3 * f + 1];
                const double *Rk = ms.Rm + 4 * (z0 + k);
#pragma unroll
                for (int e = 0; e < 2; e++)
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        double v = (((sH[k][3 * e] * sWR[l][f] + sH[k][3 * e + 1] * sWR[l][2 + f]) + sH[k][3 * e + 2] * sWR[l][4 + f]) - sH[k][3 * e] * T[f]) -
                                   sH[k][3 * e + 1] * T[2 + f];
                        const bool live = (e == 0 || sBoth[k]) && (f == 0 || sBoth[l]);
                        if (live && k == l) v += Rk[2 * f + e];  // (a one-component entry: the table holds its variance at 0, zeros behind it)
                        A[2 * k + e][2 * l + f] = live ? v : k == l && e == f ? 1.0 : 0.0;
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

// grid (landmarks / 256, entries of the round, filters); behind k_polar_factor, which has accepted fs.m_round[b] entries.
// Thread (l, k): the rows of landmark l in column pair k of W, from P_lR (the R rows, coalesced over l), the block (l, i_k) from its
// one home (fuse_block) and the table; the column of an inert row is the constant 0.
__global__ __launch_bounds__(256) void k_polar_gather(EkfDev dv, FuseScratch fs, MatchScratch ms, int buf, int round, int b_off) {
    const int b = b_off + blockIdx.z;
    const int k = blockIdx.y;
    if (k >= fs.m_round[b]) return;
    const int n = dv.n_lm[b];
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n) return;
    const int packed = ms.ids[(size_t)b * ms.zcap + (size_t)round * dv.maxp + k];
    const int i = packed & POLAR_ID_MASK;
    const bool both = (packed >> POLAR_KIND_SHIFT) == EKF_POLAR_BOTH;
    const double *t = ms.tab + ((size_t)b * EKF_MAX_PENDING + k) * MATCH_TAB;
    double pb[4];
    fuse_block(dv, filt_Bm(dv, buf, b), filt_D(dv, b), l, i, pb);
    double w[4];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const double p0 = filt_R(dv, b, 0)[3 + 2 * l + e], p1 = filt_R(dv, b, 1)[3 + 2 * l + e], p2 = filt_R(dv, b, 2)[3 + 2 * l + e];
#pragma unroll
        for (int f = 0; f < 2; f++) {
            const double v = (((p0 * t[3 * f] + p1 * t[3 * f + 1]) + p2 * t[3 * f + 2]) - pb[2 * e] * t[3 * f]) - pb[2 * e + 1] * t[3 * f + 1];
            w[2 * e + f] = f == 0 || both ? v : 0.0;
        }
    }
    fuse_store_w(dv, b, l, k, w);
}
