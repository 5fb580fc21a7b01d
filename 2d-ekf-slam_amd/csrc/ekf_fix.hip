// ekf_fix.hip -- absolute observations as joint updates (ekf_update_fixes) and the read-only score of such a list (ekf_fix_compat).
// The third client of the fusion machinery of ekf_fuse.hip: the rows of H are rows of the identity.  Entry k of a round is one slot,
// two columns of W, by its kind (MatchScratch::ids carries `what`):
//   EKF_FIX_POSITION   rows e_0, e_1               columns P[:, 0], P[:, 1]            d = (x_R - z_0, y_R - z_1)
//   EKF_FIX_HEADING    row e_2 and an inert row    columns P[:, 2], 0                  d = (wrap(phi - z_0), 0)
//   landmark i         rows e_3+2i, e_4+2i         columns P[:, 3 + 2i], P[:, 4 + 2i]  d = L_i - z
//   S = H W + blockdiag(R_k) = U^T U,   V = W U^-1,   y = U^-T d,   x -= V y,   P -= V V^T.
// No trigonometry and no linearisation: the result depends on how a list is cut into rounds by rounding alone.
// The inert row of a heading entry keeps the two-columns-per-slot shape of the machinery: its row and column of S are 0, its
// diagonal entry exactly 1 and its d 0, so its pivot is 1, its row of U the unit row, its y and its column of V exact zeros --
// k_fuse_apply, k_fuse_finish and the dense pass over set 0 run unchanged.  z[1] and R[1..3] of a heading entry are not read.
//
// Not on the hot path: once per call and round on a settled handle, all streams idle.  Included by ekf_api.hip behind ekf_match.hip
// (MATCH_PIVOT_TOL, match_round_count) and ekf_fuse.hip, whose header says what the machinery takes from a client and what it
// gives back.  This client's own, per round of at most dv.maxp entries of every filter:
//   k_fix_factor  every column's state row; A = [S | d | W_R^T] straight from P_RR, the R rows and the blocks (i_k, i_l); the pivot
//                 rule of k_match_factor
//   k_fix_gather  W's landmark rows, one thread per (landmark, entry) of the filters that take part: from the R rows or fuse_block
// The factor runs BEFORE the gather, and ekf_fix_compat is k_fix_factor alone with apply = 0, as in ekf_match.hip.

#define FIX_ROW_NONE (-1)  // the inert row of a heading entry

// the state row (0..2 robot, 3 + 2 i + e landmark i) that component e of an entry of kind `what` observes
__device__ __forceinline__ int fix_state_row(int what, int e) {
    if (what == EKF_FIX_POSITION) return e;
    if (what == EKF_FIX_HEADING) return e ? FIX_ROW_NONE : 2;
    return 3 + 2 * what + e;
}

// One workgroup per filter.  A = [S | d | W_R^T] as in k_fuse_factor.
__global__ __launch_bounds__(256) void k_fix_factor(EkfDev dv, FuseScratch fs, MatchScratch ms, int buf, int round, int rs, int apply, int b_off) {
    __shared__ double A[FUSE_MAX_COLS][FUSE_LD];
    __shared__ double sFloor[FUSE_MAX_COLS];
    __shared__ int sWhat[EKF_MAX_PENDING];
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
            const int k = tid, what = ms.ids[z0 + k];
            sWhat[k] = what;
            double d0, d1 = 0.0;
            if (what == EKF_FIX_HEADING) {
                d0 = x[2] - ms.z[2 * (z0 + k)];
                d0 -= 6.283185307179586 * floor((d0 + 3.141592653589793) / 6.283185307179586);  // (nees_sample's wrap)
            } else {
                d0 = x[fix_state_row(what, 0)] - ms.z[2 * (z0 + k)], d1 = x[fix_state_row(what, 1)] - ms.z[2 * (z0 + k) + 1];
            }
            A[2 * k][M] = d0, A[2 * k + 1][M] = d1;
        }
        __syncthreads();
        {
            const double *bm = filt_Bm(dv, buf, b);
            const double *Dx = filt_D(dv, b);
            for (int idx = tid; idx < m * m; idx += 256) {
                const int k = idx / m, l = idx - k * m;
                if (k > l) continue;  // (the upper triangle is all the factorisation reads)
                const int wk = sWhat[k], wl = sWhat[l];
                double pb[4];  // P[row(k, e), row(l, f)] at 2 e + f
                if (wk >= 0 && wl >= 0) {
                    fuse_block(dv, bm, Dx, wk, wl, pb);
                } else {
#pragma unroll
                    for (int e = 0; e < 2; e++)
#pragma unroll
                        for (int f = 0; f < 2; f++) {
                            const int ra = fix_state_row(wk, e), rc = fix_state_row(wl, f);
                            // (a robot row holds the whole state row; a landmark row against a robot column: its transpose)
                            pb[2 * e + f] = ra < 0 || rc < 0 ? 0.0 : ra < 3 ? filt_R(dv, b, ra)[rc] : filt_R(dv, b, rc)[ra];
                        }
                }
                if (k == l) {
                    const double *Rk = ms.Rm + 4 * (z0 + k);
                    if (wk == EKF_FIX_HEADING) {
                        pb[0] += Rk[0], pb[1] = 0.0, pb[2] = 0.0, pb[3] = 1.0;
                    } else {
#pragma unroll
                        for (int e = 0; e < 2; e++)
#pragma unroll
                            for (int f = 0; f < 2; f++) pb[2 * e + f] += Rk[2 * f + e];
                    }
                }
#pragma unroll
                for (int e = 0; e < 2; e++)
#pragma unroll
                    for (int f = 0; f < 2; f++) A[2 * k + e][2 * l + f] = pb[2 * e + f];
            }
            for (int idx = tid; idx < 3 * M; idx += 256) {
                const int r = idx / M, a = idx - r * M;
                const int ra = fix_state_row(sWhat[a >> 1], a & 1);
                A[a][M + 1 + r] = ra < 0 ? 0.0 : filt_R(dv, b, r)[ra];
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

// grid (landmarks / 256, entries of the round, filters); behind k_fix_factor, which has accepted fs.m_round[b] entries.
// Thread (l, k): the rows of landmark l in column pair k of W -- P_lR from the R rows (coalesced over l) for a robot entry, the
// block (l, i_k) from its one home (fuse_block) for a landmark entry.
__global__ __launch_bounds__(256) void k_fix_gather(EkfDev dv, FuseScratch fs, MatchScratch ms, int buf, int round, int b_off) {
    const int b = b_off + blockIdx.z;
    const int k = blockIdx.y;
    if (k >= fs.m_round[b]) return;
    const int n = dv.n_lm[b];
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n) return;
    const int what = ms.ids[(size_t)b * ms.zcap + (size_t)round * dv.maxp + k];
    double w[4];  // element (row e of the landmark, column f of the pair) at 2 e + f
    if (what >= 0) {
        fuse_block(dv, filt_Bm(dv, buf, b), filt_D(dv, b), l, what, w);
    } else {
#pragma unroll
        for (int e = 0; e < 2; e++)
#pragma unroll
            for (int f = 0; f < 2; f++) {
                const int rc = fix_state_row(what, f);
                w[2 * e + f] = rc < 0 ? 0.0 : filt_R(dv, b, rc)[3 + 2 * l + e];
            }
    }
    fuse_store_w(dv, b, l, k, w);
}
