// ekf_fuse.hip -- landmark fusion on the device (ekf_fuse_landmarks): the equality constraint L_i = L_j of m pairs as one update of
// the whole state,  W = P H^T,  S = H W + slack I = U^T U,  V = W U^-1,  y = U^-T d,   x -= V y,  P -= V V^T,
// with the rank-2m correction of P_LL handed to the dense pass as m ordinary slots FA = -V, FB = V of slot set 0.
//
// Not on the hot path: once per call and round, every slot folded in and all streams idle.  Included by ekf_api.hip behind
// ekf_pairs.hip (filt_x / filt_R / filt_D / filt_Bm, item_block, double4_t); where a block of P lives and where a column of a
// round sits in the slot rows is in ekf_device.h (fuse_source, fuse_slot_offset), checked on the CPU by tests/cpp/fuse_map_check.cpp.
//
// A round (at most dv.maxp pairs of every filter of the call), on the chain stream:
//   k_fuse_gather  W's landmark rows into the FA slot rows, one thread per (landmark, pair): the blocks (l, i) and (l, j) from their
//                  one home each -- stored tile (either orientation), D, -- as 32-byte pieces; W's robot rows and d into the scratch
//   k_fuse_factor  one workgroup per filter: S from the W rows at i_k and j_k, Cholesky in LDS with d and W's robot rows as four
//                  extra columns (they come out as y and V's robot rows); decides whether the filter takes part in the round
//   k_fuse_apply   one thread per landmark-space row: V_row = W_row U^-1, 16 columns at a time in registers, U broadcast from LDS; the
//                  slot rows, x, the landmark's block in D and its robot columns in R
//   k_fuse_finish  one thread per filter: P_RR and the pose
//   k_flush_rb     the dense pass over set 0, in place
// Nothing is read after it was overwritten: a row's thread reads its own W row, x, D and R entries and nobody else's; U, y and
// V's robot rows are in the scratch; the pass reads the slot rows alone.  One writer per value, every sum in a fixed order: the
// same bits on every call and in the batch form.
// A filter whose S is not positive definite stops: k_fuse_factor records the pivot, leaves its slots inactive and sizes its pass
// to zero tiles; this round and the later ones return at once for it, and nothing of it but the slot rows (cleared at the end of
// the call) has been written.
//
// The machinery and its clients (fusion here, ekf_match.hip, ekf_match_iter.hip, ekf_fix.hip, ekf_polar.hip).  A client supplies, per round, a factor kernel -- one
// workgroup per filter that fills A = [S | d | W_R^T] in LDS, runs fuse_cholesky and ends in fuse_publish -- and a gather kernel
// that leaves W's landmark rows in the FA slot rows (fuse_store_w), for the entries fuse_publish accepted (fs.m_round) or, in front
// of the factor, for all of them.  It gets back x -= V y and P -= V V^T from k_fuse_apply, k_fuse_finish and the pass, the count
// of applied entries and the refused pivot in fs.done, and from fuse_prefix_d2 the joint distance cut after every entry.  The host
// side of a round is fuse_rounds (ekf_map_api.hip).  A client keeps the rule above -- one writer per value, every sum in a fixed
// order, no atomics -- and so the same bits on every call and in the batch form.

#include "ekf_map_scratch.h"  // FuseScratch, FUSE_MAX_COLS

// pairs of filter b in round `round` (0: none left, or the filter has stopped)
__device__ __forceinline__ int fuse_round_pairs(const EkfDev &dv, const FuseScratch &fs, int b, int round) {
    if (fs.done[2 * b + 1]) return 0;
    const int m = fs.cnt[b] - round * dv.maxp;
    return m < 0 ? 0 : m > dv.maxp ? dv.maxp : m;
}

// the block (landmark l, landmark c) of P as {(0,0), (0,1), (1,0), (1,1)}; F = EkfDev or JoinSrc (ekf_extract.hip reads another handle)
template <typename F>
__device__ __forceinline__ void fuse_block(const F &dv, const double *bm, const double *Dx, int l, int c, double m[4]) {
    const FuseSource s = fuse_source(dv.T, l, c);
    if (s.where == FW_D) {
        const double xy = Dx[dv.dn + s.off];
        m[0] = Dx[s.off], m[1] = xy, m[2] = xy, m[3] = Dx[2 * (size_t)dv.dn + s.off];
        return;
    }
    const int half = (int)(s.off & 1);
    const double *p = bm + (s.off - half);
    double4_t v[2];
    v[0] = *(const double4_t *)p;
    v[1] = *(const double4_t *)(p + 32);
    double t[4];
    t[0] = half ? v[0][1] : v[0][0], t[1] = half ? v[0][3] : v[0][2], t[2] = half ? v[1][1] : v[1][0], t[3] = half ? v[1][3] : v[1][2];
    const bool tr = s.where == FW_BM_T;
    m[0] = t[0], m[1] = tr ? t[2] : t[1], m[2] = tr ? t[1] : t[2], m[3] = t[3];
}

// The rows of landmark l in column pair k of W (w: element (row e, column f) at 2 e + f) into filter b's FA slot rows: the end of
// a list client's gather (k_fuse_gather forms its differences in the stores themselves).
__device__ __forceinline__ void fuse_store_w(const EkfDev &dv, int b, int l, int k, const double w[4]) {
    double *fa = dv.FA + (size_t)b * 2 * dv.f_stride;
    *(double2_t *)(fa + fuse_slot_offset(dv.rows, 2 * l, 2 * k)) = (double2_t){w[0], w[1]};
    *(double2_t *)(fa + fuse_slot_offset(dv.rows, 2 * l + 1, 2 * k)) = (double2_t){w[2], w[3]};
}

// grid (landmarks / 256, pairs of the round, filters)
__global__ __launch_bounds__(256) void k_fuse_gather(EkfDev dv, FuseScratch fs, int buf, int round, int b_off) {
    const int b = b_off + blockIdx.z;
    const int k = blockIdx.y;
    if (k >= fuse_round_pairs(dv, fs, b, round)) return;
    const int n = dv.n_lm[b];
    const int *pr = fs.pairs + ((size_t)b * fs.pcap + (size_t)round * dv.maxp + k) * 2;
    const int i = pr[0], j = pr[1];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid < 8) {  // W's robot rows and d, columns 2k and 2k + 1
        const int r = tid >> 1, f = tid & 1;
        const double *src = r < 3 ? filt_R(dv, b, r) : filt_x(dv, b);
        fs.wr[((size_t)b * 4 + r) * FUSE_MAX_COLS + 2 * k + f] = src[3 + 2 * i + f] - src[3 + 2 * j + f];
    }
    const int l = blockIdx.x * 256 + tid;
    if (l >= n) return;
    const double *bm = filt_Bm(dv, buf, b);
    const double *Dx = filt_D(dv, b);
    double pi[4], pj[4];
    fuse_block(dv, bm, Dx, l, i, pi);
    fuse_block(dv, bm, Dx, l, j, pj);
    double *fa = dv.FA + (size_t)b * 2 * dv.f_stride;
    *(double2_t *)(fa + fuse_slot_offset(dv.rows, 2 * l, 2 * k)) = (double2_t){pi[0] - pj[0], pi[1] - pj[1]};
    *(double2_t *)(fa + fuse_slot_offset(dv.rows, 2 * l + 1, 2 * k)) = (double2_t){pi[2] - pj[2], pi[3] - pj[3]};
}

// One workgroup per filter.  A = [S | d | W_R^T], upper triangle, right-looking: step k scales row k by 1 / sqrt(pivot) and takes
// its outer product off the rows below, the four extra columns with it -- they end as U^-T d = y and U^-T W_R^T = V_R^T.
#define FUSE_LD (FUSE_MAX_COLS + 5)

// The factorisation itself, by the 256 threads of a workgroup on A in LDS (filled, and a barrier behind it): M rows, NC = M + 4
// columns.  Returns 0, or 1 + the index of the first pivot that is not positive (FLOOR: not above floor[k]; ekf_match.hip) -- the
// rows in front of it are final.  The same value in every thread.
template <bool FLOOR>
__device__ __forceinline__ int fuse_cholesky(double (*A)[FUSE_LD], int M, int NC, int tid, const double *floor) {
    for (int k = 0; k < M; k++) {
        const double piv = A[k][k];  // (the same value in every thread: the loop stays uniform)
        if (!(piv > (FLOOR ? floor[k] : 0.0))) return k + 1;
        const double s = sqrt(piv);
        __syncthreads();
        for (int c = k + tid; c < NC; c += 256) A[k][c] = A[k][c] / s;
        __syncthreads();
        for (int idx = tid; idx < (M - 1 - k) * NC; idx += 256) {
            const int a = k + 1 + idx / NC, c = idx % NC;
            if (c >= a) A[a][c] = A[a][c] - A[k][a] * A[k][c];
        }
        __syncthreads();
    }
    return 0;
}

// The end of every client's factor kernel, by the 256 threads of filter b's workgroup behind fuse_cholesky (m entries, `bad` its
// return value): U, y and V's robot rows into the scratch, the slot flags of set 0, the size of the pass, and the progress record
// -- fs.m_round[b] = the entries the rest of the round applies (0: k_fuse_apply, k_fuse_finish and the client's gather return at
// once), fs.done[2 b] += them, fs.done[2 b + 1] = the refused pivot (1 + its index), which stops the filter for the later rounds.
__device__ __forceinline__ void fuse_publish(const EkfDev &dv, const FuseScratch &fs, double (*A)[FUSE_LD], int b, int m, int bad, int tid) {
    const int M = 2 * m;
    const bool ok = m > 0 && !bad;
    if (ok) {
        double *U = fs.U + (size_t)b * FUSE_MAX_COLS * FUSE_MAX_COLS;
        double *wr = fs.wr + (size_t)b * 4 * FUSE_MAX_COLS;
        for (int idx = tid; idx < M * M; idx += 256) {
            const int a = idx / M, c = idx - a * M;
            U[a * FUSE_MAX_COLS + c] = c >= a ? A[a][c] : 0.0;
        }
        for (int idx = tid; idx < 4 * M; idx += 256) {
            const int r = idx / M, a = idx - r * M;
            wr[(size_t)r * FUSE_MAX_COLS + a] = A[a][M + ((r + 1) & 3)];
        }
    }
    if (tid < dv.maxp) dv.slot_active[((size_t)b * 2) * dv.maxp + tid] = ok && tid < m ? 1 : 0;
    if (tid == 0) {
        dv.n_lm_flush[(size_t)b * 2] = ok ? dv.n_lm[b] : 0;  // (0: the pass skips every tile of this filter)
        fs.m_round[b] = ok ? m : 0;
        if (ok) fs.done[2 * b] += m;
        if (bad) fs.done[2 * b + 1] = bad;
    }
}

// The joint distance of a round cut after each of its m entries, by one thread behind fuse_cholesky: d2[k] = the sum of y^2 up to
// and including entry k, every addition in this order; NaN from the refused pivot on.
__device__ __forceinline__ void fuse_prefix_d2(double *d2, double (*A)[FUSE_LD], int m, int bad) {
    const int M = 2 * m;
    double acc = 0.0;
    for (int k = 0; k < m; k++) {
        const bool have = !bad || 2 * k + 1 < bad - 1;
        acc = acc + A[2 * k][M] * A[2 * k][M];
        acc = acc + A[2 * k + 1][M] * A[2 * k + 1][M];
        d2[k] = have ? acc : __builtin_nan("");
    }
}

__global__ __launch_bounds__(256) void k_fuse_factor(EkfDev dv, FuseScratch fs, int round, double slack, int b_off) {
    __shared__ double A[FUSE_MAX_COLS][FUSE_LD];
    const int b = b_off + blockIdx.x;
    const int tid = threadIdx.x;
    const int m = fuse_round_pairs(dv, fs, b, round);
    const int M = 2 * m, NC = M + 4;
    double *wr = fs.wr + (size_t)b * 4 * FUSE_MAX_COLS;
    int bad = 0;
    if (m > 0) {
        const int *pr = fs.pairs + ((size_t)b * fs.pcap + (size_t)round * dv.maxp) * 2;
        const double *fa = dv.FA + (size_t)b * 2 * dv.f_stride;
        for (int idx = tid; idx < M * NC; idx += 256) {
            const int a = idx / NC, c = idx - a * NC;
            double val;
            if (c < M) {
                const int i = pr[2 * (a >> 1)], j = pr[2 * (a >> 1) + 1], e = a & 1;
                val = fa[fuse_slot_offset(dv.rows, 2 * i + e, c)] - fa[fuse_slot_offset(dv.rows, 2 * j + e, c)];
                if (a == c) val += slack;
            } else {
                val = wr[(size_t)((c - M + 3) & 3) * FUSE_MAX_COLS + a];  // column M: d (row 3), then the robot rows
            }
            A[a][c] = val;
        }
        __syncthreads();
        bad = fuse_cholesky<false>(A, M, NC, tid, nullptr);
    }
    fuse_publish(dv, fs, A, b, m, bad, tid);
}

// Thread = landmark-space row ip of filter b_off + blockIdx.y, up to the end of the map's last tile row (rows beyond the map get
// zero slot rows: the pass reads them).  The row is walked in chunks of 16 columns (8 slots), the chunk in registers: first the
// finished columns are taken off it -- they come back from the row's own FB line, which this thread has just stored --, then the
// chunk is solved against its diagonal block of U, stored (FB = V, FA = -V over the W it was read from) and folded into x, D and R.
// (The whole row of 64 columns in registers is what the build's register allocator spills: 1.6 KB of scratch per lane.)
#define FUSE_CH 16
__global__ __launch_bounds__(256) void k_fuse_apply(EkfDev dv, FuseScratch fs, int b_off) {
    __shared__ double sU[FUSE_MAX_COLS][FUSE_MAX_COLS];
    __shared__ double sR[4][FUSE_MAX_COLS];  // V's robot rows, y
    const int b = b_off + blockIdx.y;
    const int m = fs.m_round[b];
    if (m == 0) return;
    const int M = 2 * m;
    const int tid = threadIdx.x;
    {
        const double *U = fs.U + (size_t)b * FUSE_MAX_COLS * FUSE_MAX_COLS;
        const double *wr = fs.wr + (size_t)b * 4 * FUSE_MAX_COLS;
        for (int idx = tid; idx < FUSE_MAX_COLS * FUSE_MAX_COLS; idx += 256) {
            const int k = idx / FUSE_MAX_COLS, c = idx % FUSE_MAX_COLS;
            sU[k][c] = k < M && c < M ? U[idx] : k == c ? 1.0 : 0.0;  // (columns beyond the round: V = 0 / 1)
        }
        for (int idx = tid; idx < 4 * FUSE_MAX_COLS; idx += 256) {
            const int c = idx % FUSE_MAX_COLS;
            sR[idx / FUSE_MAX_COLS][c] = c < M ? wr[idx] : 0.0;
        }
    }
    __syncthreads();
    const int n = dv.n_lm[b];
    const int ip = blockIdx.x * 256 + tid;
    if (ip >= 64 * lm_tiles(n)) return;  // (whole waves)
    const bool live = ip < 2 * n;
    double *fa = dv.FA + (size_t)b * 2 * dv.f_stride, *fb = dv.FB + (size_t)b * 2 * dv.f_stride;
    const int l = ip >> 1, e = ip & 1;
    double *Dx = filt_D(dv, b);
    double *x = filt_x(dv, b);
    double own = 0.0, xy = 0.0, xv = 0.0, rr[3] = {0.0, 0.0, 0.0};
    if (live) {
        own = Dx[(size_t)(2 * e) * dv.dn + l], xy = Dx[dv.dn + l], xv = x[3 + ip];
#pragma unroll
        for (int r = 0; r < 3; r++) rr[r] = filt_R(dv, b, r)[3 + ip];
    }
    for (int c0 = 0; c0 < M; c0 += FUSE_CH) {
        double t[FUSE_CH];
#pragma unroll
        for (int q = 0; q < FUSE_CH / 4; q++) {
            const int col = c0 + 4 * q;
            const bool has = col < M;  // (else the row's first pair once more: no branch, the value is dropped)
            const double4_t w = *(const double4_t *)(fa + pair_offset(dv.rows, ip, has ? col >> 2 : 0));
#pragma unroll
            for (int r = 0; r < 4; r++) t[4 * q + r] = live && col + r < M ? w[r] : 0.0;
        }
        for (int kp = 0; 4 * kp < c0; kp++) {
            const double4_t vk = *(const double4_t *)(fb + pair_offset(dv.rows, ip, kp));
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < FUSE_CH; c++) t[c] = t[c] - vk[r] * sU[4 * kp + r][c0 + c];
        }
#pragma unroll
        for (int k = 0; k < FUSE_CH; k++) {
            t[k] = t[k] / sU[c0 + k][c0 + k];
#pragma unroll
            for (int c = k + 1; c < FUSE_CH; c++) t[c] = t[c] - t[k] * sU[c0 + k][c0 + c];
        }
#pragma unroll
        for (int q = 0; q < FUSE_CH / 4; q++) {
            if (c0 + 4 * q < M) {
                const size_t at = pair_offset(dv.rows, ip, (c0 >> 2) + q);
                *(double4_t *)(fb + at) = (double4_t){t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]};
                *(double4_t *)(fa + at) = (double4_t){-t[4 * q], -t[4 * q + 1], -t[4 * q + 2], -t[4 * q + 3]};
            }
        }
        // The landmark's own block as the dense pass would fold it: one fused multiply-add per column, columns ascending.  The
        // other row of the landmark is the neighbouring lane's.
#pragma unroll
        for (int c = 0; c < FUSE_CH; c++) {
            const double other = __shfl_xor(t[c], 1);
            own = __builtin_fma(-t[c], t[c], own);
            xy = e ? __builtin_fma(-other, t[c], xy) : __builtin_fma(-t[c], other, xy);
            xv = xv - t[c] * sR[3][c0 + c];
#pragma unroll
            for (int r = 0; r < 3; r++) rr[r] = rr[r] - t[c] * sR[r][c0 + c];
        }
    }
    if (!live) return;
    Dx[(size_t)(2 * e) * dv.dn + l] = own;
    if (!e) Dx[dv.dn + l] = xy;
    x[3 + ip] = xv;
#pragma unroll
    for (int r = 0; r < 3; r++) filt_R(dv, b, r)[3 + ip] = rr[r];
}

// Thread 0 of block blockIdx.x = filter b_off + blockIdx.x: P_RR -= V_R V_R^T (the upper triangle, mirrored) and the pose.  The
// bookkeeping and the host mirror follow at the end of the call (k_set_meta).
__global__ void k_fuse_finish(EkfDev dv, FuseScratch fs, int b_off) {
    if (threadIdx.x != 0) return;
    const int b = b_off + blockIdx.x;
    const int M = 2 * fs.m_round[b];
    if (M == 0) return;
    const double *wr = fs.wr + (size_t)b * 4 * FUSE_MAX_COLS;
    double *x = filt_x(dv, b);
    double *R0 = filt_R(dv, b);
    for (int i = 0; i < 3; i++) {
        double xv = x[i];
        for (int c = 0; c < M; c++) xv = xv - wr[(size_t)i * FUSE_MAX_COLS + c] * wr[3 * (size_t)FUSE_MAX_COLS + c];
        x[i] = xv;
        for (int j = i; j < 3; j++) {
            double p = R0[(size_t)i * dv.xs + j];
            for (int c = 0; c < M; c++) p = p - wr[(size_t)i * FUSE_MAX_COLS + c] * wr[(size_t)j * FUSE_MAX_COLS + c];
            R0[(size_t)i * dv.xs + j] = p;
            R0[(size_t)j * dv.xs + i] = p;
        }
    }
}
