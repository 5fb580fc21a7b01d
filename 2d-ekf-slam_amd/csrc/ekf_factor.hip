// ekf_factor.hip -- map assessment on the device (ekf_joint_consistency): a tile-blocked Cholesky P_LL = U^T U of the settled
// landmark covariance in a scratch copy, four right-hand sides carried along, and from them the joint / map NEES, log det P, the
// pivots and the pose covariance conditioned on the map.  Nothing of the filter is written.
//
// Not on the hot path: once per call, every slot folded in and all streams idle.  Included by ekf_api.hip behind ekf_rewrite.hip
// (filt_x / filt_R / filt_D / filt_Bm, double2_t, double4_t); the index helpers are in ekf_device.h.
//
// Robot last:  U^T [y | W] = [e_L | P_LR],  S_R = P_RR - W^T W,  r = e_R - W^T y,
//   nees_map = |y|^2,  nees_joint = |y|^2 + r^T S_R^-1 r,  logdet_map = sum log U_ii^2,  logdet_joint = logdet_map + log det S_R
// so the map quantities stay valid when P_RR = 0 (a fresh or an anchored filter).
//
// The scratch S has the layout of one Bm buffer (64 x 64 tiles of the upper triangle, fragment order).  Per tile step k, three
// launches whose grids cover every filter of the call:
//   k_chol_diag   tile (k, k) factored in LDS with the tile's 64 right-hand-side rows as four more columns (y_k = U_kk^-T b_k falls
//                 out of the same elimination); pivots, sum of logs and the products of y_k and W_k accumulated in a fixed order
//   k_chol_panel  tiles (k, j > k): U_kj = U_kk^-T A_kj, a thread per column with the column in registers; b_j -= U_kj^T y_k
//   k_chol_trail  tiles (i, j), k < i <= j: A_ij -= U_ki^T U_kj on v_mfma_f64_16x16x4_f64.  A stored chain IS an MFMA operand of the
//                 two panel tiles (ekf_device.h: chol_operand_offset), so they are read straight from L2 in fragment order, a wave's
//                 load one 1 KiB run; nothing is staged in LDS.
// A filter whose pivot is not positive records `info` and min_pivot; every later kernel of the call returns at once for it.
// Every sum has one writer and a fixed order: no atomics, the same bits on every call and in the batch form.

#include "ekf_map_scratch.h"  // FactorScratch, FAC_*

// One workgroup per stored tile (blockIdx.x over the triangle of side nT_grid) and filter b_off + blockIdx.y: the settled tile into
// the scratch.  A landmark's own 2 x 2 block comes from D (the tile's own-block places are nobody's home: remove_source); rows and
// columns beyond the map get a unit diagonal and zeros (they factor to 1 and solve to 0).  The workgroup of a diagonal tile also
// fills the tile's 64 right-hand-side rows, the first workgroup the accumulators.
__global__ __launch_bounds__(256) void k_chol_stage(EkfDev dv, FactorScratch fs, int buf, int b_off, int nT_grid, int have_truth) {
    const int b = b_off + blockIdx.y;
    const int n = dv.n_lm[b];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid < FAC_ACC) fs.acc[(size_t)b * FAC_ACC + tid] = tid == FAC_MINP ? __builtin_huge_val() : 0.0;
    int I, J;
    tri_tile_ij(blockIdx.x, nT_grid, &I, &J);
    if (J >= lm_tiles(n)) return;
    const double *src = filt_Bm(dv, buf, b) + bm_tile_base(dv.T, I, J);
    double *dst = fs.S + (size_t)b * dv.bm_stride + bm_tile_base(dv.T, I, J);
    const double *Dx = filt_D(dv, b);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int o = (q * 256 + tid) * 2;
        const double2_t in = *(const double2_t *)(src + o);
        double v[2] = {in.x, in.y};
#pragma unroll
        for (int e = 0; e < 2; e++) {
            int il, jl;
            bm_tile_coords(o + e, &il, &jl);
            const int gi = 64 * I + il, gj = 64 * J + jl;
            if (gi >= 2 * n || gj >= 2 * n) v[e] = gi == gj ? 1.0 : 0.0;
            else if ((gi >> 1) == (gj >> 1)) v[e] = Dx[(size_t)((gi & 1) + (gj & 1)) * dv.dn + (gi >> 1)];
        }
        *(double2_t *)(dst + o) = (double2_t){v[0], v[1]};
    }
    if (I == J && tid < 64) {
        const int row = 64 * I + tid;
        double4_t r = {0.0, 0.0, 0.0, 0.0};
        if (row < 2 * n) {
            const double *x = filt_x(dv, b);
            const double *R0 = filt_R(dv, b);
            r.x = have_truth ? x[3 + row] - fs.xt[(size_t)b * dv.xs + 3 + row] : 0.0;
            r.y = R0[3 + row], r.z = R0[(size_t)dv.xs + 3 + row], r.w = R0[2 * (size_t)dv.xs + 3 + row];
        }
        *(double4_t *)(fs.rhs + ((size_t)b * dv.rows + row) * 4) = r;
    }
}

// Step k, tile (k, k) of filter b_off + blockIdx.x.  Threads 0..255: column tid & 63, rows = tid >> 6 (mod 4) of the tile; threads
// 256..319: right-hand side (tid & 3), rows = (tid - 256) >> 2 (mod 16).  Row i is left unscaled in LDS (nothing below it reads it
// again but through the division by its pivot's root), so a step needs one barrier.
__global__ __launch_bounds__(320) void k_chol_diag(EkfDev dv, FactorScratch fs, int k, int b_off) {
    __shared__ double A[64][64];
    __shared__ __attribute__((aligned(32))) double Bv[64][4];
    __shared__ double piv[64];
    const int b = b_off + blockIdx.x;
    const int n = dv.n_lm[b];
    double *acc = fs.acc + (size_t)b * FAC_ACC;
    if (k >= lm_tiles(n) || acc[FAC_INFO] != 0.0) return;
    const int tid = threadIdx.x;
    double *tile = fs.S + (size_t)b * dv.bm_stride + bm_tile_base(dv.T, k, k);
    double *rhs = fs.rhs + ((size_t)b * dv.rows + 64 * (size_t)k) * 4;
    const bool mat = tid < 256;
    const int c = tid & 63, q = (tid >> 6) & 3;  // matrix threads
    const int rc = tid & 3, q16 = (tid - 256) >> 2;  // right-hand-side threads
    if (mat) {
#pragma unroll
        for (int p = 0; p < 8; p++) {
            const int o = (p * 256 + tid) * 2;
            const double2_t in = *(const double2_t *)(tile + o);
            int il, jl;
            bm_tile_coords(o, &il, &jl);
            A[il][jl] = in.x;
            bm_tile_coords(o + 1, &il, &jl);
            A[il][jl] = in.y;
        }
    } else {
        const double4_t r = *(const double4_t *)(rhs + (size_t)(tid - 256) * 4);
        Bv[tid - 256][0] = r.x, Bv[tid - 256][1] = r.y, Bv[tid - 256][2] = r.z, Bv[tid - 256][3] = r.w;
    }
    double logsum = acc[FAC_LOGDET], minp = acc[FAC_MINP], maxp = acc[FAC_MAXP];
    __syncthreads();
    for (int i = 0; i < 64; i++) {
        const double d = A[i][i];  // (the same value in every thread: the branch below is taken by all or by none)
        if (64 * k + i < 2 * n) {
            if (!(d > 0.0)) {
                if (tid == 0) acc[FAC_INFO] = (double)(64 * k + i + 1), acc[FAC_MINP] = d, acc[FAC_MAXP] = maxp;
                return;
            }
            logsum += log(d);
            minp = d < minp ? d : minp;
            maxp = d > maxp ? d : maxp;
        }
        const double s = sqrt(d);
        if (tid == 0) piv[i] = s;
        if (mat) {
            const double uic = A[i][c] / s;
#pragma unroll
            for (int t = 0; t < 16; t++) {
                const int r = q + 4 * t;
                if (r > i && r <= c) A[r][c] -= (A[i][r] / s) * uic;
            }
        } else {
            const double yi = Bv[i][rc] / s;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int r = q16 + 16 * t;
                if (r > i) Bv[r][rc] -= (A[i][r] / s) * yi;
            }
        }
        __syncthreads();
    }
    if (mat) {
#pragma unroll
        for (int p = 0; p < 8; p++) {
            const int o = (p * 256 + tid) * 2;
            double v[2];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                int il, jl;
                bm_tile_coords(o + e, &il, &jl);
                v[e] = il == jl ? piv[il] : il < jl ? A[il][jl] / piv[il] : 0.0;
            }
            *(double2_t *)(tile + o) = (double2_t){v[0], v[1]};
        }
    } else {
        const int row = tid - 256;
        const double4_t y = {Bv[row][0] / piv[row], Bv[row][1] / piv[row], Bv[row][2] / piv[row], Bv[row][3] / piv[row]};
        *(double4_t *)(rhs + (size_t)row * 4) = y;
    }
    __syncthreads();  // (the reductions below read what the right-hand-side threads left in Bv, unscaled, and piv)
    if (tid < 10) {  // |y|^2, the upper triangle of W^T W, W^T y: one thread per sum, rows in order
        const int u = tid == 0 ? 0 : tid <= 3 ? 1 : tid <= 5 ? 2 : tid == 6 ? 3 : tid - 6;
        const int v = tid == 0 ? 0 : tid <= 3 ? tid : tid <= 5 ? tid - 2 : tid == 6 ? 3 : 0;
        double sum = acc[FAC_YY + tid];
        for (int i = 0; i < 64; i++) sum += (Bv[i][u] / piv[i]) * (Bv[i][v] / piv[i]);
        acc[FAC_YY + tid] = sum;
    }
    if (tid == 0) acc[FAC_LOGDET] = logsum, acc[FAC_MINP] = minp, acc[FAC_MAXP] = maxp;
}

// Step k, tile (k, j = k + 1 + blockIdx.x) of filter b_off + blockIdx.y: one wave, thread c owns column c of the tile in 64
// registers.  U_kk is read from LDS (every lane the same word: a broadcast), y_k from LDS too.
__global__ __launch_bounds__(64) void k_chol_panel(EkfDev dv, FactorScratch fs, int k, int b_off) {
    __shared__ double U[64][64];
    __shared__ __attribute__((aligned(32))) double Y[64][4];
    const int b = b_off + blockIdx.y;
    const int n = dv.n_lm[b];
    const int j = k + 1 + blockIdx.x;
    if (j >= lm_tiles(n) || fs.acc[(size_t)b * FAC_ACC + FAC_INFO] != 0.0) return;
    const int c = threadIdx.x;
    double *S = fs.S + (size_t)b * dv.bm_stride;
    const double *ukk = S + bm_tile_base(dv.T, k, k);
    double *tile = S + bm_tile_base(dv.T, k, j);
    for (int p = 0; p < 32; p++) {
        const int o = (p * 64 + c) * 2;
        const double2_t in = *(const double2_t *)(ukk + o);
        int il, jl;
        bm_tile_coords(o, &il, &jl);
        U[il][jl] = in.x;
        bm_tile_coords(o + 1, &il, &jl);
        U[il][jl] = in.y;
    }
    *(double4_t *)&Y[c][0] = *(const double4_t *)(fs.rhs + ((size_t)b * dv.rows + 64 * (size_t)k + c) * 4);
    double x[64];
#pragma unroll
    for (int i = 0; i < 64; i++) x[i] = tile[bm_offset(1, i, c)];
    __syncthreads();
    double dot[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 64; i++) {
        const double xi = x[i] / U[i][i];
        x[i] = xi;
#pragma unroll
        for (int r = i + 1; r < 64; r++) x[r] -= U[i][r] * xi;
#pragma unroll
        for (int e = 0; e < 4; e++) dot[e] += xi * Y[i][e];
    }
#pragma unroll
    for (int i = 0; i < 64; i++) tile[bm_offset(1, i, c)] = x[i];
    double4_t *bj = (double4_t *)(fs.rhs + ((size_t)b * dv.rows + 64 * (size_t)j + c) * 4);
    const double4_t v = *bj;
    *bj = (double4_t){v.x - dot[0], v.y - dot[1], v.z - dot[2], v.w - dot[3]};
}

// Step k, trailing tile blockIdx.x (ekf_device.h: chol_trail_ij) of filter b_off + blockIdx.y, in place.  Wave w owns the tile's
// row block w: four accumulators loaded and stored in the tile's fragment order, 16 k-steps each.
__global__ __launch_bounds__(256) void k_chol_trail(EkfDev dv, FactorScratch fs, int k, int b_off, int nT_grid) {
    const int b = b_off + blockIdx.y;
    const int n = dv.n_lm[b];
    int I, J;
    chol_trail_ij(blockIdx.x, nT_grid, k, &I, &J);
    if (J >= lm_tiles(n) || fs.acc[(size_t)b * FAC_ACC + FAC_INFO] != 0.0) return;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *S = fs.S + (size_t)b * dv.bm_stride;
    const double *ui = S + bm_tile_base(dv.T, k, I);
    const double *uj = S + bm_tile_base(dv.T, k, J);
    double *tp = S + bm_tile_base(dv.T, I, J);
    double4_t acc[4];
#pragma unroll
    for (int cc = 0; cc < 4; cc++) {
        const double2_t l2 = *(const double2_t *)(tp + (w * 4 + cc) * 256 + lane * 2);
        const double2_t h2 = *(const double2_t *)(tp + (w * 4 + cc) * 256 + 128 + lane * 2);
        acc[cc] = (double4_t){l2.x, l2.y, h2.x, h2.y};
    }
#pragma unroll
    for (int sb = 0; sb < 4; sb++) {  // k-steps 4 sb .. 4 sb + 3: rows 16 sb .. 16 sb + 15 of the two panel tiles
        double a[4], bq[4][4];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const double2_t av = *(const double2_t *)(ui + chol_operand_offset(4 * sb + 2 * h, w, lane));
            a[2 * h] = -av.x, a[2 * h + 1] = -av.y;
#pragma unroll
            for (int cc = 0; cc < 4; cc++) {
                const double2_t bv = *(const double2_t *)(uj + chol_operand_offset(4 * sb + 2 * h, cc, lane));
                bq[2 * h][cc] = bv.x, bq[2 * h + 1][cc] = bv.y;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int cc = 0; cc < 4; cc++) acc[cc] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], bq[s][cc], acc[cc], 0, 0, 0);
    }
#pragma unroll
    for (int cc = 0; cc < 4; cc++) {
        *(double2_t *)(tp + (w * 4 + cc) * 256 + lane * 2) = (double2_t){acc[cc].x, acc[cc].y};
        *(double2_t *)(tp + (w * 4 + cc) * 256 + 128 + lane * 2) = (double2_t){acc[cc].z, acc[cc].w};
    }
}

// Thread 0 of block blockIdx.x = filter b_off + blockIdx.x: the robot block last, and the results record.
__global__ __launch_bounds__(64) void k_chol_finish(EkfDev dv, FactorScratch fs, int b_off, int have_truth) {
    if (threadIdx.x != 0) return;
    const int b = b_off + blockIdx.x;
    const int n = dv.n_lm[b];
    const double *acc = fs.acc + (size_t)b * FAC_ACC;
    const double *x = filt_x(dv, b);
    const double *R0 = filt_R(dv, b);
    const double nan = __builtin_nan("");
    ekf_joint o;
    o.n_landmarks = n;
    o.info = n > 0 ? (int)acc[FAC_INFO] : 0;
    o.nees_map = o.nees_joint = o.logdet_map = o.logdet_joint = nan;
    o.min_pivot = n > 0 ? acc[FAC_MINP] : 0.0;
    o.max_pivot = n > 0 ? acc[FAC_MAXP] : 0.0;
    for (int i = 0; i < 9; i++) o.cov_robot_given_map[i] = nan;
    if (o.info == 0) {
        const double yy = n > 0 ? acc[FAC_YY] : 0.0;
        double ww[3][3], wy[3];
        for (int i = 0, t = 0; i < 3; i++)
            for (int j = i; j < 3; j++, t++) ww[i][j] = ww[j][i] = n > 0 ? acc[FAC_WW + t] : 0.0;
        for (int i = 0; i < 3; i++) wy[i] = n > 0 ? acc[FAC_WY + i] : 0.0;
        o.logdet_map = n > 0 ? acc[FAC_LOGDET] : 0.0;
        if (have_truth) o.nees_map = yy;
        double s[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = i; j < 3; j++) s[i][j] = s[j][i] = R0[(size_t)i * dv.xs + j] - ww[i][j];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) o.cov_robot_given_map[3 * i + j] = s[i][j];
        // S_R = L L^T, written out (no indexed local arrays: one thread, everything in registers)
        const double d0 = s[0][0];
        const double l00 = sqrt(d0), l10 = s[1][0] / l00, l20 = s[2][0] / l00;
        const double d1 = s[1][1] - l10 * l10;
        const double l11 = sqrt(d1), l21 = (s[2][1] - l20 * l10) / l11;
        const double d2 = s[2][2] - l20 * l20 - l21 * l21;
        const double l22 = sqrt(d2);
        const bool pd = d0 > 0.0 && d1 > 0.0 && d2 > 0.0;  // (a pivot that is not positive makes every later one NaN or meaningless: the test fails then)
        const double ld = log(d0) + log(d1) + log(d2);
        if (!pd) {
            o.info = -1;
        } else {
            o.logdet_joint = o.logdet_map + ld;
            if (have_truth) {
                const double *xt = fs.xt + (size_t)b * dv.xs;
                double e[3] = {x[0] - xt[0], x[1] - xt[1], x[2] - xt[2]};
                e[2] -= 6.283185307179586 * floor((e[2] + 3.141592653589793) / 6.283185307179586);  // (ekf_filter_math.h: nees_sample)
                const double r0 = e[0] - wy[0], r1 = e[1] - wy[1], r2 = e[2] - wy[2];
                const double z0 = r0 / l00, z1 = (r1 - l10 * z0) / l11, z2 = (r2 - l20 * z0 - l21 * z1) / l22;
                const double q = z0 * z0 + z1 * z1 + z2 * z2;
                o.nees_joint = yy + q;
            }
        }
    }
    fs.out[b] = o;
}

// The factor of filter b as a dense matrix, column-major with leading dimension ld (ekf_debug_joint_factor): thread per element.
__global__ void k_chol_export(EkfDev dv, FactorScratch fs, int b, int m, double *out, int ld) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= m) return;
    out[(size_t)j * ld + i] = i <= j ? fs.S[(size_t)b * dv.bm_stride + bm_offset(dv.T, i, j)] : 0.0;
}
