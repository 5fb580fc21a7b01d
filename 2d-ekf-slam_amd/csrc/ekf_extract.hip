// ekf_extract.hip -- submap extraction on the device (ekf_extract_map, ekf_get_submap): the marginal of the robot and chosen landmarks,
//   x' = x[sel],  P' = P[sel, sel],  sel = [0, 1, 2, 3 + 2 ids[0], 4 + 2 ids[0], ...],
// rows and columns of x and P bit for bit.  No arithmetic: all the work is in the layouts.
//
// Not on the hot path of the filter: once per call, with every slot of the source (and of the destination) folded in and all their
// streams idle.  Included by ekf_api.hip behind ekf_fuse.hip (fuse_block) and ekf_rewrite.hip (filt_*, JoinSrc, item_store); which
// source landmark, block or element a destination place takes is in ekf_device.h (extract_landmark, extract_block,
// extract_element), checked on the CPU by tests/cpp/extract_map_check.cpp.
//
// The source is only read and travels as a JoinSrc: its own tile count, strides and settled buffer (another handle of another
// capacity, kernel family and pipeline mode, or the destination's own handle with another filter index).
// `ex` = [filters of the launch][2] {landmarks the destination held before, landmarks it holds afterwards}, then
// [filters of the launch][mstride] ids.  The launch covers destination filters bd0 + blockIdx.y and source filters bs0 + blockIdx.y.
// On the destination's chain stream:
//   k_ext_tiles  Bm of the destination's settled buffer, one workgroup per destination tile and filter, up to the larger of the two maps
//   k_ext_vec    x, R and D, zeros behind the new map; the pose and P_RR with them
//   k_set_meta   (finish_rewrite) count, bookkeeping and the host mirror from what now lies in memory
// One writer per value, no atomics.  Every buffer ends as ekf_set_state of the extracted state would leave it.

// One workgroup per destination tile (blockIdx.x over the triangle of side nT_grid) and filter.  The tile's 32 row landmarks and 32
// column landmarks are mapped to source landmarks in LDS; the tile is walked in the frame changes' work items (reframe_item): a lane
// owns two complete destination blocks per item and stores two 32-byte pieces, a wave whole 256-byte runs.  A block reads its source
// block through fuse_block: its own block from D, the stored block, or the stored block transposed -- the order of the two ids
// decides, so the places below the diagonal of a diagonal tile and the landmarks' own blocks get what k_import stores there.  A
// scattered selection uses half of each 32-byte piece it reads.  Beyond the new map: zeros, up to the destination's previous map.
// `other`: the destination's second Bm buffer in overlap mode, which ekf_set_state leaves cleared, else null.
__global__ __launch_bounds__(256) void k_ext_tiles(EkfDev dv, int buf, double *other, JoinSrc sv, const int *ex, int mstride, int nb, int nT_grid, int bd0, int bs0) {
    __shared__ int lm[64];  // source landmark of the tile's row landmark [0, 32) and column landmark [32, 64); -1 beyond the new map
    const int k = blockIdx.y;
    const int n_old = ex[2 * k], n_new = ex[2 * k + 1];
    int I, J;
    tri_tile_ij(blockIdx.x, nT_grid, &I, &J);
    if (J >= lm_tiles(n_old > n_new ? n_old : n_new)) return;
    const int tid = threadIdx.x;
    if (tid < 64) lm[tid] = extract_landmark(ex + 2 * nb + (size_t)k * mstride, n_new, 32 * (tid < 32 ? I : J) + (tid & 31));
    __syncthreads();
    const bool live = J < lm_tiles(n_new);  // (else the whole tile is zeros)
    const double *sb = filt_Bm(sv, bs0 + k);
    const double *sD = filt_D(sv, bs0 + k);
    const size_t tile = bm_tile_base(dv.T, I, J);
    double *tp = filt_Bm(dv, buf, bd0 + k) + tile;
    double *tz = other ? other + (size_t)(bd0 + k) * dv.bm_stride + tile : nullptr;
    const double zero[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const ReframeItem it = reframe_item(r * 256 + tid);
        double o[2][4];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int a = lm[it.row[q] >> 1], c = lm[32 + (it.col >> 1)];
            o[q][0] = o[q][1] = o[q][2] = o[q][3] = 0.0;
            if (live && extract_block(sv.T, a, c).where != EX_ZERO) fuse_block(sv, sb, sD, a, c, o[q]);
        }
        item_store(tp, it, o);
        if (tz) item_store(tz, it, zero);
    }
}

// x, the three R rows and the three D components of destination filter bd0 + blockIdx.y (row blockIdx.x: 0 = x, 1..3 = R, 4..6 = D)
// from the source's, zeros behind the new map up to the previous one.  The robot entries (first three of x and of each R row: the
// pose and P_RR) are the source's.
__global__ __launch_bounds__(1024) void k_ext_vec(EkfDev dv, JoinSrc sv, const int *ex, int mstride, int nb, int bd0, int bs0) {
    const int k = blockIdx.y, row = blockIdx.x;
    const int n_old = ex[2 * k], n_new = ex[2 * k + 1];
    const int n_hi = n_old > n_new ? n_old : n_new;
    const int *ids = ex + 2 * nb + (size_t)k * mstride;
    const bool isD = row >= 4;
    const double *src = isD ? filt_D(sv, bs0 + k, row - 4) : row == 0 ? filt_x(sv, bs0 + k) : filt_R(sv, bs0 + k, row - 1);
    double *dst = isD ? filt_D(dv, bd0 + k, row - 4) : row == 0 ? filt_x(dv, bd0 + k) : filt_R(dv, bd0 + k, row - 1);
    const int len = isD ? n_hi : 3 + 2 * n_hi;
    for (int j = threadIdx.x; j < len; j += 1024) {
        double val = 0.0;
        if (isD) {
            const int a = extract_landmark(ids, n_new, j);
            if (a >= 0) val = src[a];
        } else if (j < 3) {
            val = src[j];
        } else {
            const int s = remove_row(ids, n_new, j - 3);
            if (s >= 0) val = src[3 + s];
        }
        dst[j] = val;
    }
}

// The dense read-out (ekf_get_submap): thread = element (i, column j = blockIdx.y) of the n x n staging matrix, n = 3 + 2 count,
// consecutive threads down a column.  The robot rows and columns come from R (P_RR with them), a landmark element from its one home
// (extract_element: D, or the upper-triangle place of the two source rows), so the matrix is symmetric bit for bit; column 0's
// threads bring x along.  The full P is never formed.
__global__ __launch_bounds__(256) void k_ext_dense(JoinSrc sv, int b, const int *ids, int count, double *xd, double *Pd, int ld, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= n) return;
    const double *R0 = filt_R(sv, b);
    const int si = i < 3 ? i : 3 + remove_row(ids, count, i - 3);
    if (j == 0) xd[i] = filt_x(sv, b)[si];
    double v;
    if (j < 3) {
        v = R0[(size_t)j * sv.xs + si];
    } else if (i < 3) {
        v = R0[(size_t)i * sv.xs + 3 + remove_row(ids, count, j - 3)];
    } else {
        const RmSource s = extract_element(sv.T, sv.dn, ids, count, i - 3, j - 3);
        v = s.where == RM_D ? filt_D(sv, b)[s.off] : filt_Bm(sv, b)[s.off];
    }
    Pd[(size_t)j * ld + i] = v;
}
