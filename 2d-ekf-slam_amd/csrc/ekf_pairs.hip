// ekf_pairs.hip -- duplicate search on the device (ekf_find_duplicates): the pairwise gate d^T S^-1 d <= gate over the settled
// landmark covariance, S = P_ii + P_jj - P_ij - P_ij^T, with the cross block P_ij read where it lives: one streaming read of the
// stored upper triangle.  Nothing of the filter is written.
//
// Not on the hot path: once per call, every slot folded in and all streams idle.  Included by ekf_api.hip behind ekf_rewrite.hip
// (filt_x / filt_D / filt_Bm, item_load, item_block, double4_t); the pair enumeration and the gate are in ekf_device.h
// (dup_tile_count, dup_tile_ij, dup_pair, dup_gate), checked on the CPU by tests/cpp/dup_map_check.cpp.
//
//   k_dup_boxes  (max_dist > 0 only) the bounding box of every group of 32 landmarks, a thread per group
//   k_dup_tiles  one workgroup per stored tile that can hold a considered pair; a thread owns two work items = four complete 2 x 2
//                cross blocks in two pairs of 32-byte loads, the positions and own blocks of the tile's 32 + 32 landmarks come
//                through LDS; no value crosses a lane
// A listed pair is appended through an INTEGER counter (the order is whatever the hardware makes it; the host sorts the short list
// by (i, j)), a degenerate pair is counted the same way: every value written is a function of the pair alone, so the sorted list
// has the same bits on every call and in the batch form.

#include "ekf_map_scratch.h"  // DupScratch

// What a call carries in its kernel arguments; md2 < 0: no Euclidean bound.
struct DupArgs {
    double gate, md2;
    int split_one;  // the split of every filter of the call when the scratch's table is not used
    int use_tab;
};

__device__ __forceinline__ int dup_split(const DupScratch &ds, const DupArgs &da, int b) { return da.use_tab ? ds.split[b] : da.split_one; }

// Thread = group g of 32 landmarks of filter b_off + blockIdx.y.  A NaN coordinate is ignored (fmin / fmax): its pairs fail
// the bound anyway.  A group beyond the map is never looked at.
__global__ __launch_bounds__(64) void k_dup_boxes(EkfDev dv, DupScratch ds, int b_off) {
    const int b = b_off + blockIdx.y;
    const int n = dv.n_lm[b];
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (32 * g >= n) return;
    const double *x = filt_x(dv, b) + 3;
    const double inf = __builtin_huge_val();
    double4_t bx = {inf, -inf, inf, -inf};
    const int l1 = 32 * g + 32 < n ? 32 * g + 32 : n;
    for (int l = 32 * g; l < l1; l++) {
        const double px = x[2 * l], py = x[2 * l + 1];
        bx.x = fmin(bx.x, px), bx.y = fmax(bx.y, px), bx.z = fmin(bx.z, py), bx.w = fmax(bx.w, py);
    }
    *(double4_t *)(ds.box + ((size_t)b * (dv.dn >> 5) + g) * 4) = bx;
}

__global__ __launch_bounds__(256) void k_dup_tiles(EkfDev dv, DupScratch ds, DupArgs da, int buf, int b_off) {
    __shared__ double lm[64][5];  // [tile row landmark | 32 + tile column landmark][x, y, D.xx, D.xy, D.yy]
    const int b = b_off + blockIdx.y;
    const int n = dv.n_lm[b];
    const int split = dup_split(ds, da, b);
    int I, J;
    if (!dup_tile_ij(blockIdx.x, n, split, &I, &J)) return;
    if (da.md2 >= 0.0) {  // the two groups' boxes further apart than the bound: no pair of the tile is considered
        const double *bx = ds.box + (size_t)b * (dv.dn >> 5) * 4;
        const double4_t bi = *(const double4_t *)(bx + 4 * I), bj = *(const double4_t *)(bx + 4 * J);
        if (dup_dist2(dup_box_gap(bi.x, bi.y, bj.x, bj.y), dup_box_gap(bi.z, bi.w, bj.z, bj.w)) > da.md2) return;
    }
    const int tid = threadIdx.x;
    // the tile's landmarks: requested here, staged in LDS behind the tile's own loads
    double st[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (tid < 64) {
        const int l = 32 * (tid < 32 ? I : J) + (tid & 31);
        if (l < n) {
            const double *x = filt_x(dv, b), *Dx = filt_D(dv, b);
            st[0] = x[3 + 2 * l], st[1] = x[4 + 2 * l];
            st[2] = Dx[l], st[3] = Dx[dv.dn + l], st[4] = Dx[2 * (size_t)dv.dn + l];
        }
    }
    const double *tp = filt_Bm(dv, buf, b) + bm_tile_base(dv.T, I, J);
    ReframeItem it[2];
    int pi[2][2], pj[2][2];
    bool pair[2][2];
    double4_t v[2][2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        it[r] = reframe_item(r * 256 + tid);
#pragma unroll
        for (int k = 0; k < 2; k++) pair[r][k] = dup_pair(n, split, I, J, it[r], k, &pi[r][k], &pj[r][k]);
        if (pair[r][0] || pair[r][1]) item_load(tp, it[r], v[r]);
    }
    if (tid < 64) {
#pragma unroll
        for (int e = 0; e < 5; e++) lm[tid][e] = st[e];
    }
    __syncthreads();
    int *cnt = ds.cnt + 2 * (size_t)b;
    ekf_dup_pair *list = ds.list + (size_t)b * ds.cap;
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (!pair[r][k]) continue;
            const double *li = lm[it[r].row[k] >> 1], *lj = lm[32 + (it[r].col >> 1)];
            const double dx = li[0] - lj[0], dy = li[1] - lj[1];
            if (da.md2 >= 0.0 && !(dup_dist2(dx, dy) <= da.md2)) continue;
            double m[4], d2 = 0.0;
            item_block(v[r], k, m);
            if (dup_gate(dx, dy, li + 2, lj + 2, m, &d2)) {
                atomicAdd(cnt + 1, 1);
                continue;
            }
            if (!(d2 <= da.gate)) continue;
            const int at = atomicAdd(cnt, 1);
            if (at < ds.cap) {
                ekf_dup_pair p;
                p.i = pi[r][k], p.j = pj[r][k], p.d2 = d2;
                list[at] = p;
            }
        }
}
