// ekf_rewrite.hip -- the kernels that rewrite a settled filter in place: dense import / export, landmark removal, frame changes, map joining.
//
// None of them is on the hot path: each runs once per call, with every slot folded in and all streams idle, and is bandwidth- or
// launch-bound.  Included by ekf_api.hip behind ekf_kernels.hip (double2_t, double4_t); the index helpers are in ekf_device.h.

// Filter b's own part of the handle's arrays: x, the three R rows (stride xs), the three D components (stride dn), its tiles in Bm[buf].
// F = EkfDev or JoinSrc (a join's source handle, read only, has strides of its own).  By value where no member is indexed by a
// variable (the copy dissolves into the kernel's own argument loads), by reference for Bm[buf]: the forms that leave the kernels' code
// as it was measured.
template <typename F>
__device__ __forceinline__ auto filt_x(const F f, int b) { return f.x + (size_t)b * f.xs; }
template <typename F>
__device__ __forceinline__ auto filt_R(const F f, int b, int row = 0) { return f.R + ((size_t)b * 3 + row) * f.xs; }
template <typename F>
__device__ __forceinline__ auto filt_D(const F f, int b, int comp = 0) { return f.D + ((size_t)b * 3 + comp) * f.dn; }
__device__ __forceinline__ double *filt_Bm(const EkfDev &dv, int buf, int b) { return dv.Bm[buf] + (size_t)b * dv.bm_stride; }

// Value k of the launch's per-filter argument (a struct A of doubles) for its filter `by`: a one-filter call carries the argument in
// the kernel arguments (`one`), a batch call passes a table `tab` = [filters of the launch][doubles of A] instead.
template <typename A>
__device__ __forceinline__ double arg_value(const A &one, const double *tab, int by, int k) {
    static_assert(sizeof(A) % sizeof(double) == 0, "doubles only");
    return tab ? tab[(int)(sizeof(A) / sizeof(double)) * by + k] : ((const double *)&one)[k];
}

// The end of every rewrite of filter b, which now holds n_lm landmarks (dv.n_lm[b] is the caller's): both dense passes sized for
// the new map, the sticky status cleared, no slot pending, and the host mirror refreshed with the pose (x) and the robot block
// (3 x 3, leading dimension ld) the caller has just stored.
__device__ __forceinline__ void settle_meta(const EkfDev dv, int b, int n_lm, const double *x, const double *prr, size_t ld) {
    dv.n_lm_sweep[b] = n_lm;
    dv.n_lm_flush[(size_t)b * 2] = n_lm;
    dv.n_lm_flush[(size_t)b * 2 + 1] = n_lm;
    dv.status[b] = 0;
    EkfMirror *mr = dv.mirror + b;
    for (int i = 0; i < 3; i++) mr->pose[i] = x[i];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) mr->Prr[i * 3 + j] = prr[i * ld + j];
    mr->n_lm = n_lm;
    mr->status = 0;
    mr->log_count = dv.log_count[b];
    for (int m = 0; m < 2 * dv.maxp; m++) dv.slot_active[(size_t)b * 2 * dv.maxp + m] = 0;
}

// ---------------------------------------------------------------------------------------------
// Dense import / export (tests, checkpoint).  Pd is n x n with leading dimension ld, symmetric.
// Both run with every slot folded in and both streams idle; `buf` is the settled Bm buffer.
// (They keep their own index expressions, one sum per access: through the accessors k_export needs 11 instead of 9 VGPRs.)
// ---------------------------------------------------------------------------------------------
__global__ void k_import(EkfDev dv, int b, int buf, const double *xd, const double *Pd, int ld, int n) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    int i = blockIdx.y;
    if (j >= n) return;
    double v = Pd[(size_t)i * ld + j];
    double *R0 = dv.R + (size_t)b * 3 * dv.xs;
    double *Dx = dv.D + (size_t)b * 3 * dv.dn;
    if (i == 0) dv.x[(size_t)b * dv.xs + j] = xd[j];
    if (i < 3) {
        R0[(size_t)i * dv.xs + j] = v;
        return;
    }
    if (j < 3) return;
    int ip = i - 3, jp = j - 3;
    if ((ip >> 6) > (jp >> 6)) return;  // only tiles of the upper triangle are stored
    dv.Bm[buf][(size_t)b * dv.bm_stride + bm_offset(dv.T, ip, jp)] = v;
    if ((ip >> 1) == (jp >> 1) && ip <= jp) {
        int lm = ip >> 1;
        int comp = (ip & 1) + (jp & 1);  // (0,0)->xx, (0,1)->xy, (1,1)->yy
        Dx[(size_t)comp * dv.dn + lm] = v;
    }
}

__global__ void k_export(EkfDev dv, int b, int buf, double *xd, double *Pd, int ld, int n) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    int i = blockIdx.y;
    if (j >= n) return;
    const double *R0 = dv.R + (size_t)b * 3 * dv.xs;
    const double *Dx = dv.D + (size_t)b * 3 * dv.dn;
    if (i == 0) xd[j] = dv.x[(size_t)b * dv.xs + j];
    double v;
    if (i < 3) v = R0[(size_t)i * dv.xs + j];
    else if (j < 3) v = R0[(size_t)j * dv.xs + i];
    else {
        int ip = i - 3, jp = j - 3;
        if ((ip >> 1) == (jp >> 1)) v = Dx[(size_t)((ip & 1) + (jp & 1)) * dv.dn + (ip >> 1)];
        else if (ip < jp) v = dv.Bm[buf][(size_t)b * dv.bm_stride + bm_offset(dv.T, ip, jp)];
        else v = dv.Bm[buf][(size_t)b * dv.bm_stride + bm_offset(dv.T, jp, ip)];
    }
    Pd[(size_t)i * ld + j] = v;
}

__global__ void k_set_meta(EkfDev dv, int b, int n_lm) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    dv.n_lm[b] = n_lm;
    settle_meta(dv, b, n_lm, filt_x(dv, b), filt_R(dv, b), dv.xs);  // (the state as it lies in memory)
}

// ---------------------------------------------------------------------------------------------
// Landmark removal (ekf_remove_landmarks): the kept rows and columns of x and P, no arithmetic.  `rm` = [B][2] (old, new landmark
// count; new == old: the filter keeps everything) then [B][mstride] maps (ekf_device.h: remove_row).  Every buffer ends as k_import
// of the reduced dense state would leave it.  Run with every slot folded in and both streams idle.
// ---------------------------------------------------------------------------------------------
// One workgroup per destination tile (blockIdx.x over the triangle of side nT_grid) and filter (blockIdx.y): every element reads its
// source through L2 and the tile goes out as wave-contiguous 16-byte stores.  dst: the other Bm buffer (layout dv.T, stride
// dv.bm_stride; tiles up to the old map) or, in place, a scratch of side Tdst (tiles up to the reduced map).
__global__ __launch_bounds__(256) void k_rm_gather(EkfDev dv, int buf_src, const int *rm, int mstride, int nT_grid, double *dst, int Tdst,
                                                   size_t dst_stride, int to_scratch) {
    __shared__ int srow[64], scol[64];
    const int b = blockIdx.y;
    const int n_old = rm[2 * b], n_new = rm[2 * b + 1];
    const int limit = lm_tiles(to_scratch ? n_new : n_old);
    if (to_scratch && n_new == n_old) return;  // in place, nothing to move for this filter
    int I, J;
    tri_tile_ij(blockIdx.x, nT_grid, &I, &J);
    if (J >= limit) return;
    const int *map = rm + 2 * dv.B + (size_t)b * mstride;
    const int tid = threadIdx.x;
    if (tid < 64) srow[tid] = remove_row(map, n_new, 64 * I + tid);
    else if (tid < 128) scol[tid - 64] = remove_row(map, n_new, 64 * J + tid - 64);
    __syncthreads();
    const double *src = filt_Bm(dv, buf_src, b);
    const double *Dx = filt_D(dv, b);
    double *out = dst + (size_t)b * dst_stride + bm_tile_base(Tdst, I, J);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int o = (q * 256 + tid) * 2;
        double v[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            int il, jl;
            bm_tile_coords(o + e, &il, &jl);
            const RmSource s = remove_source(dv.T, dv.dn, srow[il], scol[jl]);
            v[e] = s.where == RM_BM ? src[s.off] : s.where == RM_D ? Dx[s.off] : 0.0;
        }
        *(double2_t *)(out + o) = (double2_t){v[0], v[1]};
    }
}

// Second half of a removal, tiles up to each filter's old map: in place, the scratch copied back into Bm[buf] (zeros from the reduced
// map's last tile on); in overlap mode (scratch == nullptr) the buffer the gather read from is cleared, as ekf_set_state leaves it.
__global__ __launch_bounds__(256) void k_rm_finish(EkfDev dv, int buf, const int *rm, int nT_grid, const double *scratch, int Tdst, size_t scratch_stride) {
    const int b = blockIdx.y;
    const int n_old = rm[2 * b], n_new = rm[2 * b + 1];
    if (scratch && n_new == n_old) return;
    int I, J;
    tri_tile_ij(blockIdx.x, nT_grid, &I, &J);
    if (J >= lm_tiles(n_old)) return;
    const bool copy = scratch && J < lm_tiles(n_new);
    const double *in = copy ? scratch + (size_t)b * scratch_stride + bm_tile_base(Tdst, I, J) : nullptr;
    double *out = filt_Bm(dv, buf, b) + bm_tile_base(dv.T, I, J);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int o = (q * 256 + threadIdx.x) * 2;
        double2_t v = (double2_t){0.0, 0.0};
        if (copy) v = *(const double2_t *)(in + o);
        *(double2_t *)(out + o) = v;
    }
}

// x, the three R rows and the three D components of filter blockIdx.y (row blockIdx.x: 0 = x, 1..3 = R, 4..6 = D), compacted in place:
// chunks in increasing order, each read whole before it is stored (a destination never lies after its source), zeros behind the
// reduced map.  The robot entries (first three of x and R) stay where they are.
__global__ __launch_bounds__(1024) void k_rm_vec(EkfDev dv, const int *rm, int mstride) {
    const int b = blockIdx.y, row = blockIdx.x;
    const int n_old = rm[2 * b], n_new = rm[2 * b + 1];
    if (n_new == n_old) return;
    const int *map = rm + 2 * dv.B + (size_t)b * mstride;
    const bool isD = row >= 4;
    double *v = isD ? filt_D(dv, b, row - 4) : row == 0 ? filt_x(dv, b) : filt_R(dv, b, row - 1);
    const int len = isD ? n_old : 3 + 2 * n_old;
    for (int c0 = 0; c0 < len; c0 += 1024) {
        const int k = c0 + threadIdx.x;
        double val = 0.0;
        if (k < len) {
            if (isD) val = k < n_new ? v[map[k]] : 0.0;
            else if (k < 3) val = v[k];
            else {
                const int s = remove_row(map, n_new, k - 3);
                val = s >= 0 ? v[3 + s] : 0.0;
            }
        }
        __syncthreads();
        if (k < len) v[k] = val;
    }
}

// ---------------------------------------------------------------------------------------------
// Frame changes (ekf_transform_frame / ekf_anchor_at_robot): x' = g(x), P' = J P J^T with J block diagonal over the landmarks
// (Q = Rot(-theta) resp. Rot(-phi)) plus, for the anchor, three dense robot columns A_l = -Q [I | S (L_l - p)].  With
// W_l = Q P_lR + A_l P_RR / 2 every landmark block is  P_lm' = Q P_lm Q^T + A_l W_m^T + W_l A_m^T  (rigid: A = W = 0), so a stored
// tile depends on nothing but itself and six doubles per row and column.  Launch order on the chain stream, every slot folded in
// and both streams idle:  k_reframe_vec (landmark entries of x, R, D; the anchor's operands; reads the robot entries, which it
// leaves alone)  ->  k_reframe_tiles (Bm in place)  ->  k_reframe_finish (robot entries, bookkeeping, host mirror).
// A rigid frame is six doubles: t_x, t_y, cos(theta), sin(theta), theta (cos / sin taken on the host).  A one-filter call carries it in
// the kernel arguments (`one`); a batch call passes a table `fr` = [filters of the launch][6] instead.  The anchor takes cos / sin of
// the filter's own heading on the device, the same expression in both kernels.  The launch covers filters b_off + blockIdx.y.
// The anchor's operands live in slot set 0 of FA (A rows) and FB (W rows), four doubles per landmark-space row (f_stride >= 8 *
// rows): the window is folded, nobody reads the slot arrays, and the host clears them behind the tile kernel.
// ---------------------------------------------------------------------------------------------
struct Rot2 {
    double c, s;  // Q = [[c, s], [-s, c]]
};
struct ReframeFrame {
    double v[6];
};
// Q M Q^T of a general 2x2 block (m00 m01; m10 m11); c = 1, s = 0 returns M bit for bit
__device__ inline void rot_block(const Rot2 q, double m00, double m01, double m10, double m11, double o[4]) {
    const double a00 = q.c * m00 + q.s * m10, a01 = q.c * m01 + q.s * m11;
    const double a10 = q.c * m10 - q.s * m00, a11 = q.c * m11 - q.s * m01;
    o[0] = a00 * q.c + a01 * q.s, o[1] = a01 * q.c - a00 * q.s;
    o[2] = a10 * q.c + a11 * q.s, o[3] = a11 * q.c - a10 * q.s;
}
// the rank-3 pair A_r W_c^T + W_r A_c^T of one element: rows of [A (3) . W (3) .] as the operands are stored
__device__ inline double cross_term(const double *r, const double *c) {
    return r[0] * c[4] + r[1] * c[5] + r[2] * c[6] + r[4] * c[0] + r[5] * c[1] + r[6] * c[2];
}

// A work item's eight doubles (ekf_device.h: reframe_item) as they lie in memory, two 32-byte pieces: value v of piece s is element
// (row[v & 1] + s, col + (v >> 1)).  item_block: the item's block k as {(0,0), (0,1), (1,0), (1,1)}; item_store: two such blocks back
// into their pieces (non-temporal: nobody reads the tile again before the call returns).
__device__ __forceinline__ void item_load(const double *tp, const ReframeItem &it, double4_t v[2]) {
    v[0] = *(const double4_t *)(tp + it.off);
    v[1] = *(const double4_t *)(tp + it.off + 32);
}
__device__ __forceinline__ void item_block(const double4_t v[2], int k, double m[4]) { m[0] = v[0][k], m[1] = v[0][2 + k], m[2] = v[1][k], m[3] = v[1][2 + k]; }
__device__ __forceinline__ void item_store(double *tp, const ReframeItem &it, const double o[2][4]) {
    __builtin_nontemporal_store(((double4_t){o[0][0], o[1][0], o[0][1], o[1][1]}), (double4_t *)(tp + it.off));
    __builtin_nontemporal_store(((double4_t){o[0][2], o[1][2], o[0][3], o[1][3]}), (double4_t *)(tp + it.off + 32));
}

template <bool ANCHOR>
__global__ __launch_bounds__(256) void k_reframe_vec(EkfDev dv, ReframeFrame one, const double *fr, int b_off) {
    const int b = b_off + blockIdx.y;
    const int n = dv.n_lm[b];
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= 32 * lm_tiles(n)) return;  // landmark slots of the map's last tile row included: their operands are zeros
    double *x = dv.x + (size_t)b * dv.xs;  // (not filt_x: the anchor's register count follows this line)
    double *R0 = filt_R(dv, b);
    double *Dx = filt_D(dv, b);
    double *opA = dv.FA + (size_t)b * 2 * dv.f_stride + (size_t)l * 8;
    double *opW = dv.FB + (size_t)b * 2 * dv.f_stride + (size_t)l * 8;
    if (l >= n) {
        if (ANCHOR)
            for (int k = 0; k < 8; k++) opA[k] = 0.0, opW[k] = 0.0;
        return;
    }
    // everything this landmark needs is read before anything is stored; the robot entries are not written in this kernel
    const double px = x[0], py = x[1];
    Rot2 q;
    double tx, ty;
    if (ANCHOR) q.c = cos(x[2]), q.s = sin(x[2]), tx = px, ty = py;
    else tx = arg_value(one, fr, blockIdx.y, 0), ty = arg_value(one, fr, blockIdx.y, 1), q.c = arg_value(one, fr, blockIdx.y, 2), q.s = arg_value(one, fr, blockIdx.y, 3);
    const double dx = x[3 + 2 * l] - tx, dy = x[4 + 2 * l] - ty;
    const double lx = q.c * dx + q.s * dy, ly = q.c * dy - q.s * dx;
    double r[3][2];  // P_Rl
    for (int k = 0; k < 3; k++) r[k][0] = R0[(size_t)k * dv.xs + 3 + 2 * l], r[k][1] = R0[(size_t)k * dv.xs + 4 + 2 * l];
    const double xx = Dx[l], xy = Dx[dv.dn + l], yy = Dx[2 * (size_t)dv.dn + l];
    double d[4];
    rot_block(q, xx, xy, xy, yy, d);  // (d[1] is the stored xy: one expression, so the block stays symmetric by construction)
    if (!ANCHOR) {
        double v[3][2];  // P_Rl Q^T, then J_R = diag(Q, 1) from the left
        for (int k = 0; k < 3; k++) v[k][0] = r[k][0] * q.c + r[k][1] * q.s, v[k][1] = r[k][1] * q.c - r[k][0] * q.s;
        for (int e = 0; e < 2; e++) {
            R0[3 + 2 * l + e] = q.c * v[0][e] + q.s * v[1][e];
            R0[(size_t)dv.xs + 3 + 2 * l + e] = q.c * v[1][e] - q.s * v[0][e];
            R0[2 * (size_t)dv.xs + 3 + 2 * l + e] = v[2][e];
        }
        x[3 + 2 * l] = lx, x[4 + 2 * l] = ly;
        Dx[l] = d[0], Dx[dv.dn + l] = d[1], Dx[2 * (size_t)dv.dn + l] = d[3];
        return;
    }
    double prr[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) prr[i][j] = R0[(size_t)i * dv.xs + j];
    // A_l = -Q [I | S (L - p)] with Q S (L - p) = S L' = (-L'_y, L'_x);  W_l = Q P_lR + A_l P_RR / 2
    const double A[2][3] = {{-q.c, -q.s, ly}, {q.s, -q.c, -lx}};
    double W[2][3];
    for (int k = 0; k < 3; k++) {
        W[0][k] = q.c * r[k][0] + q.s * r[k][1] + 0.5 * (A[0][0] * prr[0][k] + A[0][1] * prr[1][k] + A[0][2] * prr[2][k]);
        W[1][k] = q.c * r[k][1] - q.s * r[k][0] + 0.5 * (A[1][0] * prr[0][k] + A[1][1] * prr[1][k] + A[1][2] * prr[2][k]);
    }
    double row[2][8];
    for (int e = 0; e < 2; e++) {
        for (int k = 0; k < 3; k++) row[e][k] = A[e][k], row[e][4 + k] = W[e][k];
        row[e][3] = 0.0, row[e][7] = 0.0;
    }
    Dx[l] = d[0] + cross_term(row[0], row[0]);
    Dx[dv.dn + l] = d[1] + cross_term(row[0], row[1]);
    Dx[2 * (size_t)dv.dn + l] = d[3] + cross_term(row[1], row[1]);
    x[3 + 2 * l] = lx, x[4 + 2 * l] = ly;
    for (int k = 0; k < 3; k++) R0[(size_t)k * dv.xs + 3 + 2 * l] = 0.0, R0[(size_t)k * dv.xs + 4 + 2 * l] = 0.0;
    for (int e = 0; e < 2; e++)
        for (int k = 0; k < 4; k++) opA[4 * e + k] = row[e][k], opW[4 * e + k] = row[e][4 + k];
}

// One workgroup per stored tile (blockIdx.x over the triangle of side nT_grid) and filter: one read and one write of every live
// chain, in place in Bm[buf].  A thread owns two work items (ekf_device.h: reframe_item), i.e. four 32-byte loads in flight and
// four complete 2x2 blocks, all loaded before the first store; a wave's loads and stores are whole 256-byte runs.  Tiles beyond
// the filter's map and the dead chains of a diagonal tile (block row > block column) are skipped as the dense pass skips them;
// elements beyond the map inside a live tile are zeros with zero operands and stay zeros.
// Diagonal chains of a diagonal tile (4 of its 10 live chains; 0.4 % of all chains at N = 4096) also hold places that are nobody's
// home -- the landmarks' own blocks (home: D) and the blocks below the diagonal -- which are stale in normal operation.  They are
// never transformed: a wave takes the chain with one lane per 2x2 block (eight-byte accesses that together cover the chain's 2 KiB
// exactly once), lane (a, c) with a < c transforms its block and stores it twice, at home and transposed at (c, a); lane (a, a)
// writes the own block from the NEW D (k_reframe_vec has run).  That is what k_import of the transformed state stores there.
template <bool ANCHOR>
__global__ __launch_bounds__(256) void k_reframe_tiles(EkfDev dv, int buf, ReframeFrame one, const double *fr, int b_off, int nT_grid) {
    __shared__ double ops[128][8];  // [tile row | 64 + tile column][A row . W row .]
    const int b = b_off + blockIdx.y;
    const int n = dv.n_lm[b];
    int I, J;
    tri_tile_ij(blockIdx.x, nT_grid, &I, &J);
    if (J >= lm_tiles(n)) return;
    const int tid = threadIdx.x;
    Rot2 q;
    double4_t opa = {0.0, 0.0, 0.0, 0.0}, opw = {0.0, 0.0, 0.0, 0.0};
    if (ANCHOR) {
        const double phi = filt_x(dv, b)[2];  // (k_reframe_finish zeroes it behind this kernel)
        q.c = cos(phi), q.s = sin(phi);
        if (tid < 128) {  // the operand rows of the tile's 64 rows and 64 columns: requested here, staged in LDS behind the tile's own loads
            const size_t rowi = (size_t)64 * (tid < 64 ? I : J) + (tid & 63);
            opa = *(const double4_t *)(dv.FA + (size_t)b * 2 * dv.f_stride + rowi * 4);
            opw = *(const double4_t *)(dv.FB + (size_t)b * 2 * dv.f_stride + rowi * 4);
        }
    } else {
        q.c = arg_value(one, fr, blockIdx.y, 2), q.s = arg_value(one, fr, blockIdx.y, 3);
    }
    const bool diag = I == J;
    double *tp = filt_Bm(dv, buf, b) + bm_tile_base(dv.T, I, J);
    ReframeItem it[2];
    bool live[2];
    double4_t v[2][2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        it[r] = reframe_item(r * 256 + tid);
        live[r] = !diag || (it[r].chain >> 2) < (it[r].chain & 3);
        if (live[r]) item_load(tp, it[r], v[r]);
    }
    if (ANCHOR) {
        if (tid < 128) {
            *(double4_t *)&ops[tid][0] = opa;
            *(double4_t *)&ops[tid][4] = opw;
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (!live[r]) continue;
        double o[2][4];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            double m[4];
            item_block(v[r], k, m);
            rot_block(q, m[0], m[1], m[2], m[3], o[k]);
            if (ANCHOR) {
                const double *r0 = ops[it[r].row[k]], *r1 = ops[it[r].row[k] + 1], *c0 = ops[64 + it[r].col], *c1 = ops[64 + it[r].col + 1];
                o[k][0] += cross_term(r0, c0), o[k][1] += cross_term(r0, c1);
                o[k][2] += cross_term(r1, c0), o[k][3] += cross_term(r1, c1);
            }
        }
        item_store(tp, it[r], o);
    }
    if (!diag) return;
    const int w = tid >> 6, a = (tid >> 3) & 7, c = tid & 7;  // wave w: chain (w, w); lane: block row a, block column c of its 8 x 8 blocks
    if (a > c) return;
    double *ch = tp + w * 5 * 256;
    int at[2][2], mirror[2][2];
    for (int d = 0; d < 2; d++)
        for (int e = 0; e < 2; e++) at[d][e] = bm_chain_offset(2 * a + d, 2 * c + e), mirror[d][e] = bm_chain_offset(2 * c + e, 2 * a + d);
    if (a == c) {
        const double *Dx = filt_D(dv, b);
        const int l = 32 * I + 8 * w + a;  // (l < dn = 32 T; zeros beyond the map)
        const double xy = Dx[dv.dn + l];
        ch[at[0][0]] = Dx[l], ch[at[0][1]] = xy, ch[at[1][0]] = xy, ch[at[1][1]] = Dx[2 * (size_t)dv.dn + l];
        return;
    }
    double o[4];
    rot_block(q, ch[at[0][0]], ch[at[0][1]], ch[at[1][0]], ch[at[1][1]], o);
    if (ANCHOR) {
        const double *r0 = ops[16 * w + 2 * a], *r1 = r0 + 8, *c0 = ops[64 + 16 * w + 2 * c], *c1 = c0 + 8;
        o[0] += cross_term(r0, c0), o[1] += cross_term(r0, c1), o[2] += cross_term(r1, c0), o[3] += cross_term(r1, c1);
    }
    for (int d = 0; d < 2; d++)
        for (int e = 0; e < 2; e++) ch[at[d][e]] = o[2 * d + e], ch[mirror[d][e]] = o[2 * d + e];
}

// Thread 0 of block blockIdx.x = filter b_off + blockIdx.x: the robot entries (pose, P_RR) and, as k_set_meta does behind a removal,
// the bookkeeping and the host mirror; the landmark count stays.
template <bool ANCHOR>
__global__ void k_reframe_finish(EkfDev dv, ReframeFrame one, const double *fr, int b_off) {
    if (threadIdx.x != 0) return;
    const int b = b_off + blockIdx.x;
    double *x = filt_x(dv, b);
    double *R0 = filt_R(dv, b);
    double p[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (ANCHOR) {
        x[0] = 0.0, x[1] = 0.0, x[2] = 0.0;
    } else {
        double f[5];
        for (int k = 0; k < 5; k++) f[k] = arg_value(one, fr, blockIdx.x, k);
        const Rot2 q = {f[2], f[3]};
        const double dx = x[0] - f[0], dy = x[1] - f[1];
        x[0] = q.c * dx + q.s * dy, x[1] = q.c * dy - q.s * dx, x[2] = x[2] - f[4];
        // J_R P_RR J_R^T, J_R = diag(Q, 1), from the upper triangle and mirrored
        double d[4];
        rot_block(q, R0[0], R0[1], R0[1], R0[(size_t)dv.xs + 1], d);
        const double p02 = R0[2], p12 = R0[(size_t)dv.xs + 2];
        p[0][0] = d[0], p[0][1] = p[1][0] = d[1], p[1][1] = d[3];
        p[0][2] = p[2][0] = q.c * p02 + q.s * p12;
        p[1][2] = p[2][1] = q.c * p12 - q.s * p02;
        p[2][2] = R0[2 * (size_t)dv.xs + 2];
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R0[(size_t)i * dv.xs + j] = p[i][j];
    settle_meta(dv, b, dv.n_lm[b], x, &p[0][0], 3);
}

// ---------------------------------------------------------------------------------------------
// Pose reset (ekf_reset_pose): x[0..2] <- pose, P_RR <- the caller's (symmetrised on the host), every robot-landmark block +0.0; the
// landmarks of x, D and Bm are not touched.  The three robot rows are the only copy of P_RL the kernels keep (the slot rows are
// cleared behind every rewrite), so one O(N) pass over them is all of it: thread j of filter b_off + blockIdx.y takes column j of the
// three rows; the thread of column 0 also stores the pose and does the bookkeeping of k_reframe_finish.  The per-filter argument is
// thirteen doubles: the pose, P_RR row-major, apply (0.0: the filter is left alone -- ekf_batch_relocalize's refused filters).
// ---------------------------------------------------------------------------------------------
struct ResetPose {
    double v[13];
};
__global__ __launch_bounds__(256) void k_reset_pose(EkfDev dv, ResetPose one, const double *tab, int b_off) {
    const int b = b_off + blockIdx.y;
    if (arg_value(one, tab, blockIdx.y, 12) == 0.0) return;
    const int n = dv.n_lm[b];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= 3 + 2 * n) return;
    double *R0 = filt_R(dv, b);
    for (int i = 0; i < 3; i++) R0[(size_t)i * dv.xs + j] = j < 3 ? arg_value(one, tab, blockIdx.y, 3 + 3 * i + j) : 0.0;
    if (j != 0) return;
    double *x = filt_x(dv, b);
    double p[9];
    for (int k = 0; k < 3; k++) x[k] = arg_value(one, tab, blockIdx.y, k);
    for (int k = 0; k < 9; k++) p[k] = arg_value(one, tab, blockIdx.y, 3 + k);
    settle_meta(dv, b, n, x, p, 3);
}

// ---------------------------------------------------------------------------------------------
// Map joining (ekf_join_map): the Ns landmarks of a source filter, expressed in the frame of the destination's estimated pose
// p = (t, phi), appended behind the destination's Ng landmarks; the old pose is marginalised out, the source's pose becomes the
// robot.  With C = Rot(phi), h_k = J C M_k (the third column of G_k = [I | C J M_k]) and g = J C u (of G_R):
//   new landmark k:  M_k' = t + C M_k,   P' blocks as in include/ekfslam_c.h.
// Per landmark-space row i' of the joined map the tile kernel needs four doubles, {w (3), h}: an old row's w = P_iR (its robot
// columns); a new row's h = h_k[e] and w = (row e of G_k) P_RR = P_RR[e] + h P_RR[2].  Element (i', j'), j' new, is then
// w_i[f] + w_i[2] h_j (f = j' & 1) -- plus, when i' is new too, the source's block rotated by C.
// Launch order on the destination's chain stream, every slot of BOTH filters folded in and all their streams idle:
//   k_join_tiles (the destination tiles that hold a new column; reads the old robot rows and the old P_RR)  ->  k_join_vec (x, D,
//   robot rows of the new landmarks, own blocks of the diagonal tiles; the robot rows of the OLD landmarks in place)  ->
//   k_join_finish (pose, P_RR, count, bookkeeping, host mirror).  Nothing is read after it was overwritten: the tile kernel
//   writes Bm only, k_join_vec reads the pose and P_RR and leaves them alone.
// The source is only read; its layout (strides of its own capacity) travels in JoinSrc.  cos / sin of the destination's heading are
// taken on the host: in the kernel arguments (`one`) for a one-filter call, in a table `rot` = [filters of the launch][2] for the
// batch form.  The launch covers destination filters bd0 + blockIdx.y and source filters bs0 + blockIdx.y.
// ---------------------------------------------------------------------------------------------
struct JoinSrc {
    const double *x, *R, *D, *Bm;  // the source handle's arrays, Bm = its settled buffer
    const int *n_lm;
    int xs, dn, T;
    size_t bm_stride;
};
__device__ __forceinline__ const double *filt_Bm(const JoinSrc &sv, int b) { return sv.Bm + (size_t)b * sv.bm_stride; }
// C of the launch's filter `by`, as the join carries it: {cos phi, sin phi}, C = [[c, -s], [s, c]] -- so C M C^T is rot_block with
// Q = {c, -s} (join_q).  Not arg_value: the copy and the plain inline keep the two halves of `one` two scalar loads in k_join_vec and
// k_join_finish, as they have been measured.
__device__ inline Rot2 join_c(const Rot2 &one, const double *rot, int by) {
    Rot2 q = one;
    if (rot) q.c = rot[2 * by], q.s = rot[2 * by + 1];
    return q;
}
__device__ __forceinline__ Rot2 join_q(const Rot2 q) { return {q.c, -q.s}; }

// {w0, w1, w2, h} of landmark-space row ip of the joined map (zeros beyond it), from the destination's OLD robot entries
__device__ inline void join_operand(const EkfDev &dv, const JoinSrc &sv, int bd, int bs, Rot2 q, int Ng, int Ns, int ip, double op[4]) {
    const double *R0 = filt_R(dv, bd);
    const int l = ip >> 1, e = ip & 1;
    op[0] = op[1] = op[2] = op[3] = 0.0;
    if (l < Ng) {
        for (int k = 0; k < 3; k++) op[k] = R0[(size_t)k * dv.xs + 3 + ip];
    } else if (l < Ng + Ns) {
        const double *m = filt_x(sv, bs) + 3 + 2 * (l - Ng);
        const double h = e ? q.c * m[0] - q.s * m[1] : -(q.s * m[0] + q.c * m[1]);
        for (int k = 0; k < 3; k++) op[k] = R0[(size_t)e * dv.xs + k] + h * R0[2 * (size_t)dv.xs + k];
        op[3] = h;
    }
}

// One workgroup per destination tile that holds a new column (ekf_device.h: join_tile_ij) and filter pair, in place in Bm[buf].
// The tile is walked in the frame changes' work items (reframe_item: a lane owns whole 2x2 blocks and stores 32-byte pieces, a
// wave whole 256-byte runs); every block is classified by join_source.  Old x old blocks of a straddling tile are loaded and
// stored back unchanged, stale places included; in a diagonal tile the places below the diagonal get the transposed upper value
// (the same expression, so the same bits) as k_import stores them, and a new landmark's own block is left to k_join_vec.
__global__ __launch_bounds__(256) void k_join_tiles(EkfDev dv, int buf, JoinSrc sv, Rot2 one, const double *rot, int bd0, int bs0) {
    __shared__ double ops[128][4];  // [tile row | 64 + tile column]{w0, w1, w2, h}
    const int bd = bd0 + blockIdx.y, bs = bs0 + blockIdx.y;
    const int Ng = dv.n_lm[bd], Ns = sv.n_lm[bs];
    if (Ns <= 0) return;
    int I, J;
    if (!join_tile_ij(blockIdx.x, Ng >> 5, lm_tiles(Ng + Ns), &I, &J)) return;
    const int tid = threadIdx.x;
    const Rot2 q = join_c(one, rot, blockIdx.y);
    if (tid < 128) {
        double op[4];
        join_operand(dv, sv, bd, bs, q, Ng, Ns, 64 * (tid < 64 ? I : J) + (tid & 63), op);
        *(double4_t *)&ops[tid][0] = (double4_t){op[0], op[1], op[2], op[3]};
    }
    __syncthreads();
    const Rot2 cq = join_q(q);
    double *tp = filt_Bm(dv, buf, bd) + bm_tile_base(dv.T, I, J);
    const double *sb = filt_Bm(sv, bs);
    ReframeItem it[2];
    double o[2][2][4];  // [item][block]{(0,0), (0,1), (1,0), (1,1)}
#pragma unroll
    for (int r = 0; r < 2; r++) {
        it[r] = reframe_item(r * 256 + tid);
        const int lc = 32 * J + (it[r].col >> 1);
        JoinSource src[2];
        bool swap[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int lr = 32 * I + (it[r].row[k] >> 1);
            swap[k] = lr > lc;  // (a diagonal tile's places below the diagonal)
            src[k] = join_source(Ng, Ns, sv.T, sv.dn, 2 * (swap[k] ? lc : lr), 2 * (swap[k] ? lr : lc));
        }
        double4_t v[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        if (src[0].where == JM_OLD || src[1].where == JM_OLD) item_load(tp, it[r], v);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            double *ob = o[r][k];
            ob[0] = ob[1] = ob[2] = ob[3] = 0.0;  // beyond the joined map; a new landmark's own block (k_join_vec)
            if (src[k].where == JM_OLD) {
                item_block(v, k, ob);
            } else if (src[k].where == JM_ROBOT || src[k].where == JM_BM) {
                const int ri = swap[k] ? 64 + it[r].col : it[r].row[k], ci = swap[k] ? it[r].row[k] : 64 + it[r].col;
                double g[2][2];
                for (int e = 0; e < 2; e++)
                    for (int f = 0; f < 2; f++) g[e][f] = ops[ri + e][f] + ops[ri + e][2] * ops[ci + f][3];
                if (src[k].where == JM_BM) {
                    const double *m = sb + src[k].off;
                    double rb[4];
                    rot_block(cq, m[0], m[2], m[32], m[34], rb);
                    g[0][0] += rb[0], g[0][1] += rb[1], g[1][0] += rb[2], g[1][1] += rb[3];
                }
                ob[0] = g[0][0], ob[3] = g[1][1];
                ob[1] = swap[k] ? g[1][0] : g[0][1], ob[2] = swap[k] ? g[0][1] : g[1][0];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; r++) item_store(tp, it[r], o[r]);
}

// One thread per landmark of the joined map.  An old landmark: its robot rows P_mR G_R^T, in place.  New landmark k: position, own
// block (into D and into its stale place of the diagonal tile, as k_import stores it) and robot rows
// G_k P_RR G_R^T + C P_s,kR C3^T.  Reads the destination's pose and P_RR and the source, writes neither.
__global__ __launch_bounds__(256) void k_join_vec(EkfDev dv, int buf, JoinSrc sv, Rot2 one, const double *rot, int bd0, int bs0) {
    const int bd = bd0 + blockIdx.y, bs = bs0 + blockIdx.y;
    const int Ng = dv.n_lm[bd], Ns = sv.n_lm[bs];
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= Ng + Ns) return;
    const Rot2 q = join_c(one, rot, blockIdx.y);
    double *x = filt_x(dv, bd);
    double *R0 = filt_R(dv, bd);
    const double *sx = filt_x(sv, bs);
    const double *sR = filt_R(sv, bs);
    const double g0 = -(q.s * sx[0] + q.c * sx[1]), g1 = q.c * sx[0] - q.s * sx[1];  // C J u
    if (l < Ng) {
        for (int e = 0; e < 2; e++) {
            const size_t c = 3 + 2 * (size_t)l + e;
            const double r0 = R0[c], r1 = R0[dv.xs + c], r2 = R0[2 * (size_t)dv.xs + c];
            R0[c] = r0 + r2 * g0, R0[dv.xs + c] = r1 + r2 * g1;
        }
        return;
    }
    const int k = l - Ng;
    const double mx = sx[3 + 2 * k], my = sx[4 + 2 * k];
    const double cx = q.c * mx - q.s * my, cy = q.s * mx + q.c * my;
    const double h[2] = {-cy, cx};
    double w[2][3];
    for (int e = 0; e < 2; e++)
        for (int j = 0; j < 3; j++) w[e][j] = R0[(size_t)e * dv.xs + j] + h[e] * R0[2 * (size_t)dv.xs + j];
    const Rot2 cq = join_q(q);
    const double *sD = filt_D(sv, bs);
    const double sxy = sD[sv.dn + k];
    double d[4];
    rot_block(cq, sD[k], sxy, sxy, sD[2 * (size_t)sv.dn + k], d);
    const double dxx = (w[0][0] + w[0][2] * h[0]) + d[0], dxy = (w[0][1] + w[0][2] * h[1]) + d[1], dyy = (w[1][1] + w[1][2] * h[1]) + d[3];
    double p[3][2];  // P_s,Rk
    for (int j = 0; j < 3; j++) p[j][0] = sR[(size_t)j * sv.xs + 3 + 2 * k], p[j][1] = sR[(size_t)j * sv.xs + 4 + 2 * k];
    double rr[3][2];
    for (int e = 0; e < 2; e++) {
        double cp[3];  // row e of C P_s,kR
        for (int j = 0; j < 3; j++) cp[j] = e ? q.s * p[j][0] + q.c * p[j][1] : q.c * p[j][0] - q.s * p[j][1];
        rr[0][e] = (w[e][0] + w[e][2] * g0) + (cp[0] * q.c - cp[1] * q.s);
        rr[1][e] = (w[e][1] + w[e][2] * g1) + (cp[0] * q.s + cp[1] * q.c);
        rr[2][e] = w[e][2] + cp[2];
    }
    x[3 + 2 * l] = x[0] + cx, x[4 + 2 * l] = x[1] + cy;
    for (int j = 0; j < 3; j++) R0[(size_t)j * dv.xs + 3 + 2 * l] = rr[j][0], R0[(size_t)j * dv.xs + 4 + 2 * l] = rr[j][1];
    double *Dx = filt_D(dv, bd);
    Dx[l] = dxx, Dx[dv.dn + l] = dxy, Dx[2 * (size_t)dv.dn + l] = dyy;
    double *own = filt_Bm(dv, buf, bd) + bm_offset(dv.T, 2 * l, 2 * l);
    own[0] = dxx, own[2] = dxy, own[32] = dxy, own[34] = dyy;
}

// Thread 0 of block blockIdx.x: the robot entries t' = t + C u, phi' = phi + psi, P_RR' = G_R P_RR G_R^T + C3 P_s,RR C3^T (the
// upper triangle, mirrored), the new landmark count and k_set_meta's bookkeeping and host mirror.
__global__ void k_join_finish(EkfDev dv, JoinSrc sv, Rot2 one, const double *rot, int bd0, int bs0) {
    if (threadIdx.x != 0) return;
    const int bd = bd0 + blockIdx.x, bs = bs0 + blockIdx.x;
    const Rot2 q = join_c(one, rot, blockIdx.x);
    double *x = filt_x(dv, bd);
    double *R0 = filt_R(dv, bd);
    const double *sx = filt_x(sv, bs);
    const double *sR = filt_R(sv, bs);
    const double ux = sx[0], uy = sx[1];
    const double g[2] = {-(q.s * ux + q.c * uy), q.c * ux - q.s * uy};
    double P[3][3], S[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = i; j < 3; j++) P[i][j] = P[j][i] = R0[(size_t)i * dv.xs + j], S[i][j] = S[j][i] = sR[(size_t)i * sv.xs + j];
    double A[3][3];  // G_R P
    for (int j = 0; j < 3; j++) A[0][j] = P[0][j] + g[0] * P[2][j], A[1][j] = P[1][j] + g[1] * P[2][j], A[2][j] = P[2][j];
    const Rot2 cq = join_q(q);
    double d[4];
    rot_block(cq, S[0][0], S[0][1], S[0][1], S[1][1], d);
    double p[3][3];
    p[0][0] = (A[0][0] + A[0][2] * g[0]) + d[0];
    p[0][1] = p[1][0] = (A[0][1] + A[0][2] * g[1]) + d[1];
    p[1][1] = (A[1][1] + A[1][2] * g[1]) + d[3];
    p[0][2] = p[2][0] = A[0][2] + (q.c * S[0][2] - q.s * S[1][2]);
    p[1][2] = p[2][1] = A[1][2] + (q.s * S[0][2] + q.c * S[1][2]);
    p[2][2] = A[2][2] + S[2][2];
    const double tx = x[0] + (q.c * ux - q.s * uy), ty = x[1] + (q.s * ux + q.c * uy);
    x[0] = tx, x[1] = ty, x[2] = x[2] + sx[2];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R0[(size_t)i * dv.xs + j] = p[i][j];
    const int n_lm = dv.n_lm[bd] + sv.n_lm[bs];
    dv.n_lm[bd] = n_lm;
    settle_meta(dv, bd, n_lm, x, &p[0][0], 3);
}

// ---------------------------------------------------------------------------------------------
// Landmark initialisation (ekf_add_landmarks): the m measurements of a table become landmarks Ng .. Ng + m - 1, all linearised at
// the entry state -- the join of a source x = (0, 0, 0, z_0, z_1, ..), P_s = blockdiag(0_3, R_0, R_1, ..) (u = 0, so G_R = I: the
// pose, P_RR and every old row stay untouched) without the source.  With C = Rot(phi), h_k = C J z_k, G_k = [I | h_k]:
//   L_k = p + C z_k,   P[k, robot] = G_k P_RR,   P[k, old m] = G_k P_R,m,   P[k, l] = G_k P_RR G_l^T + [k == l] C R_k C^T.
// Per landmark-space row i' the tile kernel needs the join's four doubles {w (3), h}: an old row's w = P_iR; a new row's h = h_k[e]
// and w = P_RR[e] + h P_RR[2].  Element (i', j'), j' new, is w_i[f] + w_i[2] h_j (f = j' & 1).
// Launch order on the chain stream, every slot folded in and both streams idle:
//   k_add_vec (a thread per new landmark: x, the three robot-row entries, D, and its two operand rows into AddScratch::ops; reads
//   the pose and P_RR)  ->  k_add_tiles (the tiles that hold a new column, join_tile_ij; reads the old robot rows, the operand rows
//   and the new D)  ->  k_add_finish (count, bookkeeping, host mirror).  Nothing that is read is ever written: the pose, P_RR and the
//   old landmarks' robot rows stay as they are.  cos / sin of the heading are taken on the device, sincos(x[2]) as the chain kernels
//   take them, in k_add_vec alone: the tiles see them through the operand rows.
// The table (ekf_device.h: add_tab_stride) and the operand rows live in a scratch the handle keeps; a record's count is a double.
// The launch covers filters b0 + blockIdx.y.
// ---------------------------------------------------------------------------------------------
#include "ekf_map_scratch.h"  // AddScratch
__device__ __forceinline__ const double *add_record(const AddScratch &as, int b) { return as.tab + (size_t)b * add_tab_stride(as.zcap); }

__global__ __launch_bounds__(64) void k_add_vec(EkfDev dv, AddScratch as, int b0) {
    const int b = b0 + blockIdx.y;
    const double *rec = add_record(as, b);
    const int m = (int)rec[0], Ng = dv.n_lm[b];
    const int k = blockIdx.x * 64 + threadIdx.x;
    const int l = Ng + k;
    if (k >= m || k >= as.zcap || l >= dv.Ncap) return;  // (the host has checked the room: no thread leaves here)
    double *x = filt_x(dv, b);
    double *R0 = filt_R(dv, b);
    double s, c;
    sincos(x[2], &s, &c);
    const double *e = rec + 2 + 6 * (size_t)k;
    const double zx = e[0], zy = e[1];
    const double cx = c * zx - s * zy, cy = s * zx + c * zy;
    const double h[2] = {-cy, cx};
    double w[2][3];
    for (int r = 0; r < 2; r++)
        for (int j = 0; j < 3; j++) w[r][j] = R0[(size_t)r * dv.xs + j] + h[r] * R0[2 * (size_t)dv.xs + j];
    const double rxy = 0.5 * (e[3] + e[4]);  // only the symmetric part of R enters (Update.cpp:193)
    double d[4];
    rot_block(Rot2{c, -s}, e[2], rxy, rxy, e[5], d);  // C R C^T
    const double dxx = (w[0][0] + w[0][2] * h[0]) + d[0], dxy = (w[0][1] + w[0][2] * h[1]) + d[1], dyy = (w[1][1] + w[1][2] * h[1]) + d[3];
    x[3 + 2 * l] = x[0] + cx, x[4 + 2 * l] = x[1] + cy;
    for (int j = 0; j < 3; j++) R0[(size_t)j * dv.xs + 3 + 2 * l] = w[0][j], R0[(size_t)j * dv.xs + 4 + 2 * l] = w[1][j];
    double *Dx = filt_D(dv, b);
    Dx[l] = dxx, Dx[dv.dn + l] = dxy, Dx[2 * (size_t)dv.dn + l] = dyy;
    double *op = as.ops + ((size_t)b * as.zcap + k) * 8;
    for (int r = 0; r < 2; r++) *(double4_t *)(op + 4 * r) = (double4_t){w[r][0], w[r][1], w[r][2], h[r]};
}

// One workgroup per tile that holds a new column and filter, in place in Bm[buf], walked and stored as k_join_tiles walks its tiles
// (reframe_item; join_where with m in place of the source's count classifies the blocks).  Old x old blocks of a straddling tile
// are loaded and stored back unchanged, stale places included; the places below the diagonal of a diagonal tile get the transposed
// upper value (the same expression, so the same bits) and a new landmark's own block the new D, as k_import stores them.
__global__ __launch_bounds__(256) void k_add_tiles(EkfDev dv, int buf, AddScratch as, int b0) {
    __shared__ double ops[128][4];  // [tile row | 64 + tile column]{w0, w1, w2, h}
    const int b = b0 + blockIdx.y;
    const int m = (int)add_record(as, b)[0], Ng = dv.n_lm[b];
    if (m <= 0 || m > as.zcap || Ng + m > dv.Ncap) return;
    int I, J;
    if (!join_tile_ij(blockIdx.x, Ng >> 5, lm_tiles(Ng + m), &I, &J)) return;
    const int tid = threadIdx.x;
    if (tid < 128) {
        const int ip = 64 * (tid < 64 ? I : J) + (tid & 63), l = ip >> 1;
        double4_t op = {0.0, 0.0, 0.0, 0.0};  // (beyond the map)
        if (l < Ng) {
            const double *R0 = filt_R(dv, b);
            op = (double4_t){R0[3 + ip], R0[(size_t)dv.xs + 3 + ip], R0[2 * (size_t)dv.xs + 3 + ip], 0.0};
        } else if (l < Ng + m) {
            op = *(const double4_t *)(as.ops + ((size_t)b * as.zcap + (l - Ng)) * 8 + 4 * (ip & 1));
        }
        *(double4_t *)&ops[tid][0] = op;
    }
    __syncthreads();
    double *tp = filt_Bm(dv, buf, b) + bm_tile_base(dv.T, I, J);
    const double *Dx = filt_D(dv, b);
    ReframeItem it[2];
    double o[2][2][4];  // [item][block]{(0,0), (0,1), (1,0), (1,1)}
#pragma unroll
    for (int r = 0; r < 2; r++) {
        it[r] = reframe_item(r * 256 + tid);
        const int lc = 32 * J + (it[r].col >> 1);
        int lr[2], where[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            lr[k] = 32 * I + (it[r].row[k] >> 1);
            where[k] = join_where(Ng, m, lr[k] > lc ? lc : lr[k], lr[k] > lc ? lr[k] : lc);
        }
        double4_t v[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        if (where[0] == JM_OLD || where[1] == JM_OLD) item_load(tp, it[r], v);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            double *ob = o[r][k];
            ob[0] = ob[1] = ob[2] = ob[3] = 0.0;  // beyond the new map
            const bool swap = lr[k] > lc;         // (a diagonal tile's places below the diagonal)
            if (where[k] == JM_OLD) {
                item_block(v, k, ob);
            } else if (where[k] == JM_D) {
                const double xy = Dx[dv.dn + lc];
                ob[0] = Dx[lc], ob[1] = xy, ob[2] = xy, ob[3] = Dx[2 * (size_t)dv.dn + lc];
            } else if (where[k] == JM_ROBOT || where[k] == JM_BM) {
                const int ri = swap ? 64 + it[r].col : it[r].row[k], ci = swap ? it[r].row[k] : 64 + it[r].col;
                double g[2][2];
                for (int e = 0; e < 2; e++)
                    for (int f = 0; f < 2; f++) g[e][f] = ops[ri + e][f] + ops[ri + e][2] * ops[ci + f][3];
                ob[0] = g[0][0], ob[3] = g[1][1];
                ob[1] = swap ? g[1][0] : g[0][1], ob[2] = swap ? g[0][1] : g[1][0];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; r++) item_store(tp, it[r], o[r]);
}

// Thread 0 of block blockIdx.x: the new landmark count and k_set_meta's bookkeeping and host mirror (pose and P_RR as they lie).
__global__ void k_add_finish(EkfDev dv, AddScratch as, int b0) {
    if (threadIdx.x != 0) return;
    const int b = b0 + blockIdx.x;
    const int m = (int)add_record(as, b)[0];
    const int n_lm = dv.n_lm[b] + (m > 0 && m <= as.zcap && dv.n_lm[b] + m <= dv.Ncap ? m : 0);
    dv.n_lm[b] = n_lm;
    settle_meta(dv, b, n_lm, filt_x(dv, b), filt_R(dv, b), dv.xs);
}
