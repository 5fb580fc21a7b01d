// ekf_locate.hip -- the scan-to-map pose search on the device (ekf_locate_scan): brute-force Euclidean geometry over landmark pairs.
// Only x of the filter is read, which the chain kernels keep current inside an open window: no fold, no pass, nothing written but
// the call's own scratch (LocScratch, ekf_map_scratch.h).  The definition -- base pairs, candidates, pair pose, score, order,
// refit -- is in include/ekfslam_c.h; the base pairs come from the host (plan_locate_table, ekf_map_plan.h).
//
// Once per call, the chain stream idle.  Included by ekf_api.hip behind ekf_kernels.hip (wave_argmin, double2_t) and ekf_rewrite.hip
// (filt_x).  A candidate is one 32-bit key, r << 28 | i << 14 | j (r < 16 base pairs, i, j < EKF_MAX_CAPACITY = 16000 < 2^14), whose
// integer order is the (r, i, j) order of the definition.
//
//   k_loc_pairs   grid (ceil(N / 256), ceil(N / 256), filters): a thread holds landmark i, the workgroup walks 256 landmarks j
//                 staged in LDS; the length |L_j - L_i| is taken once per pair and compared with every base pair's separation;
//                 a passing (r, i, j) is appended with one INTEGER atomic per wave (ballot, prefix popcount), as k_gate appends.
//   k_loc_score   the hot path, candidates x n_z x N fp64 distance tests.  A workgroup of four waves stages the map's (x, y) pairs
//                 in LDS once (LOC_LDS_LM = 4096 landmarks, 64 KB; a larger map is walked in chunks, staged again per chunk) and
//                 takes many candidates, one per wave at a time.  A lane walks the landmarks 64 apart, four per step (one 16-byte
//                 LDS load each), and keeps the running minimum (d2, index) of EVERY measurement in registers -- KMAX of them, the
//                 kernel is instantiated for 8, 16 and 32; the measurements' transformed positions are read from LDS as wave-wide
//                 broadcasts, once per four landmarks.  A lane's landmarks ascend and its test is a strict <, the cross-lane
//                 reduction (wave_argmin: the DPP steps, then cand_better) breaks ties to the lower index; measurement k's winner
//                 ends in lane k.  The one-to-one pass and the sums run across those lanes by shuffles in ascending k: the order
//                 one lane would take.
//   k_loc_pick    top-max_out selection by (inliers descending, ssr ascending, key ascending), twice: LOC_PICK_PARTS workgroups
//                 per filter select from their slice of the list into partial lists, one workgroup merges those.  A round picks the
//                 best entry that is WORSE than the round before's pick: the order is total and strict (keys are unique), so
//                 nothing is marked, the rounds' result does not depend on where an entry was appended, and no score travels to
//                 the host.
//   k_loc_fit     one wave per selected hypothesis: scores it again from x in global memory (the same expressions, so the same
//                 bits and the same inliers), writes the ids, the closed-form refit and the record.
// Every value written is a function of the candidate alone or comes out of a fixed-order reduction: the same bits on every call and
// in the batch form.

#include "ekf_map_scratch.h"  // LocScratch, LOC_THREADS, LOC_LDS_LM, LOC_PICK_PARTS

typedef double double2_u __attribute__((ext_vector_type(2), aligned(8)));  // (x + 3 + 2 l is 8-byte aligned only)

#define LOC_FAR 1e300  // a landmark slot behind the map: its squared distance is +inf, which is below no running minimum

__device__ __forceinline__ unsigned loc_key(int r, int i, int j) { return ((unsigned)r << 28) | ((unsigned)i << 14) | (unsigned)j; }

struct LocPose {
    double c, s, px, py, dot, crs;
};
// The pair pose of measurements za, zb (separation blen) on landmarks Li, Lj: include/ekfslam_c.h.
__device__ __forceinline__ LocPose loc_pair_pose(double2_t za, double2_t zb, double blen, double2_t Li, double2_t Lj) {
    const double dzx = zb.x - za.x, dzy = zb.y - za.y, dlx = Lj.x - Li.x, dly = Lj.y - Li.y;
    const double q = blen * sqrt(dlx * dlx + dly * dly);
    LocPose p;
    p.dot = dzx * dlx + dzy * dly, p.crs = dzx * dly - dzy * dlx;
    p.c = p.dot / q, p.s = p.crs / q;
    const double mx = 0.5 * (za.x + zb.x), my = 0.5 * (za.y + zb.y);
    p.px = 0.5 * (Li.x + Lj.x) - (p.c * mx - p.s * my);
    p.py = 0.5 * (Li.y + Lj.y) - (p.s * mx + p.c * my);
    return p;
}
// ... of candidate `key` of filter b, whose compacted measurements are zf and landmarks x3 = x + 3.
__device__ __forceinline__ LocPose loc_pose_of(const LocScratch &ls, int b, unsigned key, const double *zf, const double *x3) {
    const int r = (int)(key >> 28), i = (int)((key >> 14) & 0x3fff), j = (int)(key & 0x3fff);
    const int *bp = ls.base + ((size_t)b * EKF_LOCATE_MAX_BASE + r) * 2;
    const double2_t za = *(const double2_t *)(zf + 2 * bp[0]), zb = *(const double2_t *)(zf + 2 * bp[1]);
    const double2_u Li = *(const double2_u *)(x3 + 2 * i), Lj = *(const double2_u *)(x3 + 2 * j);
    return loc_pair_pose(za, zb, ls.blen[(size_t)b * EKF_LOCATE_MAX_BASE + r], (double2_t){Li.x, Li.y}, (double2_t){Lj.x, Lj.y});
}

__global__ __launch_bounds__(LOC_THREADS) void k_loc_pairs(EkfDev dv, LocScratch ls, double two_tol, int b_off) {
    __shared__ double2_t lj[LOC_THREADS];
    __shared__ double bl[EKF_LOCATE_MAX_BASE];
    const int b = b_off + blockIdx.z;
    const int n = dv.n_lm[b] < dv.Ncap ? dv.n_lm[b] : dv.Ncap;
    const int nbase = ls.nbase[b] < EKF_LOCATE_MAX_BASE ? ls.nbase[b] : EKF_LOCATE_MAX_BASE;
    const int i0 = blockIdx.x * LOC_THREADS, j0 = blockIdx.y * LOC_THREADS;
    if (nbase <= 0 || n < 2 || i0 >= n || j0 >= n) return;  // (the whole workgroup)
    const int tid = threadIdx.x, lane = tid & 63;
    const double *x3 = filt_x(dv, b) + 3;
    const int i = i0 + tid;
    const bool have = i < n;
    double2_t Li = {0.0, 0.0};
    if (have) {
        const double2_u v = *(const double2_u *)(x3 + 2 * i);
        Li = (double2_t){v.x, v.y};
    }
    {
        const int j = j0 + tid;
        double2_t v = {0.0, 0.0};
        if (j < n) {
            const double2_u u = *(const double2_u *)(x3 + 2 * j);
            v = (double2_t){u.x, u.y};
        }
        lj[tid] = v;
        if (tid < EKF_LOCATE_MAX_BASE) bl[tid] = tid < nbase ? ls.blen[(size_t)b * EKF_LOCATE_MAX_BASE + tid] : 0.0;
    }
    __syncthreads();
    const int jn = n - j0 < LOC_THREADS ? n - j0 : LOC_THREADS;
    unsigned long long *cnt = ls.cnt + b;
    unsigned *list = ls.key + (size_t)b * ls.ccap;
    for (int q = 0; q < jn; q++) {  // (workgroup-uniform: all 64 lanes of every wave are active at the ballots)
        const double2_t L = lj[q];
        const double dx = L.x - Li.x, dy = L.y - Li.y;
        const double len = sqrt(dx * dx + dy * dy);
        const bool pair = have && i != j0 + q;
        for (int r = 0; r < nbase; r++) {
            const bool listed = pair && fabs(len - bl[r]) <= two_tol;
            const unsigned long long lmask = __ballot(listed);
            if (lmask) {  // (wave-uniform) one integer atomic per wave; a lane's place = the listed lanes below it
                const int leader = __builtin_ctzll(lmask);
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(cnt, (unsigned long long)__popcll(lmask));
                base = ((unsigned long long)(unsigned)__shfl((int)(base >> 32), leader) << 32) | (unsigned)__shfl((int)base, leader);
                const unsigned long long at = base + __builtin_amdgcn_mbcnt_hi((unsigned)(lmask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)lmask, 0u));
                if (listed && at < (unsigned long long)ls.ccap) list[at] = loc_key(r, i, j0 + q);
            }
        }
    }
}

// The running minima of KMAX measurements over the landmark slots [0, count) of `src` (count a multiple of 256; slot t is landmark
// first + t), the lane's share: slots lane + 64 u.  tz: the measurements' transformed positions (wave-uniform reads).
template <int KMAX, typename Src>
__device__ __forceinline__ void loc_scan(const Src &src, int count, int first, const double (*tz)[2], int nz, int lane, double (&best)[KMAX], int (&idx)[KMAX]) {
    for (int t0 = 0; t0 < count; t0 += 256) {
        double2_t L[4];
#pragma unroll
        for (int u = 0; u < 4; u++) L[u] = src(t0 + u * 64 + lane);
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            if (k < nz) {  // (wave-uniform)
                const double tx = tz[k][0], ty = tz[k][1];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const double dx = tx - L[u].x, dy = ty - L[u].y;
                    const double d = dx * dx + dy * dy;
                    const bool take = d < best[k];
                    best[k] = take ? d : best[k], idx[k] = take ? first + t0 + u * 64 + lane : idx[k];
                }
            }
        }
    }
}

struct LocMatch {
    double d2;  // lane k: measurement k's nearest squared distance
    int lm;     // ... its landmark
    bool win;   // ... is an inlier after the one-to-one pass
    int inliers;
    double ssr;
};
// From the lanes' minima to the match: the cross-lane arg-min per measurement (ties: the lower index), measurement k's into lane k;
// inlier iff d2 <= tol^2; of several inliers naming one landmark the smallest distance keeps it (ties: the lower k); the count and
// the sum in ascending k.  All 64 lanes active.
template <int KMAX>
__device__ __forceinline__ LocMatch loc_resolve(double (&best)[KMAX], int (&idx)[KMAX], int nz, double tol_sq, int lane) {
    LocMatch m = {INFINITY, 0x7fffffff, false, 0, 0.0};
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        if (k < nz) {
            double d = best[k];
            int i = idx[k], who = lane;
            wave_argmin(d, i, who);
            if (lane == k) m.d2 = d, m.lm = i;
        }
    }
    const bool inl = lane < nz && m.d2 <= tol_sq;
    bool lose = false;
    for (int k = 0; k < nz; k++) {
        const double od = __shfl(m.d2, k);
        const int oi = __shfl(m.lm, k), oin = __shfl((int)inl, k);
        lose = lose || (k != lane && oin && oi == m.lm && (od < m.d2 || (od == m.d2 && k < lane)));
    }
    m.win = inl && !lose;
    m.inliers = __popcll(__ballot(m.win));
    for (int k = 0; k < nz; k++) m.ssr += __shfl(m.win ? m.d2 : 0.0, k);  // (x + 0.0 == x: the sum over the inliers in ascending k)
    return m;
}

template <int KMAX>
__global__ __launch_bounds__(LOC_THREADS) void k_loc_score(EkfDev dv, LocScratch ls, double tol_sq, int b_off) {
    __shared__ double2_t lm[LOC_LDS_LM];
    __shared__ double tz[LOC_THREADS / 64][KMAX][2];
    const int b = b_off + blockIdx.y;
    const int n = dv.n_lm[b] < dv.Ncap ? dv.n_lm[b] : dv.Ncap;
    const int nz = ls.nz[b] < KMAX ? ls.nz[b] : KMAX;
    const unsigned long long found = ls.cnt[b];
    const int cnt = found < (unsigned long long)ls.ccap ? (int)found : ls.ccap;
    const int per = LOC_THREADS / 64;
    if ((int)blockIdx.x * per >= cnt || n < 2) return;  // (the whole workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *x3 = filt_x(dv, b) + 3, *zf = ls.z + (size_t)b * EKF_MAX_PENDING * 2;
    const unsigned *keys = ls.key + (size_t)b * ls.ccap;
    const int nchunk = (n + LOC_LDS_LM - 1) / LOC_LDS_LM;
    const auto src = [&](int t) { return lm[t]; };
    bool staged = false;
    for (int c0 = (int)blockIdx.x * per; c0 < cnt; c0 += (int)gridDim.x * per) {  // (workgroup-uniform trip count)
        const int ci = c0 + wave;
        const bool live = ci < cnt;  // (wave-uniform)
        const LocPose p = loc_pose_of(ls, b, keys[live ? ci : c0], zf, x3);
        if (lane < nz) {
            const double zx = zf[2 * lane], zy = zf[2 * lane + 1];
            tz[wave][lane][0] = p.px + (p.c * zx - p.s * zy), tz[wave][lane][1] = p.py + (p.s * zx + p.c * zy);
        }
        double best[KMAX];
        int idx[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; k++) best[k] = INFINITY, idx[k] = 0x7fffffff;
        for (int ch = 0; ch < nchunk; ch++) {
            const int first = ch * LOC_LDS_LM;
            const int used = n - first < LOC_LDS_LM ? n - first : LOC_LDS_LM, count = (used + 255) & ~255;
            if (nchunk > 1 || !staged) {
                __syncthreads();  // (the chunk before has been read)
                for (int t = tid; t < count; t += LOC_THREADS) {
                    double2_t v = {LOC_FAR, LOC_FAR};
                    if (t < used) {
                        const double2_u u = *(const double2_u *)(x3 + 2 * (size_t)(first + t));
                        v = (double2_t){u.x, u.y};
                    }
                    lm[t] = v;
                }
                staged = true;
            }
            __syncthreads();  // (the chunk, and this round's tz)
            loc_scan<KMAX>(src, count, first, tz[wave], nz, lane, best, idx);
        }
        const LocMatch m = loc_resolve<KMAX>(best, idx, nz, tol_sq, lane);
        if (live && lane == 0) ls.inl[(size_t)b * ls.ccap + ci] = m.inliers, ls.ssr[(size_t)b * ls.ccap + ci] = m.ssr;
    }
}

// a is in front of b in the order of the hypotheses
__device__ __forceinline__ bool loc_before(int ia, double sa, unsigned ka, int ib, double sb, unsigned kb) {
    return (ia > ib) | ((ia == ib) & ((sa < sb) | ((sa == sb) & (ka < kb))));
}

// stage 0: workgroup g of filter b selects the first max_out of its slice of the list into partial list g; stage 1: workgroup 0
// merges the partial lists into the selection.  Entries that do not exist are written with inliers = -1.
__global__ __launch_bounds__(LOC_THREADS) void k_loc_pick(LocScratch ls, int stage, int max_out, int b_off) {
    __shared__ int wi[LOC_THREADS / 64];
    __shared__ double wsr[LOC_THREADS / 64];
    __shared__ unsigned wk[LOC_THREADS / 64];
    const int b = b_off + blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const unsigned long long found = ls.cnt[b];
    const int cnt = found < (unsigned long long)ls.ccap ? (int)found : ls.ccap;
    int parts = (cnt + 4095) / 4096;
    parts = parts < LOC_PICK_PARTS ? parts : LOC_PICK_PARTS;
    const size_t sel = (size_t)b * EKF_LOCATE_MAX_OUT, part0 = sel * LOC_PICK_PARTS;
    const int *inl;
    const double *ssr;
    const unsigned *key;
    int lo, hi, *oi;
    double *os;
    unsigned *ok;
    if (stage == 0) {
        if (g >= parts) return;
        const int slice = (cnt + parts - 1) / parts;
        lo = g * slice, hi = lo + slice < cnt ? lo + slice : cnt;
        inl = ls.inl + (size_t)b * ls.ccap, ssr = ls.ssr + (size_t)b * ls.ccap, key = ls.key + (size_t)b * ls.ccap;
        oi = ls.pinl + part0 + (size_t)g * EKF_LOCATE_MAX_OUT, os = ls.pssr + part0 + (size_t)g * EKF_LOCATE_MAX_OUT, ok = ls.pkey + part0 + (size_t)g * EKF_LOCATE_MAX_OUT;
    } else {
        if (g > 0) return;
        lo = 0, hi = parts * max_out;
        inl = ls.pinl + part0, ssr = ls.pssr + part0, key = ls.pkey + part0;
        oi = ls.winl + sel, os = ls.wssr + sel, ok = ls.wkey + sel;
    }
    int li = 0x7fffffff;  // the pick of the round before: in front of every entry
    double lsr = -INFINITY;
    unsigned lk = 0;
    for (int t = 0; t < max_out; t++) {  // (workgroup-uniform)
        int bi = -1;
        double bs = INFINITY;
        unsigned bk = 0xffffffffu;
        for (int q = lo + tid; q < hi; q += LOC_THREADS) {
            const int e = stage ? (q / max_out) * EKF_LOCATE_MAX_OUT + q % max_out : q;  // (a partial list's first max_out entries are written)
            const int ei = inl[e];
            const double es = ssr[e];
            const unsigned ek = key[e];
            if (ei >= 0 && loc_before(li, lsr, lk, ei, es, ek) && (bi < 0 || loc_before(ei, es, ek, bi, bs, bk))) bi = ei, bs = es, bk = ek;
        }
        for (int off = 32; off > 0; off >>= 1) {  // (a butterfly: the order is total, every lane ends with the wave's first)
            const int oi2 = __shfl_xor(bi, off);
            const double os2 = __shfl_xor(bs, off);
            const unsigned ok2 = (unsigned)__shfl_xor((int)bk, off);
            if (oi2 >= 0 && (bi < 0 || loc_before(oi2, os2, ok2, bi, bs, bk))) bi = oi2, bs = os2, bk = ok2;
        }
        __syncthreads();  // (the round before has been read)
        if ((tid & 63) == 0) wi[tid >> 6] = bi, wsr[tid >> 6] = bs, wk[tid >> 6] = bk;
        __syncthreads();
        bi = wi[0], bs = wsr[0], bk = wk[0];
        for (int w = 1; w < LOC_THREADS / 64; w++)
            if (wi[w] >= 0 && (bi < 0 || loc_before(wi[w], wsr[w], wk[w], bi, bs, bk))) bi = wi[w], bs = wsr[w], bk = wk[w];
        if (tid == 0) oi[t] = bi, os[t] = bs, ok[t] = bk;
        if (bi < 0) {  // (workgroup-uniform) nothing is left: the rest does not exist
            for (int u = t + 1 + tid; u < max_out; u += LOC_THREADS) oi[u] = -1, os[u] = INFINITY, ok[u] = 0xffffffffu;
            break;
        }
        li = bi, lsr = bs, lk = bk;
    }
}

// One wave per selected hypothesis blockIdx.x of filter b_off + blockIdx.y: the ids, the refit, the record.
__global__ __launch_bounds__(64) void k_loc_fit(EkfDev dv, LocScratch ls, double tol_sq, int b_off) {
    __shared__ double tz[EKF_MAX_PENDING][2];
    const int b = b_off + blockIdx.y, t = blockIdx.x, lane = threadIdx.x;
    const int n = dv.n_lm[b] < dv.Ncap ? dv.n_lm[b] : dv.Ncap;
    const int nz = ls.nz[b] < EKF_MAX_PENDING ? ls.nz[b] : EKF_MAX_PENDING;
    const size_t at = (size_t)b * EKF_LOCATE_MAX_OUT + t;
    if (ls.winl[at] < 0 || n < 2 || ls.cnt[b] == 0) return;  // (the whole wave)
    const unsigned key = ls.wkey[at];
    const double *x3 = filt_x(dv, b) + 3, *zf = ls.z + (size_t)b * EKF_MAX_PENDING * 2;
    const LocPose p = loc_pose_of(ls, b, key, zf, x3);
    double zx = 0.0, zy = 0.0;
    if (lane < nz) {
        zx = zf[2 * lane], zy = zf[2 * lane + 1];
        tz[lane][0] = p.px + (p.c * zx - p.s * zy), tz[lane][1] = p.py + (p.s * zx + p.c * zy);
    }
    __syncthreads();
    double best[EKF_MAX_PENDING];
    int idx[EKF_MAX_PENDING];
#pragma unroll
    for (int k = 0; k < EKF_MAX_PENDING; k++) best[k] = INFINITY, idx[k] = 0x7fffffff;
    const auto src = [&](int l) {
        double2_t v = {LOC_FAR, LOC_FAR};
        if (l < n) {
            const double2_u u = *(const double2_u *)(x3 + 2 * (size_t)l);
            v = (double2_t){u.x, u.y};
        }
        return v;
    };
    loc_scan<EKF_MAX_PENDING>(src, (n + 255) & ~255, 0, tz, nz, lane, best, idx);
    const LocMatch m = loc_resolve<EKF_MAX_PENDING>(best, idx, nz, tol_sq, lane);
    if (lane < EKF_MAX_PENDING) ls.ids[at * EKF_MAX_PENDING + lane] = m.win ? m.lm : -1;
    double lx = 0.0, ly = 0.0;
    if (m.win) lx = x3[2 * (size_t)m.lm], ly = x3[2 * (size_t)m.lm + 1];
    // the closed-form fit over the inliers, every sum in ascending k (x + 0.0 == x: the others add nothing)
    const double cntd = (double)m.inliers;
    double c = p.c, s = p.s, tx = p.px, ty = p.py, phi = atan2(p.crs, p.dot), rms = 0.0;
    const double pair_phi = phi;
    if (m.inliers > 0) {
        double mzx = 0.0, mzy = 0.0, mlx = 0.0, mly = 0.0;
        for (int k = 0; k < nz; k++) {
            const bool w = __shfl((int)m.win, k);
            mzx += w ? __shfl(zx, k) : 0.0, mzy += w ? __shfl(zy, k) : 0.0, mlx += w ? __shfl(lx, k) : 0.0, mly += w ? __shfl(ly, k) : 0.0;
        }
        mzx /= cntd, mzy /= cntd, mlx /= cntd, mly /= cntd;
        const double ax = zx - mzx, ay = zy - mzy, bx = lx - mlx, by = ly - mly;
        double sd = 0.0, sx = 0.0;
        for (int k = 0; k < nz; k++) {
            const bool w = __shfl((int)m.win, k);
            sd += w ? __shfl(ax * bx + ay * by, k) : 0.0, sx += w ? __shfl(ax * by - ay * bx, k) : 0.0;
        }
        const double nrm = sqrt(sd * sd + sx * sx);
        if (nrm > 0.0) c = sd / nrm, s = sx / nrm, phi = atan2(sx, sd);
        tx = mlx - (c * mzx - s * mzy), ty = mly - (s * mzx + c * mzy);
        const double ex = tx + (c * zx - s * zy) - lx, ey = ty + (s * zx + c * zy) - ly;
        double rss = 0.0;
        for (int k = 0; k < nz; k++) rss += __shfl((int)m.win, k) ? __shfl(ex * ex + ey * ey, k) : 0.0;
        rms = sqrt(rss / cntd);
    }
    if (lane == 0) {
        const int r = (int)(key >> 28);
        const int *bp = ls.base + ((size_t)b * EKF_LOCATE_MAX_BASE + r) * 2;
        ekf_locate_hyp h;
        h.pose[0] = tx, h.pose[1] = ty, h.pose[2] = phi;
        h.pair_pose[0] = p.px, h.pair_pose[1] = p.py, h.pair_pose[2] = pair_phi;
        h.ssr = m.ssr, h.rms = rms;
        h.inliers = m.inliers, h.meas_a = bp[0], h.meas_b = bp[1];
        h.lm_i = (int)((key >> 14) & 0x3fff), h.lm_j = (int)(key & 0x3fff), h.reserved = 0;
        ls.hyp[at] = h;
    }
}
