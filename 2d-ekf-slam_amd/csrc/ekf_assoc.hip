// ekf_assoc.hip -- the joint-compatibility search of a scan on the device (ekf_associate_joint): from the per-measurement candidate
// table to the chosen landmark of every measurement in ONE launch, whatever the number of nodes.  The search itself -- traversal,
// pruning, node budget and the O(q^2) extension of a hypothesis by one pairing -- is ekf_assoc_search.h, which the CPU runs too
// (tests/cpp/assoc_search_check.cpp); this file gives it the filter: the blocks of P through fuse_block, x and the robot rows, the
// call's measurements as ekf_gate.hip's sweep left them in GateScratch, cos phi and sin phi once per filter (cos() and sin() of the
// device library on x[2], as k_match_factor takes them).
//
// Not on the hot path: once per call on a settled handle, all streams idle.  Included by ekf_api.hip behind ekf_gate.hip (GateScratch)
// and ekf_match.hip (MatchScratch, fuse_block through ekf_fuse.hip).
//
//   k_assoc_search  one wave per filter.  Lane c scores child c of the node being expanded (at most ASSOC_MAX_BRANCH = 16 lanes work
//                   there; the copy of a child's columns into the factor runs over all 64): the forward substitution against U and y
//                   in LDS (every lane reads the same element: a broadcast), its own columns in a work area of LDS interleaved by
//                   lane (element e of lane c at e * 16 + c: no bank conflict between the lanes).  Cross blocks of P_LL are read on
//                   demand, one fuse_block per pairing of the hypothesis and child.  The winner goes out as ids per measurement and,
//                   compacted, into MatchScratch: k_match_factor with apply = 0 behind it gives d2 exactly as ekf_joint_compat does.
// Nothing of the filter is written.  One writer per value, every sum in a fixed order, no atomics; every loop is bounded by the
// node budget, the branch limit and 32; the kernel waits on nobody.

#include "ekf_assoc_search.h"

#include "ekf_map_scratch.h"  // AssocScratch

struct AssocArgs {
    double jg[ASSOC_MAX_MEAS];
    long long max_nodes;
};

struct AssocWave {
    int lane, nl;
    __device__ void sync() const { __syncthreads(); }  // (one wave per workgroup)
};

struct AssocFilter {
    const EkfDev *dv;
    const double *bm, *Dx, *xv, *zt, *Rt;
    const int *cd;
    double c, s, px, py, prr[9];
    int b, n;
    __device__ int cand(int i, int k) const { return cd[i * ASSOC_MAX_BRANCH + k]; }
    __device__ bool landmark(int l, double *lx, double *ly, double pr[6]) const {
        if (l >= n) return false;
        *lx = xv[3 + 2 * l], *ly = xv[4 + 2 * l];
#pragma unroll
        for (int r = 0; r < 3; r++) pr[2 * r] = filt_R(*dv, b, r)[3 + 2 * l], pr[2 * r + 1] = filt_R(*dv, b, r)[4 + 2 * l];
        return true;
    }
    __device__ void block(int l1, int l2, double pb[4]) const { fuse_block(*dv, bm, Dx, l1, l2, pb); }
    __device__ const double *z(int i) const { return zt + 2 * i; }
    __device__ const double *Rm(int i) const { return Rt + 4 * i; }
};

__global__ __launch_bounds__(64) void k_assoc_search(EkfDev dv, GateScratch gs, AssocScratch as, MatchScratch ms, AssocArgs aa, int buf, int b_off) {
    __shared__ AssocStack st;
    __shared__ double work[ASSOC_MAX_BRANCH * ASSOC_WORK];
    __shared__ double sJg[ASSOC_MAX_MEAS];
    __shared__ int sNc[ASSOC_MAX_MEAS], sCd[ASSOC_MAX_MEAS * ASSOC_MAX_BRANCH];
    const int b = b_off + blockIdx.x, lane = threadIdx.x;
    int m = gs.nz[b] < gs.zcap ? gs.nz[b] : gs.zcap;
    m = m < 0 ? 0 : m > ASSOC_MAX_MEAS ? ASSOC_MAX_MEAS : m;
    if (lane < ASSOC_MAX_MEAS) {
        const int nc = lane < m ? as.ncand[(size_t)b * ASSOC_MAX_MEAS + lane] : 0;
        sNc[lane] = nc < 0 ? 0 : nc > ASSOC_MAX_BRANCH ? ASSOC_MAX_BRANCH : nc;
        sJg[lane] = aa.jg[lane];
    }
    for (int q = lane; q < ASSOC_MAX_MEAS * ASSOC_MAX_BRANCH; q += 64) sCd[q] = as.cand[(size_t)b * ASSOC_MAX_MEAS * ASSOC_MAX_BRANCH + q];
    __syncthreads();
    AssocFilter f;
    f.dv = &dv, f.b = b;
    f.n = dv.n_lm[b] < dv.Ncap ? dv.n_lm[b] : dv.Ncap;
    f.bm = filt_Bm(dv, buf, b), f.Dx = filt_D(dv, b), f.xv = filt_x(dv, b);
    f.zt = gs.z + 2 * (size_t)b * gs.zcap, f.Rt = gs.Rm + 4 * (size_t)b * gs.zcap;
    f.cd = sCd;
    f.c = cos(f.xv[2]), f.s = sin(f.xv[2]);
    f.px = f.xv[0], f.py = f.xv[1];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int g = 0; g < 3; g++) f.prr[3 * r + g] = filt_R(dv, b, r)[g];
    AssocWave wv = {lane, 64};
    AssocResult res;
    assoc_search(f, wv, &st, m, sNc, sJg, aa.max_nodes, work, ASSOC_MAX_BRANCH, 1, &res);
    __syncthreads();
    if (lane < ASSOC_MAX_MEAS) as.ids[(size_t)b * ASSOC_MAX_MEAS + lane] = lane < m ? st.best[lane] : -1;
    if (lane == 0) {
        as.out[b] = res;
        const size_t z0 = (size_t)b * ms.zcap;
        int j = 0;
        for (int k = 0; k < m; k++) {  // the winner as ekf_joint_compat's table would hold it: the paired measurements in order
            if (st.best[k] < 0 || j >= ms.zcap) continue;
            ms.ids[z0 + j] = st.best[k];
            ms.z[2 * (z0 + j)] = f.zt[2 * k], ms.z[2 * (z0 + j) + 1] = f.zt[2 * k + 1];
#pragma unroll
            for (int e = 0; e < 4; e++) ms.Rm[4 * (z0 + j) + e] = f.Rt[4 * k + e];
            j++;
        }
        ms.cnt[b] = j;
    }
}
