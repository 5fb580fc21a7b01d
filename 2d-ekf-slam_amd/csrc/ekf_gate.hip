// ekf_gate.hip -- the individual compatibility table of a scan on the device (ekf_gate_candidates): for every measurement of the call
// and every landmark of the filter the association sweep's res, S and d2 (sweep_const / sweep_single of ekf_filter_math.h, the
// arithmetic k_chain and k_solo run), every measurement against the SAME state.  Nothing of the filter is written, and only what the
// chain kernels keep current inside an open window is read: x, the three robot rows and the diagonal blocks D -- no fold, no pass.
//
// Not on the hot path: once per call, the chain stream idle.  Included by ekf_api.hip behind ekf_kernels.hip (wave_argmin, cand_better)
// and ekf_rewrite.hip (filt_x / filt_R / filt_D).
//
//   k_gate          grid (ceil(N / 256), filters).  A thread holds ONE landmark's LmState in registers for the whole call (its 88 bytes
//                   are read once, however long the scan); the measurements go through LDS in chunks of GATE_CHUNK, their SweepConst
//                   computed once per workgroup; every lane runs sweep_single per measurement.  A gate-passer is appended with one
//                   INTEGER atomic per wave (ballot, prefix popcount); the nearest is reduced across the wave (DPP), then across the
//                   workgroup's four waves in LDS in wave order, and written as this workgroup's partial; skipped landmarks are counted
//                   the same way.
//   k_gate_nearest  a thread per measurement: the workgroups' partials in workgroup order (cand_better: ties keep the lower index),
//                   the skip counts summed, the filter's gate (Update.cpp:152,181,191) on the winner.
// The appended order is the hardware's; the host sorts the list by (meas, d2, landmark).  Every value written is a function of the
// (measurement, landmark) pair alone or comes out of a fixed-order reduction: the same bits on every call and in the batch form.

#define GATE_CHUNK 32

#include "ekf_map_scratch.h"  // GateScratch, GATE_THREADS

__global__ __launch_bounds__(GATE_THREADS) void k_gate(EkfDev dv, GateScratch gs, double gate, int b_off) {
    __shared__ SweepConst kc[GATE_CHUNK];
    __shared__ double zc[GATE_CHUNK][2];
    __shared__ double wd[GATE_CHUNK][GATE_THREADS / 64];
    __shared__ int wl[GATE_CHUNK][GATE_THREADS / 64], ws[GATE_CHUNK][GATE_THREADS / 64];
    const int b = b_off + blockIdx.y, g = blockIdx.x;
    const int n = dv.n_lm[b] < dv.Ncap ? dv.n_lm[b] : dv.Ncap;
    const int nz = gs.nz[b] < gs.zcap ? gs.nz[b] : gs.zcap;
    if (g * GATE_THREADS >= n || g >= gs.npart) return;  // (the whole workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lm = g * GATE_THREADS + tid;
    const bool have = lm < n;
    const double *x = filt_x(dv, b), *R0 = filt_R(dv, b), *Dx = filt_D(dv, b);
    LmState st = {0, 0, {0, 0, 0, 0, 0, 0}, 0, 0, 0};
    if (have) {
        const int Li = 3 + 2 * lm;
        st.x0 = x[Li], st.x1 = x[Li + 1];
        for (int i = 0; i < 3; i++) st.rc[i * 2] = R0[(size_t)i * dv.xs + Li], st.rc[i * 2 + 1] = R0[(size_t)i * dv.xs + Li + 1];
        st.dxx = Dx[lm], st.dxy = Dx[dv.dn + lm], st.dyy = Dx[2 * (size_t)dv.dn + lm];
    }
    const size_t zb = (size_t)b * gs.zcap, pb = ((size_t)b * gs.npart + g) * gs.zcap;
    int *cnt = gs.cnt + b;
    ekf_candidate *list = gs.list + (size_t)b * gs.ccap;
    for (int k0 = 0; k0 < nz; k0 += GATE_CHUNK) {
        const int m = nz - k0 < GATE_CHUNK ? nz - k0 : GATE_CHUNK;
        __syncthreads();  // (the chunk before has been read)
        if (tid < m) {
            double Prr[9], c, s;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) Prr[i * 3 + j] = R0[(size_t)i * dv.xs + j];
            sincos(x[2], &s, &c);
            kc[tid] = sweep_const(c, s, x[0], x[1], Prr, gs.Rm + 4 * (zb + k0 + tid));
            zc[tid][0] = gs.z[2 * (zb + k0 + tid)], zc[tid][1] = gs.z[2 * (zb + k0 + tid) + 1];
        }
        __syncthreads();
        for (int q = 0; q < m; q++) {  // (workgroup-uniform: all 64 lanes of every wave are active at the ballots and DPP steps)
            const SweepOne so = sweep_single(st, zc[q][0], zc[q][1], kc[q], dv.cond_k2);
            const bool skipped = have && sweep_skips(so, dv.cond_k2);
            // (so.d where sweep_single kept the pair: a listed pair's d2 and the nearest's mahal are ONE value, not two copies of an expression)
            const double d2 = so.d < EKF_INF ? so.d : sweep_raw_d2(so);
            const bool listed = have && !skipped && d2 <= gate;  // (false for NaN)
            const unsigned long long lmask = __ballot(listed);
            if (lmask) {  // (wave-uniform) one integer atomic per wave; a lane's place = the listed lanes below it
                const int leader = __builtin_ctzll(lmask);
                int base = 0;
                if (lane == leader) base = atomicAdd(cnt, __popcll(lmask));
                base = __shfl(base, leader);
                const int at = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(lmask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)lmask, 0u));
                if (listed && at >= 0 && at < gs.ccap) {
                    ekf_candidate cd;
                    cd.meas = k0 + q, cd.landmark = lm, cd.d2 = d2;
                    list[at] = cd;
                }
            }
            const int nskip = __popcll(__ballot(skipped));
            const bool cand = have && so.d < EKF_INF;  // (sweep_single: EKF_INF when skipped, NaN or no smaller than EKF_INF, Update.cpp:140)
            double bd = cand ? so.d : EKF_INF;
            int bi = cand ? lm : 0x7fffffff, who = lane;
            wave_argmin(bd, bi, who);
            if (lane == 0) wd[q][wave] = bd, wl[q][wave] = bi, ws[q][wave] = nskip;
        }
        __syncthreads();
        if (tid < m) {
            double bd = wd[tid][0];
            int bi = wl[tid][0], nskip = ws[tid][0];
            for (int w = 1; w < GATE_THREADS / 64; w++) {
                const bool take = cand_better(wd[tid][w], wl[tid][w], bd, bi);
                bd = take ? wd[tid][w] : bd, bi = take ? wl[tid][w] : bi;
                nskip += ws[tid][w];
            }
            gs.pd[pb + k0 + tid] = bd, gs.pl[pb + k0 + tid] = bi, gs.ps[pb + k0 + tid] = nskip;
        }
    }
}

__global__ __launch_bounds__(64) void k_gate_nearest(EkfDev dv, GateScratch gs, int b_off) {
    const int b = b_off + blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    const int n = dv.n_lm[b] < dv.Ncap ? dv.n_lm[b] : dv.Ncap;
    const int nz = gs.nz[b] < gs.zcap ? gs.nz[b] : gs.zcap;
    if (k >= nz) return;
    int parts = (n + GATE_THREADS - 1) / GATE_THREADS;
    parts = parts < gs.npart ? parts : gs.npart;
    double bd = EKF_INF;
    int bi = 0x7fffffff, nskip = 0;
    for (int g = 0; g < parts; g++) {
        const size_t at = ((size_t)b * gs.npart + g) * gs.zcap + k;
        const double d = gs.pd[at];
        const int i = gs.pl[at];
        const bool take = cand_better(d, i, bd, bi);
        bd = take ? d : bd, bi = take ? i : bi;
        nskip += gs.ps[at];
    }
    const bool found = bi != 0x7fffffff;
    const double mahal = found ? bd : EKF_INF;
    ekf_decision e;
    if (!found || mahal > dv.gamma_max) e.decision = EKF_DECISION_NEW;   // Update.cpp:152
    else if (mahal < dv.gamma_min) e.decision = EKF_DECISION_OLD;        // :181
    else e.decision = EKF_DECISION_IGNORE;                               // :191
    e.matched = found ? 3 + 2 * bi : 0;
    e.mahal = mahal;
    gs.near[(size_t)b * gs.zcap + k] = e;
    gs.skip[(size_t)b * gs.zcap + k] = nskip;
}
