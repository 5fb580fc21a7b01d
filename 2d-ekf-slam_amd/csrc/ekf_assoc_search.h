// ekf_assoc_search.h -- the joint-compatibility search of ekf_associate_joint as code for host and device: the depth-first
// traversal (stack, pruning, node budget, the best hypothesis) and the incremental solve that scores one more pairing, on plain
// arrays.  k_assoc_search (ekf_assoc.hip) runs it with the 64 lanes of a wave and the arrays in LDS; tests/cpp/assoc_search_check.cpp
// runs the same text with one lane on synthetic systems against a brute-force enumeration.  No HIP call in here.
//
// A hypothesis H with q pairings (measurement k_p, landmark l_p), p = 0..q-1 in measurement order, is kept as the upper factor U of
// its S (2q x 2q, U^T U = S, S as ekf_match.hip builds it) and y = U^-T d; its joint distance is D2 = |y|^2.  One more pairing
// (k, l) costs O(q^2), not a refactorisation:
//     s  = the cross column of S, rows of the q pairings against (k, l)          (2q x 2)   assoc_cross per block
//     w  = U^-T s                                                                 forward substitution, the sums in row order
//     S' = S_ll + R_k - w^T w,   e = d_kl - w^T y                                 the 2 x 2 Schur complement
//     S' = u^T u,  y' = u^-T e,  D2' = D2 + y'_0^2 + y'_1^2
// The columns [w; u] are the two new columns of U and y' the two new entries of y: exactly the rows 2q, 2q + 1 of the right-looking
// factorisation of the extended S (every element takes its subtractions in the same order there), so the pivots are the same
// numbers and the rule of MATCH_PIVOT_TOL applies to them unchanged: a pivot that is not above 2^-44 of its own diagonal entry of S
// (or NaN) makes the extension not compatible.
//
// The traversal is the one include/ekfslam_c.h states (ekf_associate_joint): measurements in list order, the candidates of each
// in list order, then "no pairing"; a node is entered only if it can still beat the best; Best = most pairings, then smallest D2,
// then first found.  A node's children are all scored when the node is expanded -- that is where the lanes work side by side, one
// child each -- and their distances kept per level; going down into a child that is not the one scored last, the one lane scores it
// again to get its columns back (the factor is ONE array: the columns of pairing q are overwritten on the way back up).
// Scalars of the traversal are computed by every lane from the same shared values: uniform without a broadcast.  Shared arrays
// have one writer per value, with sync() between a write and the other lanes' reads.
#pragma once
#include <math.h>

#ifdef __HIP__
#define ASSOC_HD __host__ __device__ inline
#else
#define ASSOC_HD inline
#endif

#define ASSOC_MAX_MEAS 32                         // EKF_MAX_PENDING: pairings of a hypothesis, levels of the traversal
#define ASSOC_MAX_BRANCH 16                       // EKF_ASSOC_MAX_BRANCH: candidates kept per measurement
#define ASSOC_COLS (2 * ASSOC_MAX_MEAS)
#define ASSOC_PIVOT_TOL 0x1p-44                   // MATCH_PIVOT_TOL
#define ASSOC_WORK (2 * (ASSOC_COLS + 2) + 2 + 12)  // doubles of a child's work area: two columns of 66 rows, y', h and pr

// What the traversal keeps (LDS on the device: 32 768 + 512 + 264 + 4 096 + 3 072 bytes of doubles, 644 of ints).
struct AssocStack {
    double U[ASSOC_COLS * ASSOC_COLS];               // the factor of the current hypothesis, element (row k, column j) at j * ASSOC_COLS + k
    double y[ASSOC_COLS];
    double D2[ASSOC_MAX_MEAS + 1];                   // the distance on entering level i
    double cD2[ASSOC_MAX_MEAS * ASSOC_MAX_BRANCH];   // level i's children: D2', NaN where the extension is not feasible
    double lin[ASSOC_MAX_MEAS * 12];                 // pairing p: H_R (6) and the landmark's robot columns P_R,l (6)
    int lm[ASSOC_MAX_MEAS];                          // pairing p's landmark
    int cnt[ASSOC_MAX_MEAS + 1];                     // pairings on entering level i
    int cur[ASSOC_MAX_MEAS];                         // level i's next child (its candidate count + 1: "no pairing" taken too)
    int choice[ASSOC_MAX_MEAS];                      // level i's pairing in the current hypothesis: a candidate's place in its list, or -1
    int best[ASSOC_MAX_MEAS];                        // Best: measurement i's landmark, or -1
};

struct AssocResult {
    long long nodes;
    double d2;
    int n_paired, complete;
};

// H_R = [-C^T | -C^T J dp] of a landmark at (lx, ly) seen from (px, py, phi), the predicted measurement zh = C^T dp, and W's robot
// rows of its column pair, wr (r, f) at 2 r + f, from P_RR (prr, row-major) and the landmark's robot columns pr (r, g) at 2 r + g:
// the expressions of k_match_factor.
ASSOC_HD void assoc_linearise(double c, double s, double px, double py, double lx, double ly, const double prr[9], const double pr[6], double h[6], double zh[2],
                              double wr[6]) {
    const double dpx = lx - px, dpy = ly - py;
    h[0] = -c, h[1] = -s, h[2] = c * dpy - s * dpx;
    h[3] = s, h[4] = -c, h[5] = -(s * dpy) - c * dpx;
    zh[0] = c * dpx + s * dpy, zh[1] = c * dpy - s * dpx;
    const double Cm[4] = {c, -s, s, c};
    for (int r = 0; r < 3; r++)
        for (int f = 0; f < 2; f++)
            wr[2 * r + f] = (((prr[3 * r] * h[3 * f] + prr[3 * r + 1] * h[3 * f + 1]) + prr[3 * r + 2] * h[3 * f + 2]) + pr[2 * r] * Cm[f]) + pr[2 * r + 1] * Cm[2 + f];
}

// The block of S between pairing p (rows: H_R hp, robot columns prp of its landmark) and pairing n (columns: H_R hn, wrn), pb = the
// block (l_p, l_n) of P; v (e, f) at 2 e + f, R not added.  The expressions of k_match_factor with k = p, l = n.
ASSOC_HD void assoc_cross(const double *hp, const double *prp, const double *hn, const double *wrn, const double pb[4], double c, double s, double v[4]) {
    const double Cm[4] = {c, -s, s, c};
    double T[4];
    for (int g = 0; g < 2; g++)
        for (int f = 0; f < 2; f++)
            T[2 * g + f] = (((prp[g] * hn[3 * f] + prp[2 + g] * hn[3 * f + 1]) + prp[4 + g] * hn[3 * f + 2]) + pb[2 * g] * Cm[f]) + pb[2 * g + 1] * Cm[2 + f];
    for (int e = 0; e < 2; e++)
        for (int f = 0; f < 2; f++)
            v[2 * e + f] = (((hp[3 * e] * wrn[f] + hp[3 * e + 1] * wrn[2 + f]) + hp[3 * e + 2] * wrn[4 + f]) + Cm[e] * T[f]) + Cm[2 + e] * T[2 + f];
}

// One more pairing behind a hypothesis of n = 2 q rows (U, y as in AssocStack).  w: element (row r, column f) at w[(2 r + f) * ws];
// in: rows 0 .. n - 1 the cross column, (n, 0), (n, 1), (n + 1, 1) the upper triangle of S_ll + R_k; d = d_kl.  out: the two new
// columns of U in w (rows 0 .. n + 1), yo = y'.  false: a pivot was refused (w is then of no use).
ASSOC_HD bool assoc_extend(const double *U, const double *y, int n, double *w, int ws, const double d[2], double yo[2]) {
    for (int j = 0; j < n; j++) {
        const double *Uj = U + (long)j * ASSOC_COLS;
        double t0 = w[(2 * j) * ws], t1 = w[(2 * j + 1) * ws];
        for (int k = 0; k < j; k++) {
            const double u = Uj[k];
            t0 = t0 - u * w[(2 * k) * ws], t1 = t1 - u * w[(2 * k + 1) * ws];
        }
        w[(2 * j) * ws] = t0 / Uj[j], w[(2 * j + 1) * ws] = t1 / Uj[j];
    }
    const double S00 = w[(2 * n) * ws], S01 = w[(2 * n + 1) * ws], S11 = w[(2 * n + 3) * ws];
    double s00 = S00, s01 = S01, s11 = S11, e0 = d[0], e1 = d[1];
    for (int k = 0; k < n; k++) {
        const double a = w[(2 * k) * ws], b = w[(2 * k + 1) * ws], yk = y[k];
        s00 = s00 - a * a, s01 = s01 - a * b, s11 = s11 - b * b;
        e0 = e0 - a * yk, e1 = e1 - b * yk;
    }
    if (!(s00 > ASSOC_PIVOT_TOL * S00)) return false;
    const double u00 = sqrt(s00), u01 = s01 / u00;
    yo[0] = e0 / u00;
    s11 = s11 - u01 * u01, e1 = e1 - u01 * yo[0];
    if (!(s11 > ASSOC_PIVOT_TOL * S11)) return false;
    const double u11 = sqrt(s11);
    yo[1] = e1 / u11;
    w[(2 * n) * ws] = u00, w[(2 * n + 1) * ws] = u01, w[(2 * n + 2) * ws] = 0.0, w[(2 * n + 3) * ws] = u11;
    return true;
}

// Child c of level i behind the hypothesis in st (cnt pairings, distance D2): D2', or NaN where it is not feasible -- the landmark is
// used already or not one of the map's, a pivot is refused, or D2' > gate_q (the joint gate of cnt + 1 pairings; false for NaN).
// Its columns, y', H_R and P_R,l stay in the work area w (stride ws) for assoc_commit.
// P: cand(i, c) -> landmark (or < 0), landmark(l, lx, ly, pr) -> false if l is none of the map's, block(l1, l2, pb), z(i), Rm(i)
// (column-major 2 x 2), c, s, px, py, prr[9].
template <class P>
ASSOC_HD double assoc_eval_child(const P &pb_, const AssocStack *st, int i, int c, int cnt, double D2, double gate_q, double *w, int ws) {
    const double nan = __builtin_nan("");
    const int l = pb_.cand(i, c);
    double lx, ly, pr[6];
    if (l < 0 || !pb_.landmark(l, &lx, &ly, pr)) return nan;
    for (int p = 0; p < cnt; p++)
        if (st->lm[p] == l) return nan;
    double h[6], zh[2], wr[6], v[4], blk[4];
    assoc_linearise(pb_.c, pb_.s, pb_.px, pb_.py, lx, ly, pb_.prr, pr, h, zh, wr);
    const int n = 2 * cnt;
    for (int p = 0; p < cnt; p++) {
        pb_.block(st->lm[p], l, blk);
        assoc_cross(st->lin + 12 * p, st->lin + 12 * p + 6, h, wr, blk, pb_.c, pb_.s, v);
        w[(4 * p) * ws] = v[0], w[(4 * p + 1) * ws] = v[1], w[(4 * p + 2) * ws] = v[2], w[(4 * p + 3) * ws] = v[3];
    }
    pb_.block(l, l, blk);
    assoc_cross(h, pr, h, wr, blk, pb_.c, pb_.s, v);
    const double *Rk = pb_.Rm(i);
    w[(2 * n) * ws] = v[0] + Rk[0], w[(2 * n + 1) * ws] = v[1] + Rk[2], w[(2 * n + 3) * ws] = v[3] + Rk[3];
    const double *zk = pb_.z(i);
    const double d[2] = {zh[0] - zk[0], zh[1] - zk[1]};
    double yo[2];
    if (!assoc_extend(st->U, st->y, n, w, ws, d, yo)) return nan;
    double acc = D2;
    acc = acc + yo[0] * yo[0];
    acc = acc + yo[1] * yo[1];
    if (!(acc <= gate_q)) return nan;
    double *x = w + (long)(2 * (ASSOC_COLS + 2)) * ws;
    x[0] = yo[0], x[ws] = yo[1];
    for (int q = 0; q < 6; q++) x[(2 + q) * ws] = h[q], x[(8 + q) * ws] = pr[q];
    return acc;
}

// The lanes of a traversal: X has lane, nl (lanes), sync().  One lane on the host.
struct AssocOneLane {
    int lane = 0, nl = 1;
    void sync() const {}
};

// Child c of level i becomes pairing cnt of the hypothesis: its columns from the work area of the lane that scored it (lane c % nl;
// fresh: scored by the expansion just before, else that lane scores it again first).
template <class P, class X>
ASSOC_HD void assoc_commit(const P &pb_, X &x, AssocStack *st, int i, int c, int cnt, double gate_q, bool fresh, double *work, int ws, int lane_stride) {
    double *w = work + (long)(c % x.nl) * lane_stride;
    if (!fresh) {
        if (x.lane == c % x.nl) (void)assoc_eval_child(pb_, st, i, c, cnt, st->D2[i], gate_q, w, ws);
        x.sync();
    }
    const int n = 2 * cnt;
    for (int r = x.lane; r < n + 2; r += x.nl) {
        st->U[(long)n * ASSOC_COLS + r] = w[(2 * r) * ws];
        st->U[(long)(n + 1) * ASSOC_COLS + r] = w[(2 * r + 1) * ws];
    }
    if (x.lane == 0) {
        const double *e = w + (long)(2 * (ASSOC_COLS + 2)) * ws;
        st->y[n] = e[0], st->y[n + 1] = e[ws];
        for (int q = 0; q < 12; q++) st->lin[12 * cnt + q] = e[(2 + q) * ws];
        st->lm[cnt] = pb_.cand(i, c);
        st->choice[i] = c;
    }
    x.sync();
}

// The search over m measurements, measurement i with nc[i] candidates (each at most ASSOC_MAX_BRANCH; m at most ASSOC_MAX_MEAS),
// jg[q - 1] the gate of q pairings, at most max_nodes expanded nodes.  work: nl work areas, lane t's at work + t * lane_stride, its
// elements ws apart.  The result in *res (every lane's copy the same) and st->best.  Without a candidate anywhere nothing is
// searched: no node, complete.
template <class P, class X>
ASSOC_HD void assoc_search(const P &pb_, X &x, AssocStack *st, int m, const int *nc, const double *jg, long long max_nodes, double *work, int ws, int lane_stride,
                           AssocResult *res) {
    res->nodes = 0, res->d2 = 0.0, res->n_paired = 0, res->complete = 1;
    for (int k = x.lane; k < ASSOC_MAX_MEAS; k += x.nl) st->best[k] = -1;
    int total = 0;
    for (int k = 0; k < m; k++) total += nc[k];
    x.sync();
    if (total == 0) return;
    enum { ENTER, NEXT, BACK };
    int mode = ENTER, i = 0, cnt = 0, best_cnt = 0;
    double D2 = 0.0, best_D2 = 0.0;
    long long nodes = 0;
    bool fresh = false;
    for (;;) {
        if (mode == ENTER) {
            const int most = cnt + (m - i);
            if (most < best_cnt || (most == best_cnt && D2 >= best_D2)) {
                mode = BACK;
                continue;
            }
            if (i == m) {  // (better than Best: the check above let it through)
                x.sync();  // (the lanes have read Best's predecessor)
                for (int k = x.lane; k < m; k += x.nl) st->best[k] = st->choice[k] >= 0 ? pb_.cand(k, st->choice[k]) : -1;
                best_cnt = cnt, best_D2 = D2;
                mode = BACK;
                continue;
            }
            if (nodes == max_nodes) {
                res->complete = 0;
                break;
            }
            nodes++;
            if (x.lane == 0) st->cnt[i] = cnt, st->D2[i] = D2, st->cur[i] = 0;
            x.sync();
            for (int c = x.lane; c < nc[i]; c += x.nl)
                st->cD2[i * ASSOC_MAX_BRANCH + c] = assoc_eval_child(pb_, st, i, c, cnt, D2, jg[cnt], work + (long)(c % x.nl) * lane_stride, ws);
            x.sync();
            fresh = true, mode = NEXT;
        }
        if (mode == NEXT) {
            int c = st->cur[i];
            while (c < nc[i] && !(st->cD2[i * ASSOC_MAX_BRANCH + c] == st->cD2[i * ASSOC_MAX_BRANCH + c])) c++;
            // (a lane's next use of a work area is a level further down; with more children than lanes the first pass's columns are gone)
            const bool kept = fresh && nc[i] <= x.nl;
            fresh = false;
            if (c < nc[i]) {
                const double d2c = st->cD2[i * ASSOC_MAX_BRANCH + c];
                x.sync();  // (cur[i] has been read)
                if (x.lane == 0) st->cur[i] = c + 1;
                assoc_commit(pb_, x, st, i, c, cnt, jg[cnt], kept, work, ws, lane_stride);
                i++, cnt++, D2 = d2c, mode = ENTER;
            } else if (c == nc[i]) {
                x.sync();
                if (x.lane == 0) st->cur[i] = nc[i] + 1, st->choice[i] = -1;
                x.sync();
                i++, mode = ENTER;
            } else
                mode = BACK;
            continue;
        }
        // BACK
        if (i == 0) break;
        i--;
        cnt = st->cnt[i], D2 = st->D2[i], mode = NEXT;
    }
    res->nodes = nodes, res->d2 = best_D2, res->n_paired = best_cnt;
}
