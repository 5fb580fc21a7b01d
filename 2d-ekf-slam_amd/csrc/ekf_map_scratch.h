// ekf_map_scratch.h -- the device scratch a handle keeps for its map operations (ekf_map_api.hip): each kernel file's scratch struct
// and the layout of the block behind it.  Host- and device-compilable: the kernels take the structs by value, the host carves them,
// tests/cpp/map_scratch_check.cpp runs the carving on the CPU.
// A block is laid out by ONE function, carve_<block>(scratch, carver, geometry[, capacity]): a take<T>(count) per array in the block's
// order.  On a Carver without a base it yields the block's size (bytes()), on the allocation the pointers: one text, so the two cannot
// drift apart.  Every block lays its 8-byte-aligned arrays before its ints: natural alignment pads nothing.
#pragma once
#include "ekf_device.h"
#include "ekf_assoc_search.h"

// What the extents follow, from EkfDev (size_t: a product of them is one).
struct ScratchGeom {
    size_t B;
    int Ncap;
    size_t rows, xs, dn, bm_stride;
};

struct Carver {
    char *base;  // nullptr: sizes only
    size_t off = 0;
    template <typename T>
    T *take(size_t count) {
        off = (off + alignof(T) - 1) & ~(alignof(T) - 1);
        T *p = base ? (T *)(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return off; }
};

// ---- ekf_factor.hip (ekf_joint_consistency) ---------------------------------------------------------------------------------------
enum { FAC_LOGDET = 0, FAC_MINP = 1, FAC_MAXP = 2, FAC_YY = 3, FAC_WW = 4 /* 00 01 02 11 12 22 */, FAC_WY = 10 /* 3 */, FAC_INFO = 13, FAC_ACC = 16 };
struct FactorScratch {
    double *S;       // [B][bm_stride]   the factor in the making: tiles of U at and above step k's row, the Schur complement below
    double *rhs;     // [B][rows][4]     {e_L, P_LR (3)} -> {y, W (3)}
    double *acc;     // [B][FAC_ACC]
    double *xt;      // [B][xs]          x_true
    ekf_joint *out;  // [B]
};
inline void carve_factor(FactorScratch &fs, Carver &c, const ScratchGeom &g) {
    fs.S = c.take<double>(g.B * g.bm_stride);
    fs.rhs = c.take<double>(g.B * g.rows * 4);
    fs.acc = c.take<double>(g.B * FAC_ACC);
    fs.xt = c.take<double>(g.B * g.xs);
    fs.out = c.take<ekf_joint>(g.B);
}

// ---- ekf_pairs.hip (ekf_find_duplicates) ------------------------------------------------------------------------------------------
struct DupScratch {
    double *box;         // [B][dn / 32][4]  {min x, max x, min y, max y} of landmarks [32 g, 32 g + 32) (below the filter's count)
    int *cnt;            // [B][2]           {pairs found, degenerate pairs} of the call
    int *split;          // [B]              the batch form's per-filter splits
    ekf_dup_pair *list;  // [B][cap]         the first cap pairs appended
    int cap;
};
inline void carve_dup(DupScratch &ds, Carver &c, const ScratchGeom &g) {
    ds.box = c.take<double>(g.B * (g.dn >> 5) * 4);
    ds.cnt = c.take<int>(2 * g.B);
    ds.split = c.take<int>(g.B);
}
inline void carve_dup_list(DupScratch &ds, Carver &c, const ScratchGeom &g, int cap) {
    ds.list = c.take<ekf_dup_pair>(g.B * (size_t)cap);
    ds.cap = cap;
}

// ---- ekf_fuse.hip (ekf_fuse_landmarks; the matched updates run its apply and finish kernels) ---------------------------------------
#define FUSE_MAX_COLS (2 * EKF_MAX_PENDING)
struct FuseScratch {
    double *wr;    // [B][4][FUSE_MAX_COLS]  rows 0..2: W's robot rows of the round, after k_fuse_factor V's; row 3: d, then y
    double *U;     // [B][FUSE_MAX_COLS][FUSE_MAX_COLS]  the round's factor, row-major, upper
    int *pairs;    // [B][pcap][2]  the call's pair list {i, j}
    int *cnt;      // [B]           pairs in the list
    int *done;     // [B][2]        {pairs fused so far; 0, or 1 + the index of the first pivot of S that was not positive}
    int *m_round;  // [B]           pairs of the current round once k_fuse_factor has accepted it, else 0
    int pcap;
};
// (a landmark is in at most one pair of a call: Ncap / 2 pairs per filter)
inline void carve_fuse(FuseScratch &fs, Carver &c, const ScratchGeom &g) {
    const int pcap = g.Ncap / 2 + 1;
    fs.wr = c.take<double>(g.B * 4 * FUSE_MAX_COLS);
    fs.U = c.take<double>(g.B * FUSE_MAX_COLS * FUSE_MAX_COLS);
    fs.pairs = c.take<int>(g.B * (size_t)pcap * 2);
    fs.cnt = c.take<int>(g.B);
    fs.done = c.take<int>(2 * g.B);
    fs.m_round = c.take<int>(g.B);
    fs.pcap = pcap;
}

// ---- ekf_match.hip (ekf_update_matched, ekf_joint_compat) -------------------------------------------------------------------------
#define MATCH_TAB 8                // doubles per measurement in MatchScratch::tab: H_R row 0, H_R row 1, cos phi, sin phi
struct MatchScratch {
    double *z;    // [B][zcap][2]  the call's measurements, the skipped ones left out
    double *Rm;   // [B][zcap][4]  their covariances, column-major
    double *d2;   // [B][zcap]     running joint distance within each measurement's round (NaN from a refused pivot on)
    double *tab;  // [B][EKF_MAX_PENDING][MATCH_TAB]  the round's table, k_match_factor to k_match_gather
    int *ids;     // [B][zcap]     their landmarks
    int *cnt;     // [B]           measurements in the list
    int zcap;
};
inline void carve_match(MatchScratch &ms, Carver &c, const ScratchGeom &g, int zcap) {
    const size_t B = g.B, nz = B * (size_t)zcap;
    ms.z = c.take<double>(nz * 2);
    ms.Rm = c.take<double>(nz * 4);
    ms.d2 = c.take<double>(nz);
    ms.tab = c.take<double>(B * EKF_MAX_PENDING * MATCH_TAB);
    ms.ids = c.take<int>(nz);
    ms.cnt = c.take<int>(B);
    ms.zcap = zcap;
}

// ---- ekf_match_iter.hip (ekf_update_matched_iter): what the iterating factor tells of each measurement's round, beside MatchScratch ---
struct IterScratch {
    double *step;  // [B][zcap]  the last step of the measurement's round
    int *iters;    // [B][zcap]  the factorisations of its round
    int zcap;
};
inline void carve_iter(IterScratch &is, Carver &c, const ScratchGeom &g, int zcap) {
    const size_t nz = g.B * (size_t)zcap;
    is.step = c.take<double>(nz);
    is.iters = c.take<int>(nz);
    is.zcap = zcap;
}

// ---- ekf_gate.hip (ekf_gate_candidates) -------------------------------------------------------------------------------------------
#define GATE_THREADS 256
struct GateScratch {
    double *z;            // [B][zcap][2]        the call's valid measurements of each filter, compacted
    double *Rm;           // [B][zcap][4]
    double *pd;           // [B][npart][zcap]    workgroup g's nearest distance of measurement k (EKF_INF: none)
    ekf_decision *near;   // [B][zcap]
    int *pl;              // [B][npart][zcap]    ... its landmark (0x7fffffff: none)
    int *ps;              // [B][npart][zcap]    ... the landmarks it skipped
    int *skip;            // [B][zcap]
    int *nz;              // [B]                 valid measurements of the call
    int *cnt;             // [B]                 pairs listed by the call
    ekf_candidate *list;  // [B][ccap]           the first ccap pairs appended (meas = the compacted index)
    int zcap, ccap, npart;
};
// (a partial per workgroup of GATE_THREADS landmarks)
inline void carve_gate(GateScratch &gs, Carver &c, const ScratchGeom &g, int zcap) {
    const int npart = (g.Ncap + GATE_THREADS - 1) / GATE_THREADS;
    const size_t B = g.B, nz = B * (size_t)zcap, np = nz * (size_t)npart;
    gs.z = c.take<double>(nz * 2);
    gs.Rm = c.take<double>(nz * 4);
    gs.pd = c.take<double>(np);
    gs.near = c.take<ekf_decision>(nz);
    gs.pl = c.take<int>(np);
    gs.ps = c.take<int>(np);
    gs.skip = c.take<int>(nz);
    gs.nz = c.take<int>(B);
    gs.cnt = c.take<int>(B);
    gs.zcap = zcap, gs.npart = npart;
}
inline void carve_gate_list(GateScratch &gs, Carver &c, const ScratchGeom &g, int ccap) {
    gs.list = c.take<ekf_candidate>(g.B * (size_t)ccap);
    gs.ccap = ccap;
}

// ---- ekf_assoc.hip (ekf_associate_joint): 2 328 bytes per filter whatever the capacity --------------------------------------------
struct AssocScratch {
    int *ncand;        // [B][32]      candidates kept of each valid measurement (compacted index, as GateScratch)
    int *cand;         // [B][32][16]  their landmarks in list order
    int *ids;          // [B][32]      out: the landmark of each valid measurement, -1: none
    AssocResult *out;  // [B]
};
inline void carve_assoc(AssocScratch &as, Carver &c, const ScratchGeom &g) {
    as.out = c.take<AssocResult>(g.B);
    as.ncand = c.take<int>(g.B * EKF_MAX_PENDING);
    as.cand = c.take<int>(g.B * EKF_MAX_PENDING * EKF_ASSOC_MAX_BRANCH);
    as.ids = c.take<int>(g.B * EKF_MAX_PENDING);
}

// ---- ekf_locate.hip (ekf_locate_scan) ---------------------------------------------------------------------------------------------
#define LOC_THREADS 256
#define LOC_LDS_LM 4096     // landmarks of x a k_loc_score workgroup stages in LDS at a time (64 KB)
#define LOC_PICK_PARTS 64   // partial lists of the selection per filter
#define LOC_LIST_FLOOR 4096 // candidates per filter the list starts with
struct LocScratch {
    double *z;                // [B][32][2]     the call's valid measurements of each filter, compacted
    double *blen;             // [B][16]        the base pairs' separations
    double *pssr;             // [B][LOC_PICK_PARTS][64]  the partial lists of the selection: ssr, ...
    double *wssr;             // [B][64]        the selected hypotheses, best first
    ekf_locate_hyp *hyp;      // [B][64]        their records (meas_a, meas_b: compacted indices)
    unsigned long long *cnt;  // [B]            candidates found by the call
    unsigned *pkey;           // [B][LOC_PICK_PARTS][64]  ... key (r << 28 | i << 14 | j), ...
    unsigned *wkey;           // [B][64]
    int *pinl;                // [B][LOC_PICK_PARTS][64]  ... inliers (-1: no entry)
    int *winl;                // [B][64]
    int *ids;                 // [B][64][32]    the landmark of each compacted measurement under each selected hypothesis, -1: none
    int *nz;                  // [B]            valid measurements of the call
    int *nbase;               // [B]            base pairs of the call (0: nothing to search)
    int *base;                // [B][16][2]     their measurements (compacted indices a < b)
    double *ssr;              // [B][ccap]      the list: the score of candidate q, ...
    unsigned *key;            // [B][ccap]      ... its key, the first ccap appended, ...
    int *inl;                 // [B][ccap]      ... its inliers
    int ccap;
};
inline void carve_loc(LocScratch &ls, Carver &c, const ScratchGeom &g) {
    const size_t B = g.B, sel = B * EKF_LOCATE_MAX_OUT, part = sel * LOC_PICK_PARTS;
    ls.z = c.take<double>(B * EKF_MAX_PENDING * 2);
    ls.blen = c.take<double>(B * EKF_LOCATE_MAX_BASE);
    ls.pssr = c.take<double>(part);
    ls.wssr = c.take<double>(sel);
    ls.hyp = c.take<ekf_locate_hyp>(sel);
    ls.cnt = c.take<unsigned long long>(B);
    ls.pkey = c.take<unsigned>(part);
    ls.wkey = c.take<unsigned>(sel);
    ls.pinl = c.take<int>(part);
    ls.winl = c.take<int>(sel);
    ls.ids = c.take<int>(sel * EKF_MAX_PENDING);
    ls.nz = c.take<int>(B);
    ls.nbase = c.take<int>(B);
    ls.base = c.take<int>(B * EKF_LOCATE_MAX_BASE * 2);
}
inline void carve_loc_list(LocScratch &ls, Carver &c, const ScratchGeom &g, int ccap) {
    ls.ssr = c.take<double>(g.B * (size_t)ccap);
    ls.key = c.take<unsigned>(g.B * (size_t)ccap);
    ls.inl = c.take<int>(g.B * (size_t)ccap);
    ls.ccap = ccap;
}

// ---- ekf_rewrite.hip (ekf_add_landmarks) ------------------------------------------------------------------------------------------
struct AddScratch {
    double *tab;  // [B][add_tab_stride(zcap)]
    double *ops;  // [B][zcap][2]{w0, w1, w2, h}
    int zcap;
};
inline void carve_add(AddScratch &as, Carver &c, const ScratchGeom &g, int zcap) {
    as.tab = c.take<double>(g.B * add_tab_stride(zcap));
    as.ops = c.take<double>(g.B * (size_t)zcap * 8);
    as.zcap = zcap;
}
