// ekf_map_plan.h -- the host-side planning of the map operations (ekf_map_api.hip) as pure code: the checks of the lists a caller
// hands in and the tables the kernels of ekf_rewrite.hip, ekf_extract.hip, ekf_pairs.hip, ekf_fuse.hip, ekf_match.hip, ekf_fix.hip, ekf_polar.hip,
// ekf_gate.hip and ekf_locate.hip read.  No HIP call and no handle in here: landmark counts come in as plain arrays, n_lm[k] = landmarks of the k-th filter of the call, whose number in its
// handle is b0 + k (error texts name that number).  A check reports a status and a text; the caller hands both to set_error.
// tests/cpp/map_plan_check.cpp, tests/cpp/match_plan_check.cpp, tests/cpp/fix_plan_check.cpp, tests/cpp/gate_plan_check.cpp,
// tests/cpp/assoc_plan_check.cpp, tests/cpp/add_plan_check.cpp, tests/cpp/locate_plan_check.cpp, tests/cpp/iter_plan_check.cpp and tests/cpp/polar_plan_check.cpp run all of
// it on the CPU.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ekf_device.h"

// printf into a string: the library's one formatter of error texts (set_error in ekf_api.hip, plan_fail here)
inline std::string format_text(const char *fmt, va_list ap) {
    std::string s(256, '\0');
    for (;;) {
        va_list again;
        va_copy(again, ap);
        const int n = vsnprintf(&s[0], s.size(), fmt, again);
        va_end(again);
        const bool fits = n < (int)s.size();
        s.resize(fits ? (size_t)(n > 0 ? n : 0) : (size_t)n + 1);
        if (fits) return s;
    }
}

struct PlanStatus {
    int code = EKF_OK;
    std::string text;
};

__attribute__((format(printf, 2, 3))) inline PlanStatus plan_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    PlanStatus st = {code, format_text(fmt, ap)};
    va_end(ap);
    return st;
}

inline int most_landmarks(const int *n_lm, int nb) { return nb > 0 ? std::max(0, *std::max_element(n_lm, n_lm + nb)) : 0; }

// The one growth rule of the kept scratch (ekf_map_scratch.h): the entries per filter a table or list holds for `need` when the
// handle's holds `have` -- at least `floor`, doubled until it fits, never shrunk (tests/cpp/map_scratch_check.cpp).
inline int plan_grown_cap(int have, long long need, int floor) {
    long long cap = have > floor ? have : floor;
    while (cap < need) cap *= 2;
    return (int)cap;
}

// A map of n landmarks (and joined: more behind them) that a handle of capacity Ncap cannot hold; joined < 0: n alone.
inline PlanStatus plan_no_room(int filter, int n, int joined, int Ncap, const char *verb) {
    if (joined < 0) return plan_fail(EKF_ERR_CAPACITY, "filter %d: %d landmarks do not fit capacity_landmarks = %d (ekf_reserve, then %s again)", filter, n, Ncap, verb);
    return plan_fail(EKF_ERR_CAPACITY, "filter %d: %d + %d landmarks do not fit capacity_landmarks = %d (ekf_reserve, then %s again)", filter, n, joined, Ncap, verb);
}

// z and R of entry `at` of a call's measurement lists (z [..][2], R [..][4]) are finite: the check of every call that takes such lists.
inline bool plan_entry_finite(const double *z, const double *R, size_t at) {
    bool finite = __builtin_isfinite(z[2 * at]) && __builtin_isfinite(z[2 * at + 1]);
    for (int e = 0; e < 4; e++) finite = finite && __builtin_isfinite(R[4 * at + e]);
    return finite;
}

// ---- id lists (ekf_extract_map, ekf_get_submap) ---------------------------------------------------------------------------------
// Every id non-negative, no id twice: checked before any handle is touched.
inline PlanStatus plan_ids_distinct(const int *ids, int count, int filter) {
    std::vector<int> sorted(ids, ids + count);
    std::sort(sorted.begin(), sorted.end());
    if (count > 0 && sorted[0] < 0) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: landmark id %d is negative", filter, sorted[0]);
    for (int k = 1; k < count; k++)
        if (sorted[k] == sorted[k - 1]) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: landmark id %d is named twice", filter, sorted[k]);
    return {};
}
// ... and against the source's landmark count, once the source is at rest.
inline PlanStatus plan_ids_in_range(const int *ids, int count, int N, int filter) {
    for (int k = 0; k < count; k++)
        if (ids[k] >= N) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: landmark id %d is not one of its %d landmarks", filter, ids[k], N);
    return {};
}

// The lists of an extraction over nb filters, filter k's at ids + k * ld_ids with count[k] entries (ids == nullptr: every landmark
// of the source in order): the counts and plan_ids_distinct of each.
inline PlanStatus plan_extract_lists(const int *ids, int ld_ids, const int *count, int bs0, int nb) {
    for (int k = 0; ids && k < nb; k++) {
        if (count[k] < 0 || count[k] > ld_ids) return plan_fail(EKF_ERR_BAD_ARG, "bad landmark count");
        const PlanStatus st = plan_ids_distinct(ids + (size_t)k * ld_ids, count[k], bs0 + k);
        if (st.code) return st;
    }
    return {};
}
// ... plan_ids_in_range of each against the source's counts n_src[k]; *mstride = the longest list, at least 1.
inline PlanStatus plan_extract_range(const int *ids, int ld_ids, const int *count, const int *n_src, int bs0, int nb, int *mstride) {
    *mstride = 1;
    for (int k = 0; k < nb; k++) {
        const int cnt = ids ? count[k] : n_src[k];
        if (ids) {
            const PlanStatus st = plan_ids_in_range(ids + (size_t)k * ld_ids, cnt, n_src[k], bs0 + k);
            if (st.code) return st;
        }
        *mstride = std::max(*mstride, cnt);
    }
    return {};
}
// The table k_ext_tiles and k_ext_vec read: ex[2 k] = previous landmark count of destination filter k (plan_extract_old_counts
// fills it), ex[2 k + 1] = its new one, then nb lists of mstride ids.  A list longer than the destination's capacity ends it.
inline PlanStatus plan_extract_table(const int *ids, int ld_ids, const int *count, const int *n_src, int bd0, int nb, int mstride, int Ncap, std::vector<int> *ex) {
    ex->assign((size_t)nb * (2 + mstride), 0);
    for (int k = 0; k < nb; k++) {
        const int cnt = ids ? count[k] : n_src[k];
        if (cnt > Ncap) return plan_no_room(bd0 + k, cnt, -1, Ncap, "extract");
        (*ex)[2 * k + 1] = cnt;
        int *tab = ex->data() + 2 * nb + (size_t)k * mstride;
        for (int q = 0; q < cnt; q++) tab[q] = ids ? ids[(size_t)k * ld_ids + q] : q;
    }
    return {};
}
// The destination's previous maps, what has to be overwritten: n_dst[k], or the whole capacity where the count is not to be
// trusted (the caller passes -1 for a timed-out filter).  Returns the largest of the old and new counts of the call.
inline int plan_extract_old_counts(std::vector<int> *ex, const int *n_dst, int nb, int Ncap) {
    int n_hi = 0;
    for (int k = 0; k < nb; k++) {
        const int n_old = n_dst[k] < 0 || n_dst[k] > Ncap ? Ncap : n_dst[k];
        (*ex)[2 * k] = n_old;
        n_hi = std::max(n_hi, std::max(n_old, (*ex)[2 * k + 1]));
    }
    return n_hi;
}

// ---- removal (ekf_remove_landmarks, the end of ekf_fuse_landmarks) ----------------------------------------------------------------
// The table k_rm_gather, k_rm_finish and k_rm_vec read, over ALL B filters of the handle: rm[2 b] = old count, rm[2 b + 1] = new
// count, then B maps of mstride entries, map[new] = old.  Filter b0 + k of the call's nb has the keep mask keep + k * ld_keep (a
// landmark without an entry is kept); the other filters keep everything.  nTo / nTn: the most tiles per side before / after.
struct RemovalPlan {
    std::vector<int> rm;
    int nTo = 0, nTn = 0;
    bool any = false;  // some landmark goes
    int n_new(int b) const { return rm[2 * b + 1]; }
};
inline RemovalPlan plan_removal(const int *n_lm, int B, int mstride, const unsigned char *keep, int ld_keep, int b0, int nb) {
    RemovalPlan p;
    p.rm.assign((size_t)B * (2 + mstride), 0);
    for (int b = 0; b < B; b++) {
        const int n_old = n_lm[b];
        const unsigned char *k = b >= b0 && b < b0 + nb ? keep + (size_t)(b - b0) * ld_keep : nullptr;
        int *map = p.rm.data() + 2 * B + (size_t)b * mstride;
        int n_new = 0;
        for (int l = 0; l < n_old; l++)
            if (!k || l >= ld_keep || k[l]) map[n_new++] = l;
        p.rm[2 * b] = n_old, p.rm[2 * b + 1] = n_new;
        p.any = p.any || n_new != n_old;
        p.nTo = std::max(p.nTo, lm_tiles(n_old)), p.nTn = std::max(p.nTn, lm_tiles(n_new));
    }
    return p;
}

// ---- duplicate search ---------------------------------------------------------------------------------------------------------------
// split[k] (or split_one for every filter) within [0, n_lm[k]]; *nt = the most tiles of a filter's search (dup_tile_count).
inline PlanStatus plan_dup_tiles(const int *n_lm, int b0, int nb, int split_one, const int *split, int *nt) {
    *nt = 0;
    for (int k = 0; k < nb; k++) {
        const int n = n_lm[k], sp = split ? split[k] : split_one;
        if (sp < 0 || sp > n) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: split = %d is outside [0, %d landmarks]", b0 + k, sp, n);
        *nt = std::max(*nt, dup_tile_count(n, sp));
    }
    return {};
}

// ---- fusion -------------------------------------------------------------------------------------------------------------------------
// Filter k's n_pairs[k] pairs at pairs + k * ld_pairs: 0 <= i < j < n_lm[k], every landmark in at most one pair.  *most = the
// longest list.
inline PlanStatus plan_fuse_pairs(const ekf_dup_pair *pairs, int ld_pairs, const int *n_pairs, const int *n_lm, int b0, int nb, int *most) {
    *most = 0;
    std::vector<unsigned char> seen;
    for (int k = 0; k < nb; k++) {
        const int N = n_lm[k], np = n_pairs[k];
        if (np < 0 || (np > 0 && (!pairs || np > ld_pairs))) return plan_fail(EKF_ERR_BAD_ARG, "bad pair count or list");
        seen.assign((size_t)(N > 0 ? N : 1), 0);
        for (int q = 0; q < np; q++) {
            const ekf_dup_pair &pr = pairs[(size_t)k * ld_pairs + q];
            if (!(0 <= pr.i && pr.i < pr.j && pr.j < N))
                return plan_fail(EKF_ERR_BAD_ARG, "filter %d, pair %d: (%d, %d) does not name two landmarks i < j of %d", b0 + k, q, pr.i, pr.j, N);
            if (seen[pr.i] || seen[pr.j])
                return plan_fail(EKF_ERR_BAD_ARG, "filter %d, pair %d: landmark %d is in another pair of the call", b0 + k, q, seen[pr.i] ? pr.i : pr.j);
            seen[pr.i] = seen[pr.j] = 1;
        }
        *most = std::max(*most, np);
    }
    return {};
}
// The pair table k_fuse_gather reads (FuseScratch::pairs of the call's filters): nb lists of pcap (i, j).
inline PlanStatus plan_fuse_table(const ekf_dup_pair *pairs, int ld_pairs, const int *n_pairs, int nb, int pcap, std::vector<int> *tab) {
    tab->assign((size_t)nb * pcap * 2, 0);
    for (int k = 0; k < nb; k++) {
        if (n_pairs[k] > pcap) return plan_fail(EKF_ERR_STATE, "more pairs than the pair table holds");  // (each landmark once: cannot happen)
        for (int q = 0; q < n_pairs[k]; q++) {
            (*tab)[((size_t)k * pcap + q) * 2] = pairs[(size_t)k * ld_pairs + q].i;
            (*tab)[((size_t)k * pcap + q) * 2 + 1] = pairs[(size_t)k * ld_pairs + q].j;
        }
    }
    return {};
}

// ---- the list clients of the fusion machinery: what the two below share ------------------------------------------------------------
// The check against the landmark counts and the tables have one body each: skip(id) tells the entries that are left out, `noun`
// names an entry in the texts.
inline bool plan_match_skip(int id) { return id < 0; }
inline bool plan_fix_skip(int what) { return what == EKF_FIX_SKIP; }
inline PlanStatus plan_list_ids(const int *ids, int n, const int *n_lm, int b0, int nb, int *most, bool (*skip)(int), const char *noun) {
    *most = 0;
    for (int k = 0; k < nb; k++) {
        int kept = 0;
        for (int q = 0; q < n; q++) {
            const int id = ids[(size_t)k * n + q];
            if (skip(id)) continue;
            if (id >= n_lm[k]) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, %s %d: landmark id %d is not one of its %d landmarks", b0 + k, noun, q, id, n_lm[k]);
            kept++;
        }
        *most = std::max(*most, kept);
    }
    return {};
}
// The tables a list client's factor reads (MatchScratch of the call's filters), nb lists of zcap entries with the skipped ones left
// out: zt [nb][zcap][2], Rt [nb][zcap][4], idt [nb][zcap] (the ids, or the kinds), cnt [nb]; src [nb][zcap] = the caller's index of
// each entry.  Of a heading entry z[0] and R[0] alone -- the rest of its row stays 0 (a matched list has none: every id it keeps
// is a landmark's).
struct MatchTable {
    std::vector<double> zt, Rt;
    std::vector<int> idt, cnt, src;
};
inline MatchTable plan_list_table(const double *z, const double *R, const int *ids, int n, int nb, int zcap, bool (*skip)(int)) {
    MatchTable t;
    t.zt.assign((size_t)nb * zcap * 2, 0.0), t.Rt.assign((size_t)nb * zcap * 4, 0.0);
    t.idt.assign((size_t)nb * zcap, 0), t.src.assign((size_t)nb * zcap, -1), t.cnt.assign((size_t)nb, 0);
    for (int k = 0; k < nb; k++)
        for (int q = 0; q < n; q++) {
            const size_t at = (size_t)k * n + q;
            if (skip(ids[at]) || t.cnt[k] >= zcap) continue;
            const size_t to = (size_t)k * zcap + t.cnt[k]++;
            const int width = ids[at] == EKF_FIX_HEADING ? 1 : 2;  // (a kept id is a kind of ekf_update_fixes or a landmark: skip() drops the rest)
            for (int e = 0; e < width; e++) t.zt[2 * to + e] = z[2 * at + e];
            for (int e = 0; e < width * width; e++) t.Rt[4 * to + e] = R[4 * at + e];
            t.idt[to] = ids[at], t.src[to] = q;
        }
    return t;
}

// ---- matched updates (ekf_update_matched, ekf_joint_compat) -----------------------------------------------------------------------
// The lists of nb filters, filter k's n_z measurements at z + k * n_z * 2, R + k * n_z * 4 and ids + k * n_z; ids[q] == -1: no
// measurement, skipped (its z and R are not looked at).  Checked before the handle is touched: the pointers, n_z, every id >= -1,
// z and R of every measurement finite, and at most `limit` measurements per filter (limit < 0: any number).
inline PlanStatus plan_match_values(const double *z, const double *R, const int *ids, int n_z, int b0, int nb, int limit) {
    if (n_z < 0) return plan_fail(EKF_ERR_BAD_ARG, "negative measurement count");
    if (n_z > 0 && (!z || !R || !ids)) return plan_fail(EKF_ERR_BAD_ARG, "a null list with n_z > 0");
    for (int k = 0; k < nb; k++) {
        int kept = 0;
        for (int q = 0; q < n_z; q++) {
            const size_t at = (size_t)k * n_z + q;
            if (ids[at] < -1) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, measurement %d: id %d (a landmark, or -1 to skip)", b0 + k, q, ids[at]);
            if (ids[at] < 0) continue;
            kept++;
            if (!plan_entry_finite(z, R, at)) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, measurement %d: z or R is not finite", b0 + k, q);
        }
        if (limit >= 0 && kept > limit) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: %d measurements in one hypothesis (at most %d)", b0 + k, kept, limit);
    }
    return {};
}
// ... and against the landmark counts n_lm[k], once they are current.  *most = the most measurements of a filter.
inline PlanStatus plan_match_ids(const int *ids, int n_z, const int *n_lm, int b0, int nb, int *most) {
    return plan_list_ids(ids, n_z, n_lm, b0, nb, most, plan_match_skip, "measurement");
}
inline MatchTable plan_match_table(const double *z, const double *R, const int *ids, int n_z, int nb, int zcap) {
    return plan_list_table(z, R, ids, n_z, nb, zcap, plan_match_skip);
}

// The iterations of ekf_update_matched_iter: 1 .. EKF_ITER_MAX factorisations per round, a step bound that is finite and not negative
// (0: every round runs to max_iter).
inline PlanStatus plan_iter_args(int max_iter, double tol) {
    if (max_iter < 1 || max_iter > EKF_ITER_MAX) return plan_fail(EKF_ERR_BAD_ARG, "max_iter = %d is not in 1 .. %d", max_iter, EKF_ITER_MAX);
    if (!(__builtin_isfinite(tol) && tol >= 0.0)) return plan_fail(EKF_ERR_BAD_ARG, "tol is not finite and not negative");
    return {};
}

// ---- absolute fixes (ekf_update_fixes, ekf_fix_compat) ----------------------------------------------------------------------------
// The lists of nb filters, filter k's n entries at z + k * n * 2, R + k * n * 4 and what + k * n; what[q] == EKF_FIX_SKIP: no
// entry (its z and R are not looked at).  Checked before the handle is touched: the pointers, n, every kind >= EKF_FIX_HEADING, the
// values a kind reads finite (EKF_FIX_HEADING: z[0] and R[0] alone, and R[0] not negative), and at most `limit` entries per filter
// (limit < 0: any number).
inline PlanStatus plan_fix_values(const double *z, const double *R, const int *what, int n, int b0, int nb, int limit) {
    if (n < 0) return plan_fail(EKF_ERR_BAD_ARG, "negative entry count");
    if (n > 0 && (!z || !R || !what)) return plan_fail(EKF_ERR_BAD_ARG, "a null list with n > 0");
    for (int k = 0; k < nb; k++) {
        int kept = 0;
        for (int q = 0; q < n; q++) {
            const size_t at = (size_t)k * n + q;
            const int w = what[at];
            if (w < EKF_FIX_HEADING)
                return plan_fail(EKF_ERR_BAD_ARG, "filter %d, entry %d: kind %d (a landmark, EKF_FIX_POSITION, EKF_FIX_HEADING or EKF_FIX_SKIP)", b0 + k, q, w);
            if (w == EKF_FIX_SKIP) continue;
            kept++;
            if (w == EKF_FIX_HEADING) {
                if (!__builtin_isfinite(z[2 * at]) || !__builtin_isfinite(R[4 * at])) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, entry %d: z or R is not finite", b0 + k, q);
                if (R[4 * at] < 0.0) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, entry %d: a negative heading variance", b0 + k, q);
            } else if (!plan_entry_finite(z, R, at)) {
                return plan_fail(EKF_ERR_BAD_ARG, "filter %d, entry %d: z or R is not finite", b0 + k, q);
            }
        }
        if (limit >= 0 && kept > limit) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: %d entries in one list (at most %d)", b0 + k, kept, limit);
    }
    return {};
}
// ... and the landmark entries against the landmark counts n_lm[k], once they are current.  *most = the most entries of a filter.
inline PlanStatus plan_fix_ids(const int *what, int n, const int *n_lm, int b0, int nb, int *most) {
    return plan_list_ids(what, n, n_lm, b0, nb, most, plan_fix_skip, "entry");
}
inline MatchTable plan_fix_table(const double *z, const double *R, const int *what, int n, int nb, int zcap) {
    return plan_list_table(z, R, what, n, nb, zcap, plan_fix_skip);
}

// ---- polar measurements (ekf_update_polar, ekf_polar_compat) ----------------------------------------------------------------------
// The lists of nb filters, filter k's n entries at ids + k * n and kind + k * n; ids[q] == -1: no entry (its kind is not looked at).
// The structural checks -- n, the two pointers, every id >= -1, the kind of every kept entry one of EKF_POLAR_* -- and the list the
// device takes: *packed [nb][n], -1 for a skipped entry, else the landmark with its kind above it (POLAR_KIND_SHIFT, ekf_device.h).
// An id that does not fit below the kind is no landmark of any handle: it is packed as POLAR_ID_MASK, which plan_polar_ids refuses
// under its own number.
inline int plan_polar_id(int packed) { return packed & POLAR_ID_MASK; }
inline int plan_polar_kind(int packed) { return packed >> POLAR_KIND_SHIFT; }
inline PlanStatus plan_polar_pack(const int *ids, const int *kind, int n, int b0, int nb, std::vector<int> *packed) {
    packed->clear();
    if (n < 0) return plan_fail(EKF_ERR_BAD_ARG, "negative entry count");
    if (n > 0 && (!ids || !kind)) return plan_fail(EKF_ERR_BAD_ARG, "a null list with n > 0");
    packed->assign((size_t)nb * n, -1);
    for (int k = 0; k < nb; k++)
        for (int q = 0; q < n; q++) {
            const size_t at = (size_t)k * n + q;
            if (ids[at] < -1) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, entry %d: id %d (a landmark, or -1 to skip)", b0 + k, q, ids[at]);
            if (ids[at] < 0) continue;
            if (kind[at] < EKF_POLAR_RANGE || kind[at] > EKF_POLAR_BOTH)
                return plan_fail(EKF_ERR_BAD_ARG, "filter %d, entry %d: kind %d (EKF_POLAR_RANGE, EKF_POLAR_BEARING or EKF_POLAR_BOTH)", b0 + k, q, kind[at]);
            (*packed)[at] = std::min(ids[at], POLAR_ID_MASK) | kind[at] << POLAR_KIND_SHIFT;
        }
    return {};
}
// The values of a packed list, z + k * n * 2 and R + k * n * 4: the pointers, the values a kind reads finite (RANGE: z[0] and R[0];
// BEARING: z[1] and R[3]; BOTH: all six), no negative variance of a one-component entry, and at most `limit` entries per filter
// (limit < 0: any number).  With plan_polar_pack: everything that is checked before the handle is touched.
inline PlanStatus plan_polar_values(const double *z, const double *R, const int *packed, int n, int b0, int nb, int limit) {
    if (n < 0) return plan_fail(EKF_ERR_BAD_ARG, "negative entry count");
    if (n > 0 && (!z || !R || !packed)) return plan_fail(EKF_ERR_BAD_ARG, "a null list with n > 0");
    for (int k = 0; k < nb; k++) {
        int kept = 0;
        for (int q = 0; q < n; q++) {
            const size_t at = (size_t)k * n + q;
            if (packed[at] < 0) continue;
            kept++;
            const int kd = plan_polar_kind(packed[at]);
            if (kd == EKF_POLAR_BOTH) {
                if (!plan_entry_finite(z, R, at)) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, entry %d: z or R is not finite", b0 + k, q);
                continue;
            }
            const int e = kd == EKF_POLAR_BEARING;  // the component read: z[e], R[3 e]
            if (!__builtin_isfinite(z[2 * at + e]) || !__builtin_isfinite(R[4 * at + 3 * e])) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, entry %d: z or R is not finite", b0 + k, q);
            if (R[4 * at + 3 * e] < 0.0) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, entry %d: a negative %s variance", b0 + k, q, e ? "bearing" : "range");
        }
        if (limit >= 0 && kept > limit) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: %d entries in one list (at most %d)", b0 + k, kept, limit);
    }
    return {};
}
// ... and the landmarks against the landmark counts n_lm[k], once they are current.  *most = the most entries of a filter.
inline PlanStatus plan_polar_ids(const int *packed, int n, const int *n_lm, int b0, int nb, int *most) {
    *most = 0;
    for (int k = 0; k < nb; k++) {
        int kept = 0;
        for (int q = 0; q < n; q++) {
            const int p = packed[(size_t)k * n + q];
            if (p < 0) continue;
            if (plan_polar_id(p) >= n_lm[k]) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, entry %d: landmark id %d is not one of its %d landmarks", b0 + k, q, plan_polar_id(p), n_lm[k]);
            kept++;
        }
        *most = std::max(*most, kept);
    }
    return {};
}
// The tables k_polar_factor reads, as plan_list_table builds them, idt the packed entries: the live component of a one-component
// entry in row 0 -- of a RANGE entry z[0] and R[0], of a BEARING entry z[1] and R[3] moved to z[0] and R[0] --, zeros behind it.
inline MatchTable plan_polar_table(const double *z, const double *R, const int *packed, int n, int nb, int zcap) {
    MatchTable t;
    t.zt.assign((size_t)nb * zcap * 2, 0.0), t.Rt.assign((size_t)nb * zcap * 4, 0.0);
    t.idt.assign((size_t)nb * zcap, 0), t.src.assign((size_t)nb * zcap, -1), t.cnt.assign((size_t)nb, 0);
    for (int k = 0; k < nb; k++)
        for (int q = 0; q < n; q++) {
            const size_t at = (size_t)k * n + q;
            if (packed[at] < 0 || t.cnt[k] >= zcap) continue;
            const size_t to = (size_t)k * zcap + t.cnt[k]++;
            const int kd = plan_polar_kind(packed[at]);
            if (kd == EKF_POLAR_BOTH) {
                for (int e = 0; e < 2; e++) t.zt[2 * to + e] = z[2 * at + e];
                for (int e = 0; e < 4; e++) t.Rt[4 * to + e] = R[4 * at + e];
            } else {
                const int e = kd == EKF_POLAR_BEARING;
                t.zt[2 * to] = z[2 * at + e], t.Rt[4 * to] = R[4 * at + 3 * e];
            }
            t.idt[to] = packed[at], t.src[to] = q;
        }
    return t;
}

// ---- individual compatibility (ekf_gate_candidates) -------------------------------------------------------------------------------
// The scans of nb filters, filter k's n_z measurements at z + k * n_z * 2 and R + k * n_z * 4, entry q looked at unless
// valid[k * n_z + q] == 0 (valid == nullptr: every entry).  Checked before the handle is touched: n_z, the pointers, the gate (not
// negative, not NaN; +inf lists every kept pair), the room for the list, z and R of every valid entry finite.
inline PlanStatus plan_gate_args(const double *z, const double *R, const unsigned char *valid, int n_z, int b0, int nb, double gate, const ekf_candidate *cand_out, int max_cand) {
    if (n_z < 0) return plan_fail(EKF_ERR_BAD_ARG, "negative measurement count");
    if (n_z > 0 && (!z || !R)) return plan_fail(EKF_ERR_BAD_ARG, "a null list with n_z > 0");
    if (!(gate >= 0.0)) return plan_fail(EKF_ERR_BAD_ARG, "the gate is negative or NaN");
    if (max_cand < 0 || (!cand_out && max_cand > 0)) return plan_fail(EKF_ERR_BAD_ARG, "bad candidate list or max_cand");
    for (int k = 0; k < nb; k++)
        for (int q = 0; q < n_z; q++) {
            const size_t at = (size_t)k * n_z + q;
            if (valid && !valid[at]) continue;
            if (!plan_entry_finite(z, R, at)) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, measurement %d: z or R is not finite", b0 + k, q);
        }
    return {};
}
// The most valid entries of a filter of the call.
inline int plan_gate_most(const unsigned char *valid, int n_z, int nb) {
    int most = 0;
    for (int k = 0; k < nb; k++) {
        int kept = 0;
        for (int q = 0; q < n_z; q++) kept += !valid || valid[(size_t)k * n_z + q];
        most = std::max(most, kept);
    }
    return most;
}
// The tables k_gate reads (GateScratch of the call's filters), nb lists of zcap entries with the masked entries left out:
// zt [nb][zcap][2], Rt [nb][zcap][4], cnt [nb]; src [nb][zcap] = the caller's index of each entry (increasing).
struct GateTable {
    std::vector<double> zt, Rt;
    std::vector<int> cnt, src;
};
inline GateTable plan_gate_table(const double *z, const double *R, const unsigned char *valid, int n_z, int nb, int zcap) {
    GateTable t;
    t.zt.assign((size_t)nb * zcap * 2, 0.0), t.Rt.assign((size_t)nb * zcap * 4, 0.0);
    t.src.assign((size_t)nb * zcap, -1), t.cnt.assign((size_t)nb, 0);
    for (int k = 0; k < nb; k++)
        for (int q = 0; q < n_z; q++) {
            const size_t at = (size_t)k * n_z + q;
            if ((valid && !valid[at]) || t.cnt[k] >= zcap) continue;
            const size_t to = (size_t)k * zcap + t.cnt[k]++;
            t.zt[2 * to] = z[2 * at], t.zt[2 * to + 1] = z[2 * at + 1];
            for (int e = 0; e < 4; e++) t.Rt[4 * to + e] = R[4 * at + e];
            t.src[to] = q;
        }
    return t;
}
// One filter's list as the device appended it (meas = the table's index; any order) into the order handed out: meas becomes the
// caller's index src[meas], then (meas, d2 ascending, landmark).  An entry whose meas is not one of the table's `cnt` stops it:
// false, the list untouched from there on.
inline bool plan_gate_sort(ekf_candidate *list, size_t count, const int *src, int cnt) {
    for (size_t q = 0; q < count; q++) {
        if (list[q].meas < 0 || list[q].meas >= cnt) return false;
        list[q].meas = src[list[q].meas];
    }
    std::sort(list, list + count, [](const ekf_candidate &a, const ekf_candidate &b) {
        if (a.meas != b.meas) return a.meas < b.meas;
        if (a.d2 != b.d2) return a.d2 < b.d2;
        return a.landmark < b.landmark;
    });
    return true;
}
// The device's per-entry results, near and skip [nb][zcap], back into the caller's [nb][n_z] arrays (either may be null): entry q of
// filter k to src; a masked entry gets an all-zero decision and no skip.
inline void plan_gate_scatter(const GateTable &t, int zcap, int n_z, int nb, const ekf_decision *near, const int *skip, ekf_decision *nearest_out, int *n_skipped_out) {
    const ekf_decision none = {0, 0, 0.0};
    for (size_t q = 0; q < (size_t)nb * (n_z > 0 ? n_z : 0); q++) {
        if (nearest_out) nearest_out[q] = none;
        if (n_skipped_out) n_skipped_out[q] = 0;
    }
    for (int k = 0; k < nb; k++)
        for (int q = 0; q < t.cnt[k]; q++) {
            const size_t from = (size_t)k * zcap + q, to = (size_t)k * n_z + t.src[from];
            if (nearest_out) nearest_out[to] = near[from];
            if (n_skipped_out) n_skipped_out[to] = skip[from];
        }
}

// ---- joint compatibility search (ekf_associate_joint) -----------------------------------------------------------------------------
// What plan_gate_args checks of the scan, then: ids_out, the branch limit and the node budget, the joint gates (null: the defaults),
// and at most `limit` (EKF_MAX_PENDING) valid entries per filter.  Checked before the handle is touched.
inline PlanStatus plan_assoc_args(const double *z, const double *R, const unsigned char *valid, int n_z, int b0, int nb, double gate, const double *joint_gate, int max_branch,
                                  long long max_nodes, const int *ids_out, int limit) {
    const PlanStatus st = plan_gate_args(z, R, valid, n_z, b0, nb, gate, nullptr, 0);
    if (st.code) return st;
    if (n_z > 0 && !ids_out) return plan_fail(EKF_ERR_BAD_ARG, "ids_out is null");
    if (max_branch < 1 || max_branch > EKF_ASSOC_MAX_BRANCH) return plan_fail(EKF_ERR_BAD_ARG, "max_branch = %d is outside [1, %d]", max_branch, EKF_ASSOC_MAX_BRANCH);
    if (max_nodes < 1 || max_nodes > EKF_ASSOC_MAX_NODES) return plan_fail(EKF_ERR_BAD_ARG, "max_nodes = %lld is outside [1, %d]", max_nodes, EKF_ASSOC_MAX_NODES);
    for (int q = 0; joint_gate && q < EKF_MAX_PENDING; q++)
        if (!(joint_gate[q] >= 0.0)) return plan_fail(EKF_ERR_BAD_ARG, "joint_gate[%d] is negative or NaN", q);
    for (int k = 0; k < nb; k++) {
        int kept = 0;
        for (int q = 0; q < n_z; q++) kept += !valid || valid[(size_t)k * n_z + q];
        if (kept > limit) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: %d valid measurements in one scan (at most %d)", b0 + k, kept, limit);
    }
    return {};
}
// The survival function of chi-square with 2 q degrees of freedom, exp(-x / 2) sum_{i < q} (x / 2)^i / i! (positive terms: no
// cancellation).
inline double plan_chi2_even_sf(double x, int q) {
    double term = 1.0, sum = 0.0;
    for (int i = 0; i < q; i++) sum += term, term = term * (0.5 * x) / (i + 1);
    return exp(-0.5 * x) * sum;
}
// out[q - 1] = the `confidence` quantile for q = 1 .. EKF_MAX_PENDING pairings: bisection of the survival function down to two
// neighbouring doubles.  false: confidence is not inside (0, 1).
inline bool plan_assoc_gates(double confidence, double *out) {
    if (!(confidence > 0.0 && confidence < 1.0)) return false;
    const double tail = 1.0 - confidence;
    for (int q = 1; q <= EKF_MAX_PENDING; q++) {
        double lo = 0.0, hi = 1.0;
        while (plan_chi2_even_sf(hi, q) > tail) hi *= 2.0;
        for (int it = 0; it < 200; it++) {
            const double mid = 0.5 * (lo + hi);
            if (!(mid > lo && mid < hi)) break;
            if (plan_chi2_even_sf(mid, q) > tail) lo = mid;
            else hi = mid;
        }
        out[q - 1] = hi;
    }
    return true;
}
// The candidate table k_assoc_search reads, nb filters: ncand [nb][32] and cand [nb][32][EKF_ASSOC_MAX_BRANCH] by the COMPACTED
// index of a measurement (its place among the filter's valid entries, as plan_gate_table counts them), from filter k's list in
// ekf_gate_candidates' order at lists + k * ld with found[k] entries (meas = the caller's index): the first max_branch of each
// measurement.  listed / dropped [nb]: the pairs of the list, those cut.  src [nb][32]: the caller's index of a compacted entry.
struct AssocTable {
    std::vector<int> ncand, cand, listed, dropped, src, cnt;
    bool any = false;  // some filter has a candidate
};
inline AssocTable plan_assoc_table(const ekf_candidate *lists, size_t ld, const int *found, const unsigned char *valid, int n_z, int nb, int max_branch) {
    AssocTable t;
    t.ncand.assign((size_t)nb * EKF_MAX_PENDING, 0), t.cand.assign((size_t)nb * EKF_MAX_PENDING * EKF_ASSOC_MAX_BRANCH, -1);
    t.listed.assign((size_t)nb, 0), t.dropped.assign((size_t)nb, 0), t.cnt.assign((size_t)nb, 0), t.src.assign((size_t)nb * EKF_MAX_PENDING, -1);
    std::vector<int> place((size_t)(n_z > 0 ? n_z : 0));
    for (int k = 0; k < nb; k++) {
        int kept = 0;
        for (int q = 0; q < n_z; q++) {
            const bool look = !valid || valid[(size_t)k * n_z + q];
            place[q] = look && kept < EKF_MAX_PENDING ? kept : -1;
            if (place[q] >= 0) t.src[(size_t)k * EKF_MAX_PENDING + kept++] = q;
        }
        t.cnt[k] = kept;
        for (int q = 0; q < found[k]; q++) {
            const ekf_candidate &c = lists[(size_t)k * ld + q];
            if (c.meas < 0 || c.meas >= n_z || place[c.meas] < 0) continue;
            t.listed[k]++;
            int &n = t.ncand[(size_t)k * EKF_MAX_PENDING + place[c.meas]];
            if (n >= max_branch) {
                t.dropped[k]++;
                continue;
            }
            t.cand[((size_t)k * EKF_MAX_PENDING + place[c.meas]) * EKF_ASSOC_MAX_BRANCH + n++] = c.landmark;
            t.any = true;
        }
    }
    return t;
}
// The device's results back into the caller's order: ids [nb][32] by compacted index to ids_out [nb][n_z] (-1 elsewhere), and the
// winner's running distances d2 (filter k's at d2 + k * ld_d2, one per PAIRED measurement in order) to d2_out (NaN elsewhere; may
// be null) -- what ekf_joint_compat returns for ids_out.  ids == nullptr: nothing was searched.
inline void plan_assoc_scatter(const AssocTable &t, const int *ids, const double *d2, size_t ld_d2, int n_z, int nb, int *ids_out, double *d2_out) {
    for (size_t q = 0; q < (size_t)nb * (n_z > 0 ? n_z : 0); q++) {
        ids_out[q] = -1;
        if (d2_out) d2_out[q] = __builtin_nan("");
    }
    for (int k = 0; ids && k < nb; k++) {
        int j = 0;
        for (int q = 0; q < t.cnt[k]; q++) {
            const int id = ids[(size_t)k * EKF_MAX_PENDING + q];
            if (id < 0) continue;
            const size_t to = (size_t)k * n_z + t.src[(size_t)k * EKF_MAX_PENDING + q];
            ids_out[to] = id;
            if (d2_out) d2_out[to] = d2[(size_t)k * ld_d2 + j];
            j++;
        }
    }
}

// ---- landmark initialisation (ekf_add_landmarks, the end of ekf_update_joint) -----------------------------------------------------
// The lists of nb filters, filter k's n_z measurements at z + k * n_z * 2 and R + k * n_z * 4, entry q added unless
// add[k * n_z + q] == 0 (add == nullptr: every entry).  Checked before the handle is touched: the filter (index, one of B, or -1: the
// batch form, which needs n_out), n_z, the pointers, z and R of every selected entry finite.
inline PlanStatus plan_add_args(const double *z, const double *R, const unsigned char *add, int n_z, int index, int B, const int *n_out) {
    if (index < -1 || index >= B) return plan_fail(EKF_ERR_BAD_ARG, "filter %d is not one of the handle's %d", index, B);
    if (index < 0 && !n_out) return plan_fail(EKF_ERR_BAD_ARG, "n_out is null");
    if (n_z < 0) return plan_fail(EKF_ERR_BAD_ARG, "negative measurement count");
    if (n_z > 0 && (!z || !R)) return plan_fail(EKF_ERR_BAD_ARG, "a null list with n_z > 0");
    const int b0 = index < 0 ? 0 : index, nb = index < 0 ? B : 1;
    for (int k = 0; k < nb; k++)
        for (int q = 0; q < n_z; q++) {
            const size_t at = (size_t)k * n_z + q;
            if (add && !add[at]) continue;
            if (!plan_entry_finite(z, R, at)) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, measurement %d: z or R is not finite", b0 + k, q);
        }
    return {};
}
// The entries a table holds for a longest list of `most` when the handle's holds `have`: the growth rule from 64.
inline int plan_add_zcap(int have, int most) { return plan_grown_cap(have, most, 64); }
// The table k_add_vec and k_add_tiles read (AddScratch::tab of the call's filters), ONE block so that one copy carries it: nb records
// of add_tab_stride(zcap) doubles (ekf_device.h), record k = {count, 0, then zcap entries {z_x, z_y, R00, R10, R01, R11}} with the
// entries that are not added left out; cnt [nb] = the counts again, src [nb][zcap] = the caller's index of each entry (increasing).
struct AddTable {
    std::vector<double> tab;
    std::vector<int> cnt, src;
};
inline AddTable plan_add_table(const double *z, const double *R, const unsigned char *add, int n_z, int nb, int zcap) {
    AddTable t;
    const size_t stride = add_tab_stride(zcap);
    t.tab.assign((size_t)nb * stride, 0.0), t.cnt.assign((size_t)nb, 0), t.src.assign((size_t)nb * zcap, -1);
    for (int k = 0; k < nb; k++) {
        for (int q = 0; q < n_z; q++) {
            const size_t at = (size_t)k * n_z + q;
            if ((add && !add[at]) || t.cnt[k] >= zcap) continue;
            double *e = t.tab.data() + (size_t)k * stride + 2 + 6 * (size_t)t.cnt[k];
            e[0] = z[2 * at], e[1] = z[2 * at + 1];
            for (int c = 0; c < 4; c++) e[2 + c] = R[4 * at + c];
            t.src[(size_t)k * zcap + t.cnt[k]++] = q;
        }
        t.tab[(size_t)k * stride] = (double)t.cnt[k];
    }
    return t;
}
// Room for every filter's additions (n_lm[k] landmarks now, cnt[k] more), or the join's refusal: one filter without room ends the call.
inline PlanStatus plan_add_room(const int *n_lm, const int *cnt, int b0, int nb, int Ncap, const char *verb) {
    for (int k = 0; k < nb; k++)
        if (n_lm[k] + cnt[k] > Ncap) return plan_no_room(b0 + k, n_lm[k], cnt[k], Ncap, verb);
    return {};
}
// What the caller gets back: ids_out [nb][n_z] (may be null) = the new landmark's number, n_lm[k] + its place among the added, -1
// for the others; n_new [nb] = the new counts.  *nt / *most = the most tiles (join_tile_count) / additions of a filter.
inline void plan_add_ids(const AddTable &t, const int *n_lm, int n_z, int nb, int zcap, int *ids_out, int *n_new, int *nt, int *most) {
    *nt = 0, *most = 0;
    for (size_t q = 0; ids_out && q < (size_t)nb * (n_z > 0 ? n_z : 0); q++) ids_out[q] = -1;
    for (int k = 0; k < nb; k++) {
        for (int q = 0; ids_out && q < t.cnt[k]; q++) ids_out[(size_t)k * n_z + t.src[(size_t)k * zcap + q]] = n_lm[k] + q;
        n_new[k] = n_lm[k] + t.cnt[k];
        *nt = std::max(*nt, join_tile_count(n_lm[k], t.cnt[k])), *most = std::max(*most, t.cnt[k]);
    }
}

// ---- the scan step (ekf_update_joint) ---------------------------------------------------------------------------------------------
// The kinds of a scan from the search's result: ids [nb][n_z] (ekf_associate_joint's ids_out) and near [nb][n_z] (its nearest_out).
// kind [nb][n_z]: a masked entry 0, a paired one EKF_DECISION_OLD, an unpaired one EKF_DECISION_NEW iff the filter's own gate says
// New at the entry state, else EKF_DECISION_IGNORE; is_new [nb][n_z] = the mask ekf_add_landmarks takes.
inline void plan_joint_kinds(const int *ids, const ekf_decision *near, const unsigned char *valid, int n_z, int nb, int *kind, unsigned char *is_new) {
    for (size_t at = 0; at < (size_t)nb * (n_z > 0 ? n_z : 0); at++) {
        is_new[at] = 0;
        if (valid && !valid[at]) kind[at] = 0;
        else if (ids[at] >= 0) kind[at] = EKF_DECISION_OLD;
        else if (near[at].decision == EKF_DECISION_NEW) kind[at] = EKF_DECISION_NEW, is_new[at] = 1;
        else kind[at] = EKF_DECISION_IGNORE;
    }
}
// ... and after the matched step: filter k applied its first applied[k] pairings; the later ones (a round that was not positive
// definite, and everything behind it) become EKF_DECISION_IGNORE with id -1.  Then the added landmarks' numbers (new_ids, -1: none).
inline void plan_joint_merge(const int *applied, const int *new_ids, int n_z, int nb, int *ids, int *kind) {
    for (int k = 0; k < nb; k++) {
        int paired = 0;
        for (int q = 0; q < n_z; q++) {
            const size_t at = (size_t)k * n_z + q;
            if (kind[at] == EKF_DECISION_OLD && paired++ >= applied[k]) kind[at] = EKF_DECISION_IGNORE, ids[at] = -1;
            if (kind[at] == EKF_DECISION_NEW) ids[at] = new_ids[at];
        }
    }
}

// ---- relocalisation (ekf_locate_scan, ekf_reset_pose, ekf_relocalize) -------------------------------------------------------------
// The scans of nb filters as for plan_gate_args, without R.  Checked before the handle is touched: n_z, the pointers, tol and
// min_sep finite and positive, max_base and max_out in range, z of every valid entry finite, at most `limit` (EKF_MAX_PENDING) valid
// entries per filter.
inline PlanStatus plan_locate_args(const double *z, const unsigned char *valid, int n_z, int b0, int nb, double tol, double min_sep, int max_base, int max_out,
                                   const ekf_locate_hyp *hyp_out, const int *ids_out, int limit) {
    if (n_z < 0) return plan_fail(EKF_ERR_BAD_ARG, "negative measurement count");
    if (n_z > 0 && !z) return plan_fail(EKF_ERR_BAD_ARG, "a null list with n_z > 0");
    if (!(__builtin_isfinite(tol) && tol > 0.0)) return plan_fail(EKF_ERR_BAD_ARG, "tol is not finite and positive");
    if (!(__builtin_isfinite(min_sep) && min_sep > 0.0)) return plan_fail(EKF_ERR_BAD_ARG, "min_sep is not finite and positive");
    if (max_base < 1 || max_base > EKF_LOCATE_MAX_BASE) return plan_fail(EKF_ERR_BAD_ARG, "max_base = %d is not in 1 .. %d", max_base, EKF_LOCATE_MAX_BASE);
    if (max_out < 1 || max_out > EKF_LOCATE_MAX_OUT) return plan_fail(EKF_ERR_BAD_ARG, "max_out = %d is not in 1 .. %d", max_out, EKF_LOCATE_MAX_OUT);
    if (!hyp_out || !ids_out) return plan_fail(EKF_ERR_BAD_ARG, "hyp_out or ids_out is null");
    for (int k = 0; k < nb; k++) {
        int kept = 0;
        for (int q = 0; q < n_z; q++) {
            const size_t at = (size_t)k * n_z + q;
            if (valid && !valid[at]) continue;
            if (!(__builtin_isfinite(z[2 * at]) && __builtin_isfinite(z[2 * at + 1]))) return plan_fail(EKF_ERR_BAD_ARG, "filter %d, measurement %d: z is not finite", b0 + k, q);
            kept++;
        }
        if (kept > limit) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: %d valid measurements, a search takes at most %d", b0 + k, kept, limit);
    }
    return {};
}
// The tables the search reads (LocScratch of the call's filters): zt [nb][32][2] the valid entries compacted, cnt [nb], src [nb][32]
// the caller's index of each (increasing); the base pairs base [nb][16][2] (compacted indices a < b) with their separations
// blen [nb][16] = sqrt(dx dx + dy dy), nbase [nb]: the pairs with a separation >= min_sep, by separation descending, then (a, b)
// ascending, the first max_base; reach [nb] = the largest |z_k| of a valid entry (0: none).
struct LocateTable {
    std::vector<double> zt, blen, reach;
    std::vector<int> cnt, src, base, nbase;
};
inline LocateTable plan_locate_table(const double *z, const unsigned char *valid, int n_z, int nb, double min_sep, int max_base) {
    const int cap = EKF_MAX_PENDING, bcap = EKF_LOCATE_MAX_BASE;
    LocateTable t;
    t.zt.assign((size_t)nb * cap * 2, 0.0), t.blen.assign((size_t)nb * bcap, 0.0), t.reach.assign((size_t)nb, 0.0);
    t.cnt.assign((size_t)nb, 0), t.src.assign((size_t)nb * cap, -1), t.base.assign((size_t)nb * bcap * 2, 0), t.nbase.assign((size_t)nb, 0);
    struct Pair {
        double len;
        int a, b;
    };
    for (int k = 0; k < nb; k++) {
        double *zk = t.zt.data() + (size_t)k * cap * 2;
        for (int q = 0; q < n_z; q++) {
            const size_t at = (size_t)k * n_z + q;
            if ((valid && !valid[at]) || t.cnt[k] >= cap) continue;
            const int to = t.cnt[k]++;
            zk[2 * to] = z[2 * at], zk[2 * to + 1] = z[2 * at + 1];
            t.src[(size_t)k * cap + to] = q;
            t.reach[k] = std::max(t.reach[k], sqrt(z[2 * at] * z[2 * at] + z[2 * at + 1] * z[2 * at + 1]));
        }
        std::vector<Pair> pairs;
        for (int a = 0; a < t.cnt[k]; a++)
            for (int b = a + 1; b < t.cnt[k]; b++) {
                const double dx = zk[2 * b] - zk[2 * a], dy = zk[2 * b + 1] - zk[2 * a + 1];
                const double len = sqrt(dx * dx + dy * dy);
                if (len >= min_sep) pairs.push_back({len, a, b});
            }
        std::stable_sort(pairs.begin(), pairs.end(), [](const Pair &p, const Pair &q) { return p.len > q.len; });  // (generated in (a, b) order)
        t.nbase[k] = std::min((int)pairs.size(), max_base);
        for (int r = 0; r < t.nbase[k]; r++) {
            t.base[((size_t)k * bcap + r) * 2] = pairs[r].a, t.base[((size_t)k * bcap + r) * 2 + 1] = pairs[r].b;
            t.blen[(size_t)k * bcap + r] = pairs[r].len;
        }
    }
    return t;
}
// Two fitted poses (x, y, heading) are the same pose: positions within 2 tol, headings (their difference wrapped into [-pi, pi])
// within 2 tol / reach; reach <= 0 (no measurement away from the robot): the heading says nothing.
inline bool plan_locate_same_pose(const double a[3], const double b[3], double tol, double reach) {
    const double dx = a[0] - b[0], dy = a[1] - b[1];
    if (!(sqrt(dx * dx + dy * dy) <= 2.0 * tol)) return false;
    if (!(reach > 0.0)) return true;
    const double dphi = remainder(a[2] - b[2], 2.0 * M_PI);
    return fabs(dphi) <= 2.0 * tol / reach;
}
// ekf_relocalize's acceptance over the `n` written hypotheses of a filter, best first: the best has at least min_inliers, and every
// other one that is not the same pose as the best has at most best - lead.
inline bool plan_locate_accept(const ekf_locate_hyp *hyps, int n, double tol, double reach, int min_inliers, int lead) {
    if (n < 1 || hyps[0].inliers < min_inliers) return false;
    for (int k = 1; k < n; k++)
        if (hyps[k].inliers > hyps[0].inliers - lead && !plan_locate_same_pose(hyps[k].pose, hyps[0].pose, tol, reach)) return false;
    return true;
}
// ekf_reset_pose's arguments of one filter: every entry finite, no negative diagonal entry of P_RR.  pose == nullptr: P_RR alone
// (ekf_relocalize, whose pose comes out of the search).
inline PlanStatus plan_reset_args(const double *pose, const double *prr, int filter) {
    if (!prr) return plan_fail(EKF_ERR_BAD_ARG, "a null P_RR");
    for (int i = 0; pose && i < 3; i++)
        if (!__builtin_isfinite(pose[i])) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: the pose is not finite", filter);
    for (int i = 0; i < 9; i++)
        if (!__builtin_isfinite(prr[i])) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: P_RR is not finite", filter);
    for (int i = 0; i < 3; i++)
        if (prr[4 * i] < 0.0) return plan_fail(EKF_ERR_BAD_ARG, "filter %d: P_RR[%d][%d] is negative", filter, i, i);
    return {};
}
// ... as the kernel takes them (ekf_rewrite.hip: ResetPose): the pose, P_RR symmetrised row-major (off-diagonals 0.5 * (a + b), as
// Update.cpp:193), apply (1.0, or 0.0: the filter is left alone).
inline void plan_reset_values(const double *pose, const double *prr, bool apply, double out[13]) {
    for (int i = 0; i < 3; i++) out[i] = pose[i];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[3 + 3 * i + j] = i == j ? prr[4 * i] : 0.5 * (prr[3 * i + j] + prr[3 * j + i]);
    out[12] = apply ? 1.0 : 0.0;
}
