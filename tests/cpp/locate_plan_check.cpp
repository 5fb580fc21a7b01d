// Host-only check of the relocalisation part of ekf_map_plan.h (plan_locate_args, plan_locate_table, plan_locate_same_pose,
// plan_locate_accept, plan_reset_args, plan_reset_values), called directly.
// 1. The refusals of the search: n_z < 0, a null list, tol / min_sep not finite and positive, max_base / max_out out of range, null
//    outputs, NaN / inf in z of a valid entry, more than 32 valid entries -- each with its status and text.  What is accepted: n_z = 0
//    with a null list, NaN in a masked entry, 33 entries of which 32 are valid.
// 2. The table: masked entries left out, src naming the caller's index, reach; the base pairs by separation descending, equal
//    separations by (a, b), the cut at max_base, pairs below min_sep left out, a filter without a pair.
// 3. The same-pose rule: the position bound, the heading bound and its wrap at +-pi, reach 0.
// 4. The acceptance rule: min_inliers, the lead over a different pose, repeats of the best pose ignored, an empty list.
// 5. The reset's checks and values: non-finite entries, a negative diagonal, zeros accepted, off-diagonals averaged.
// 6. The search's kept scratch (ekf_map_scratch.h: carve_loc, carve_loc_list): the size a carve without a base reports is what the
//    carve on an allocation uses, every array naturally aligned, in order and without overlap.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../2d-ekf-slam_amd/csrc/ekf_map_plan.h"
#include "../../2d-ekf-slam_amd/csrc/ekf_map_scratch.h"

static int failures = 0;
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("line %d: %s does not hold\n", __LINE__, #cond); \
            failures++;                                             \
        }                                                           \
    } while (0)

static void refused(const PlanStatus &st, int code, const char *text, int line) {
    if (st.code != code || st.text != text) {
        printf("line %d: got (%d, \"%s\"), want (%d, \"%s\")\n", line, st.code, st.text.c_str(), code, text);
        failures++;
    }
}
#define REFUSED(st, code, text) refused(st, code, text, __LINE__)
#define ACCEPTED(st) refused(st, EKF_OK, "", __LINE__)

static ekf_locate_hyp hyp(double x, double y, double phi, int inliers) {
    ekf_locate_hyp h = {};
    h.pose[0] = x, h.pose[1] = y, h.pose[2] = phi, h.inliers = inliers;
    return h;
}

int main() {
    const double nan = std::nan(""), inf = INFINITY;
    static_assert(sizeof(ekf_locate_hyp) == 88 && sizeof(ekf_locate_hyp) % 8 == 0, "the record's size");
    // ---- 1. refusals ----
    std::vector<double> z = {0.0, 0.0, 3.0, 0.0, 0.0, 4.0, 1.0, 1.0, /* filter 1 */ 5.0, 5.0, 5.5, 5.0, 9.0, 9.0, 5.0, 5.2};
    ekf_locate_hyp room[4];
    int ids[16];
    ACCEPTED(plan_locate_args(z.data(), nullptr, 4, 0, 2, 0.1, 1.0, 4, 4, room, ids, 32));
    ACCEPTED(plan_locate_args(nullptr, nullptr, 0, 0, 2, 0.1, 1.0, 4, 4, room, ids, 32));
    REFUSED(plan_locate_args(z.data(), nullptr, -1, 0, 2, 0.1, 1.0, 4, 4, room, ids, 32), EKF_ERR_BAD_ARG, "negative measurement count");
    REFUSED(plan_locate_args(nullptr, nullptr, 4, 0, 2, 0.1, 1.0, 4, 4, room, ids, 32), EKF_ERR_BAD_ARG, "a null list with n_z > 0");
    for (double bad : {0.0, -0.1, nan, inf}) {
        REFUSED(plan_locate_args(z.data(), nullptr, 4, 0, 2, bad, 1.0, 4, 4, room, ids, 32), EKF_ERR_BAD_ARG, "tol is not finite and positive");
        REFUSED(plan_locate_args(z.data(), nullptr, 4, 0, 2, 0.1, bad, 4, 4, room, ids, 32), EKF_ERR_BAD_ARG, "min_sep is not finite and positive");
    }
    REFUSED(plan_locate_args(z.data(), nullptr, 4, 0, 2, 0.1, 1.0, 0, 4, room, ids, 32), EKF_ERR_BAD_ARG, "max_base = 0 is not in 1 .. 16");
    REFUSED(plan_locate_args(z.data(), nullptr, 4, 0, 2, 0.1, 1.0, 17, 4, room, ids, 32), EKF_ERR_BAD_ARG, "max_base = 17 is not in 1 .. 16");
    REFUSED(plan_locate_args(z.data(), nullptr, 4, 0, 2, 0.1, 1.0, 16, 0, room, ids, 32), EKF_ERR_BAD_ARG, "max_out = 0 is not in 1 .. 64");
    REFUSED(plan_locate_args(z.data(), nullptr, 4, 0, 2, 0.1, 1.0, 16, 65, room, ids, 32), EKF_ERR_BAD_ARG, "max_out = 65 is not in 1 .. 64");
    REFUSED(plan_locate_args(z.data(), nullptr, 4, 0, 2, 0.1, 1.0, 4, 4, nullptr, ids, 32), EKF_ERR_BAD_ARG, "hyp_out or ids_out is null");
    REFUSED(plan_locate_args(z.data(), nullptr, 4, 0, 2, 0.1, 1.0, 4, 4, room, nullptr, 32), EKF_ERR_BAD_ARG, "hyp_out or ids_out is null");
    std::vector<double> zn = z;
    zn[2 * 5 + 1] = nan;  // filter 1, measurement 1
    REFUSED(plan_locate_args(zn.data(), nullptr, 4, 3, 2, 0.1, 1.0, 4, 4, room, ids, 32), EKF_ERR_BAD_ARG, "filter 4, measurement 1: z is not finite");
    zn[2 * 5 + 1] = inf;
    REFUSED(plan_locate_args(zn.data(), nullptr, 4, 0, 2, 0.1, 1.0, 4, 4, room, ids, 32), EKF_ERR_BAD_ARG, "filter 1, measurement 1: z is not finite");
    const unsigned char mask[8] = {1, 1, 1, 1, 1, 0, 1, 1};
    ACCEPTED(plan_locate_args(zn.data(), mask, 4, 0, 2, 0.1, 1.0, 4, 4, room, ids, 32));  // a masked entry is not looked at
    std::vector<double> z33(66, 1.0);
    std::vector<unsigned char> v33(33, 1);
    REFUSED(plan_locate_args(z33.data(), nullptr, 33, 2, 1, 0.1, 1.0, 4, 4, room, ids, 32), EKF_ERR_BAD_ARG, "filter 2: 33 valid measurements, a search takes at most 32");
    v33[7] = 0;
    ACCEPTED(plan_locate_args(z33.data(), v33.data(), 33, 2, 1, 0.1, 1.0, 4, 4, room, ids, 32));

    // ---- 2. the table ----
    {
        // filter 0: (0,0) (3,0) (0,4) (1,1): separations 01 = 3, 02 = 4, 12 = 5, 03 = sqrt 2, 13 = sqrt 5, 23 = sqrt 10
        const LocateTable t = plan_locate_table(z.data(), nullptr, 4, 2, 1.5, 4);
        CHECK(t.cnt[0] == 4 && t.cnt[1] == 4 && t.nbase[0] == 4);
        const int want[4][2] = {{1, 2}, {0, 2}, {2, 3}, {0, 1}};
        const double len[4] = {5.0, 4.0, sqrt(10.0), 3.0};
        for (int r = 0; r < 4; r++) CHECK(t.base[2 * r] == want[r][0] && t.base[2 * r + 1] == want[r][1] && t.blen[r] == len[r]);
        CHECK(t.reach[0] == 4.0 && t.src[0] == 0 && t.src[3] == 3 && t.src[4] == -1);
        // filter 1: (5,5) (5.5,5) (9,9) (5,5.2): above 1.5 only the three pairs with entry 2
        CHECK(t.nbase[1] == 3 && t.base[(16 + 0) * 2] == 0 && t.base[(16 + 0) * 2 + 1] == 2);
        CHECK(t.base[(16 + 1) * 2] == 2 && t.base[(16 + 1) * 2 + 1] == 3 && t.base[(16 + 2) * 2] == 1 && t.base[(16 + 2) * 2 + 1] == 2);
        CHECK(t.blen[16] > t.blen[17] && t.blen[17] > t.blen[18] && t.zt[64 + 4] == 9.0);
        const LocateTable all = plan_locate_table(z.data(), nullptr, 4, 1, 1.0, 16);
        CHECK(all.nbase[0] == 6 && all.base[2 * 4] == 1 && all.base[2 * 4 + 1] == 3 && all.base[2 * 5] == 0 && all.base[2 * 5 + 1] == 3);
        const LocateTable one = plan_locate_table(z.data(), nullptr, 4, 1, 1.0, 1);
        CHECK(one.nbase[0] == 1 && one.base[0] == 1 && one.base[1] == 2);
        const LocateTable none = plan_locate_table(z.data(), nullptr, 4, 1, 5.5, 4);
        CHECK(none.nbase[0] == 0);
        // equal separations go by (a, b): a square of side 2 -- the diagonals 03 and 12 first, then 01, 02, 13, 23
        const double sq[8] = {0, 0, 2, 0, 0, 2, 2, 2};
        const LocateTable e = plan_locate_table(sq, nullptr, 4, 1, 1.0, 16);
        const int eq[6][2] = {{0, 3}, {1, 2}, {0, 1}, {0, 2}, {1, 3}, {2, 3}};
        CHECK(e.nbase[0] == 6);
        for (int r = 0; r < 6; r++) CHECK(e.base[2 * r] == eq[r][0] && e.base[2 * r + 1] == eq[r][1]);
        // a mask: entries 0 and 2 of filter 0 only; the pair is (compacted) (0, 1), src names 0 and 2
        const unsigned char m[4] = {1, 0, 1, 0};
        const LocateTable k = plan_locate_table(z.data(), m, 4, 1, 1.0, 4);
        CHECK(k.cnt[0] == 2 && k.src[0] == 0 && k.src[1] == 2 && k.nbase[0] == 1 && k.base[0] == 0 && k.base[1] == 1 && k.blen[0] == 4.0 && k.reach[0] == 4.0);
        const LocateTable empty = plan_locate_table(nullptr, nullptr, 0, 2, 1.0, 4);
        CHECK(empty.cnt[1] == 0 && empty.nbase[1] == 0 && empty.reach[1] == 0.0);
    }

    // ---- 3. the same pose ----
    {
        const double a[3] = {1.0, 2.0, 0.5};
        const double near[3] = {1.11, 2.15, 0.5 + 0.039}, far_xy[3] = {1.13, 2.17, 0.5}, far_phi[3] = {1.0, 2.0, 0.5 + 0.041};
        CHECK(plan_locate_same_pose(a, near, 0.1, 5.0));      // 0.186 of 0.2 in position, 0.039 of 0.04 in heading
        CHECK(!plan_locate_same_pose(a, far_xy, 0.1, 5.0));
        CHECK(!plan_locate_same_pose(a, far_phi, 0.1, 5.0));
        CHECK(plan_locate_same_pose(a, far_phi, 0.1, 0.0));   // no reach: the heading says nothing
        const double p[3] = {0.0, 0.0, 3.14}, q[3] = {0.0, 0.0, -3.14}, w[3] = {0.0, 0.0, 3.14 + 4.0 * M_PI};
        CHECK(plan_locate_same_pose(p, q, 0.1, 5.0) && plan_locate_same_pose(q, p, 0.1, 5.0));  // 0.0032 apart across the wrap
        CHECK(plan_locate_same_pose(p, w, 0.1, 5.0));
    }

    // ---- 4. acceptance ----
    {
        std::vector<ekf_locate_hyp> h = {hyp(0, 0, 0, 10), hyp(0.05, 0.0, 0.01, 10), hyp(5, 5, 1, 6), hyp(0.01, 0.01, 0.0, 9), hyp(7, 1, 2, 8)};
        CHECK(plan_locate_accept(h.data(), 3, 0.1, 5.0, 6, 4));    // the repeat of the best is no rival; 6 <= 10 - 4
        CHECK(!plan_locate_accept(h.data(), 3, 0.1, 5.0, 6, 5));   // 6 > 10 - 5
        CHECK(!plan_locate_accept(h.data(), 3, 0.1, 5.0, 11, 0));  // min_inliers
        CHECK(plan_locate_accept(h.data(), 4, 0.1, 5.0, 6, 4));    // 9 inliers at the same pose
        CHECK(!plan_locate_accept(h.data(), 5, 0.1, 5.0, 6, 4));   // a rival of 8 behind it
        CHECK(plan_locate_accept(h.data(), 5, 0.1, 5.0, 6, 2));
        CHECK(plan_locate_accept(h.data(), 1, 0.1, 5.0, 10, 0) && !plan_locate_accept(h.data(), 0, 0.1, 5.0, 2, 0));
        CHECK(plan_locate_accept(h.data(), 2, 0.01, 5.0, 6, 0));  // lead 0: an equal rival at another pose is tolerated (10 <= 10)
        CHECK(!plan_locate_accept(h.data(), 2, 0.01, 5.0, 6, 1));           // ... a lead of 1 is not held
    }

    // ---- 5. the reset ----
    {
        const double pose[3] = {1.0, -2.0, 0.3};
        double prr[9] = {4.0, 1.0, 0.5, 3.0, 9.0, -1.0, 0.25, -2.0, 0.0};
        ACCEPTED(plan_reset_args(pose, prr, 0));
        ACCEPTED(plan_reset_args(nullptr, prr, 0));
        const double zeros[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        ACCEPTED(plan_reset_args(pose, zeros, 0));
        REFUSED(plan_reset_args(pose, nullptr, 0), EKF_ERR_BAD_ARG, "a null P_RR");
        double out[13];
        plan_reset_values(pose, prr, true, out);
        const double want[13] = {1.0, -2.0, 0.3, 4.0, 2.0, 0.375, 2.0, 9.0, -1.5, 0.375, -1.5, 0.0, 1.0};
        for (int k = 0; k < 13; k++) CHECK(out[k] == want[k]);
        plan_reset_values(pose, prr, false, out);
        CHECK(out[12] == 0.0);
        const double bad_pose[3] = {1.0, nan, 0.0};
        REFUSED(plan_reset_args(bad_pose, prr, 3), EKF_ERR_BAD_ARG, "filter 3: the pose is not finite");
        prr[5] = inf;
        REFUSED(plan_reset_args(pose, prr, 1), EKF_ERR_BAD_ARG, "filter 1: P_RR is not finite");
        prr[5] = -1.0, prr[4] = -1e-300;
        REFUSED(plan_reset_args(pose, prr, 2), EKF_ERR_BAD_ARG, "filter 2: P_RR[1][1] is negative");
    }

    // ---- 6. the scratch ----
    for (size_t B : {(size_t)1, (size_t)3}) {
        const ScratchGeom g = {B, 320, 643, 644, 320, 1000};
        LocScratch probe = {}, ls = {};
        Carver size{nullptr};
        carve_loc(probe, size, g);
        std::vector<char> mem(size.bytes() + 16);
        char *base = mem.data() + (16 - (size_t)mem.data() % 16) % 16;
        Carver at{base};
        carve_loc(ls, at, g);
        CHECK(at.bytes() == size.bytes() && probe.z == nullptr);
        const size_t sel = B * EKF_LOCATE_MAX_OUT, part = sel * LOC_PICK_PARTS;
        const std::vector<std::pair<const void *, size_t>> arrays = {
            {ls.z, B * 64 * 8}, {ls.blen, B * 16 * 8}, {ls.pssr, part * 8}, {ls.wssr, sel * 8}, {ls.hyp, sel * sizeof(ekf_locate_hyp)}, {ls.cnt, B * 8},
            {ls.pkey, part * 4}, {ls.wkey, sel * 4}, {ls.pinl, part * 4}, {ls.winl, sel * 4}, {ls.ids, sel * 32 * 4}, {ls.nz, B * 4}, {ls.nbase, B * 4}, {ls.base, B * 32 * 4}};
        const char *end = base;
        for (size_t k = 0; k < arrays.size(); k++) {
            const char *p = (const char *)arrays[k].first;
            CHECK(p >= end && (size_t)p % (k < 6 ? 8 : 4) == 0);
            end = p + arrays[k].second;
        }
        CHECK(end == base + size.bytes());
        Carver lsize{nullptr}, lat{base};
        carve_loc_list(probe, lsize, g, 4096);
        carve_loc_list(ls, lat, g, 4096);
        CHECK(lsize.bytes() == B * 4096 * 16 && lat.bytes() == lsize.bytes() && ls.ccap == 4096);
        CHECK((const char *)ls.key == (const char *)ls.ssr + B * 4096 * 8 && (const char *)ls.inl == (const char *)ls.key + B * 4096 * 4);
    }
    CHECK(plan_grown_cap(0, 15192, LOC_LIST_FLOOR) == 16384 && plan_grown_cap(0, 4096, LOC_LIST_FLOOR) == 4096);

    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("locate plan ok\n");
    return 0;
}
