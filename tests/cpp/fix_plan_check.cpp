// Host-only check of the absolute-fix part of ekf_map_plan.h (plan_fix_values, plan_fix_ids, plan_fix_table), called directly.
// 1. The refusals: n < 0, a null list with n > 0, a kind below EKF_FIX_HEADING, NaN / inf among the values a kind reads, a negative
//    variance of a heading entry, more entries than the limit, a landmark id equal to the landmark count -- each with its status and
//    text (written out here).  What is accepted: n = 0 with null lists, NaN in z and R of a skipped entry, NaN in z[1] and R[1..3]
//    of a heading entry, R = 0, position and heading entries on a filter without landmarks, the same thing several times.
// 2. The table: skipped entries left out, order kept, src naming the caller's index, of a heading entry z[0] and R[0] alone, for a
//    batch of three ragged lists.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../2d-ekf-slam_amd/csrc/ekf_map_plan.h"

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

int main() {
    const double nan = std::nan(""), inf = INFINITY;
    const int P = EKF_FIX_POSITION, H = EKF_FIX_HEADING, S = EKF_FIX_SKIP;
    CHECK(S == -1 && P == -2 && H == -3);
    // two filters, three entries each
    std::vector<double> z = {1, 2, 3, 4, 5, 6, /**/ 7, 8, 9, 10, 11, 12};
    std::vector<double> R(24, 0.5);
    std::vector<int> what = {P, S, 4, /**/ S, H, 9};
    ACCEPTED(plan_fix_values(z.data(), R.data(), what.data(), 3, 0, 2, -1));
    ACCEPTED(plan_fix_values(nullptr, nullptr, nullptr, 0, 0, 2, -1));
    REFUSED(plan_fix_values(z.data(), R.data(), what.data(), -1, 0, 2, -1), EKF_ERR_BAD_ARG, "negative entry count");
    REFUSED(plan_fix_values(nullptr, R.data(), what.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "a null list with n > 0");
    REFUSED(plan_fix_values(z.data(), nullptr, what.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "a null list with n > 0");
    REFUSED(plan_fix_values(z.data(), R.data(), nullptr, 3, 0, 2, -1), EKF_ERR_BAD_ARG, "a null list with n > 0");
    {
        std::vector<int> bad = what;
        bad[5] = -4;
        REFUSED(plan_fix_values(z.data(), R.data(), bad.data(), 3, 4, 2, -1), EKF_ERR_BAD_ARG,
                "filter 5, entry 2: kind -4 (a landmark, EKF_FIX_POSITION, EKF_FIX_HEADING or EKF_FIX_SKIP)");
    }
    {
        std::vector<double> zb = z, Rb = R;
        zb[2] = nan, Rb[4 * 3 + 1] = inf;  // entry 1 of filter 0 and entry 0 of filter 1: both skipped
        ACCEPTED(plan_fix_values(zb.data(), Rb.data(), what.data(), 3, 0, 2, -1));
        zb = z, Rb = R;
        zb[2 * 4 + 1] = nan, Rb[4 * 4 + 1] = nan, Rb[4 * 4 + 2] = inf, Rb[4 * 4 + 3] = -inf;  // the heading entry: what it does not read
        ACCEPTED(plan_fix_values(zb.data(), Rb.data(), what.data(), 3, 0, 2, -1));
        zb = z, zb[2 * 4] = nan;
        REFUSED(plan_fix_values(zb.data(), R.data(), what.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "filter 1, entry 1: z or R is not finite");
        Rb = R, Rb[4 * 4] = inf;
        REFUSED(plan_fix_values(z.data(), Rb.data(), what.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "filter 1, entry 1: z or R is not finite");
        Rb = R, Rb[4 * 4] = -1e-9;
        REFUSED(plan_fix_values(z.data(), Rb.data(), what.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "filter 1, entry 1: a negative heading variance");
        zb = z, zb[1] = inf;  // the position entry reads both values of z ...
        REFUSED(plan_fix_values(zb.data(), R.data(), what.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "filter 0, entry 0: z or R is not finite");
        Rb = R, Rb[2] = nan;  // ... and all of R
        REFUSED(plan_fix_values(z.data(), Rb.data(), what.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "filter 0, entry 0: z or R is not finite");
        Rb = R, Rb[4 * 2 + 3] = -inf;
        REFUSED(plan_fix_values(z.data(), Rb.data(), what.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "filter 0, entry 2: z or R is not finite");
        Rb.assign(24, 0.0);  // hard fixes
        ACCEPTED(plan_fix_values(z.data(), Rb.data(), what.data(), 3, 0, 2, -1));
    }
    ACCEPTED(plan_fix_values(z.data(), R.data(), what.data(), 3, 0, 2, 2));
    REFUSED(plan_fix_values(z.data(), R.data(), what.data(), 3, 0, 2, 1), EKF_ERR_BAD_ARG, "filter 0: 2 entries in one list (at most 1)");
    int most = -1;
    const int n_ok[] = {5, 10}, n_short[] = {5, 9}, n_none[] = {0, 0};
    ACCEPTED(plan_fix_ids(what.data(), 3, n_ok, 0, 2, &most));
    CHECK(most == 2);
    REFUSED(plan_fix_ids(what.data(), 3, n_short, 2, 2, &most), EKF_ERR_BAD_ARG, "filter 3, entry 2: landmark id 9 is not one of its 9 landmarks");
    REFUSED(plan_fix_ids(what.data(), 3, n_none, 0, 2, &most), EKF_ERR_BAD_ARG, "filter 0, entry 2: landmark id 4 is not one of its 0 landmarks");
    const int robot_only[] = {P, H, S, P};
    ACCEPTED(plan_fix_ids(robot_only, 4, n_none, 0, 1, &most));  // no landmark is needed for these
    CHECK(most == 3);
    const int skipped[] = {S, S, S};
    ACCEPTED(plan_fix_ids(skipped, 3, n_none, 0, 1, &most));
    CHECK(most == 0);

    // the table: three filters, lists {P, -, 4}, {-, H, 9}, {-, -, -}
    z.insert(z.end(), {13, 14, 15, 16, 17, 18});
    R.resize(36, 0.5);
    for (size_t q = 0; q < R.size(); q++) R[q] = 100.0 + (double)q;
    z[2 * 4 + 1] = nan, R[4 * 4 + 1] = nan, R[4 * 4 + 2] = nan, R[4 * 4 + 3] = nan;  // the heading entry's unread values
    what.insert(what.end(), {S, S, S});
    const int zcap = 4;
    const MatchTable t = plan_fix_table(z.data(), R.data(), what.data(), 3, 3, zcap);
    CHECK(t.cnt == (std::vector<int>{2, 2, 0}));
    CHECK(t.zt.size() == 3u * zcap * 2 && t.Rt.size() == 3u * zcap * 4 && t.idt.size() == 3u * zcap && t.src.size() == 3u * zcap);
    CHECK(t.idt[0] == P && t.idt[1] == 4 && t.src[0] == 0 && t.src[1] == 2 && t.src[2] == -1);
    CHECK(t.zt[0] == 1 && t.zt[1] == 2 && t.zt[2] == 5 && t.zt[3] == 6);
    CHECK(t.Rt[0] == 100.0 && t.Rt[3] == 103.0 && t.Rt[4] == 108.0 && t.Rt[7] == 111.0);
    CHECK(t.idt[zcap] == H && t.src[zcap] == 1 && t.zt[2 * zcap] == 9 && t.zt[2 * zcap + 1] == 0.0);
    CHECK(t.Rt[4 * zcap] == 116.0 && t.Rt[4 * zcap + 1] == 0.0 && t.Rt[4 * zcap + 2] == 0.0 && t.Rt[4 * zcap + 3] == 0.0);
    CHECK(t.idt[zcap + 1] == 9 && t.src[zcap + 1] == 2 && t.zt[2 * zcap + 2] == 11 && t.zt[2 * zcap + 3] == 12 && t.Rt[4 * zcap + 4] == 120.0);
    CHECK(t.src[2 * zcap] == -1);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("fix plan ok\n");
    return 0;
}
