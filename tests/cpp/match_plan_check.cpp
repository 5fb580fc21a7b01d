// Host-only check of the matched-update part of ekf_map_plan.h (plan_match_values, plan_match_ids, plan_match_table), called
// directly.
// 1. The refusals: n_z < 0, a null list with n_z > 0, an id below -1, NaN / inf in z or R of a measurement, more measurements than
//    the limit, an id equal to the landmark count -- each with its status and text (written out here).  What is accepted: n_z = 0
//    with null lists, NaN in z and R of a skipped entry, an id that is the last landmark, the same landmark several times.
// 2. The table: skipped entries left out, order kept, src naming the caller's index, for a batch of three ragged lists.
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
    // two filters, three entries each
    std::vector<double> z = {1, 2, 3, 4, 5, 6, /**/ 7, 8, 9, 10, 11, 12};
    std::vector<double> R(24, 0.5);
    std::vector<int> ids = {4, -1, 4, /**/ -1, -1, 9};
    ACCEPTED(plan_match_values(z.data(), R.data(), ids.data(), 3, 0, 2, -1));
    ACCEPTED(plan_match_values(nullptr, nullptr, nullptr, 0, 0, 2, -1));
    REFUSED(plan_match_values(z.data(), R.data(), ids.data(), -1, 0, 2, -1), EKF_ERR_BAD_ARG, "negative measurement count");
    REFUSED(plan_match_values(nullptr, R.data(), ids.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "a null list with n_z > 0");
    REFUSED(plan_match_values(z.data(), nullptr, ids.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "a null list with n_z > 0");
    REFUSED(plan_match_values(z.data(), R.data(), nullptr, 3, 0, 2, -1), EKF_ERR_BAD_ARG, "a null list with n_z > 0");
    {
        std::vector<int> bad = ids;
        bad[5] = -2;
        REFUSED(plan_match_values(z.data(), R.data(), bad.data(), 3, 4, 2, -1), EKF_ERR_BAD_ARG, "filter 5, measurement 2: id -2 (a landmark, or -1 to skip)");
    }
    {
        std::vector<double> zb = z, Rb = R;
        zb[2] = nan, Rb[4 * 4 + 1] = inf;  // entries 1 of filter 0 and 1 of filter 1: both skipped
        ACCEPTED(plan_match_values(zb.data(), Rb.data(), ids.data(), 3, 0, 2, -1));
        zb = z, zb[2 * 5 + 1] = nan;
        REFUSED(plan_match_values(zb.data(), R.data(), ids.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "filter 1, measurement 2: z or R is not finite");
        Rb = R, Rb[4 * 2 + 3] = -inf;
        REFUSED(plan_match_values(z.data(), Rb.data(), ids.data(), 3, 0, 2, -1), EKF_ERR_BAD_ARG, "filter 0, measurement 2: z or R is not finite");
    }
    ACCEPTED(plan_match_values(z.data(), R.data(), ids.data(), 3, 0, 2, 2));
    REFUSED(plan_match_values(z.data(), R.data(), ids.data(), 3, 0, 2, 1), EKF_ERR_BAD_ARG, "filter 0: 2 measurements in one hypothesis (at most 1)");
    int most = -1;
    const int n_ok[] = {5, 10}, n_short[] = {5, 9}, n_none[] = {0, 0};
    ACCEPTED(plan_match_ids(ids.data(), 3, n_ok, 0, 2, &most));
    CHECK(most == 2);
    REFUSED(plan_match_ids(ids.data(), 3, n_short, 2, 2, &most), EKF_ERR_BAD_ARG, "filter 3, measurement 2: landmark id 9 is not one of its 9 landmarks");
    REFUSED(plan_match_ids(ids.data(), 3, n_none, 0, 2, &most), EKF_ERR_BAD_ARG, "filter 0, measurement 0: landmark id 4 is not one of its 0 landmarks");
    const int skipped[] = {-1, -1, -1};
    ACCEPTED(plan_match_ids(skipped, 3, n_none, 0, 1, &most));
    CHECK(most == 0);

    // the table: three filters, lists {4, -, 4}, {-, -, 9}, {-, -, -}
    z.insert(z.end(), {13, 14, 15, 16, 17, 18});
    R.resize(36, 0.5);
    for (size_t q = 0; q < R.size(); q++) R[q] = 100.0 + (double)q;
    ids.insert(ids.end(), {-1, -1, -1});
    const int zcap = 4;
    const MatchTable t = plan_match_table(z.data(), R.data(), ids.data(), 3, 3, zcap);
    CHECK(t.cnt == (std::vector<int>{2, 1, 0}));
    CHECK(t.zt.size() == 3u * zcap * 2 && t.Rt.size() == 3u * zcap * 4 && t.idt.size() == 3u * zcap && t.src.size() == 3u * zcap);
    CHECK(t.idt[0] == 4 && t.idt[1] == 4 && t.src[0] == 0 && t.src[1] == 2 && t.src[2] == -1);
    CHECK(t.zt[0] == 1 && t.zt[1] == 2 && t.zt[2] == 5 && t.zt[3] == 6);
    CHECK(t.Rt[0] == 100.0 && t.Rt[3] == 103.0 && t.Rt[4] == 108.0 && t.Rt[7] == 111.0);
    CHECK(t.idt[zcap] == 9 && t.src[zcap] == 2 && t.zt[2 * zcap] == 11 && t.zt[2 * zcap + 1] == 12 && t.Rt[4 * zcap] == 120.0);
    CHECK(t.src[2 * zcap] == -1);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("match plan ok\n");
    return 0;
}
