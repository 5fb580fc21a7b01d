// Host-only check of the landmark-initialisation part of ekf_map_plan.h (plan_add_args, plan_add_zcap, plan_add_table, plan_add_room,
// plan_add_ids, plan_joint_kinds, plan_joint_merge) and of the tile list the add kernel walks (ekf_device.h: join_tile_ij,
// join_tile_count), called directly.
// 1. The refusals of ekf_add_landmarks: n_z < 0, a null z or R with n_z > 0, NaN / inf in z or R of a selected entry, a null n_out in
//    the batch form, an index out of range -- each with its status and text.  Accepted: n_z = 0 with null lists, NaN in an entry
//    that is not selected.
// 2. The table: one block, record k = {count, 0, entries of six doubles}, entries that are not added left out, order kept.
// 3. The room: N + m == capacity fits, N + m == capacity + 1 is the join's refusal, for the filter that lacks it.
// 4. ids_out and the new counts.
// 5. The tiles visited for (N, m) against a brute-force enumeration of "stored tile (I <= J) that holds a column >= 2 N of the new map".
// 6. The kinds of ekf_update_joint and the merge behind the matched step.
#include <cmath>
#include <cstdio>
#include <set>
#include <string>
#include <utility>
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
    // three filters, four entries each
    std::vector<double> z(24), R(48);
    for (int i = 0; i < 24; i++) z[i] = i + 1;
    for (int i = 0; i < 48; i++) R[i] = 100 + i;
    const std::vector<unsigned char> add = {0, 1, 1, 0, /**/ 0, 0, 0, 0, /**/ 1, 1, 1, 1};
    int n_out[3];
    // ---- 1. the refusals ----
    ACCEPTED(plan_add_args(z.data(), R.data(), add.data(), 4, -1, 3, n_out));
    ACCEPTED(plan_add_args(z.data(), R.data(), nullptr, 4, 2, 3, nullptr));
    ACCEPTED(plan_add_args(nullptr, nullptr, nullptr, 0, 0, 3, nullptr));
    REFUSED(plan_add_args(z.data(), R.data(), nullptr, -1, 0, 3, nullptr), EKF_ERR_BAD_ARG, "negative measurement count");
    REFUSED(plan_add_args(nullptr, R.data(), nullptr, 4, 0, 3, nullptr), EKF_ERR_BAD_ARG, "a null list with n_z > 0");
    REFUSED(plan_add_args(z.data(), nullptr, nullptr, 4, 0, 3, nullptr), EKF_ERR_BAD_ARG, "a null list with n_z > 0");
    REFUSED(plan_add_args(z.data(), R.data(), add.data(), 4, -1, 3, nullptr), EKF_ERR_BAD_ARG, "n_out is null");
    REFUSED(plan_add_args(z.data(), R.data(), nullptr, 4, 3, 3, nullptr), EKF_ERR_BAD_ARG, "filter 3 is not one of the handle's 3");
    REFUSED(plan_add_args(z.data(), R.data(), nullptr, 4, -2, 3, n_out), EKF_ERR_BAD_ARG, "filter -2 is not one of the handle's 3");
    {
        std::vector<double> zb = z, Rb = R;
        zb[0] = nan, Rb[7 * 4 + 2] = inf;  // filter 0 entry 0, filter 1 entry 3: neither selected
        ACCEPTED(plan_add_args(zb.data(), Rb.data(), add.data(), 4, -1, 3, n_out));
        REFUSED(plan_add_args(zb.data(), Rb.data(), nullptr, 4, -1, 3, n_out), EKF_ERR_BAD_ARG, "filter 0, measurement 0: z or R is not finite");
        zb = z, zb[2 * 2 + 1] = inf;  // filter 0 entry 2: selected
        REFUSED(plan_add_args(zb.data(), R.data(), add.data(), 4, -1, 3, n_out), EKF_ERR_BAD_ARG, "filter 0, measurement 2: z or R is not finite");
        Rb = R, Rb[(8 + 1) * 4 + 3] = nan;  // filter 2 entry 1
        REFUSED(plan_add_args(z.data(), Rb.data(), add.data(), 4, -1, 3, n_out), EKF_ERR_BAD_ARG, "filter 2, measurement 1: z or R is not finite");
        // the one-filter form reads its own list only: index 1 with the list of "filter 0"
        REFUSED(plan_add_args(zb.data(), R.data(), nullptr, 4, 1, 3, nullptr), EKF_ERR_BAD_ARG, "filter 1, measurement 2: z or R is not finite");
    }
    // ---- 2. the table ----
    CHECK(plan_add_zcap(0, 1) == 64 && plan_add_zcap(0, 64) == 64 && plan_add_zcap(0, 65) == 128 && plan_add_zcap(128, 3) == 128 && plan_add_zcap(64, 300) == 512);
    CHECK(add_tab_stride(64) == 388 && add_tab_stride(128) == 772 && add_tab_stride(1) == 8);  // >= 2 + 6 zcap, a multiple of 4
    {
        const int zcap = 64;
        const AddTable t = plan_add_table(z.data(), R.data(), add.data(), 4, 3, zcap);
        const size_t st = add_tab_stride(zcap);
        CHECK(t.tab.size() == 3 * st && t.cnt.size() == 3 && t.src.size() == 3 * (size_t)zcap);
        CHECK(t.cnt[0] == 2 && t.cnt[1] == 0 && t.cnt[2] == 4);
        for (int k = 0; k < 3; k++) CHECK(t.tab[k * st] == (double)t.cnt[k] && t.tab[k * st + 1] == 0.0);
        const int want_src[3][4] = {{1, 2, -1, -1}, {-1, -1, -1, -1}, {0, 1, 2, 3}};
        for (int k = 0; k < 3; k++)
            for (int q = 0; q < 4; q++) {
                CHECK(t.src[(size_t)k * zcap + q] == want_src[k][q]);
                const double *e = t.tab.data() + k * st + 2 + 6 * q;
                if (want_src[k][q] < 0) {
                    for (int c = 0; c < 6; c++) CHECK(e[c] == 0.0);
                    continue;
                }
                const size_t at = (size_t)k * 4 + want_src[k][q];
                CHECK(e[0] == z[2 * at] && e[1] == z[2 * at + 1]);
                for (int c = 0; c < 4; c++) CHECK(e[2 + c] == R[4 * at + c]);
            }
        const AddTable all = plan_add_table(z.data(), R.data(), nullptr, 4, 3, zcap);
        CHECK(all.cnt[0] == 4 && all.cnt[1] == 4 && all.cnt[2] == 4 && all.tab[st + 2] == z[8]);
        // ---- 4. ids_out and the counts ----
        const int n_lm[3] = {31, 5, 0};
        int ids[12], n_new[3], nt, most;
        plan_add_ids(t, n_lm, 4, 3, zcap, ids, n_new, &nt, &most);
        const int want_ids[12] = {-1, 31, 32, -1, -1, -1, -1, -1, 0, 1, 2, 3};
        for (int q = 0; q < 12; q++) CHECK(ids[q] == want_ids[q]);
        CHECK(n_new[0] == 33 && n_new[1] == 5 && n_new[2] == 4 && most == 4);
        CHECK(nt == join_tile_count(31, 2) && nt == 3);  // tile columns 0 and 1 of a two-tile map: (0,0), (0,1), (1,1)
        plan_add_ids(t, n_lm, 4, 3, zcap, nullptr, n_new, &nt, &most);  // (no ids wanted)
        // ---- 3. the room ----
        ACCEPTED(plan_add_room(n_lm, t.cnt.data(), 0, 3, 33, "add"));
        REFUSED(plan_add_room(n_lm, t.cnt.data(), 0, 3, 32, "add"), EKF_ERR_CAPACITY,
                "filter 0: 31 + 2 landmarks do not fit capacity_landmarks = 32 (ekf_reserve, then add again)");
        const int n2[3] = {1, 5, 29};
        REFUSED(plan_add_room(n2, t.cnt.data(), 4, 3, 32, "add"), EKF_ERR_CAPACITY,
                "filter 6: 29 + 4 landmarks do not fit capacity_landmarks = 32 (ekf_reserve, then add again)");
    }
    // ---- 5. the tiles ----
    const int cases[6][2] = {{0, 1}, {31, 1}, {31, 2}, {32, 1}, {33, 40}, {63, 66}};
    for (const auto &c : cases) {
        const int N = c[0], m = c[1], nT = lm_tiles(N + m);
        std::set<std::pair<int, int>> want, got;
        for (int I = 0; I < nT; I++)
            for (int J = I; J < nT; J++) {
                bool holds = false;
                for (int col = 64 * J; col < 64 * J + 64; col++) holds = holds || (col >= 2 * N && col < 2 * (N + m));
                if (holds) want.insert({I, J});
            }
        const int nt = join_tile_count(N, m);
        for (int t = 0; t < nt + 3; t++) {
            int I, J;
            const bool in = join_tile_ij(t, N >> 5, nT, &I, &J);
            CHECK(in == (t < nt));
            if (in) CHECK(I <= J && got.insert({I, J}).second);
        }
        CHECK(got == want);
        if (got != want) printf("(N, m) = (%d, %d): %zu tiles visited, %zu hold a new column\n", N, m, got.size(), want.size());
    }
    CHECK(join_tile_count(200, 0) == 0);
    // the add kernel's classifier against the join's, every pair of landmarks around the map's ends
    for (const auto &c : cases)
        for (int li = 0; li < c[0] + c[1] + 3; li++)
            for (int lj = 0; lj < c[0] + c[1] + 3; lj++)
                CHECK(join_where(c[0], c[1], li, lj) == join_source(c[0], c[1], 4, 128, 2 * li + 1, 2 * lj).where);
    // ---- 6. kinds and merge ----
    {
        const int n_z = 6;
        int ids[6] = {4, -1, -1, 7, -1, 2};
        const ekf_decision near[6] = {{EKF_DECISION_OLD, 11, 1.0}, {EKF_DECISION_NEW, 0, 999999999999.0}, {EKF_DECISION_IGNORE, 9, 20.0},
                                      {EKF_DECISION_OLD, 17, 2.0}, {EKF_DECISION_NEW, 5, 70.0},           {EKF_DECISION_OLD, 7, 0.5}};
        const unsigned char valid[6] = {1, 1, 1, 1, 0, 1};
        int kind[6];
        unsigned char is_new[6];
        plan_joint_kinds(ids, near, valid, n_z, 1, kind, is_new);
        const int want[6] = {EKF_DECISION_OLD, EKF_DECISION_NEW, EKF_DECISION_IGNORE, EKF_DECISION_OLD, 0, EKF_DECISION_OLD};
        for (int q = 0; q < 6; q++) CHECK(kind[q] == want[q] && is_new[q] == (q == 1));
        plan_joint_kinds(ids, near, nullptr, n_z, 1, kind, is_new);
        CHECK(kind[4] == EKF_DECISION_NEW && is_new[4] == 1);
        plan_joint_kinds(ids, near, valid, n_z, 1, kind, is_new);
        const int applied = 2, new_ids[6] = {-1, 10, -1, -1, -1, -1};
        plan_joint_merge(&applied, new_ids, n_z, 1, ids, kind);
        const int ids_after[6] = {4, 10, -1, 7, -1, -1};
        const int kind_after[6] = {EKF_DECISION_OLD, EKF_DECISION_NEW, EKF_DECISION_IGNORE, EKF_DECISION_OLD, 0, EKF_DECISION_IGNORE};
        for (int q = 0; q < 6; q++) CHECK(ids[q] == ids_after[q] && kind[q] == kind_after[q]);
    }
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("add plan ok\n");
    return 0;
}
